// contrasts_file.hpp -- the file of `mmseq -contrasts FILE`: one contrast per line,
//     name<TAB>id,id,...<TAB>id,id,...
// (numerator and denominator; transcript ids as in the hits file header).  '#' lines and blank lines are skipped.  Plain host code:
// parsed before any device work, and compiled into the sanitizer build of the host tools (make asan).
#pragma once
#include <cstdint>
#include <fstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

struct ContrastsFile {
    std::vector<std::string> names;
    std::vector<std::vector<uint32_t>> num, den;   // header indices of the members, in file order
    size_t size() const { return names.size(); }
};

// the fields of `text` between separators, empty ones kept
inline std::vector<std::string> contrast_fields(const std::string &text, char sep)
{
    std::vector<std::string> out(1);
    for (char ch : text) {
        if (ch == sep) out.emplace_back();
        else out.back() += ch;
    }
    return out;
}

// false with `error` = "FILE:LINE: cause" (or "cannot open FILE" / "FILE: no contrasts") on the first fault; header_index: id -> header index
inline bool read_contrasts_file(const std::string &path, const std::unordered_map<std::string, uint32_t> &header_index, ContrastsFile &out,
                                std::string &error)
{
    std::ifstream ifs(path.c_str());
    if (!ifs.good()) { error = "cannot open contrasts file " + path; return false; }
    std::unordered_set<std::string> seen_names;
    std::string line;
    for (size_t lineno = 1; std::getline(ifs, line); ++lineno) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        auto fault = [&](const std::string &cause) { error = path + ":" + std::to_string(lineno) + ": " + cause; return false; };
        const std::vector<std::string> f = contrast_fields(line, '\t');
        if (f.size() != 3) return fault("expected 3 tab-separated fields (name, numerator ids, denominator ids), found " + std::to_string(f.size()));
        if (f[0].empty()) return fault("empty contrast name");
        if (!seen_names.insert(f[0]).second) return fault("duplicate contrast name '" + f[0] + "'");
        std::vector<uint32_t> side[2];
        const char *what[2] = {"numerator", "denominator"};
        for (int k = 0; k < 2; ++k) {
            if (f[1 + k].empty()) return fault(std::string("empty ") + what[k]);
            std::unordered_set<uint32_t> members;
            for (const std::string &id : contrast_fields(f[1 + k], ',')) {
                const auto it = header_index.find(id);
                if (it == header_index.end()) return fault("unknown transcript id '" + id + "' in the " + what[k]);
                if (!members.insert(it->second).second) return fault("transcript '" + id + "' twice in the " + what[k]);
                side[k].push_back(it->second);
            }
        }
        out.names.push_back(f[0]);
        out.num.push_back(std::move(side[0]));
        out.den.push_back(std::move(side[1]));
    }
    if (out.size() == 0) { error = path + ": no contrasts"; return false; }
    return true;
}
