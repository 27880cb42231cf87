// trace_io.hpp -- what the host programs that read a sample's posterior share (mmcollapse, mmfold): the tab-separated .mmseq tables
// and the gzip trace files mmseq writes (a header line of ids, then one line of values per kept sample).
#pragma once
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

namespace traceio {

inline std::vector<std::string> tokenise(const std::string &str, const std::string &delim)
{
    std::vector<std::string> out;
    std::string::size_type last = str.find_first_not_of(delim, 0), pos = str.find_first_of(delim, last);
    while (pos != std::string::npos || last != std::string::npos) {
        out.push_back(str.substr(last, pos - last));
        last = str.find_first_not_of(delim, pos);
        pos = str.find_first_of(delim, last);
    }
    return out;
}

inline bool readable(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fclose(f);
    return true;
}

inline int find_col(const std::vector<std::string> &hdr, const char *name)
{
    for (size_t i = 0; i < hdr.size(); ++i) if (hdr[i] == name) return (int)i;
    return -1;
}

inline double num(const std::string &s) { return atof(s.c_str()); }

// One .mmseq table: open() reads the '#' lines (kept in `comments`) and the header line; row() the lines below it, until the end of
// the file or an empty line.
struct TableReader {
    enum { OK = 0, CANNOT_OPEN = 1, TRUNCATED = 2 };
    std::ifstream ifs;
    std::vector<std::string> comments, hdr;
    std::string line;   // the row last read, as it stands in the file
    int open(const std::string &path)
    {
        ifs.open(path.c_str());
        if (!ifs.good()) return CANNOT_OPEN;
        getline(ifs, line);
        while (ifs.good() && !line.empty() && line[0] == '#') { comments.push_back(line); getline(ifs, line); }
        if (!ifs.good()) return TRUNCATED;
        hdr = tokenise(line, "\t");
        return OK;
    }
    bool row(std::vector<std::string> &t)
    {
        if (!getline(ifs, line)) return false;
        t = tokenise(line, "\t");
        return !t.empty();
    }
};

// whitespace-separated tokens of a gzip file
struct GzTokens {
    gzFile f = nullptr;
    std::vector<char> buf = std::vector<char>(1 << 20);
    size_t pos = 0, len = 0;
    bool eof = false;
    explicit GzTokens(const std::string &path) { f = gzopen(path.c_str(), "rb"); if (f) gzbuffer(f, 1 << 20); }
    ~GzTokens() { if (f) gzclose(f); }
    int get()
    {
        if (pos == len) {
            if (eof) return -1;
            const int r = gzread(f, buf.data(), (unsigned)buf.size());
            if (r <= 0) { eof = true; return -1; }
            len = (size_t)r; pos = 0;
        }
        return (unsigned char)buf[pos++];
    }
    bool line(std::string &out)
    {
        out.clear();
        int c;
        while ((c = get()) >= 0 && c != '\n') out.push_back((char)c);
        return c >= 0 || !out.empty();
    }
    bool token(char *tmp, size_t cap)
    {
        int c;
        while ((c = get()) >= 0 && (c == ' ' || c == '\n' || c == '\t' || c == '\r')) {}
        if (c < 0) return false;
        size_t n = 0;
        while (c >= 0 && !(c == ' ' || c == '\n' || c == '\t' || c == '\r')) { if (n + 1 < cap) tmp[n++] = (char)c; c = get(); }
        tmp[n] = 0;
        return true;
    }
};

// One trace file: the ids of its header line and the tracelen x ids values, row-major (values as atof reads them: "NA" is 0)
inline std::string read_trace(const std::string &path, int tracelen, std::vector<std::string> &ids, std::vector<double> &vals)
{
    GzTokens g(path);
    if (!g.f) return "Error: couldn't open " + path + ".";
    std::string head;
    if (!g.line(head)) return "Error: " + path + " is empty.";
    ids = tokenise(head, " ");
    vals.assign((size_t)tracelen * ids.size(), 0.0);
    char tmp[64];
    for (size_t i = 0; i < vals.size(); ++i) {
        if (!g.token(tmp, sizeof tmp)) return "Error: " + path + " is truncated (fewer than " + std::to_string(tracelen) + " rows).";
        vals[i] = atof(tmp);
    }
    return std::string();
}

} // namespace traceio
