// The value of mmseq -iso_thresholds: up to 8 comma-separated shares of a gene, each a number in [0, 1).  Plain host code.
#pragma once
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace isocli {

constexpr size_t MAX_THRESHOLDS = 8;

// false with `error` set: an empty field, a field that is no number or has trailing characters, a value that is not finite or lies
// outside [0, 1), more than MAX_THRESHOLDS fields
inline bool parse_thresholds(const std::string &text, std::vector<double> &out, std::string &error)
{
    out.clear();
    size_t at = 0;
    for (;;) {
        const size_t end = text.find(',', at);
        const std::string field = text.substr(at, end == std::string::npos ? std::string::npos : end - at);
        char *stop = nullptr;
        const double v = field.empty() ? 0.0 : strtod(field.c_str(), &stop);
        if (field.empty() || stop == field.c_str() || *stop != '\0') {
            error = "-iso_thresholds: `" + field + "` is no number.";
            return false;
        }
        if (!std::isfinite(v) || !(v >= 0.0 && v < 1.0)) {
            error = "-iso_thresholds: " + field + " lies outside [0, 1).";
            return false;
        }
        if (out.size() == MAX_THRESHOLDS) {
            error = "-iso_thresholds takes at most " + std::to_string(MAX_THRESHOLDS) + " thresholds.";
            return false;
        }
        out.push_back(v);
        if (end == std::string::npos) return true;
        at = end + 1;
    }
}

} // namespace isocli
