// pairs_gen.hpp -- the pairs of mmseq -pairs: which transcripts share a hit set.  Plain host code, no device.
//
// Every hit set (row of the collapsed hits: its transcripts col_idx[row_ptr[i] .. row_ptr[i + 1]) and its multiplicity k[i]) with 2 to
// maxset transcripts contributes each unordered pair of its transcripts, with shared_hits += k[i] and shared_sets += 1.  Longer sets
// contribute nothing and are counted (a paralogue family row of 5 000 transcripts would be 12.5 M pairs, none of them informative).
// The output is the distinct pairs with a < b in the numbering of `label` (null: the columns themselves), sorted by (a, b):
// emit, sort, reduce.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace pairsgen {

struct Pair {
    uint32_t a, b;             // a < b
    uint64_t shared_hits;      // the summed multiplicity of the sets that hold both
    uint32_t shared_sets;
};

struct Result {
    std::vector<Pair> pairs;
    uint64_t skipped_sets = 0, skipped_hits = 0;   // the sets longer than maxset, and their summed multiplicity
};

constexpr uint64_t MAX_TUPLES = 1ull << 31;

// false with `error` set: maxset < 2, or more than 2^31 tuples would be emitted (nothing is emitted then)
inline bool generate(uint64_t n_sets, const uint64_t *row_ptr, const uint32_t *col_idx, const uint32_t *k, const uint32_t *label, int maxset,
                     Result &out, std::string &error)
{
    out = Result();
    if (maxset < 2) { error = "pairs_maxset must be at least 2"; return false; }
    uint64_t tuples = 0;
    for (uint64_t i = 0; i < n_sets; ++i) {
        const uint64_t L = row_ptr[i + 1] - row_ptr[i];
        if (L > (uint64_t)maxset) { out.skipped_sets += 1; out.skipped_hits += k[i]; continue; }
        tuples += L * (L - (L > 0)) / 2;
        if (tuples > MAX_TUPLES) {
            error = "the hit sets of up to " + std::to_string(maxset) + " transcripts hold more than 2^31 pairs of transcripts: a lower -pairs_maxset is the way out";
            out = Result();
            return false;
        }
    }
    struct Tuple { uint64_t key; uint32_t k; };
    std::vector<Tuple> t;
    t.reserve(tuples);
    for (uint64_t i = 0; i < n_sets; ++i) {
        const uint64_t b0 = row_ptr[i], e0 = row_ptr[i + 1];
        if (e0 - b0 < 2 || e0 - b0 > (uint64_t)maxset) continue;
        for (uint64_t x = b0; x < e0; ++x)
            for (uint64_t y = x + 1; y < e0; ++y) {
                uint32_t a = label ? label[col_idx[x]] : col_idx[x], b = label ? label[col_idx[y]] : col_idx[y];
                if (a == b) continue;          // (a transcript listed twice in a set is no pair)
                if (a > b) std::swap(a, b);
                t.push_back(Tuple{((uint64_t)a << 32) | b, k[i]});
            }
    }
    std::sort(t.begin(), t.end(), [](const Tuple &x, const Tuple &y) { return x.key < y.key; });
    for (size_t i = 0; i < t.size();) {
        Pair p{(uint32_t)(t[i].key >> 32), (uint32_t)t[i].key, 0, 0};
        size_t j = i;
        for (; j < t.size() && t[j].key == t[i].key; ++j) { p.shared_hits += t[j].k; p.shared_sets += 1; }
        out.pairs.push_back(p);
        i = j;
    }
    return true;
}

} // namespace pairsgen
