// pairs_gen_test FILE MAXSET: the pair generation of mmseq -pairs (pairs_gen.hpp) on a file of hit sets, one per line as
// `k t0 t1 ...`; prints `a b shared_hits shared_sets` per pair in (a, b) order and a last line `skipped_sets N skipped_hits K`
// (tests/test_pairs_cli.py compares with its restatement of the rule).
#include "pairs_gen.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char **argv)
{
    if (argc != 3) { std::cerr << "usage: pairs_gen_test FILE MAXSET\n"; return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
    std::vector<uint64_t> row_ptr(1, 0);
    std::vector<uint32_t> col, k;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        unsigned long long v;
        if (!(fields >> v)) continue;          // a blank line
        k.push_back((uint32_t)v);
        while (fields >> v) col.push_back((uint32_t)v);
        row_ptr.push_back(col.size());
    }
    pairsgen::Result r;
    std::string error;
    if (!pairsgen::generate(k.size(), row_ptr.data(), col.data(), k.data(), nullptr, atoi(argv[2]), r, error)) {
        std::cerr << "Error: " << error << "\n";
        return 1;
    }
    for (const pairsgen::Pair &p : r.pairs) printf("%u %u %llu %u\n", p.a, p.b, (unsigned long long)p.shared_hits, p.shared_sets);
    printf("skipped_sets %llu skipped_hits %llu\n", (unsigned long long)r.skipped_sets, (unsigned long long)r.skipped_hits);
    return 0;
}
