// mmfold -- the posterior log fold change of every feature between two samples, from all pairs of their posterior draws.
//
//   Usage: mmfold [-level transcript|identical|gene] [-nonorm | -offset FLOAT] [-uhmin INT] [-percentiles 2.5,50,97.5] [-gfold 0.01]
//                 [-device INT] baseA baseB > out.mmfold
//
// Two samples are independent given their reads, so every pair (draw i of A, draw j of B) of the 1024 kept draws of each is a draw
// from the joint posterior of the log fold change: 2^20 of them per feature.  The host reads the two tables and the two gzip traces
// of the chosen level, matches the trace columns to the table's features by name and takes the offset from the tables; the moments,
// the exact counts and the exact order statistics come from the device through libmmgibbs' C ABI (include/mmgibbs.h: mmg_fold_*,
// DESIGN.md section 16).  tests/fold_ref.py restates the offset, the ranks, gfold and the table.
// There is no CPU path: without a HIP device the program stops with an error once the inputs are checked.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../../../include/mmgibbs.h"
#include "trace_io.hpp"

using namespace std;
using traceio::TableReader;
using traceio::find_col;
using traceio::tokenise;

static const int TRACELEN = 1024;   // the kept draws of an mmseq run
static const uint32_t MAX_RANKS = 64;
enum { STATUS_BAD_A = 1, STATUS_BAD_B = 2, STATUS_NO_TRACE = 4 };

static void printUsage(ostream &out)
{
    out << "Usage: mmfold [-level transcript|identical|gene] [-nonorm | -offset FLOAT] [-uhmin INT]" << endl
        << "              [-percentiles 2.5,50,97.5] [-gfold 0.01] [-device INT] baseA baseB > out.mmfold" << endl
        << "Posterior log fold change of every feature of sample A against sample B, from all 1024 x 1024 pairs of their posterior draws." << endl
        << "This is the posterior given the reads of these two libraries; it says nothing about biological variability: for groups" << endl
        << "with replicates the tool is mmdiff." << endl
        << "  -level STRING       which tables and traces to read: transcript (<base>.mmseq, <base>.trace_gibbs.gz), identical" << endl
        << "                      (<base>.identical.mmseq, ...) or gene (<base>.gene.mmseq, ...) (default: transcript)" << endl
        << "  -nonorm             no offset between the samples (default: the median of log_mu_A - log_mu_B over the features with" << endl
        << "                      at least -uhmin unique hits and a finite log_mu in both samples, added to sample B)" << endl
        << "  -offset FLOAT       the offset, on the natural-log scale, instead of the median; not with -nonorm" << endl
        << "  -uhmin INT          unique hits a feature needs in both samples to count towards the offset (default: 1)" << endl
        << "  -percentiles STR    comma-separated percentiles of the log fold change to output, each in [0, 100] (default: 2.5,50,97.5)" << endl
        << "  -gfold FLOAT        c in (0, 0.5): gfold is the 100 c-th percentile if it is above 0, the 100 (1 - c)-th if that is" << endl
        << "                      below 0, else 0 (default: 0.01)" << endl
        << "  -device INT         the HIP device to use (default: 0)" << endl;
}

[[noreturn]] static void refuse(const string &msg)
{
    cerr << msg << endl;
    printUsage(cerr);
    exit(1);
}

[[noreturn]] static void die(const string &msg)
{
    cerr << msg << endl;
    exit(1);
}

// ostream's default formatting of a double (%g, 6 digits), as mmdiff prints its numbers
static string fmt(double x)
{
    if (std::isnan(x)) return std::signbit(x) ? "-nan" : "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%g", x);
    return buf;
}

static bool parse_double(const string &s, double &v)
{
    char *end = nullptr;
    v = strtod(s.c_str(), &end);
    return !s.empty() && *end == '\0';
}

struct Table {
    vector<string> id;
    vector<double> log_mu;
    vector<long> uh;
};

static void read_table(const string &path, Table &tb)
{
    TableReader r;
    const int rc = r.open(path);
    if (rc == TableReader::CANNOT_OPEN) refuse("Error: cannot open " + path);
    if (rc == TableReader::TRUNCATED) refuse("Error: " + path + " is truncated (no header line).");
    const char *need[] = {"feature_id", "log_mu", "unique_hits"};
    int col[3];
    for (int i = 0; i < 3; ++i) {
        col[i] = find_col(r.hdr, need[i]);
        if (col[i] < 0) refuse("Error: " + path + " does not contain a \"" + need[i] + "\" column.");
    }
    const int maxcol = *max_element(col, col + 3);
    vector<string> t;
    while (r.row(t)) {
        if ((int)t.size() <= maxcol) refuse("Error: malformed line in " + path + ": " + r.line);
        tb.id.push_back(t[col[0]]);
        double v;
        tb.log_mu.push_back(parse_double(t[col[1]], v) ? v : NAN);   // "NA": no estimate
        tb.uh.push_back(atol(t[col[2]].c_str()));
    }
    if (tb.id.empty()) refuse("Error: " + path + " lists no feature.");
}

// C's round() of p / 100 (n - 1), as mmseq -percentiles turns a percentage into an index of the sorted draws
static uint32_t rank_of(double p, uint64_t n)
{
    return (uint32_t)round(p / 100.0 * (double)(n - 1));
}

#define MMG_CHECK(call)                                                                                   \
    do {                                                                                                  \
        if ((call) != 0) die(string("Error: ") + #call + ": " + mmg_last_error());                       \
    } while (0)

int main(int argc, char **argv)
{
    string level = "transcript";
    bool nonorm = false, have_offset = false;
    double offset = 0.0, gfold_c = 0.01;
    long uhmin = 1;
    int device = 0;
    vector<double> percentiles = {2.5, 50.0, 97.5};
    vector<string> bases;
    for (int i = 1; i < argc; i++) {
        const string a = argv[i];
        auto value = [&]() -> string {
            if (i + 1 >= argc) refuse("Error: " + a + " needs a value.");
            return argv[++i];
        };
        if (a == "-h" || a == "-help" || a == "--help") {
            printUsage(cerr);
            return 1;
        } else if (a == "-level") {
            level = value();
            if (level != "transcript" && level != "identical" && level != "gene") refuse("Error: unknown level " + level + " (transcript, identical or gene).");
        } else if (a == "-nonorm") {
            nonorm = true;
        } else if (a == "-offset") {
            const string v = value();
            if (!parse_double(v, offset) || !std::isfinite(offset)) refuse("Error: -offset must be a finite number.");
            have_offset = true;
        } else if (a == "-uhmin") {
            const string v = value();
            char *end = nullptr;
            uhmin = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || uhmin < 0) refuse("Error: -uhmin must be a non-negative integer.");
        } else if (a == "-percentiles") {
            percentiles.clear();
            for (const string &tok : tokenise(value(), ",")) {
                double p;
                if (!parse_double(tok, p) || !(p >= 0.0 && p <= 100.0)) refuse("Error: percentiles must be numbers between 0 and 100.");
                percentiles.push_back(p);
            }
            if (percentiles.empty()) refuse("Error: -percentiles needs at least one percentile.");
        } else if (a == "-gfold") {
            if (!parse_double(value(), gfold_c) || !(gfold_c > 0.0 && gfold_c < 0.5)) refuse("Error: -gfold must be above 0 and below 0.5.");
        } else if (a == "-device") {
            const string v = value();
            char *end = nullptr;
            device = (int)strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || device < 0) refuse("Error: -device must be a non-negative integer.");
        } else if (a.size() > 1 && a[0] == '-') {
            refuse("Error: unrecognised option " + a + ".");
        } else bases.push_back(a);
    }
    if (bases.size() != 2) refuse("Error: exactly two basenames are needed (" + to_string(bases.size()) + " given).");
    if (nonorm && have_offset) refuse("Error: -nonorm and -offset exclude each other.");
    if (percentiles.size() + 2 > MAX_RANKS)
        refuse("Error: more than " + to_string(MAX_RANKS) + " ranks (" + to_string(percentiles.size()) + " percentiles and the two of -gfold).");

    // ---- tables: the same features in the same order
    const string infix = level == "transcript" ? "" : "." + level;
    Table tab[2];
    for (int s = 0; s < 2; ++s) read_table(bases[s] + infix + ".mmseq", tab[s]);
    const size_t F = tab[0].id.size();
    if (tab[1].id.size() != F) refuse("Error: the two tables list different numbers of features (" + to_string(F) + " and " + to_string(tab[1].id.size()) + ").");
    for (size_t f = 0; f < F; ++f)
        if (tab[0].id[f] != tab[1].id[f])
            refuse("Error: the two tables do not list the same features in the same order (row " + to_string(f + 1) + ": " + tab[0].id[f] + " and " + tab[1].id[f] + ").");

    // ---- the offset (readmmseq's scaling rule for two samples)
    size_t n_off = 0;
    if (!nonorm && !have_offset) {
        vector<double> d;
        for (size_t f = 0; f < F; ++f)
            if (tab[0].uh[f] >= uhmin && tab[1].uh[f] >= uhmin && std::isfinite(tab[0].log_mu[f]) && std::isfinite(tab[1].log_mu[f]))
                d.push_back(tab[0].log_mu[f] - tab[1].log_mu[f]);
        if (d.empty()) refuse("Error: no feature has " + to_string(uhmin) + " unique hits and a finite log_mu in both samples: use -nonorm or -offset.");
        sort(d.begin(), d.end());
        n_off = d.size();
        offset = n_off % 2 ? d[n_off / 2] : (d[n_off / 2 - 1] + d[n_off / 2]) / 2.0;
    }

    // ---- traces, their columns matched to the features by name
    vector<string> ids[2];
    vector<double> vals[2];
    for (int s = 0; s < 2; ++s) {
        const string err = traceio::read_trace(bases[s] + infix + ".trace_gibbs.gz", TRACELEN, ids[s], vals[s]);
        if (!err.empty()) refuse(err);
    }
    const uint32_t Sa = TRACELEN, Sb = TRACELEN;
    const uint64_t n_pairs = (uint64_t)Sa * Sb;
    vector<uint32_t> ranks;
    for (double p : percentiles) ranks.push_back(rank_of(p, n_pairs));
    ranks.push_back(rank_of(100.0 * gfold_c, n_pairs));
    ranks.push_back(rank_of(100.0 * (1.0 - gfold_c), n_pairs));
    const uint32_t nr = (uint32_t)ranks.size(), nP = (uint32_t)percentiles.size();

    map<string, size_t> col_of[2];
    for (int s = 0; s < 2; ++s)
        for (size_t c = 0; c < ids[s].size(); ++c) col_of[s].emplace(ids[s][c], c);
    vector<size_t> have;   // the features with a column in both files
    vector<double> A, B;   // their draws, series-major
    for (size_t f = 0; f < F; ++f) {
        const auto ia = col_of[0].find(tab[0].id[f]), ib = col_of[1].find(tab[0].id[f]);
        if (ia == col_of[0].end() || ib == col_of[1].end()) continue;
        have.push_back(f);
        const size_t wa = ids[0].size(), wb = ids[1].size();
        for (uint32_t k = 0; k < Sa; ++k) A.push_back(vals[0][k * wa + ia->second]);
        for (uint32_t k = 0; k < Sb; ++k) B.push_back(vals[1][k * wb + ib->second]);
    }

    int ndev = 0;
    if (mmg_device_count(&ndev) != 0 || ndev < 1) die("Error: no HIP device available: mmfold has no CPU fallback");

    const size_t H = have.size();
    vector<double> mean_a(H), mean_b(H), ss_a(H), ss_b(H), q((size_t)H * nr);
    vector<uint32_t> n_gt(H), n_eq(H);
    vector<uint8_t> status(H);
    if (H) {
        mmg_fold *h = nullptr;
        MMG_CHECK(mmg_fold_of_traces(device, (uint32_t)H, Sa, A.data(), Sb, B.data(), offset, nr, ranks.data(), &h));
        MMG_CHECK(mmg_fold_get(h, mean_a.data(), mean_b.data(), ss_a.data(), ss_b.data(), n_gt.data(), n_eq.data(), q.data(), status.data()));
        mmg_fold_destroy(h);
    }

    // ---- the table
    cout << "# mmfold: posterior log fold change of A against B from all pairs of their draws, given the reads of these two libraries" << "\n"
         << "# A: " << bases[0] << "\n"
         << "# B: " << bases[1] << "\n"
         << "# level: " << level << "\n"
         << "# Sa: " << Sa << "\n"
         << "# Sb: " << Sb << "\n"
         << "# offset: " << fmt(offset) << "\n"
         << "# offset_features: " << n_off << "\n";
    cout << "feature_id\tlog_mu_a\tlog_mu_b\tlfc\tsd\tp_gt\tn_gt\tn_eq\tgfold\tpercentiles";
    for (uint32_t i = 0; i < nP; ++i) cout << (i ? "," : "") << fmt(percentiles[i]);
    cout << "\tstatus\n";
    size_t at = 0;
    const string nan = fmt(NAN);
    for (size_t f = 0; f < F; ++f) {
        const bool traced = at < H && have[at] == f;
        const int st = traced ? status[at] : STATUS_NO_TRACE;
        cout << tab[0].id[f] << "\t";
        if (st != 0) {
            cout << nan << "\t" << nan << "\t" << nan << "\t" << nan << "\t" << nan << "\t0\t0\t" << nan << "\t";
            for (uint32_t i = 0; i < nP; ++i) cout << (i ? "," : "") << nan;
        } else {
            const double lfc = mean_a[at] - mean_b[at];
            const double sd = sqrt(ss_a[at] / (double)(Sa - 1) + ss_b[at] / (double)(Sb - 1));
            const double p_gt = ((double)n_gt[at] + (double)n_eq[at] / 2.0) / (double)n_pairs;
            const double lo = q[at * nr + nP], hi = q[at * nr + nP + 1];
            const double gfold = lo > 0 ? lo : hi < 0 ? hi : 0.0;
            cout << fmt(mean_a[at]) << "\t" << fmt(mean_b[at]) << "\t" << fmt(lfc) << "\t" << fmt(sd) << "\t" << fmt(p_gt) << "\t" << n_gt[at] << "\t"
                 << n_eq[at] << "\t" << fmt(gfold) << "\t";
            for (uint32_t i = 0; i < nP; ++i) cout << (i ? "," : "") << fmt(q[at * nr + i]);
        }
        cout << "\t" << st << "\n";
        if (traced) ++at;
    }
    cout.flush();
    if (!cout) die("Error: writing the table failed");
    return 0;
}
