// mmsim -- posterior distances and correlations between samples, from their joint posterior draws.
//
//   Usage: mmsim [-level transcript|identical|gene] [-nonorm] [-uhfrac FLOAT] [-uhmin INT] [-centre mean|none]
//                [-percentiles 2.5,50,97.5] [-matrix FILE] [-device INT] base1 base2 [base3 ...] > out.mmsim
//
// Samples are independent given their reads, so draw t of every sample together is one draw from the joint posterior of all the
// expression profiles: a distance matrix computed per draw gives as many posterior draws of that matrix as a trace has rows.  The host
// reads the tables and the gzip traces of the chosen level, takes the offsets by mmdiff's normalisation rule and the centre from the
// tables, and matches the trace columns to the table's features by name; the Gram matrices (on the matrix cores) and the summaries
// come from the device through libmmgibbs' C ABI (include/mmgibbs.h: mmg_sim_*).  tests/sim_ref.py restates the
// offsets, the mask, the centre, the ranks and the texts.
// There is no CPU path: without a HIP device the program stops with an error once the inputs are checked.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

static const size_t MAX_SAMPLES = 256;
static const uint32_t MAX_RANKS = 64, MAX_T = 4096;
static const size_t MIN_NORM_FEATURES = 100;   // mmdiff: "fewer than 100 features found for normalisation. Skipping."

static void printUsage(ostream &out)
{
    out << "Usage: mmsim [-level transcript|identical|gene] [-nonorm] [-uhfrac FLOAT] [-uhmin INT] [-centre mean|none]" << endl
        << "             [-percentiles 2.5,50,97.5] [-matrix FILE] [-device INT] base1 base2 [base3 ...] > out.mmsim" << endl
        << "Posterior distance (root-mean-square log ratio) and correlation across features of every pair of samples, and every" << endl
        << "sample's nearest neighbour, from the joint posterior draws of all the samples." << endl
        << "  -level STRING       which tables and traces to read: transcript (<base>.mmseq, <base>.trace_gibbs.gz), identical" << endl
        << "                      (<base>.identical.mmseq, ...) or gene (<base>.gene.mmseq, ...) (default: transcript)" << endl
        << "  -nonorm             no offsets between the samples (default: mmdiff's normalisation: per sample minus the median of" << endl
        << "                      log_mu minus the features' means, over the features with a unique hit in at least uhfrac of the" << endl
        << "                      samples; skipped with fewer than 100 such features)" << endl
        << "  -uhfrac FLOAT       see -nonorm; <= 1 and >= 1/N (default: max(0.2, (N - floor(N^2/160))/N))" << endl
        << "  -uhmin INT          unique hits a feature needs in every sample to be used (default: 1)" << endl
        << "  -centre STRING      mean: subtract from every feature its mean log_mu over the samples, offsets included, so that the" << endl
        << "                      correlation is one of deviations; none: the raw correlation (default: mean)" << endl
        << "  -percentiles STR    comma-separated percentiles of the distance and of the correlation, each in [0, 100]" << endl
        << "                      (default: 2.5,50,97.5)" << endl
        << "  -matrix FILE        also write the matrix of mean distances to FILE" << endl
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
    if (std::isnan(x)) return "nan";
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

// The ids of a trace file's header line and the number of values below it.  No value is copied or parsed: the inflated blocks are
// scanned for the starts of tokens, so this pass costs the inflation and little more (DESIGN.md section 17 has the measured share).
// Returns an error message, or "".
static string scan_trace(const string &path, vector<string> &ids, uint64_t &n_values)
{
    traceio::GzTokens g(path);
    if (!g.f) return "Error: couldn't open " + path + ".";
    string head;
    if (!g.line(head)) return "Error: " + path + " is empty.";
    ids = tokenise(head, " ");
    if (ids.empty()) return "Error: " + path + " has no column.";
    n_values = 0;
    bool in_token = false;
    for (;;) {
        const char *p = g.buf.data() + g.pos, *const end = g.buf.data() + g.len;
        uint64_t starts = 0;
        for (; p != end; ++p) {
            const bool tok = !(*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r');
            starts += tok && !in_token;
            in_token = tok;
        }
        n_values += starts;
        g.pos = g.len;
        if (g.get() < 0) break;   // (refills the block)
        --g.pos;
    }
    return string();
}

// C's round() of p / 100 (T - 1), as mmseq -percentiles turns a percentage into an index of the sorted draws
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
    string level = "transcript", centre_mode = "mean", matrix_path;
    bool nonorm = false, custom_uhfrac = false;
    double uhfrac = -1;
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
        } else if (a == "-centre") {
            centre_mode = value();
            if (centre_mode != "mean" && centre_mode != "none") refuse("Error: unknown centre " + centre_mode + " (mean or none).");
        } else if (a == "-nonorm") {
            nonorm = true;
        } else if (a == "-uhfrac") {
            if (!parse_double(value(), uhfrac) || !std::isfinite(uhfrac)) refuse("Error: -uhfrac must be a number.");
            custom_uhfrac = true;
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
        } else if (a == "-matrix") {
            matrix_path = value();
        } else if (a == "-device") {
            const string v = value();
            char *end = nullptr;
            device = (int)strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != '\0' || device < 0) refuse("Error: -device must be a non-negative integer.");
        } else if (a.size() > 1 && a[0] == '-') {
            refuse("Error: unrecognised option " + a + ".");
        } else bases.push_back(a);
    }
    const size_t S = bases.size();
    if (S < 2) refuse("Error: at least two basenames are needed (" + to_string(S) + " given).");
    if (S > MAX_SAMPLES) refuse("Error: at most " + to_string(MAX_SAMPLES) + " basenames are taken (" + to_string(S) + " given).");
    if (percentiles.size() > MAX_RANKS) refuse("Error: more than " + to_string(MAX_RANKS) + " ranks (" + to_string(percentiles.size()) + " percentiles).");
    if (custom_uhfrac && (uhfrac > 1 || uhfrac < 1.0 / (double)S)) refuse("Error: uhfrac must be <= 1 and >= 1/N.");
    if (!custom_uhfrac) uhfrac = max(0.2, (double)((long)S - (long)(S * S / 160)) / (double)S);   // (signed: above 160 samples the term is negative)

    // ---- tables: the same features in the same order
    const string infix = level == "transcript" ? "" : "." + level;
    vector<Table> tab(S);
    for (size_t s = 0; s < S; ++s) read_table(bases[s] + infix + ".mmseq", tab[s]);
    const size_t F = tab[0].id.size();
    for (size_t s = 1; s < S; ++s) {
        if (tab[s].id.size() != F)
            refuse("Error: the tables of " + bases[0] + " and " + bases[s] + " list different numbers of features (" + to_string(F) + " and " +
                   to_string(tab[s].id.size()) + ").");
        for (size_t f = 0; f < F; ++f)
            if (tab[0].id[f] != tab[s].id[f])
                refuse("Error: the tables of " + bases[0] + " and " + bases[s] + " do not list the same features in the same order (row " + to_string(f + 1) +
                       ": " + tab[0].id[f] + " and " + tab[s].id[f] + ").");
    }
    if (F > 0x7fffffffu) refuse("Error: more than 2^31 - 1 features.");

    // ---- traces: the columns of every file and one trace length
    map<string, size_t> row_of;
    for (size_t f = 0; f < F; ++f) row_of.emplace(tab[0].id[f], f);
    vector<vector<int64_t>> feature_of(S);   // per file: the table's row of every column, -1 for a column the tables do not list
    vector<uint8_t> traced(F * S, 0);
    uint64_t T = 0;
    for (size_t s = 0; s < S; ++s) {
        const string path = bases[s] + infix + ".trace_gibbs.gz";
        vector<string> ids;
        uint64_t n_values = 0;
        const string err = scan_trace(path, ids, n_values);
        if (!err.empty()) refuse(err);
        if (n_values == 0 || n_values % ids.size())
            refuse("Error: " + path + " is truncated (" + to_string(n_values) + " values are not whole rows of " + to_string(ids.size()) + ").");
        const uint64_t rows = n_values / ids.size();
        if (rows > MAX_T) refuse("Error: " + path + " has " + to_string(rows) + " rows, more than " + to_string(MAX_T) + ".");
        if (s == 0) T = rows;
        else if (rows != T)
            refuse("Error: the trace lengths differ (" + to_string(T) + " rows in " + bases[0] + infix + ".trace_gibbs.gz and " + to_string(rows) + " in " + path + ").");
        feature_of[s].assign(ids.size(), -1);
        for (size_t c = 0; c < ids.size(); ++c) {
            const auto it = row_of.find(ids[c]);
            if (it == row_of.end() || traced[it->second * S + s]) continue;   // (a name listed twice: its first column)
            feature_of[s][c] = (int64_t)it->second;
            traced[it->second * S + s] = 1;
        }
    }

    // ---- the mask, the offsets (mmdiff's normalisation; off_s = minus the sample's median) and the centre
    vector<uint8_t> mask(F);
    for (size_t f = 0; f < F; ++f) {
        bool ok = true;
        for (size_t s = 0; s < S; ++s) ok = ok && tab[s].uh[f] >= uhmin && std::isfinite(tab[s].log_mu[f]) && traced[f * S + s];
        mask[f] = ok;
    }
    vector<double> off(S, 0.0);
    if (!nonorm) {
        vector<size_t> use;
        for (size_t f = 0; f < F; ++f) {
            int sum = 0;
            bool finite = true;
            for (size_t s = 0; s < S; ++s) {
                if (tab[s].uh[f] > 0) sum++;
                finite = finite && std::isfinite(tab[s].log_mu[f]);
            }
            if ((double)sum / (double)S >= uhfrac && finite) use.push_back(f);
        }
        if (use.size() < MIN_NORM_FEATURES) cerr << "Warning: fewer than 100 features found for normalisation. Skipping.\n";
        else {
            vector<double> rowMeans;
            for (size_t f : use) {
                double sum = 0;
                for (size_t s = 0; s < S; ++s) sum += tab[s].log_mu[f];
                rowMeans.push_back(sum / (double)S);
            }
            for (size_t s = 0; s < S; ++s) {
                vector<double> ydiff;
                for (size_t i = 0; i < use.size(); ++i) ydiff.push_back(tab[s].log_mu[use[i]] - rowMeans[i]);
                sort(ydiff.begin(), ydiff.end());
                off[s] = -ydiff[ydiff.size() / 2];
            }
        }
    }
    vector<double> centre;
    if (centre_mode == "mean") {
        centre.assign(F, 0.0);
        for (size_t f = 0; f < F; ++f) {
            if (!mask[f]) continue;
            double sum = 0.0;
            for (size_t s = 0; s < S; ++s) sum += tab[s].log_mu[f] + off[s];
            centre[f] = sum / (double)S;
        }
    }
    vector<uint32_t> ranks;
    for (double p : percentiles) ranks.push_back(rank_of(p, T));
    const uint32_t nr = (uint32_t)ranks.size();

    int ndev = 0;
    if (mmg_device_count(&ndev) != 0 || ndev < 1) die("Error: no HIP device available: mmsim has no CPU fallback");

    // ---- the samples one after another: one trace in host memory at a time, a column without a feature skipped
    mmg_sim *h = nullptr;
    MMG_CHECK(mmg_sim_create(device, (uint32_t)S, (uint32_t)F, (uint32_t)T, centre.empty() ? nullptr : centre.data(), mask.data(), 0, &h));
    {
        vector<double> buf((size_t)T * F);
        char tmp[64];
        for (size_t s = 0; s < S; ++s) {
            const string path = bases[s] + infix + ".trace_gibbs.gz";
            traceio::GzTokens g(path);
            string head;
            if (!g.f || !g.line(head)) die("Error: couldn't read " + path + " again.");
            fill(buf.begin(), buf.end(), 0.0);   // (a feature without a column: no valid draw; the mask leaves it out already)
            const size_t W = feature_of[s].size();
            for (uint64_t t = 0; t < T; ++t)
                for (size_t c = 0; c < W; ++c) {
                    if (!g.token(tmp, sizeof tmp)) die("Error: " + path + " changed while it was read.");
                    if (feature_of[s][c] >= 0) buf[t * F + (size_t)feature_of[s][c]] = atof(tmp);
                }
            MMG_CHECK(mmg_sim_set_sample(h, (uint32_t)s, buf.data(), off[s]));
        }
    }
    MMG_CHECK(mmg_sim_run(h, nr, ranks.data()));
    const size_t P = S * (S - 1) / 2;
    vector<double> mean_D(P), ss_D(P), mean_R(P), ss_R(P), q_D(P * nr), q_R(P * nr);
    vector<uint32_t> nn(S * S);
    vector<uint8_t> pair_status(P);
    uint8_t status = 0;
    uint64_t n_used = 0;
    MMG_CHECK(mmg_sim_get_used(h, nullptr, &n_used));
    MMG_CHECK(mmg_sim_get(h, mean_D.data(), ss_D.data(), q_D.data(), mean_R.data(), ss_R.data(), q_R.data(), nn.data(), pair_status.data(), &status));
    mmg_sim_destroy(h);

    // ---- the table
    cout << "# mmsim: posterior distance (root-mean-square log ratio) and correlation between samples, from their joint posterior draws\n"
         << "# level: " << level << "\n"
         << "# T: " << T << "\n"
         << "# features: " << n_used << "/" << F << "\n"
         << "# centre: " << centre_mode << "\n";
    for (size_t s = 0; s < S; ++s) cout << "# sample " << s << ": " << bases[s] << " offset " << fmt(off[s]) << "\n";
    string pc;
    for (size_t i = 0; i < percentiles.size(); ++i) pc += (i ? "," : "") + fmt(percentiles[i]);
    cout << "sample_a\tsample_b\tdist\tdist_sd\tdist_percentiles" << pc << "\tcor\tcor_sd\tcor_percentiles" << pc << "\tnearest_a\tnearest_b\tstatus\n";
    size_t p = 0;
    for (size_t a = 0; a < S; ++a)
        for (size_t b = a + 1; b < S; ++b, ++p) {
            cout << bases[a] << "\t" << bases[b] << "\t" << fmt(mean_D[p]) << "\t" << fmt(sqrt(ss_D[p] / (double)(T - 1))) << "\t";
            for (uint32_t k = 0; k < nr; ++k) cout << (k ? "," : "") << fmt(q_D[p * nr + k]);
            cout << "\t" << fmt(mean_R[p]) << "\t" << fmt(sqrt(ss_R[p] / (double)(T - 1))) << "\t";
            for (uint32_t k = 0; k < nr; ++k) cout << (k ? "," : "") << fmt(q_R[p * nr + k]);
            cout << "\t" << fmt(status ? NAN : (double)nn[a * S + b] / (double)T) << "\t" << fmt(status ? NAN : (double)nn[b * S + a] / (double)T) << "\t"
                 << (int)(pair_status[p] | status) << "\n";
        }
    cout.flush();
    if (!cout) die("Error: writing the table failed");

    if (!matrix_path.empty()) {
        ofstream mf(matrix_path.c_str());
        vector<double> M(S * S, 0.0);
        p = 0;
        for (size_t a = 0; a < S; ++a)
            for (size_t b = a + 1; b < S; ++b, ++p) M[a * S + b] = M[b * S + a] = mean_D[p];
        for (size_t b = 0; b < S; ++b) mf << "\t" << bases[b];
        mf << "\n";
        for (size_t a = 0; a < S; ++a) {
            mf << bases[a];
            for (size_t b = 0; b < S; ++b) mf << "\t" << (a == b ? string("0") : fmt(M[a * S + b]));
            mf << "\n";
        }
        mf.flush();
        if (!mf) die("Error: writing " + matrix_path + " failed");
    }
    return 0;
}
