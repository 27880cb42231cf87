// mmcollapse -- drop-in for the reference's `mmcollapse` (src/mmcollapse.cpp): transcripts that no sample can tell apart are merged,
// by their mean posterior anti-correlation across samples, into "*"-joined sets, and <base>.collapsed.mmseq is written per sample.
//
//   Usage: mmcollapse [-thres FLOAT] basename1 [basename2 ...]
//
// The host reads the tables, the gzip traces (each file once, a thread per sample) and the .M / .k files, and writes the tables; the
// covariances, the mean correlations, the greedy loop and the per-series summaries run on the device through libmmgibbs' C ABI
// (include/mmgibbs.h: mmg_collapse_*).  Deliberate differences from the reference (DESIGN.md "mmcollapse"): simulated traces come from
// the library's keyed gamma streams (seed 13837, the sample, feature index, row) rather than GSL's MT19937; -thres 100 and fewer than
// two candidates are defined (the threshold index is clamped to C - 1; with fewer than two candidates nothing collapses); an invalid
// -thres stops with the usage text; V is computed in fp64 in a fixed summation order (reruns are bit-identical).
// There is no CPU path: without a HIP device the program stops with an error once the inputs are checked.
#include <omp.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mmgibbs.h"
#include "stage_timer.hpp"
#include "trace_io.hpp"

using namespace std;
using traceio::TableReader;
using traceio::find_col;
using traceio::num;
using traceio::readable;
using traceio::tokenise;

static const int TRACELEN = 1024;
static const double IACTTHRES = 1.1;
static const double ALPHA = 0.1, BETA = 0.1;
static const uint64_t SIMU_SEED = 13837;

static void printUsage(ostream &out)
{
    out << "Usage: mmcollapse [-thres FLOAT] basename1 [basename2...]" << endl;
    out << "       -thres FLOAT   stopping threshold as -percentile of the maximum (over transcripts)" << endl
        << "                      mean (over samples) correlation (default 97.5; must lie in (0, 100])" << endl;
}

[[noreturn]] static void die(const string &msg)
{
    cerr << msg;
    if (msg.empty() || msg.back() != '\n') cerr << endl;
    exit(1);
}

// what one sample's tables contribute (get_unidentifiable_transcripts, src/mmcollapse.cpp:117-396)
struct Tables {
    vector<string> candidates, zeros, toremove;
    map<string, double> zero_efflen;
    long mapped = 0;
};

static void read_tables(const string &base, Tables &tb, vector<string> &all_features, bool want_all, map<string, bool> &isIdent)
{
    vector<double> sd;
    TableReader itab;
    int rc = itab.open(base + ".identical.mmseq");
    if (rc == TableReader::CANNOT_OPEN) die("Error: cannot open " + base + ".identical.mmseq");
    if (rc == TableReader::TRUNCATED) die("Error: truncated *identical.mmseq file?");
    const vector<string> &hdr = itab.hdr;
    const char *need[] = {"feature_id", "iact", "unique_hits", "observed", "sd", "log_mu", "effective_length"};
    int col[7];
    for (int i = 0; i < 7; ++i) {
        col[i] = find_col(hdr, need[i]);
        if (col[i] < 0) die("Error: " + base + ".identical.mmseq file does not contain \"" + need[i] + "\" column.");
    }
    int maxcol = *max_element(col, col + 7);
    const int ic = col[0], ac = col[1], ob = col[3], si = col[4], el = col[6];
    vector<string> t;
    while (itab.row(t)) {
        if ((int)t.size() <= maxcol) die("Error: malformed line in " + base + ".identical.mmseq: " + itab.line);
        tb.candidates.push_back(t[ic]);
        for (auto &m : tokenise(t[ic], "+")) isIdent[m] = true;
        if (want_all) all_features.push_back(t[ic]);
        if (t[ob] == "0") {
            sd.push_back(INFINITY);
            tb.zeros.push_back(t[ic]);
            tb.zero_efflen[t[ic]] = num(t[el]);
        } else sd.push_back(num(t[si]));
    }
    (void)ac;

    TableReader table;
    rc = table.open(base + ".mmseq");
    if (rc == TableReader::CANNOT_OPEN) die("Error: cannot open " + base + ".mmseq");
    bool have_mapped = false;
    for (const string &str : table.comments)
        if (str.find("Mapped fragments") != string::npos) {
            tb.mapped = (long)num(tokenise(str, " ").back());
            have_mapped = true;
        }
    if (rc == TableReader::TRUNCATED) die("Error: truncated *mmseq file?");
    if (!have_mapped) die("Error: " + base + ".mmseq has no \"# Mapped fragments\" line.");
    const char *need2[] = {"feature_id", "unique_hits", "iact", "observed", "sd", "log_mu", "effective_length"};
    for (int i = 0; i < 7; ++i) {
        col[i] = find_col(table.hdr, need2[i]);
        if (col[i] < 0) die("Error: " + base + ".mmseq file does not contain \"" + need2[i] + "\" column.");
    }
    maxcol = *max_element(col, col + 7);
    const int ic2 = col[0], uc = col[1], ac2 = col[2], ob2 = col[3], si2 = col[4], el2 = col[6];
    double max_h1_sd = 0;
    while (table.row(t)) {
        if ((int)t.size() <= maxcol) die("Error: malformed line in " + base + ".mmseq: " + table.line);
        const bool ident = isIdent.count(t[ic2]) > 0;
        if (!ident && want_all) all_features.push_back(t[ic2]);
        if (t[uc] == "0" && !ident) {
            tb.candidates.push_back(t[ic2]);
            if (t[ob2] == "0") {
                sd.push_back(INFINITY);
                tb.zeros.push_back(t[ic2]);
                tb.zero_efflen[t[ic2]] = num(t[el2]);
            } else sd.push_back(num(t[si2]));
        } else if (t[uc] == "1") {
            if (num(t[si2]) > max_h1_sd && num(t[ac2]) < IACTTHRES) max_h1_sd = num(t[si2]);
            tb.toremove.push_back(t[ic2]);
        } else tb.toremove.push_back(t[ic2]);
    }
    cerr << "SD thres=" << max_h1_sd << endl;
    for (int i = (int)tb.candidates.size() - 1; i >= 0; i--)
        if (sd[i] < max_h1_sd || isIdent.count(tb.candidates[i]) > 0) {
            tb.toremove.push_back(tb.candidates[i]);
            tb.candidates.erase(tb.candidates.begin() + i);
        }
}

struct SampleTraces {
    vector<string> ids;        // output column names: the trace file's non-identical columns, then the identical sets' columns
    vector<double> M;          // [TRACELEN][ids.size()]
    string err;
};

#define MMG_CHECK(call)                                                                                   \
    do {                                                                                                  \
        if ((call) != 0) die(string("Error: ") + #call + ": " + mmg_last_error());                       \
    } while (0)

int main(int argc, char **argv)
{
    double stoppingthreshold = 0.975;
    vector<string> basenames;
    for (int i = 1; i < argc; i++) {
        const string a = argv[i];
        if (a == "-thres" && argc > i + 1) {
            char *end = nullptr;
            stoppingthreshold = strtod(argv[i + 1], &end) / 100.0;
            if (end == argv[i + 1] || *end != 0 || !(stoppingthreshold > 0 && stoppingthreshold <= 1)) {
                printUsage(cerr);
                return 1;
            }
            i++;
        } else if (a.find("-") == 0) {
            printUsage(cerr);
            return 1;
        } else basenames.push_back(a);
    }
    if (basenames.empty()) {
        printUsage(cerr);
        return 1;
    }
    const size_t S = basenames.size();
    StageTimer timer;
    cerr << "Stopping threshold: -" << stoppingthreshold * 100 << "th percentile of the distribution of correlations\n";

    // ---- candidates (:620-686)
    vector<Tables> tabs(S);
    vector<string> all_features;
    map<string, bool> isIdent;
    vector<string> candidates, zeros, toremove;
    for (size_t s = 0; s < S; ++s) {
        cerr << basenames[s] << " ";
        read_tables(basenames[s], tabs[s], all_features, s == 0, isIdent);
        toremove.insert(toremove.end(), tabs[s].toremove.begin(), tabs[s].toremove.end());
        vector<string> c = tabs[s].candidates, z = tabs[s].zeros;
        if (s == 0) { candidates = c; zeros = z; continue; }
        sort(candidates.begin(), candidates.end()); sort(c.begin(), c.end());
        vector<string> u;
        set_union(candidates.begin(), candidates.end(), c.begin(), c.end(), back_inserter(u));
        candidates.swap(u);
        sort(zeros.begin(), zeros.end()); sort(z.begin(), z.end());
        vector<string> x;
        set_intersection(zeros.begin(), zeros.end(), z.begin(), z.end(), back_inserter(x));
        zeros.swap(x);
    }
    {
        sort(candidates.begin(), candidates.end()); sort(zeros.begin(), zeros.end());
        vector<string> d;
        set_difference(candidates.begin(), candidates.end(), zeros.begin(), zeros.end(), back_inserter(d));
        sort(toremove.begin(), toremove.end());
        toremove.erase(unique(toremove.begin(), toremove.end()), toremove.end());
        candidates.clear();
        set_difference(d.begin(), d.end(), toremove.begin(), toremove.end(), back_inserter(candidates));
    }
    const uint32_t C = (uint32_t)candidates.size();
    cerr << C << " transcripts or sets of identical transcripts are unidentifiable in all samples.\n";
    map<string, int> cand2ind;
    for (uint32_t i = 0; i < C; ++i) cand2ind[candidates[i]] = (int)i;
    vector<uint8_t> observed((size_t)C * S, 1);   // [C][S] (:688-698)
    for (size_t s = 0; s < S; ++s)
        for (auto &z : tabs[s].zeros) {
            auto it = cand2ind.find(z);
            if (it != cand2ind.end()) observed[(size_t)it->second * S + s] = 0;
        }
    // every input exists before the device is touched
    for (auto &b : basenames)
        for (const char *suf : {".trace_gibbs.gz", ".identical.trace_gibbs.gz", ".M", ".k"})
            if (!readable(b + suf)) {
                if (suf[1] == 'M' || suf[1] == 'k') die("Error reading " + b + suf + " file.");
                die("Error: couldn't open " + b + suf + ".");
            }
    timer.mark("tables");

    // ---- traces: both files of every sample, once, a thread per sample
    vector<SampleTraces> tr(S);
    {
        const unsigned nth = max(1u, min((unsigned)S, thread::hardware_concurrency()));
        vector<thread> pool;
        for (unsigned w = 0; w < nth; ++w)
            pool.emplace_back([&, w]() {
                for (size_t s = w; s < S; s += nth) {
                    SampleTraces &t = tr[s];
                    vector<string> ids1, ids2;
                    vector<double> m1, m2;
                    t.err = traceio::read_trace(basenames[s] + ".trace_gibbs.gz", TRACELEN, ids1, m1);
                    if (t.err.empty()) t.err = traceio::read_trace(basenames[s] + ".identical.trace_gibbs.gz", TRACELEN, ids2, m2);
                    if (!t.err.empty()) continue;
                    vector<size_t> keep;   // the non-identical columns of the transcript trace (:838-849)
                    for (size_t c = 0; c < ids1.size(); ++c) if (!isIdent.count(ids1[c])) keep.push_back(c);
                    const size_t w1 = ids1.size(), w2 = ids2.size(), w = keep.size() + w2;
                    t.M.assign((size_t)TRACELEN * w, 0.0);
                    for (size_t k = 0; k < (size_t)TRACELEN; ++k) {
                        double *row = &t.M[k * w];
                        for (size_t c = 0; c < keep.size(); ++c) row[c] = m1[k * w1 + keep[c]];
                        for (size_t c = 0; c < w2; ++c) row[keep.size() + c] = m2[k * w2 + c];
                    }
                    for (size_t c : keep) t.ids.push_back(ids1[c]);
                    t.ids.insert(t.ids.end(), ids2.begin(), ids2.end());
                }
            });
        for (auto &th : pool) th.join();
        for (auto &t : tr) if (!t.err.empty()) die(t.err);
    }
    timer.mark("read traces");

    int ndev = 0;
    if (mmg_device_count(&ndev) != 0 || ndev < 1) die("Error: no HIP device available: mmcollapse has no CPU fallback");

    // ---- correlations, threshold, greedy loop (:700-819)
    if (C >= 2) {
        mmg_collapse *h = nullptr;
        MMG_CHECK(mmg_collapse_create(0, (uint32_t)S, C, TRACELEN, observed.data(), &h));
        {
            vector<double> X((size_t)TRACELEN * C);
            for (size_t s = 0; s < S; ++s) {
                const SampleTraces &t = tr[s];
                const size_t w = t.ids.size();
                fill(X.begin(), X.end(), 0.0);
                for (size_t c = 0; c < w; ++c) {
                    auto it = cand2ind.find(t.ids[c]);
                    if (it == cand2ind.end()) continue;
                    for (size_t k = 0; k < (size_t)TRACELEN; ++k) X[k * C + it->second] = t.M[k * w + c];
                }
                MMG_CHECK(mmg_collapse_set_sample(h, (uint32_t)s, X.data()));
            }
        }
        MMG_CHECK(mmg_collapse_correlate(h));
        timer.mark("correlations");
        vector<double> maxcorrs(C);
        MMG_CHECK(mmg_collapse_row_max(h, maxcorrs.data()));
        sort(maxcorrs.begin(), maxcorrs.end());
        size_t at = (size_t)floor((double)C * stoppingthreshold);
        if (at > C - 1) at = C - 1;   // -thres 100 (the reference reads one past the end)
        const double thr = -maxcorrs[at];
        cerr << "Threshold for mean anti-correlation: " << thr << endl;
        vector<uint32_t> pairs(2 * 4096);
        vector<double> values(4096);
        int32_t stopped = 0;
        size_t nco = 0;
        while (!stopped) {
            uint32_t got = 0;
            MMG_CHECK(mmg_collapse_run(h, thr, 4096, pairs.data(), values.data(), &got, &stopped));
            for (uint32_t m = 0; m < got; ++m) {   // collapse()'s new name (:429-440)
                const uint32_t a = pairs[2 * m], b = pairs[2 * m + 1];
                vector<string> ts = {candidates[a], candidates[b]};
                sort(ts.begin(), ts.end());
                candidates[a] = ts[0] + "*" + ts[1];
                candidates[b] = "NA";
            }
            nco += got;
        }
        mmg_collapse_destroy(h);
        cerr << "Collapsing unidentifiable transcripts based on mean anti-correlations...done (" << nco << " iterations)." << endl;
    }
    timer.mark("greedy loop");

    // ---- per sample: traces of every feature, collapsed sets joined, summaries, unique hits, the table (:827-1107)
    vector<string> forcollapsing;
    for (auto &c : candidates) if (c.find('*') != string::npos) forcollapsing.push_back(c);
    sort(forcollapsing.begin(), forcollapsing.end());
    forcollapsing.erase(unique(forcollapsing.begin(), forcollapsing.end()), forcollapsing.end());
    for (size_t s = 0; s < S; ++s) {
        const string &base = basenames[s];
        SampleTraces &t = tr[s];
        vector<string> ids = t.ids;
        const uint32_t ncols = (uint32_t)ids.size();
        set<string> gottrace(ids.begin(), ids.end());
        vector<uint64_t> vid;
        vector<double> vscale;
        for (size_t f = 0; f < all_features.size(); ++f) {
            if (gottrace.count(all_features[f])) continue;
            auto it = tabs[s].zero_efflen.find(all_features[f]);
            if (it == tabs[s].zero_efflen.end()) die("Error: couldn't get effective length for " + all_features[f]);
            ids.push_back(all_features[f]);
            vid.push_back((uint64_t)f);
            vscale.push_back(1.0 / (BETA + it->second * (double)tabs[s].mapped / 1000000000.0));
        }
        // join_traces (:443-481): a set's members, by column position, summed into its first column
        map<string, int> tmap;
        for (size_t c = 0; c < ids.size(); ++c) tmap[ids[c]] = (int)c;
        vector<vector<uint32_t>> members(ids.size());
        vector<char> shed(ids.size(), 0);
        for (size_t c = 0; c < ids.size(); ++c) members[c] = {(uint32_t)c};
        for (auto &name : forcollapsing) {
            vector<uint32_t> idx;
            for (auto &tok : tokenise(name, "*")) {
                auto it = tmap.find(tok);
                if (it == tmap.end()) die("No trace for " + tok + " and trying to collapse.");
                idx.push_back((uint32_t)it->second);
            }
            sort(idx.begin(), idx.end());
            members[idx[0]] = idx;
            for (size_t j = 1; j < idx.size(); ++j) shed[idx[j]] = 1;
            ids[idx[0]] = name;
        }
        vector<pair<string, int>> order;
        for (size_t c = 0; c < ids.size(); ++c) if (!shed[c]) order.push_back({ids[c], (int)c});
        sort(order.begin(), order.end(), [](const pair<string, int> &l, const pair<string, int> &r) { return l.first < r.first; });
        vector<uint64_t> sptr(1, 0);
        vector<uint32_t> smem;
        for (auto &o : order) { smem.insert(smem.end(), members[o.second].begin(), members[o.second].end()); sptr.push_back(smem.size()); }
        const uint32_t ns = (uint32_t)order.size();
        vector<double> lm(ns), var(ns), tau(ns);
        vector<int32_t> rc(ns);
        MMG_CHECK(mmg_collapse_summarize(0, TRACELEN, ncols, t.M.data(), (uint32_t)vid.size(), vid.data(), vscale.data(), ALPHA, SIMU_SEED,
                                         (uint32_t)s, ns, sptr.data(), smem.data(), lm.data(), var.data(), tau.data(), rc.data()));
        vector<double>().swap(t.M);

        // unique hits of every output series (uh(), src/uh.cpp:3-26): a read counts k towards the series holding all of its hits
        ifstream ifs((base + ".M").c_str());
        string str;
        getline(ifs, str);
        if (!ifs.good() || str.empty() || str[0] != '#') die("Error reading " + base + ".M file.");
        map<string, int> feature2ind;
        {
            vector<string> tk = tokenise(str, "\t");
            for (size_t i = 1; i < tk.size(); ++i) feature2ind[tk[i]] = (int)i - 1;
        }
        vector<int> series_of(feature2ind.size(), -1);
        for (uint32_t g = 0; g < ns; ++g)
            for (auto &plus : tokenise(order[g].first, "+"))
                for (auto &x : tokenise(plus, "*")) {
                    auto it = feature2ind.find(x);
                    if (it != feature2ind.end()) series_of[it->second] = (int)g;
                }
        vector<vector<int>> rows;
        {
            long i, j, maxi = -1;
            while (ifs >> i >> j) {
                if (i < 0 || j < 0 || j >= (long)series_of.size()) die("Error reading " + base + ".M file.");
                if ((long)rows.size() <= i) rows.resize((size_t)i + 1);
                rows[(size_t)i].push_back((int)j);
                maxi = max(maxi, i);
            }
        }
        vector<long> kk;
        {
            ifstream kf((base + ".k").c_str());
            string w;
            while (kf >> w) kk.push_back(atol(w.c_str()));
        }
        if (rows.size() != kk.size()) die("Error: incompatible arguments to function uh().");
        vector<long> uh(ns, 0);
        long all_k = 0;
        for (size_t r = 0; r < rows.size(); ++r) {
            if (rows[r].empty()) { all_k += kk[r]; continue; }
            const int g = series_of[rows[r][0]];
            bool same = g >= 0;
            for (size_t q = 1; same && q < rows[r].size(); ++q) same = series_of[rows[r][q]] == g;
            if (same) uh[g] += kk[r];
        }

        ofstream ofs((base + ".collapsed.mmseq").c_str());
        if (!ofs.good()) die("Error: cannot open " + base + ".collapsed.mmseq for writing");
        ifstream mm((base + ".mmseq").c_str());
        if (!mm.good()) die("Error: cannot open " + base + ".mmseq");
        getline(mm, str);
        while (mm.good() && !str.empty() && str[0] == '#') { ofs << str << endl; getline(mm, str); }
        ofs << "feature_id\tlog_mu\tsd\tmcse\teffective_length\tiact\tunique_hits\n";
        for (uint32_t g = 0; g < ns; ++g) {
            if (!isfinite(lm[g])) die("shouldn't happen");
            const double mcse = rc[g] ? (double)TRACELEN : sqrt(tau[g] * var[g] / TRACELEN);
            const double iact = rc[g] ? NAN : tau[g];
            ofs << order[g].first << "\t" << lm[g] << "\t" << sqrt(var[g]) << "\t" << mcse << "\t" << "NA" << "\t" << iact << "\t"
                << uh[g] + all_k << "\n";
        }
        ofs.close();
        if (!ofs) die("Error: writing " + base + ".collapsed.mmseq failed");
        cerr << "\tSaving new table \"" << base << ".collapsed.mmseq\".\n";
    }
    timer.mark("output");
    timer.total();
    return 0;
}
