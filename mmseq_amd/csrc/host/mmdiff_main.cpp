// mmdiff_main.cpp -- drop-in for the reference's mmdiff (src/mmdiff.cpp): Bayesian model selection between two linear models of
// every feature's expression across samples.  Tables, normalisation, permutation and the design matrices on the host; the
// per-feature MCMC (src/bms.cpp) on the device through the C ABI (include/mmgibbs.h: mmg_diff_*).  Deliberate differences from the
// reference are listed in DESIGN.md section 10: keyed streams instead of one MT19937 per thread, a keyed shuffle for -permute,
// -traces for -tracedir (without sigar<model>.txt), size caps, dlgamma for gsl_sf_lngamma.
//
// Polytomous model selection (the reference's recipe: one mmdiff run per alternative, then polyclass() of src/R/mmseq.R) is built in:
// repeated -m runs J alternatives against one model 0 on one device handle (mmg_diff_poly_*), and -polyclass combines mmdiff tables on
// the host alone.
//
// -chains C runs C independent chains of one comparison on one device handle (mmg_diff_chains_*) and prints their pooled table:
// run_chains and DESIGN.md section 10.2.
//
// -traces DIR writes the reference's MCMC trace files (its -tracedir): TraceWriter below.
//
// -effects FILE keeps thinned sampling rows on the device and writes their per-feature summaries (mean, sd, P(> 0), percentiles of
// every parameter under its own model): write_effects below and DESIGN.md section 10.3.
//
// main() is a sequence of stages over Options, Inputs, Model and Mcmc: parse_args, check_combinations, the -polyclass shortcut,
// load_inputs, the design, then run_poly, run_chains, run_perm (all three on run_replicas) or run_plain (with run_lrt).
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <charconv>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "../../../include/mmgibbs.h"
#include "../mmg_math.h"
#include "cpu_quota.hpp"

using namespace std;

#define OUTLEN 1024
#define MAXBATCHES 8192
#define MAXMODELS 16   // alternatives (-m) in one run
#define MAXCHAINS 16   // chains (-chains) in one run
#define MAXPERMS 31    // shuffled replicas (-permutations) in one run
#define MAXLRTPERMS 65535   // shuffled copies of the likelihood-ratio test (-lrtperm)

namespace {

typedef vector<double> Mat;   // row-major, with the shape carried alongside

[[noreturn]] void die(const string &msg)
{
    cerr << msg << endl;
    exit(1);
}

void tokenise(const string &str, vector<string> &tokens, const string &delimiters = " ")
{
    string::size_type lastPos = str.find_first_not_of(delimiters, 0);
    string::size_type pos = str.find_first_of(delimiters, lastPos);
    while (string::npos != pos || string::npos != lastPos) {
        tokens.push_back(str.substr(lastPos, pos - lastPos));
        lastPos = str.find_first_not_of(delimiters, pos);
        pos = str.find_first_of(delimiters, lastPos);
    }
}

bool endsWith(const string &a, const string &b)
{
    if (b.size() > a.size()) return false;
    return std::equal(a.begin() + a.size() - b.size(), a.end(), b.begin());
}

// ostream's default formatting of a double (%g, 6 digits); NaN prints as x86-64's 0.0 / 0.0 does in the reference
string fmt(double x)
{
    if (std::isnan(x)) return std::signbit(x) ? "-nan" : "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%g", x);
    return buf;
}

void printUsage(ostream &out)
{
    out << "Usage: mmdiff [OPTIONS...] [-de n1 n2 ... nC | -m matrices_file] mmseq_file1 mmseq_file2... > out.mmdiff" << endl
        << "       matrices_file contains M P0 P1 each separated by an empty line" << endl
        << "       mmdiff [OPTIONS...] [-prior P0,...,PJ] [-polyout BASE] -m alt1 -m alt2 [-m ...] mmseq_file1 mmseq_file2... > out.polyclass" << endl
        << "       mmdiff -polyclass [-prior P0,...,PJ] a.mmdiff b.mmdiff [...] > out.polyclass" << endl
        << "       mmdiff [OPTIONS...] -chains C [-chainout BASE] [-de n1 n2 ... nC | -m matrices_file] mmseq_file1 mmseq_file2... > out.mmdiff" << endl
        << "       mmdiff [OPTIONS...] -permutations B [-permout BASE] [-de n1 n2 ... nC | -m matrices_file] mmseq_file1 mmseq_file2... > out.mmdiff" << endl
        << endl;
    out << "Mandatory arguments:" << endl
        << "  ONE OF:" << endl
        << "  -de INT INT...    simple differential expression between several groups of samples, where" << endl
        << "                    each INT corresponds to a grouping of MMSEQ files into one condition" << endl
        << "  -m STRING         path to matrices file specifying the two models to compare; repeated (-m A -m B ...): one run of" << endl
        << "                    every alternative against the same model 0, posterior model probabilities on stdout" << endl
        << "  -polyclass        no MCMC: combine the mmdiff tables of J >= 2 alternatives against the same model 0 into" << endl
        << "                    posterior probabilities of models 0..J" << endl;
    out << "Optional arguments:" << endl
        << "  -tracedir STRING  not implemented in this version: MCMC traces are not written (exits with an error); use -traces" << endl
        << "  -traces STRING    directory in which to save MCMC traces, as the reference's -tracedir writes them: <param>-burnin and" << endl
        << "                    <param> (1024 lines each, one value per feature), logitp, meanLO, pseudo; sigar<model>.txt is not" << endl
        << "                    written; not with -chains or repeated -m (default: \"\" (do not write traces))" << endl
        << "  -effects STRING   file for the effects: per feature n0, n1 (the kept sampling rows under each model) and, for every parameter" << endl
        << "                    its model has, <name>_mean, <name>_sd, <name>_p_gt0 and <name>_q<p> per percentile, over the rows" << endl
        << "                    whose own gamma is the parameter's model; the rows stay on the device (8 bytes x rows x parameters" << endl
        << "                    x features); not with -traces, -chains, repeated -m or -polyclass (default: \"\" (no effects))" << endl
        << "  -effects_every INT  with -effects: keep every INT-th sampling iteration; iter / INT rows, rounded up, at most 4096" << endl
        << "                    (default: max(1, iter / 1024))" << endl
        << "  -effects_percentiles P1,P2,...  with -effects: up to 32 percentiles in [0, 100] (default: 2.5,50,97.5)" << endl
        << "  -useprops         run on isoform/gene proportions instead of expression" << endl
        << "  -permute          run on permuted dataset (a keyed shuffle per feature); combine with non-permuted results to obtain q-values" << endl
        << "  -p FLOAT          prior probability of the second model (default: 0.1)" << endl
        << "  -d FLOAT          d hyperparameter (default: 1.4)" << endl
        << "  -s FLOAT          s hyperparameter (default: 2.0)" << endl
        << "  -l INT            length of MCMC trace used to produce the input estimates (default: 1024)" << endl
        << "  -fixalpha         fix alpha=0 and do not update (default: estimate alpha)" << endl
        << "  -nonorm           do not normalise the input data" << endl
        << "  -pdash FLOAT      initial value of pdash for improved mixing of gamma (stays fixed if -notune is set) (default: 0.5)" << endl
        << "  -notune           do not tune pdash to improve mixing for gamma" << endl
        << "  -uhfrac FLOAT     if normalising, use features which have at least one unique hit" << endl
        << "                    in at least uhfrac of the samples (default: max(0.2, (N - floor(N^2/160))/N))" << endl
        << "  -burnin INT       burnin iterations (default: 8192)" << endl
        << "  -iter INT         MCMC iterations (default: 16384)" << endl
        << "  -seed INT         seed for PRNG (default: 1234)" << endl
        << "  -range INT INT    select features indexed within range (default: all)" << endl
        << "  -prior P0,...,PJ  with repeated -m or -polyclass: prior probabilities of models 0..J, adding up to 1 (default: flat)" << endl
        << "  -polyout STRING   with repeated -m: write the mmdiff table of alternative j to STRING.model<j>.mmdiff" << endl
        << "  -chains INT       run INT (1 to 16) independent chains, seeded (seed, chain), and print their pooled table: the Bayes factor" << endl
        << "                    from all chains and the columns log_bf, log_bf_sd, log_bf_mcse, chains_mixed appended (default: 1, the" << endl
        << "                    plain table); not with repeated -m or -polyclass (chains of several alternatives are left for later)" << endl
        << "  -chainout STRING  with -chains: write the mmdiff table of chain c to STRING.chain<c>.mmdiff" << endl
        << "  -permutations INT run the data and INT (1 to 31) copies of it whose samples are shuffled per feature (as -permute shuffles" << endl
        << "                    them, copy b with the seed seed ^ (b << 32)) in one run, and append to the plain table perm_ge (the" << endl
        << "                    shuffled log Bayes factors, over all copies and features, not below the feature's own) and q_value (the" << endl
        << "                    smallest estimated false discovery rate at which the feature is called); not with -permute, -chains," << endl
        << "                    repeated -m, -traces, -effects or -polyclass.  A shuffle only relabels samples: with few samples many" << endl
        << "                    shuffles reproduce the original grouping (a third of them for 2 vs 2), and the q-values are conservative" << endl
        << "  -permout STRING   with -permutations: write the mmdiff table of shuffled copy b to STRING.perm<b>.mmdiff" << endl
        << "  -lrt STRING       file for the per-feature likelihood-ratio test of the two models (maximum likelihood, no priors, no MCMC):" << endl
        << "                    loglik0, loglik1, lrt_stat, df, p_value (chi-squared with df degrees of freedom), q_value (Benjamini-" << endl
        << "                    Hochberg), the estimates alpha, beta, eta, sigmasq of both models (NA for a term a model lacks), iters and" << endl
        << "                    status per model (bits: 1 iteration cap reached, 2 singular design or weights: NaN, 4 some sigmasq is 0);" << endl
        << "                    stdout is what it is without the flag; not with -chains, repeated -m, -permutations or -polyclass" << endl
        << "  -lrtonly          with -lrt: skip the MCMC and leave stdout empty" << endl
        << "  -lrtperm INT      with -lrt: repeat the test on INT (1 to 65535, INT x features at most 2147483647) copies of the data whose" << endl
        << "                    samples are shuffled per feature (copy b as -permutations shuffles its copy b) and append to the file" << endl
        << "                    perm_ge (the feature's own shuffled lrt_stat not below its lrt_stat), perm_p ((1 + perm_ge) / (1 + the" << endl
        << "                    copies whose lrt_stat is not NaN)), null_ge (the shuffled lrt_stat of all copies and features not below it)" << endl
        << "                    and q_perm (as -permutations forms q_value); not with -permute.  With few samples many shuffles" << endl
        << "                    reproduce the original grouping, and this null is conservative too" << endl
        << "Size limits: 512 samples, 8 columns of M, 16 columns of P0 and P1, 16 variance classes per model, 16 alternatives (-m) per run, 16 chains. At most 31 permutations." << endl;
}

[[noreturn]] void usage_error(const string &msg)
{
    cerr << msg << endl;
    printUsage(cerr);
    exit(1);
}

// src/mmdiff.cpp parse_mmseq: y, e, uh as [feature][sample]
void parse_mmseq(const vector<string> &filenames, vector<string> &features, Mat &y, Mat &e, Mat &uh, int range_start, int range_end,
                 bool useprops)
{
    const size_t S = filenames.size();
    vector<vector<double>> cy(S), ce(S), cu(S);
    cerr << "Parsing ";
    for (size_t i = 0; i < S; ++i) {
        cerr << filenames[i] << " ";
        ifstream ifs(filenames[i].c_str());
        if (!ifs.good()) die("\nError: couldn't open " + filenames[i]);
        string str;
        getline(ifs, str);
        while (!ifs.eof() && !str.empty() && str[0] == '#') getline(ifs, str);
        vector<string> tokens;
        tokenise(str, tokens, "\t");
        int feature_ind = -1, lmg_ind = -1, sd_ind = -1, mp_ind = -1, sp_ind = -1, uh_ind = -1;
        for (int j = 0; j < (int)tokens.size(); ++j) {
            if (tokens[j] == "feature_id") feature_ind = j;
            if (tokens[j] == "log_mu") lmg_ind = j;
            if (tokens[j] == "sd") sd_ind = j;
            if (tokens[j] == "mean_probit_proportion") mp_ind = j;
            if (tokens[j] == "sd_probit_proportion") sp_ind = j;
            if (tokens[j] == "unique_hits") uh_ind = j;
        }
        if (useprops) {
            if ((feature_ind + 1) * (mp_ind + 1) * (sp_ind + 1) * (uh_ind + 1) == 0)
                die("\nError: input tables must have feature_id, mean_probit_proportion, sd_probit_proportion and unique_hits columns.");
        } else {
            if ((feature_ind + 1) * (lmg_ind + 1) * (sd_ind + 1) * (uh_ind + 1) == 0)
                die("\nError: input tables must have feature_id, log_mu, sd and unique_hits columns.");
        }
        const int yi = useprops ? mp_ind : lmg_ind, ei = useprops ? sp_ind : sd_ind;
        const int need = max(max(feature_ind, yi), max(ei, uh_ind));
        size_t k = 0;
        while (true) {
            getline(ifs, str);
            if (ifs.eof()) break;
            tokens.clear();
            tokenise(str, tokens, "\t");
            if ((int)tokens.size() <= need) die("\nError: line " + to_string(k + 2) + " of " + filenames[i] + " has too few columns.");
            if (k + 1 > features.size()) {
                if (i > 0) die("\nError: features across files do not match (" + to_string(k) + "," + tokens[feature_ind] + ",)");
                features.push_back(tokens[feature_ind]);
            } else if (features[k] != tokens[feature_ind]) {
                die("\nError: features across files do not match (" + to_string(k) + "," + tokens[feature_ind] + "," + features[k] + ")");
            }
            if (tokens[yi] == "NA") die("\nError: encountered NA");
            cy[i].push_back(atof(tokens[yi].c_str()));
            ce[i].push_back(atof(tokens[ei].c_str()));
            cu[i].push_back(atof(tokens[uh_ind].c_str()));
            ++k;
        }
        if (k != features.size())
            die("\nError: features across files do not match (" + to_string(k) + ",," + (k < features.size() ? features[k] : string()) + ")");
    }
    size_t lo = 0, hi = features.size();   // [lo, hi)
    if (range_start >= 0 && range_end > range_start && (size_t)range_end < features.size()) { lo = range_start; hi = (size_t)range_end + 1; }
    vector<string> kept;
    y.clear(); e.clear(); uh.clear();
    for (size_t f = lo; f < hi; ++f) {
        if (useprops && std::isinf(cy[0][f])) continue;   // single-isoform genes: infinite probit proportions
        kept.push_back(features[f]);
        for (size_t i = 0; i < S; ++i) { y.push_back(cy[i][f]); e.push_back(ce[i][f]); uh.push_back(cu[i][f]); }
    }
    features = kept;
    // the device samplers need finite estimates: "nan" and "inf" entries (atof accepts them) are errors, as "NA" is
    for (size_t f = 0; f < features.size(); ++f)
        for (size_t i = 0; i < S; ++i)
            if (!std::isfinite(y[f * S + i]) || !std::isfinite(e[f * S + i]))
                die("\nError: encountered a non-finite value (feature " + features[f] + " in " + filenames[i] + ")");
    if (useprops) cerr << endl << "Kept " << features.size() << " transcripts belonging to multi-isoform genes";
    else cerr << endl << "Analysing " << features.size() << " features";
    cerr << endl;
}

// DESeq style: y[,i] <- y[,i] - median(y[,i] - rowMeans(y)) over the features with unique hits in at least uhfrac of the samples
void apply_normalisation(const vector<string> &filenames, Mat &y, const Mat &uh, size_t F, size_t S, double uhfrac)
{
    vector<size_t> use;
    for (size_t i = 0; i < F; ++i) {
        int sum = 0;
        for (size_t j = 0; j < S; ++j)
            if (uh[i * S + j] > 0) sum++;
        if ((double)sum / (double)S >= uhfrac) use.push_back(i);
    }
    if (use.size() < 100) {
        cerr << "Warning: fewer than 100 features found for normalisation. Skipping.\n";
        return;
    }
    cerr << "Using " << use.size() << "/" << F << " features for normalisation.\n";
    vector<double> rowMeans;
    for (size_t i = 0; i < use.size(); ++i) {
        double sum = 0;
        for (size_t j = 0; j < S; ++j) sum += y[use[i] * S + j];
        rowMeans.push_back(sum / (double)S);
    }
    cerr << "Log scale normalisation factors:\n";
    for (size_t sample = 0; sample < S; ++sample) {
        vector<double> ydiff;
        for (size_t i = 0; i < use.size(); ++i) ydiff.push_back(y[use[i] * S + sample] - rowMeans[i]);
        sort(ydiff.begin(), ydiff.end());
        const double m = ydiff[ydiff.size() / 2];
        cerr << "\t" << filenames[sample] << "\t" << m << endl;
        for (size_t i = 0; i < F; ++i) y[i * S + sample] = y[i * S + sample] - m;
    }
}

// -permute: a Fisher-Yates shuffle of each feature's samples, keyed (seed, 0, TAG_DIFF_PERM, feature, 0) -- the same for every
// thread count and machine (the reference calls random_shuffle)
void apply_permutation(Mat &y, Mat &e, size_t F, size_t S, uint64_t seed, bool quiet = false)
{
    if (!quiet) cerr << "Permuting input data...";
    vector<size_t> idx(S);
    vector<double> ny(S), ne(S);
    for (size_t f = 0; f < F; ++f) {
        for (size_t j = 0; j < S; ++j) idx[j] = j;
        mmg::SeqStream q(mmg::Stream(seed, 0, mmg::TAG_DIFF_PERM, f, 0));
        for (size_t j = S - 1; j > 0; --j) {
            size_t k = (size_t)(q.next() * (double)(j + 1));
            if (k > j) k = j;
            swap(idx[j], idx[k]);
        }
        for (size_t j = 0; j < S; ++j) { ny[j] = y[f * S + idx[j]]; ne[j] = e[f * S + idx[j]]; }
        for (size_t j = 0; j < S; ++j) { y[f * S + j] = ny[j]; e[f * S + j] = ne[j]; }
    }
    if (!quiet) cerr << "done\n";
}

struct Design {
    size_t N = 0, K = 0, L0 = 0, L1 = 0, CC = 0;
    Mat M, P0, P1;
    vector<int> C;   // [N][CC]
};

void resize_cols(Mat &X, size_t N, size_t &cols, size_t ncols)
{
    if (ncols == cols) return;
    Mat Y(N * ncols, 0.0);
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < min(cols, ncols); ++j) Y[i * ncols + j] = X[i * cols + j];
    X.swap(Y);
    cols = ncols;
}

// src/mmdiff.cpp parse_matrices: blocks M, C, P0, P1 separated by empty lines; "#" starts a comment; P rows are per class
void parse_matrices(const string &file, Design &D, size_t nrows)
{
    ifstream ifs(file.c_str());
    if (!ifs.good()) die("Error: couldn't open " + file);
    D.N = nrows;
    vector<double> Cd;
    string str;
    vector<string> tokens;
    int m = -1;
    size_t i = 0;
    int P0reducedcols = 0, P1reducedcols = 0;
    auto maxC = [&](int col) { int r = INT32_MIN; for (size_t j = 0; j < nrows; ++j) r = max(r, D.C[j * D.CC + col]); return r; };
    while (true) {
        bool spacer = false;
        do {
            if (!ifs.eof()) getline(ifs, str);
            else str = "";
            str = str.substr(0, str.find_first_of("#"));
            tokens.clear();
            tokenise(str, tokens, " \t");
            if (tokens.size() < 1) spacer = true;
        } while (!ifs.eof() && tokens.size() < 1);
        if (str.size() == 0 && ifs.eof()) break;
        if (spacer) { m++; i = 0; }
        if (m == -1) m = 0;
        if (m > 3) die("Error: more than four matrices in " + file + ".");
        if (m == 0) resize_cols(D.M, nrows, D.K, tokens.size());
        if (m == 1) {
            if (D.C.size() != nrows * tokens.size()) {
                vector<int> nc(nrows * tokens.size(), 0);
                for (size_t r = 0; r < nrows; ++r)
                    for (size_t c = 0; c < min(D.CC, tokens.size()); ++c) nc[r * tokens.size() + c] = D.C[r * D.CC + c];
                D.C.swap(nc);
                D.CC = tokens.size();
            }
        }
        if (m == 2) resize_cols(D.P0, nrows, D.L0, tokens.size());
        if (m == 3) resize_cols(D.P1, nrows, D.L1, tokens.size());
        if (i >= nrows) die("Error: number of rows of matrices greater than number of samples.");
        if ((m == 2 || m == 3) && D.CC < 2) die("Error: the class matrix (the second block) must have two columns.");
        for (size_t t = 0; t < tokens.size(); ++t) {
            if (m == 0) D.M[i * D.K + t] = atof(tokens[t].c_str());
            if (m == 1) D.C[i * D.CC + t] = atoi(tokens[t].c_str());
            if (m == 2 || m == 3) {
                const int col = m - 2;
                const int mc = maxC(col);
                if ((int)i > mc)
                    die("Error: more distinct rows of P than classes for model " + to_string(col) + " (" + to_string(i) + " > " + to_string(mc) + ").");
                Mat &P = col ? D.P1 : D.P0;
                const size_t L = col ? D.L1 : D.L0;
                for (size_t j = 0; j < nrows; ++j)
                    if (D.C[j * D.CC + col] == (int)i) P[j * L + t] = atof(tokens[t].c_str());
                int &red = col ? P1reducedcols : P0reducedcols;
                red = max(red, (int)i);
            }
        }
        i++;
    }
    if (D.K == 0 || D.CC == 0 || D.L0 == 0 || D.L1 == 0) die("Error: Rows in M, P0, P1 and number of mmseq files must match.");
    if (D.CC != 2) die("Error: the class matrix (the second block) must have two columns.");
    int cmin = INT32_MAX;
    for (int c : D.C) cmin = min(cmin, c);
    if (cmin != 0) die("Error: need at least one class in each model labelled 0.");
    if (maxC(0) != P0reducedcols) die("Error: number of classes does not correspond to number of disinct rows of P for model 0.");
    if (maxC(1) != P1reducedcols) die("Error: number of classes does not correspond to number of disinct rows of P for  model 1.");
}

// det(Z'Z) == 0 by Gaussian elimination with partial pivoting (what the reference's det() decides for exactly singular products)
bool singular_gram(const Mat &Z, size_t N, size_t cols)
{
    if (cols == 0) return false;
    vector<double> G(cols * cols, 0.0);
    for (size_t a = 0; a < cols; ++a)
        for (size_t b = 0; b < cols; ++b)
            for (size_t i = 0; i < N; ++i) G[a * cols + b] += Z[i * cols + a] * Z[i * cols + b];
    for (size_t c = 0; c < cols; ++c) {
        size_t piv = c;
        for (size_t r = c + 1; r < cols; ++r)
            if (fabs(G[r * cols + c]) > fabs(G[piv * cols + c])) piv = r;
        if (G[piv * cols + c] == 0.0) return true;
        for (size_t k = 0; k < cols; ++k) swap(G[c * cols + k], G[piv * cols + k]);
        for (size_t r = c + 1; r < cols; ++r) {
            const double fct = G[r * cols + c] / G[c * cols + c];
            for (size_t k = c; k < cols; ++k) G[r * cols + k] -= fct * G[c * cols + k];
        }
    }
    return false;
}

bool is_nil(const Mat &X, size_t N, size_t cols)
{
    if (cols != 1) return false;
    const double lo = *min_element(X.begin(), X.end()), hi = *max_element(X.begin(), X.end());
    return hi - lo < 0.00001;
}

void append_cols(Mat &Z, size_t N, size_t &zc, const Mat &X, size_t xc)
{
    Mat Y(N * (zc + xc));
    for (size_t i = 0; i < N; ++i) {
        for (size_t j = 0; j < zc; ++j) Y[i * (zc + xc) + j] = Z[i * zc + j];
        for (size_t j = 0; j < xc; ++j) Y[i * (zc + xc) + zc + j] = X[i * xc + j];
    }
    Z.swap(Y);
    zc += xc;
}

void check_design(const Design &D, bool fixalpha, bool Mnil, const bool Pnil[2])
{
    for (int model = 0; model < 2; ++model) {
        cerr << "Design matrix for model " << model << " ([";
        if (!fixalpha) cerr << "1";
        if (!fixalpha && (!Mnil || !Pnil[model])) cerr << "|";
        if (!Mnil) cerr << "M";
        if (!Pnil[model] && (!fixalpha || !Mnil)) cerr << "|";
        if (!Pnil[model]) cerr << "P0";
        cerr << "]):\n";
        size_t zc = fixalpha ? 0 : 1;
        Mat Z(D.N * zc, 1.0);
        if (!Mnil) append_cols(Z, D.N, zc, D.M, D.K);
        if (singular_gram(Z, D.N, zc)) die("Error: collinearity in combined matrix of intercept and covariates for model " + to_string(model));
        const Mat &P = model ? D.P1 : D.P0;
        const size_t L = model ? D.L1 : D.L0;
        if (!Pnil[model]) {
            append_cols(Z, D.N, zc, P, L);
            if (singular_gram(P, D.N, L)) die("Error: collinearity in matrix P" + to_string(model));
        }
        for (size_t i = 0; i < D.N; ++i) {
            for (size_t j = 0; j < zc; ++j) {
                char buf[32];
                snprintf(buf, sizeof buf, "%10.4f", Z[i * zc + j]);
                cerr << buf;
            }
            cerr << "\n";
        }
        if (singular_gram(Z, D.N, zc)) cerr << "Warning: collinearity in full matrix of predictors for model " << model << endl;
    }
}

// the size caps, class labels and finiteness of one design, then check_design's collinearity tests; what is nil
void validate_design(const Design &D, size_t S, bool fixalpha, bool &Mnil, bool Pnil[2])
{
    if (D.K > 8) die("Error: this mmdiff handles at most 8 columns in M.");
    if (D.L0 > 16 || D.L1 > 16) die("Error: this mmdiff handles at most 16 columns in P0 and P1.");
    for (int c : D.C)
        if (c > 15) die("Error: this mmdiff handles at most 16 variance classes per model.");
    for (int model = 0; model < 2; ++model) {
        vector<int> seen(16, 0);
        int mx = 0;
        for (size_t i = 0; i < S; ++i) { seen[D.C[i * 2 + model]] = 1; mx = max(mx, D.C[i * 2 + model]); }
        for (int c = 0; c <= mx; ++c)
            if (!seen[c]) die("Error: the classes of model " + to_string(model) + " must be labelled 0, 1, ... without gaps.");
    }
    for (const Mat *X : {&D.M, &D.P0, &D.P1})
        for (double v : *X)
            if (!std::isfinite(v)) die("Error: non-finite value in the design matrices.");
    Mnil = is_nil(D.M, S, D.K);
    Pnil[0] = is_nil(D.P0, S, D.L0);
    Pnil[1] = is_nil(D.P1, S, D.L1);
    check_design(D, fixalpha, Mnil, Pnil);
    if (Mnil) cerr << "Note: no betas\n";
    if (Pnil[0]) cerr << "Note: no etas in model 0\n";
    if (Pnil[1]) cerr << "Note: no etas in model 1\n";
}

// ---- what the stages of a run hand on ---------------------------------------------------------------------------------------------
// the input tables: y and e as [feature][sample], normalised and permuted as the options ask
struct Inputs {
    vector<string> features, filenames;
    Mat y, e;
};

// a validated comparison: the design and what of it is nil
struct Model {
    Design D;
    bool Mnil = false, Pnil[2] = {false, false};
};

// -p, -d, -s, -pdash, -fixalpha, -notune, -burnin, -iter, -seed
struct Mcmc {
    double p = 0.1, d = 1.4, s = 2.0, pdash = 0.5;
    bool fixalpha = false, tune = true;
    int burnin = 8192, iters = 16384;
    uint64_t seed = 1234;
};

struct DiffResults {
    vector<double> gm, logitp, alpha, beta, eta;
    DiffResults(size_t F, const Design &D) : gm(F), logitp(F), alpha(2 * F), beta(2 * D.K * F), eta((D.L0 + D.L1) * F) {}
};

// what the pooled table of several chains has besides a chain's: the logarithm of its Bayes factor and three more columns, [F] each
struct PooledCols {
    vector<double> log_bf, log_bf_sd, log_bf_mcse;
    vector<uint32_t> chains_mixed;
    PooledCols(size_t F) : log_bf(F), log_bf_sd(F), log_bf_mcse(F), chains_mixed(F) {}
};

// what the table of a -permutations run has besides the plain one's: the null statistics not below the feature's own and its q-value
struct PermCols {
    vector<uint64_t> null_ge;
    vector<double> q;
    PermCols(size_t F) : null_ge(F), q(F) {}
};

// what a table has besides the plain one's columns.  warn_stuck: off for the tables of a run of several chains, which reports mixing per
// feature itself.
struct TableExtras {
    bool warn_stuck = true;
    const PooledCols *pool = nullptr;
    const PermCols *perm = nullptr;
};

// The table of one comparison: to fp (if any) and appended to *keep (if any).  The Bayes factor is the chain's own, with the warning for
// a gamma that did not mix -- or, with x.pool (the pooled table of several chains: its columns are appended), exp(log_bf).  With x.perm
// its two columns are appended.
void write_table(FILE *fp, string *keep, const Inputs &in, const Model &model, const Mcmc &mc, const DiffResults &r, const TableExtras &x = {})
{
    const vector<string> &features = in.features, &filenames = in.filenames;
    const Mat &y = in.y, &e = in.e;
    const Design &D = model.D;
    const bool fixalpha = mc.fixalpha, Mnil = model.Mnil, *Pnil = model.Pnil, warn_stuck = x.warn_stuck;
    const double p = mc.p;
    const PooledCols *pool = x.pool;
    const PermCols *perm = x.perm;
    const size_t F = features.size(), S = filenames.size();
    const vector<double> &gm = r.gm, &logitp = r.logitp, &alpha = r.alpha, &beta = r.beta, &eta = r.eta;
    auto emit = [&](const string &t) {
        if (fp) fputs(t.c_str(), fp);
        if (keep) *keep += t;
    };
    string out;
    out += "#prior_probability=" + fmt(p) + "\n";
    out += "feature_id\tbayes_factor\tposterior_probability\t";
    for (int model = 0; model < 2; model++) {
        if (!fixalpha) out += "alpha" + to_string(model) + "\t";
        if (!Mnil)
            for (size_t l = 0; l < D.K; l++) out += "beta" + to_string(model) + "_" + to_string(l) + "\t";
        if (!Pnil[model])
            for (size_t l = 0; l < (model ? D.L1 : D.L0); l++) out += "eta" + to_string(model) + "_" + to_string(l) + "\t";
    }
    vector<string> samplenames = filenames;
    for (size_t f = 0; f < S; f++) {
        if (endsWith(filenames[f], ".mmseq")) {
            const size_t found = filenames[f].find_last_of(".");
            size_t found2 = filenames[f].find_last_of("/");
            const long f2 = found2 == string::npos ? -1 : (long)found2;
            samplenames[f] = filenames[f].substr((size_t)(f2 + 1), (size_t)((long)found - f2 - 1));
        }
        out += "mu_" + samplenames[f] + "\t";
    }
    for (size_t f = 0; f < S; f++) out += "sd_" + samplenames[f] + (f < S - 1 ? "\t" : "");
    if (pool) out += "\tlog_bf\tlog_bf_sd\tlog_bf_mcse\tchains_mixed";
    if (perm) out += "\tperm_ge\tq_value";
    out += "\n";
    emit(out);
    const double logp = log(p), log1mp = log1p(-p);
    for (size_t feature = 0; feature < F; feature++) {
        out.clear();
        const double g = gm[feature];
        if (warn_stuck && (g == 0.0 || g == 1.0))
            cerr << "Warning: gamma did not mix for feature " << feature << "; stuck in model " << (int)g << endl;
        const double lgp = logitp[feature];
        const double pp_ = lgp > 0 ? 1.0 / (1.0 + exp(-lgp)) : exp(lgp) / (1.0 + exp(lgp));   // BMS::getp
        double BF = g / (1.0 - g) * (1.0 - pp_) / pp_;
        if (pool) {
            const double b = pool->log_bf[feature];
            BF = std::isnan(b) ? b : (std::isinf(b) ? (b < 0 ? 0.0 : b) : mmg::dexp(b));
        }
        const double postlogodds = log(BF) + logp - log1mp;
        double pp = 1.0 / (1.0 + exp(-postlogodds));
        if (BF >= DBL_MAX) pp = 1.0;
        out += features[feature] + "\t" + fmt(BF) + "\t" + fmt(pp) + "\t";
        for (int model = 0; model < 2; model++) {
            if (!fixalpha) out += fmt(alpha[model * F + feature]) + "\t";
            if (!Mnil)
                for (size_t l = 0; l < D.K; l++) out += fmt(beta[(model * D.K + l) * F + feature]) + "\t";
            if (!Pnil[model])
                for (size_t l = 0; l < (model ? D.L1 : D.L0); l++) out += fmt(eta[((model ? D.L0 : 0) + l) * F + feature]) + "\t";
        }
        for (size_t f = 0; f < S; f++) out += fmt(y[feature * S + f]) + "\t";
        for (size_t f = 0; f < S; f++) out += fmt(e[feature * S + f]) + (f < S - 1 ? "\t" : "");
        if (pool)
            out += "\t" + fmt(pool->log_bf[feature]) + "\t" + fmt(pool->log_bf_sd[feature]) + "\t" + fmt(pool->log_bf_mcse[feature]) + "\t"
                   + to_string(pool->chains_mixed[feature]);
        if (perm) out += "\t" + to_string(perm->null_ge[feature]) + "\t" + fmt(perm->q[feature]);
        out += "\n";
        emit(out);
    }
}

// ---- polytomous model selection: polyclass() of the reference's src/R/mmseq.R on mmdiff tables ----------------------------------

// what polyclass needs of one mmdiff table: the features, the Bayes factors as their text parses (strtod), and -- of the first table --
// the mu_* and sd_* columns as text
struct PolyTable {
    vector<string> kept_names, features, kept_cells;   // kept_cells[row]: the kept columns joined by tabs
    vector<double> bf;
};

void split_tabs(const string &line, vector<string> &cells)
{
    cells.clear();
    size_t a = 0;
    while (true) {
        const size_t b = line.find('\t', a);
        cells.push_back(line.substr(a, b == string::npos ? string::npos : b - a));
        if (b == string::npos) break;
        a = b + 1;
    }
}

void parse_poly_table(istream &in, const string &name, bool keep_cells, PolyTable &T)
{
    string line;
    vector<string> cells;
    bool header = false;
    int fi = -1, bi = -1;
    vector<int> kept;
    size_t lineno = 0;
    while (getline(in, line)) {
        ++lineno;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        split_tabs(line, cells);
        if (!header) {
            header = true;
            for (int j = 0; j < (int)cells.size(); ++j) {
                if (cells[j] == "feature_id") fi = j;
                if (cells[j] == "bayes_factor") bi = j;
                if (keep_cells && (cells[j].compare(0, 3, "mu_") == 0 || cells[j].compare(0, 3, "sd_") == 0)) {
                    kept.push_back(j);
                    T.kept_names.push_back(cells[j]);
                }
            }
            if (fi < 0 || bi < 0) die("Error: " + name + " must have feature_id and bayes_factor columns.");
            continue;
        }
        const int needed = max(max(fi, bi), kept.empty() ? 0 : kept.back());
        if ((int)cells.size() <= needed) die("Error: line " + to_string(lineno) + " of " + name + " has too few columns.");
        T.features.push_back(cells[fi]);
        T.bf.push_back(strtod(cells[bi].c_str(), NULL));
        if (keep_cells) {
            string row;
            for (size_t k = 0; k < kept.size(); ++k) row += (k ? "\t" : "") + cells[kept[k]];
            T.kept_cells.push_back(row);
        }
    }
    if (!header) die("Error: " + name + " must have feature_id and bayes_factor columns.");
}

void check_same_features(const PolyTable &A, const string &a, const PolyTable &B, const string &b)
{
    if (A.features.size() != B.features.size())
        die("Error: features across tables do not match (" + to_string(A.features.size()) + " in " + a + ", " + to_string(B.features.size()) + " in " + b + ")");
    for (size_t i = 0; i < A.features.size(); ++i)
        if (A.features[i] != B.features[i])
            die("Error: features across tables do not match (" + to_string(i) + "," + B.features[i] + "," + A.features[i] + ")");
}

// a comma-separated list (-prior, -effects_percentiles): every item all of a finite number in [lo, hi], or die(msg)
vector<double> parse_list(const string &text, double lo, double hi, const string &msg)
{
    vector<double> list;
    size_t a = 0;
    while (true) {
        const size_t b = text.find(',', a);
        const string tok = text.substr(a, b == string::npos ? string::npos : b - a);
        char *end = NULL;
        const double v = strtod(tok.c_str(), &end);
        if (tok.empty() || *end != '\0' || !std::isfinite(v) || v < lo || v > hi) die(msg);
        list.push_back(v);
        if (b == string::npos) break;
        a = b + 1;
    }
    return list;
}

// -prior: n finite values in [0, 1] adding up to 1 within 1.5e-8 (R's all.equal); without it the flat prior and R's warning
vector<double> parse_prior(bool given, const string &text, size_t n)
{
    if (!given) {
        cerr << "Warning: assuming flat prior across models" << endl;
        return vector<double>(n, 1.0 / (double)n);
    }
    const string msg = "Error: -prior must list " + to_string(n) + " prior probabilities (one per model, model 0 first) in [0, 1] adding up to 1.";
    const vector<double> prior = parse_list(text, 0, 1, msg);
    double sum = 0;
    for (double v : prior) sum += v;
    if (prior.size() != n || !(fabs(sum - 1.0) <= 1.5e-8)) die(msg);
    return prior;
}

// Posterior model probabilities: model 0 has Bayes factor 1, model j table j's; w_j = bf_j * prior_j, postprob_j = w_j / sum(w), the
// sum in index order.  Where that is undefined (deliberate differences from polyclass()): one infinite Bayes factor
// -- that model 1, the others 0; several -- those NaN, the others 0; a NaN Bayes factor or a zero sum -- the whole row NaN.
void polyclass(const vector<PolyTable> &T, const vector<double> &prior, FILE *fp)
{
    const size_t J = T.size(), n = J + 1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    string out = "#prior_probabilities=";
    for (size_t j = 0; j < n; ++j) out += (j ? "," : "") + fmt(prior[j]);
    out += "\nfeature_id";
    for (const string &c : T[0].kept_names) out += "\t" + c;
    for (size_t j = 0; j < n; ++j) out += "\tpostprob_model" + to_string(j);
    out += "\n";
    fputs(out.c_str(), fp);
    vector<double> bf(n), post(n);
    for (size_t i = 0; i < T[0].features.size(); ++i) {
        bf[0] = 1.0;
        for (size_t j = 0; j < J; ++j) bf[j + 1] = T[j].bf[i];
        size_t ninf = 0, nnan = 0;
        for (double v : bf) { ninf += std::isinf(v) ? 1 : 0; nnan += std::isnan(v) ? 1 : 0; }
        if (nnan) {
            cerr << "Warning: NaN Bayes factor for feature " << i << " (" << T[0].features[i] << "): posterior probabilities undefined" << endl;
            post.assign(n, nan);
        } else if (ninf == 1) {
            for (size_t j = 0; j < n; ++j) post[j] = std::isinf(bf[j]) ? 1.0 : 0.0;
        } else if (ninf > 1) {
            cerr << "Warning: more than one infinite Bayes factor for feature " << i << " (" << T[0].features[i] << ")" << endl;
            for (size_t j = 0; j < n; ++j) post[j] = std::isinf(bf[j]) ? nan : 0.0;
        } else {
            double sum = 0.0;
            for (size_t j = 0; j < n; ++j) { post[j] = bf[j] * prior[j]; sum += post[j]; }
            if (sum == 0.0) {
                cerr << "Warning: every model of feature " << i << " (" << T[0].features[i] << ") has zero prior times Bayes factor" << endl;
                post.assign(n, nan);
            } else {
                for (size_t j = 0; j < n; ++j) post[j] = post[j] / sum;
            }
        }
        out = T[0].features[i];
        if (!T[0].kept_names.empty()) out += "\t" + T[0].kept_cells[i];
        for (size_t j = 0; j < n; ++j) out += "\t" + fmt(post[j]);
        out += "\n";
        fputs(out.c_str(), fp);
    }
}

#define MMG_CHECK(call)                                                                                       \
    do {                                                                                                      \
        if ((call) != 0) die(string("Error: ") + #call + ": " + mmg_last_error());                           \
    } while (0)

bool need(const vector<string> &a, size_t n)
{
    if (a.size() < n) usage_error("Error: mandatory arguments missing.");
    return true;
}

// ---- -traces DIR: the files of the reference's -tracedir (BMS::initialise_streams, print, printtune, print_pseudo) ------------------
// The library hands the recorded rows of a launch to sink() on the main thread, which copies them and returns; writer threads format
// them while the chain goes on.  File s belongs to thread s % T and every thread takes the chunks in order, so a file's lines are in
// order without a lock per file.  At most PENDING chunks wait: beyond that sink() waits for the writers, and the chain with it.

// fmt() into a buffer (at least 32 bytes): std::to_chars in the general format with 6 digits is printf's %g
char *fmt_to(char *out, double x)
{
    if (std::isnan(x)) {
        const char *t = std::signbit(x) ? "-nan" : "nan";
        const size_t n = strlen(t);
        memcpy(out, t, n);
        return out + n;
    }
    return std::to_chars(out, out + 32, x, std::chars_format::general, 6).ptr;
}

class TraceWriter {
public:
    static constexpr size_t PENDING = 4;
    atomic<uint64_t> bytes{0};   // written to the trace directory

    TraceWriter(const string &dir, const vector<string> &names, size_t F) : dir_(dir), F_(F), P_(names.size())
    {
        // burn-in files of every parameter but gamma, then the sampling files; gamma-burnin and logitp-burnin stay empty
        for (int phase = 0; phase < 2; ++phase)
            for (size_t s = 0; s + (phase ? 0 : 1) < P_; ++s) files_.push_back(open(names[s] + (phase ? "" : "-burnin")));
        fclose(open("gamma-burnin"));
        fclose(open("logitp-burnin"));
        meanLO_[0] = open("meanLO-burnin");
        meanLO_[1] = open("meanLO");
        logitp_ = open("logitp");
        // as many writers as the container's CPU quota (or, without one, the hardware) allows, 16 at most
        const int quota = cpu_quota();
        const size_t cpus = quota ? (size_t)quota : max<size_t>(1, thread::hardware_concurrency());
        const size_t T = max<size_t>(1, min<size_t>(min<size_t>(P_, 16), cpus));
        for (size_t t = 0; t < T; ++t) threads_.emplace_back([this, t, T] { work(t, T); });
    }
    ~TraceWriter() { finish(); }

    static int sink(void *user, int phase, uint32_t first_row, uint32_t n_rows, const double *rows)
    {
        return ((TraceWriter *)user)->push(phase, n_rows, rows);
    }

    // BMS::printtune: one line of each of meanLO and logitp
    void tune_line(const vector<double> &mean_lo, const vector<double> &logitp)
    {
        line(meanLO_[1], mean_lo);
        line(logitp_, logitp);
    }

    // BMS::print_pseudo; cols[c * F + f]
    void pseudo(size_t K, const size_t L[2], const uint32_t nc[2], const vector<double> &cols)
    {
        FILE *fp = open("pseudo");
        string out;
        for (int m = 0; m < 2; ++m) {
            const string M = to_string(m);
            out += "A" + M + "\tValpha" + M + "\t";
            for (size_t l = 0; l < K; ++l) out += "B" + M + "_" + to_string(l) + "\tVbeta" + M + "_" + to_string(l) + "\t";
            for (size_t l = 0; l < L[m]; ++l) out += "F" + M + "_" + to_string(l) + "\tVeta" + M + "_" + to_string(l) + "\tS" + M + "_" + to_string(l) + "\t";
            for (uint32_t c = 0; c < nc[m]; ++c) out += "J" + M + "_" + to_string(c) + "\tL" + M + "_" + to_string(c) + "\t";
            out += "Q" + M + "\tR" + M + "\t";
        }
        out += "\n";
        const size_t Q = cols.size() / F_;
        for (size_t f = 0; f < F_; ++f) {
            for (size_t c = 0; c < Q; ++c) out += fmt(cols[c * F_ + f]) + "\t";
            out += "\n";
        }
        put(fp, out.data(), out.size());
        if (fclose(fp) != 0) failed_ = true;
    }

    // waits for the writers and closes every file; false if anything could not be written
    bool finish()
    {
        {
            lock_guard<mutex> g(mu_);
            done_ = true;
        }
        cv_.notify_all();
        for (thread &t : threads_) t.join();
        threads_.clear();
        for (FILE **f : {&meanLO_[0], &meanLO_[1], &logitp_})
            if (*f) { if (fclose(*f) != 0) failed_ = true; *f = nullptr; }
        for (FILE *&f : files_)
            if (f) { if (fclose(f) != 0) failed_ = true; f = nullptr; }
        return !failed_;
    }

private:
    struct Chunk {
        int phase;
        uint32_t rows;
        vector<double> v;   // [rows][P of the phase][F]
        size_t left;        // threads that have not written it yet
    };

    FILE *open(const string &name)
    {
        const string path = dir_ + "/" + name;
        FILE *f = fopen(path.c_str(), "w");
        if (!f) die("Error: couldn't create " + path);
        return f;
    }
    void put(FILE *f, const char *data, size_t n)
    {
        if (fwrite(data, 1, n, f) != n) fail();
        bytes += n;
    }
    void line(FILE *f, const vector<double> &v)
    {
        string out(v.size() * 32 + 1, '\0');
        char *q = &out[0];
        for (double x : v) { q = fmt_to(q, x); *q++ = ' '; }
        *q++ = '\n';
        put(f, out.data(), (size_t)(q - out.data()));
    }
    int push(int phase, uint32_t rows, const double *data)
    {
        // the reference's print() ends a line in meanLO for every recorded iteration, though printtune alone writes values there
        const string nl(rows, '\n');
        put(meanLO_[phase], nl.data(), nl.size());
        auto c = make_shared<Chunk>();
        c->phase = phase; c->rows = rows; c->left = threads_.size();
        c->v.assign(data, data + (size_t)rows * (P_ - (phase ? 0 : 1)) * F_);
        unique_lock<mutex> g(mu_);
        cv_.wait(g, [&] { return pushed_ - retired_ < PENDING || failed_; });
        if (failed_) return 1;
        chunks_.push_back(c);
        ++pushed_;
        g.unlock();
        cv_.notify_all();
        return 0;
    }
    void work(size_t t, size_t T)
    {
        string out;
        for (size_t next = 0;; ++next) {
            shared_ptr<Chunk> c;
            {
                unique_lock<mutex> g(mu_);
                cv_.wait(g, [&] { return next < pushed_ || done_; });
                if (next >= pushed_) return;
                c = chunks_[next - retired_];
            }
            const size_t P = P_ - (c->phase ? 0 : 1), base = c->phase ? P_ - 1 : 0;
            for (size_t s = t; s < P; s += T) {
                out.resize((size_t)c->rows * (F_ * 32 + 1));
                char *q = &out[0];
                const bool gamma = c->phase && s + 1 == P_;   // printed as the int it is
                for (uint32_t r = 0; r < c->rows; ++r) {
                    const double *v = &c->v[((size_t)r * P + s) * F_];
                    for (size_t f = 0; f < F_; ++f) {
                        if (gamma) *q++ = v[f] != 0.0 ? '1' : '0';
                        else q = fmt_to(q, v[f]);
                        *q++ = ' ';
                    }
                    *q++ = '\n';
                }
                put(files_[base + s], out.data(), (size_t)(q - out.data()));
            }
            {
                lock_guard<mutex> g(mu_);
                // chunks retire in order: every thread takes them in order, so the oldest is the first to be written by all
                if (--c->left == 0) { chunks_.pop_front(); ++retired_; }
            }
            cv_.notify_all();
        }
    }

    string dir_;
    size_t F_, P_;
    vector<FILE *> files_;   // [P - 1] burn-in, then [P] sampling
    FILE *meanLO_[2] = {nullptr, nullptr}, *logitp_ = nullptr;
    vector<thread> threads_;
    mutex mu_;
    condition_variable cv_;
    deque<shared_ptr<Chunk>> chunks_;   // chunks retired_ .. pushed_ - 1
    size_t pushed_ = 0, retired_ = 0;
    bool done_ = false;
    atomic<bool> failed_{false};   // set by any thread; push() waits on it too
    void fail()
    {
        { lock_guard<mutex> g(mu_); failed_ = true; }   // (under the lock: push() must not miss the wake-up)
        cv_.notify_all();
    }
};

// ---- -effects FILE ---------------------------------------------------------------------------------------------------------------
#define MAXEFFECTROWS 4096
#define MAXPERCENTILES 32

// -effects_percentiles: a comma-separated list of 1 to 32 finite values in [0, 100]
vector<double> parse_percentiles(const string &text)
{
    const string msg = "Error: -effects_percentiles takes a comma-separated list of 1 to " + to_string(MAXPERCENTILES) + " percentiles in [0, 100].";
    const vector<double> pct = parse_list(text, 0, 100, msg);
    if (pct.size() > MAXPERCENTILES) die(msg);
    return pct;
}

// %.9g, NaN as "nan"
string fmt9(double x)
{
    if (std::isnan(x)) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", x);
    return buf;
}

// whether the model of traced parameter `name` (alpha<m>, beta<m>_k, eta<m>_l, lambda<m>_l, sigmasq<m>_c, rho<m>) has it
bool model_has(const string &name, bool fixalpha, const Model &model)
{
    const string stem = name.substr(0, name.find('_'));
    const int m = stem.back() - '0';
    const string kind = stem.substr(0, stem.size() - 1);
    if (kind == "alpha") return !fixalpha;
    if (kind == "beta") return !model.Mnil;
    if (kind == "eta" || kind == "lambda") return !model.Pnil[m];
    return true;
}

// what mmg_effects_get gives, and the traced parameters without gamma
struct Effects {
    vector<string> names;
    vector<uint32_t> n, n_gt;
    vector<double> mean, sd, q;
};

// The effects table: a line per feature, in the order of the stdout table.
void write_effects(const string &file, const vector<string> &features, const vector<double> &pct, bool fixalpha, const Model &model, const Effects &fx)
{
    const vector<string> &names = fx.names;
    const vector<uint32_t> &n = fx.n, &n_gt = fx.n_gt;
    const vector<double> &mean = fx.mean, &sd = fx.sd, &q = fx.q;
    FILE *fp = fopen(file.c_str(), "w");
    if (!fp) die("Error: couldn't create " + file);
    const size_t F = features.size(), np = pct.size();
    vector<size_t> cols;
    for (size_t s = 0; s < names.size(); ++s)
        if (model_has(names[s], fixalpha, model)) cols.push_back(s);
    string out = "feature_id\tn0\tn1";
    for (size_t s : cols) {
        out += "\t" + names[s] + "_mean\t" + names[s] + "_sd\t" + names[s] + "_p_gt0";
        for (double p : pct) out += "\t" + names[s] + "_q" + fmt9(p);
    }
    out += "\n";
    bool ok = fputs(out.c_str(), fp) >= 0;
    for (size_t f = 0; f < F && ok; ++f) {
        out = features[f] + "\t" + to_string(n[f]) + "\t" + to_string(n[F + f]);
        for (size_t s : cols) {
            const int m = names[s].substr(0, names[s].find('_')).back() - '0';
            const double nm = (double)n[(size_t)m * F + f];
            out += "\t" + fmt9(mean[s * F + f]) + "\t" + fmt9(sd[s * F + f]) + "\t" + fmt9((double)n_gt[s * F + f] / nm);
            for (size_t j = 0; j < np; ++j) out += "\t" + fmt9(q[(s * np + j) * F + f]);
        }
        out += "\n";
        ok = fputs(out.c_str(), fp) >= 0;
    }
    if (fclose(fp) != 0 || !ok) die("Error: couldn't write " + file);
}

// The likelihood-ratio table: a line per feature, in the order of the stdout table; the estimates are named as the trace files are,
// NA where a model has no such term.
void write_lrt(FILE *fp, const string &file, const vector<string> &features, const Design &D, bool fixalpha, mmg_diff_lrt *h,
               mmg_diff_lrt_perm *perm = nullptr)
{
    const size_t F = features.size();
    int32_t flags[3] = {0, 0, 0}, df = 0;
    uint32_t nc[2] = {0, 0}, pc[2] = {0, 0};
    MMG_CHECK(mmg_diff_lrt_info(h, flags, nc, pc));
    const bool Mnil = flags[0] != 0, Pnil[2] = {flags[1] != 0, flags[2] != 0};
    const size_t L[2] = {D.L0, D.L1};
    vector<double> ll(2 * F), stat(F), pv(F), qv(F), theta[2], sig[2];
    vector<uint32_t> iters(2 * F), status(2 * F);
    for (int m = 0; m < 2; ++m) { theta[m].resize((size_t)pc[m] * F); sig[m].resize((size_t)nc[m] * F); }
    MMG_CHECK(mmg_diff_lrt_get(h, ll.data(), stat.data(), pv.data(), qv.data(), &df, theta[0].data(), theta[1].data(), sig[0].data(), sig[1].data(),
                               iters.data(), status.data()));
    // -lrtperm: four columns after the plain line
    vector<uint64_t> perm_ge(perm ? F : 0), null_ge(perm ? F : 0);
    vector<double> perm_p(perm ? F : 0), q_perm(perm ? F : 0);
    if (perm) MMG_CHECK(mmg_diff_lrt_perm_get(perm, perm_ge.data(), NULL, perm_p.data(), null_ge.data(), q_perm.data()));
    string out = "feature_id\tloglik0\tloglik1\tlrt_stat\tdf\tp_value\tq_value\talpha0\talpha1";
    for (int m = 0; m < 2; ++m)
        for (size_t k = 0; k < D.K; ++k) out += "\tbeta" + to_string(m) + "_" + to_string(k);
    for (int m = 0; m < 2; ++m)
        for (size_t l = 0; l < L[m]; ++l) out += "\teta" + to_string(m) + "_" + to_string(l);
    for (int m = 0; m < 2; ++m)
        for (uint32_t c = 0; c < nc[m]; ++c) out += "\tsigmasq" + to_string(m) + "_" + to_string(c);
    out += "\titers0\titers1\tstatus0\tstatus1";
    if (perm) out += "\tperm_ge\tperm_p\tnull_ge\tq_perm";
    out += "\n";
    bool ok = fputs(out.c_str(), fp) >= 0;
    const size_t a_cols = fixalpha ? 0 : 1, b_cols = Mnil ? 0 : D.K;
    for (size_t f = 0; f < F && ok; ++f) {
        out = features[f] + "\t" + fmt(ll[f]) + "\t" + fmt(ll[F + f]) + "\t" + fmt(stat[f]) + "\t" + to_string(df) + "\t" + fmt(pv[f]) + "\t" + fmt(qv[f]);
        for (int m = 0; m < 2; ++m) out += "\t" + (fixalpha ? string("NA") : fmt(theta[m][f]));
        for (int m = 0; m < 2; ++m)
            for (size_t k = 0; k < D.K; ++k) out += "\t" + (Mnil ? string("NA") : fmt(theta[m][(a_cols + k) * F + f]));
        for (int m = 0; m < 2; ++m)
            for (size_t l = 0; l < L[m]; ++l) out += "\t" + (Pnil[m] ? string("NA") : fmt(theta[m][(a_cols + b_cols + l) * F + f]));
        for (int m = 0; m < 2; ++m)
            for (uint32_t c = 0; c < nc[m]; ++c) out += "\t" + fmt(sig[m][(size_t)c * F + f]);
        out += "\t" + to_string(iters[f]) + "\t" + to_string(iters[F + f]) + "\t" + to_string(status[f]) + "\t" + to_string(status[F + f]);
        if (perm) out += "\t" + to_string(perm_ge[f]) + "\t" + fmt(perm_p[f]) + "\t" + to_string(null_ge[f]) + "\t" + fmt(q_perm[f]);
        out += "\n";
        ok = fputs(out.c_str(), fp) >= 0;
    }
    if (fflush(fp) != 0 || !ok) die("Error: couldn't write " + file);
}

// ---- options ------------------------------------------------------------------------------------------------------------------------
struct Options {
    vector<string> matrices_files;   // every -m; more than one: the polytomous run
    vector<int> simple_de;           // -de
    vector<string> files;            // what follows the options: the mmseq tables or, with -polyclass, mmdiff tables
    bool polyclass_mode = false, prior_given = false, polyout_given = false, chains_given = false, chainout_given = false, perms_given = false,
         permout_given = false, lrt_given = false, lrt_only = false, lrtperm_given = false, effects_every_given = false, effects_pct_given = false;
    string prior_text, polyout, chainout, permout, traces, effects, effects_pct_text = "2.5,50,97.5", lrt_file;
    long lrt_perms = 0, effects_every = 0;
    uint32_t effects_rows = 0;       // with -effects: the rows -iter and -effects_every give
    vector<double> effects_pct;
    int chains = 1, perms = 0, range_start = -1, range_end = -1;
    bool useprops = false, normalise = true, customuhfrac = false, permute = false;
    double uhfrac = -1;
    Mcmc mc;
    bool poly_run() const { return matrices_files.size() > 1; }
};

// the value of -chains, -permutations, -lrtperm or -effects_every: all of `v` a decimal number between lo and hi
long int_option(const string &name, const string &v, long lo, long hi, bool usage = false)
{
    char *end = NULL;
    const long n = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end != '\0' || n < lo || n > hi) {
        const string msg = "Error: " + name + " takes an integer between " + to_string(lo) + " and " + to_string(hi) + ".";
        if (usage) usage_error(msg);
        die(msg);
    }
    return n;
}

// -m FILE [-m FILE ...] or -de n1 n2 ...: the last option, `arguments` what follows its name; the mmseq tables are left in `arguments`
void parse_design_option(const string &a0, vector<string> &arguments, Options &opt)
{
    // -m FILE -m FILE ...: consecutive pairs are one polytomous run
    size_t first_other = 0;
    if (a0 == "-m")
        for (first_other = arguments.empty() ? 0 : 1; first_other + 1 < arguments.size() && arguments[first_other] == "-m";) first_other += 2;
    size_t n_m = a0 == "-m" ? 1 : 0;
    bool de_too = a0 == "-de";
    for (size_t i = 0; i < arguments.size(); i++) {
        if (arguments[i] == "-m" && i + 1 < arguments.size()) n_m++;
        if (arguments[i] == "-de") de_too = true;
    }
    if (de_too && n_m > 1) usage_error("Error: -de cannot be combined with more than one -m.");
    if (opt.polyclass_mode) usage_error("Error: -polyclass takes mmdiff tables, not -de or -m.");
    for (size_t i = first_other; i < arguments.size(); i++)
        if (arguments[i].find("-") == 0) {
            cerr << "Error: optional arguments must be specified before -de or -m." << endl << endl;
            printUsage(cerr);
            exit(1);
        }
    if (a0 == "-m") {
        need(arguments, 1);
        opt.matrices_files.push_back(arguments[0]);
        arguments.erase(arguments.begin());
        while (arguments.size() >= 2 && arguments[0] == "-m") {
            opt.matrices_files.push_back(arguments[1]);
            arguments.erase(arguments.begin(), arguments.begin() + 2);
        }
        if (opt.matrices_files.size() > MAXMODELS)
            die("Error: this mmdiff handles at most " + to_string(MAXMODELS) + " alternative models (-m) in one run.");
    } else {
        int ss = 0;
        cerr << "Number of samples in each group:";
        while (ss < (int)arguments.size()) {
            opt.simple_de.push_back(atoi(arguments[0].c_str()));
            cerr << " " << opt.simple_de.back();
            arguments.erase(arguments.begin());
            if (opt.simple_de.back() < 1) die("\nError: each grouping must contain at least one sample");
            ss += opt.simple_de.back();
        }
        cerr << endl;
        if (ss != (int)arguments.size()) die("Error: total number of samples specified with -de must equal number of MMSEQ files");
    }
}

Options parse_args(int argc, char **argv)
{
    Options opt;
    Mcmc &mc = opt.mc;
    vector<string> arguments;
    for (int i = 1; i < argc; i++) arguments.push_back(string(argv[i]));

    while (true) {
        const string a0 = arguments.empty() ? string() : arguments[0];
        auto flag = [&]() { arguments.erase(arguments.begin()); return true; };
        auto take = [&]() { arguments.erase(arguments.begin()); need(arguments, 1); string v = arguments[0]; arguments.erase(arguments.begin()); return v; };
        if (a0 == "-tracedir") {
            die("Error: -tracedir is not implemented in this version of mmdiff (MCMC traces are not written); use -traces DIR.");
        } else if (a0 == "-traces") {
            opt.traces = take();
            if (opt.traces.empty()) die("Error: -traces needs a directory.");
        } else if (a0 == "-effects") {
            opt.effects = take();
            if (opt.effects.empty()) die("Error: -effects needs a file name.");
        } else if (a0 == "-lrt") {
            opt.lrt_file = take();
            if (opt.lrt_file.empty()) die("Error: -lrt needs a file name.");
            opt.lrt_given = true;
        } else if (a0 == "-lrtonly") {
            opt.lrt_only = flag();
        } else if (a0 == "-lrtperm") {
            opt.lrt_perms = int_option(a0, take(), 1, MAXLRTPERMS, true);
            opt.lrtperm_given = true;
        } else if (a0 == "-effects_every") {
            opt.effects_every = int_option(a0, take(), 1, 1L << 30);
            opt.effects_every_given = true;
        } else if (a0 == "-effects_percentiles") {
            opt.effects_pct_text = take();
            opt.effects_pct_given = true;
        } else if (a0 == "-m" || a0 == "-de") {
            arguments.erase(arguments.begin());
            parse_design_option(a0, arguments, opt);
        } else if (a0 == "-useprops") {
            opt.useprops = flag();
        } else if (a0 == "-p") {
            mc.p = strtod(take().c_str(), NULL);
            if (!(mc.p >= 0 && mc.p <= 1)) die("Error: p must be between 0 and 1.");
        } else if (a0 == "-s") {
            mc.s = strtod(take().c_str(), NULL);
            if (!(mc.s > 0) || !std::isfinite(mc.s)) die("Error: s must be positive.");
        } else if (a0 == "-d") {
            mc.d = strtod(take().c_str(), NULL);
            if (!(mc.d > 0) || !std::isfinite(mc.d)) die("Error: d must be positive.");
        } else if (a0 == "-pdash") {
            mc.pdash = strtod(take().c_str(), NULL);
            if (!(mc.pdash >= 0 && mc.pdash <= 1)) die("Error: pdash must be between 0 and 1.");
        } else if (a0 == "-fixalpha") {
            mc.fixalpha = flag();
        } else if (a0 == "-l") {
            take();   // accepted for compatibility; the reference does not use it either
        } else if (a0 == "-burnin") {
            mc.burnin = atoi(take().c_str());
        } else if (a0 == "-iter") {
            mc.iters = atoi(take().c_str());
        } else if (a0 == "-seed") {
            mc.seed = (uint64_t)(uint32_t)atoi(take().c_str());
        } else if (a0 == "-nonorm") {
            opt.normalise = !flag();
        } else if (a0 == "-notune") {
            mc.tune = !flag();
        } else if (a0 == "-permute") {
            opt.permute = flag();
        } else if (a0 == "-uhfrac") {
            opt.customuhfrac = true;
            opt.uhfrac = atof(take().c_str());
        } else if (a0 == "-range") {
            arguments.erase(arguments.begin());
            need(arguments, 2);
            opt.range_start = atoi(arguments[0].c_str());
            opt.range_end = atoi(arguments[1].c_str());
            arguments.erase(arguments.begin(), arguments.begin() + 2);
        } else if (a0 == "-polyclass") {
            opt.polyclass_mode = flag();
        } else if (a0 == "-prior") {
            opt.prior_text = take();
            opt.prior_given = true;
        } else if (a0 == "-polyout") {
            opt.polyout = take();
            opt.polyout_given = true;
        } else if (a0 == "-chains") {
            opt.chains = (int)int_option(a0, take(), 1, MAXCHAINS);
            opt.chains_given = true;
        } else if (a0 == "-chainout") {
            opt.chainout = take();
            opt.chainout_given = true;
        } else if (a0 == "-permutations") {
            opt.perms = (int)int_option(a0, take(), 1, MAXPERMS);
            opt.perms_given = true;
        } else if (a0 == "-permout") {
            opt.permout = take();
            opt.permout_given = true;
        } else if (a0 == "-h" || a0 == "--help" || a0 == "-help") {
            cerr << "Bayesian model selection for RNA-seq expression estimates.\n";
            printUsage(cerr);
            exit(1);
        } else if (a0 == "-v" || a0 == "--version" || a0 == "-version") {
            die("mmdiff-1.0.10-gfx950");
        } else {
            if (!a0.empty() && a0[0] == '-') usage_error("Error: unrecognised option " + a0 + ".");
            else if (opt.polyclass_mode && arguments.size() >= 2) break;
            else if (opt.polyclass_mode) usage_error("Error: -polyclass needs at least two mmdiff tables.");
            else if (arguments.size() <= 2) usage_error("Error: mandatory arguments missing.");
            else break;
        }
    }
    opt.files = arguments;
    return opt;
}

// the options that need or exclude each other; the percentiles of -effects
void check_combinations(Options &opt)
{
    const bool poly_run = opt.poly_run(), polyclass_mode = opt.polyclass_mode, traces = !opt.traces.empty(), effects = !opt.effects.empty();
    if ((opt.prior_given || opt.polyout_given) && !poly_run && !polyclass_mode)
        usage_error("Error: -prior and -polyout need more than one -m (or, -prior, -polyclass).");
    if (opt.polyout_given && !poly_run) usage_error("Error: -polyout needs more than one -m.");
    if (opt.chainout_given && !opt.chains_given) usage_error("Error: -chainout needs -chains.");
    if (opt.chains_given && (poly_run || polyclass_mode))
        usage_error("Error: -chains cannot be combined with more than one -m or with -polyclass (chains of several alternatives are left for later).");
    if (traces && (opt.chains_given || poly_run || polyclass_mode))
        usage_error("Error: -traces cannot be combined with -chains, more than one -m or -polyclass (traces of several chains or alternatives are left for later).");
    if ((opt.effects_every_given || opt.effects_pct_given) && !effects)
        usage_error("Error: -effects_every and -effects_percentiles need -effects.");
    if (effects && traces)
        usage_error("Error: -effects cannot be combined with -traces (the handle records rows for one of them).");
    if (effects && (opt.chains_given || poly_run || polyclass_mode))
        usage_error("Error: -effects cannot be combined with -chains, more than one -m or -polyclass (effects of several chains or alternatives are left for later).");
    if (opt.permout_given && !opt.perms_given) usage_error("Error: -permout needs -permutations.");
    if (opt.perms_given && (opt.permute || opt.chains > 1 || opt.chainout_given || poly_run || polyclass_mode || traces || effects))
        usage_error("Error: -permutations cannot be combined with -permute, -chains above 1 (or -chainout), more than one -m, -traces, -effects or -polyclass.");
    if (opt.lrt_only && !opt.lrt_given) usage_error("Error: -lrtonly needs -lrt.");
    if ((opt.lrt_given || opt.lrt_only) && (opt.chains_given || poly_run || opt.perms_given || polyclass_mode))
        usage_error("Error: -lrt and -lrtonly cannot be combined with -chains, more than one -m, -permutations or -polyclass.");
    if (opt.lrtperm_given && !opt.lrt_given) usage_error("Error: -lrtperm needs -lrt.");
    if (opt.lrtperm_given && opt.permute) usage_error("Error: -lrtperm cannot be combined with -permute.");
    if (effects) opt.effects_pct = parse_percentiles(opt.effects_pct_text);
}

// what a run on mmseq tables checks of its options before it reads them: the lengths, the rows of -effects, a design, the trace directory
void check_run(Options &opt)
{
    const Mcmc &mc = opt.mc;
    if (mc.burnin <= 0 || mc.iters <= 0) usage_error("Error: negative burnin and iter parameters.");
    if (mc.burnin % OUTLEN != 0 || mc.iters % OUTLEN != 0) usage_error("Error: burnin and iter parameters must be multiples of " + to_string(OUTLEN));
    if (opt.useprops) {
        cerr << "Using proportions, therefore disabling normalisation.\n";
        opt.normalise = false;
    }
    if (!opt.effects.empty()) {
        if (!opt.effects_every_given) opt.effects_every = max(1, mc.iters / 1024);
        const long rows = ((long)mc.iters + opt.effects_every - 1) / opt.effects_every;
        if (rows > MAXEFFECTROWS)
            die("Error: -effects keeps at most " + to_string(MAXEFFECTROWS) + " rows: -iter " + to_string(mc.iters) + " with -effects_every "
                + to_string(opt.effects_every) + " needs " + to_string(rows) + ".");
        opt.effects_rows = (uint32_t)rows;
    }
    if (opt.matrices_files.empty() && opt.simple_de.size() == 0) die("Error: either -de or -m must be specified");
    if (opt.matrices_files.empty() && opt.simple_de.size() == 1) die("Error: -de requires at least two groupings");
    if (!opt.traces.empty()) {   // src/mmdiff.cpp:594-603
        mkdir(opt.traces.c_str(), 0755);
        if (::access(opt.traces.c_str(), F_OK | R_OK | W_OK | X_OK) == -1) die("Error: can't write to trace directory " + opt.traces + ".");
    }
}

// ---- the stages of a run ------------------------------------------------------------------------------------------------------------
// -polyclass: host only, no device is looked for
int run_polyclass(const Options &opt)
{
    const vector<string> &tables = opt.files;
    const size_t J = tables.size();
    const vector<double> prior = parse_prior(opt.prior_given, opt.prior_text, J + 1);
    vector<PolyTable> T(J);
    for (size_t j = 0; j < J; ++j) {
        ifstream ifs(tables[j].c_str());
        if (!ifs.good()) die("Error: couldn't open " + tables[j]);
        parse_poly_table(ifs, tables[j], j == 0, T[j]);
        if (j > 0) check_same_features(T[0], tables[0], T[j], tables[j]);
    }
    polyclass(T, prior, stdout);
    return 0;
}

// the mmseq tables, normalised and permuted as asked
Inputs load_inputs(Options &opt)
{
    Inputs in;
    in.filenames = opt.files;
    const size_t S = in.filenames.size();
    if (opt.customuhfrac && (opt.uhfrac > 1 || opt.uhfrac < 1.0 / (double)S)) die("Error: uhfrac must be <= 1 and >= 1/N.");
    if (!opt.customuhfrac) opt.uhfrac = max(0.2, (double)(S - S * S / 160) / (double)S);
    if (opt.normalise) cerr << "Min unique hits fraction for normalisation: " << opt.uhfrac << endl;
    if (S > 512) die("Error: this mmdiff handles at most 512 samples.");
    Mat uh;
    parse_mmseq(in.filenames, in.features, in.y, in.e, uh, opt.range_start, opt.range_end, opt.useprops);
    const size_t F = in.features.size();
    if (F == 0) die("Error: no features to analyse.");
    if (opt.normalise) apply_normalisation(in.filenames, in.y, uh, F, S, opt.uhfrac);
    if (opt.permute) apply_permutation(in.y, in.e, F, S, opt.mc.seed);
    return in;
}

// -de n1 n2 ...: model 0 one mean and one variance class; model 1 a mean and a class per group (two groups: a contrast of +-0.5)
Design de_design(const vector<int> &simple_de, size_t S)
{
    Design D;
    const size_t G = simple_de.size();
    D.N = S; D.K = 1; D.L0 = 1; D.L1 = G > 2 ? G : 1; D.CC = 2;
    D.M.assign(S, 0.0); D.P0.assign(S, 0.0); D.P1.assign(S * D.L1, 0.0); D.C.assign(S * 2, 0);
    size_t k = 0;
    for (size_t i = 0; i < G; i++)
        for (int j = 0; j < simple_de[i]; j++) {
            D.C[k * 2 + 1] = (int)i;
            D.P0[k] = 1.0;
            if (G > 2) D.P1[k * D.L1 + i] = 1.0;
            else D.P1[k] = i == 0 ? .5 : -.5;
            k++;
        }
    return D;
}

// The files of -polyout, -chainout, -permout and -lrt: created before the device is looked for, closed when the run ends.
struct OutFiles {
    vector<FILE *> f;
    vector<string> names;
    explicit OutFiles(size_t n) : f(n, nullptr), names(n) {}
    ~OutFiles() { for (FILE *x : f) if (x) fclose(x); }
    void open(size_t i, const string &name)
    {
        names[i] = name;
        if (!(f[i] = fopen(name.c_str(), "w"))) die("Error: couldn't create " + name);
    }
    void flush(size_t i) { if (f[i] && fflush(f[i]) != 0) die("Error: couldn't write " + names[i]); }
};

template <typename H> using Owner = unique_ptr<H, void (*)(H *)>;   // a handle of the library and the entry that destroys it

void require_device()
{
    int ndev = 0;
    if (mmg_device_count(&ndev) != 0 || ndev < 1) die("Error: no HIP device available: mmdiff has no CPU fallback");
}

// The entries that the handles of several replicas (alternatives, chains, the data and its permutations) share apart from the handle
// type, and their family in the entries' names.
template <typename H> struct ReplicaApi {
    const char *family;
    int (*burnin)(H *, uint32_t);
    int (*tune_batch)(H *, uint32_t *, int32_t *);
    int (*info)(H *, uint32_t, int32_t *, uint32_t *, uint32_t *, int32_t *);
    int (*sample)(H *, uint32_t);
    void (*destroy)(H *);
};
const ReplicaApi<mmg_diff_poly> POLY = {"poly", mmg_diff_poly_burnin, mmg_diff_poly_tune_batch, mmg_diff_poly_info, mmg_diff_poly_sample,
                                        mmg_diff_poly_destroy};
const ReplicaApi<mmg_diff_chains> CHAINS = {"chains", mmg_diff_chains_burnin, mmg_diff_chains_tune_batch, mmg_diff_chains_info,
                                            mmg_diff_chains_sample, mmg_diff_chains_destroy};
const ReplicaApi<mmg_diff_perm> PERM = {"perm", mmg_diff_perm_burnin, mmg_diff_perm_tune_batch, mmg_diff_perm_info, mmg_diff_perm_sample,
                                        mmg_diff_perm_destroy};

// The MCMC of R replicas on the handle create() gives: the device check, the burn-in, tuning batches until every replica has ended (each
// stops at the first batch after which none of its features is untuned, or with the others at MAXBATCHES), the batch count of each, the
// sampling.  what: the replicas in the burn-in line; label(r): replica r in its own line.
template <typename H, typename Create, typename Label>
Owner<H> run_replicas(const ReplicaApi<H> &api, Create create, size_t R, const Mcmc &mc, const string &what, Label label)
{
    auto check = [&](int rc, const char *entry) {
        if (rc != 0) die(string("Error: mmg_diff_") + api.family + "_" + entry + ": " + mmg_last_error());
    };
    // every input is checked: now the device
    require_device();
    Owner<H> h(create(), api.destroy);
    cerr << "BURNIN (" << mc.burnin << " iterations, " << what << ")...";
    check(api.burnin(h.get(), (uint32_t)mc.burnin), "burnin");
    cerr << "\nSetting pseudopriors...done.\n";
    if (mc.tune) {
        vector<uint32_t> untuned(R);
        vector<int32_t> ended(R);
        int numbatches = 0;
        bool all_ended = false;
        while (!all_ended && numbatches != MAXBATCHES) {
            check(api.tune_batch(h.get(), untuned.data(), ended.data()), "tune_batch");
            numbatches++;
            all_ended = true;
            uint64_t left = 0;
            for (size_t r = 0; r < R; ++r) { all_ended = all_ended && ended[r]; left += untuned[r]; }
            if (numbatches % 64 == 0) cerr << "TUNING BATCH " << numbatches << " (" << left << " left)\r";
        }
    }
    for (size_t r = 0; r < R; ++r) {
        uint32_t nb = 0;
        check(api.info(h.get(), (uint32_t)r, NULL, NULL, &nb, NULL), "info");
        cerr << label(r) << ": sampling after " << nb << " tuning batches\n";
    }
    cerr << "TRACE (" << mc.iters << " iterations)";
    check(api.sample(h.get(), (uint32_t)mc.iters), "sample");
    return h;
}

// repeated -m: J alternatives against one model 0 on one device handle.  Table j (what `mmdiff <same options> -m alt_j <same tables>`
// prints) goes to BASE.model<j>.mmdiff with -polyout; stdout gets polyclass of the tables, from the Bayes factors as the tables print
// them (%g text parsed back), so that `mmdiff -polyclass` on the written tables reproduces it byte for byte.
int run_poly(const Options &opt, const Inputs &in)
{
    const Mcmc &mc = opt.mc;
    const vector<string> &mats = opt.matrices_files;
    const size_t J = mats.size(), S = in.filenames.size(), F = in.features.size();
    vector<Model> models(J);
    const Design &D0 = models[0].D;
    for (size_t j = 0; j < J; ++j) {
        Design &D = models[j].D;
        cerr << "Alternative " << j + 1 << " (" << mats[j] << "):\n";
        parse_matrices(mats[j], D, S);
        validate_design(D, S, mc.fixalpha, models[j].Mnil, models[j].Pnil);
        bool same = D.K == D0.K && D.L0 == D0.L0 && D.M == D0.M && D.P0 == D0.P0;
        for (size_t i = 0; same && i < S; ++i) same = D.C[i * 2] == D0.C[i * 2];
        if (!same) die("Error: model 0 differs between " + mats[0] + " and " + mats[j]);
    }
    const vector<double> prior = parse_prior(opt.prior_given, opt.prior_text, J + 1);
    OutFiles files(J);
    if (opt.polyout_given)
        for (size_t j = 0; j < J; ++j) files.open(j, opt.polyout + ".model" + to_string(j + 1) + ".mmdiff");

    vector<uint32_t> L1(J);
    Mat P1;
    vector<int> C0(S), C1(J * S);
    for (size_t i = 0; i < S; ++i) C0[i] = D0.C[i * 2];
    for (size_t j = 0; j < J; ++j) {
        const Design &D = models[j].D;
        L1[j] = (uint32_t)D.L1;
        P1.insert(P1.end(), D.P1.begin(), D.P1.end());
        for (size_t i = 0; i < S; ++i) C1[j * S + i] = D.C[i * 2 + 1];
    }
    auto create = [&] {
        mmg_diff_poly *h = nullptr;
        MMG_CHECK(mmg_diff_poly_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D0.K, D0.M.data(), (uint32_t)D0.L0,
                                       D0.P0.data(), C0.data(), (uint32_t)J, L1.data(), P1.data(), C1.data(), mc.d, mc.s, mc.pdash,
                                       mc.fixalpha ? 1 : 0, mc.seed, &h));
        return h;
    };
    Owner<mmg_diff_poly> h = run_replicas(POLY, create, J, mc, to_string(J) + " alternatives", [](size_t j) { return "model " + to_string(j + 1); });
    cerr << "\nDONE MCMC\n";
    vector<PolyTable> T(J);
    for (size_t j = 0; j < J; ++j) {
        DiffResults r(F, models[j].D);
        MMG_CHECK(mmg_diff_poly_get_results(h.get(), (uint32_t)j, r.gm.data(), r.logitp.data(), r.alpha.data(), r.beta.data(), r.eta.data()));
        string text;
        write_table(files.f[j], &text, in, models[j], mc, r);
        files.flush(j);
        istringstream table(text);
        parse_poly_table(table, "the table of alternative " + to_string(j + 1), j == 0, T[j]);
    }
    polyclass(T, prior, stdout);
    return 0;
}

// -chains C, C >= 2: C chains of one comparison on one device handle, chain c keyed (seed, c).  Table c (what a single run prints for
// that chain) goes to BASE.chain<c>.mmdiff with -chainout; stdout gets the pooled table.
int run_chains(const Options &opt, const Inputs &in, const Model &model)
{
    const Mcmc &mc = opt.mc;
    const Design &D = model.D;
    const size_t C = (size_t)opt.chains, S = in.filenames.size(), F = in.features.size();
    OutFiles files(C);
    if (opt.chainout_given)
        for (size_t c = 0; c < C; ++c) files.open(c, opt.chainout + ".chain" + to_string(c) + ".mmdiff");
    auto create = [&] {
        mmg_diff_chains *h = nullptr;
        MMG_CHECK(mmg_diff_chains_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D.K, D.M.data(), (uint32_t)D.L0,
                                         D.P0.data(), (uint32_t)D.L1, D.P1.data(), D.C.data(), mc.d, mc.s, mc.pdash, mc.fixalpha ? 1 : 0, mc.seed,
                                         (uint32_t)C, (uint32_t)mc.iters, &h));
        return h;
    };
    Owner<mmg_diff_chains> h = run_replicas(CHAINS, create, C, mc, to_string(C) + " chains", [](size_t c) { return "chain " + to_string(c); });
    MMG_CHECK(mmg_diff_chains_pool(h.get()));
    cerr << "\nDONE MCMC\n";
    DiffResults r(F, D);
    TableExtras extras;
    extras.warn_stuck = false;
    for (size_t c = 0; c < C && opt.chainout_given; ++c) {
        MMG_CHECK(mmg_diff_chains_get_results(h.get(), (uint32_t)c, r.gm.data(), r.logitp.data(), r.alpha.data(), r.beta.data(), r.eta.data()));
        write_table(files.f[c], nullptr, in, model, mc, r, extras);
        files.flush(c);
    }
    // the pooled table: chain 0's gamma mean and logit p' are not printed (the Bayes factor is exp(log_bf)), the means are the pooled ones
    PooledCols pool(F);
    MMG_CHECK(mmg_diff_chains_get_results(h.get(), 0, r.gm.data(), r.logitp.data(), NULL, NULL, NULL));
    MMG_CHECK(mmg_diff_chains_get_pooled(h.get(), pool.log_bf.data(), pool.log_bf_sd.data(), pool.log_bf_mcse.data(), pool.chains_mixed.data(),
                                         r.alpha.data(), r.beta.data(), r.eta.data()));
    for (size_t f = 0; f < F; ++f)
        if (pool.chains_mixed[f] < (uint32_t)C)
            cerr << "Warning: gamma mixed in " << pool.chains_mixed[f] << " of " << C << " chains for feature " << f << endl;
    extras.pool = &pool;
    write_table(stdout, nullptr, in, model, mc, r, extras);
    return 0;
}

// -permutations B: the data and B shuffled copies of it on one device handle.  stdout gets the plain run's
// table with perm_ge and q_value appended; the table of shuffled copy b (what -permute prints with the seed seed ^ (b << 32)) goes to
// BASE.perm<b>.mmdiff with -permout.
int run_perm(const Options &opt, const Inputs &in, const Model &model)
{
    const Mcmc &mc = opt.mc;
    const Design &D = model.D;
    const size_t B = (size_t)opt.perms, R = B + 1, S = in.filenames.size(), F = in.features.size();
    OutFiles files(R);
    if (opt.permout_given)
        for (size_t b = 1; b < R; ++b) files.open(b, opt.permout + ".perm" + to_string(b) + ".mmdiff");
    auto create = [&] {
        mmg_diff_perm *h = nullptr;
        MMG_CHECK(mmg_diff_perm_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D.K, D.M.data(), (uint32_t)D.L0,
                                       D.P0.data(), (uint32_t)D.L1, D.P1.data(), D.C.data(), mc.d, mc.s, mc.pdash, mc.fixalpha ? 1 : 0, mc.seed,
                                       (uint32_t)B, &h));
        return h;
    };
    Owner<mmg_diff_perm> h = run_replicas(PERM, create, R, mc, "the data and " + to_string(B) + " permutations",
                                          [](size_t b) { return "replica " + to_string(b); });
    MMG_CHECK(mmg_diff_perm_qvalues(h.get()));
    cerr << "\nDONE MCMC\n";
    DiffResults r(F, D);
    TableExtras extras;
    extras.warn_stuck = false;
    Inputs shuffled = in;
    for (size_t b = 1; b < R && opt.permout_given; ++b) {
        // the table's mu_ / sd_ columns: the shuffle the device applied to replica b, on the host
        shuffled.y = in.y;
        shuffled.e = in.e;
        apply_permutation(shuffled.y, shuffled.e, F, S, mc.seed ^ ((uint64_t)b << 32), true);
        MMG_CHECK(mmg_diff_perm_get_results(h.get(), (uint32_t)b, r.gm.data(), r.logitp.data(), r.alpha.data(), r.beta.data(), r.eta.data()));
        write_table(files.f[b], nullptr, shuffled, model, mc, r, extras);
        files.flush(b);
    }
    PermCols cols(F);
    MMG_CHECK(mmg_diff_perm_get_results(h.get(), 0, r.gm.data(), r.logitp.data(), r.alpha.data(), r.beta.data(), r.eta.data()));
    MMG_CHECK(mmg_diff_perm_get_qvalues(h.get(), NULL, cols.null_ge.data(), cols.q.data()));
    extras.warn_stuck = true;
    extras.perm = &cols;
    write_table(stdout, nullptr, in, model, mc, r, extras);
    return 0;
}

// -lrt FILE: the likelihood-ratio test of the y, e and design the chain gets, with -lrtperm its permutation null; the table to `out`
void run_lrt(const Options &opt, const Inputs &in, const Model &model, FILE *out)
{
    const Design &D = model.D;
    const size_t S = in.filenames.size(), F = in.features.size();
    const int fixalpha = opt.mc.fixalpha ? 1 : 0;
    if (!opt.lrtperm_given) {
        mmg_diff_lrt *lh = nullptr;
        MMG_CHECK(mmg_diff_lrt_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D.K, D.M.data(), (uint32_t)D.L0, D.P0.data(),
                                      (uint32_t)D.L1, D.P1.data(), D.C.data(), fixalpha, 0, &lh));
        const Owner<mmg_diff_lrt> owner(lh, mmg_diff_lrt_destroy);
        write_lrt(out, opt.lrt_file, in.features, D, opt.mc.fixalpha, lh);
    } else {
        // copy b: the data of BASE.perm<b>.mmdiff of this command line with -permutations (the seed run_perm hands on)
        mmg_diff_lrt_perm *ph = nullptr;
        MMG_CHECK(mmg_diff_lrt_perm_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D.K, D.M.data(), (uint32_t)D.L0,
                                           D.P0.data(), (uint32_t)D.L1, D.P1.data(), D.C.data(), fixalpha, 0, (uint32_t)opt.lrt_perms, opt.mc.seed,
                                           0, &ph));
        const Owner<mmg_diff_lrt_perm> owner(ph, mmg_diff_lrt_perm_destroy);
        write_lrt(out, opt.lrt_file, in.features, D, opt.mc.fixalpha, mmg_diff_lrt_perm_observed(ph), ph);
        vector<uint8_t> st((size_t)opt.lrt_perms * F);
        MMG_CHECK(mmg_diff_lrt_perm_get_null(ph, 0, (uint32_t)opt.lrt_perms, NULL, st.data()));
        uint64_t bits[3] = {0, 0, 0};
        for (uint8_t v : st)
            for (int k = 0; k < 3; ++k) bits[k] += ((v >> k) & 1) + ((v >> (4 + k)) & 1);
        cerr << "Null of the likelihood-ratio test: " << 2 * st.size() << " fits on " << opt.lrt_perms << " shuffled copies; status bit 1 (cap) on "
             << bits[0] << ", bit 2 (singular) on " << bits[1] << ", bit 4 (boundary) on " << bits[2] << "\n";
    }
    cerr << "Wrote the likelihood-ratio tests of " << F << " features to " << opt.lrt_file << "\n";
}

// the names of the traced parameters in row order; gamma, the last one, only if asked for
vector<string> traced_names(mmg_diff *h, bool with_gamma)
{
    uint32_t np = 0;
    MMG_CHECK(mmg_diff_trace_layout(h, &np, NULL));
    vector<string> names(with_gamma ? np : np - 1);
    for (uint32_t i = 0; i < names.size(); ++i) {
        char name[32];
        MMG_CHECK(mmg_diff_trace_name(h, i, name, sizeof name));
        names[i] = name;
    }
    return names;
}

// -effects FILE, after sampling: the summaries of the rows the handle kept
void write_run_effects(mmg_diff *h, const Options &opt, const Inputs &in, const Model &model)
{
    const size_t F = in.features.size();
    Effects fx;
    fx.names = traced_names(h, false);   // gamma has no effects of its own
    const size_t Q = fx.names.size(), np = opt.effects_pct.size();
    mmg_effects *e = nullptr;
    MMG_CHECK(mmg_diff_effects_summarize(h, (uint32_t)np, opt.effects_pct.data(), &e));
    const Owner<mmg_effects> owner(e, mmg_effects_destroy);
    fx.n.resize(2 * F); fx.n_gt.resize(Q * F);
    fx.mean.resize(Q * F); fx.sd.resize(Q * F); fx.q.resize(Q * np * F);
    MMG_CHECK(mmg_effects_get(e, fx.n.data(), fx.mean.data(), fx.sd.data(), fx.n_gt.data(), fx.q.data()));
    write_effects(opt.effects, in.features, opt.effects_pct, opt.mc.fixalpha, model, fx);
    cerr << "Wrote the effects of " << opt.effects_rows << " rows to " << opt.effects << "\n";
}

// One chain of one comparison, and what only it offers: -lrt ahead of it (or, with -lrtonly, alone), -traces, -effects, and with
// -chains 1 -chainout BASE its table to BASE.chain0.mmdiff as well.
int run_plain(const Options &opt, const Inputs &in, const Model &model)
{
    const Mcmc &mc = opt.mc;
    const Design &D = model.D;
    const size_t S = in.filenames.size(), F = in.features.size();
    OutFiles chain0(1), lrt_out(1);
    if (opt.chainout_given) chain0.open(0, opt.chainout + ".chain0.mmdiff");
    if (opt.lrt_given) lrt_out.open(0, opt.lrt_file);

    // every input is checked: now the device
    require_device();
    if (opt.lrt_given) {
        run_lrt(opt, in, model, lrt_out.f[0]);
        if (opt.lrt_only) return 0;
    }
    mmg_diff *h = nullptr;
    MMG_CHECK(mmg_diff_create(0, (uint32_t)F, (uint32_t)S, in.y.data(), in.e.data(), (uint32_t)D.K, D.M.data(), (uint32_t)D.L0, D.P0.data(),
                              (uint32_t)D.L1, D.P1.data(), D.C.data(), mc.d, mc.s, mc.pdash, mc.fixalpha ? 1 : 0, mc.seed, &h));
    Owner<mmg_diff> owner(h, mmg_diff_destroy);
    unique_ptr<TraceWriter> tw;
    if (!opt.traces.empty()) {
        tw.reset(new TraceWriter(opt.traces, traced_names(h, true), F));
        // a line per burnin / OUTLEN burn-in and per iters / OUTLEN sampling iterations (src/mmdiff.cpp:733-734, 837)
        MMG_CHECK(mmg_diff_trace_open(h, (uint32_t)(mc.burnin / OUTLEN), (uint32_t)(mc.iters / OUTLEN), TraceWriter::sink, tw.get()));
    }
    if (!opt.effects.empty()) MMG_CHECK(mmg_diff_effects_open(h, (uint32_t)opt.effects_every, opt.effects_rows));
    cerr << "BURNIN (" << mc.burnin << " iterations)...";
    MMG_CHECK(mmg_diff_burnin(h, (uint32_t)mc.burnin));
    cerr << "\nSetting pseudopriors...done.\n";
    vector<double> mean_lo, tune_logitp;
    if (tw) {
        uint32_t nq = 0, nc[2] = {0, 0};
        MMG_CHECK(mmg_diff_trace_layout(h, NULL, &nq));
        MMG_CHECK(mmg_diff_info(h, NULL, nc, NULL));
        vector<double> cols((size_t)nq * F);
        MMG_CHECK(mmg_diff_get_pseudo(h, cols.data()));
        const size_t L[2] = {D.L0, D.L1};
        tw->pseudo(D.K, L, nc, cols);
        mean_lo.resize(F);
        tune_logitp.resize(F);
    }
    int numbatches = 0;
    if (mc.tune) {
        uint32_t untuned = 0;
        MMG_CHECK(mmg_diff_tune_batch(h, &untuned));
        numbatches = 1;
        while (untuned > 0 && numbatches != MAXBATCHES) {
            if (tw) {   // BMS::printtune at the start of a batch, before its tuning step
                MMG_CHECK(mmg_diff_get_tune_state(h, mean_lo.data(), tune_logitp.data()));
                tw->tune_line(mean_lo, tune_logitp);
            }
            MMG_CHECK(mmg_diff_tune_batch(h, &untuned));
            numbatches++;
            if (numbatches % 64 == 0) cerr << "TUNING BATCH " << numbatches << " (" << untuned << " left)\r";
        }
    }
    cerr << "TRACE (" << mc.iters << " iterations, sampling after " << numbatches << " tuning batches)";
    MMG_CHECK(mmg_diff_sample(h, (uint32_t)mc.iters));
    cerr << "\nDONE MCMC\n";
    DiffResults r(F, D);
    MMG_CHECK(mmg_diff_get_results(h, r.gm.data(), r.logitp.data(), r.alpha.data(), r.beta.data(), r.eta.data()));
    if (!opt.effects.empty()) write_run_effects(h, opt, in, model);
    owner.reset();
    if (tw) {
        if (!tw->finish()) die("Error: couldn't write the trace files in " + opt.traces);
        cerr << "Wrote " << tw->bytes << " bytes of traces to " << opt.traces << "\n";
    }
    string text;
    write_table(stdout, chain0.f[0] ? &text : nullptr, in, model, mc, r);
    if (chain0.f[0] && fputs(text.c_str(), chain0.f[0]) < 0) die("Error: couldn't write " + chain0.names[0]);
    chain0.flush(0);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    Options opt = parse_args(argc, argv);
    check_combinations(opt);
    if (opt.polyclass_mode) return run_polyclass(opt);
    check_run(opt);
    const Inputs in = load_inputs(opt);
    const size_t S = in.filenames.size();

    Model model;
    if (opt.matrices_files.empty()) model.D = de_design(opt.simple_de, S);
    else if (!opt.poly_run()) parse_matrices(opt.matrices_files[0], model.D, S);
    if (opt.mc.fixalpha) cerr << "Fixing alpha=0, so setting v_beta^2=25 instead of 4.\n";
    if (opt.poly_run()) return run_poly(opt, in);
    validate_design(model.D, S, opt.mc.fixalpha, model.Mnil, model.Pnil);
    if (opt.chains > 1) return run_chains(opt, in, model);
    if (opt.perms_given) return run_perm(opt, in, model);
    return run_plain(opt, in, model);
}
