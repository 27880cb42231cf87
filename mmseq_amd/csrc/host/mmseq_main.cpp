// mmseq -- drop-in for the reference's `mmseq` CLI (src/mmseq.cpp:179-1728) with the Gibbs loop
// (and the EM that seeds it) running on MI355X through libmmgibbs' C ABI (include/mmgibbs.h).
//
//   Usage: mmseq [OPTIONS...] hits_file output_base          (same flags as src/mmseq.cpp:156-177)
//
// What is the same as the reference: flags, validation and exit codes (:183-299), hits-file input
// (hitsio), transcript / hit-set index order (:395-441), every output file, its column names, row
// order and default 6-significant-digit formatting (:682-695, :823-831, :1033-1108, :1469-1669).
// What differs on purpose: random numbers come from keyed Philox streams (results do not depend on
// a thread count, cf. :834-838), the per-iteration "\r" progress line is throttled (:852), traces
// are written after the loop from the device-resident trace, VLAs are heap vectors (:1308-1348).
// There is no CPU sampler here: without a HIP device the program stops with an error.
#include <omp.h>
#include "cpu_quota.hpp"
#include <atomic>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <charconv>
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/mmgibbs.h"
#include "auto_rule.hpp"
#include "contrasts_file.hpp"
#include "iso_thresholds.hpp"
#include "hitsio.hpp"
#include "huffenc.hpp"
#include "numerics.hpp"
#include "pairs_gen.hpp"
#include "stage_timer.hpp"

#ifndef MMSEQ_VERSION
#define MMSEQ_VERSION "1.0.11-mi355x"
#endif

using namespace std;

static void printUsage(ostream &out)
{
    out << "Usage: mmseq [OPTIONS...] hits_file output_base" << endl
        << endl
        << "Mandatory arguments:" << endl
        << "  hits_file          hits file generated with `bam2hits`\n"
        << "  output_base        base name for output files" << endl
        << endl
        << "Optional arguments:\n"
        << "  -alpha FLOAT       value of alpha in Gamma prior for mu (default: 0.1)" << endl
        << "  -beta FLOAT        value of beta in Gamma prior for mu (default: 0.1)" << endl
        << "  -max_em_iter INT   maximum number of EM iterations (default: 1000)" << endl
        << "  -epsilon FLOAT     minimum loglik ratio between successive EM iterations (default: 0.1)" << endl
        << "  -gibbs_iter INT    number of Gibbs iterations (default: 16384)" << endl
        << "  -gibbs_ss INT      subsampling interval for Gibbs output (default: gibbs_iter/1024)" << endl
        << "  -seed INT          seed for the PRNG in thread 0 (default: 1234).  A 32-bit signed integer, sign-extended to the 64-bit key" << endl
        << "                     of the random streams: -seed -7 is the library's seed 2^64 - 7, not 7" << endl
        << "  -percentiles STR   comma-separated list of real-scale marginal posterior percentiles to output (default: "
           "\"5,25,50,75,95\")"
        << endl
        << "  -debug             output additional diagnostic files" << endl
        << "  -help              print this help message" << endl
        << "  -version           print the version" << endl
        << "  -device INT        first HIP device to run on (default: 0)        [MI355X build]" << endl
        << "  -gpus INT          number of devices, device .. device+gpus-1 (default: 1).  With one chain the reads are sharded" << endl
        << "                     over them (same results as on one device); with -chains >= gpus every device runs chains/gpus chains" << endl
        << "  -chains INT        independent Gibbs chains (default: 1); log_mu, sd and mcse pool all chains, traces are chain 0's" << endl
        << "  -em_one_device     with -gpus > 1 and one chain: run the EM on the first device alone instead of over the read shards" << endl
        << "  -convergence       also write output_base.convergence, .identical.convergence and .gene.convergence: rank-normalized" << endl
        << "                     split R-hat and bulk / tail effective sample sizes across the chains (one device only)" << endl
        << "  -pool              with -chains: every column of .mmseq, .identical.mmseq and .gene.mmseq -- log_mu, sd, mcse, iact, the percentiles," << endl
        << "                     the proportion columns -- from the kept samples of all chains instead of chain 0's.  log_mu is then the mean of" << endl
        << "                     log mu over the kept samples (without -pool, -chains takes it from the sampler's running moments over every" << endl
        << "                     iteration).  Trace files, -assign and -contrasts stay chain 0's (one device only)" << endl
        << "  -assign            also write output_base.assign (the lines of output_base.M with the posterior probability that the hit set's" << endl
        << "                     reads come from that transcript), .counts and .gene.counts (expected hits per feature; one device only)" << endl
        << "  -contrasts FILE    also write output_base.contrasts.mmseq: per line `name<TAB>id,id,...<TAB>id,id,...` of FILE the posterior of" << endl
        << "                     log(sum of mu over the first ids / sum over the second) from chain 0's samples (one device only)" << endl
        << "  -pairs             also write output_base.pairs: for every two transcripts that share a hit set the posterior correlation of" << endl
        << "                     their log mu, the sd of each and of the log of their sum, from chain 0's samples (one device only)" << endl
        << "  -pairs_maxset INT  with -pairs: hit sets of more transcripts than this contribute no pairs (default: 16)" << endl
        << "  -isoforms          also write output_base.isoforms and output_base.gene.isoforms: per gene, from the joint draws of its isoforms" << endl
        << "                     in chain 0's samples, the probability that each isoform is the major one, the entropy of the usage and the" << endl
        << "                     share of the top isoform (one device only)" << endl
        << "  -iso_thresholds STR  with -isoforms: comma-separated shares of the gene in [0, 1), at most 8; per isoform the probability that" << endl
        << "                     it carries more than each (default: \"0.1,0.5\")" << endl
        << "  -gibbs_auto MAX    run gibbs_iter iterations, judge the transcripts' R-hat and effective sample sizes across the chains, and" << endl
        << "                     double the run (bit for bit the run planned that long) until -auto_frac of them meet the targets or twice" << endl
        << "                     the length would pass MAX (gibbs_iter times a power of 2, at most 2^30).  Also writes output_base.autolength;" << endl
        << "                     every other output is that of -gibbs_iter L for the length L it stopped at (one device only)" << endl
        << "  -auto_ess FLOAT    with -gibbs_auto: least bulk and tail effective sample size of a transcript that passes (default: 400)" << endl
        << "  -auto_rhat FLOAT   with -gibbs_auto: largest R-hat of a transcript that passes (default: 1.01)" << endl
        << "  -auto_frac FLOAT   with -gibbs_auto: share of the judged transcripts that must pass, in (0, 1] (default: 0.99)" << endl
        << endl;
}

// the fields of `text` between separators (empty fields dropped)
static vector<string> split_fields(const string &text, char sep)
{
    vector<string> out;
    string cur;
    for (char ch : text) {
        if (ch != sep) { cur += ch; continue; }
        if (!cur.empty()) out.push_back(cur);
        cur.clear();
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

static bool is_power_of_two(unsigned v) { return v != 0 && (v & (v - 1)) == 0; }

// Command line: a table of options -- name, the variable it sets, how its value is read -- walked once.  Same flags, defaults,
// messages and exit codes as the reference's loop at src/mmseq.cpp:206-276 (tests/test_cli.py holds them), plus -device / -gpus /
// -chains / -em_one_device / -convergence / -pool / -assign / -contrasts / -pairs / -pairs_maxset of this build.
struct CliOption {
    const char *name;
    enum Kind { REAL, INT, FLAG, LIST, TEXT, HELP, VERSION } kind;
    void *target;
};

// The one error path.  A failure on the main thread prints its message where it happens and throws Exit; main() catches it and
// returns the code.  Unwinding does the cleanup, in the reverse order of run()'s declarations: the trace writers are stopped and
// joined (TraceWriters), the library handles destroyed, the .k / .M writer joined (the reference has written both by then,
// src/mmseq.cpp:682-695) and last the device warm-up thread.  Exit never crosses an OpenMP region or leaves a thread's body.
struct Exit { int code; };
[[noreturn]] static void leave_with(const string &text) { cerr << text; throw Exit{1}; }
[[noreturn]] static void fatal(const string &msg) { leave_with("Error: " + msg + "\n"); }
#define MMG_TRY(expr)                                                                     \
    do {                                                                                  \
        if ((expr) != 0) fatal(std::string(mmg_last_error()) + " (" + #expr + ")");        \
    } while (0)

// a library handle, destroyed with its *_destroy when its owner goes
template <class T, void (*Destroy)(T *)> struct Destroyer { void operator()(T *p) const { Destroy(p); } };
template <class T, void (*Destroy)(T *)> using Owned = unique_ptr<T, Destroyer<T, Destroy>>;
using Problem = Owned<mmg_problem, mmg_problem_destroy>;
using Group = Owned<mmg_group, mmg_group_destroy>;
using Summary = Owned<mmg_summary, mmg_summary_destroy>;
using Convergence = Owned<mmg_convergence, mmg_convergence_destroy>;
using PooledSummary = Owned<mmg_pooled, mmg_pooled_destroy>;
using Assign = Owned<mmg_assign, mmg_assign_destroy>;
using Contrast = Owned<mmg_contrast, mmg_contrast_destroy>;
using Pairs = Owned<mmg_pairs, mmg_pairs_destroy>;
using Isoform = Owned<mmg_isoform, mmg_isoform_destroy>;
// handles of one kind, one per device, destroyed together in order; reads as the array of raw handles the calls take
template <class T, void (*Destroy)(T *)> struct HandleSet {
    vector<T *> h;
    explicit HandleSet(size_t count = 0) : h(count, nullptr) {}
    HandleSet(HandleSet &&o) noexcept : h(std::move(o.h)) { o.h.clear(); }
    ~HandleSet() { for (T *p : h) if (p) Destroy(p); }
    T **data() { return h.data(); }
    T *const *data() const { return h.data(); }
    T *&operator[](size_t i) { return h[i]; }
    T *operator[](size_t i) const { return h[i]; }
    typename vector<T *>::const_iterator begin() const { return h.begin(); }
    typename vector<T *>::const_iterator end() const { return h.end(); }
};
using Problems = HandleSet<mmg_problem, mmg_problem_destroy>;
using Samplers = HandleSet<mmg_sampler, mmg_sampler_destroy>;
using Ems = HandleSet<mmg_em, mmg_em_destroy>;

// a thread joined when it goes out of scope: on success, and while an Exit unwinds
struct JoiningThread {
    thread t;
    JoiningThread() = default;
    template <class F> explicit JoiningThread(F &&f) : t(std::forward<F>(f)) {}
    JoiningThread(JoiningThread &&) = default;
    ~JoiningThread() { join(); }
    void join() { if (t.joinable()) t.join(); }
};

// The trace writers and what they share with the main thread.  Worker threads (the writers and their fetchers) never throw and never
// call exit(): exit() runs the atexit handlers and the HIP / RCCL teardown under the main thread's feet.  A worker RECORDS its error
// (first one wins) and returns; the main thread sees it (check) and leaves with the message.  Going out of scope -- on success after
// finish(), or while an Exit unwinds -- stops the workers (flag, wake) and joins them, before the summary and samplers they read go.
struct TraceWriters {
    mutex mu;
    condition_variable cv;
    int samples_ready = 0;        // samples whose rows may be fetched (trace and derived traces)
    atomic<bool> stop{false};     // a worker failed or the main thread is leaving: every worker returns
    string failure;               // the first worker's error
    vector<JoiningThread> threads; // (the last member: joined before the rest goes)
    ~TraceWriters() { { lock_guard<mutex> lk(mu); stop.store(true); } cv.notify_all(); }
    void record(const string &msg) { { lock_guard<mutex> lk(mu); if (failure.empty()) failure = msg; stop.store(true); } cv.notify_all(); }
    bool failed(int rc, const char *what) { if (rc != 0) record(string(mmg_last_error()) + " (" + what + ")"); return rc != 0; }
    void wait_for(int upto) { unique_lock<mutex> lk(mu); cv.wait(lk, [&] { return samples_ready >= upto || stop.load(); }); }
    void publish(int ready) { { lock_guard<mutex> lk(mu); samples_ready = ready; } cv.notify_all(); }
    void check() { string msg; { lock_guard<mutex> lk(mu); msg = failure; } if (!msg.empty()) fatal(msg); } // (main thread)
    void finish() { for (auto &t : threads) t.join(); check(); }
};

// gzip text sink: ONE standard gzip member whose deflate stream is produced chunk-wise in parallel.
// Every chunk is compressed independently as raw deflate and closed with a sync flush (byte-aligned,
// no dictionary carried over), so the concatenation is a valid deflate stream; the CRCs are merged with
// crc32_combine.  Any gzip reader (zlib, Boost gzip_decompressor of mmcollapse, R) reads it unchanged.
// Numbers are formatted with "%g" == default ostream formatting (6 significant digits).
// "%g" (6 significant digits, what the reference's default ostream formatting prints) without going through printf:
// to_chars(general, 6) is specified to produce exactly the %.6g digits; nan/inf keep printf's spelling.
static inline int fmt_g(char *tmp, double v)
{
    if (!(v - v == 0.0)) return snprintf(tmp, 40, "%g", v);
    auto r = to_chars(tmp, tmp + 39, v, chars_format::general, 6);
    return (int)(r.ptr - tmp);
}

// Trace files are megabytes of 6-digit numbers: deflate level 6 (the reference's Boost default) manages 12 MB/s per core on
// them, level 1 73 MB/s for files 11 % larger, Huffman coding alone (such text has next to no repeats for LZ77 to find) 110 MB/s for
// another 3 %.  Huffman-only unless MMSEQ_GZIP_LEVEL asks for a level (default strategy then); any gzip reader reads all of them.
// The Huffman-only blocks are written by host/huffenc.hpp (4.4 x zlib's rate for them: with zlib the trace writers needed more CPUs
// than a 16-CPU quota leaves next to the .M writer, and finished a second after the chain).
static int gzip_level()
{
    static const int level = [] { const char *e = getenv("MMSEQ_GZIP_LEVEL"); const int v = e ? atoi(e) : 1; return v >= 0 && v <= 9 ? v : 1; }();
    return level;
}
static int gzip_strategy()
{
    static const int strategy = getenv("MMSEQ_GZIP_LEVEL") ? Z_DEFAULT_STRATEGY : Z_HUFFMAN_ONLY;
    return strategy;
}

struct GzText {
    FILE *f = nullptr;
    uLong crc = 0;
    unsigned long long total = 0;
    string pending; // small writes are gathered here and compressed on flush
    explicit GzText(const string &path) // (a file that cannot be opened: !ok(), the caller reports it)
    {
        f = fopen(path.c_str(), "wb");
        if (!f) return;
        const unsigned char hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
        fwrite(hdr, 1, 10, f);
        crc = crc32(0L, Z_NULL, 0);
    }
    GzText(const GzText &) = delete;
    ~GzText() { if (f) fclose(f); }
    bool ok() const { return f != nullptr; }
    static string deflate_chunk(const string &in, bool last)
    {
        if (!last && gzip_strategy() == Z_HUFFMAN_ONLY) { // the default: host/huffenc.hpp, the same kind of block several times faster
            string out;
            if (huffenc::deflate_literals(in.data(), in.size(), out)) return out;
        }
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, gzip_level(), Z_DEFLATED, -15, 8, gzip_strategy()) != Z_OK) {
            cerr << "Error initialising zlib.\n";
            exit(1);
        }
        string out;
        out.resize(deflateBound(&zs, (uLong)in.size()) + 16);
        zs.next_in = (Bytef *)in.data();
        zs.avail_in = (uInt)in.size();
        zs.next_out = (Bytef *)&out[0];
        zs.avail_out = (uInt)out.size();
        deflate(&zs, last ? Z_FINISH : Z_SYNC_FLUSH);
        out.resize(out.size() - zs.avail_out);
        deflateEnd(&zs);
        return out;
    }
    // already deflated pieces (deflate_chunk of consecutive text), their crc32s and text sizes, appended in order
    void append_compressed(const vector<string> &comp, const vector<uLong> &crcs, const vector<size_t> &sizes)
    {
        for (size_t i = 0; i < comp.size(); ++i) {
            fwrite(comp[i].data(), 1, comp[i].size(), f);
            crc = crc32_combine(crc, crcs[i], (z_off_t)sizes[i]);
            total += sizes[i];
        }
    }
    void flush_pending()
    {
        if (pending.empty()) return;
        string c = deflate_chunk(pending, false);
        fwrite(c.data(), 1, c.size(), f);
        crc = crc32(crc, (const Bytef *)pending.data(), (uInt)pending.size());
        total += pending.size();
        pending.clear();
    }
    void str(const string &s) { pending += s; if (pending.size() > (1u << 24)) flush_pending(); }
    void num(double v)
    {
        char tmp[40];
        pending.append(tmp, fmt_g(tmp, v));
    }
    void close()
    {
        flush_pending();
        const string fin = deflate_chunk(string(), true); // final (empty) block
        fwrite(fin.data(), 1, fin.size(), f);
        unsigned char tr[8];
        const uint32_t c = (uint32_t)crc, n = (uint32_t)(total & 0xffffffffull);
        for (int i = 0; i < 4; ++i) { tr[i] = (unsigned char)(c >> (8 * i)); tr[4 + i] = (unsigned char)(n >> (8 * i)); }
        fwrite(tr, 1, 8, f);
        fclose(f);
        f = nullptr;
    }
};

// Rows of n numbers, each followed by a space, one line per sample (src/mmseq.cpp:912-916), from rows fetched on demand (the trace
// lives on the device, sample-major: a line of the file is a row there).  Three things overlap: the fetch of the next round of rows
// (device gather + copy), the formatting and compression of this round -- in parallel over pieces of <= 32 k columns of a line
// (~ 290 KB of text each, deflated independently and joined with sync flushes) -- and the write of the previous round's bytes.
static void write_trace_rows(GzText &gz, int n_lines, size_t n_cols, const function<void(int, int, double *)> &fetch,
                             const function<bool(size_t)> &keep, const atomic<bool> &stop, int threads)
{
    vector<char> mask(n_cols);
    size_t n_keep = 0;
    for (size_t c = 0; c < n_cols; ++c) n_keep += (mask[c] = keep(c) ? 1 : 0);
    if (n_keep == 0) { for (int i = 0; i < n_lines; ++i) gz.str("\n"); return; }
    const size_t cols_per_piece = 32768, pieces_per_line = (n_cols + cols_per_piece - 1) / cols_per_piece;
    const size_t want_pieces = (size_t)threads * 2;
    size_t lines_per_round = max<size_t>((size_t)(64u << 20) / (n_cols * 8), (want_pieces + pieces_per_line - 1) / pieces_per_line);
    lines_per_round = max<size_t>(1, min<size_t>({lines_per_round, (size_t)(512u << 20) / (n_cols * 8) + 1, (size_t)n_lines}));
    vector<double> buf[2];
    buf[0].resize(lines_per_round * n_cols);
    buf[1].resize(lines_per_round * n_cols);
    gz.flush_pending();
    fetch(0, (int)min<size_t>(lines_per_round, (size_t)n_lines), buf[0].data());
    thread writer;
    vector<string> comp_prev; // owned by the writer thread while it runs
    for (int l0 = 0, r = 0; l0 < n_lines && !stop.load(); l0 += (int)lines_per_round, ++r) {
        const int cnt = (int)min<size_t>(lines_per_round, (size_t)(n_lines - l0));
        const int next0 = l0 + cnt, next_cnt = (int)min<size_t>(lines_per_round, (size_t)max(0, n_lines - next0));
        thread fetcher;
        if (next_cnt > 0) fetcher = thread([&, next0, next_cnt, r]() { fetch(next0, next_cnt, buf[(r + 1) & 1].data()); });
        const double *rows = buf[r & 1].data();
        const int64_t n_pieces = (int64_t)cnt * (int64_t)pieces_per_line;
        vector<string> comp((size_t)n_pieces);
        vector<uLong> crcs((size_t)n_pieces);
        vector<size_t> sizes((size_t)n_pieces);
#pragma omp parallel num_threads(threads)
        {
            string text;
            char tmp[48];
#pragma omp for schedule(dynamic, 1)
            for (int64_t pc = 0; pc < n_pieces; ++pc) {
                const size_t line = (size_t)pc / pieces_per_line, piece = (size_t)pc % pieces_per_line;
                const size_t c0 = piece * cols_per_piece, c1 = min(n_cols, c0 + cols_per_piece);
                const double *row = rows + line * n_cols;
                text.clear();
                for (size_t c = c0; c < c1; ++c) {
                    if (!mask[c]) continue;
                    int len = fmt_g(tmp, row[c]);
                    tmp[len++] = ' ';
                    text.append(tmp, (size_t)len);
                }
                if (piece + 1 == pieces_per_line) text += "\n";
                comp[(size_t)pc] = GzText::deflate_chunk(text, false);
                crcs[(size_t)pc] = crc32(crc32(0L, Z_NULL, 0), (const Bytef *)text.data(), (uInt)text.size());
                sizes[(size_t)pc] = text.size();
            }
        }
        if (writer.joinable()) writer.join();
        comp_prev.swap(comp);
        writer = thread([&gz, &comp_prev, crcs, sizes]() { gz.append_compressed(comp_prev, crcs, sizes); });
        if (fetcher.joinable()) fetcher.join();
    }
    if (writer.joinable()) writer.join();
}

// the sample count of every trace (src/mmseq.cpp:187: gibbs_iter / gibbs_ss)
constexpr int trace_length = 1024;

struct Options {
    // DEFAULT PARAMETER VALUES (src/mmseq.cpp:183-205)
    double alpha = 0.1, beta = 0.1;
    int max_em_iter = 1000;
    double epsilon = 0.1;
    int gibbs_iter = 16384;
    int gibbs_ss = gibbs_iter / trace_length;
    vector<double> percentiles = {5.0, 25.0, 50.0, 75.0, 95.0};
    int seed = 1234;
    bool debug = false;
    int device = 0, gpus = 1, chains = 1;
    bool em_one_device = false, convergence = false, assign = false, pool = false;
    string contrasts_file;
    bool pairs = false;
    int pairs_maxset = 16;
    bool isoforms = false;
    vector<double> iso_thresholds = {0.1, 0.5};
    // -gibbs_auto: the run is doubled from gibbs_iter until the rule of host/auto_rule.hpp holds or twice the length would pass gibbs_auto
    bool auto_on = false;
    int gibbs_auto = 0;
    autolen::Targets auto_targets;
    string hits_file, output_base;
};

// the flags and their checks; a bad command line leaves here (no thread runs yet)
static Options parse_options(int argc, char **argv)
{
    Options o;
    vector<string> percentile_fields;
    string iso_thresholds_text;
    bool iso_thresholds_given = false, auto_target_given = false;
    const CliOption options[] = {
        {"-alpha", CliOption::REAL, &o.alpha},        {"-beta", CliOption::REAL, &o.beta},
        {"-max_em_iter", CliOption::INT, &o.max_em_iter}, {"-epsilon", CliOption::REAL, &o.epsilon},
        {"-gibbs_iter", CliOption::INT, &o.gibbs_iter},   {"-gibbs_ss", CliOption::INT, &o.gibbs_ss},
        {"-seed", CliOption::INT, &o.seed},           {"-device", CliOption::INT, &o.device},
        {"-gpus", CliOption::INT, &o.gpus},           {"-chains", CliOption::INT, &o.chains},
        {"-percentiles", CliOption::LIST, &percentile_fields},
        {"-debug", CliOption::FLAG, &o.debug},        {"-em_one_device", CliOption::FLAG, &o.em_one_device},
        {"-convergence", CliOption::FLAG, &o.convergence}, {"-assign", CliOption::FLAG, &o.assign},
        {"-contrasts", CliOption::TEXT, &o.contrasts_file}, {"-pool", CliOption::FLAG, &o.pool},
        {"-pairs", CliOption::FLAG, &o.pairs},        {"-pairs_maxset", CliOption::INT, &o.pairs_maxset},
        {"-isoforms", CliOption::FLAG, &o.isoforms},  {"-iso_thresholds", CliOption::TEXT, &iso_thresholds_text},
        {"-gibbs_auto", CliOption::INT, &o.gibbs_auto},   {"-auto_ess", CliOption::REAL, &o.auto_targets.ess},
        {"-auto_rhat", CliOption::REAL, &o.auto_targets.rhat}, {"-auto_frac", CliOption::REAL, &o.auto_targets.frac},
        {"-h", CliOption::HELP, nullptr},          {"-help", CliOption::HELP, nullptr},       {"--help", CliOption::HELP, nullptr},
        {"-v", CliOption::VERSION, nullptr},        {"-version", CliOption::VERSION, nullptr}, {"--version", CliOption::VERSION, nullptr},
    };
    auto usage_error = [&](const string &msg) { cerr << msg << "\n"; printUsage(cerr); exit(1); };
    int pos = 1;                                   // next word of the command line
    for (;;) {
        const CliOption *opt = nullptr;
        if (pos < argc) for (const CliOption &op : options) if (strcmp(argv[pos], op.name) == 0) opt = &op;
        if (!opt) {                                // not an option: exactly the two positional arguments must be left
            if (argc - pos == 2) break;
            if (pos < argc && argv[pos][0] == '-') usage_error(string("Error: unrecognised option ") + argv[pos] + ".");
            usage_error("Error: mandatory arguments missing.");
        }
        if (opt->kind == CliOption::HELP) { cerr << "Calculate mmseq expression estimates.\n"; printUsage(cerr); exit(1); } // exit code 1, as src/mmseq.cpp:256-259
        if (opt->kind == CliOption::VERSION) { cerr << "mmseq-" << MMSEQ_VERSION << endl; exit(1); }
        if (opt->kind == CliOption::FLAG) { *(bool *)opt->target = true; pos += 1; continue; }
        if (pos + 1 >= argc) usage_error("Error: mandatory arguments missing.");
        const char *value = argv[pos + 1];
        if (opt->target == &o.gibbs_auto) o.auto_on = true;
        if (strncmp(opt->name, "-auto_", 6) == 0) { // (a value that is no number is NaN: refused by the checks below)
            auto_target_given = true;
            char *end = nullptr;
            const double v = strtod(value, &end);
            *(double *)opt->target = end == value || *end != '\0' ? NAN : v;
        } else
        if (opt->kind == CliOption::REAL) *(double *)opt->target = strtod(value, NULL);
        else if (opt->kind == CliOption::INT) *(int *)opt->target = atoi(value);
        else if (opt->kind == CliOption::TEXT) { *(string *)opt->target = value; if (opt->target == &iso_thresholds_text) iso_thresholds_given = true; }
        else *(vector<string> *)opt->target = split_fields(value, ',');
        pos += 2;
    }
    if (!percentile_fields.empty()) {
        o.percentiles.resize(percentile_fields.size());
        for (size_t i = 0; i < percentile_fields.size(); i++) {
            const double v = strtod(percentile_fields[i].c_str(), NULL);
            if (!(v >= 0 && v <= 100)) { cerr << "Percentiles must be in (0,100)\n"; exit(1); }
            o.percentiles[i] = v;
        }
    }
    o.hits_file = argv[pos];
    o.output_base = argv[pos + 1];
    auto check = [](bool ok, const string &msg) { if (!ok) { cerr << msg; printUsage(cerr); exit(1); } };
    check(o.gibbs_ss != 0 && o.gibbs_iter % o.gibbs_ss == 0, "Error: gibbs_iter must be divisible by gibbs_ss.\n"); // :278 (gibbs_ss == 0 is a division by zero there)
    o.gibbs_ss = o.gibbs_iter / trace_length; // :284 -- the user's -gibbs_ss is overwritten, as in the reference
    check(o.gibbs_iter > 0 && trace_length > 0, "Error: no. of iteratons or trace length <= 0. Possible integer overflow - is gibbs_iter too high?\n");
    // the reference overruns its trace / divides by zero here (App. A)
    check(o.gibbs_ss >= 1 && o.gibbs_iter % trace_length == 0, "Error: gibbs_iter must be a positive multiple of " + to_string(trace_length) + ".\n");
    check(o.gpus >= 1 && o.chains >= 1 && !(o.gpus > 1 && o.chains > 1 && o.chains % o.gpus != 0),
          "Error: -gpus and -chains must be positive, and chains a multiple of gpus when both exceed 1.\n");
    // the diagnostic reads every chain's trace on one device
    check(!(o.convergence && o.gpus > 1), "Error: -convergence needs every chain on one device: it cannot be combined with -gpus > 1.\n");
    // the pooled summary reads every chain's trace on one device
    check(!(o.pool && o.gpus > 1), "Error: -pool needs every chain on one device: it cannot be combined with -gpus > 1.\n");
    // the pass reads the chain's trace where one sampler holds it
    check(!(o.assign && o.gpus > 1), "Error: -assign reads the chain's trace on one device: it cannot be combined with -gpus > 1.\n");
    // the pass reads chain 0's trace where one sampler holds it
    check(!(!o.contrasts_file.empty() && o.gpus > 1), "Error: -contrasts reads the chain's trace on one device: it cannot be combined with -gpus > 1.\n");
    check(!(o.pairs && o.gpus > 1), "Error: -pairs reads the chain's trace on one device: it cannot be combined with -gpus > 1.\n");
    check(o.pairs_maxset >= 2, "Error: -pairs_maxset must be at least 2.\n");
    // the pass reads chain 0's trace where one sampler holds it, a group's samples in the lanes of one wave and the LDS of one workgroup
    check(!(o.isoforms && o.gpus > 1), "Error: -isoforms reads the chain's trace on one device: it cannot be combined with -gpus > 1.\n");
    check(!(o.isoforms && trace_length > 4096), "Error: -isoforms takes traces of at most 4096 samples.\n");
    check(!(iso_thresholds_given && !o.isoforms), "Error: -iso_thresholds needs -isoforms.\n");
    if (iso_thresholds_given) {
        string error;
        const bool parsed = isocli::parse_thresholds(iso_thresholds_text, o.iso_thresholds, error);
        check(parsed, "Error: " + error + "\n");
    }
    check(is_power_of_two((unsigned)trace_length), "Error: gibbs_iter/gibbs_ss must be a power of 2.\n");
    check(!(auto_target_given && !o.auto_on), "Error: -auto_ess, -auto_rhat and -auto_frac need -gibbs_auto.\n");
    if (o.auto_on) {
        // the run is extended on the one sampler that holds every chain
        check(o.gpus == 1, "Error: -gibbs_auto extends the chains on one device: it cannot be combined with -gpus > 1.\n");
        check(o.gibbs_auto <= (1 << 30), "Error: -gibbs_auto must be at most 2^30 = 1073741824.\n");
        check(o.gibbs_auto >= o.gibbs_iter && o.gibbs_auto % o.gibbs_iter == 0 && is_power_of_two((unsigned)(o.gibbs_auto / o.gibbs_iter)),
              "Error: -gibbs_auto must be gibbs_iter times a power of 2 (gibbs_iter, 2 gibbs_iter, 4 gibbs_iter, ...).\n");
        check(o.auto_targets.ess > 0.0, "Error: -auto_ess must be a number > 0.\n");
        check(o.auto_targets.rhat > 1.0, "Error: -auto_rhat must be a number > 1.\n");
        check(o.auto_targets.frac > 0.0 && o.auto_targets.frac <= 1.0, "Error: -auto_frac must be a number in (0, 1].\n");
    }
    return o;
}

// ---- header (src/mmseq.cpp:332-379)
struct Header {
    map<string, double> sidLen;
    map<string, int> sidSeqLen;
    vector<string> transcriptList;
    map<string, vector<string>> gene2transcripts;
    vector<vector<string>> identical_transcripts;
    map<string, string> transcript2gene;
    // (lookups that never insert: the table writers run in several threads; a name the header did not describe reads as 0, which
    // is what the maps' operator[] would have inserted)
    double len_of(const string &name) const { auto it = sidLen.find(name); return it == sidLen.end() ? 0.0 : it->second; }
    int seqlen_of(const string &name) const { auto it = sidSeqLen.find(name); return it == sidSeqLen.end() ? 0 : it->second; }
    size_t gene_size_of(const string &name) const
    {
        auto tg = transcript2gene.find(name);
        auto it = gene2transcripts.find(tg == transcript2gene.end() ? string() : tg->second);
        return it == gene2transcripts.end() ? (size_t)0 : it->second.size();
    }
};

static Header read_header(HitsfileReader &reader)
{
    Header h;
    reader.readHeader(&h.transcriptList, &h.sidLen, &h.sidSeqLen, &h.gene2transcripts, &h.identical_transcripts);
    vector<string> transcriptListGI;
    for (auto &g : h.gene2transcripts)
        for (auto &t : g.second) {
            if (h.transcript2gene.count(t) > 0) leave_with("Error: transcripts must be nested within genes in GeneIsoforms metadata.\n");
            transcriptListGI.push_back(t);
            h.transcript2gene[t] = g.first;
        }
    vector<string> a = h.transcriptList, b = transcriptListGI;
    sort(a.begin(), a.end());
    sort(b.begin(), b.end());
    if ((size_t)(unique(a.begin(), a.end()) - a.begin()) != h.transcriptList.size())
        leave_with("Error: duplicate transcripts in @TranscriptMetaData entries.\n");
    if ((size_t)(unique(b.begin(), b.end()) - b.begin()) != transcriptListGI.size())
        leave_with("Error: duplicate transcripts in @GeneIsoforms entries.\n");
    for (auto &t : h.transcriptList)
        if (h.transcript2gene.count(t) == 0) leave_with("Error: " + t + " does not belong to a gene in the @GeneIsoforms header entries.\n");
    return h;
}

// the collapsed hits: one row per distinct hit set (first-seen order), its columns the observed transcripts it hits
struct Hits {
    vector<uint32_t> obs2hdr;             // indexSid: observed index -> header index
    vector<int> doublehits;
    vector<uint32_t> k;                   // multiplicity per hit set
    vector<uint64_t> row_ptr = {0};       // hit sets in first-seen order
    vector<uint32_t> col_idx;
    long long numbermappedreads = 0;
    uint32_t n() const { return (uint32_t)obs2hdr.size(); }
    uint64_t m() const { return k.size(); }
};

// ---- READ LOOP (src/mmseq.cpp:395-441): transcript index = first-seen order, row = first-seen hit set
static Hits ingest(HitsfileReader &hitsfileReader, const string &hits_file, size_t nHeader, bool timing)
{
    Hits H;
    vector<uint32_t> &obs2hdr = H.obs2hdr, &k = H.k, &col_idx = H.col_idx;
    vector<uint64_t> &row_ptr = H.row_ptr;
    vector<int32_t> hdr2obs(nHeader, -1); // header index -> observed index
    // hit set -> row: open-addressing table keyed by a 64-bit hash of the sorted set; an entry is (upper hash half, row id), a
    // candidate whose tag matches is confirmed against the stored row itself, so there is no per-set key allocation
    // (src/mmseq.cpp:395-441 keeps a map<vector<int>,int> and regrows M).  The stage is bound by cache misses (one table line
    // per read, the stored row for a repeat): the slot of a read a dozen ahead is prefetched, and the table starts at the size
    // the file suggests (a record is >= 16 compressed bytes) instead of being rebuilt at every doubling.
    constexpr uint64_t EMPTY = ~0ull;
    size_t table_size = 1u << 16;
    struct stat st_;
    const uint64_t fsz = stat(hits_file.c_str(), &st_) == 0 ? (uint64_t)st_.st_size : 0;
    while (table_size < fsz / 16 && table_size < (1ull << 31)) table_size <<= 1;
    vector<uint64_t> table(table_size, EMPTY);
    vector<uint64_t> row_hash;
    // The arrays of the hit sets grow to GIGABYTES at 50 M reads (4 GB of column indices): grown by doubling they are copied
    // 8 GB worth and fault in twice their final pages -- on the thread every other stage waits for.  Address space is
    // reserved from the file's size instead (a binary record of c hits is >= 16 compressed bytes and inflates about 2.5 x;
    // untouched pages cost nothing); a reservation the system refuses is simply not made.
    try {
        col_idx.reserve((size_t)min<uint64_t>(fsz * 3 / 4, 3ull << 30));
        const size_t rows = (size_t)min<uint64_t>(fsz / 24, 1ull << 28);
        row_ptr.reserve(rows + 1); row_hash.reserve(rows); k.reserve(rows);
        // ... and is advised to come in huge pages: 5 GB first touched on this thread are 1.2 M page faults otherwise
        auto huge = [](void *p, size_t bytes) {
            const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
            if (e > a) (void)madvise((void *)a, e - a, MADV_HUGEPAGE);
        };
        huge(col_idx.data(), col_idx.capacity() * 4); huge(row_ptr.data(), row_ptr.capacity() * 8);
        huge(row_hash.data(), row_hash.capacity() * 8); huge(k.data(), k.capacity() * 4);
    } catch (const std::bad_alloc &) {}
    auto grow = [&]() {
        vector<uint64_t> bigger(table.size() * 2, EMPTY);
        const size_t mask = bigger.size() - 1;
        for (uint32_t r = 0; r < (uint32_t)row_hash.size(); ++r) {
            size_t s = (size_t)row_hash[r] & mask;
            while (bigger[s] != EMPTY) s = (s + 1) & mask;
            bigger[s] = (row_hash[r] & 0xffffffff00000000ull) | r;
        }
        table.swap(bigger);
    };
    // Four stages over a ring of blocks of reads, each stage its own thread(s): (1) the reader -- inflate (a thread of its own inside
    // hitsio) + record decode, strictly sequential (src/hitsio.hpp:77-79); (2) first-seen transcript numbering (:399-408),
    // sequential as well; (3) NSORT threads, alternate blocks: every read's hit set sorted and freed of repeats, its hash -- the
    // longest stage at 50 M reads; (4) this thread: the hit-set table.
    struct Block { vector<uint32_t> len, idx, dups; vector<uint64_t> hash; bool last = false; };
    // (round 5: with the file inflated by several threads and the records parsed in place, the two sorters of round 4 became the
    // pace of the pipeline -- reader and numberer both waited 4.7 s of a 6.3 s read: four, over a ring twice as deep)
    constexpr int NB = 16, NSORT = 4;
    Block blocks[NB];
    int state[NB] = {0}; // 0: free for the reader, 1: decoded, 2: numbered, 3: prepared for the table
    mutex mtx;
    condition_variable cv;
    atomic<uint32_t> n_seen{0}; // transcripts numbered so far (progress line only)
    double waited[4] = {0.0, 0.0, 0.0, 0.0}; // seconds a stage spent waiting for a block (MMSEQ_TIMING: which stage bounds the pipeline)
    auto wait_for = [&](int b, int want, int stage_id) {
        const double t0 = omp_get_wtime();
        { unique_lock<mutex> lk(mtx); cv.wait(lk, [&] { return state[b] == want; }); }
        if (stage_id >= 0) waited[stage_id] += omp_get_wtime() - t0;
    };
    auto set_state = [&](int b, int v) { { lock_guard<mutex> lk(mtx); state[b] = v; } cv.notify_all(); };
    thread producer([&]() {
        bool more = true;
        for (int b = 0; more; b = (b + 1) % NB) {
            wait_for(b, 0, 0);
            Block &B = blocks[b];
            B.len.clear(); B.idx.clear();
            more = hitsfileReader.readReadMapRecordsBulk(B.len, B.idx, 65536); // the read names are not used (:395-441)
            B.last = !more;
            set_state(b, 1);
        }
    });
    thread numberer([&]() {
        bool last = false;
        for (int b = 0; !last; b = (b + 1) % NB) {
            wait_for(b, 1, 1);
            Block &B = blocks[b];
            last = B.last;
            for (uint32_t &x : B.idx) {
                const uint32_t hidx = x;
                if (hidx >= nHeader) {
                    cerr << "Error: a read maps to a transcript that has no @TranscriptMetaData entry (no length).\n";
                    hits_die(); // (a pipeline thread: no static destructors under the other threads)
                }
                if (hdr2obs[hidx] < 0) {
                    hdr2obs[hidx] = (int32_t)obs2hdr.size(); obs2hdr.push_back(hidx);
                    n_seen.store((uint32_t)obs2hdr.size(), memory_order_relaxed);
                }
                x = (uint32_t)hdr2obs[hidx];
            }
            set_state(b, 2);
        }
    });
    atomic<int> last_block{-1}; // index of the block that ends the file, once known
    vector<thread> sorters;
    for (int w = 0; w < NSORT; ++w)
        sorters.emplace_back([&, w]() {
            for (int b = w;; b = (b + NSORT) % NB) {
                { // this sorter's next block, or the end of the file in the other sorter's hands
                    unique_lock<mutex> lk(mtx);
                    cv.wait(lk, [&] { return state[b] == 2 || last_block.load() >= 0; });
                    if (state[b] != 2) return;
                }
                Block &B = blocks[b];
                B.hash.resize(B.len.size());
                B.dups.clear();
                size_t at = 0, out = 0;
                for (size_t r = 0; r < B.len.size(); ++r) {
                    uint32_t *c = B.idx.data() + out; // the set is written over the block's own indices (never ahead of the read position)
                    const uint32_t nin = B.len[r];
                    for (uint32_t q = 0; q < nin; ++q) c[q] = B.idx[at++];
                    sort(c, c + nin);
                    uint32_t nu = 0;
                    for (uint32_t q = 0; q < nin; ++q) {
                        if (nu && c[nu - 1] == c[q]) B.dups.push_back(c[q]); // a transcript listed twice for one read (:421-424)
                        else c[nu++] = c[q];
                    }
                    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)nu;
                    for (uint32_t q = 0; q < nu; ++q) { h ^= c[q]; h *= 0xff51afd7ed558ccdull; h ^= h >> 32; }
                    B.hash[r] = h;
                    B.len[r] = nu;
                    out += nu;
                }
                const bool was_last = B.last;
                if (was_last) last_block.store(b);
                set_state(b, 3);
                if (was_last) return;
            }
        });
    vector<uint32_t> all_dups;
    bool last = false;
    for (int b = 0; !last; b = (b + 1) % NB) {
        wait_for(b, 3, 3);
        const Block &B = blocks[b];
        last = B.last;
        all_dups.insert(all_dups.end(), B.dups.begin(), B.dups.end());
        size_t at = 0;
        for (size_t r = 0; r < B.len.size(); ++r) {
            H.numbermappedreads++;
            const uint32_t *comb = B.idx.data() + at;
            const uint32_t nc = B.len[r];
            at += nc;
            const uint64_t h = B.hash[r];
            const size_t mask = table.size() - 1;
            if (r + 12 < B.len.size()) __builtin_prefetch(&table[(size_t)B.hash[r + 12] & mask]);
            size_t s = (size_t)h & mask;
            uint32_t row = 0xffffffffu;
            for (;; s = (s + 1) & mask) {
                const uint64_t e = table[s];
                if (e == EMPTY) break;
                if ((e ^ h) >> 32) continue; // another set's tag
                const uint32_t rr = (uint32_t)e;
                if (row_hash[rr] == h && row_ptr[rr + 1] - row_ptr[rr] == nc && equal(comb, comb + nc, col_idx.begin() + (ptrdiff_t)row_ptr[rr])) { row = rr; break; }
            }
            if (row == 0xffffffffu) {
                row = (uint32_t)k.size();
                if ((row & 0xffff) == 0)
                    cout << "Found " << n_seen.load(memory_order_relaxed) << " transcripts in " << row << " transcript combinations.\r" << flush;
                table[s] = (h & 0xffffffff00000000ull) | row;
                row_hash.push_back(h);
                k.push_back(0);
                col_idx.insert(col_idx.end(), comb, comb + nc);
                row_ptr.push_back(col_idx.size());
                if ((uint64_t)k.size() * 2 > table.size()) grow();
            }
            k[row]++;
        }
        set_state(b, 0);
    }
    numberer.join();
    cv.notify_all();
    for (auto &t : sorters) t.join();
    H.doublehits.assign(obs2hdr.size(), 0);
    for (uint32_t o : all_dups) H.doublehits[o]++;
    if (timing) fprintf(stderr, "[timing] ingest stages waited: decode %.1f s, numbering %.1f s, table %.1f s (the sort + hash stage is the rest)\n", waited[0], waited[1], waited[3]);
    producer.join();
    cout << "Found " << obs2hdr.size() << " transcripts in " << k.size() << " transcript combinations." << endl;
    if (H.n() == 0 || H.m() == 0) leave_with("Error: no reads with transcript hits found in the hits file.\n");
    return H;
}

// the observed transcripts by index (sid, indexSid of src/mmseq.cpp) and by name (sidIndex; -1: no hits) -- built once after the
// read, read by the stages after it (some of them from several threads)
struct Observed {
    vector<string> names;
    unordered_map<string, int32_t> index;
    Observed(const Header &hdr, const Hits &hits)
    {
        names.reserve(hits.n());
        index.reserve(hits.n());
        for (uint32_t t = 0; t < hits.n(); ++t) {
            names.push_back(hdr.transcriptList[hits.obs2hdr[t]]);
            index[names.back()] = (int32_t)t;
        }
    }
    int32_t of(const string &name) const { auto it = index.find(name); return it == index.end() ? -1 : it->second; }
};

// ---- l[t] (src/mmseq.cpp:593-608)
static vector<double> effective_lengths(const Header &hdr, const Hits &hits)
{
    vector<double> l(hits.n());
    for (uint32_t t = 0; t < hits.n(); t++) {
        const string &sid = hdr.transcriptList[hits.obs2hdr[t]];
        if (hdr.sidLen.count(sid) == 0) leave_with("Error: transcript '" + sid + "' has no length.\n");
        l[t] = hdr.sidLen.at(sid) * (double)hits.numbermappedreads / 1000000000.0;
        if (l[t] <= 0) leave_with("Error: transcript '" + sid + "' has a length of zero.\n");
    }
    return l;
}

// ---- start values and unique hits (src/mmseq.cpp:610-638) come from the device once the problem is there
//      (mmg_problem_start_values: the shares k_i / |row i| summed EXACTLY in fixed point -- the reference adds them in floating point
//      in the order it read the file, so its start value depends on that order in the last bits; this one is a function of the hit
//      sets).  The 100-bin histogram of shared counts is only ever written by -debug (.sharedcounts): a host pass, then.
static vector<vector<int>> shared_counts(const Hits &hits)
{
    const uint32_t n = hits.n();
    const uint64_t m = hits.m();
    vector<vector<int>> counts_shared(n, vector<int>(100, 0));
#pragma omp parallel num_threads(max(1, min(8, omp_get_max_threads() / 2))) // every thread reads the whole hit list: more only adds traffic
    {
        const uint64_t nth = (uint64_t)omp_get_num_threads(), tid = (uint64_t)omp_get_thread_num();
        const uint32_t lo = (uint32_t)((uint64_t)n * tid / nth), hi = (uint32_t)((uint64_t)n * (tid + 1) / nth);
        if (lo < hi)
            for (uint64_t i = 0; i < m; ++i) {
                const uint64_t b = hits.row_ptr[i], e = hits.row_ptr[i + 1];
                const int L = (int)(e - b);
                for (uint64_t j = b; j < e; ++j) {
                    const uint32_t c = hits.col_idx[j];
                    if (c - lo < hi - lo) counts_shared[c][min(L, 100) - 1] += (int)hits.k[i];
                }
            }
    }
    return counts_shared;
}

struct UniqueHits {
    vector<int> identical, gene;
    vector<int32_t> transcript;   // (from the device, with the start values)
};

// ---- unique hits to identical sets and genes: O(nnz) form of src/uh.cpp:3-26
static UniqueHits count_unique_hits(const Header &hdr, const Hits &hits, const Observed &obs)
{
    const uint32_t n = hits.n();
    const uint64_t m = hits.m();
    const vector<uint64_t> &row_ptr = hits.row_ptr;
    const vector<uint32_t> &col_idx = hits.col_idx, &k = hits.k;
    UniqueHits uh;
    uh.identical.assign(hdr.identical_transcripts.size(), 0);
    uh.gene.assign(hdr.gene2transcripts.size(), 0);
    cerr << "Counting unique hits to sets of identical transcripts...";
    vector<vector<uint32_t>> t2sets(n);
    for (size_t v = 0; v < hdr.identical_transcripts.size(); ++v)
        for (auto &name : hdr.identical_transcripts[v]) {
            const int32_t t = obs.of(name);
            if (t >= 0) t2sets[t].push_back((uint32_t)v);
        }
    // rows in parallel, integer counts per thread summed at the end (the sums do not depend on the split)
    const int uh_threads = max(1, omp_get_max_threads());
    int64_t empty_rows_k = 0;
    {
        vector<vector<int>> part((size_t)uh_threads, vector<int>(uh.identical.size(), 0));
#pragma omp parallel num_threads(uh_threads) reduction(+ : empty_rows_k)
        {
            vector<int> &mine = part[(size_t)omp_get_thread_num()];
            vector<uint32_t> cand, tmp;
#pragma omp for schedule(static)
            for (int64_t i = 0; i < (int64_t)m; ++i) {
                const uint64_t b = row_ptr[i], e = row_ptr[i + 1];
                if (b == e) { empty_rows_k += (int64_t)k[i]; continue; } // an empty row counts for every group
                if (t2sets[col_idx[b]].empty()) continue;
                cand = t2sets[col_idx[b]];
                for (uint64_t j = b + 1; j < e && !cand.empty(); ++j) {
                    tmp.clear();
                    for (uint32_t s : cand)
                        if (find(t2sets[col_idx[j]].begin(), t2sets[col_idx[j]].end(), s) != t2sets[col_idx[j]].end()) tmp.push_back(s);
                    cand.swap(tmp);
                }
                sort(cand.begin(), cand.end());
                cand.erase(unique(cand.begin(), cand.end()), cand.end());
                for (uint32_t s : cand) mine[s] += (int)k[i];
            }
        }
        for (auto &pt : part) for (size_t v = 0; v < pt.size(); ++v) uh.identical[v] += pt[v];
        for (auto &x : uh.identical) x += (int)empty_rows_k;
    }
    cerr << "done." << endl;
    cerr << "Counting unique hits to genes...";
    map<string, int> gene2index;
    { int g = 0; for (auto &gt : hdr.gene2transcripts) gene2index[gt.first] = g++; }
    vector<int> t2g(n);
    for (uint32_t t = 0; t < n; ++t) t2g[t] = gene2index[hdr.transcript2gene.at(obs.names[t])];
    {
        vector<vector<int>> part((size_t)uh_threads, vector<int>(uh.gene.size(), 0));
#pragma omp parallel num_threads(uh_threads)
        {
            vector<int> &mine = part[(size_t)omp_get_thread_num()];
#pragma omp for schedule(static)
            for (int64_t i = 0; i < (int64_t)m; ++i) {
                const uint64_t b = row_ptr[i], e = row_ptr[i + 1];
                if (b == e) continue;
                const int g = t2g[col_idx[b]];
                bool uniq = true;
                for (uint64_t j = b + 1; j < e; ++j) if (t2g[col_idx[j]] != g) { uniq = false; break; }
                if (uniq) mine[g] += (int)k[i];
            }
        }
        for (auto &pt : part) for (size_t g = 0; g < pt.size(); ++g) uh.gene[g] += pt[g];
        for (auto &x : uh.gene) x += (int)empty_rows_k;
    }
    cerr << "done." << endl;
    return uh;
}

// ---- .k and .M (src/mmseq.cpp:682-695): 14 GB of text at 50 M reads, written by a thread of its own while the device builds the
//      problem and runs EM and Gibbs (the arrays it reads are not touched again; joined before the run ends).  Its formatting
//      threads leave three CPUs of the container's quota alone: with all of them busy the quota runs out and the main thread is
//      throttled with them -- the upload of the matrix (4 GB of pageable memory through the runtime's staging copies) took 2.8 s
//      instead of 0.3 s, and an EM sweep (a kernel and a read-back) 8 ms instead of 1.3.
static JoiningThread start_km_writer(const string &output_base, const Hits &hits, const Observed &obs)
{
    const int km_threads = max(1, omp_get_max_threads() - 3);
    return JoiningThread([&hits, &obs, output_base, km_threads]() { // integer tables: chunks of rows formatted in parallel (to_chars), written in order
        const uint64_t m = hits.m();
        const uint32_t n = hits.n();
        ofstream ofs;
        auto write_rows = [&](ofstream &o, const function<void(uint64_t, string &)> &fmt) {
            const uint64_t chunk = 1u << 16;
            const int64_t nchunks = (int64_t)((m + chunk - 1) / chunk);
            const int64_t batch = max<int64_t>(1, km_threads * 2);
            for (int64_t c0 = 0; c0 < nchunks; c0 += batch) {
                const int64_t nb = min(batch, nchunks - c0);
                vector<string> out(nb);
#pragma omp parallel for schedule(dynamic, 1) num_threads(km_threads)
                for (int64_t c = 0; c < nb; ++c) {
                    const uint64_t r0 = (uint64_t)(c0 + c) * chunk, r1 = min<uint64_t>(m, r0 + chunk);
                    for (uint64_t i = r0; i < r1; ++i) fmt(i, out[c]);
                }
                for (auto &x : out) o.write(x.data(), (streamsize)x.size());
            }
        };
        auto put = [](string &o, uint64_t v, char sep) {
            char tmp[24];
            auto r = to_chars(tmp, tmp + sizeof tmp, v);
            o.append(tmp, r.ptr - tmp);
            o.push_back(sep);
        };
        ofs.open((output_base + ".k").c_str());
        write_rows(ofs, [&](uint64_t i, string &o) { put(o, hits.k[i], '\n'); });
        ofs.close(); ofs.clear();
        ofs.open((output_base + ".M").c_str());
        ofs << "#";
        for (uint32_t t = 0; t < n; t++) ofs << "\t" << obs.names[t];
        ofs << "\n";
        // one line "row<TAB>column" per hit (:690-694): 13.7 GB of text at 50 M reads.  The row's digits are formatted once per row,
        // the lines of a chunk go into one buffer sized beforehand (a row index and a column index have at most 10 digits each)
        write_rows(ofs, [&](uint64_t i, string &o) {
            const uint64_t b = hits.row_ptr[i], e = hits.row_ptr[i + 1];
            if (b == e) return;
            char head[24];
            const size_t hl = (size_t)(to_chars(head, head + 22, i).ptr - head);
            head[hl] = '\t';
            const size_t at = o.size();
            o.resize(at + (e - b) * (hl + 1 + 11));
            char *w = &o[at];
            for (uint64_t j = b; j < e; ++j) {
                memcpy(w, head, hl + 1);
                w = to_chars(w + hl + 1, w + hl + 12, hits.col_idx[j]).ptr;
                *w++ = '\n';
            }
            o.resize((size_t)(w - o.data()));
        });
        ofs.close(); ofs.clear();
    });
}

// src/mmseq.cpp:697-731
static void write_debug_files(const string &output_base, const Header &hdr, const Hits &hits, const Observed &obs,
                              const vector<vector<int>> &counts_shared)
{
    const uint32_t n = hits.n();
    ofstream ofs((output_base + ".sharedcounts").c_str());
    for (auto &name : hdr.transcriptList) {
        ofs << name << "\t";
        const int32_t t = obs.of(name);
        for (int i = 0; i < 100; i++) ofs << (t >= 0 ? counts_shared[t][i] : 0) << "\t";
        ofs << endl;
    }
    ofs.close(); ofs.clear();
    ofs.open((output_base + ".doublehits").c_str());
    for (uint32_t i = 0; i < n; i++) ofs << hits.doublehits[i] << endl;
    ofs.close(); ofs.clear();
    // transposed matrix without consecutive duplicate rows, and the ids of the duplicates
    vector<vector<uint32_t>> Mt(n);
    for (uint64_t i = 0; i < hits.m(); ++i)
        for (uint64_t j = hits.row_ptr[i]; j < hits.row_ptr[i + 1]; ++j) Mt[hits.col_idx[j]].push_back((uint32_t)i);
    ofs.open((output_base + ".Mt-nodups").c_str());
    ofstream ofs2((output_base + ".dupIDs").c_str());
    for (uint32_t t = 0; t < n; ++t) {
        if (t > 0 && Mt[t] == Mt[t - 1]) ofs2 << obs.names[t] << endl;
        else for (uint32_t r : Mt[t]) ofs << t << "\t" << r << endl;
    }
}

// the problem on the device(s).  Declared in this order, released in the reverse one: the problems made for the other devices, the
// whole problem, the group (as the run has always released them)
struct Device {
    Group grp;                  // several devices only
    Problem prob;               // the whole problem, on the first device (dropped once nothing runs on it any more)
    Problems copies;            // problems made here for the devices (besides prob)
    vector<mmg_problem *> part; // problem of device i
    bool shard = false;         // several devices, one chain: the reads are cut into shards
};

// ---- device problem.  Rows go up in first-seen order and observed-transcript numbering, exactly as src/mmseq.cpp:399-418 builds
//      them; the library stores the rows in its own canonical order and -- given tx_order -- numbers the transcripts gene by gene
//      (header order, the isoforms of a gene adjacent: the sample kernel keeps a window of consecutive transcripts in LDS and
//      wants a read's hits close together).  Both orders are irrelevant to the model; every array that comes back is in
//      observed-transcript numbering.
static Problem build_problem(const Options &opt, const Header &hdr, const Hits &hits, const Observed &obs, const vector<double> &l,
                             JoiningThread &device_warmup, StageTimer &stage, vector<double> &mu, vector<int32_t> &unique_hits)
{
    const uint32_t n = hits.n();
    const size_t nHeader = hdr.transcriptList.size();
    // key: (smallest header index of the transcript's gene, own header index)
    unordered_map<string, uint32_t> hdr_of_name;
    hdr_of_name.reserve(nHeader * 2);
    for (size_t i = 0; i < nHeader; ++i) hdr_of_name.emplace(hdr.transcriptList[i], (uint32_t)i);
    map<string, uint32_t> gene_first;
    for (auto &gt : hdr.gene2transcripts) {
        uint32_t f = 0xffffffffu;
        for (auto &name : gt.second) { auto it = hdr_of_name.find(name); if (it != hdr_of_name.end()) f = min(f, it->second); }
        gene_first[gt.first] = f;
    }
    vector<uint64_t> tx_order(n);
    for (uint32_t t = 0; t < n; ++t) {
        auto tg = hdr.transcript2gene.find(obs.names[t]);
        const uint32_t gf = tg == hdr.transcript2gene.end() ? hits.obs2hdr[t] : min(gene_first[tg->second], hits.obs2hdr[t]);
        tx_order[t] = ((uint64_t)gf << 32) | hits.obs2hdr[t];
    }
    mmg_problem_desc pd;
    memset(&pd, 0, sizeof pd);
    pd.m = hits.m(); pd.n = n; pd.row_ptr = hits.row_ptr.data(); pd.col_idx = hits.col_idx.data(); pd.k = hits.k.data(); pd.l = l.data();
    pd.row_id_base = 0; pd.layout = MMG_LAYOUT_CANONICAL; pd.tx_order = tx_order.data();
    device_warmup.join();
    // (the handles keep the names of the calls' text in their error messages: prob, smp, summ, grp, smps, part, ...)
    const int device = opt.device;
    mmg_problem *prob = nullptr;
    MMG_TRY(mmg_problem_create(&pd, device, &prob));
    Problem owned(prob);
    mmg_problem_info inf0;
    MMG_TRY(mmg_problem_info_get(prob, &inf0));
    if (inf0.tx_renumbered & MMG_ORDER_SKIPPED)
        cerr << "Warning: not enough free device memory to try a gene order derived from the hit graph; the run uses the hits file's gene order "
                "(slower on reads that hit paralogues, and the traces differ from a run that had the memory)" << endl;
    if (stage.on) {
        mmg_problem_info inf;
        MMG_TRY(mmg_problem_info_get(prob, &inf));
        fprintf(stderr, "[timing] sample kernel %d (2 sliced-ELL stream, 0 CSR tiles), %llu of %llu tiles on the register path, %llu with far lists, %.1f MB on the device%s\n",
                inf.sample_kernel, (unsigned long long)inf.fast_tiles, (unsigned long long)inf.n_tiles, (unsigned long long)inf.far_tiles, inf.device_bytes / 1e6,
                (inf.tx_renumbered & 0xff) == 3 ? "; the genes reordered by the gene-level hit graph (reads that also hit paralogues)" : "");
    }
    stage.mark("device problem build");
    MMG_TRY(mmg_problem_start_values(prob, mu.data(), unique_hits.data()));
    stage.mark("start values, unique hits (device)");
    return owned;
}

// ---- several devices: the stored problem (canonical order, device numbering) is cut into contiguous read shards, one per device
//      (one chain: EM and Gibbs both run sharded), or replicated (chains >= devices).  Cut on device 0 and copied device to
//      device (mmg_problem_shard): nothing comes back to the host.
static void spread(const Options &opt, Device &dev, const vector<double> &mu, StageTimer &stage)
{
    const int gpus = opt.gpus;
    const bool shard = dev.shard = gpus > 1 && opt.chains == 1;
    mmg_problem *prob = dev.prob.get();
    vector<mmg_problem *> &part = dev.part;
    if (gpus == 1) { part.assign(1, prob); return; }
    vector<int> devs(gpus);
    for (int i = 0; i < gpus; ++i) devs[i] = opt.device + i;
    mmg_group *grp = nullptr;
    MMG_TRY(mmg_group_create(devs.data(), gpus, &grp));
    dev.grp.reset(grp);
    mmg_problem_info inf;
    MMG_TRY(mmg_problem_info_get(prob, &inf));
    vector<uint64_t> bounds(gpus + 1, 0);
    // cut by measured cost: every candidate shard is timed on device 0 with the start values as weights (0.1 s), so that the devices
    // finish their sweeps together whatever the mix of near rows, far rows and multiplicities (src/mmseq.cpp:864 splits the rows evenly)
    if (shard) MMG_TRY(mmg_problem_shard_bounds_timed(prob, mu.data(), gpus, bounds.data()));
    part.assign(gpus, nullptr);
    for (int i = 0; i < gpus; ++i) {
        if (!shard && i == 0) { part[0] = prob; continue; }
        MMG_TRY(mmg_problem_shard(prob, shard ? bounds[i] : 0, shard ? bounds[i + 1] : inf.m, devs[i], &part[i]));
        dev.copies.h.push_back(part[i]);
    }
    if (stage.on && shard) {
        fprintf(stderr, "[timing] read shards (rows):");
        for (int i = 0; i < gpus; ++i) fprintf(stderr, " %llu", (unsigned long long)(bounds[i + 1] - bounds[i]));
        fprintf(stderr, "\n");
    }
    stage.mark(shard ? "read shards" : "replicas");
}

// ---- EM on the device(s) (src/mmseq.cpp:741-811): mu stays there; this loop owns the stopping rule and the output
static vector<double> run_em(const Options &opt, const Observed &obs, Device &dev, vector<double> mu, StageTimer &stage)
{
    const uint32_t n = (uint32_t)obs.names.size();
    const bool shard_em = dev.shard && !opt.em_one_device;
    // the whole problem is needed on device 0 only while something runs on it: with sharded EM and Gibbs, not beyond this point
    if (shard_em) dev.prob.reset();
    unique_ptr<GzText> gz_em;
    if (opt.debug) {
        const string path = opt.output_base + ".trace_em.gz";
        gz_em = make_unique<GzText>(path);
        if (!gz_em->ok()) fatal("cannot open " + path + " for writing.");
        for (uint32_t t = 0; t < n; t++) { gz_em->str(obs.names[t]); gz_em->str(" "); }
        gz_em->str("\n");
    }
    {
        double loglik = 0.0;
        mmg_group *grp = dev.grp.get();
        mmg_problem *prob = dev.prob.get();
        const vector<mmg_problem *> &part = dev.part;
        Ems ems(shard_em ? opt.gpus : 1);
        if (shard_em) MMG_TRY(mmg_group_em_create(grp, part.data(), mu.data(), ems.data(), &loglik)); // exact integer sums: the bits of the unsharded EM
        else MMG_TRY(mmg_em_create(prob, mu.data(), &ems[0], &loglik));
        mmg_em *em = ems[0];
        stage.mark("EM set-up + first pass");
        double llr = opt.epsilon + 1;
        int iter = 0;
        cout.precision(5);
        cout.setf(ios::fixed, ios::floatfield);
        while (iter < opt.max_em_iter && llr > opt.epsilon) {
            cout << "EM iteration " << iter << flush;
            if (gz_em) {
                if (iter) MMG_TRY(mmg_em_get_mu(em, mu.data()));
                for (uint32_t t = 0; t < n; t++) { gz_em->num(mu[t]); gz_em->str(" "); }
                gz_em->str("\n");
            }
            double ll = 0.0;
            MMG_TRY(mmg_em_step(em, &ll));
            llr = ll - loglik;
            loglik = ll;
            cout << ", log likelihood ratio: " << llr << "            \r";
            iter++;
        }
        MMG_TRY(mmg_em_get_mu(em, mu.data()));
    }
    if (dev.shard) dev.prob.reset();   // (-em_one_device: the whole problem has served)
    cout << endl;
    cout.unsetf(ios::floatfield);
    cout.precision(6);
    if (gz_em) gz_em->close();
    return mu;
}

// the series of the summary: isoforms without hits, identical sets and genes (their members: caller's transcripts or n + virtual index)
struct SeriesLayout {
    vector<uint64_t> vid, iptr{0}, gptr{0};
    vector<double> vscale;
    vector<uint32_t> imem, gmem;
    map<string, uint32_t> simuIndex; // isoform without hits -> its simulated ("virtual") trace
    vector<int> pind;                // the sample index of each percentile
    vector<string> identical_ids, gene_ids; // the feature ids of the identical sets ("+"-joined members) and of the genes
    uint32_t simu_of(const string &name) const { auto it = simuIndex.find(name); return it == simuIndex.end() ? 0u : it->second; }
    mmg_summary_desc desc() const
    {
        mmg_summary_desc d;
        memset(&d, 0, sizeof d);
        d.n_virtual = (uint32_t)vid.size(); d.virtual_id = vid.data(); d.virtual_scale = vscale.data();
        d.n_identical = (uint32_t)(iptr.size() - 1); d.identical_ptr = iptr.data(); d.identical_member = imem.data();
        d.n_genes = (uint32_t)(gptr.size() - 1); d.gene_ptr = gptr.data(); d.gene_member = gmem.data();
        return d;
    }
};

static SeriesLayout series_layout(const Options &opt, const Header &hdr, const Hits &hits, const Observed &obs)
{
    SeriesLayout s;
    const uint32_t n = hits.n();
    const size_t nHeader = hdr.transcriptList.size();
    map<string, uint32_t> headerIndexOf;
    for (size_t i = 0; i < nHeader; ++i) headerIndexOf[hdr.transcriptList[i]] = (uint32_t)i;
    for (auto &set : hdr.identical_transcripts) {
        string id;
        for (auto &name : set) {
            const int32_t t = obs.of(name);
            if (t >= 0) s.imem.push_back((uint32_t)t);
            id += name;
            if (name.compare(set.back()) != 0) id += "+";
        }
        s.iptr.push_back(s.imem.size());
        s.identical_ids.push_back(id);
    }
    size_t g = 0;
    for (auto &gt : hdr.gene2transcripts) {
        s.gene_ids.push_back(gt.first);
        for (auto &name : gt.second) {
            const int32_t t = obs.of(name);
            if (t >= 0) { s.gmem.push_back((uint32_t)t); continue; }
            // no hits: simulate from the prior-only conditional (keyed by the header index, :971-978)
            s.simuIndex[name] = (uint32_t)s.vid.size();
            s.gmem.push_back(n + (uint32_t)s.vid.size());
            s.vid.push_back(headerIndexOf.count(name) ? headerIndexOf[name] : (uint64_t)nHeader + g);
            s.vscale.push_back(1.0 / (opt.beta + hdr.len_of(name) * (double)hits.numbermappedreads / 1000000000.0));
        }
        s.gptr.push_back(s.gmem.size());
        g++;
    }
    for (double p : opt.percentiles) s.pind.push_back(static_cast<int>(round(p / 100.0 * (trace_length - 1))));
    return s;
}

// the chains on the device(s) and the posterior summary that is fed while they run.  Released in the reverse order: summary, samplers
struct Chains {
    Samplers smps;              // sampler of device i
    Summary summ;
    mmg_sampler *smp() const { return smps.h[0]; } // traces and per-feature summaries come from chain 0 (every shard holds the whole chain)
};

// ---- Gibbs on the device(s) (src/mmseq.cpp:833-918); the trace stays there.
//      one device: `chains` chains in one sampler.  several devices, one chain: the stored rows are cut into contiguous shards
//      (mmg_shard_bounds), one per device, counts all-reduced over RCCL every iteration -- bit-identical to the one-device run.
//      several devices, chains >= devices: the stored problem is replicated, every device runs chains / gpus chains.
static void begin_summary(Chains &ch, const SeriesLayout &layout);
static Chains start_chains(const Options &opt, const Device &dev, const vector<double> &mu_em, const SeriesLayout &layout)
{
    Chains ch;
    mmg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.alpha = opt.alpha; cfg.beta = opt.beta; cfg.seed = (uint64_t)(int64_t)opt.seed;
    cfg.n_chains = opt.gpus > 1 ? max(1, opt.chains / opt.gpus) : opt.chains; cfg.chain_base = 0; cfg.gibbs_iter = opt.gibbs_iter; cfg.trace_len = trace_length;
    cfg.keep_trace = 1; cfg.timing = 0;
    Samplers &smps = ch.smps;
    mmg_problem *prob = dev.prob.get();
    const vector<mmg_problem *> &part = dev.part;
    smps.h.assign(opt.gpus, nullptr);
    if (opt.gpus == 1) MMG_TRY(mmg_sampler_create(prob, &cfg, mu_em.data(), &smps[0]));
    else
        for (int i = 0; i < opt.gpus; ++i) {
            mmg_config ci = cfg;
            ci.chain_base = dev.shard ? 0 : i * cfg.n_chains; // (far below MMG_MAX_CHAINS: at most 4096 chains per sampler, and mmg_sampler_create checks)
            MMG_TRY(mmg_sampler_create(part[i], &ci, mu_em.data(), &smps[i]));
        }
    // ---- the posterior summary is set up BEFORE the loop and fed while it runs (src/mmseq.cpp:911-917 prints sample s inside the
    //      loop; :927-1108 derives the other traces after it): sample s is final after iteration s * gibbs_ss, so the four trace files
    //      are formatted, compressed and written by background threads while the device runs on -- rows come off the device on
    //      streams of their own (mmg_sampler_get_trace_rows_done, mmg_summary_get_rows), nothing waits for the chain.
    //      (-gibbs_auto: begun behind the last stage -- an extension replaces the samples a summary was begun on)
    if (!opt.auto_on) begin_summary(ch, layout);
    return ch;
}

static void begin_summary(Chains &ch, const SeriesLayout &layout)
{
    mmg_summary_desc sd = layout.desc();
    sd.chain = 0;
    sd.n_percentiles = (uint32_t)layout.pind.size(); sd.percentile_index = layout.pind.data();
    mmg_sampler *smp = ch.smp();
    mmg_summary *summ = nullptr;
    MMG_TRY(mmg_summary_begin(smp, &sd, &summ));
    ch.summ.reset(summ);
}

// One trace file, written by a worker thread: the ids of the series kept, then trace_length rows fetched as they become final.  With
// what_first, a series whose first sample has no finite logarithm is left out of the file (:1040 for identical sets, :1068 for genes).
// (what, what_first: the fetches' call text for an error message; what_first is null for files that keep every series)
static void start_trace_file(TraceWriters &w, const string &path, const vector<string> &ids, const char *what_first,
                             const function<int(int, int, double *)> &fetch, const char *what, int threads)
{
    w.threads.emplace_back([&w, path, &ids, what_first, fetch, what, threads] {
        vector<char> keep(ids.size(), 1);
        if (what_first) {
            w.wait_for(1);
            if (w.stop.load()) return;
            vector<double> first(max<size_t>(ids.size(), 1));
            if (w.failed(fetch(0, 1, first.data()), what_first)) return;
            for (size_t i = 0; i < ids.size(); ++i) keep[i] = isfinite(log(first[i])) != 0;
        }
        GzText gz(path);
        if (!gz.ok()) { w.record("cannot open " + path + " for writing."); return; }
        for (size_t i = 0; i < ids.size(); ++i)
            if (keep[i]) { gz.str(ids[i]); gz.str(" "); }
        gz.str("\n");
        write_trace_rows(gz, trace_length, ids.size(), [&](int first, int count, double *out) { w.wait_for(first + count); if (w.stop.load()) return; (void)w.failed(fetch(first, count, out), what); },
                         [&](size_t i) { return keep[i] != 0; }, w.stop, threads);
        gz.close();
    });
}

// the writers of the four trace files, each waiting for the samples `w` publishes
static void start_trace_writers(const Options &opt, const Observed &obs, const SeriesLayout &layout, const Chains &ch, TraceWriters &w)
{
    const int writer_threads = max(1, omp_get_max_threads());
    const int t_big = max(1, (writer_threads - 1) * 9 / 20), t_gene = max(1, writer_threads / 10);
    mmg_sampler *smp = ch.smp();
    mmg_summary *summ = ch.summ.get();
    auto rows = [summ](int kind) { return [summ, kind](int first, int count, double *out) { return mmg_summary_get_rows(summ, kind, first, count, out); }; };
    const string &base = opt.output_base;
    w.threads.reserve(4);
    start_trace_file(w, base + ".trace_gibbs.gz", obs.names, nullptr,
                     [smp](int first, int count, double *out) { return mmg_sampler_get_trace_rows_done(smp, 0, first, count, out); },
                     "mmg_sampler_get_trace_rows_done(smp, 0, first, count, out)", t_big);
    start_trace_file(w, base + ".identical.trace_gibbs.gz", layout.identical_ids,
                     "mmg_summary_get_rows(summ, MMG_SERIES_IDENTICAL, 0, 1, firstI.data())", rows(MMG_SERIES_IDENTICAL),
                     "mmg_summary_get_rows(summ, MMG_SERIES_IDENTICAL, first, count, out)", 1);
    start_trace_file(w, base + ".gene.trace_gibbs.gz", layout.gene_ids, "mmg_summary_get_rows(summ, MMG_SERIES_GENE, 0, 1, firstG.data())",
                     rows(MMG_SERIES_GENE),
                     "mmg_summary_get_rows(summ, MMG_SERIES_GENE, first, count, out)", t_gene);
    start_trace_file(w, base + ".prop.trace_gibbs.gz", obs.names, nullptr, rows(MMG_SERIES_TRANSCRIPT),
                     "mmg_summary_get_rows(summ, MMG_SERIES_TRANSCRIPT, first, count, out)", t_big);
}

// the Gibbs loop; the four trace files are written alongside by `w` (whose threads outlive it: they are joined after the tables are
// written -- the tail of their work runs next to the summary columns and the tables instead of in front of them)
static void run_gibbs(const Options &opt, const Observed &obs, const SeriesLayout &layout, const Device &dev, const Chains &ch,
                      TraceWriters &w, StageTimer &stage)
{
    mmg_summary *summ = ch.summ.get();
    mmg_group *grp = dev.grp.get();
    const Samplers &smps = ch.smps;
    start_trace_writers(opt, obs, layout, ch, w);
    // chunks of 1/64 of the run: the writers start on a chunk's samples when it ends, so what is left of their work after the last
    // iteration is 1/64 of the files
    const int gibbs_iter = opt.gibbs_iter, gibbs_ss = opt.gibbs_ss;
    const int chunk = max(1, gibbs_iter / 64);
    double t_enqueue = 0.0, t_sync = 0.0, t_advance = 0.0;
    auto enqueue = [&](int it) {
        const double c0 = omp_get_wtime();
        if (opt.gpus == 1) MMG_TRY(mmg_sampler_run(smps[0], it));
        else if (dev.shard) MMG_TRY(mmg_group_run_sharded(grp, smps.data(), it));
        else MMG_TRY(mmg_group_run_chains(grp, smps.data(), it));
        t_enqueue += omp_get_wtime() - c0;
    };
    // one chunk is always enqueued ahead of the one waited for: the device does not idle while this thread hands samples on (or is
    // held up: the writers use every CPU of the quota)
    enqueue(min(chunk, gibbs_iter));
    for (int done = 0; done < gibbs_iter; done += chunk) {
        cout << "Gibbs iteration " << done << "       \r" << flush;
        w.check();
        const int it = min(chunk, gibbs_iter - done);
        if (done + it < gibbs_iter) enqueue(min(chunk, gibbs_iter - done - it));
        // sample s is kept by iteration s * gibbs_ss (:911): the samples of the iterations up to done + it are final once the
        // iteration that stored the last of them is
        const int final_samples = min(trace_length, (done + it - 1) / gibbs_ss + 1);
        const double c1 = omp_get_wtime();
        for (auto sp : smps) MMG_TRY(mmg_sampler_wait_iterations(sp, done + it < gibbs_iter ? (final_samples - 1) * gibbs_ss + 1 : gibbs_iter));
        const double c2 = omp_get_wtime();
        MMG_TRY(mmg_summary_advance(summ, final_samples));
        w.publish(final_samples);
        t_sync += c2 - c1; t_advance += omp_get_wtime() - c2;
    }
    for (auto sp : smps) MMG_TRY(mmg_sampler_sync(sp));
    w.check();
    cout << "Gibbs iteration " << gibbs_iter - 1 << "       \r" << endl;
    if (stage.on) fprintf(stderr, "[timing] Gibbs loop: enqueue %.3f s, wait for the device %.3f s, derived rows %.3f s\n", t_enqueue, t_sync, t_advance);
    stage.mark("Gibbs (trace files written alongside)");
}

// ostream's default formatting of a double (%g, 6 digits), NaN as "nan": the numbers of output_base.autolength, as mmdiff prints its own
static string fmt_auto(double x)
{
    if (std::isnan(x)) return std::signbit(x) ? "-nan" : "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%g", x);
    return buf;
}

// -gibbs_auto: the run in stages.  Each stage runs the sampler to its planned end and judges the transcripts' R-hat and bulk / tail
// ESS across the chains (host/auto_rule.hpp); while the rule says no and twice the length stays within gibbs_auto the sampler is
// extended (mmg_sampler_extend: bit for bit the run planned at twice the length) and the next stage runs the second half.  No sample
// is final before the last stage ends, so the summary is begun and advanced to trace_length in one step behind it, and the four
// trace writers start with every sample published: their whole work follows the chain.  On return opt.gibbs_iter / gibbs_ss are the
// length the run stopped at, and everything downstream is what `mmseq -gibbs_iter L` does.
static void run_gibbs_auto(Options &opt, const Observed &obs, const SeriesLayout &layout, Chains &ch, uint32_t n, TraceWriters &w, StageTimer &stage)
{
    mmg_sampler *smp = ch.smp();
    const string path = opt.output_base + ".autolength";
    ofstream out(path.c_str());
    if (!out) fatal("cannot open " + path + " for writing.");
    const autolen::Targets &tg = opt.auto_targets;
    out << "# auto_ess " << fmt_auto(tg.ess) << " auto_rhat " << fmt_auto(tg.rhat) << " auto_frac " << fmt_auto(tg.frac) << " chains " << opt.chains << "\n";
    mmg_summary_desc cd;   // transcripts only: no isoforms without hits, no identical sets, no genes
    memset(&cd, 0, sizeof cd);
    vector<double> rhat(max<uint32_t>(n, 1), NAN), ess_bulk(rhat.size(), NAN), ess_tail(rhat.size(), NAN);
    double t_chain = 0.0, t_diag = 0.0, t_extend = 0.0;
    int done = 0;
    for (;;) {
        const double c0 = omp_get_wtime();
        MMG_TRY(mmg_sampler_run(smp, opt.gibbs_iter - done));
        MMG_TRY(mmg_sampler_sync(smp));
        done = opt.gibbs_iter;
        const double c1 = omp_get_wtime();
        {
            mmg_convergence *conv = nullptr;
            MMG_TRY(mmg_convergence_create(smp, &cd, &conv));
            const Convergence owned(conv);
            MMG_TRY(mmg_convergence_get(conv, MMG_SERIES_TRANSCRIPT, rhat.data(), ess_bulk.data(), ess_tail.data()));
        }
        const autolen::Verdict v = autolen::judge(n, rhat.data(), ess_bulk.data(), ess_tail.data(), tg);
        const double c2 = omp_get_wtime();
        t_chain += c1 - c0; t_diag += c2 - c1;
        const char *decision = v.stop ? "stop" : (opt.gibbs_iter <= opt.gibbs_auto / 2 ? "extend" : "max");
        out << opt.gibbs_iter << "\t" << opt.gibbs_iter / trace_length << "\t" << v.judged << "\t" << v.passes << "\t" << fmt_auto(v.min_ess) << "\t"
            << fmt_auto(v.max_rhat) << "\t" << decision << "\n";
        cout << "Gibbs auto: length " << opt.gibbs_iter << ", judged " << v.judged << ", passes " << v.passes << ", worst ESS " << fmt_auto(v.min_ess)
             << ", worst R-hat " << fmt_auto(v.max_rhat) << ": " << decision << endl;
        if (decision[0] != 'e') break;
        MMG_TRY(mmg_sampler_extend(smp));
        opt.gibbs_iter *= 2;
        t_extend += omp_get_wtime() - c2;
    }
    opt.gibbs_ss = opt.gibbs_iter / trace_length;
    out.close();
    if (!out) fatal("cannot write " + path + ".");
    if (stage.on) fprintf(stderr, "[timing] Gibbs auto: chain %.3f s, diagnostics %.3f s, extensions %.3f s\n", t_chain, t_diag, t_extend);
    stage.mark("Gibbs (auto length)");
    begin_summary(ch, layout);
    MMG_TRY(mmg_summary_advance(ch.summ.get(), trace_length));
    start_trace_writers(opt, obs, layout, ch, w);
    w.publish(trace_length);
    stage.mark("derived rows, writers started");
}

// moments of log mu pooled over all chains and devices (one fp64 all-reduce): log_mu, sd and mcse of multi-chain runs
struct Pooled { vector<double> sl, sl2; int64_t ns = 0; };
static Pooled pool_moments(const Options &opt, const Device &dev, const Chains &ch, uint32_t n)
{
    Pooled p;
    if (opt.chains <= 1) return p;
    vector<double> &pooled_sl = p.sl, &pooled_sl2 = p.sl2;
    int64_t &pooled_ns = p.ns;
    mmg_group *grp = dev.grp.get();
    mmg_sampler *smp = ch.smp();
    const Samplers &smps = ch.smps;
    pooled_sl.resize(n); pooled_sl2.resize(n);
    if (grp) { MMG_TRY(mmg_group_pool_moments(grp, smps.data(), pooled_sl.data(), pooled_sl2.data(), &pooled_ns)); return p; }
    vector<double> a_(n), b_(n);
    for (int c = 0; c < opt.chains; ++c) {
        int64_t ns = 0;
        MMG_TRY(mmg_sampler_get_moments(smp, c, a_.data(), b_.data(), &ns));
        for (uint32_t t = 0; t < n; ++t) { pooled_sl[t] += a_[t]; pooled_sl2[t] += b_[t]; }
        pooled_ns += ns;
    }
    return p;
}

// ---- convergence across the chains (-convergence): per series of the three tables R-hat, bulk and tail ESS, on the device
struct Conv { vector<double> rhat, ess_bulk, ess_tail; };
struct ConvAll { Conv T, V, I, G; };   // transcripts, isoforms without hits, identical sets, genes
static ConvAll fetch_convergence(const Chains &ch, const SeriesLayout &layout, uint32_t n)
{
    ConvAll c;
    const mmg_summary_desc cd = layout.desc();
    mmg_sampler *smp = ch.smp();
    mmg_convergence *conv = nullptr;
    MMG_TRY(mmg_convergence_create(smp, &cd, &conv));
    const Convergence owned(conv);
    auto fetch_conv = [&](int kind, size_t count, Conv &o) {
        o.rhat.assign(max<size_t>(count, 1), NAN); o.ess_bulk.assign(max<size_t>(count, 1), NAN); o.ess_tail.assign(max<size_t>(count, 1), NAN);
        MMG_TRY(mmg_convergence_get(conv, kind, o.rhat.data(), o.ess_bulk.data(), o.ess_tail.data()));
    };
    fetch_conv(MMG_SERIES_TRANSCRIPT, n, c.T);
    fetch_conv(MMG_SERIES_VIRTUAL, cd.n_virtual, c.V);
    fetch_conv(MMG_SERIES_IDENTICAL, cd.n_identical, c.I);
    fetch_conv(MMG_SERIES_GENE, cd.n_genes, c.G);
    return c;
}

// ---- the summary over all chains (-pool): the columns of the three tables from the kept samples of every chain, on the device
struct PooledSeries { vector<double> log_mean, var, tau, mcse2, pct; vector<int32_t> rc; };
struct PooledProps { vector<double> mean, probit_mean, probit_sd, pct; };
struct PooledAll { bool on = false; PooledSeries ser[4]; PooledProps prop[2]; };   // indexed by MMG_SERIES_*
static PooledAll fetch_pooled(const Options &opt, const Chains &ch, const SeriesLayout &layout, uint32_t n)
{
    PooledAll a;
    a.on = true;
    mmg_summary_desc pd = layout.desc();
    vector<int> pind;   // positions among the chains * trace_length pooled draws
    for (double p : opt.percentiles) pind.push_back(static_cast<int>(round(p / 100.0 * ((double)opt.chains * trace_length - 1))));
    pd.n_percentiles = (uint32_t)pind.size(); pd.percentile_index = pind.data();
    mmg_pooled *pooled = nullptr;
    MMG_TRY(mmg_pooled_create(ch.smp(), &pd, &pooled));
    const PooledSummary owned(pooled);
    const size_t nP = pind.size();
    const size_t counts[4] = {n, pd.n_virtual, pd.n_identical, pd.n_genes};
    for (int kind = 0; kind < 4; ++kind) {
        PooledSeries &o = a.ser[kind];
        const size_t c = max<size_t>(counts[kind], 1);
        o.log_mean.resize(c); o.var.resize(c); o.tau.resize(c); o.mcse2.resize(c); o.rc.resize(c); o.pct.resize(max<size_t>(counts[kind] * nP, 1));
        MMG_TRY(mmg_pooled_get(pooled, kind, o.log_mean.data(), o.var.data(), o.tau.data(), o.mcse2.data(), o.rc.data(), o.pct.data()));
    }
    for (int kind = 0; kind < 2; ++kind) {
        PooledProps &o = a.prop[kind];
        const size_t c = max<size_t>(counts[kind], 1);
        o.mean.resize(c); o.probit_mean.resize(c); o.probit_sd.resize(c); o.pct.resize(max<size_t>(counts[kind] * nP, 1));
        MMG_TRY(mmg_pooled_get_proportions(pooled, kind, o.mean.data(), o.probit_mean.data(), o.probit_sd.data(), o.pct.data()));
    }
    return a;
}

// ---- summary columns (src/mmseq.cpp:1110-1363) and the .mmseq, .identical.mmseq and .gene.mmseq tables
static void write_tables(const Options &opt, const Header &hdr, const Hits &hits, const Observed &obs, const UniqueHits &uh,
                         const vector<double> &mu_em, const SeriesLayout &layout, const Chains &ch, const Pooled &pooled, const PooledAll &all_chains,
                         StageTimer &stage)
{
    const uint32_t n = hits.n();
    const size_t nI = hdr.identical_transcripts.size(), nG = hdr.gene2transcripts.size(), nV = layout.simuIndex.size();
    const size_t nP = opt.percentiles.size();
    const long long numbermappedreads = hits.numbermappedreads;
    mmg_summary *summ = ch.summ.get();
    struct Series { vector<double> mean, sd, mcse, iact, pct; };
    auto fetch_series = [&](int kind, size_t count, Series &o) {
        o.mean.resize(max<size_t>(count, 1)); o.sd.resize(max<size_t>(count, 1)); o.mcse.resize(max<size_t>(count, 1));
        o.iact.resize(max<size_t>(count, 1)); o.pct.resize(max<size_t>(count * nP, 1));
        vector<double> var(max<size_t>(count, 1)), tau(max<size_t>(count, 1));
        vector<int32_t> rc(max<size_t>(count, 1));
        if (all_chains.on) { // -pool: the same columns from the draws of every chain; the Monte Carlo error is that of the mean of the chains' means
            const PooledSeries &ps = all_chains.ser[kind];
            o.mean = ps.log_mean; o.pct = ps.pct;
            for (size_t t = 0; t < count; ++t) {
                if (ps.rc[t] != 0) { o.mcse[t] = (double)opt.chains * trace_length; o.iact[t] = NAN; }
                else { o.mcse[t] = sqrt(ps.mcse2[t]); o.iact[t] = ps.tau[t]; }
                o.sd[t] = sqrt(ps.var[t]);
            }
            return;
        }
        MMG_TRY(mmg_summary_get(summ, kind, o.mean.data(), var.data(), tau.data(), rc.data(), o.pct.data()));
        for (size_t t = 0; t < count; ++t) { // :1311-1324
            if (rc[t] != 0) { o.mcse[t] = trace_length; o.iact[t] = NAN; }
            else { o.mcse[t] = sqrt(tau[t] * var[t] / trace_length); o.iact[t] = tau[t]; }
            o.sd[t] = sqrt(var[t]);
        }
    };
    Series sT, sV, sI, sG;
    fetch_series(MMG_SERIES_TRANSCRIPT, n, sT);
    if (!all_chains.on && opt.chains > 1 && pooled.ns > 1) { // all chains: mean and sd of log mu from the pooled moments, Monte Carlo error of the pooled mean
        for (uint32_t t = 0; t < n; ++t) {
            const double mean = pooled.sl[t] / (double)pooled.ns;
            const double var = (pooled.sl2[t] - (double)pooled.ns * mean * mean) / (double)(pooled.ns - 1);
            sT.mean[t] = mean;
            sT.sd[t] = sqrt(var > 0 ? var : 0.0);
            sT.mcse[t] = sT.mcse[t] / sqrt((double)opt.chains);
        }
    }
    fetch_series(MMG_SERIES_VIRTUAL, nV, sV);
    fetch_series(MMG_SERIES_IDENTICAL, nI, sI);
    fetch_series(MMG_SERIES_GENE, nG, sG);
    struct Props { vector<double> mean, probit_mean, probit_sd, pct; };
    auto fetch_props = [&](int kind, size_t count, Props &o) {
        o.mean.resize(max<size_t>(count, 1)); o.probit_mean.resize(max<size_t>(count, 1)); o.probit_sd.resize(max<size_t>(count, 1));
        o.pct.resize(max<size_t>(count * nP, 1));
        if (all_chains.on) {
            const PooledProps &pp = all_chains.prop[kind];
            o.mean = pp.mean; o.probit_mean = pp.probit_mean; o.probit_sd = pp.probit_sd; o.pct = pp.pct;
            return;
        }
        MMG_TRY(mmg_summary_get_proportions(summ, kind, o.mean.data(), o.probit_mean.data(), o.probit_sd.data(), o.pct.data()));
    };
    Props pT, pV;
    fetch_props(MMG_SERIES_TRANSCRIPT, n, pT);
    fetch_props(MMG_SERIES_VIRTUAL, nV, pV);
    auto pct_row = [&](const vector<double> &pct, size_t i) { return vector<double>(pct.begin() + (ptrdiff_t)(i * nP), pct.begin() + (ptrdiff_t)((i + 1) * nP)); };

    // the draws behind a row: a gene without observed transcripts has independent simulated draws, its mcse is sd / sqrt(draws)
    const double row_draws = all_chains.on ? (double)opt.chains * trace_length : (double)trace_length;
    const double digalpha = mmnum::digamma(opt.alpha);                 // gsl_sf_psi(alpha)        :1372
    const double sqrtpolygalpha = sqrt(mmnum::trigamma(opt.alpha));    // sqrt(gsl_sf_psi_n(1,.))  :1373
    auto prior_logmu = [&](const string &name) { return digalpha - log(opt.beta + hdr.len_of(name) * (double)numbermappedreads / 1000000000.0); };

    // ---- gene-level expression-weighted effective length (src/mmseq.cpp:1375-1395)
    vector<double> gene_lengths(nG, 0.0);
    {
        size_t g = 0;
        for (auto &gt : hdr.gene2transcripts) {
            if (isfinite(sG.mean[g]) != 0) {
                double sum = 0;
                for (auto &name : gt.second) {
                    const int32_t t = obs.of(name);
                    const double e = t >= 0 ? exp(sT.mean[t]) : exp(prior_logmu(name));
                    gene_lengths[g] += hdr.len_of(name) * e;
                    sum += e;
                }
                gene_lengths[g] /= sum;
            }
            g++;
        }
    }

    auto join_pct = [&](ostream &o, const vector<double> &v, const char *term) {
        for (size_t i = 0; i < nP; i++) { o << v[i]; o << (i == nP - 1 ? term : ","); }
    };
    auto pct_header = [&](ostream &o, const char *label, const char *term) {
        o << label;
        for (size_t i = 0; i < nP; i++) { o << opt.percentiles[i]; o << (i == nP - 1 ? term : ","); }
    };

    // ---- .gene.mmseq (src/mmseq.cpp:1615-1669)
    auto write_gene_table = [&]() {
    ofstream ofs((opt.output_base + ".gene.mmseq").c_str());
    ofs << "# Mapped fragments: " << numbermappedreads << endl;
    ofs << "feature_id\tlog_mu\tsd\tmcse\tiact\teffective_length\ttrue_length\tunique_hits\tntranscripts\tobserved\t";
    pct_header(ofs, "percentiles", "\n");
    {
        size_t g = 0;
        for (auto &gt : hdr.gene2transcripts) {
            bool observed = false;
            for (auto &name : gt.second) if (obs.of(name) >= 0) { observed = true; break; }
            if (observed) {
                ofs << gt.first << "\t" << sG.mean[g] << "\t" << sG.sd[g] << "\t" << sG.mcse[g] << "\t" << sG.iact[g] << "\t"
                    << gene_lengths[g] << "\t"
                    << "NA"
                    << "\t" << uh.gene[g] << "\t" << gt.second.size() << "\t"
                    << "1"
                    << "\t";
            } else {
                ofs << gt.first << "\t" << sG.mean[g] << "\t" << sG.sd[g] << "\t" << sG.sd[g] / sqrt(row_draws) << "\t" << 1 << "\t"
                    << gene_lengths[g] << "\t"
                    << "NA"
                    << "\t"
                    << "0"
                    << "\t" << gt.second.size() << "\t"
                    << "0"
                    << "\t";
            }
            join_pct(ofs, pct_row(sG.pct, g), "\n");
            g++;
        }
    }
    ofs.close();
    };

    stage.mark("summary columns");
    // ---- .mmseq (src/mmseq.cpp:1469-1554)
    ofstream ofs((opt.output_base + ".mmseq").c_str());
    ofs << "# Mapped fragments: " << numbermappedreads << endl;
    ofs << "feature_id\tlog_mu\tsd\tmcse\tiact\teffective_length\ttrue_length\tunique_hits\tmean_proportion\tmean_probit_proportion\tsd_"
           "probit_proportion\tlog_mu_em\tobserved\tntranscripts\t";
    pct_header(ofs, "percentiles", "\t");
    pct_header(ofs, "percentiles_proportion", "\n");
    // (the rows are formatted in parallel, a slice of the list per thread into a stream of its own with the default formatting of
    // the file stream, and written in order; the gene table, which shares nothing with this one, is written by a thread of its own)
    auto mmseq_row = [&](ostream &o, const string &name) {
        const int32_t t = obs.of(name);
        if (t >= 0) {
            o << name << "\t" << sT.mean[t] << "\t" << sT.sd[t] << "\t" << sT.mcse[t] << "\t" << sT.iact[t] << "\t" << hdr.len_of(name) << "\t"
                << hdr.seqlen_of(name) << "\t" << uh.transcript[t] << "\t" << pT.mean[t] << "\t" << pT.probit_mean[t] << "\t"
                << pT.probit_sd[t] << "\t" << log(mu_em[t]) << "\t"
                << "1"
                << "\t" << hdr.gene_size_of(name) << "\t";
            join_pct(o, pct_row(sT.pct, t), "\t");
            join_pct(o, pct_row(pT.pct, t), "\n");
        } else {
            const uint32_t v = layout.simu_of(name);
            o << name << "\t" << prior_logmu(name) << "\t" << sqrtpolygalpha << "\t"
                << "0"
                << "\t"
                << "1"
                << "\t" << hdr.len_of(name) << "\t" << hdr.seqlen_of(name) << "\t" << 0 << "\t" << pV.mean[v] << "\t"
                << pV.probit_mean[v] << "\t" << pV.probit_sd[v] << "\t"
                << "NA"
                << "\t"
                << "0"
                << "\t" << hdr.gene_size_of(name) << "\t";
            join_pct(o, pct_row(sV.pct, v), "\t");
            join_pct(o, pct_row(pV.pct, v), "\n");
        }
        };
    JoiningThread gene_table([&]() { write_gene_table(); });
    {
        const vector<string> &transcriptList = hdr.transcriptList;
        const int tt = max(1, min(omp_get_max_threads(), (int)(transcriptList.size() / 4096) + 1));
        vector<string> parts((size_t)tt);
#pragma omp parallel num_threads(tt)
        {
            const size_t me = (size_t)omp_get_thread_num(), nt = (size_t)omp_get_num_threads();
            const size_t lo = transcriptList.size() * me / nt, hi = transcriptList.size() * (me + 1) / nt;
            ostringstream o;
            for (size_t i = lo; i < hi; ++i) mmseq_row(o, transcriptList[i]);
            parts[me] = o.str();
        }
        for (auto &pt : parts) ofs.write(pt.data(), (streamsize)pt.size());
    }
    ofs.close(); ofs.clear();

    // ---- .identical.mmseq (src/mmseq.cpp:1556-1613)
    ofs.open((opt.output_base + ".identical.mmseq").c_str());
    ofs << "# Mapped fragments: " << numbermappedreads << endl;
    ofs << "feature_id\tlog_mu\tsd\tmcse\tiact\teffective_length\ttrue_length\tunique_hits\tobserved\tntranscripts\t";
    pct_header(ofs, "percentiles", "\n");
    for (size_t v = 0; v < nI; ++v) {
        const vector<string> &set = hdr.identical_transcripts[v];
        const bool fin = isfinite(sI.mean[v]);
        for (auto &name : set) {
            ofs << name;
            if (name.compare(set.back()) != 0) ofs << "+";
            else if (fin)
                ofs << "\t" << sI.mean[v] << "\t" << sI.sd[v] << "\t" << sI.mcse[v] << "\t" << sI.iact[v] << "\t"
                    << hdr.len_of(set.front()) << "\t" << hdr.seqlen_of(set.front()) << "\t" << uh.identical[v] << "\t"
                    << "1"
                    << "\t" << set.size() << "\t";
            else
                ofs << "\t" << log((double)set.size()) + prior_logmu(name) << "\t" << sqrtpolygalpha << "\t"
                    << "0"
                    << "\t"
                    << "NA"
                    << "\t" << hdr.len_of(set.front()) << "\t" << hdr.seqlen_of(set.front()) << "\t" << 0 << "\t"
                    << "0"
                    << "\t" << set.size() << "\t";
        }
        if (fin) join_pct(ofs, pct_row(sI.pct, v), "\n");
        else for (size_t i = 0; i < nP; i++) ofs << "NA" << (i == nP - 1 ? "\n" : ",");
    }
    ofs.close(); ofs.clear();
}

// ---- the convergence tables: the rows of .mmseq, .identical.mmseq and .gene.mmseq, in their order, with their feature ids
static void write_convergence_tables(const Options &opt, const Header &hdr, const Observed &obs, const SeriesLayout &layout, const ConvAll &c)
{
    auto conv_head = [&](ostream &o) {
        o << "# chains " << opt.chains << ", samples per chain " << trace_length << endl;
        o << "feature_id\trhat\tess_bulk\tess_tail" << endl;
    };
    auto conv_row = [&](ostream &o, const Conv &cv, size_t i) { o << "\t" << cv.rhat[i] << "\t" << cv.ess_bulk[i] << "\t" << cv.ess_tail[i] << "\n"; };
    ofstream ofs((opt.output_base + ".convergence").c_str());
    conv_head(ofs);
    for (auto &name : hdr.transcriptList) {
        const int32_t t = obs.of(name);
        ofs << name;
        if (t >= 0) conv_row(ofs, c.T, (size_t)t);
        else conv_row(ofs, c.V, layout.simu_of(name));
    }
    ofs.close(); ofs.clear();
    ofs.open((opt.output_base + ".identical.convergence").c_str());
    conv_head(ofs);
    for (size_t v = 0; v < hdr.identical_transcripts.size(); ++v) {
        ofs << layout.identical_ids[v]; // (the id of .identical.mmseq)
        conv_row(ofs, c.I, v);
    }
    ofs.close(); ofs.clear();
    ofs.open((opt.output_base + ".gene.convergence").c_str());
    conv_head(ofs);
    size_t g = 0;
    for (auto &gt : hdr.gene2transcripts) { ofs << gt.first; conv_row(ofs, c.G, g++); }
}

// ---- -assign: the posterior assignment probability of every hit, and the expected hits per transcript and gene that follow from it.
//      The device pass (mmg_assign_*) runs over chain 0's trace_length kept samples -- the samples the .mmseq summaries are taken over
//      (mmg_summary_begin with chain 0 in start_chains; post.hip reads all cfg.trace_len samples of that chain) -- on the rows as the
//      .M file lists them: first-seen order, observed-transcript numbering.  The sums over hits are the host's, in ascending hit index.
static void write_assignments(const Options &opt, const Header &hdr, const Hits &hits, const Observed &obs, const Chains &ch)
{
    const uint64_t m = hits.m(), H = hits.col_idx.size();
    const uint32_t n = hits.n();
    vector<double> P(max<uint64_t>(H, 1));
    {
        mmg_assign *raw = nullptr;
        MMG_TRY(mmg_assign_create(opt.device, m, n, hits.row_ptr.data(), hits.col_idx.data(), &raw));
        Assign as(raw);
        MMG_TRY(mmg_assign_run_sampler(raw, ch.smp(), 0, 0, trace_length));
        MMG_TRY(mmg_assign_get(raw, 0, H, P.data()));
    }
    // .assign: the lines of .M (start_km_writer) with a third column; chunks of rows formatted in parallel, written in order
    {
        ofstream ofs((opt.output_base + ".assign").c_str());
        const int threads = max(1, omp_get_max_threads());
        const uint64_t chunk = 1u << 14;
        const int64_t nchunks = (int64_t)((m + chunk - 1) / chunk), batch = max<int64_t>(1, threads * 2);
        for (int64_t c0 = 0; c0 < nchunks; c0 += batch) {
            const int64_t nb = min(batch, nchunks - c0);
            vector<string> out(nb);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
            for (int64_t c = 0; c < nb; ++c) {
                const uint64_t r0 = (uint64_t)(c0 + c) * chunk, r1 = min<uint64_t>(m, r0 + chunk);
                string &o = out[c];
                char tmp[96];
                for (uint64_t i = r0; i < r1; ++i)
                    for (uint64_t j = hits.row_ptr[i]; j < hits.row_ptr[i + 1]; ++j)
                        o.append(tmp, (size_t)snprintf(tmp, sizeof tmp, "%llu\t%u\t%.9g\n", (unsigned long long)i, hits.col_idx[j], P[j]));
            }
            for (auto &x : out) ofs.write(x.data(), (streamsize)x.size());
        }
        ofs.close();
        if (!ofs) fatal("cannot write " + opt.output_base + ".assign");
    }
    vector<double> expected(n, 0.0);
    for (uint64_t i = 0; i < m; ++i)
        for (uint64_t j = hits.row_ptr[i]; j < hits.row_ptr[i + 1]; ++j) expected[hits.col_idx[j]] += (double)hits.k[i] * P[j];
    auto of_name = [&](const string &name) { const int32_t t = obs.of(name); return t >= 0 ? expected[t] : 0.0; };
    auto line = [](ostream &o, const string &id, double v) {
        char tmp[40];
        snprintf(tmp, sizeof tmp, "%.9g", v);
        o << id << "\t" << tmp << "\n";
    };
    ofstream ofs((opt.output_base + ".counts").c_str());          // the rows of .mmseq, in its order
    ofs << "feature_id\texpected_hits\n";
    for (auto &name : hdr.transcriptList) line(ofs, name, of_name(name));
    ofs.close();
    if (!ofs) fatal("cannot write " + opt.output_base + ".counts");
    ofs.clear();
    ofs.open((opt.output_base + ".gene.counts").c_str());         // the rows of .gene.mmseq; a gene's isoforms added in @GeneIsoforms order
    ofs << "feature_id\texpected_hits\n";
    for (auto &gt : hdr.gene2transcripts) {
        double sum = 0.0;
        for (auto &name : gt.second) sum += of_name(name);
        line(ofs, gt.first, sum);
    }
    ofs.close();
    if (!ofs) fatal("cannot write " + opt.output_base + ".gene.counts");
}

// ---- -contrasts: the file is read against the header's ids right after the header, before the reads and any device work
static ContrastsFile read_contrasts(const Options &opt, const Header &hdr)
{
    ContrastsFile cf;
    if (opt.contrasts_file.empty()) return cf;
    unordered_map<string, uint32_t> header_index;
    header_index.reserve(hdr.transcriptList.size());
    for (size_t i = 0; i < hdr.transcriptList.size(); ++i) header_index[hdr.transcriptList[i]] = (uint32_t)i;
    string error;
    if (!read_contrasts_file(opt.contrasts_file, header_index, cf, error)) fatal(error);
    return cf;
}

// ---- .contrasts.mmseq: per contrast the posterior of log(sum of mu over the numerator / sum over the denominator) over chain 0's
//      trace_length kept samples -- the samples the .mmseq summaries are taken over -- on the device (mmg_contrast_*).  The columns
//      mmdiff reads are there under its names: log_mu is the mean log-ratio, sd its posterior standard deviation.
static void write_contrasts(const Options &opt, const Header &hdr, const Hits &hits, const Observed &obs, const UniqueHits &uh,
                            const SeriesLayout &layout, const Chains &ch, const ContrastsFile &cf)
{
    const uint32_t n = hits.n();
    const size_t C = cf.size(), nP = opt.percentiles.size();
    vector<uint64_t> ptr[2] = {{0}, {0}};
    vector<uint32_t> mem[2];
    vector<long long> side_hits[2];
    vector<char> side_observed[2];
    for (size_t c = 0; c < C; ++c)
        for (int k = 0; k < 2; ++k) {
            long long hits_sum = 0;
            bool any = false;
            for (uint32_t hidx : (k == 0 ? cf.num[c] : cf.den[c])) {
                const string &name = hdr.transcriptList[hidx];
                const int32_t t = obs.of(name);
                if (t >= 0) { mem[k].push_back((uint32_t)t); hits_sum += uh.transcript[t]; any = true; }
                else mem[k].push_back(n + layout.simu_of(name));   // no hits: its simulated trace
            }
            ptr[k].push_back(mem[k].size());
            side_hits[k].push_back(hits_sum);
            side_observed[k].push_back(any);
        }
    mmg_contrast_desc cd;
    memset(&cd, 0, sizeof cd);
    cd.n_contrasts = (uint32_t)C;
    cd.num_ptr = ptr[0].data(); cd.num_member = mem[0].data();
    cd.den_ptr = ptr[1].data(); cd.den_member = mem[1].data();
    cd.n_percentiles = (uint32_t)layout.pind.size(); cd.percentile_index = layout.pind.data();
    vector<double> mean(C), var(C), tau(C), p_gt(C), pct(max<size_t>(C * nP, 1));
    vector<int32_t> rc(C);
    {
        mmg_contrast *raw = nullptr;
        MMG_TRY(mmg_contrast_create(ch.smp(), ch.summ.get(), &cd, &raw));
        Contrast owned(raw);
        MMG_TRY(mmg_contrast_get(raw, mean.data(), var.data(), tau.data(), rc.data(), p_gt.data(), pct.data()));
    }
    ofstream ofs((opt.output_base + ".contrasts.mmseq").c_str());
    ofs << "# Log-ratios between transcript sets of this sample: log_mu is the posterior mean of log(numerator / denominator); mmdiff needs -nonorm on this table" << endl;
    ofs << "feature_id\tlog_mu\tsd\tmcse\tiact\tunique_hits\tp_gt\tn_num\tn_den\tobserved\t";
    ofs << "percentiles";
    for (size_t i = 0; i < nP; i++) { ofs << opt.percentiles[i]; ofs << (i == nP - 1 ? "\n" : ","); }
    for (size_t c = 0; c < C; ++c) {
        // sd, mcse, iact as write_tables' fetch_series derives them (:1311-1324)
        const double sd = sqrt(var[c]);
        const double mcse = rc[c] != 0 ? (double)trace_length : sqrt(tau[c] * var[c] / trace_length);
        const double iact = rc[c] != 0 ? NAN : tau[c];
        ofs << cf.names[c] << "\t" << mean[c] << "\t" << sd << "\t" << mcse << "\t" << iact << "\t" << min(side_hits[0][c], side_hits[1][c]) << "\t"
            << p_gt[c] << "\t" << cf.num[c].size() << "\t" << cf.den[c].size() << "\t" << (side_observed[0][c] && side_observed[1][c] ? "1" : "0") << "\t";
        for (size_t i = 0; i < nP; i++) { ofs << pct[c * nP + i]; ofs << (i == nP - 1 ? "\n" : ","); }
    }
    ofs.close();
    if (!ofs) fatal("cannot write " + opt.output_base + ".contrasts.mmseq");
}

// ---- -pairs: every two transcripts that share a hit set of at most -pairs_maxset transcripts, in the header's transcript order
//      (pairs_gen.hpp); generated before any device work, so that a refusal costs nothing
static pairsgen::Result generate_pairs(const Options &opt, const Hits &hits)
{
    pairsgen::Result r;
    if (!opt.pairs) return r;
    string error;
    if (!pairsgen::generate(hits.m(), hits.row_ptr.data(), hits.col_idx.data(), hits.k.data(), hits.obs2hdr.data(), opt.pairs_maxset, r, error)) fatal(error);
    return r;
}

// ---- .pairs: per pair the posterior correlation of log mu_a and log mu_b, their sd, the sd and mean of log(mu_a + mu_b) and the
//      share of samples with mu_a > mu_b over chain 0's trace_length kept samples -- the samples the .mmseq summaries are taken
//      over -- on the device (mmg_pairs_*); cor, the sd and the share are derived here from the sums the device returns
static void write_pairs(const Options &opt, const Header &hdr, const Hits &hits, const Chains &ch, const pairsgen::Result &gen)
{
    const size_t P = gen.pairs.size();
    vector<double> mean_sum(P), saa(P), sbb(P), sab(P), sss(P);
    vector<uint32_t> n_gt(P);
    if (P) {
        vector<int32_t> hdr2obs(hdr.transcriptList.size(), -1);
        for (uint32_t t = 0; t < hits.n(); ++t) hdr2obs[hits.obs2hdr[t]] = (int32_t)t;
        vector<uint32_t> a(P), b(P);
        for (size_t p = 0; p < P; ++p) { a[p] = (uint32_t)hdr2obs[gen.pairs[p].a]; b[p] = (uint32_t)hdr2obs[gen.pairs[p].b]; }
        mmg_pairs *raw = nullptr;
        MMG_TRY(mmg_pairs_create(ch.smp(), 0, P, a.data(), b.data(), &raw));
        Pairs owned(raw);
        MMG_TRY(mmg_pairs_get(raw, nullptr, nullptr, mean_sum.data(), saa.data(), sbb.data(), sab.data(), sss.data(), n_gt.data()));
    }
    ofstream ofs((opt.output_base + ".pairs").c_str());
    ofs << "# " << P << " pairs of transcripts that share a hit set of at most " << opt.pairs_maxset << " transcripts (-pairs_maxset); "
        << gen.skipped_sets << " larger sets skipped with " << gen.skipped_hits << " hits" << endl;
    ofs << "feature_a\tfeature_b\tshared_hits\tshared_sets\tcor\tsd_a\tsd_b\tsd_sum\tlog_mu_sum\tp_a_gt_b\n";
    const double d = (double)trace_length - 1.0;
    for (size_t p = 0; p < P; ++p) {
        const pairsgen::Pair &g = gen.pairs[p];
        ofs << hdr.transcriptList[g.a] << "\t" << hdr.transcriptList[g.b] << "\t" << g.shared_hits << "\t" << g.shared_sets << "\t"
            << sab[p] / (sqrt(saa[p]) * sqrt(sbb[p])) << "\t" << sqrt(saa[p] / d) << "\t" << sqrt(sbb[p] / d) << "\t" << sqrt(sss[p] / d) << "\t"
            << mean_sum[p] << "\t" << (double)n_gt[p] / (double)trace_length << "\n";
    }
    ofs.close();
    if (!ofs) fatal("cannot write " + opt.output_base + ".pairs");
}

// ---- -isoforms: .isoforms and .gene.isoforms.  The groups are the genes of the summary (the hits header's, isoforms without hits as
//      their simulated traces), the samples chain 0's trace_length kept samples -- the samples the .mmseq summaries are taken over --
//      and everything per sample happens on the device (mmg_isoform_*).  From its counts and sums come, here: the shares count / S,
//      sd = sqrt(ss / (S - 1)), the effective number of isoforms exp(mean entropy), and an isoform's rank in its gene by the number
//      of samples it tops (the earlier of equals first).  A gene with a draw that is not valid prints NA and nan, and its status.
static void write_isoforms(const Options &opt, const Header &hdr, const SeriesLayout &layout, const Chains &ch)
{
    const size_t G = layout.gptr.size() - 1, NM = layout.gmem.size(), nq = opt.iso_thresholds.size(), nP = opt.percentiles.size();
    vector<uint32_t> n_top(NM), n_second(NM), n_above(max<size_t>(NM * nq, 1)), major(G), n_distinct(G);
    vector<uint8_t> status(G);
    vector<double> mean_H(G), ss_H(G), mean_P(G), ss_P(G), q_H(max<size_t>(G * nP, 1)), q_P(max<size_t>(G * nP, 1));
    if (G) {
        const vector<uint32_t> ranks(layout.pind.begin(), layout.pind.end());
        mmg_isoform_desc d;
        memset(&d, 0, sizeof d);
        d.n_groups = (uint32_t)G; d.ptr = layout.gptr.data(); d.member = layout.gmem.data();
        d.n_thresholds = (uint32_t)nq; d.threshold = opt.iso_thresholds.data();
        d.n_ranks = (uint32_t)ranks.size(); d.rank = ranks.data();
        mmg_isoform *raw = nullptr;
        MMG_TRY(mmg_isoform_create(ch.smp(), ch.summ.get(), &d, &raw));
        Isoform owned(raw);
        MMG_TRY(mmg_isoform_get_members(raw, n_top.data(), n_second.data(), n_above.data()));
        MMG_TRY(mmg_isoform_get_groups(raw, status.data(), major.data(), n_distinct.data(), mean_H.data(), ss_H.data(), mean_P.data(), ss_P.data(),
                                       q_H.data(), q_P.data()));
    }
    const double S = (double)trace_length;
    auto comment = [&](ostream &o) {
        o << "# Isoform usage from the joint draws of a gene's isoforms: S = " << trace_length << " kept samples of chain 0; thresholds: ";
        for (size_t q = 0; q < nq; ++q) o << opt.iso_thresholds[q] << (q + 1 < nq ? "," : "");
        o << endl;
    };
    // where a transcript sits: its gene and its entry of the flat member list (the order series_layout built them in)
    unordered_map<string, pair<uint32_t, uint64_t>> where;
    where.reserve(NM);
    vector<uint32_t> rank(NM, 0);
    {
        size_t g = 0;
        uint64_t at = 0;
        vector<uint32_t> order;
        for (auto &gt : hdr.gene2transcripts) {
            for (auto &name : gt.second) where[name] = {(uint32_t)g, at++};
            const uint64_t b = layout.gptr[g], K = layout.gptr[g + 1] - b;
            order.resize(K);
            for (uint32_t j = 0; j < K; ++j) order[j] = j;
            stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return n_top[b + x] > n_top[b + y]; });
            for (uint32_t r = 0; r < K; ++r) rank[b + order[r]] = r + 1;
            ++g;
        }
    }
    ofstream ofs((opt.output_base + ".isoforms").c_str());
    comment(ofs);
    ofs << "feature_id\tgene_id\tn_isoforms\trank_in_gene\tp_major\tp_second";
    for (size_t q = 0; q < nq; ++q) ofs << "\tp_above_" << opt.iso_thresholds[q];
    ofs << "\n";
    for (auto &name : hdr.transcriptList) {
        auto it = where.find(name);
        if (it == where.end()) {   // a transcript the header puts in no gene
            ofs << name << "\tNA\t0\tNA\tnan\tnan";
            for (size_t q = 0; q < nq; ++q) ofs << "\tnan";
            ofs << "\n";
            continue;
        }
        const uint32_t g = it->second.first;
        const uint64_t j = it->second.second;
        const bool ok = status[g] == 0;
        ofs << name << "\t" << layout.gene_ids[g] << "\t" << layout.gptr[g + 1] - layout.gptr[g] << "\t";
        if (ok) ofs << rank[j]; else ofs << "NA";
        ofs << "\t" << (ok ? n_top[j] / S : NAN) << "\t" << (ok ? n_second[j] / S : NAN);
        for (size_t q = 0; q < nq; ++q) ofs << "\t" << (ok ? n_above[j * nq + q] / S : NAN);
        ofs << "\n";
    }
    ofs.close();
    if (!ofs) fatal("cannot write " + opt.output_base + ".isoforms");

    ofstream ofg((opt.output_base + ".gene.isoforms").c_str());
    comment(ofg);
    ofg << "gene_id\tn_isoforms\tmajor_id\tp_major\tn_distinct\tentropy\tentropy_sd\teff_isoforms\tmax_prop\tmax_prop_sd\t";
    for (const char *what : {"percentiles_entropy", "percentiles_max_prop"}) {
        ofg << what;
        for (size_t i = 0; i < nP; i++) ofg << opt.percentiles[i] << (i == nP - 1 ? "\t" : ",");
    }
    ofg << "status\n";
    size_t g = 0;
    for (auto &gt : hdr.gene2transcripts) {
        const bool ok = status[g] == 0;
        const uint64_t b = layout.gptr[g];
        ofg << gt.first << "\t" << gt.second.size() << "\t" << (ok ? gt.second[major[g]] : string("NA")) << "\t" << (ok ? n_top[b + major[g]] / S : NAN) << "\t"
            << n_distinct[g] << "\t" << mean_H[g] << "\t" << sqrt(ss_H[g] / (S - 1.0)) << "\t" << exp(mean_H[g]) << "\t" << mean_P[g] << "\t"
            << sqrt(ss_P[g] / (S - 1.0)) << "\t";
        for (const vector<double> *qv : {&q_H, &q_P})
            for (size_t i = 0; i < nP; i++) ofg << (*qv)[g * nP + i] << (i == nP - 1 ? "\t" : ",");
        ofg << (int)status[g] << "\n";
        ++g;
    }
    ofg.close();
    if (!ofg) fatal("cannot write " + opt.output_base + ".gene.isoforms");
}

static void print_parameters(const Options &opt, int max_threads)
{
    cout << "Running mmseq with parameters:\n"
         << "  alpha:         " << opt.alpha << endl
         << "  beta:          " << opt.beta << endl
         << "  max_em_iter:   " << opt.max_em_iter << endl
         << "  epsilon:       " << opt.epsilon << endl
         << "  gibbs_iter:    " << opt.gibbs_iter << endl
         << "  gibbs_ss:      " << opt.gibbs_ss << endl
         << "  seed[0]:       " << opt.seed << endl
         << "  debug:         " << opt.debug << endl
         << "  threads:       " << max_threads << endl
         << "  device:        " << opt.device << " (HIP, libmmgibbs ABI " << mmg_abi_version() << ")" << endl
         << "  gpus:          " << opt.gpus << endl
         << "  chains:        " << opt.chains << endl;
}

static void print_output_files(const Options &opt)
{
    cout << "done." << endl;
    cout << "Output files: " << endl
         << "  " << opt.output_base << ".mmseq" << endl
         << "  " << opt.output_base << ".identical.mmseq" << endl
         << "  " << opt.output_base << ".gene.mmseq" << endl;
    cout << "  " << opt.output_base << ".M" << endl << "  " << opt.output_base << ".k" << endl << endl;
    cout << "  " << opt.output_base << ".trace_gibbs.gz" << endl
         << "  " << opt.output_base << ".identical.trace_gibbs.gz" << endl
         << "  " << opt.output_base << ".gene.trace_gibbs.gz" << endl
         << "  " << opt.output_base << ".prop.trace_gibbs.gz" << endl
         << endl;
    if (opt.assign)
        cout << "  " << opt.output_base << ".assign" << endl
             << "  " << opt.output_base << ".counts" << endl
             << "  " << opt.output_base << ".gene.counts" << endl
             << endl;
    if (!opt.contrasts_file.empty()) cout << "  " << opt.output_base << ".contrasts.mmseq" << endl << endl;
    if (opt.pairs) cout << "  " << opt.output_base << ".pairs" << endl << endl;
    if (opt.isoforms)
        cout << "  " << opt.output_base << ".isoforms" << endl
             << "  " << opt.output_base << ".gene.isoforms" << endl
             << endl;
    if (opt.auto_on) cout << "  " << opt.output_base << ".autolength" << endl << endl;
    if (opt.debug) {
        cout << endl
             << "  " << opt.output_base << ".trace_em.gz" << endl
             << "  " << opt.output_base << ".sharedcounts" << endl
             << "  " << opt.output_base << ".Mt-nodups" << endl
             << "  " << opt.output_base << ".doublehits" << endl
             << "  " << opt.output_base << ".dupIDs" << endl;
    }
}

// The stages in order.  Declaration order is release order reversed: on an Exit the trace writers stop first, then the library
// handles go, then the .k / .M writer and the device warm-up thread are joined.
static int run(int argc, char **argv)
{
    StageTimer stage;
    if (!getenv("OMP_NUM_THREADS")) { // an explicit thread count is the user's (src/mmseq.cpp:323 prints it); otherwise respect the quota
        const int q = cpu_quota();
        if (q > 0 && q < omp_get_max_threads()) omp_set_num_threads(q);
    }
    const int max_threads = omp_get_max_threads();
    Options opt = parse_options(argc, argv);   // (-gibbs_auto: gibbs_iter and gibbs_ss become the length the run stopped at)
    HitsfileReader hitsfileReader(opt.hits_file);
    print_parameters(opt, max_threads);

    // The HIP runtime, the device context and the library's code object are brought up while the hits file is read (they are first
    // needed at the device problem build, where they used to cost about two seconds of an otherwise idle GPU): one tiny kernel
    // launch on a thread of its own.  Its result is ignored -- a device that cannot be used is reported by mmg_problem_create.
    // Every way out of run() joins it first: exit() under a thread that is still INSIDE the runtime's initialisation tears the
    // runtime down under its feet (found by tools/hitsio_fuzz.py: 7 of 800 runs on damaged headers ended in the sanitizer's allocator
    // instead of with exit code 1).
    JoiningThread device_warmup([device = opt.device]() {
        const uint32_t ctr[4] = {0, 0, 0, 0}, key[2] = {0, 0};
        uint32_t out[6];
        (void)mmg_selftest_philox(device, ctr, key, out);
    });
    const Header hdr = read_header(hitsfileReader);
    const ContrastsFile contrasts = read_contrasts(opt, hdr);
    const Hits hits = ingest(hitsfileReader, opt.hits_file, hdr.transcriptList.size(), stage.on);
    stage.mark("read hits file + collapse");
    const vector<double> l = effective_lengths(hdr, hits);
    const vector<vector<int>> counts_shared = opt.debug ? shared_counts(hits) : vector<vector<int>>();
    stage.mark("l");
    const pairsgen::Result pair_list = generate_pairs(opt, hits);
    const Observed obs(hdr, hits);
    UniqueHits uh = count_unique_hits(hdr, hits, obs);
    stage.mark("unique hits (sets, genes)");
    JoiningThread km_writer = start_km_writer(opt.output_base, hits, obs);
    if (opt.debug) write_debug_files(opt.output_base, hdr, hits, obs, counts_shared);
    stage.mark("start the .k .M writer");
    {
        Device dev;
        vector<double> mu(hits.n(), 0.0);
        uh.transcript.assign(hits.n(), 0);
        dev.prob = build_problem(opt, hdr, hits, obs, l, device_warmup, stage, mu, uh.transcript);
        spread(opt, dev, mu, stage);
        const vector<double> mu_em = run_em(opt, obs, dev, std::move(mu), stage);
        stage.mark("EM");
        const SeriesLayout layout = series_layout(opt, hdr, hits, obs);
        Chains ch = start_chains(opt, dev, mu_em, layout);
        TraceWriters writers;   // (stopped and joined before the summary and samplers they read are released)
        if (opt.auto_on) run_gibbs_auto(opt, obs, layout, ch, (uint32_t)hits.n(), writers, stage);
        else run_gibbs(opt, obs, layout, dev, ch, writers, stage);
        const Pooled pooled = pool_moments(opt, dev, ch, hits.n());
        cout << "Amalgamating transcripts and calculating summary statistics..." << flush;
        // ---- posterior summary on the device (src/mmseq.cpp:927-1363): the derived traces were computed while the chain ran; what is
        //      left are the per-series columns -- percentiles, log means, Sokal -- of which only the columns come back.
        mmg_summary *summ = ch.summ.get();
        MMG_TRY(mmg_summary_finish(summ));
        stage.mark("device summary");
        ConvAll conv;
        if (opt.convergence) {
            conv = fetch_convergence(ch, layout, hits.n());
            stage.mark("convergence diagnostics");
        }
        PooledAll all_chains;
        if (opt.pool) {
            all_chains = fetch_pooled(opt, ch, layout, hits.n());
            stage.mark("summary over all chains");
        }
        write_tables(opt, hdr, hits, obs, uh, mu_em, layout, ch, pooled, all_chains, stage);
        if (opt.convergence) {
            write_convergence_tables(opt, hdr, obs, layout, conv);
            stage.mark("convergence tables");
        }
        if (opt.assign) {
            stage.mark("write tables");
            write_assignments(opt, hdr, hits, obs, ch);
        }
        if (!opt.contrasts_file.empty()) {
            stage.mark(opt.assign ? "assignment probabilities" : "write tables");
            write_contrasts(opt, hdr, hits, obs, uh, layout, ch, contrasts);
        }
        const char *before_pairs = !opt.contrasts_file.empty() ? "contrasts" : opt.assign ? "assignment probabilities" : "write tables";
        if (opt.pairs) {
            stage.mark(before_pairs);
            write_pairs(opt, hdr, hits, ch, pair_list);
        }
        const char *before_isoforms = opt.pairs ? "pairs" : before_pairs;
        if (opt.isoforms) {
            stage.mark(before_isoforms);
            write_isoforms(opt, hdr, layout, ch);
        }
        print_output_files(opt);
        stage.mark(opt.isoforms ? "isoform usage" : before_isoforms);
        // (the writers fetch the last 1/64 of the rows behind the loop's last check: a failure there -- a HIP error in a row fetch --
        // would leave a valid but truncated trace file; it ends the run like any other)
        writers.finish();
    }   // the summary, the samplers, the problems and the group are released here, once the trace writers are done
    stage.mark("trace files: the rest");
    km_writer.join();
    stage.mark("wait for the .k .M writer");
    stage.total();
    return 0;
}

int main(int argc, char **argv)
{
    try {
        return run(argc, argv);
    } catch (const Exit &e) {
        return e.code;
    }
}
