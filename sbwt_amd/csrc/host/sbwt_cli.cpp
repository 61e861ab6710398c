// sbwt_cli.cpp -- the `sbwt` command: `search` with the reference's flags, output format and log
// lines (reference src/CLI/sbwt_search.cpp, src/CLI/sbwt.cpp), running the queries on the GPU in
// batches; plus a minimal in-memory `build` so that indexes can be produced without KMC.
//
//   sbwt build  -i <in> -o <index> -k <k> [-p <precalc>] [--add-reverse-complements]
//               [--no-streaming-support] [-t <threads>]      (subset of sbwt_build.cpp:40-55)
//   sbwt search -o <out> -i <index> -q <query> [-z]        (sbwt_search.cpp:151-157)
//   sbwt matching-statistics -i <index> -q <query> -o <out> [-z] [--intervals]
//               k-bounded matching statistics: one line per read, one token per base ("d", or "d,first,second")
//   sbwt dump-unitigs -i <index> -o <out> [-z] [--gfa] [--colors <colours> [--sets-out <sets.txt>]]
//               the index turned back into sequence: FASTA, one record per unitig, the header the unitig's number; --colors
//               cuts the unitigs where the colour set changes (header "number set-id"); --gfa writes GFA 1, the unitigs as
//               segments and the links between them
//   sbwt thread -i <index> -q <reads> -o <walks> [-z] [--colors <colours>] [--coverage <cov.tsv>] [--gfa <graph.gfa>]
//               the reads threaded through the unitig graph: one line per read, its number, then one
//               `read_pos:unitig:offset:n_kmers` per step; --coverage: `unitig n_kmers kmer_hits` per unitig
//   sbwt bubbles -i <index> [-c <colours>] -o <bubbles.tsv> [-z] [--snps-only]
//               [-q <reads> [--both-strands] [--min-breadth 1.0] [--min-depth 1] [--refs-out <refs.tsv>] [--batch-bases <n>]]
//               the variant sites of the unitig graph: a header line, then per bubble source, branches, sink, k-mers of each
//               branch, SNP|OTHER and the two alleles; with -c the colours of each branch; with -q the reads genotyped at the
//               bubbles: per allele the k-mers seen, the hits and the smallest k-mer depth, and the call (. a b ab)
//   sbwt set-op -a <index A> -b <index B> [--op union|intersection|difference|symmetric-difference] -o <index> [--counts-only]
//               two index files combined on the GPU without their input sequences: the index `sbwt build` would write for
//               the result's k-mers
//   sbwt read-hits -i <index> -q <query> -o <out> [-z] [--both-strands] [--positions <index.pos> | --occurrences <index.occ> [--max-occ N]]
//               [--refs <refs.txt> [--band N] [--cigar] [--pileup-out <pile.tsv>] [--calls-out <calls.tsv>] [--min-votes N] [--unique]
//               [--max-edit N] [--min-depth N] [--min-alt N] [--min-frac F]]
//               one line per read: n_kmers n_found covered_bases longest_run; with --positions six more columns, the read's
//               placement on the references by diagonal voting: seq strand start votes votes2 n_anchored; with --occurrences
//               the same six columns from the vote over every occurrence of every k-mer (--max-occ, default 1024: a k-mer
//               with more occurrences casts no vote); with --refs (the list build-colors -r took, its files read in order and
//               their sequences numbered as the position file numbers them) beside a placement option three more columns,
//               the placement checked against the reference's bases: mismatches edit ref_end (--band, default 8: the edit
//               distance is the best over the window of band bases either side; -1 -1 0: no placement to check); with --cigar
//               two more, the best alignment in that window: ref_begin cigar (runs of = X I D; 0 *: no alignment); with
//               --pileup-out and --calls-out the alignments of all reads are piled up on the references (--min-votes, --unique,
//               --max-edit say which reads count) and written per base with depth > 0, seq pos ref depth A C G T del ins other,
//               and per call (--min-depth, --min-alt, --min-frac), seq pos ref alt depth count; the hits file does not change
//   sbwt build-colors -i <index> -r <refs.txt> -o <colours> [--both-strands] [--wide | --compress [--stream]]
//               [--positions-out <index.pos>] [--occurrences-out <index.occ>]
//               one colour per listed reference file, set on the columns of the index's k-mers that the file holds
//               (--wide: up to 4096 files, a colour file of several words per column; --compress: up to 4096 files, a
//               colour-set file of one id per column and the distinct colour sets; --compress --stream: the same file, built
//               one reference at a time without the wide matrix on the device); --positions-out: also the position file,
//               per column the smallest (sequence, offset) at which its k-mer occurs, the sequences numbered in reading order;
//               --occurrences-out: also the occurrence file, per column every (sequence, offset, strand) of its k-mer
//   sbwt compress-colors -i <index> -c <colours> -o <colour sets>
//               the colour-set file of a colour file written with or without --wide
//   sbwt merge-colors -u <index U> -a <index A> --colors-a <colours of A> [-b <index B> --colors-b <colours of B>]
//               [--color-offset <n>] -o <colour sets of U>
//               the colour sets of A (and B, its colours moved up by the offset) carried onto U's k-mers: run set-op first,
//               then merge-colors on its output
//   sbwt color-matrix -i <index> -c <colours> -o <shared.tsv> [--jaccard-ppm]
//               the k-mers each pair of references shares, C lines of C tab-separated integers; --jaccard-ppm: the Jaccard
//               index of each pair in parts per million instead
//   sbwt color-select -i <index> -c <colours> [--include 0,3-5|all] [--exclude <list>] [--min <n>] [--max <n>]
//               -o <sub-index> [--colors-out <colour sets of the sub-index>] [--counts-only]
//               the k-mers whose colour set has none of the excluded colours and between min and max of the included ones,
//               as an index: core (--include g --min |g|), unique (--include g --exclude the others), accessory
//               (--max C-1), soft core (--include g --min p)
//   sbwt screen -i <index> -c <colours> -q <reads> -o <screen.tsv> [--both-strands] [--sets-out <sets.tsv>]
//               a read set screened against the references: per colour its index k-mers, those the reads contain, and the
//               hits on them; the accumulator stays on the GPU across batches
//   sbwt pseudoalign -i <index> -c <colours> -q <query> -o <out> [-z] [--threshold 0.7] [--all-kmers] [--both-strands]
//               one line per read: its number, then the colours that hold it
// Extra, GPU-only flags of `search` (defaults keep the reference behaviour and output):
//   --gpu <id>            HIP device to use (default 0)
//   --gpus <n>            shard every batch over HIP devices 0..n-1 (index replicated by one RCCL broadcast)
//   --gpu-list a,b,...    the same with an explicit device list (a device may be listed twice)
//   --batch-bases <n>     bases sent to the GPU per batch (default 64 Mi); the next batch is parsed and the
//                         previous one written by their own threads meanwhile
//   --host-format         print_vector on the CPU (default: formatted on the GPU, pipelined over PCIe)
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <functional>
#include <vector>

#include "SBWT.hh"
#include "../../../include/sbwthost.h"

using namespace sbwt;
using std::string;
using std::vector;

namespace {

// what cxxopts throws for bad command lines is a std::exception that is not a runtime_error, so
// main() prints it with the "Error: " prefix (sbwt.cpp:53-56)
struct option_error : public std::exception {
    string msg;
    explicit option_error(string m) : msg(std::move(m)) {}
    const char *what() const noexcept override { return msg.c_str(); }
};

struct OptSpec { string longname; char shortname; bool takes_value; string help; string def; };

class Options {
public:
    explicit Options(vector<OptSpec> specs) : specs_(std::move(specs)) {}
    void parse(int argc, char **argv) {
        for (int i = 1; i < argc; i++) {
            string a = argv[i];
            const OptSpec *s = nullptr;
            string val;
            bool has_val = false;
            if (a.rfind("--", 0) == 0) {
                string name = a.substr(2);
                size_t eq = name.find('=');
                if (eq != string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
                for (auto &x : specs_) if (x.longname == name) s = &x;
                if (!s) throw option_error("Option ‘" + name + "’ does not exist");
            } else if (a.size() == 2 && a[0] == '-') {
                for (auto &x : specs_) if (x.shortname == a[1]) s = &x;
                if (!s) throw option_error(string("Option ‘") + a[1] + "’ does not exist");
            } else {
                continue;   // positional arguments are ignored like in the reference
            }
            if (s->takes_value) {
                if (!has_val) {
                    if (i + 1 >= argc) throw option_error("Option ‘" + s->longname + "’ is missing an argument");
                    val = argv[++i];
                }
                values_[s->longname] = val;
            } else {
                values_[s->longname] = "true";
            }
        }
    }
    bool count(const string &name) const { return values_.count(name) > 0; }
    string get(const string &name) const {
        auto it = values_.find(name);
        if (it != values_.end()) return it->second;
        for (auto &x : specs_)
            if (x.longname == name && !x.def.empty()) return x.def;
        throw option_error("Option ‘" + name + "’ has no value");
    }
    string help(const string &prog, const string &desc) const {
        string h = desc + "\nUsage:\n  " + prog + " [OPTION...]\n\n";
        for (auto &x : specs_) {
            string l = "  ";
            if (x.shortname) { l += "-"; l += x.shortname; l += ", "; } else l += "    ";
            l += "--" + x.longname + (x.takes_value ? " arg" : "");
            while (l.size() < 28) l += " ";
            h += l + " " + x.help + (x.def.empty() ? "" : " (default: " + x.def + ")") + "\n";
        }
        return h;
    }

private:
    vector<OptSpec> specs_;
    std::map<string, string> values_;
};

// ---- what the subcommands share ----
// Parses the command line (first, so that a bad option is reported before any usage text); without arguments or with --help
// prints the usage text and leaves with status 1.
void parse_or_usage(Options &opts, int argc, char **argv, const string &description) {
    opts.parse(argc, argv);
    if (argc == 1 || opts.count("help")) {
        std::cerr << opts.help(argv[0], description) << std::endl;
        exit(1);
    }
}
// --gpu and --batch-bases (at least 1); the defaults are the strings in each command's spec
void use_gpu_option(const Options &opts) { set_default_device(atoi(opts.get("gpu").c_str())); }
int64_t batch_bases_option(const Options &opts) { return std::max<int64_t>(1, atoll(opts.get("batch-bases").c_str())); }

// `refusal` names the path in the sentence that refuses another variant ("GPU path", "GPU search path")
void load_plain_matrix(const string &indexfile, plain_matrix_sbwt_t &index, const char *refusal = "GPU path") {
    std::ifstream in(indexfile, std::ios::binary);
    if (!in.good()) throw std::runtime_error("Error opening file: " + indexfile);
    const string variant = load_string(in);
    if (variant != "plain-matrix")
        throw std::runtime_error(string("Error: only the plain-matrix variant is supported by the ") + refusal + " (got " + variant + ")");
    index.load(in);
}

// --precalc-length of the commands that write an index, at most k (sbwt_build.cpp:101-105)
int64_t precalc_option(const Options &opts, int64_t k) {
    const int64_t precalc = atoll(opts.get("precalc-length").c_str());
    if (precalc <= k) return precalc;
    write_log("Warning: precalc length " + std::to_string(precalc) + " is longer than k = " + std::to_string(k), LogLevel::MAJOR);
    write_log("Setting precalc length to " + std::to_string(k), LogLevel::MAJOR);
    return k;
}
// the index file of `sbwt build`: the variant's name (sbwt_build.cpp:142), then the index with the intervals of all strings
// of `precalc` characters (sbwt_build.cpp:157); the bytes the index took come back
int64_t write_index_file(plain_matrix_sbwt_t &index, const string &file, int64_t precalc) {
    std::ofstream out(file, std::ios::binary);
    if (!out.good()) throw std::runtime_error("Error opening file: " + file);
    serialize_string("plain-matrix", out);
    index.do_kmer_prefix_precalc(precalc);
    return index.serialize(out);
}

// --query-file and --out-file of search, matching-statistics and read-hits: one file each, or with a query file named *.txt
// two lists of files, one per line.  Every input is checked for reading, then every output for writing (which creates it);
// --out-file is looked at after the inputs (sbwt_search.cpp:170-190).
struct QueryFiles { vector<string> in, out; };
QueryFiles query_and_output_files(const Options &opts) {
    const string queryfile = opts.get("query-file");
    const bool multi_file = queryfile.size() >= 4 && queryfile.substr(queryfile.size() - 4) == ".txt";
    QueryFiles f;
    f.in = multi_file ? readlines(queryfile) : vector<string>{queryfile};
    for (const string &file : f.in) check_readable(file);
    const string outfile = opts.get("out-file");
    f.out = multi_file ? readlines(outfile) : vector<string>{outfile};
    for (const string &file : f.out) check_writable(file);
    return f;
}
void check_same_count(const QueryFiles &f) {   // run_queries, sbwt_search.cpp:111-115
    if (f.in.size() != f.out.size())
        throw std::runtime_error("Number of input and output files does not match (" + std::to_string(f.in.size()) + " vs " +
                                 std::to_string(f.out.size()) + ")");
}

// Reads `reader` to its end in batches of about batch_bases bases: fn(bases, read_off, n_reads) for every batch that holds a
// read.  The caller opens the reader, since where it is opened relative to the log line and to the output file shows.
template <typename Fn>
void for_each_batch(seq_io::Reader &reader, int64_t batch_bases, Fn &&fn) {
    vector<char> bases;
    vector<int64_t> read_off;
    for (bool more = true; more;) {
        bases.clear();
        read_off.assign(1, 0);
        more = reader.read_batch(bases, read_off, batch_bases);
        const int64_t n_reads = (int64_t)read_off.size() - 1;
        if (n_reads > 0) fn(bases, read_off, n_reads);
    }
}

void write_text_file(const string &path, const string &text, bool gzip) {
    if (sbwthost_write_file(path.c_str(), text.data(), (int64_t)text.size(), gzip ? 1 : 0, 0) != 0)
        throw std::runtime_error(string("Error writing ") + path + ": " + sbwthost_last_error());
}

void append_int(int64_t x, string &out) {
    char buf[24];
    int i = 0;
    uint64_t u = (uint64_t)x;
    if (x < 0) { out.push_back('-'); u = 0 - u; }        // (a read's start on a reference may be negative, its seq -1)
    if (u == 0) buf[i++] = '0';
    while (u > 0) { buf[i++] = (char)('0' + u % 10); u /= 10; }
    while (i > 0) out.push_back(buf[--i]);
}
// the set bits of a `words`-word row as ascending colour numbers: `first` before the first one, `sep` before every other
void append_set_bits(const uint64_t *row, int64_t words, const char *first, const char *sep, string &out) {
    const char *lead = first;
    for (int64_t w = 0; w < words; w++)
        for (uint64_t bits = row[w]; bits; bits &= bits - 1) {
            out.append(lead);
            append_int(w * 64 + __builtin_ctzll(bits), out);
            lead = sep;
        }
}

// print_vector, sbwt_search.cpp:21-43: each value followed by one space, '\n' per read; -1 special
// cased; 0 prints as an empty token (kept: that is what the reference emits)
inline void print_vector(const int64_t *v, int64_t n, string &out) {
    char buffer[32];
    for (int64_t t = 0; t < n; t++) {
        int64_t x = v[t];
        int i = 0;
        if (x == -1) { buffer[0] = '1'; buffer[1] = '-'; i = 2; }
        else while (x > 0) { buffer[i++] = (char)('0' + (x % 10)); x /= 10; }
        while (i > 0) out.push_back(buffer[--i]);
        out.push_back(' ');
    }
    out.push_back('\n');
}

struct QueryStats { int64_t queries = 0; int64_t micros = 0; };

// A bounded hand-off between two threads (reader -> search -> writer).
template <typename T>
class Channel {
public:
    explicit Channel(size_t cap) : cap_(cap) {}
    void push(T &&v) {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return q_.size() < cap_; });
        q_.push_back(std::move(v));
        cv_.notify_all();
    }
    bool pop(T &out) {   // false when closed and drained
        std::unique_lock<std::mutex> lk(m_);
        waiting_ = true;
        cv_.notify_all();
        cv_.wait(lk, [&] { return !q_.empty() || closed_; });
        waiting_ = false;
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cv_.notify_all();
        return true;
    }
    void close() {
        std::lock_guard<std::mutex> lk(m_);
        closed_ = true;
        cv_.notify_all();
    }
    // blocks until every item pushed so far has been popped AND its consumer has come back for the next one
    void drain() {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return q_.empty() && waiting_; });
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false, waiting_ = false;
};

struct ReadBatch {
    vector<char> bases;
    vector<int64_t> read_off{0}, out_off{0};
};
struct TextBatch {
    std::vector<plain_matrix_sbwt_t::TextPiece> pieces;   // GPU-formatted output
    string host_text;                                      // --host-format output
};

// run_file + run_queries_streaming / run_queries_not_streaming (sbwt_search.cpp:46-105), batched and
// pipelined: a reader thread parses the next batch and a writer thread writes the previous one while
// the GPU searches the current one.  The output is written strictly in input order.
// (get_index: the index, waited for at the first use -- while it loads, the reader thread already parses the input)
static int64_t g_t0 = 0;             // process time at the start of search_main (stage marks under SBWT_CLI_TIMING)
static void timing_mark(const char *what) {
    if (getenv("SBWT_CLI_TIMING")) std::cerr << "timing: t+" << (cur_time_micros() - g_t0) / 1e6 << " s " << what << std::endl;
}

QueryStats run_file(const string &infile, const string &outfile, const std::function<const plain_matrix_sbwt_t &()> &get_index,
                    bool gzip_output, int64_t batch_bases, bool host_format) {
    // SBWT_CLI_PARSER_THREADS=n (off by default): a plain regular file is parsed by n threads, piece by piece (seqio.hh
    // read_file_chunked: the parser is the same, the pieces are cut at record starts and handed on in file order).  Measured on
    // 10 M reads: the run is bound by the one thread at a time that writes the text (0.74-0.94 s of a 0.9-1.2 s loop), so
    // 1 / 2 / 3 parser threads give 1.40-1.46 / 1.36-1.44 / 1.50 s against 1.42-1.55 s with the one reader: nothing that would
    // pay for cutting FASTQ files by a heuristic.  (SBWT_CLI_CHUNK_MIN_BYTES: the smallest file read that way, default 32 MiB.)
    int64_t in_size = 0;
    const char *cm = getenv("SBWT_CLI_CHUNK_MIN_BYTES"), *pt = getenv("SBWT_CLI_PARSER_THREADS");
    const int parser_threads = pt ? atoi(pt) : 0;
    const bool chunked = parser_threads > 0 && seq_io::chunkable_file(infile, &in_size) &&
                         in_size >= (cm ? atoll(cm) : ((int64_t)32 << 20));
    std::unique_ptr<seq_io::Reader> reader_p;
    if (!chunked) reader_p.reset(new seq_io::Reader(infile));
    seq_io::Buffered_ofstream writer(outfile, gzip_output);
    QueryStats st;
    Channel<ReadBatch> to_search(2);
    Channel<TextBatch> to_write(2);
    std::exception_ptr reader_err, writer_err;

    const bool timing = getenv("SBWT_CLI_TIMING") != nullptr;       // stage times on stderr (tools/e2e_bench.py)
    int64_t t_parse = 0, t_write = 0;
    std::thread reader_thread([&] {
        try {
            if (chunked) {
                // a piece of the file holds about batch_bases bases: 2.1 bytes of a FASTQ file per base, 1.03 of a FASTA file
                const bool fq = seq_io::figure_out_file_format(infile).format == seq_io::FASTQ;
                const int64_t piece = (int64_t)((double)batch_bases * (fq ? 2.1 : 1.03)) + 4096;
                const int64_t p0 = cur_time_micros();
                int64_t t_push = 0;
                seq_io::read_file_chunked(infile, in_size, piece, parser_threads,
                                          [&](std::vector<char> &&b, std::vector<int64_t> &&off, bool) {
                                              if (off.size() <= 1) return;
                                              ReadBatch rb;
                                              rb.bases = std::move(b);
                                              rb.read_off = std::move(off);
                                              const int64_t q0 = cur_time_micros();
                                              to_search.push(std::move(rb));
                                              t_push += cur_time_micros() - q0;
                                          });
                t_parse += cur_time_micros() - p0 - t_push;      // (wall time of the parsers, waiting for the search excluded)
            }
            bool more = !chunked;
            while (more) {
                ReadBatch rb;
                rb.bases.reserve((size_t)batch_bases + 4096);
                const int64_t p0 = cur_time_micros();
                more = reader_p->read_batch(rb.bases, rb.read_off, batch_bases);
                t_parse += cur_time_micros() - p0;
                if (rb.read_off.size() > 1) to_search.push(std::move(rb));
            }
        } catch (...) {
            reader_err = std::current_exception();
        }
        to_search.close();
    });
    std::thread writer_thread([&] {
        try {
            TextBatch tb;
            while (to_write.pop(tb)) {
                for (const auto &pc : tb.pieces)
                    for (int64_t pos = 0; pos < pc.size; pos += (int64_t)1 << 30)
                        writer.write(pc.data + pos, std::min<int64_t>((int64_t)1 << 30, pc.size - pos));
                writer.write(tb.host_text.data(), (int64_t)tb.host_text.size());
                tb = TextBatch();
            }
        } catch (...) {
            writer_err = std::current_exception();
            TextBatch drop;
            while (to_write.pop(drop)) {}
        }
    });

    std::exception_ptr search_err;
    try {
        const plain_matrix_sbwt_t &index = get_index();
        timing_mark("index ready");
        const bool streaming = index.has_streaming_query_support();
        write_log(string("Running ") + (streaming ? "streaming" : "non-streaming") + " queries from input file " + infile +
                      " to output file " + outfile,
                  LogLevel::MAJOR);
        const int64_t k = index.get_k();
        if (!host_format && index.number_of_devices_in_use() <= 1 && !gzip_output) {
            // The default: search + print_vector on the GPU, pipelined over PCIe; the text goes from the pinned
            // staging buffers straight into the output file (one copy, into the page cache).  TWO threads take the batches
            // in turn: while one copies its batch's text into the file -- the longest stage, one thread's write(2) at the
            // page cache's rate -- the other's batch is already on the GPU and its first pieces of text are waiting; its
            // sink blocks until the batch before it is written.  The output is in input order, piece by piece.
            std::mutex pop_m, turn_m;
            std::condition_variable turn_cv;
            int64_t next_seq = 0, turn = 0;
            bool failed = false;
            std::exception_ptr worker_err[2];
            auto worker = [&](int w) {
                try {
                    for (;;) {
                        ReadBatch rb;
                        int64_t seq;
                        {
                            std::lock_guard<std::mutex> lk(pop_m);
                            if (!to_search.pop(rb)) break;
                            seq = next_seq++;
                        }
                        const int64_t n_reads = (int64_t)rb.read_off.size() - 1;
                        bool mine = false;
                        int64_t t_sink = 0, t_wait = 0, nq = 0;
                        auto take_turn = [&] {
                            if (mine) return;
                            const int64_t w0 = cur_time_micros();
                            std::unique_lock<std::mutex> lk(turn_m);
                            turn_cv.wait(lk, [&] { return turn == seq || failed; });
                            if (failed && turn != seq) throw std::runtime_error("search stopped: another batch failed");
                            mine = true;
                            t_wait += cur_time_micros() - w0;
                        };
                        const int64_t t0 = cur_time_micros();
                        try {
                            nq = index.search_text_stream(rb.bases.data(), rb.read_off.data(), n_reads,
                                                          [&](const char *text, int64_t bytes) {
                                                              take_turn();
                                                              const int64_t w0 = cur_time_micros();
                                                              writer.write(text, bytes);
                                                              t_sink += cur_time_micros() - w0;
                                                          });
                            take_turn();                       // (a batch without any text still waits for its turn)
                        } catch (...) {
                            std::lock_guard<std::mutex> lk(turn_m);
                            failed = true;
                            turn_cv.notify_all();
                            throw;
                        }
                        {
                            std::lock_guard<std::mutex> lk(turn_m);
                            st.queries += nq;
                            st.micros += cur_time_micros() - t0 - t_sink - t_wait;
                            t_write += t_sink;
                            turn = seq + 1;
                        }
                        turn_cv.notify_all();
                        timing_mark("a batch searched and written");
                    }
                } catch (...) {
                    worker_err[w] = std::current_exception();
                }
            };
            // SBWT_CLI_SEARCH_THREADS=1: one worker (three staging slots instead of six: pinned and device memory are tight)
            const char *st_env = getenv("SBWT_CLI_SEARCH_THREADS");
            const bool one_worker = st_env && atoi(st_env) == 1;
            std::thread second;
            if (!one_worker) second = std::thread([&] { worker(1); });
            worker(0);
            if (second.joinable()) second.join();
            for (auto &e : worker_err)
                if (e) std::rethrow_exception(e);
        }
        ReadBatch rb;
        vector<int64_t> out;
        while (to_search.pop(rb)) {
            const int64_t n_reads = (int64_t)rb.read_off.size() - 1;
            rb.out_off.resize(rb.read_off.size());
            for (size_t r = 1; r < rb.read_off.size(); r++)
                rb.out_off[r] = rb.out_off[r - 1] + std::max<int64_t>(0, rb.read_off[r] - rb.read_off[r - 1] - k + 1);
            TextBatch tb;
            if (host_format) {
                // reference-style: raw ranks back to the host, print_vector on the CPU
                out.resize((size_t)rb.out_off.back());
                int64_t t0 = cur_time_micros();
                if (streaming) index.streaming_search_batch(rb.bases.data(), rb.read_off.data(), n_reads, out.data(), rb.out_off.data());
                else index.search_batch(rb.bases.data(), rb.read_off.data(), n_reads, out.data(), rb.out_off.data());
                st.micros += cur_time_micros() - t0;
                st.queries += rb.out_off.back();
                for (int64_t r = 0; r < n_reads; r++)
                    print_vector(out.data() + rb.out_off[(size_t)r], rb.out_off[(size_t)r + 1] - rb.out_off[(size_t)r], tb.host_text);
            } else {
                // several devices (every device's text is a piece of its own), or compressed output (a writer thread)
                int64_t t0 = cur_time_micros();
                st.queries += index.search_text_batch(rb.bases.data(), rb.read_off.data(), n_reads, tb.pieces);
                st.micros += cur_time_micros() - t0;
            }
            to_write.push(std::move(tb));
        }
    } catch (...) {
        search_err = std::current_exception();
        ReadBatch drop;
        while (to_search.pop(drop)) {}
    }
    timing_mark("search loop left");
    to_write.close();
    reader_thread.join();
    timing_mark("reader joined");
    writer_thread.join();
    timing_mark("writer joined");
    if (search_err) std::rethrow_exception(search_err);
    if (reader_err) std::rethrow_exception(reader_err);
    if (writer_err) std::rethrow_exception(writer_err);
    write_log("us/query: " + std::to_string((double)st.micros / (double)st.queries) + " (excluding I/O etc)",
              LogLevel::MAJOR);
    writer.close();
    timing_mark("output closed");
    if (timing)
        std::cerr << "timing: parse " << t_parse / 1e6 << " s, search (GPU + PCIe) " << st.micros / 1e6 << " s, write "
                  << t_write / 1e6 << " s" << std::endl;
    return st;
}

int search_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    g_t0 = micros_start;
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output filename.", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"query-file", 'q', true,
         "The query in FASTA or FASTQ format, possibly gzipped. Multi-line FASTQ is not supported. If the file "
         "extension is .txt, this is interpreted as a list of query files, one per line. In this case, --out-file is "
         "also interpreted as a list of output files in the same manner, one line for each input file.", ""},
        {"gzip-output", 'z', false,
         "Writes output in gzipped form. This can shrink the output files by an order of magnitude.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"gpus", 0, true, "Shard every batch over HIP devices 0..n-1.", "1"},
        {"gpu-list", 0, true, "Explicit comma separated device list to shard over.", "-"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "67108864"},
        {"host-format", 0, false, "Format the output on the CPU (print_vector) instead of on the GPU.", ""},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Query all k-mers of all input reads.");
    string indexfile = opts.get("index-file");
    check_readable(indexfile);
    const QueryFiles files = query_and_output_files(opts);
    bool gzip_output = opts.count("gzip-output");

    vector<int> devices;
    if (opts.get("gpu-list") != "-") {
        string l = opts.get("gpu-list");
        for (size_t pos = 0; pos <= l.size();) {
            size_t e = l.find(',', pos);
            if (e == string::npos) e = l.size();
            devices.push_back(atoi(l.substr(pos, e - pos).c_str()));
            pos = e + 1;
        }
    } else {
        int n = atoi(opts.get("gpus").c_str());
        if (n > 1) for (int g = 0; g < n; g++) devices.push_back(g);
        else devices.push_back(atoi(opts.get("gpu").c_str()));
    }
    set_default_device(devices[0]);
    const int64_t batch_bases = batch_bases_option(opts);

    std::ifstream in(indexfile, std::ios::binary);
    if (!in.good()) throw std::runtime_error("Error opening file: " + indexfile);
    string variant = load_string(in);
    static const char *variants[] = {"plain-matrix", "rrr-matrix", "mef-matrix", "plain-split", "rrr-split",
                                     "mef-split", "plain-concat", "mef-concat", "plain-subsetwt", "rrr-subsetwt"};
    if (std::find(std::begin(variants), std::end(variants), variant) == std::end(variants)) {
        std::cerr << "Error loading index from file: unrecognized variant specified in the file" << std::endl;
        return 1;
    }
    write_log("Loading the index variant " + variant, LogLevel::MAJOR);
    if (variant != "plain-matrix")
        throw std::runtime_error("Error: only the plain-matrix variant is supported by the GPU search path (got " +
                                 variant + ")");
    check_same_count(files);
    // The index loads (file, HIP start-up, device image: a few tenths of a second) on a thread of its own while the first
    // input file is already being parsed; the search waits for it.
    plain_matrix_sbwt_t index;
    std::exception_ptr load_err;
    std::thread loader([&] {
        try {
            const int64_t load0 = cur_time_micros();
            timing_mark("loader thread started");
            index.load(in);
            if (getenv("SBWT_CLI_TIMING"))
                std::cerr << "timing: index load + device image " << (cur_time_micros() - load0) / 1e6 << " s" << std::endl;
            if (devices.size() > 1) {
                index.use_devices(devices);
                write_log("Index replicated onto " + std::to_string(devices.size()) + " GPU contexts", LogLevel::MAJOR);
            }
        } catch (...) {
            load_err = std::current_exception();
        }
    });
    bool joined = false;
    std::mutex join_mutex;
    const std::function<const plain_matrix_sbwt_t &()> get_index = [&]() -> const plain_matrix_sbwt_t & {
        std::lock_guard<std::mutex> lk(join_mutex);
        if (!joined) { loader.join(); joined = true; }
        if (load_err) std::rethrow_exception(load_err);
        return index;
    };
    int64_t number_of_queries = 0;
    try {
        for (size_t i = 0; i < files.in.size(); i++)
            number_of_queries += run_file(files.in[i], files.out[i], get_index, gzip_output, batch_bases,
                                          opts.count("host-format")).queries;
    } catch (...) {
        if (!joined) { loader.join(); joined = true; }
        throw;
    }
    if (!joined) { loader.join(); joined = true; }

    timing_mark("all files done");
    int64_t total_micros = cur_time_micros() - micros_start;
    write_log("us/query end-to-end: " + std::to_string((double)total_micros / (double)number_of_queries), LogLevel::MAJOR);
    return 0;
}

int build_main(int argc, char **argv) {
    set_log_level(LogLevel::MAJOR);
    Options opts({
        {"in-file", 'i', true,
         "The input sequences as a FASTA or FASTQ file, possibly gzipped. If the file extension is .txt, the file is "
         "interpreted as a list of input files, one file on each line.", ""},
        {"out-file", 'o', true, "Output file for the constructed index.", ""},
        {"kmer-length", 'k', true, "The k-mer length.", ""},
        {"precalc-length", 'p', true, "Precalculate SBWT intervals of strings of this length.", "8"},
        {"variant", 0, true, "The SBWT variant to build (only plain-matrix here).", "plain-matrix"},
        {"add-reverse-complements", 0, false, "Also add the reverse complement of every k-mer to the index.", ""},
        {"no-streaming-support", 0, false, "Do not build the streaming query support bit vector.", ""},
        {"n-threads", 't', true, "Number of parallel threads.", "1"},
        {"temp-dir", 'd', true, "Ignored (construction is in memory).", "."},
        {"gpu", 0, true, "HIP device used for the prefix table.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Construct a plain-matrix SBWT (in memory).");
    string variant = opts.get("variant");
    if (variant != "plain-matrix") {
        std::cerr << "Error: unknown variant: " << variant << std::endl;
        return 1;
    }
    string out_file = opts.get("out-file");
    check_writable(out_file);
    string in_file = opts.get("in-file");
    vector<string> input_files;
    if (in_file.size() >= 4 && in_file.substr(in_file.size() - 4) == ".txt") input_files = readlines(in_file);
    else input_files = {in_file};
    for (const string &f : input_files) check_readable(f);
    int64_t k = atoll(opts.get("kmer-length").c_str());
    const int64_t precalc = precalc_option(opts, k);
    use_gpu_option(opts);
    vector<string> seqs;
    for (const string &f : input_files) {
        seq_io::Reader reader(f);
        for (;;) {
            int64_t len = reader.get_next_read_to_buffer();
            if (len == 0) break;
            seqs.emplace_back(reader.read_buf, (size_t)len);
        }
    }
    write_log("Building SBWT subset sequence in memory", LogLevel::MAJOR);
    PlainMatrixBits bits = build_plain_matrix_bits_any(seqs, (int)k, opts.count("add-reverse-complements"),
                                                   !opts.count("no-streaming-support"), atoi(opts.get("n-threads").c_str()));
    plain_matrix_sbwt_t index(bits, 0);
    write_log("Build SBWT for " + std::to_string(index.number_of_kmers()) + " distinct k-mers", LogLevel::MAJOR);
    write_log("SBWT has " + std::to_string(index.number_of_subsets()) + " subsets", LogLevel::MAJOR);
    const int64_t bytes_written = write_index_file(index, out_file, precalc);
    write_log("Built variant " + variant + " to file " + out_file, LogLevel::MAJOR);
    write_log("Space on disk: " + std::to_string(bytes_written * 8.0 / (double)index.number_of_subsets()) +
                  " bits per column, " + std::to_string(bytes_written * 8.0 / (double)index.number_of_kmers()) +
                  " bits per k-mer",
              LogLevel::MAJOR);
    return 0;
}

// `sbwt matching-statistics`: the query handling of `search` (FASTA / FASTQ, gzipped, .txt lists of files), one line per
// read with one token per base, each followed by a space (print_vector's layout): the match length d, or "d,first,second"
// with --intervals.  Batches go to the GPU one at a time; the text is formatted on the host.
int matching_statistics_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output filename (a list of output files if the query file is a .txt list).", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"query-file", 'q', true,
         "The query in FASTA or FASTQ format, possibly gzipped. If the file extension is .txt, this is interpreted as a "
         "list of query files, one per line, and --out-file as a list of output files.", ""},
        {"gzip-output", 'z', false, "Writes output in gzipped form.", ""},
        {"intervals", 0, false, "Print d,first,second (the colex interval of the matched suffix) instead of d.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "67108864"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "k-bounded matching statistics of every base of all input reads.");
    const string indexfile = opts.get("index-file");
    check_readable(indexfile);
    const QueryFiles files = query_and_output_files(opts);
    check_same_count(files);
    const bool gzip_output = opts.count("gzip-output"), intervals = opts.count("intervals");
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);

    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index, "GPU search path");
    int64_t positions = 0;
    for (size_t f = 0; f < files.in.size(); f++) {
        write_log("Running matching statistics from input file " + files.in[f] + " to output file " + files.out[f],
                  LogLevel::MAJOR);
        seq_io::Reader reader(files.in[f]);
        seq_io::Buffered_ofstream writer(files.out[f], gzip_output);
        vector<uint8_t> len;
        vector<int64_t> first, second;
        string text;
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            const int64_t total = read_off.back();
            len.resize((size_t)total);
            if (intervals) { first.resize((size_t)total); second.resize((size_t)total); }
            index.matching_statistics_batch(bases.data(), read_off.data(), n_reads, len.data(), intervals ? first.data() : nullptr,
                                            intervals ? second.data() : nullptr);
            text.clear();
            for (int64_t r = 0; r < n_reads; r++) {
                for (int64_t b = read_off[(size_t)r]; b < read_off[(size_t)r + 1]; b++) {
                    append_int(len[(size_t)b], text);
                    if (intervals) {
                        text.push_back(',');
                        append_int(first[(size_t)b], text);
                        text.push_back(',');
                        append_int(second[(size_t)b], text);
                    }
                    text.push_back(' ');
                }
                text.push_back('\n');
            }
            writer.write(text.data(), (int64_t)text.size());
            positions += total;
        });
    }
    write_log("us/base end-to-end: " + std::to_string((double)(cur_time_micros() - micros_start) / (double)std::max<int64_t>(1, positions)),
              LogLevel::MAJOR);
    return 0;
}

// a fraction option as parts per million (defined with the colour helpers, below); allow_zero: 0 .. 1, not (0, 1]
int64_t parse_threshold_ppm(const string &s, const char *option, bool allow_zero);

// The two files of read-hits' pileup.  Both begin with a # line of the totals; pile.tsv has one line per base with depth > 0,
// seq pos ref depth A C G T del ins other, and calls.tsv one per call, seq pos ref alt depth count (alt: A C G T - +).
static void write_pileup_files(const RefSeqs &refseqs, const Pileup &pileup, const string &pilefile, const string &callsfile, int32_t min_depth,
                               int32_t min_alt, int32_t min_frac_ppm) {
    const Pileup::Info pi = pileup.info();
    string head = "#";
    const std::pair<const char *, int64_t> totals[] = {{"n_seqs", pi.n_seqs}, {"total_bases", pi.total_bases}, {"n_offered", pi.n_offered},
                                                       {"n_piled", pi.n_piled}, {"n_columns", pi.n_columns}, {"n_clipped", pi.n_clipped},
                                                       {"n_overhang", pi.n_overhang}};
    for (const auto &t : totals) {
        head.push_back(' ');
        head.append(t.first);
        head.push_back('=');
        append_int(t.second, head);
    }
    head.push_back('\n');
    if (!pilefile.empty()) {
        seq_io::Buffered_ofstream writer(pilefile, false);
        writer.write(head.data(), (int64_t)head.size());
        vector<int64_t> len((size_t)pi.n_seqs);
        if (sbwtgpu_refseqs_lengths_copy(refseqs.h, len.data()) != SBWTGPU_OK) throw std::runtime_error(string("Error: ") + sbwtgpu_last_error());
        vector<char> ref;
        string text;
        const int64_t piece = (int64_t)1 << 20;
        for (int64_t s = 0; s < pi.n_seqs; s++) {
            for (int64_t pos = 0; pos < len[(size_t)s]; pos += piece) {
                const int64_t n = std::min(piece, len[(size_t)s] - pos);
                const vector<sbwtgpu_pileup_base> rec = pileup.counts(s, pos, n);
                ref.resize((size_t)n);
                if (sbwtgpu_refseqs_get(refseqs.h, s, pos, n, ref.data()) != SBWTGPU_OK) throw std::runtime_error(string("Error: ") + sbwtgpu_last_error());
                text.clear();
                for (int64_t q = 0; q < n; q++) {
                    const sbwtgpu_pileup_base &b = rec[(size_t)q];
                    if (b.depth == 0) continue;
                    append_int(s, text);
                    text.push_back('\t');
                    append_int(pos + q, text);
                    text.push_back('\t');
                    text.push_back(ref[(size_t)q]);
                    for (int64_t v : {(int64_t)b.depth, (int64_t)b.n[0], (int64_t)b.n[1], (int64_t)b.n[2], (int64_t)b.n[3], (int64_t)b.n_del, (int64_t)b.n_ins,
                                      (int64_t)b.n_other}) {
                        text.push_back('\t');
                        append_int(v, text);
                    }
                    text.push_back('\n');
                }
                writer.write(text.data(), (int64_t)text.size());
            }
        }
    }
    if (!callsfile.empty()) {
        seq_io::Buffered_ofstream writer(callsfile, false);
        string text = head;
        for (const sbwtgpu_pileup_call &c : pileup.calls(min_depth, min_alt, min_frac_ppm)) {
            append_int(c.seq, text);
            text.push_back('\t');
            append_int(c.pos, text);
            text.push_back('\t');
            text.push_back("ACGT"[c.ref & 3]);
            text.push_back('\t');
            text.push_back("ACGT-+"[c.allele >= 0 && c.allele < 6 ? c.allele : 0]);
            text.push_back('\t');
            append_int(c.depth, text);
            text.push_back('\t');
            append_int(c.count, text);
            text.push_back('\n');
        }
        writer.write(text.data(), (int64_t)text.size());
    }
}

// sbwt read-hits: one line per read, `n_kmers n_found covered_bases longest_run` (include/sbwtgpu.h: the profile a screen of
// reads against the index needs, 16 bytes per read from the GPU instead of a value per k-mer).  Batches go to the GPU one at a
// time; the table is formatted on the host.
int read_hits_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output filename (a list of output files if the query file is a .txt list).", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"query-file", 'q', true,
         "The query in FASTA or FASTQ format, possibly gzipped. If the file extension is .txt, this is interpreted as a "
         "list of query files, one per line, and --out-file as a list of output files.", ""},
        {"gzip-output", 'z', false, "Writes output in gzipped form.", ""},
        {"both-strands", 0, false, "A k-mer also counts as found when its reverse complement is in the index.", ""},
        {"positions", 0, true, "A position file of the index (build-colors --positions-out): every line gains the read's placement on the references, seq strand start votes votes2 n_anchored (seq -1: no placement).", ""},
        {"occurrences", 0, true, "An occurrence file of the index (build-colors --occurrences-out): every line gains the same six columns, seq strand start votes votes2 n_anchored, from the vote over every occurrence of every k-mer; votes2 == votes says that an equally good placement exists. Cannot be combined with --positions.", ""},
        {"max-occ", 0, true, "With --occurrences: a k-mer with more occurrences than this casts no vote (1 .. 1048576). The default is 1024.", "1024"},
        {"refs", 0, true, "With --positions or --occurrences: the list of reference files that build-colors -r took (FASTA or FASTQ, possibly gzipped, one per line). They are read in order and their sequences numbered 0, 1, ... as the position file numbers them; every line gains three more columns behind the six of the placement, the read checked against the reference's bases there: mismatches edit ref_end (mismatches on the voted diagonal, the best edit distance in the window of --band bases either side, the end of that alignment on the reference; -1 -1 0: no placement to check, and a read of more than 1024 bases gets its mismatches only, edit -1).", ""},
        {"band", 0, true, "With --refs: the bases either side of the voted placement that the edit distance may use (0 .. 256). The default is 8.", "8"},
        {"cigar", 0, false, "With --refs: every line gains two more columns behind mismatches edit ref_end, the best alignment in that window: ref_begin cigar (where the alignment begins on the reference, and its runs with the four letters = X I D: match, substitution, a read base that faces nothing, a reference base that faces nothing; 0 *: no alignment, for a read without a placement or of more than 1024 bases). A batch then holds room for its runs on the device, 8 bytes per base of --batch-bases beside some 300 MB of scratch (2 GB more at the default batch): lower --batch-bases on a small device. Reads of more than 256 bases, and reads of more than 31 edits, are aligned by a far slower kernel.", ""},
        {"pileup-out", 0, true, "With --refs: the alignments of all reads of all query files are piled up on the references, and this file receives one line per reference base with depth > 0, tab-separated: seq pos ref depth A C G T del ins other (ref is N at a base that is not upper-case ACGT; the matches count under the reference's own base; ins counts the insertions behind the base). The first line is a # line with the totals: n_seqs total_bases n_offered n_piled n_columns n_clipped n_overhang. The hits file is what it is without the option.", ""},
        {"calls-out", 0, true, "With --refs: the same pileup's calls, tab-separated: seq pos ref alt depth count, alt one of A C G T - + (- a deleted base, + an insertion behind the base), behind the same # line. See --min-depth, --min-alt and --min-frac.", ""},
        {"min-votes", 0, true, "With --pileup-out or --calls-out: only reads whose placement has at least this many votes are piled. The default is 0.", "0"},
        {"unique", 0, false, "With --pileup-out or --calls-out: only reads whose placement has more votes than the runner-up (votes > votes2) are piled.", ""},
        {"max-edit", 0, true, "With --pileup-out or --calls-out: only reads of at most this many edits are piled (-1: no limit). The default is -1.", "-1"},
        {"min-depth", 0, true, "With --calls-out: a call needs at least this depth at its base (at least 1). The default is 1.", "1"},
        {"min-alt", 0, true, "With --calls-out: a call needs at least this many observations of its allele (at least 1). The default is 1.", "1"},
        {"min-frac", 0, true, "With --calls-out: a call needs at least this fraction of the depth, a decimal number in 0 .. 1 with at most six decimals. The default is 0.", "0"},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Per read: k-mers, k-mers found in the index, bases they cover, longest run of found k-mers; with a placement option the read's placement on the references, and with --refs that placement checked against the reference's bases.");
    const string indexfile = opts.get("index-file");
    check_readable(indexfile);
    const QueryFiles files = query_and_output_files(opts);
    check_same_count(files);
    const bool gzip_output = opts.count("gzip-output");
    const int strands = opts.count("both-strands") ? 2 : 1;
    const string posfile = opts.count("positions") ? opts.get("positions") : "";
    if (!posfile.empty()) check_readable(posfile);
    const string occfile = opts.count("occurrences") ? opts.get("occurrences") : "";
    if (!occfile.empty() && !posfile.empty()) throw std::runtime_error("Error: --positions and --occurrences cannot be combined");
    if (!occfile.empty()) check_readable(occfile);
    int64_t max_occ = 1024;
    if (opts.count("max-occ")) {
        if (occfile.empty()) throw std::runtime_error("Error: --max-occ needs --occurrences");
        const string text = opts.get("max-occ");
        char *end = nullptr;
        max_occ = strtoll(text.c_str(), &end, 10);
        if (text.empty() || *end != 0 || max_occ < 1 || max_occ > SBWTGPU_OCCURRENCES_MAX_OCC)
            throw std::runtime_error("Error: --max-occ must be a number in 1 .. 1048576, not " + text);
    }
    const string refsfile = opts.count("refs") ? opts.get("refs") : "";
    if (!refsfile.empty() && posfile.empty() && occfile.empty())
        throw std::runtime_error("Error: --refs needs --positions or --occurrences (it checks the placement they give)");
    int64_t band = 8;
    if (opts.count("band")) {
        if (refsfile.empty()) throw std::runtime_error("Error: --band needs --refs");
        const string text = opts.get("band");
        char *end = nullptr;
        band = strtoll(text.c_str(), &end, 10);
        if (text.empty() || *end != 0 || band < 0 || band > SBWTGPU_VERIFY_MAX_BAND)
            throw std::runtime_error("Error: --band must be a number in 0 .. 256, not " + text);
    }
    const bool cigar = opts.count("cigar");
    if (cigar && refsfile.empty()) throw std::runtime_error("Error: --cigar needs --refs");
    const string pilefile = opts.count("pileup-out") ? opts.get("pileup-out") : "";
    const string callsfile = opts.count("calls-out") ? opts.get("calls-out") : "";
    if (!pilefile.empty() && refsfile.empty()) throw std::runtime_error("Error: --pileup-out needs --refs");
    if (!callsfile.empty() && refsfile.empty()) throw std::runtime_error("Error: --calls-out needs --refs");
    const bool piling = !pilefile.empty() || !callsfile.empty();
    // a number option of the pileup: `needs` names what it is for
    auto pile_number = [&](const char *name, int64_t lo, int64_t hi, int64_t fallback, bool present, const char *needs) -> int64_t {
        if (!opts.count(name)) return fallback;
        if (!present) throw std::runtime_error(string("Error: --") + name + " needs " + needs);
        const string text = opts.get(name);
        char *end = nullptr;
        const int64_t v = strtoll(text.c_str(), &end, 10);
        if (text.empty() || *end != 0 || v < lo || v > hi)
            throw std::runtime_error(string("Error: --") + name + " must be a number in " + std::to_string(lo) + " .. " + std::to_string(hi) + ", not " + text);
        return v;
    };
    sbwtgpu_pileup_filter pile_filter{0, 0, -1, 0};
    pile_filter.min_votes = (int32_t)pile_number("min-votes", 0, INT32_MAX, 0, piling, "--pileup-out or --calls-out");
    pile_filter.max_edit = (int32_t)pile_number("max-edit", -1, INT32_MAX, -1, piling, "--pileup-out or --calls-out");
    if (opts.count("unique")) {
        if (!piling) throw std::runtime_error("Error: --unique needs --pileup-out or --calls-out");
        pile_filter.require_unique = 1;
    }
    const int32_t min_depth = (int32_t)pile_number("min-depth", 1, INT32_MAX, 1, !callsfile.empty(), "--calls-out");
    const int32_t min_alt = (int32_t)pile_number("min-alt", 1, INT32_MAX, 1, !callsfile.empty(), "--calls-out");
    int32_t min_frac_ppm = 0;
    if (opts.count("min-frac")) {
        if (callsfile.empty()) throw std::runtime_error("Error: --min-frac needs --calls-out");
        min_frac_ppm = (int32_t)parse_threshold_ppm(opts.get("min-frac"), "--min-frac", true);
    }
    vector<string> refs;
    if (!refsfile.empty()) {
        check_readable(refsfile);
        refs = readlines(refsfile);
        for (const string &file : refs) check_readable(file);
    }
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);

    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index, "GPU search path");
    plain_matrix_sbwt_t::Positions positions;
    if (!posfile.empty()) positions = index.load_positions(posfile);
    plain_matrix_sbwt_t::Occurrences occurrences;
    if (!occfile.empty()) occurrences = index.load_occurrences(occfile);
    const bool placing = positions.h || occurrences.h;
    vector<sbwtgpu_read_map> placed;
    // the reference sequences, numbered in reading order as build-colors numbered them
    RefSeqs refseqs;
    if (!refsfile.empty()) {
        refseqs = RefSeqs::create();
        for (const string &file : refs) {
            seq_io::Reader reader(file);
            for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
                refseqs.add(bases.data(), read_off.data(), n_reads);
            });
        }
        const size_t listed = positions.h ? positions.seqs.size() : occurrences.seqs.size();
        if ((size_t)refseqs.info().n_seqs != listed)
            throw std::runtime_error("Error: " + refsfile + " holds " + std::to_string(refseqs.info().n_seqs) + " sequences, the placement file lists " +
                                     std::to_string(listed));
    }
    Pileup pileup;
    if (piling) pileup = Pileup::create(refseqs);
    vector<sbwtgpu_read_verify> verified;
    vector<sbwtgpu_read_align> aligned;
    vector<int64_t> op_off;
    vector<uint32_t> ops;
    int64_t total_reads = 0;
    for (size_t f = 0; f < files.in.size(); f++) {
        write_log("Running read-hits from input file " + files.in[f] + " to output file " + files.out[f], LogLevel::MAJOR);
        seq_io::Reader reader(files.in[f]);
        seq_io::Buffered_ofstream writer(files.out[f], gzip_output);
        vector<sbwtgpu_read_hits> rec;
        string text;
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            rec.resize((size_t)n_reads);
            index.read_hits_batch(bases.data(), read_off.data(), n_reads, strands, rec.data());
            if (placing) placed.resize((size_t)n_reads);
            if (positions.h) positions.map(bases.data(), read_off.data(), n_reads, strands, placed.data());
            if (occurrences.h) occurrences.map(bases.data(), read_off.data(), n_reads, strands, (int)max_occ, placed.data());
            if (refseqs.h) {
                verified.resize((size_t)n_reads);
                if (cigar) {
                    aligned.resize((size_t)n_reads);
                    refseqs.align(bases.data(), read_off.data(), n_reads, placed.data(), (int)band, verified.data(), aligned.data(), op_off, ops);
                } else {
                    refseqs.verify(bases.data(), read_off.data(), n_reads, placed.data(), (int)band, verified.data());
                }
                if (piling) pileup.add(bases.data(), read_off.data(), n_reads, placed.data(), (int)band, pile_filter);
            }
            text.clear();
            for (size_t r = 0; r < rec.size(); r++) {
                const sbwtgpu_read_hits &h = rec[r];
                append_int(h.n_kmers, text);
                text.push_back(' ');
                append_int(h.n_found, text);
                text.push_back(' ');
                append_int(h.covered_bases, text);
                text.push_back(' ');
                append_int(h.longest_run, text);
                if (placing) {
                    const sbwtgpu_read_map &m = placed[r];
                    for (int64_t v : {(int64_t)m.seq, (int64_t)m.strand, (int64_t)m.start, (int64_t)m.votes, (int64_t)m.votes2, (int64_t)m.n_anchored}) {
                        text.push_back(' ');
                        append_int(v, text);
                    }
                }
                if (refseqs.h) {
                    const sbwtgpu_read_verify &v = verified[r];
                    for (int64_t x : {(int64_t)v.mismatches, (int64_t)v.edit, (int64_t)v.ref_end}) {
                        text.push_back(' ');
                        append_int(x, text);
                    }
                }
                if (cigar) {
                    text.push_back(' ');
                    append_int(aligned[r].ref_begin, text);
                    text.push_back(' ');
                    if (op_off[r + 1] == op_off[r]) text.push_back('*');
                    for (int64_t o = op_off[r]; o < op_off[r + 1]; o++) {
                        append_int((int64_t)(ops[(size_t)o] >> 4), text);
                        text.push_back("?ID????=X???????"[ops[(size_t)o] & 15u]);
                    }
                }
                text.push_back('\n');
            }
            writer.write(text.data(), (int64_t)text.size());
            total_reads += n_reads;
        });
    }
    if (piling) write_pileup_files(refseqs, pileup, pilefile, callsfile, min_depth, min_alt, min_frac_ppm);
    write_log("us/read end-to-end: " + std::to_string((double)(cur_time_micros() - micros_start) / (double)std::max<int64_t>(1, total_reads)),
              LogLevel::MAJOR);
    return 0;
}

// sbwt dump-unitigs: the index turned back into sequence -- FASTA, one record per unitig in the order of the API (ascending
// first column), the header the unitig's number.  With --colors the unitigs are cut where the colour set changes and the
// header is "number set-id" (dump_unitigs_colored, below the colour helpers); --sets-out writes the table of the sets.
// With --gfa the output file is GFA 1 instead: the unitigs as segments, then the links between them.
int dump_unitigs_colored(const plain_matrix_sbwt_t &index, const string &indexfile, const string &colorsfile, const string &outfile,
                         const string &setsfile, bool gzip, bool gfa);
// GFA 1: "H VN:Z:1.0", one "S number bases [cs:i:set-id] [KC:i:k-mer hits]" per unitig, then one "L i + j + (k-1)M" per link in
// link order
static string gfa_text(const vector<char> &bases, const vector<int64_t> &off, const vector<int64_t> &link_off,
                       const vector<uint32_t> &link_to, const vector<uint32_t> *set_id, int64_t k, const vector<int64_t> *kc = nullptr) {
    const int64_t n = (int64_t)off.size() - 1;
    string text;
    text.reserve(bases.size() + (size_t)n * 24 + link_to.size() * 32 + 16);
    text.append("H\tVN:Z:1.0\n");
    for (int64_t i = 0; i < n; i++) {
        text.append("S\t");
        append_int(i, text);
        text.push_back('\t');
        text.append(bases.data() + off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]));
        if (set_id) {
            text.append("\tcs:i:");
            append_int((int64_t)(*set_id)[(size_t)i], text);
        }
        if (kc) {
            text.append("\tKC:i:");
            append_int((*kc)[(size_t)i], text);
        }
        text.push_back('\n');
    }
    string overlap;
    append_int(k - 1, overlap);
    overlap.append("M\n");
    for (int64_t i = 0; i < n; i++)
        for (int64_t e = link_off[(size_t)i]; e < link_off[(size_t)i + 1]; e++) {
            text.append("L\t");
            append_int(i, text);
            text.append("\t+\t");
            append_int((int64_t)link_to[(size_t)e], text);
            text.append("\t+\t");
            text.append(overlap);
        }
    return text;
}
int dump_unitigs_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output FASTA filename.", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"gzip-output", 'z', false, "Writes output in gzipped form.", ""},
        {"colors", 0, true, "Colour file or colour-set file of the index: cut the unitigs where the colour set changes; headers become `>number set-id`.", ""},
        {"sets-out", 0, true, "With --colors: write one line per set id -- the id, then its colours, ascending.", ""},
        {"gfa", 0, false, "Write the output file as GFA 1: segments and the links between them (with --colors a cs:i: tag per segment).", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Write the unitigs of the de Bruijn graph of the indexed k-mers as FASTA.");
    const string indexfile = opts.get("index-file"), outfile = opts.get("out-file");
    const bool colored = opts.count("colors");
    if (opts.count("sets-out") && !colored) throw std::runtime_error("Error: --sets-out needs --colors");
    const string colorsfile = colored ? opts.get("colors") : string(), setsfile = opts.count("sets-out") ? opts.get("sets-out") : string();
    check_readable(indexfile);
    if (colored) check_readable(colorsfile);
    check_writable(outfile);
    if (!setsfile.empty()) check_writable(setsfile);
    use_gpu_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    const bool gfa = opts.count("gfa");
    if (colored) return dump_unitigs_colored(index, indexfile, colorsfile, outfile, setsfile, opts.count("gzip-output"), gfa);
    const plain_matrix_sbwt_t::Unitigs u = index.unitigs(gfa);
    const int64_t n = (int64_t)u.first_col.size();
    string text;
    if (gfa) {
        text = gfa_text(u.bases, u.off, u.link_off, u.link_to, nullptr, index.get_k());
    } else {
        text.reserve(u.bases.size() + (size_t)n * 12);
        for (int64_t i = 0; i < n; i++) {
            text.push_back('>');
            append_int(i, text);
            text.push_back('\n');
            text.append(u.bases.data() + u.off[(size_t)i], (size_t)(u.off[(size_t)i + 1] - u.off[(size_t)i]));
            text.push_back('\n');
        }
    }
    write_text_file(outfile, text, opts.count("gzip-output"));
    write_log("Wrote " + std::to_string(n) + " unitigs, " + std::to_string(u.bases.size()) + " bases" +
                  (gfa ? ", " + std::to_string(u.link_to.size()) + " links" : string()),
              LogLevel::MAJOR);
    return 0;
}

// sbwt set-op: two index files combined on the GPU without their input sequences -- the result is the index `sbwt build`
// would write for the result's k-mers (same serialisation and precalc step as build_main)
int set_op_main(int argc, char **argv) {
    set_log_level(LogLevel::MAJOR);
    Options opts({
        {"index-a", 'a', true, "First index input file.", ""},
        {"index-b", 'b', true, "Second index input file.", ""},
        {"op", 0, true, "union, intersection, difference (a minus b) or symmetric-difference.", "union"},
        {"out-file", 'o', true, "Output file for the resulting index.", ""},
        {"no-streaming-support", 0, false, "Do not build the streaming query support bit vector.", ""},
        {"precalc-length", 'p', true, "Precalculate SBWT intervals of strings of this length.", "8"},
        {"counts-only", 0, false, "Write no index: print `n_a n_b n_both n_either` to stdout.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Union, intersection or difference of the k-mer sets of two indexes, as an index.");
    static const vector<string> names = {"union", "intersection", "difference", "symmetric-difference"};
    const string opname = opts.get("op");
    int op = -1;
    for (size_t i = 0; i < names.size(); i++)
        if (names[i] == opname) op = (int)i;
    if (op < 0) throw std::runtime_error("Error: unknown set operation: " + opname);
    const bool counts_only = opts.count("counts-only");
    const string file_a = opts.get("index-a"), file_b = opts.get("index-b");
    const string out_file = counts_only ? string() : opts.get("out-file");          // (--counts-only writes no file: no -o needed)
    check_readable(file_a);
    check_readable(file_b);
    if (!counts_only) check_writable(out_file);
    use_gpu_option(opts);
    plain_matrix_sbwt_t A, B;
    load_plain_matrix(file_a, A);
    load_plain_matrix(file_b, B);
    auto log_counts = [](const sbwtgpu_setop_info &c) {
        write_log("k-mers: " + std::to_string(c.n_a) + " in a, " + std::to_string(c.n_b) + " in b, " + std::to_string(c.n_both) +
                      " in both, " + std::to_string(c.n_either) + " in either; Jaccard index " +
                      std::to_string(c.n_either ? (double)c.n_both / (double)c.n_either : 1.0),
                  LogLevel::MAJOR);
    };
    if (counts_only) {
        const sbwtgpu_setop_info c = plain_matrix_sbwt_t::set_operation_counts(A, B);
        log_counts(c);
        std::cout << c.n_a << " " << c.n_b << " " << c.n_both << " " << c.n_either << std::endl;
        return 0;
    }
    const int64_t precalc = precalc_option(opts, A.get_k());
    sbwtgpu_setop_info info;
    PlainMatrixBits bits = plain_matrix_sbwt_t::set_operation(A, B, op, !opts.count("no-streaming-support"), &info);
    log_counts(info);
    plain_matrix_sbwt_t index(bits, 0);
    write_log("The " + opname + " has " + std::to_string(index.number_of_kmers()) + " distinct k-mers, " +
                  std::to_string(index.number_of_subsets()) + " subsets", LogLevel::MAJOR);
    write_index_file(index, out_file, precalc);
    write_log("Wrote the index to " + out_file, LogLevel::MAJOR);
    return 0;
}

// ---- colours and pseudoalignment (include/sbwtgpu.h) ----
// `--threshold` (or the fraction of `option`) as parts per million, from its decimal text and without floating point:
// "0.7" -> 700000, "1" -> 1000000.  Digits (at least one), optionally '.' and digits; what comes after the sixth decimal must
// be zeros; 0 < value <= 1, or with allow_zero 0 <= value <= 1.
int64_t parse_threshold_ppm(const string &s, const char *option = "--threshold", bool allow_zero = false) {
    const size_t dot = s.find('.');
    const string ip = s.substr(0, dot), fp = dot == string::npos ? string() : s.substr(dot + 1);
    bool ok = !ip.empty() && ip.size() <= 9 && (dot == string::npos || !fp.empty());
    for (char ch : ip + fp) ok = ok && ch >= '0' && ch <= '9';
    int64_t ppm = 0;
    if (ok) {
        ppm = atoll(ip.c_str()) * 1000000;
        int64_t scale = 100000;
        for (size_t i = 0; i < fp.size(); i++) {
            if (i < 6) { ppm += (fp[i] - '0') * scale; scale /= 10; }
            else if (fp[i] != '0') ok = false;
        }
    }
    if (!ok || ppm < (allow_zero ? 0 : 1) || ppm > 1000000)
        throw std::runtime_error(string("Error: ") + option + " must be a decimal number in " + (allow_zero ? "0 .. 1" : "(0, 1]") +
                                 " with at most six decimals, not '" + s + "'");
    return ppm;
}

void colors_check(int rc) {
    if (rc != SBWTGPU_OK) throw std::runtime_error(string("Error: ") + sbwtgpu_last_error());
}
struct ColorsHandle {
    sbwtgpu_colors *h = nullptr;
    ~ColorsHandle() { sbwtgpu_colors_destroy(h); }
};
struct ColorSetsHandle {
    sbwtgpu_colorsets *h = nullptr;
    ~ColorSetsHandle() { sbwtgpu_colorsets_destroy(h); }
};
struct ColorSetsBuilderHandle {
    sbwtgpu_colorsets_builder *h = nullptr;
    ~ColorSetsBuilderHandle() { sbwtgpu_colorsets_builder_destroy(h); }
};

// the first 8 bytes of a colour file say which calls it goes through
bool file_has_magic(const string &file, const char *magic) {
    std::ifstream in(file, std::ios::binary);
    char got[8] = {0};
    in.read(got, 8);
    return in.gcount() == 8 && memcmp(got, magic, 8) == 0;
}

void host_check(int rc) {
    if (rc != 0) throw std::runtime_error(sbwthost_last_error());
}

// A colour file of `index` read and put on the device; a file of another index is refused.  What the file may be:
//   ROWS_ONLY    an "SBWTCOL1" or "SBWTCOL2" file, both through the wide reader into a wide colours object (compress-colors)
//   ANY_AS_WIDE  the same, or an "SBWTCOL3" file into a colour-set object (load_colorsets)
//   ANY          "SBWTCOL3" into a colour-set object, "SBWTCOL2" into a wide colours object, anything else through the
//                narrow reader into a narrow one: the three routes of pseudoalign
struct ColorFile {
    enum Accept { ROWS_ONLY, ANY_AS_WIDE, ANY };
    ColorsHandle col;          // one of col.h and sets.h is set
    ColorSetsHandle sets;
    bool wide = true;          // col holds rows of `words` words (sbwtgpu_colors_create_wide)
    int64_t words = 1;
};
void load_color_file(const string &colorsfile, const string &indexfile, const plain_matrix_sbwt_t &index, ColorFile::Accept accept,
                     ColorFile &out) {
    const char *file = colorsfile.c_str();
    const bool sets = accept != ColorFile::ROWS_ONLY && file_has_magic(colorsfile, "SBWTCOL3");
    const bool wide = sets || accept != ColorFile::ANY || file_has_magic(colorsfile, "SBWTCOL2");
    int64_t n_columns = 0, n_colors = 0, ck = 0, words = 1, n_sets = 0;
    host_check(sets   ? sbwthost_colorsets_read(file, &n_columns, &n_colors, &ck, &words, &n_sets, nullptr, 0, nullptr, 0)
               : wide ? sbwthost_colors_read_wide(file, &n_columns, &n_colors, &ck, &words, nullptr, 0)
                      : sbwthost_colors_read(file, &n_columns, &n_colors, &ck, nullptr, 0));
    if (n_columns != index.number_of_subsets() || ck != index.get_k())
        throw std::runtime_error("Error: " + colorsfile + " colours an index of " + std::to_string(n_columns) + " columns at k = " +
                                 std::to_string(ck) + ", " + indexfile + " has " + std::to_string(index.number_of_subsets()) +
                                 " columns at k = " + std::to_string(index.get_k()));
    if (sets) {
        vector<uint32_t> ids((size_t)n_columns);
        vector<uint64_t> table((size_t)(n_sets * words));
        host_check(sbwthost_colorsets_read(file, &n_columns, &n_colors, &ck, &words, &n_sets, ids.data(), n_columns, table.data(),
                                           n_sets * words));
        colors_check(sbwtgpu_colorsets_create(index.device_handle(), (int)n_colors, ids.data(), n_sets, table.data(), &out.sets.h));
    } else {
        vector<uint64_t> rows((size_t)(n_columns * words));
        host_check(wide ? sbwthost_colors_read_wide(file, &n_columns, &n_colors, &ck, &words, rows.data(), n_columns * words)
                        : sbwthost_colors_read(file, &n_columns, &n_colors, &ck, rows.data(), n_columns));
        if (wide) colors_check(sbwtgpu_colors_create_wide(index.device_handle(), (int)n_colors, rows.data(), &out.col.h));
        else colors_check(sbwtgpu_colors_create(index.device_handle(), (int)n_colors, rows.data(), &out.col.h));
    }
    out.wide = wide;
    out.words = words;
}

// writes a colour-set object as an "SBWTCOL3" file; count_color >= 0: *count_out = the columns whose set holds that colour
void write_colorsets(const sbwtgpu_colorsets *sets, const string &outfile, int count_color = -1, int64_t *count_out = nullptr) {
    int64_t n_columns = 0, ck = 0, n_sets = 0, n_colored = 0, bytes = 0;
    int32_t n_colors = 0, words = 0;
    colors_check(sbwtgpu_colorsets_info(sets, &n_columns, &ck, &n_colors, &words, &n_sets, &n_colored, &bytes));
    vector<uint32_t> ids((size_t)n_columns);
    vector<uint64_t> table((size_t)(n_sets * words));
    colors_check(sbwtgpu_colorsets_copy(sets, ids.data(), table.data()));
    if (count_color >= 0 && count_out) {
        *count_out = 0;
        for (uint32_t id : ids) *count_out += (int64_t)((table[(size_t)id * words + (count_color >> 6)] >> (count_color & 63)) & 1u);
    }
    host_check(sbwthost_colorsets_write(outfile.c_str(), ids.data(), table.data(), n_columns, n_colors, ck, n_sets));
    write_log("Wrote " + std::to_string(n_sets) + " colour sets of " + std::to_string(n_colors) + " colours over " +
                  std::to_string(n_colored) + " coloured columns (" + std::to_string(bytes) + " bytes on the device) to " + outfile,
              LogLevel::MAJOR);
}

// compresses a colours object (sbwtgpu_colorsets_compress: the canonical form) and writes it as an "SBWTCOL3" file
void compress_and_write(const sbwtgpu_colors *col, const string &outfile) {
    ColorSetsHandle sets;
    colors_check(sbwtgpu_colorsets_compress(col, &sets.h));
    write_colorsets(sets.h, outfile);
}

// sbwt build-colors: refs.txt holds one sequence file per line, colour = 0-based line number (at most 64, with --wide at most
// 4096 and an "SBWTCOL2" colour file whatever the number); every file's k-mers that the index holds get the file's colour
int build_colors_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"refs", 'r', true, "A list of sequence files (FASTA or FASTQ, possibly gzipped), one per line: the colour of a file is its 0-based line number. At most 64 lines.", ""},
        {"out-file", 'o', true, "Output colour file.", ""},
        {"both-strands", 0, false, "Also colour the reverse complement of every k-mer (for indexes built with reverse complements).", ""},
        {"wide", 0, false, "Up to 4096 lines in the list; writes a wide colour file (several 64-bit words per column).", ""},
        {"compress", 0, false, "Up to 4096 lines in the list; writes a colour-set file (one id per column and the distinct colour sets).", ""},
        {"stream", 0, false, "With --compress: merge one reference at a time into the colour sets, without the wide matrix on the device. The same file.", ""},
        {"positions-out", 0, true, "Also write a position file: per column of the index the smallest (sequence, offset) at which its k-mer occurs; the sequences of the listed files are numbered 0, 1, ... in the order they are read.", ""},
        {"occurrences-out", 0, true, "Also write an occurrence file: per column of the index every (sequence, offset, strand) at which its k-mer occurs, the sequences numbered as for --positions-out. May be given together with --positions-out.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Colour the k-mers of an index by the reference files that hold them.");
    const string indexfile = opts.get("index-file"), refsfile = opts.get("refs"), outfile = opts.get("out-file");
    check_readable(indexfile);
    check_readable(refsfile);
    const vector<string> refs = readlines(refsfile);
    const bool compress = opts.count("compress");
    const bool stream = opts.count("stream");
    if (stream && !compress)
        throw std::runtime_error("Error: --stream builds a colour-set file and needs --compress (a colour file of rows is the matrix itself)");
    const bool wide = opts.count("wide") || compress;
    if (wide && (refs.empty() || refs.size() > SBWTGPU_MAX_COLORS))
        throw std::runtime_error("Error: " + refsfile + " lists " + std::to_string(refs.size()) + " files; a wide colour file holds 1 to " +
                                 std::to_string(SBWTGPU_MAX_COLORS) + " colours");
    if (!wide && (refs.empty() || refs.size() > 64))
        throw std::runtime_error("Error: " + refsfile + " lists " + std::to_string(refs.size()) +
                                 " files; a colour file holds 1 to 64 colours (use --wide for more)");
    for (const string &file : refs) check_readable(file);
    check_writable(outfile);
    const string posfile = opts.count("positions-out") ? opts.get("positions-out") : "";
    if (!posfile.empty()) check_writable(posfile);
    const string occfile = opts.count("occurrences-out") ? opts.get("occurrences-out") : "";
    if (!occfile.empty()) check_writable(occfile);
    const int strands = opts.count("both-strands") ? 2 : 1;
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    plain_matrix_sbwt_t::Positions positions;
    if (!posfile.empty()) positions = index.positions();
    plain_matrix_sbwt_t::Occurrences occurrences;
    if (!occfile.empty()) occurrences = index.occurrences();
    ColorsHandle col;
    ColorSetsBuilderHandle builder;
    if (stream) colors_check(sbwtgpu_colorsets_builder_create(index.device_handle(), (int)refs.size(), &builder.h));
    else if (wide) colors_check(sbwtgpu_colors_create_wide(index.device_handle(), (int)refs.size(), nullptr, &col.h));
    else colors_check(sbwtgpu_colors_create(index.device_handle(), (int)refs.size(), nullptr, &col.h));
    vector<int64_t> windows(refs.size(), 0), hit_windows(refs.size(), 0);
    int open_color = -1;            // --stream: the colour that only finish closes
    for (size_t c = 0; c < refs.size(); c++) {
        seq_io::Reader reader(refs[c]);
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            int64_t w = 0, h = 0;
            if (stream) {
                colors_check(sbwtgpu_colorsets_builder_add_batch(builder.h, (int)c, bases.data(), read_off.data(), n_reads, strands, &w, &h));
                open_color = (int)c;
            } else {
                colors_check(sbwtgpu_colors_add_batch(col.h, (int)c, bases.data(), read_off.data(), n_reads, strands, &w, &h));
            }
            windows[c] += w;
            hit_windows[c] += h;
            if (positions.h) positions.add(bases.data(), read_off.data(), n_reads, strands, (int32_t)c);
            if (occurrences.b) occurrences.add(bases.data(), read_off.data(), n_reads, strands, (int32_t)c);
        });
    }
    if (positions.h) {
        positions.save(posfile);
        const plain_matrix_sbwt_t::Positions::Info pi = positions.info();
        write_log("Wrote the positions of " + std::to_string(pi.n_positioned) + " columns on " + std::to_string(positions.seqs.size()) +
                      " sequences to " + posfile,
                  LogLevel::MAJOR);
    }
    if (occurrences.b) {
        occurrences.finish();
        occurrences.save(occfile);
        const plain_matrix_sbwt_t::Occurrences::Info oi = occurrences.info();
        write_log("Wrote " + std::to_string(oi.n_occurrences) + " occurrences of " + std::to_string(oi.n_positioned) + " columns on " +
                      std::to_string(occurrences.seqs.size()) + " sequences to " + occfile,
                  LogLevel::MAJOR);
    }
    int64_t n_columns = 0, ck = 0, n_colored = 0;
    int32_t n_colors = 0;
    vector<int64_t> per_color(refs.size(), 0);
    ColorSetsHandle streamed;
    if (stream) {
        // per_color of the closed colours; the last colour with sequences is still open, finish closes it, and the builder
        // answers nothing afterwards: its columns are counted in the object that is written
        colors_check(sbwtgpu_colorsets_builder_info(builder.h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, per_color.data(), nullptr));
        colors_check(sbwtgpu_colorsets_builder_finish(builder.h, &streamed.h));
        int64_t last = 0;
        write_colorsets(streamed.h, outfile, open_color, &last);
        if (open_color >= 0) per_color[(size_t)open_color] = last;
    } else if (wide) {
        colors_check(sbwtgpu_colors_info_wide(col.h, &n_columns, &ck, &n_colors, &n_colored, per_color.data()));
    } else {
        sbwtgpu_colors_info_t info;
        colors_check(sbwtgpu_colors_info(col.h, &info));
        n_columns = info.n_columns, ck = info.k, n_colors = info.n_colors, n_colored = info.n_colored_columns;
        std::copy(info.per_color, info.per_color + refs.size(), per_color.begin());
    }
    for (size_t c = 0; c < refs.size(); c++)
        std::cout << "colour " << c << ": " << windows[c] << " windows, " << hit_windows[c] << " hit windows, " << per_color[c]
                  << " coloured columns" << std::endl;
    if (stream) return 0;
    if (compress) {
        compress_and_write(col.h, outfile);
        return 0;
    }
    vector<uint64_t> rows((size_t)n_columns * (size_t)sbwtgpu_colors_words(col.h));
    colors_check(sbwtgpu_colors_copy(col.h, rows.data()));
    host_check(wide ? sbwthost_colors_write_wide(outfile.c_str(), rows.data(), n_columns, n_colors, ck)
                    : sbwthost_colors_write(outfile.c_str(), rows.data(), n_columns, n_colors, ck));
    write_log("Wrote " + std::to_string(n_colors) + " colours of " + std::to_string(n_colored) + " coloured columns to " + outfile,
              LogLevel::MAJOR);
    return 0;
}

// sbwt compress-colors: an "SBWTCOL1" or "SBWTCOL2" colour file of the index -> the "SBWTCOL3" file that
// `sbwt build-colors --compress` writes for the same colouring
int compress_colors_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors, with or without --wide).", ""},
        {"out-file", 'o', true, "Output colour-set file.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Deduplicate the colour sets of a colour file: one id per column and a table of the distinct sets.");
    const string indexfile = opts.get("index-file"), colorsfile = opts.get("colors-file"), outfile = opts.get("out-file");
    check_readable(indexfile);
    check_readable(colorsfile);
    check_writable(outfile);
    use_gpu_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorFile f;
    load_color_file(colorsfile, indexfile, index, ColorFile::ROWS_ONLY, f);
    compress_and_write(f.col.h, outfile);
    return 0;
}

// the colour-set object of a colour file of `index`: an "SBWTCOL3" file goes in directly, an "SBWTCOL1" or "SBWTCOL2" file is
// compressed on the device first (sbwtgpu_colorsets_compress, as compress-colors does); a file of another index is refused
void load_colorsets(const string &colorsfile, const string &indexfile, const plain_matrix_sbwt_t &index, ColorSetsHandle &out) {
    ColorFile f;
    load_color_file(colorsfile, indexfile, index, ColorFile::ANY_AS_WIDE, f);
    if (f.sets.h) std::swap(out.h, f.sets.h);
    else colors_check(sbwtgpu_colorsets_compress(f.col.h, &out.h));
}

// floor(shared * 10^6 / (ka + kb - shared)) in 128-bit integers, 0 where the denominator is 0: no floats, so the text is stable
int64_t jaccard_ppm(int64_t shared, int64_t ka, int64_t kb) {
    const __int128 den = (__int128)ka + (__int128)kb - (__int128)shared;
    if (den <= 0) return 0;
    return (int64_t)((__int128)shared * 1000000 / den);
}

// sbwt color-matrix: the k-mers each pair of references shares (sbwtgpu_colorsets_shared_kmers), C lines of C tab-separated
// integers; --jaccard-ppm: the Jaccard index of each pair in parts per million instead
int color_matrix_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors with or without --wide or --compress, compress-colors, merge-colors).", ""},
        {"out-file", 'o', true, "Output file: line a holds the shared k-mer counts of reference a with every reference, tab-separated.", ""},
        {"jaccard-ppm", 0, false, "Write floor(10^6 * shared / (k-mers of a + k-mers of b - shared)) instead of the counts (0 where both have none).", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Count the k-mers that each pair of references shares.");
    const string indexfile = opts.get("index-file"), colorsfile = opts.get("colors-file"), outfile = opts.get("out-file");
    const bool jaccard = opts.count("jaccard-ppm") > 0;
    check_readable(indexfile);
    check_readable(colorsfile);
    check_writable(outfile);
    use_gpu_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorSetsHandle sets;
    load_colorsets(colorsfile, indexfile, index, sets);
    int32_t n_colors = 0;
    colors_check(sbwtgpu_colorsets_info(sets.h, nullptr, nullptr, &n_colors, nullptr, nullptr, nullptr, nullptr));
    const size_t C = (size_t)n_colors;
    vector<int64_t> G(C * C);
    sbwtgpu_shared_info info;
    colors_check(sbwtgpu_colorsets_shared_kmers(sets.h, nullptr, G.data(), &info));
    string text;
    text.reserve(C * C * 8);
    for (size_t a = 0; a < C; a++)
        for (size_t b = 0; b < C; b++) {
            append_int(jaccard ? jaccard_ppm(G[a * C + b], G[a * C + a], G[b * C + b]) : G[a * C + b], text);
            text.push_back(b + 1 == C ? '\n' : '\t');
        }
    write_text_file(outfile, text, false);
    write_log("Wrote the shared k-mers of " + std::to_string(n_colors) + " references from " + std::to_string(info.n_sets_used) +
                  " colour sets (" + (info.used_mfma ? "matrix cores" : "plain kernel") + ")",
              LogLevel::MAJOR);
    return 0;
}

// sbwt screen: which references are in a read set, and how much of each (include/sbwtgpu.h, "screen").  The output starts with
// "# windows <n_windows> hits <n_hits> seen <n_seen>", then one line per colour: colour, ref_kmers, ref_seen, ref_hits,
// tab-separated; --sets-out: one line per set id: id, set_kmers, set_seen, set_hits.  Batches go to the GPU one at a time and
// nothing comes back until the end.
int screen_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors with or without --wide or --compress, compress-colors, merge-colors).", ""},
        {"query-file", 'q', true, "The reads in FASTA or FASTQ format, possibly gzipped.", ""},
        {"out-file", 'o', true, "Output file: a header line, then per colour its k-mers, the k-mers the reads contain, and the hits.", ""},
        {"sets-out", 0, true, "Also write the same three numbers per colour set, one line per set id.", ""},
        {"both-strands", 0, false, "The reverse complement of every window counts as a window too.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Screen a read set against the references: per colour k-mers, k-mers seen, hits.");
    const string indexfile = opts.get("index-file"), colorsfile = opts.get("colors-file"), queryfile = opts.get("query-file"),
                 outfile = opts.get("out-file"), setsfile = opts.count("sets-out") ? opts.get("sets-out") : string();
    check_readable(indexfile);
    check_readable(colorsfile);
    check_readable(queryfile);
    check_writable(outfile);
    if (!setsfile.empty()) check_writable(setsfile);
    const int strands = opts.count("both-strands") ? 2 : 1;
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorSetsHandle sets;
    load_colorsets(colorsfile, indexfile, index, sets);
    plain_matrix_sbwt_t::Screen screen = index.screen(sets.h);
    int64_t total_reads = 0;
    {
        seq_io::Reader reader(queryfile);
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            screen.add(bases.data(), read_off.data(), n_reads, strands);
            total_reads += n_reads;
        });
    }
    const plain_matrix_sbwt_t::Screen::Info info = screen.info();
    auto table = [](const plain_matrix_sbwt_t::Screen::Vectors &v, string &text) {
        for (size_t i = 0; i < v.kmers.size(); i++) {
            append_int((int64_t)i, text);
            text.push_back('\t');
            append_int(v.kmers[i], text);
            text.push_back('\t');
            append_int(v.seen[i], text);
            text.push_back('\t');
            append_int(v.hits[i], text);
            text.push_back('\n');
        }
    };
    string text = "# windows " + std::to_string(info.n_windows) + " hits " + std::to_string(info.n_hits) + " seen " +
                  std::to_string(info.n_seen) + "\n";
    table(screen.colors(), text);
    write_text_file(outfile, text, false);
    if (!setsfile.empty()) {
        text.clear();
        table(screen.sets(), text);
        write_text_file(setsfile, text, false);
    }
    write_log("Screened " + std::to_string(total_reads) + " reads against " + std::to_string(info.n_colors) + " references: " +
                  std::to_string(info.n_hits) + " hits in " + std::to_string(info.n_windows) + " windows, " +
                  std::to_string(info.n_seen) + " k-mers seen",
              LogLevel::MAJOR);
    write_log("us/read end-to-end: " + std::to_string((double)(cur_time_micros() - micros_start) / (double)std::max<int64_t>(1, total_reads)),
              LogLevel::MAJOR);
    return 0;
}

// dump-unitigs --colors: coloured unitigs as FASTA, the header "number set-id" (a parser that takes the id up to the first
// blank still sees the number); --sets-out: line i = "i c1 c2 ..." for set id i = 0 .. n_sets - 1, the line of set 0 is "0"
int dump_unitigs_colored(const plain_matrix_sbwt_t &index, const string &indexfile, const string &colorsfile, const string &outfile,
                         const string &setsfile, bool gzip, bool gfa) {
    ColorSetsHandle sets;
    load_colorsets(colorsfile, indexfile, index, sets);
    const plain_matrix_sbwt_t::ColoredUnitigs u = index.colored_unitigs(sets.h, gfa);
    const int64_t n = (int64_t)u.first_col.size();
    string text;
    if (gfa) {
        text = gfa_text(u.bases, u.off, u.link_off, u.link_to, &u.set_id, index.get_k());
    } else {
        text.reserve(u.bases.size() + (size_t)n * 20);
        for (int64_t i = 0; i < n; i++) {
            text.push_back('>');
            append_int(i, text);
            text.push_back(' ');
            append_int((int64_t)u.set_id[(size_t)i], text);
            text.push_back('\n');
            text.append(u.bases.data() + u.off[(size_t)i], (size_t)(u.off[(size_t)i + 1] - u.off[(size_t)i]));
            text.push_back('\n');
        }
    }
    write_text_file(outfile, text, gzip);
    if (!setsfile.empty()) {
        int32_t words = 0;
        int64_t n_columns = 0, n_sets = 0;
        colors_check(sbwtgpu_colorsets_info(sets.h, &n_columns, nullptr, nullptr, &words, &n_sets, nullptr, nullptr));
        vector<uint32_t> ids((size_t)n_columns);
        vector<uint64_t> table((size_t)(n_sets * words));
        colors_check(sbwtgpu_colorsets_copy(sets.h, ids.data(), table.data()));
        string lines;
        for (int64_t i = 0; i < n_sets; i++) {
            append_int(i, lines);
            append_set_bits(table.data() + i * words, words, " ", " ", lines);
            lines.push_back('\n');
        }
        write_text_file(setsfile, lines, false);
    }
    write_log("Wrote " + std::to_string(n) + " coloured unitigs, " + std::to_string(u.bases.size()) + " bases, " +
                  std::to_string(u.n_color_breaks) + " colour breaks, " + std::to_string(u.n_sets) + " colour sets" +
                  (gfa ? ", " + std::to_string(u.link_to.size()) + " links" : string()),
              LogLevel::MAJOR);
    return 0;
}

// sbwt thread: the reads threaded through the unitig graph of the index.  One line per read, in read
// order: the 0-based read number, then one `read_pos:unitig:offset:n_kmers` per step, space-separated.  --colors threads
// through the coloured graph; --coverage writes `unitig<TAB>n_kmers<TAB>kmer_hits` per unitig; --gfa writes the graph as
// `dump-unitigs --gfa` does with a KC:i: tag (the k-mer hits) on every segment.
int thread_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output filename.", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"query-file", 'q', true, "The reads in FASTA or FASTQ format, possibly gzipped.", ""},
        {"gzip-output", 'z', false, "Writes the walks in gzipped form.", ""},
        {"colors", 0, true, "Colour file or colour-set file of the index: thread through the coloured unitigs.", ""},
        {"coverage", 0, true, "Write one line per unitig: unitig, its k-mers, the k-mer hits of the reads on it (tab-separated).", ""},
        {"gfa", 0, true, "Write the graph as GFA 1, as dump-unitigs --gfa does, with the k-mer hits as a KC:i: tag per segment.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Per read: the unitigs of the de Bruijn graph it runs along, as read_pos:unitig:offset:n_kmers steps.");
    const string indexfile = opts.get("index-file"), queryfile = opts.get("query-file"), outfile = opts.get("out-file");
    const bool colored = opts.count("colors");
    const string colorsfile = colored ? opts.get("colors") : string();
    const string covfile = opts.count("coverage") ? opts.get("coverage") : string(), gfafile = opts.count("gfa") ? opts.get("gfa") : string();
    check_readable(indexfile);
    check_readable(queryfile);
    if (colored) check_readable(colorsfile);
    check_writable(outfile);
    if (!covfile.empty()) check_writable(covfile);
    if (!gfafile.empty()) check_writable(gfafile);
    const bool gzip_output = opts.count("gzip-output"), coverage = !covfile.empty() || !gfafile.empty();
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);

    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorSetsHandle sets;
    if (colored) load_colorsets(colorsfile, indexfile, index, sets);
    const plain_matrix_sbwt_t::UnitigGraph graph = index.unitig_graph(colored ? sets.h : nullptr);
    vector<int64_t> kmer_hits;
    int64_t total_reads = 0, total_steps = 0;
    {
        write_log("Threading the reads of " + queryfile + " to output file " + outfile, LogLevel::MAJOR);
        seq_io::Reader reader(queryfile);
        seq_io::Buffered_ofstream writer(outfile, gzip_output);
        string text;
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            const plain_matrix_sbwt_t::Walks w = index.walks(graph, bases.data(), read_off.data(), n_reads, coverage);
            text.clear();
            for (int64_t r = 0; r < n_reads; r++) {
                append_int(total_reads + r, text);
                for (int64_t s = w.step_off[(size_t)r]; s < w.step_off[(size_t)r + 1]; s++) {
                    const sbwtgpu_walk_step &st = w.steps[(size_t)s];
                    text.push_back(' ');
                    append_int(st.read_pos, text);
                    text.push_back(':');
                    append_int((int64_t)st.unitig, text);
                    text.push_back(':');
                    append_int((int64_t)st.offset, text);
                    text.push_back(':');
                    append_int(st.n_kmers, text);
                }
                text.push_back('\n');
            }
            writer.write(text.data(), (int64_t)text.size());
            if (coverage) {
                if (kmer_hits.empty()) kmer_hits = w.unitig_kmers;
                else for (size_t i = 0; i < kmer_hits.size(); i++) kmer_hits[i] += w.unitig_kmers[i];
            }
            total_reads += n_reads;
            total_steps += (int64_t)w.steps.size();
        });
    }
    if (coverage) {
        const plain_matrix_sbwt_t::ColoredUnitigs u = graph.unitigs();
        const int64_t n = (int64_t)u.first_col.size(), k = index.get_k();
        kmer_hits.resize((size_t)n, 0);                  // (no read at all: zeros)
        if (!covfile.empty()) {
            string lines;
            for (int64_t i = 0; i < n; i++) {
                append_int(i, lines);
                lines.push_back('\t');
                append_int(u.off[(size_t)i + 1] - u.off[(size_t)i] - (k - 1), lines);
                lines.push_back('\t');
                append_int(kmer_hits[(size_t)i], lines);
                lines.push_back('\n');
            }
            write_text_file(covfile, lines, false);
        }
        if (!gfafile.empty())
            write_text_file(gfafile, gfa_text(u.bases, u.off, u.link_off, u.link_to, colored ? &u.set_id : nullptr, k, &kmer_hits), false);
    }
    write_log("Threaded " + std::to_string(total_reads) + " reads: " + std::to_string(total_steps) + " steps; us/read end-to-end: " +
                  std::to_string((double)(cur_time_micros() - micros_start) / (double)std::max<int64_t>(1, total_reads)),
              LogLevel::MAJOR);
    return 0;
}

// the set bits of a `words`-word row as comma-separated ascending colours, "-" for none
void append_color_list(const uint64_t *row, int32_t words, string &text) {
    const size_t before = text.size();
    append_set_bits(row, words, "", ",", text);
    if (text.size() == before) text.push_back('-');
}

// sbwt bubbles: the variant sites of the plain unitig graph (include/sbwtgpu.h, "bubbles").  The output starts with
// "# unitigs U links L bubbles B snps S", then one line per bubble in record order: source, branch_a, branch_b, sink, n_a,
// n_b, SNP|OTHER, allele_a, allele_b, tab-separated; with -c two more fields, the colours of each branch: those of inter,
// comma-separated ascending ("-" for none), and "|" and those of uni where the two differ.  --snps-only keeps the SNP lines.
// With -q the reads are genotyped at the bubbles (include/sbwtgpu.h, "genotype"): the header gains " windows W hits H
// site_hits S", every line seen_a, hits_a, min_a, seen_b, hits_b, min_b and the call (. a b ab); --refs-out writes per colour
// `colour sites match only`.  Batches go to the GPU one at a time and nothing comes back until the end.
int bubbles_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors with or without --wide or --compress, compress-colors, merge-colors): adds the colours of each branch.", ""},
        {"out-file", 'o', true, "Output file: a header line, then one tab-separated line per bubble.", ""},
        {"gzip-output", 'z', false, "Writes the output in gzipped form.", ""},
        {"snps-only", 0, false, "Write only the bubbles of kind SNP (the header still counts all).", ""},
        {"query-file", 'q', true, "Reads in FASTA or FASTQ format, possibly gzipped: genotype them at the bubbles (per allele k-mers seen, hits, smallest depth; the call).", ""},
        {"both-strands", 0, false, "With -q: the reverse complement of every window counts as a window too.", ""},
        {"min-breadth", 0, true, "With -q: an allele is present when at least this fraction of its k-mers is seen.", "1.0"},
        {"min-depth", 0, true, "With -q: ... and its hits are at least this many times its k-mers.", "1"},
        {"refs-out", 0, true, "With -q and -c: write per colour the called bubbles where it is informative, those that match it, those that carry only its allele.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Find the bubbles of the unitig graph: where the references differ, and which reference carries which allele.");
    const string indexfile = opts.get("index-file"), outfile = opts.get("out-file");
    const bool colored = opts.count("colors-file") > 0, gzip_output = opts.count("gzip-output") > 0, snps_only = opts.count("snps-only") > 0;
    const bool query = opts.count("query-file") > 0;
    const string colorsfile = colored ? opts.get("colors-file") : string(), queryfile = query ? opts.get("query-file") : string();
    const string refsfile = opts.count("refs-out") ? opts.get("refs-out") : string();
    for (const char *name : {"both-strands", "min-breadth", "min-depth", "refs-out"})
        if (!query && opts.count(name)) throw std::runtime_error(string("Error: --") + name + " needs a query file (-q)");
    if (!refsfile.empty() && !colored) throw std::runtime_error("Error: --refs-out needs a colour file (-c)");
    const int strands = opts.count("both-strands") ? 2 : 1;
    const int breadth_ppm = query ? (int)parse_threshold_ppm(opts.get("min-breadth"), "--min-breadth") : 1000000;
    const string depth_text = opts.get("min-depth");
    if (depth_text.empty() || depth_text.size() > 18 || depth_text.find_first_not_of("0123456789") != string::npos)
        throw std::runtime_error("Error: --min-depth must be a non-negative integer, not '" + depth_text + "'");
    const int64_t min_depth = atoll(depth_text.c_str());
    check_readable(indexfile);
    if (colored) check_readable(colorsfile);
    if (query) check_readable(queryfile);
    check_writable(outfile);
    if (!refsfile.empty()) check_writable(refsfile);
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorSetsHandle sets;
    if (colored) load_colorsets(colorsfile, indexfile, index, sets);
    const plain_matrix_sbwt_t::UnitigGraph graph = index.unitig_graph();
    plain_matrix_sbwt_t::Genotype gt;
    plain_matrix_sbwt_t::Genotype::Info gi;
    plain_matrix_sbwt_t::Genotype::Branches gb;
    plain_matrix_sbwt_t::Genotype::Calls gc;
    if (query) {
        gt = index.genotype(graph, colored ? sets.h : nullptr);
        seq_io::Reader reader(queryfile);
        for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
            gt.add(bases.data(), read_off.data(), n_reads, strands);
        });
        gi = gt.info();
        gb = gt.branches();
        gc = gt.calls(breadth_ppm, min_depth);
    }
    const plain_matrix_sbwt_t::Bubbles own = query ? plain_matrix_sbwt_t::Bubbles() : index.bubbles(graph, colored ? sets.h : nullptr);
    const plain_matrix_sbwt_t::Bubbles &bb = query ? gt.bubbles : own;
    const plain_matrix_sbwt_t::ColoredUnitigs u = graph.unitigs();
    string text = "# unitigs ";
    append_int((int64_t)u.first_col.size(), text);
    text += " links ";
    append_int((int64_t)u.link_to.size(), text);
    text += " bubbles ";
    append_int((int64_t)bb.rec.size(), text);
    text += " snps ";
    append_int(bb.n_snps, text);
    if (query) {
        text += " windows ";
        append_int(gi.n_windows, text);
        text += " hits ";
        append_int(gi.n_hits, text);
        text += " site_hits ";
        append_int(gi.n_site_hits, text);
    }
    text.push_back('\n');
    const size_t W = (size_t)bb.words;
    for (size_t i = 0; i < bb.rec.size(); i++) {
        const sbwtgpu_bubble &r = bb.rec[i];
        if (snps_only && r.kind != SBWTGPU_BUBBLE_SNP) continue;
        const int64_t f[6] = {r.source, r.branch[0], r.branch[1], r.sink, r.n_kmers[0], r.n_kmers[1]};
        for (int j = 0; j < 6; j++) {
            append_int(f[j], text);
            text.push_back('\t');
        }
        text += r.kind == SBWTGPU_BUBBLE_SNP ? "SNP" : "OTHER";
        for (int j = 0; j < 2; j++) {                      // the allele: the last n_kmers characters of the branch
            text.push_back('\t');
            const int64_t end = u.off[(size_t)r.branch[j] + 1];
            text.append(u.bases.data() + (end - (int64_t)r.n_kmers[j]), (size_t)r.n_kmers[j]);
        }
        for (int j = 0; colored && j < 2; j++) {
            text.push_back('\t');
            const uint64_t *in = bb.inter.data() + (2 * i + (size_t)j) * W, *un = bb.uni.data() + (2 * i + (size_t)j) * W;
            append_color_list(in, bb.words, text);
            if (!std::equal(in, in + W, un)) {
                text.push_back('|');
                append_color_list(un, bb.words, text);
            }
        }
        if (query) {
            static const char *const CALL[4] = {".", "a", "b", "ab"};
            for (size_t s = 2 * i; s < 2 * i + 2; s++)
                for (const int64_t x : {gb.seen[s], gb.hits[s], gb.min_hits[s]}) {
                    text.push_back('\t');
                    append_int(x, text);
                }
            text.push_back('\t');
            text += CALL[gc.call[i] & 3];
        }
        text.push_back('\n');
    }
    {
        seq_io::Buffered_ofstream writer(outfile, gzip_output);
        writer.write(text.data(), (int64_t)text.size());
    }
    if (!refsfile.empty()) {
        string lines;
        for (size_t c = 0; c < gc.ref_sites.size(); c++) {
            append_int((int64_t)c, lines);
            for (const int64_t x : {gc.ref_sites[c], gc.ref_match[c], gc.ref_only[c]}) {
                lines.push_back('\t');
                append_int(x, lines);
            }
            lines.push_back('\n');
        }
        write_text_file(refsfile, lines, false);
    }
    write_log("Wrote " + std::to_string(bb.rec.size()) + " bubbles (" + std::to_string(bb.n_snps) + " SNPs) of " +
                  std::to_string(u.first_col.size()) + " unitigs", LogLevel::MAJOR);
    return 0;
}

// sbwt merge-colors: the colour sets of one or two coloured indexes carried onto index U (the output of `sbwt set-op`, for
// one), without any sequence file: the "SBWTCOL3" file that build-colors --compress writes for U and the same colouring
int merge_colors_main(int argc, char **argv) {
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"index-u", 'u', true, "Target index input file (the output of set-op, or any index with the same k).", ""},
        {"index-a", 'a', true, "First coloured index input file.", ""},
        {"colors-a", 0, true, "Colour file or colour-set file of the first index.", ""},
        {"index-b", 'b', true, "Second coloured index input file (optional; needs --colors-b).", ""},
        {"colors-b", 0, true, "Colour file or colour-set file of the second index.", ""},
        {"color-offset", 0, true, "Added to every colour of the second index (default: the number of colours of the first; 0 shares the colour space).", ""},
        {"out-file", 'o', true, "Output colour-set file of the target index.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Carry the colour sets of one or two indexes onto another index (merge-colors), without the sequences.");
    const string file_u = opts.get("index-u"), file_a = opts.get("index-a"), colors_a = opts.get("colors-a"), outfile = opts.get("out-file");
    const bool two = opts.count("index-b") || opts.count("colors-b");
    if (two && !(opts.count("index-b") && opts.count("colors-b")))
        throw std::runtime_error("Error: --index-b and --colors-b come together");
    if (!two && opts.count("color-offset") && atoll(opts.get("color-offset").c_str()) != 0)
        throw std::runtime_error("Error: --color-offset needs a second index (--index-b and --colors-b)");
    const string file_b = two ? opts.get("index-b") : string(), colors_b = two ? opts.get("colors-b") : string();
    for (const string &f : {file_u, file_a, colors_a}) check_readable(f);
    if (two) {
        check_readable(file_b);
        check_readable(colors_b);
    }
    check_writable(outfile);
    use_gpu_option(opts);
    plain_matrix_sbwt_t U, A, B;
    load_plain_matrix(file_u, U);
    load_plain_matrix(file_a, A);
    if (two) load_plain_matrix(file_b, B);
    ColorSetsHandle sa, sb, merged;
    load_colorsets(colors_a, file_a, A, sa);
    if (two) load_colorsets(colors_b, file_b, B, sb);
    int32_t n_colors_a = 0;
    colors_check(sbwtgpu_colorsets_info(sa.h, nullptr, nullptr, &n_colors_a, nullptr, nullptr, nullptr, nullptr));
    const long long offset = opts.count("color-offset") ? atoll(opts.get("color-offset").c_str()) : (two ? n_colors_a : 0);
    if (offset < -2147483647ll || offset > 2147483647ll) throw std::runtime_error("Error: --color-offset " + opts.get("color-offset") + " is out of range");
    sbwtgpu_colorsets_merge_info info;
    colors_check(sbwtgpu_colorsets_merge(U.device_handle(), sa.h, sb.h, (int)offset, &merged.h, &info));
    write_colorsets(merged.h, outfile);
    std::cout << "merge-colors: " << info.n_real_u << " k-mers in u, " << info.n_from_a << " from a, " << info.n_from_b << " from b, "
              << info.n_from_both << " from both, " << info.n_pairs << " pairs, " << info.n_sets << " colour sets" << std::endl;
    return 0;
}

// a colour list of color-select: "all", or numbers and ranges "a-b" (a <= b) separated by commas, every colour below n_colors;
// the mask's words come back
vector<uint64_t> parse_color_list(const string &text, const string &flag, int n_colors) {
    vector<uint64_t> mask((size_t)(n_colors + 63) / 64, 0);
    auto bad = [&](const string &why) {
        return std::runtime_error("Error: malformed colour list for " + flag + " (" + why + "): '" + text + "'");
    };
    auto set_range = [&](int64_t lo, int64_t hi) {
        for (int64_t c = lo; c <= hi; c++) mask[(size_t)(c >> 6)] |= 1ull << (c & 63);
    };
    if (text == "all") {
        set_range(0, n_colors - 1);
        return mask;
    }
    if (text.empty()) throw bad("it is empty");
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t end = text.find(',', pos);
        if (end == string::npos) end = text.size();
        const string item = text.substr(pos, end - pos);
        const size_t dash = item.find('-');
        const string a = item.substr(0, dash), b = dash == string::npos ? a : item.substr(dash + 1);
        for (const string &num : {a, b}) {
            if (num.empty() || num.size() > 9) throw bad("'" + item + "' is no number or range");
            for (char ch : num)
                if (ch < '0' || ch > '9') throw bad("'" + item + "' is no number or range");
        }
        const int64_t lo = atoll(a.c_str()), hi = atoll(b.c_str());
        if (lo > hi) throw bad("the range '" + item + "' runs backwards");
        if (hi >= n_colors) throw bad("colour " + std::to_string(hi) + " of " + std::to_string(n_colors) + " colours");
        set_range(lo, hi);
        pos = end + 1;
    }
    return mask;
}
// --min / --max of color-select: a decimal number of at most nine digits
int parse_count(const string &text, const string &flag) {
    bool ok = !text.empty() && text.size() <= 9;
    for (char ch : text) ok = ok && ch >= '0' && ch <= '9';
    if (!ok) throw std::runtime_error("Error: " + flag + " must be a non-negative integer, not '" + text + "'");
    return atoi(text.c_str());
}

// sbwt color-select: the k-mers of a coloured index whose colour set satisfies a predicate, as the index `sbwt build` would
// write for them (sbwtgpu_colorsets_select; serialised as set-op serialises its result); --colors-out: their colour sets on
// that index (sbwtgpu_colorsets_merge of the input's object onto it), an "SBWTCOL3" file
int color_select_main(int argc, char **argv) {
    set_log_level(LogLevel::MAJOR);
    Options opts({
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors with or without --wide or --compress, compress-colors, merge-colors).", ""},
        {"include", 0, true, "Colours that count: `all`, or numbers and ranges such as 0,3-5.", "all"},
        {"exclude", 0, true, "Colours a selected k-mer must not have (the same syntax; default: none).", ""},
        {"min", 0, true, "A selected k-mer has at least this many of the included colours.", "1"},
        {"max", 0, true, "... and at most this many (default: the number of included colours).", ""},
        {"out-file", 'o', true, "Output file for the resulting index.", ""},
        {"colors-out", 0, true, "Also write the colour sets of the resulting index to this file.", ""},
        {"no-streaming-support", 0, false, "Do not build the streaming query support bit vector.", ""},
        {"precalc-length", 'p', true, "Precalculate SBWT intervals of strings of this length.", "8"},
        {"counts-only", 0, false, "Write nothing: print `n_real n_selected n_sets_matched` to stdout.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Select the k-mers of a coloured index by their colour sets (core, unique, accessory, soft core), as an index.");
    const bool counts_only = opts.count("counts-only");
    const string indexfile = opts.get("index-file"), colorsfile = opts.get("colors-file");
    const string outfile = counts_only ? string() : opts.get("out-file");              // (--counts-only writes no file: no -o needed)
    const string colors_out = (!counts_only && opts.count("colors-out")) ? opts.get("colors-out") : string();
    check_readable(indexfile);
    check_readable(colorsfile);
    if (!counts_only) check_writable(outfile);
    if (!colors_out.empty()) check_writable(colors_out);
    use_gpu_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    ColorSetsHandle sets;
    load_colorsets(colorsfile, indexfile, index, sets);
    int32_t n_colors = 0;
    colors_check(sbwtgpu_colorsets_info(sets.h, nullptr, nullptr, &n_colors, nullptr, nullptr, nullptr, nullptr));
    const vector<uint64_t> include = parse_color_list(opts.get("include"), "--include", n_colors);
    vector<uint64_t> exclude;
    if (opts.count("exclude")) exclude = parse_color_list(opts.get("exclude"), "--exclude", n_colors);
    int n_included = 0;
    for (uint64_t w : include) n_included += __builtin_popcountll(w);
    sbwtgpu_color_predicate pred;
    pred.include = include.data();
    pred.exclude_or_null = exclude.empty() ? nullptr : exclude.data();
    pred.min_in = parse_count(opts.get("min"), "--min");
    pred.max_in = opts.count("max") ? parse_count(opts.get("max"), "--max") : std::max(n_included, (int)pred.min_in);
    auto log_counts = [](const sbwtgpu_color_select_info &c) {
        write_log("color-select: " + std::to_string(c.n_selected) + " of " + std::to_string(c.n_real) + " k-mers selected, " +
                      std::to_string(c.n_sets_matched) + " colour sets matched", LogLevel::MAJOR);
    };
    sbwtgpu_color_select_info info;
    if (counts_only) {
        colors_check(sbwtgpu_colorsets_select_counts(sets.h, &pred, &info));
        log_counts(info);
        std::cout << info.n_real << " " << info.n_selected << " " << info.n_sets_matched << std::endl;
        return 0;
    }
    const int64_t precalc = precalc_option(opts, index.get_k());
    PlainMatrixBits bits = index.color_select(sets.h, pred, !opts.count("no-streaming-support"), &info);
    log_counts(info);
    plain_matrix_sbwt_t sub(bits, 0);
    write_index_file(sub, outfile, precalc);
    write_log("Wrote the index to " + outfile, LogLevel::MAJOR);
    if (!colors_out.empty()) {
        ColorSetsHandle carried;
        colors_check(sbwtgpu_colorsets_merge(sub.device_handle(), sets.h, nullptr, 0, &carried.h, nullptr));
        write_colorsets(carried.h, colors_out);
    }
    return 0;
}

// sbwt pseudoalign: one line per read in input order -- the read's 0-based number, then the ids of its colours, ascending,
// separated by single spaces
int pseudoalign_main(int argc, char **argv) {
    int64_t micros_start = cur_time_micros();
    set_log_level(LogLevel::MINOR);
    Options opts({
        {"out-file", 'o', true, "Output filename.", ""},
        {"index-file", 'i', true, "Index input file.", ""},
        {"colors-file", 'c', true, "Colour file of the index (sbwt build-colors).", ""},
        {"query-file", 'q', true, "The query in FASTA or FASTQ format, possibly gzipped.", ""},
        {"gzip-output", 'z', false, "Writes output in gzipped form.", ""},
        {"threshold", 0, true, "A colour is reported when at least this fraction of the read's k-mers carries it.", "1.0"},
        {"all-kmers", 0, false, "The fraction is taken of all k-mers of the read instead of the k-mers found in the index.", ""},
        {"both-strands", 0, false, "A k-mer also carries the colours of its reverse complement.", ""},
        {"gpu", 0, true, "HIP device to run on.", "0"},
        {"batch-bases", 0, true, "Bases sent to the GPU per batch.", "268435456"},
        {"help", 'h', false, "Print usage", ""},
    });
    parse_or_usage(opts, argc, argv, "Per read: the references (colours) that hold it.");
    const string indexfile = opts.get("index-file"), colorsfile = opts.get("colors-file");
    const string queryfile = opts.get("query-file"), outfile = opts.get("out-file");
    check_readable(indexfile);
    check_readable(colorsfile);
    check_readable(queryfile);
    check_writable(outfile);
    const int threshold_ppm = (int)parse_threshold_ppm(opts.get("threshold"));
    const int denominator = opts.count("all-kmers") ? 1 : 0;
    const int strands = opts.count("both-strands") ? 2 : 1;
    const bool gzip_output = opts.count("gzip-output");
    use_gpu_option(opts);
    const int64_t batch_bases = batch_bases_option(opts);
    plain_matrix_sbwt_t index;
    load_plain_matrix(indexfile, index);
    // the colour file's magic says which calls it goes through: "SBWTCOL2" the wide ones, "SBWTCOL3" the colour-set ones
    // (whose records are the wide ones'), anything else where it always went
    ColorFile cf;
    load_color_file(colorsfile, indexfile, index, ColorFile::ANY, cf);
    const bool sets = cf.sets.h != nullptr;
    const int64_t words = cf.words;
    write_log("Running pseudoalignment from input file " + queryfile + " to output file " + outfile, LogLevel::MAJOR);
    seq_io::Reader reader(queryfile);
    seq_io::Buffered_ofstream writer(outfile, gzip_output);
    vector<sbwtgpu_pseudoalignment> rec;
    vector<sbwtgpu_read_found> wrec;
    vector<uint64_t> wcol;
    string text;
    int64_t total_reads = 0;
    for_each_batch(reader, batch_bases, [&](const vector<char> &bases, const vector<int64_t> &read_off, int64_t n_reads) {
        text.clear();
        if (cf.wide) {
            wrec.resize((size_t)n_reads);
            wcol.resize((size_t)(n_reads * words));
            if (sets)
                colors_check(sbwtgpu_pseudoalign_sets_batch(cf.sets.h, bases.data(), read_off.data(), n_reads, strands, threshold_ppm,
                                                            denominator, wrec.data(), wcol.data(), nullptr));
            else
                colors_check(sbwtgpu_pseudoalign_wide_batch(cf.col.h, bases.data(), read_off.data(), n_reads, strands, threshold_ppm,
                                                            denominator, wrec.data(), wcol.data(), nullptr));
            for (int64_t r = 0; r < n_reads; r++) {
                append_int(total_reads++, text);
                append_set_bits(wcol.data() + r * words, words, " ", " ", text);
                text.push_back('\n');
            }
        } else {
            rec.resize((size_t)n_reads);
            colors_check(sbwtgpu_pseudoalign_batch(cf.col.h, bases.data(), read_off.data(), n_reads, strands, threshold_ppm, denominator,
                                                   rec.data(), nullptr));
            for (const sbwtgpu_pseudoalignment &p : rec) {
                append_int(total_reads++, text);
                append_set_bits(&p.colors, 1, " ", " ", text);
                text.push_back('\n');
            }
        }
        writer.write(text.data(), (int64_t)text.size());
    });
    write_log("us/read end-to-end: " + std::to_string((double)(cur_time_micros() - micros_start) / (double)std::max<int64_t>(1, total_reads)),
              LogLevel::MAJOR);
    return 0;
}

// the subcommands, in the order "Available commands" lists them
struct Command { const char *name; int (*main)(int, char **); };
const Command commands[] = {
    {"build", build_main},
    {"search", search_main},
    {"matching-statistics", matching_statistics_main},
    {"dump-unitigs", dump_unitigs_main},
    {"thread", thread_main},
    {"bubbles", bubbles_main},
    {"set-op", set_op_main},
    {"read-hits", read_hits_main},
    {"build-colors", build_colors_main},
    {"compress-colors", compress_colors_main},
    {"merge-colors", merge_colors_main},
    {"color-matrix", color_matrix_main},
    {"color-select", color_select_main},
    {"screen", screen_main},
    {"pseudoalign", pseudoalign_main},
};

void print_help(char **argv) {
    std::cerr << "Available commands: " << std::endl;
    for (const Command &c : commands) std::cerr << "   " << argv[0] << " " << c.name << std::endl;
    std::cerr << "Running a command without arguments prints the usage instructions for the command." << std::endl;
}

}  // namespace

int main(int argc, char **argv) {   // sbwt.cpp:19-57
    // the reference logs its compile-time MAX_KMER_LENGTH here (sbwt.cpp:25); this build handles any k <= 255
    write_log("Maximum k-mer length is set to 255", LogLevel::MAJOR);
    if (argc == 1) { print_help(argv); return 0; }
    string command = argv[1];
    if (command == "--help" || command == "-h") { print_help(argv); return 0; }
    for (int i = 1; i < argc; i++) argv[i - 1] = argv[i];
    argc--;
    try {
        for (const Command &c : commands) {
            if (command != c.name) continue;
            const int rc = c.main(argc, argv);
            if (c.main == search_main) {
                // every output file is closed: leave without the HIP runtime's teardown and the freeing of the index (a tenth
                // of a second of a sub-second run)
                std::cout.flush();
                std::cerr.flush();
                fflush(nullptr);
                _exit(rc);
            }
            return rc;
        }
        throw std::runtime_error("Invalid command: " + command);
    } catch (const std::runtime_error &e) {
        std::cerr << "Runtime error: " << e.what() << '\n';
        return 1;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << '\n';
        return 1;
    }
}
