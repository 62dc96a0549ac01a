// kmc_cli.cpp -- `k-mer-count`: the reference's process boundary, kept.
//
// Reference: k-mer-count/src/main.rs:43-91 takes no arguments, opens "sample.fasta" in the
// cwd (main.rs:44) and prints one sorted 54-character line per occurrence (main.rs:88-90);
// test.py:15-18 takes the FASTA path as its only positional argument.  This tool keeps both:
//
//   k-mer-count [FASTA] [-k K] [--forward] [--expand] [--device N | --gpus N] [--algo auto|stream|walk|sort] [--stats]
//               [--min-count N] [--max-count N] [--histo H] [--query-kmers FILE | --profile FILE | --map FILE | --correct FILE]
//               [--transits FILE [--min-reads N]] [--contigs FILE [--min-reads N] [--min-support N]]
//               [--pairs FILE [--insert-bins N]]
//               [--trim FILE [--trim-mode none|ends|longest] [--min-strong N] [--strong-permille N] [--min-len N] [--invert]
//                [--paired both|either]]
//               [--normalize FILE --target N [--depth-permille P] [--min-depth N] [--seed S] [--norm-paired] [--norm-invert]]
//               [--with FASTA2 (--compare | --setop intersect|union|subtract [--counts left|right|min|max|sum|diff])]
//               [--graph | --graph-stats | --unitigs | --gfa | --components | --variants [--bubble-keys N]]
//               [--clean ROUNDS [--tip-keys N] [--island-keys N] [--bubble-keys N]] [--component-keys N]
//
//   --gpus N  the file's chunks go round-robin to GPUs 0..N-1 of this process, tables reduced on GPU 0
//             (there is no CPU backend: SURVEY.md's "--backend cpu" is deliberately absent)
//
//   no -k   reference mode: LR-gapped 27+gap+27 for sizes 80..=140, expanded sorted output,
//           byte-identical to main.rs:87-90
//   -k K    count-table mode: contiguous canonical K-mers, "KMER<TAB>COUNT" lines sorted by KMER
//
//   --min-count N / --max-count N   only keys seen N times or more / at most N times (table mode: the lines printed;
//                                   reference mode: the keys expanded).  Additions: the reference has no such option.
//   --histo H   instead of the table, the abundance histogram: "COUNT<TAB>KEYS" lines, ascending, non-zero only; the line
//               for H counts the keys seen H times or more.  The count filters apply to it too.
//
//   --query-kmers FILE   (with -k K) instead of the table: for every line of FILE, a K-mer, "KMER<TAB>COUNT" in input order --
//               the k-mer as given, looked up canonically unless --forward; 0 for a k-mer the input does not hold
//   --profile FILE       (with -k K) instead of the table: for every read of FILE (FASTA / FASTQ), in file order,
//               "INDEX<TAB>WINDOWS<TAB>PRESENT<TAB>MIN<TAB>MAX<TAB>SUM": its valid K-mer windows, how many of them the
//               counted input holds --min-count times or more, and the smallest / largest / summed count over them
//   --map FILE           (with -k K) instead of the table: every read of FILE (FASTA / FASTQ) threaded through the unitigs of the
//               counted input (kmc_unitig_map; --min-count / --max-count are the solidity range), in file order
//               "INDEX<TAB>WINDOWS<TAB>PLACED<TAB>SEGMENTS<TAB>WALK": its valid K-mer windows, how many of them lie on a unitig, the
//               number of segments, and the segments as ">U:POS:LEN" (read along unitig U from key position POS, LEN windows) or
//               "<U:POS:LEN" (against it).  A segment that starts at the window right behind its predecessor -- the read crossed
//               from one unitig end to another -- is written directly behind it, one behind a gap after a ","; "*" for a read
//               with no segment.  With --clean the reads are laid on the cleaned graph.
//   --transits FILE      (with -k K) instead of the table: the walks of the reads of FILE (FASTA / FASTQ) through the unitig graph of
//               the counted input, counted per graph element (kmc_unitig_transits; --min-count / --max-count are the solidity
//               range).  First "L<TAB>END<TAB>TO<TAB>SUPPORT" per link record that a read walked, in array order: the unitig end
//               2 * U + (0 START | 1 END) it leaves, the end it reaches, the reads that stepped across in either direction.
//               Then per unitig with two or more links at both ends "U<TAB>UNITIG<TAB>VERDICT<TAB>DS<TAB>DE" -- unspanned, resolved
//               or ambiguous under --min-reads N (default 1: the reads a way through must have to count), the links at its START
//               and END end -- followed by "T<TAB>UNITIG<TAB>P<TAB>Q<TAB>COUNT" per pair of the P-th START link and the Q-th END
//               link that COUNT reads took through it.  It excludes what --map excludes, and --map; with --clean the reads
//               walk the cleaned graph.
//   --contigs FILE       (with -k K) instead of the table: the contigs the reads of FILE (FASTA / FASTQ) leave of the unitig graph of
//               the counted input (kmc_unitig_contigs behind kmc_unitig_transits, which walks FILE in chunks that add up;
//               --min-count / --max-count are the solidity range).  A repeat whose ways in pair up one to one with its ways out,
//               each pair walked by --min-reads N reads or more (default 1), gets one copy per pair; with --min-support N
//               (default 0) a link that fewer than N reads walked is ignored at the ends of the other unitigs.  Output: FASTA,
//               ">INDEX LN:i:BASES KC:i:ABUND CL:i:0|1 WK:Z:WALK" -- the abundance summed over the path, the circular flag, the
//               path as ">U" / "<U" per unitig -- then the contig on one line.  It excludes what --transits excludes, and
//               --transits; with --clean the reads walk the cleaned graph.
//   --pairs FILE         (with -k K) instead of the table: the pair evidence of the reads of FILE (FASTA / FASTQ, mates adjacent as
//               --paired takes them, forward / reverse) on the unitig graph of the counted input (kmc_unitig_pairs, which takes
//               FILE in chunks that add up; --min-count / --max-count are the solidity range).  Output, tab-separated: "I F
//               PAIRS" for every insert size F that pairs lying on one unitig have (--insert-bins N bins, default 1024, the last
//               one open), then "P A B COUNT SUM MIN MAX" per pair of unitig ends A < B that pairs connect -- how many, and the
//               sum, least and most of the bases they span up to those ends.  It excludes what --transits excludes, --transits
//               and --contigs; with --clean the pairs lie on the cleaned graph.
//   --correct FILE       (with -k K) instead of the table: every read of FILE (FASTA / FASTQ) corrected against the solid keys of
//               the counted input (kmc_correct; --min-count / --max-count are the solidity range), as FASTA in file order:
//               ">INDEX WINDOWS WEAK CANDIDATES FIXED" -- its valid K-mer windows, how many of them are not solid, the weak
//               runs that qualify as one substitution, how many of those were repaired -- then the corrected read on one
//               line.  With --clean the reads are corrected against the cleaned table.
//   --trim FILE          (with -k K) instead of the table: every read of FILE (FASTA / FASTQ) judged by its strong windows -- those
//               whose key the counted input holds within --min-count / --max-count -- and cut down to the span the table
//               supports (kmc_trim).  --trim-mode: none keeps a read whole, ends cuts it from its first to its last strong
//               window, longest (the default) to its longest run of strong windows.  A read passes with --min-strong N
//               strong windows or more, --strong-permille N thousandths or more of its valid windows strong, and a span of
//               --min-len N bases or more (default 0 each; a trimming mode also asks for one strong window).  --paired
//               both|either: reads 2i and 2i + 1 are mates and stay or go together, if both / either of them pass.
//               --invert (with --trim-mode none) prints the reads that fail instead.  Output: FASTA in file order, the
//               emitted reads only: ">INDEX WINDOWS STRONG START LEN" -- the read's number in FILE, its valid and its strong
//               windows, the span's start and length in bases -- then the span on one line.  It excludes --query-kmers /
//               --profile / --map / --correct; with --clean the reads are judged against the cleaned table.
//   --normalize FILE     (with -k K) instead of the table: every read of FILE (FASTA / FASTQ) gets a depth -- the count at
//               --depth-permille P thousandths (default 500, the lower median) of the sorted counts of its valid windows in
//               the counted input -- and the reads are normalised by it (kmc_normalize): a read shallower than --min-depth N
//               (default 0) is dropped, a read deeper than --target N is kept with probability N / depth, decided by a draw
//               from --seed S (default 0) and the read's number, so a run repeats exactly; --target 0 samples nothing down.
//               --norm-paired: reads 2i and 2i + 1 are mates, judged together by the smaller depth.  --norm-invert prints the
//               reads that go instead.  Output: FASTA in file order, the emitted reads only: ">INDEX WINDOWS DEPTH UNITDEPTH"
//               -- the read's number in FILE, its valid windows, its own depth, the depth it was judged by -- then the read on
//               one line.  It excludes --query-kmers / --profile / --map / --correct / --trim and --with; with --clean the
//               reads are judged against the cleaned table.
//
//   --with FASTA2        (with -k K) a second file, counted into a second table on the same device; one of:
//     --compare          instead of the table: "NAME<TAB>VALUE" lines -- the eight words of kmc_compare (n_a, n_b, n_both, sum_a,
//               sum_b, shared_sum_a, shared_sum_b, sum_min), then union, jaccard, containment_a, containment_b,
//               weighted_jaccard, bray_curtis (six decimals)
//     --setop OP         instead of the table: "KMER<TAB>COUNT" of FASTA OP FASTA2, the count chosen by --counts (default left)
//               --min-count / --max-count are then the range applied to the counts of BOTH inputs
//
//   --graph              (with -k K) instead of the table: the table as a de Bruijn graph.  For every solid key -- count within
//               --min-count / --max-count -- in key order "KMER<TAB>COUNT<TAB>R<TAB>L<TAB>ENDS": R / L the bases (in ACGT order, "."
//               for none) that extend the key to the right / left into another solid key, ENDS the sides at which a unitig
//               ends: ".", "R", "L" or "LR"
//   --graph-stats        (with -k K) instead of the table: "NAME<TAB>VALUE" lines -- the eight words of kmc_graph (nodes,
//               right_degrees, left_degrees, isolated, dead_ends, branching, end_sides, single_node_unitigs), then unitigs
//   --unitigs            (with -k K) instead of the table: the unitigs of that graph (kmc_unitigs) as FASTA, one record per unitig
//               in order: ">INDEX LN:i:BASES KC:i:ABUND CL:i:0|1" (ABUND the summed count of its keys, CL 1 for a circular
//               one), then the sequence on one line.  --min-count / --max-count are the solidity range.
//   --gfa                (with -k K) instead of the table: those unitigs and the links between them (kmc_unitig_links) as GFA 1.0,
//               tab-separated: "H VN:Z:1.0", then per unitig in order "S INDEX SEQ LN:i:BASES KC:i:ABUND CL:i:0|1", then per link
//               record in array order "L U +|- V +|- (K-1)M" (every link appears from both of its ends).  Same solidity range.
//
//   --clean ROUNDS       (with -k K) before whichever output was asked for -- the table, --histo, --graph*, --unitigs, --gfa -- the
//               table is cleaned: up to ROUNDS times the unitigs of the solidity range are judged (kmc_unitig_clean_into), dead-end
//               arms of at most --tip-keys keys that lose against a sibling and unconnected unitigs of at most --island-keys keys
//               (default K each, 0: none) are taken out, and the keys of the others become the table of the next round and in the
//               end of the output (--query-kmers / --profile ask the cleaned table too).  A round that removes nothing is the last.
//               With --stats one line per round on stderr; the closing --stats line still describes the counting of the file.
//   --bubble-keys N      (with --clean ROUNDS) every round also pops simple bubbles (kmc_unitig_simplify_into): a unitig of at
//               most N keys with one link at each end that loses against a parallel unitig between the same two ends (0: none).
//               Without the option nothing is popped.  The per-round --stats line gains "bubbles B bubble_keys K
//               bubble_candidates C"; a round that removes nothing, bubbles included, is the last.
//
//   --components         (with -k K) instead of the table: the connected components of the unitig graph (kmc_unitig_components), one
//               line per component in order "COMPONENT<TAB>ROOT<TAB>UNITIGS<TAB>KEYS<TAB>ABUND": its number, its smallest unitig, how many
//               unitigs and keys it has and the summed count of its keys.  Same solidity range.
//   --component-keys N   (with -k K) after any --clean rounds and before whichever output was asked for, the connected components
//               of at most N keys are taken out of the table (kmc_unitig_components_into, one step; 0: none).  It needs no
//               --clean.  With --stats one line on stderr.
//   --variants           (with -k K) instead of the table: the bubbles of the unitig graph as variant calls (kmc_unitig_bubbles), one line
//               per unitig that loses against a parallel unitig between the same two ends, in unitig order
//               "INDEX<TAB>KIND<TAB>U<TAB>W<TAB>POS<TAB>ALT<TAB>MAJOR<TAB>A_U/M_U<TAB>A_W/M_W": the record's number, S (one substitution), I (an
//               insertion or deletion: one allele empty) or C (anything else), the losing unitig U and the one it lost against W,
//               the length POS of the common prefix of the two arms (W read in U's direction), what is left of U and of W between
//               common prefix and common suffix ("-" for nothing), and the abundance / keys of the two arms.  --bubble-keys N is
//               here the most keys an arm may have (default K; it needs no --clean, and with --variants the --clean rounds pop no
//               bubbles: they would remove what is to be reported).  --min-count / --max-count are the solidity range.
//
// Errors: message on stderr, exit code 101 (what a Rust panic exits with), never partial stdout.
#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kmc.h"

static int die(const char* what, const char* msg) {
    fprintf(stderr, "k-mer-count: %s: %s\n", what, msg);
    return 101;
}

// a whole decimal number in [lo, hi], or exit code 2 (atoi turned "-k abc" and "-k 0" into the
// reference's LR mode and printed 195 MB instead of an error)
static bool parse_int(const char* opt, const char* text, long lo, long hi, int* out) {
    char* end = nullptr;
    errno = 0;
    const long v = strtol(text, &end, 10);
    if (errno || end == text || *end != '\0' || v < lo || v > hi) {
        fprintf(stderr, "k-mer-count: %s needs a whole number in %ld..%ld (got '%s')\n", opt, lo, hi, text);
        return false;
    }
    *out = (int)v;
    return true;
}

// the same for a 64-bit count (--min-count / --max-count)
static bool parse_count(const char* opt, const char* text, long long lo, long long hi, long long* out) {
    char* end = nullptr;
    errno = 0;
    const long long v = strtoll(text, &end, 10);
    if (errno || end == text || *end != '\0' || v < lo || v > hi) {
        fprintf(stderr, "k-mer-count: %s needs a whole number in %lld..%lld (got '%s')\n", opt, lo, hi, text);
        return false;
    }
    *out = v;
    return true;
}

int main(int argc, char** argv) {
    const char* path = "sample.fasta";  // main.rs:44
    int k = 0, canonical = 1, expand = 0, device = 0, algo = KMC_ALGO_AUTO, stats = 0, gpus = 1, histo = 0;
    long long min_count = 1, max_count = 0;   // (max_count 0: no upper bound)
    const char *query_path = nullptr, *profile_path = nullptr, *with_path = nullptr, *map_path = nullptr, *correct_path = nullptr;
    const char* trim_path = nullptr;
    const char* transits_path = nullptr;
    long long min_reads = -1;   // (-1: not given)
    const char* contigs_path = nullptr;
    const char* pairs_path = nullptr;
    long long insert_bins = -1;   // (-1: not given)
    long long min_support = -1;   // (-1: not given)
    int trim_mode = -1, trim_invert = 0, trim_pair = 0;   // (-1: the default mode, longest)
    long long min_strong = -1, strong_permille = -1, min_len = -1;   // (-1: not given)
    const char* norm_path = nullptr;
    int norm_paired = 0, norm_invert = 0;
    long long norm_target = -1, depth_permille = -1, min_depth = -1, norm_seed = -1;   // (-1: not given)
    int compare = 0, setop = -1, count_mode = -1, graph = 0, graph_stats = 0, unitigs = 0, gfa = 0;
    int clean = 0;
    long long tip_keys = -1, island_keys = -1;   // (-1: K)
    long long bubble_keys = -1;                  // (-1: no bubble is popped, the rounds are kmc_unitig_clean_into's)
    int components = 0, variants = 0;
    long long component_keys = -1;               // (-1: no component step)
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-k" && i + 1 < argc) { if (!parse_int("-k", argv[++i], 1, 63, &k)) return 2; }
        else if (a == "--forward") canonical = 0;
        else if (a == "--expand") expand = 1;
        else if (a == "--stats") stats = 1;
        else if (a == "--device" && i + 1 < argc) { if (!parse_int("--device", argv[++i], 0, 1023, &device)) return 2; }
        else if (a == "--gpus" && i + 1 < argc) { if (!parse_int("--gpus", argv[++i], 1, 64, &gpus)) return 2; }
        else if (a == "--min-count" && i + 1 < argc) { if (!parse_count("--min-count", argv[++i], 1, LLONG_MAX, &min_count)) return 2; }
        else if (a == "--max-count" && i + 1 < argc) { if (!parse_count("--max-count", argv[++i], 1, LLONG_MAX, &max_count)) return 2; }
        else if (a == "--histo" && i + 1 < argc) { if (!parse_int("--histo", argv[++i], 1, (1 << 24) - 1, &histo)) return 2; }
        else if (a == "--query-kmers" && i + 1 < argc) query_path = argv[++i];
        else if (a == "--profile" && i + 1 < argc) profile_path = argv[++i];
        else if (a == "--map" && i + 1 < argc) map_path = argv[++i];
        else if (a == "--correct" && i + 1 < argc) correct_path = argv[++i];
        else if (a == "--transits" && i + 1 < argc) transits_path = argv[++i];
        else if (a == "--contigs" && i + 1 < argc) contigs_path = argv[++i];
        else if (a == "--pairs" && i + 1 < argc) pairs_path = argv[++i];
        else if (a == "--insert-bins" && i + 1 < argc) { if (!parse_count("--insert-bins", argv[++i], 2, 1 << 20, &insert_bins)) return 2; }
        else if (a == "--min-support" && i + 1 < argc) { if (!parse_count("--min-support", argv[++i], 0, LLONG_MAX, &min_support)) return 2; }
        else if (a == "--min-reads" && i + 1 < argc) { if (!parse_count("--min-reads", argv[++i], 0, LLONG_MAX, &min_reads)) return 2; }
        else if (a == "--trim" && i + 1 < argc) trim_path = argv[++i];
        else if (a == "--trim-mode" && i + 1 < argc) {
            std::string v = argv[++i];
            trim_mode = v == "none" ? KMC_TRIM_NONE : v == "ends" ? KMC_TRIM_ENDS : v == "longest" ? KMC_TRIM_LONGEST : -1;
            if (trim_mode < 0) { fprintf(stderr, "k-mer-count: --trim-mode needs none, ends or longest (got '%s')\n", v.c_str()); return 2; }
        } else if (a == "--min-strong" && i + 1 < argc) { if (!parse_count("--min-strong", argv[++i], 0, LLONG_MAX, &min_strong)) return 2; }
        else if (a == "--strong-permille" && i + 1 < argc) { if (!parse_count("--strong-permille", argv[++i], 0, 1000, &strong_permille)) return 2; }
        else if (a == "--min-len" && i + 1 < argc) { if (!parse_count("--min-len", argv[++i], 0, LLONG_MAX, &min_len)) return 2; }
        else if (a == "--invert") trim_invert = 1;
        else if (a == "--paired" && i + 1 < argc) {
            std::string v = argv[++i];
            const int p = v == "both" ? (int)KMC_TRIM_PAIR_BOTH : v == "either" ? (int)KMC_TRIM_PAIR_EITHER : 0;
            if (!p) { fprintf(stderr, "k-mer-count: --paired needs both or either (got '%s')\n", v.c_str()); return 2; }
            if (trim_pair && trim_pair != p) { fprintf(stderr, "k-mer-count: --paired both and --paired either exclude each other\n"); return 2; }
            trim_pair = p;
        }
        else if (a == "--normalize" && i + 1 < argc) norm_path = argv[++i];
        else if (a == "--target" && i + 1 < argc) { if (!parse_count("--target", argv[++i], 0, LLONG_MAX, &norm_target)) return 2; }
        else if (a == "--depth-permille" && i + 1 < argc) { if (!parse_count("--depth-permille", argv[++i], 0, 1000, &depth_permille)) return 2; }
        else if (a == "--min-depth" && i + 1 < argc) { if (!parse_count("--min-depth", argv[++i], 0, LLONG_MAX, &min_depth)) return 2; }
        else if (a == "--seed" && i + 1 < argc) { if (!parse_count("--seed", argv[++i], 0, LLONG_MAX, &norm_seed)) return 2; }
        else if (a == "--norm-paired") norm_paired = 1;
        else if (a == "--norm-invert") norm_invert = 1;
        else if (a == "--with" && i + 1 < argc) with_path = argv[++i];
        else if (a == "--compare") compare = 1;
        else if (a == "--graph") graph = 1;
        else if (a == "--graph-stats") graph_stats = 1;
        else if (a == "--unitigs") unitigs = 1;
        else if (a == "--gfa") gfa = 1;
        else if (a == "--components") components = 1;
        else if (a == "--variants") variants = 1;
        else if (a == "--component-keys" && i + 1 < argc) { if (!parse_count("--component-keys", argv[++i], 0, LLONG_MAX, &component_keys)) return 2; }
        else if (a == "--clean" && i + 1 < argc) { if (!parse_int("--clean", argv[++i], 1, 1000, &clean)) return 2; }
        else if (a == "--tip-keys" && i + 1 < argc) { if (!parse_count("--tip-keys", argv[++i], 0, LLONG_MAX, &tip_keys)) return 2; }
        else if (a == "--island-keys" && i + 1 < argc) { if (!parse_count("--island-keys", argv[++i], 0, LLONG_MAX, &island_keys)) return 2; }
        else if (a == "--bubble-keys" && i + 1 < argc) { if (!parse_count("--bubble-keys", argv[++i], 0, LLONG_MAX, &bubble_keys)) return 2; }
        else if (a == "--setop" && i + 1 < argc) {
            std::string v = argv[++i];
            setop = v == "intersect" ? KMC_SETOP_INTERSECT : v == "union" ? KMC_SETOP_UNION : v == "subtract" ? KMC_SETOP_SUBTRACT : -1;
            if (setop < 0) { fprintf(stderr, "k-mer-count: --setop needs intersect, union or subtract (got '%s')\n", v.c_str()); return 2; }
        } else if (a == "--counts" && i + 1 < argc) {
            std::string v = argv[++i];
            count_mode = v == "left" ? KMC_COUNT_LEFT : v == "right" ? KMC_COUNT_RIGHT : v == "min" ? KMC_COUNT_MIN : v == "max" ? KMC_COUNT_MAX
                         : v == "sum" ? KMC_COUNT_SUM : v == "diff" ? KMC_COUNT_DIFF : -1;
            if (count_mode < 0) { fprintf(stderr, "k-mer-count: --counts needs left, right, min, max, sum or diff (got '%s')\n", v.c_str()); return 2; }
        } else if (a == "--algo" && i + 1 < argc) {
            std::string v = argv[++i];
            algo = v == "stream" ? KMC_ALGO_STREAM : v == "walk" ? KMC_ALGO_WALK : v == "sort" ? KMC_ALGO_SORT : KMC_ALGO_AUTO;
        } else if (a == "-h" || a == "--help") {
            fprintf(stderr, "usage: k-mer-count [FASTA] [-k K] [--forward] [--expand] [--device N | --gpus N] [--algo auto|stream|walk|sort] [--stats]\n"
                            "                   [--min-count N] [--max-count N] [--histo H] [--query-kmers FILE | --profile FILE | --map FILE | --correct FILE]\n"
                            "                   [--transits FILE [--min-reads N]] [--contigs FILE [--min-reads N] [--min-support N]]\n"
                            "                   [--pairs FILE [--insert-bins N]]\n"
                            "                   [--trim FILE [--trim-mode none|ends|longest] [--min-strong N] [--strong-permille N] [--min-len N] [--invert]\n"
                            "                    [--paired both|either]]\n"
                            "                   [--normalize FILE --target N [--depth-permille P] [--min-depth N] [--seed S] [--norm-paired] [--norm-invert]]\n"
                            "                   [--with FASTA2 (--compare | --setop intersect|union|subtract [--counts left|right|min|max|sum|diff])]\n"
                            "                   [--graph | --graph-stats | --unitigs | --gfa | --components | --variants [--bubble-keys N]]\n"
                            "                   [--clean ROUNDS [--tip-keys N] [--island-keys N] [--bubble-keys N]] [--component-keys N]\n");
            return 0;
        } else if (a == "-k" || a == "--device" || a == "--gpus" || a == "--algo" || a == "--min-count" || a == "--max-count" || a == "--histo" ||
                   a == "--query-kmers" || a == "--profile" || a == "--map" || a == "--correct" || a == "--with" || a == "--setop" || a == "--counts" ||
                   a == "--clean" || a == "--tip-keys" || a == "--island-keys" || a == "--bubble-keys" || a == "--component-keys" || a == "--trim" ||
                   a == "--trim-mode" || a == "--min-strong" || a == "--strong-permille" || a == "--min-len" || a == "--paired" ||
                   a == "--normalize" || a == "--target" || a == "--depth-permille" || a == "--min-depth" || a == "--seed" || a == "--transits" ||
                   a == "--min-reads" || a == "--contigs" || a == "--min-support" || a == "--pairs" || a == "--insert-bins") {
            fprintf(stderr, "k-mer-count: %s needs a value\n", a.c_str());
            return 2;
        } else if (!a.empty() && a[0] != '-') path = argv[i];
        else { fprintf(stderr, "k-mer-count: unknown option %s\n", a.c_str()); return 2; }
    }
    if (max_count && min_count > max_count) {
        fprintf(stderr, "k-mer-count: --min-count %lld is above --max-count %lld\n", min_count, max_count);
        return 2;
    }
    // --query-kmers / --profile: everything that can be wrong with them is found before a GPU is touched
    std::vector<std::string> q_text;
    std::vector<uint64_t> q_hi, q_lo;
    kmc_reads prof;
    memset(&prof, 0, sizeof(prof));
    if (query_path || profile_path) {
        const char* opt = query_path ? "--query-kmers" : "--profile";
        if (query_path && profile_path) { fprintf(stderr, "k-mer-count: --query-kmers and --profile exclude each other\n"); return 2; }
        if (!k) { fprintf(stderr, "k-mer-count: %s needs -k K\n", opt); return 2; }
        if (histo) { fprintf(stderr, "k-mer-count: %s and --histo exclude each other\n", opt); return 2; }
    }
    // --map: the same (it shares the parsed reads with --profile, which it excludes)
    if (map_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa) bad = "--graph / --graph-stats / --unitigs / --gfa exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --map %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    }
    // --transits and its option: the same again
    if (transits_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (map_path || correct_path || trim_path || norm_path) bad = "--map / --correct / --trim / --normalize exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa || components || variants)
            bad = "--graph / --graph-stats / --unitigs / --gfa / --components / --variants exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --transits %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    } else if (min_reads >= 0 && !contigs_path) {
        fprintf(stderr, "k-mer-count: --min-reads needs --transits FILE or --contigs FILE\n");
        return 2;
    }
    // --contigs and its options: the same again
    if (contigs_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (transits_path || map_path || correct_path || trim_path || norm_path) bad = "--transits / --map / --correct / --trim / --normalize exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa || components || variants)
            bad = "--graph / --graph-stats / --unitigs / --gfa / --components / --variants exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --contigs %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    } else if (min_support >= 0) {
        fprintf(stderr, "k-mer-count: --min-support needs --contigs FILE\n");
        return 2;
    }
    // --pairs and its option: the same again
    if (pairs_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (transits_path || contigs_path || map_path || correct_path || trim_path || norm_path)
            bad = "--transits / --contigs / --map / --correct / --trim / --normalize exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa || components || variants)
            bad = "--graph / --graph-stats / --unitigs / --gfa / --components / --variants exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --pairs %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    } else if (insert_bins >= 0) {
        fprintf(stderr, "k-mer-count: --insert-bins needs --pairs FILE\n");
        return 2;
    }
    // --correct: the same again
    if (correct_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (map_path) bad = "--map exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa) bad = "--graph / --graph-stats / --unitigs / --gfa exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --correct %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    }
    // --trim and its options: the same again
    if (trim_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (map_path || correct_path) bad = "--map / --correct exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa) bad = "--graph / --graph-stats / --unitigs / --gfa exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --trim %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
        if (trim_mode < 0) trim_mode = KMC_TRIM_LONGEST;
        if (trim_invert && trim_mode != KMC_TRIM_NONE) { fprintf(stderr, "k-mer-count: --invert needs --trim-mode none\n"); return 2; }
    } else if (trim_mode >= 0 || trim_invert || trim_pair || min_strong >= 0 || strong_permille >= 0 || min_len >= 0) {
        fprintf(stderr, "k-mer-count: --trim-mode / --min-strong / --strong-permille / --min-len / --invert / --paired need --trim FILE\n");
        return 2;
    }
    // --normalize and its options: the same again
    if (norm_path) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (norm_target < 0) bad = "needs --target N";
        else if (map_path || correct_path || trim_path) bad = "--map / --correct / --trim exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (graph || graph_stats || unitigs || gfa) bad = "--graph / --graph-stats / --unitigs / --gfa exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --normalize %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    } else if (norm_target >= 0 || depth_permille >= 0 || min_depth >= 0 || norm_seed >= 0 || norm_paired || norm_invert) {
        fprintf(stderr, "k-mer-count: --target / --depth-permille / --min-depth / --seed / --norm-paired / --norm-invert need --normalize FILE\n");
        return 2;
    }
    if (query_path) {
        FILE* f = fopen(query_path, "r");
        if (!f) return die(query_path, strerror(errno));
        char buf[256];
        unsigned long long line_no = 0;
        while (fgets(buf, sizeof(buf), f)) {
            ++line_no;
            size_t len = strlen(buf);
            const bool whole = len && buf[len - 1] == '\n';
            while (len && (buf[len - 1] == '\n' || buf[len - 1] == '\r')) buf[--len] = '\0';
            uint64_t h = 0, l = 0;
            const int erc = (len == (size_t)k && (whole || feof(f))) ? kmc_encode_key(buf, k, canonical, &h, &l) : KMC_ERR_ARG;
            if (erc) {
                fprintf(stderr, "k-mer-count: --query-kmers %s line %llu: %s\n", query_path, line_no,
                        erc == KMC_ERR_ALPHABET ? "a character outside ACGT" : "not a k-mer of length K");
                fclose(f);
                return 2;
            }
            q_text.emplace_back(buf, len);
            q_hi.push_back(h);
            q_lo.push_back(l);
        }
        fclose(f);
    }
    if (profile_path || map_path || correct_path || trim_path || norm_path || transits_path || contigs_path || pairs_path) {
        const char* reads_path = profile_path ? profile_path : map_path ? map_path : correct_path ? correct_path : trim_path ? trim_path : norm_path ? norm_path
                                 : transits_path ? transits_path : contigs_path ? contigs_path : pairs_path;
        char eb[256] = {0};
        const int prc = kmc_parse_fasta(reads_path, &prof, eb, sizeof(eb));
        if (prc) return die(reads_path, eb[0] ? eb : kmc_status_string(prc));
    }
    // --with / --compare / --setop: bad combinations end here, before a GPU is touched
    {
        const bool action = compare || setop >= 0;
        const char* bad = nullptr;
        if (with_path && !action) bad = "--with needs --compare or --setop";
        else if (action && !with_path) bad = "--compare / --setop need --with FASTA2";
        else if (compare && setop >= 0) bad = "--compare and --setop exclude each other";
        else if (count_mode >= 0 && setop < 0) bad = "--counts needs --setop";
        else if (with_path && !k) bad = "--with needs -k K";
        else if (with_path && (histo || query_path || profile_path)) bad = "--with and --histo / --query-kmers / --profile exclude each other";
        else if (with_path && map_path) bad = "--with and --map exclude each other";
        else if (with_path && trim_path) bad = "--with and --trim exclude each other";
        else if (with_path && gpus != 1) bad = "--with and --gpus exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: %s\n", bad); return 2; }
    }
    // --graph / --graph-stats / --unitigs / --gfa: the same
    if (graph || graph_stats || unitigs || gfa) {
        const char* opt = graph ? "--graph" : graph_stats ? "--graph-stats" : unitigs ? "--unitigs" : "--gfa";
        const char* bad = nullptr;
        if (graph && graph_stats) bad = "--graph-stats exclude each other";
        else if ((graph || graph_stats) && unitigs) bad = "--unitigs exclude each other";
        else if ((graph || graph_stats || unitigs) && gfa) bad = "--gfa exclude each other";
        else if (!k) bad = "needs -k K";
        else if (histo) bad = "--histo exclude each other";
        else if (query_path || profile_path) bad = "--query-kmers / --profile exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: %s %s%s\n", opt, strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    }
    // --clean / --tip-keys / --island-keys / --bubble-keys: the same
    if (clean || tip_keys >= 0 || island_keys >= 0 || bubble_keys >= 0) {
        const char* bad = nullptr;
        if (!clean && !(variants && tip_keys < 0 && island_keys < 0)) bad = "--tip-keys / --island-keys / --bubble-keys need --clean ROUNDS";
        else if (!k) bad = "--clean needs -k K";
        else if (with_path || compare || setop >= 0) bad = "--clean and --with / --compare / --setop exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: %s\n", bad); return 2; }
    }
    // --components / --component-keys: the same
    if (components) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (graph || graph_stats || unitigs || gfa) bad = "--graph / --graph-stats / --unitigs / --gfa exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (query_path || profile_path || map_path || correct_path || trim_path || norm_path || transits_path || contigs_path || pairs_path)
            bad = "--query-kmers / --profile / --map / --correct / --trim / --normalize / --transits / --contigs / --pairs exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --components %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
    }
    // --variants: the same
    if (variants) {
        const char* bad = nullptr;
        if (!k) bad = "needs -k K";
        else if (graph || graph_stats || unitigs || gfa || components) bad = "--graph / --graph-stats / --unitigs / --gfa / --components exclude each other";
        else if (histo) bad = "--histo exclude each other";
        else if (query_path || profile_path || map_path || correct_path || trim_path || norm_path || transits_path || contigs_path || pairs_path)
            bad = "--query-kmers / --profile / --map / --correct / --trim / --normalize / --transits / --contigs / --pairs exclude each other";
        else if (with_path || compare || setop >= 0) bad = "--with / --compare / --setop exclude each other";
        else if (expand) bad = "--expand exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: --variants %s%s\n", strncmp(bad, "needs", 5) ? "and " : "", bad); return 2; }
        if (bubble_keys >= (1ll << 31)) { fprintf(stderr, "k-mer-count: --variants needs --bubble-keys below 2^31 (got %lld)\n", bubble_keys); return 2; }
    }
    if (component_keys >= 0) {
        const char* bad = nullptr;
        if (!k) bad = "--component-keys needs -k K";
        else if (with_path || compare || setop >= 0) bad = "--component-keys and --with / --compare / --setop exclude each other";
        if (bad) { fprintf(stderr, "k-mer-count: %s\n", bad); return 2; }
    }
    const bool filtered = min_count > 1 || max_count != 0;
    kmc_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    cfg.mode = k ? KMC_MODE_CONTIG : KMC_MODE_LR;
    cfg.k = k ? k : 54;
    cfg.canonical = canonical;
    cfg.device = device;
    cfg.algo = algo;
    if (!k) expand = 1;
    if (gpus < 1 || gpus > 64) { fprintf(stderr, "k-mer-count: --gpus must be 1..64\n"); return 2; }
    // KMC_CLI_SHARE_DEVICE=D (testing on a box with fewer GPUs): all --gpus contexts live on device D
    const char* share = getenv("KMC_CLI_SHARE_DEVICE");
    std::vector<kmc_ctx*> ctxs;
    int rc = 0;
    for (int g = 0; g < gpus && !rc; ++g) {
        cfg.device = gpus == 1 ? device : (share ? atoi(share) : g);
        kmc_ctx* one = nullptr;
        rc = kmc_create(&one, &cfg);
        if (!rc) ctxs.push_back(one);
    }
    auto destroy_all = [&]() { for (kmc_ctx* x : ctxs) kmc_destroy(x); };
    if (rc) { int r = die("kmc_create", kmc_last_error(nullptr)); destroy_all(); return r; }
    kmc_ctx* ctx = ctxs[0];
    kmc_ctx* const counted = ctx;   // (the ctx that read the file: --clean moves ctx on to the cleaned table)
    uint64_t nd = 0, nt = 0;
    rc = gpus == 1 ? kmc_count_file(ctx, path, &nd, &nt) : kmc_count_file_multi(ctxs.data(), (uint32_t)ctxs.size(), path, &nd, &nt);
    if (rc) { int r = die(path, kmc_last_error(ctx)); destroy_all(); return r; }
    // --clean: round by round into a fresh ctx, which then is the table every output below reads
    for (int round = 1; round <= clean; ++round) {
        cfg.device = gpus == 1 ? device : (share ? atoi(share) : 0);
        kmc_ctx* next = nullptr;
        rc = kmc_create(&next, &cfg);
        if (rc) { int r = die("kmc_create", kmc_last_error(nullptr)); destroy_all(); return r; }
        ctxs.push_back(next);
        uint64_t w[KMC_SIMPLIFY_WORDS] = {0};
        const uint64_t tip = tip_keys < 0 ? (uint64_t)k : (uint64_t)tip_keys, isl = island_keys < 0 ? (uint64_t)k : (uint64_t)island_keys;
        if (bubble_keys < 0 || variants) {   // (with --variants the limit is the report's: the rounds pop nothing)
            rc = kmc_unitig_clean_into(ctx, next, (uint64_t)min_count, (uint64_t)max_count, tip, isl, w);
            if (rc) { int r = die("kmc_unitig_clean_into", kmc_last_error(ctx)); destroy_all(); return r; }
        } else {
            rc = kmc_unitig_simplify_into(ctx, next, (uint64_t)min_count, (uint64_t)max_count, tip, isl, (uint64_t)bubble_keys, w);
            if (rc) { int r = die("kmc_unitig_simplify_into", kmc_last_error(ctx)); destroy_all(); return r; }
        }
        rc = kmc_finalize(next, &nd, &nt);
        if (rc) { int r = die("kmc_finalize", kmc_last_error(next)); destroy_all(); return r; }
        if (stats) {
            fprintf(stderr, "clean round %d unitigs %llu tips %llu islands %llu kept_keys %llu tip_keys %llu island_keys %llu tip_candidates %llu kept_count %llu",
                    round, (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3],
                    (unsigned long long)w[4], (unsigned long long)w[5], (unsigned long long)w[6], (unsigned long long)w[7]);
            if (bubble_keys >= 0 && !variants)
                fprintf(stderr, " bubbles %llu bubble_keys %llu bubble_candidates %llu", (unsigned long long)w[8], (unsigned long long)w[9],
                        (unsigned long long)w[10]);
            fprintf(stderr, "\n");
        }
        if (ctx != counted) {   // (the table of the round before)
            kmc_destroy(ctx);
            ctxs.erase(std::find(ctxs.begin(), ctxs.end(), ctx));
        }
        ctx = next;
        if (w[1] + w[2] + w[8] == 0) break;
    }
    // --component-keys: one more step of the same kind, the table without its small components
    if (component_keys >= 0) {
        cfg.device = gpus == 1 ? device : (share ? atoi(share) : 0);
        kmc_ctx* next = nullptr;
        rc = kmc_create(&next, &cfg);
        if (rc) { int r = die("kmc_create", kmc_last_error(nullptr)); destroy_all(); return r; }
        ctxs.push_back(next);
        uint64_t w[KMC_COMPONENT_WORDS] = {0};
        rc = kmc_unitig_components_into(ctx, next, (uint64_t)min_count, (uint64_t)max_count, (uint64_t)component_keys, w);
        if (rc) { int r = die("kmc_unitig_components_into", kmc_last_error(ctx)); destroy_all(); return r; }
        rc = kmc_finalize(next, &nd, &nt);
        if (rc) { int r = die("kmc_finalize", kmc_last_error(next)); destroy_all(); return r; }
        if (stats)
            fprintf(stderr, "component step unitigs %llu components %llu single_unitig %llu max_keys %llu max_unitigs %llu small %llu kept_keys %llu kept_count %llu\n",
                    (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4],
                    (unsigned long long)w[5], (unsigned long long)w[6], (unsigned long long)w[7]);
        if (ctx != counted) {
            kmc_destroy(ctx);
            ctxs.erase(std::find(ctxs.begin(), ctxs.end(), ctx));
        }
        ctx = next;
    }
    std::vector<char> obuf(1 << 22);
    if (with_path) {
        cfg.device = device;
        kmc_ctx* other = nullptr;
        rc = kmc_create(&other, &cfg);
        if (rc) { int r = die("kmc_create", kmc_last_error(nullptr)); destroy_all(); return r; }
        ctxs.push_back(other);
        uint64_t nd2 = 0, nt2 = 0;
        rc = kmc_count_file(other, with_path, &nd2, &nt2);
        if (rc) { int r = die(with_path, kmc_last_error(other)); destroy_all(); return r; }
        const uint64_t lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count;
        if (compare) {
            uint64_t w[KMC_COMPARE_WORDS];
            rc = kmc_compare(ctx, other, lo_c, hi_c, lo_c, hi_c, w);
            if (rc) { int r = die("kmc_compare", kmc_last_error(ctx)); destroy_all(); return r; }
            static const char* names[KMC_COMPARE_WORDS] = {"n_a", "n_b", "n_both", "sum_a", "sum_b", "shared_sum_a", "shared_sum_b", "sum_min"};
            for (int i = 0; i < KMC_COMPARE_WORDS; ++i) printf("%s\t%llu\n", names[i], (unsigned long long)w[i]);
            auto ratio = [](double x, double y) { return y != 0.0 ? x / y : 0.0; };
            const uint64_t uni = w[0] + w[1] - w[2];
            printf("union\t%llu\n", (unsigned long long)uni);
            printf("jaccard\t%.6f\n", ratio((double)w[2], (double)uni));
            printf("containment_a\t%.6f\n", ratio((double)w[2], (double)w[0]));
            printf("containment_b\t%.6f\n", ratio((double)w[2], (double)w[1]));
            printf("weighted_jaccard\t%.6f\n", ratio((double)w[7], (double)w[3] + (double)w[4] - (double)w[7]));
            printf("bray_curtis\t%.6f\n", ratio(2.0 * (double)w[7], (double)w[3] + (double)w[4]));
            fflush(stdout);
            destroy_all();
            return 0;
        }
        const int cm = count_mode >= 0 ? count_mode : KMC_COUNT_LEFT;
        uint64_t n = 0;
        rc = kmc_export_setop(ctx, other, setop, cm, lo_c, hi_c, lo_c, hi_c, nullptr, nullptr, nullptr, 0, &n);
        if (rc && !(rc == KMC_ERR_ARG && n)) { int r = die("kmc_export_setop", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint64_t> shi(n ? n : 1), slo(n ? n : 1), scnt(n ? n : 1);
        rc = kmc_export_setop(ctx, other, setop, cm, lo_c, hi_c, lo_c, hi_c, shi.data(), slo.data(), scnt.data(), n, &n);
        if (rc) { int r = die("kmc_export_setop", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        char sl[96];
        for (uint64_t i = 0; i < n; ++i) {
            kmc_decode_key(shi[i], slo[i], k, sl);
            const int m = snprintf(sl + k, sizeof(sl) - k, "\t%llu\n", (unsigned long long)scnt[i]);
            fwrite(sl, 1, (size_t)(k + m), stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (query_path) {
        std::vector<uint64_t> qc(q_lo.size() ? q_lo.size() : 1);
        rc = kmc_query(ctx, q_hi.data(), q_lo.data(), q_lo.size(), qc.data());
        if (rc) { int r = die("kmc_query", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (size_t i = 0; i < q_lo.size(); ++i) printf("%s\t%llu\n", q_text[i].c_str(), (unsigned long long)qc[i]);
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (profile_path) {
        std::vector<uint64_t> rs((size_t)prof.n_reads * KMC_PROFILE_WORDS + 1);
        const uint64_t n_prof = prof.n_reads;
        rc = kmc_profile(ctx, prof.bases, prof.offsets, n_prof, (uint64_t)min_count, nullptr, rs.data());
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_profile", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t r = 0; r < n_prof; ++r) {
            const uint64_t* w = &rs[(size_t)r * KMC_PROFILE_WORDS];
            printf("%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)r, (unsigned long long)w[0], (unsigned long long)w[1],
                   (unsigned long long)w[2], (unsigned long long)w[3], (unsigned long long)w[4]);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (map_path) {
        // the host form computes on every call: the first call sizes the segment list (and fills the arrays that need no
        // size), the second copies it
        const uint64_t n_map = prof.n_reads, lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count;
        std::vector<uint32_t> rs((size_t)n_map * KMC_MAP_READ_WORDS + 1), sg(4);
        std::vector<uint64_t> so((size_t)n_map + 1);
        uint64_t ns = 0, nu = 0;
        rc = kmc_unitig_map(ctx, lo_c, hi_c, prof.bases, prof.offsets, n_map, nullptr, rs.data(), so.data(), nullptr, 0, nullptr, 0, &ns, &nu, nullptr);
        if (!rc && ns) {
            sg.resize((size_t)ns * 4);
            rc = kmc_unitig_map(ctx, lo_c, hi_c, prof.bases, prof.offsets, n_map, nullptr, nullptr, nullptr, sg.data(), ns, nullptr, 0, &ns, &nu, nullptr);
        }
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_unitig_map", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t r = 0; r < n_map; ++r) {
            const uint32_t* w = &rs[(size_t)r * KMC_MAP_READ_WORDS];
            printf("%llu\t%u\t%u\t%u\t", (unsigned long long)r, w[0], w[1], w[2]);
            uint64_t end = 0;
            for (uint64_t i = so[r]; i < so[r + 1] && i < ns; ++i) {
                const uint32_t* g = &sg[(size_t)i * 4];
                if (i > so[r] && g[0] != end) fputc(',', stdout);
                printf("%c%u:%u:%u", (g[2] & 1) ? '<' : '>', g[2] >> 1, g[3], g[1]);
                end = (uint64_t)g[0] + g[1];
            }
            if (so[r] == so[r + 1]) fputc('*', stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (transits_path) {
        // sized from the links (a unitig's slots are at most four times the records of one of its ends): the batch is walked once
        const uint64_t n_tr = prof.n_reads, lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count;
        uint64_t nu = 0, nl = 0, nsl = 0;
        rc = kmc_unitig_links(ctx, lo_c, hi_c, nullptr, 0, nullptr, 0, &nu, &nl, nullptr);
        std::vector<uint64_t> lo_((size_t)2 * nu + 1), sup((size_t)nl + 1), to_((size_t)nu + 1), cnt((size_t)std::min<uint64_t>(16 * nu, 4 * nl) + 1);
        std::vector<uint32_t> lt((size_t)nl + 1);
        std::vector<uint8_t> vd((size_t)nu + 1);
        if (!rc) rc = kmc_unitig_links(ctx, lo_c, hi_c, lo_.data(), 2 * nu, lt.data(), nl, &nu, &nl, nullptr);
        if (rc) { kmc_free_reads(&prof); int r = die("kmc_unitig_links", kmc_last_error(ctx)); destroy_all(); return r; }
        rc = kmc_unitig_transits(ctx, lo_c, hi_c, min_reads < 0 ? 1 : (uint64_t)min_reads, 0, prof.bases, prof.offsets, n_tr, sup.data(), nl, to_.data(), nu,
                                 cnt.data(), cnt.size() - 1, vd.data(), &nu, &nl, &nsl, nullptr);
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_unitig_transits", kmc_last_error(ctx)); destroy_all(); return r; }
        static const char* const verdict_name[4] = {"plain", "unspanned", "resolved", "ambiguous"};
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t e = 0; e < 2 * nu; ++e)
            for (uint64_t j = lo_[e]; j < lo_[e + 1] && j < nl; ++j)
                if (sup[j]) printf("L\t%llu\t%u\t%llu\n", (unsigned long long)e, lt[j], (unsigned long long)sup[j]);
        for (uint64_t u = 0; u < nu; ++u) {
            if (vd[u] == KMC_TRANSIT_PLAIN) continue;
            const uint64_t ds = lo_[2 * u + 1] - lo_[2 * u], de = lo_[2 * u + 2] - lo_[2 * u + 1];
            printf("U\t%llu\t%s\t%llu\t%llu\n", (unsigned long long)u, verdict_name[vd[u] & 3], (unsigned long long)ds, (unsigned long long)de);
            for (uint64_t p = 0; p < ds; ++p)
                for (uint64_t q = 0; q < de; ++q) {
                    const uint64_t at = to_[u] + p * de + q;
                    if (at < nsl && cnt[at]) printf("T\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)u, (unsigned long long)p, (unsigned long long)q, (unsigned long long)cnt[at]);
                }
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (pairs_path) {
        // the pairs in chunks that add up (an even number of reads each); the records and the histogram of the totals come with the last
        const uint64_t n_rd = prof.n_reads, lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count, chunk = 1ull << 16;
        const uint64_t bins = insert_bins < 0 ? 1024 : (uint64_t)insert_bins;
        if (n_rd & 1) { kmc_free_reads(&prof); fprintf(stderr, "k-mer-count: --pairs %s holds an odd number of reads\n", pairs_path); destroy_all(); return 1; }
        uint64_t np = 0, nr = 0, first = 0, held = 0;
        std::vector<uint64_t> offs, hist((size_t)bins), rc_, rs, rn, rx;
        std::vector<uint32_t> re;
        do {
            const uint64_t n = std::min<uint64_t>(chunk, n_rd - first), b0 = n_rd ? prof.offsets[first] : 0;
            offs.assign((size_t)n + 1, 0);
            for (uint64_t i = 0; i <= n && n_rd; ++i) offs[(size_t)i] = prof.offsets[first + i] - b0;
            const uint64_t cap = held + n / 2;   // n_records <= the pairs of this call plus the records held
            re.resize((size_t)2 * cap + 1); rc_.resize((size_t)cap + 1); rs.resize((size_t)cap + 1); rn.resize((size_t)cap + 1); rx.resize((size_t)cap + 1);
            const bool last = first + n >= n_rd;
            rc = kmc_unitig_pairs(ctx, lo_c, hi_c, bins, first ? KMC_PAIR_ACCUMULATE : 0, n_rd ? prof.bases + b0 : nullptr, offs.data(), n, nullptr, nullptr,
                                  nullptr, 0, last ? re.data() : nullptr, last ? rc_.data() : nullptr, last ? rs.data() : nullptr, last ? rn.data() : nullptr,
                                  last ? rx.data() : nullptr, cap, last ? hist.data() : nullptr, bins, &np, &nr, nullptr);
            held = nr;
            first += n;
        } while (!rc && first < n_rd);
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_unitig_pairs", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t f = 0; f < bins; ++f)
            if (hist[(size_t)f]) printf("I\t%llu\t%llu\n", (unsigned long long)f, (unsigned long long)hist[(size_t)f]);
        for (uint64_t j = 0; j < nr; ++j)
            printf("P\t%u\t%u\t%llu\t%llu\t%llu\t%llu\n", re[(size_t)2 * j], re[(size_t)2 * j + 1], (unsigned long long)rc_[(size_t)j],
                   (unsigned long long)rs[(size_t)j], (unsigned long long)rn[(size_t)j], (unsigned long long)rx[(size_t)j]);
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (contigs_path) {
        // the reads in chunks that add up, then the contigs of the totals: a sizing call, then the copy call
        const uint64_t n_rd = prof.n_reads, lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count, chunk = 1ull << 16;
        const uint64_t mr = min_reads < 0 ? 1 : (uint64_t)min_reads, ms = min_support < 0 ? 0 : (uint64_t)min_support;
        uint64_t nu = 0, nl = 0, nsl = 0, first = 0;
        std::vector<uint64_t> offs;
        do {
            const uint64_t n = std::min<uint64_t>(chunk, n_rd - first), b0 = n_rd ? prof.offsets[first] : 0;
            offs.assign((size_t)n + 1, 0);
            for (uint64_t i = 0; i <= n && n_rd; ++i) offs[(size_t)i] = prof.offsets[first + i] - b0;
            rc = kmc_unitig_transits(ctx, lo_c, hi_c, mr, first ? KMC_TRANSIT_ACCUMULATE : 0, n_rd ? prof.bases + b0 : nullptr, offs.data(), n, nullptr, 0,
                                     nullptr, 0, nullptr, 0, nullptr, &nu, &nl, &nsl, nullptr);
            first += n;
        } while (!rc && first < n_rd);
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_unitig_transits", kmc_last_error(ctx)); destroy_all(); return r; }
        uint64_t nc = 0, nn = 0, nb = 0;
        rc = kmc_unitig_contigs(ctx, lo_c, hi_c, mr, ms, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &nc, &nn, &nb, nullptr);
        std::vector<uint8_t> cb((size_t)nb + 1), fl((size_t)nc + 1);
        std::vector<uint64_t> co((size_t)nc + 1), po((size_t)nc + 1), ab((size_t)nc + 1);
        std::vector<uint32_t> pa((size_t)nn + 1);
        if (!rc) rc = kmc_unitig_contigs(ctx, lo_c, hi_c, mr, ms, cb.data(), nb, co.data(), po.data(), ab.data(), fl.data(), nc, pa.data(), nn, &nc, &nn, &nb, nullptr);
        if (rc) { int r = die("kmc_unitig_contigs", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t c = 0; c < nc; ++c) {
            printf(">%llu LN:i:%llu KC:i:%llu CL:i:%d WK:Z:", (unsigned long long)c, (unsigned long long)(co[c + 1] - co[c]), (unsigned long long)ab[c], fl[c] & 1);
            for (uint64_t i = po[c]; i < po[c + 1] && i < nn; ++i) printf("%c%u", (pa[i] & 1) ? '<' : '>', pa[i] >> 1);
            fputc('\n', stdout);
            fwrite(cb.data() + co[c], 1, (size_t)(co[c + 1] - co[c]), stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (correct_path) {
        // the records are not printed: one call fills everything this needs
        const uint64_t n_cor = prof.n_reads;
        std::vector<uint32_t> rs((size_t)n_cor * KMC_CORRECT_READ_WORDS + 1);
        std::vector<uint8_t> cb((size_t)(n_cor ? prof.offsets[n_cor] : 0) + 1);
        uint64_t nc = 0;
        rc = kmc_correct(ctx, (uint64_t)min_count, (uint64_t)max_count, prof.bases, prof.offsets, n_cor, cb.data(), rs.data(), nullptr, nullptr, 0, &nc, nullptr);
        if (rc) { kmc_free_reads(&prof); int r = die("kmc_correct", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t r = 0; r < n_cor; ++r) {
            const uint32_t* w = &rs[(size_t)r * KMC_CORRECT_READ_WORDS];
            printf(">%llu %u %u %u %u\n", (unsigned long long)r, w[0], w[1], w[2], w[3]);
            fwrite(cb.data() + prof.offsets[r], 1, (size_t)(prof.offsets[r + 1] - prof.offsets[r]), stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        kmc_free_reads(&prof);
        destroy_all();
        return 0;
    }
    if (trim_path) {
        // the host form computes on every call: the first call sizes the emitted batch (and fills the per-read rows), the second
        // copies it
        const uint64_t n_trim = prof.n_reads, lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count;
        const uint32_t flags = (trim_invert ? KMC_TRIM_INVERT : 0u) | (uint32_t)trim_pair;
        const uint64_t ms = min_strong < 0 ? 0 : (uint64_t)min_strong, ml = min_len < 0 ? 0 : (uint64_t)min_len;
        const uint32_t mp = strong_permille < 0 ? 0u : (uint32_t)strong_permille;
        if (trim_pair && (n_trim & 1)) {
            kmc_free_reads(&prof);
            fprintf(stderr, "k-mer-count: --paired needs an even number of reads (%s has %llu)\n", trim_path, (unsigned long long)n_trim);
            destroy_all();
            return 2;
        }
        std::vector<uint32_t> rs((size_t)n_trim * KMC_TRIM_READ_WORDS + 1);
        uint64_t no = 0, nb = 0;
        rc = kmc_trim(ctx, lo_c, hi_c, trim_mode, flags, ms, mp, ml, prof.bases, prof.offsets, n_trim, nullptr, 0, nullptr, nullptr, 0, rs.data(), nullptr,
                      &no, &nb, nullptr);
        std::vector<uint8_t> ob((size_t)nb + 1);
        std::vector<uint64_t> oo((size_t)no + 1), og((size_t)no + 1);
        if (!rc) rc = kmc_trim(ctx, lo_c, hi_c, trim_mode, flags, ms, mp, ml, prof.bases, prof.offsets, n_trim, ob.data(), nb, oo.data(), og.data(), no,
                               nullptr, nullptr, &no, &nb, nullptr);
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_trim", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t i = 0; i < no; ++i) {
            const uint32_t* w = &rs[(size_t)og[i] * KMC_TRIM_READ_WORDS];
            printf(">%llu %u %u %u %u\n", (unsigned long long)og[i], w[0], w[1], w[2], w[3]);
            fwrite(ob.data() + oo[i], 1, (size_t)(oo[i + 1] - oo[i]), stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (norm_path) {
        // the host form computes on every call: the first call sizes the emitted batch (and fills the per-read rows), the second
        // copies it
        const uint64_t n_norm = prof.n_reads, tg = (uint64_t)norm_target, md = min_depth < 0 ? 0 : (uint64_t)min_depth;
        const uint64_t sd = norm_seed < 0 ? 0 : (uint64_t)norm_seed;
        const uint32_t pm = depth_permille < 0 ? 500u : (uint32_t)depth_permille;
        const uint32_t flags = (norm_paired ? KMC_NORM_PAIRED : 0u) | (norm_invert ? KMC_NORM_INVERT : 0u);
        if (norm_paired && (n_norm & 1)) {
            kmc_free_reads(&prof);
            fprintf(stderr, "k-mer-count: --norm-paired needs an even number of reads (%s has %llu)\n", norm_path, (unsigned long long)n_norm);
            destroy_all();
            return 2;
        }
        std::vector<uint32_t> rs((size_t)n_norm * KMC_NORMALIZE_READ_WORDS + 1);
        uint64_t no = 0, nb = 0;
        rc = kmc_normalize(ctx, pm, tg, md, sd, flags, prof.bases, prof.offsets, n_norm, nullptr, 0, nullptr, nullptr, 0, rs.data(), nullptr, &no, &nb,
                           nullptr);
        std::vector<uint8_t> ob((size_t)nb + 1);
        std::vector<uint64_t> oo((size_t)no + 1), og((size_t)no + 1);
        if (!rc) rc = kmc_normalize(ctx, pm, tg, md, sd, flags, prof.bases, prof.offsets, n_norm, ob.data(), nb, oo.data(), og.data(), no, nullptr,
                                    nullptr, &no, &nb, nullptr);
        kmc_free_reads(&prof);
        if (rc) { int r = die("kmc_normalize", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t i = 0; i < no; ++i) {
            const uint32_t* w = &rs[(size_t)og[i] * KMC_NORMALIZE_READ_WORDS];
            printf(">%llu %u %u %u\n", (unsigned long long)og[i], w[0], w[1], w[2]);
            fwrite(ob.data() + oo[i], 1, (size_t)(oo[i + 1] - oo[i]), stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (unitigs || gfa) {
        uint64_t nu = 0, nb = 0;
        rc = kmc_unitigs(ctx, (uint64_t)min_count, (uint64_t)max_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nu, &nb, nullptr);
        if (rc) { int r = die("kmc_unitigs", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint8_t> ub(nb ? nb : 1), uf(nu ? nu : 1);
        std::vector<uint64_t> uo(nu + 1), ua(nu ? nu : 1);
        rc = kmc_unitigs(ctx, (uint64_t)min_count, (uint64_t)max_count, ub.data(), nb, uo.data(), ua.data(), uf.data(), nu, &nu, &nb, nullptr);
        if (rc) { int r = die("kmc_unitigs", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint64_t> lo_(1);
        std::vector<uint32_t> lt(1);
        uint64_t nl = 0;
        if (gfa) {   // (the unitigs are still in the ctx: the links pass alone runs)
            rc = kmc_unitig_links(ctx, (uint64_t)min_count, (uint64_t)max_count, nullptr, 0, nullptr, 0, &nu, &nl, nullptr);
            if (rc) { int r = die("kmc_unitig_links", kmc_last_error(ctx)); destroy_all(); return r; }
            lo_.resize(2 * nu + 1);
            lt.resize(nl ? nl : 1);
            rc = kmc_unitig_links(ctx, (uint64_t)min_count, (uint64_t)max_count, lo_.data(), 2 * nu, lt.data(), nl, &nu, &nl, nullptr);
            if (rc) { int r = die("kmc_unitig_links", kmc_last_error(ctx)); destroy_all(); return r; }
        }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        if (gfa) {
            printf("H\tVN:Z:1.0\n");
            for (uint64_t u = 0; u < nu; ++u) {
                printf("S\t%llu\t", (unsigned long long)u);
                fwrite(ub.data() + uo[u], 1, (size_t)(uo[u + 1] - uo[u]), stdout);
                printf("\tLN:i:%llu\tKC:i:%llu\tCL:i:%u\n", (unsigned long long)(uo[u + 1] - uo[u]), (unsigned long long)ua[u],
                       (unsigned)(uf[u] & KMC_UNITIG_CIRCULAR));
            }
            for (uint64_t e = 0; e < 2 * nu; ++e)
                for (uint64_t j = lo_[e]; j < lo_[e + 1]; ++j)
                    printf("L\t%llu\t%c\t%llu\t%c\t%dM\n", (unsigned long long)(e >> 1), (e & 1) ? '+' : '-', (unsigned long long)(lt[j] >> 1),
                           (lt[j] & 1) ? '-' : '+', k - 1);
            fflush(stdout);
            destroy_all();
            return 0;
        }
        for (uint64_t u = 0; u < nu; ++u) {
            printf(">%llu LN:i:%llu KC:i:%llu CL:i:%u\n", (unsigned long long)u, (unsigned long long)(uo[u + 1] - uo[u]),
                   (unsigned long long)ua[u], (unsigned)(uf[u] & KMC_UNITIG_CIRCULAR));
            fwrite(ub.data() + uo[u], 1, (size_t)(uo[u + 1] - uo[u]), stdout);
            fputc('\n', stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (components) {   // size, then copy: the ctx computes once
        uint64_t nc = 0, nu = 0, nk = 0;
        const uint64_t lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count;
        rc = kmc_unitig_components(ctx, lo_c, hi_c, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, &nc, &nu, &nk, nullptr);
        if (rc) { int r = die("kmc_unitig_components", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint64_t> cs((size_t)(nc ? nc : 1) * KMC_COMPONENT_STAT_WORDS);
        rc = kmc_unitig_components(ctx, lo_c, hi_c, 0, nullptr, nullptr, 0, cs.data(), nc, nullptr, nullptr, nullptr, 0, &nc, &nu, &nk, nullptr);
        if (rc) { int r = die("kmc_unitig_components", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (uint64_t c = 0; c < nc; ++c) {
            const uint64_t* w = &cs[(size_t)c * KMC_COMPONENT_STAT_WORDS];
            printf("%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)c, (unsigned long long)w[0], (unsigned long long)w[1],
                   (unsigned long long)w[2], (unsigned long long)w[3]);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (variants) {   // size, the unitigs the records refer to (held by the ctx: copied, not computed again), then copy
        const uint64_t lo_c = (uint64_t)min_count, hi_c = (uint64_t)max_count, lim = bubble_keys < 0 ? (uint64_t)k : (uint64_t)bubble_keys;
        uint64_t nr = 0, nu = 0, nb = 0;
        rc = kmc_unitig_bubbles(ctx, lo_c, hi_c, lim, nullptr, 0, &nr, &nu, nullptr);
        if (rc) { int r = die("kmc_unitig_bubbles", kmc_last_error(ctx)); destroy_all(); return r; }
        rc = kmc_unitigs(ctx, lo_c, hi_c, nullptr, 0, nullptr, nullptr, nullptr, 0, &nu, &nb, nullptr);
        if (rc) { int r = die("kmc_unitigs", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint8_t> ub(nb ? nb : 1);
        std::vector<uint64_t> uo(nu + 1), ua(nu ? nu : 1);
        rc = kmc_unitigs(ctx, lo_c, hi_c, ub.data(), nb, uo.data(), ua.data(), nullptr, nu, &nu, &nb, nullptr);
        if (rc) { int r = die("kmc_unitigs", kmc_last_error(ctx)); destroy_all(); return r; }
        std::vector<uint32_t> rec((size_t)(nr ? nr : 1) * KMC_BUBBLE_RECORD_WORDS);
        rc = kmc_unitig_bubbles(ctx, lo_c, hi_c, lim, rec.data(), nr, &nr, &nu, nullptr);
        if (rc) { int r = die("kmc_unitig_bubbles", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        std::string arm;
        for (uint64_t i = 0; i < nr; ++i) {
            const uint32_t* w = &rec[(size_t)i * KMC_BUBBLE_RECORD_WORDS];
            const uint64_t u = w[0], v = w[1], lu = uo[u + 1] - uo[u], lv = uo[v + 1] - uo[v];
            arm.assign((const char*)ub.data() + uo[v], (size_t)lv);
            if (w[6] & KMC_BUBBLE_REVERSED) {   // W in U's direction
                std::reverse(arm.begin(), arm.end());
                for (char& ch : arm) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : 'A';
            }
            printf("%llu\t%c\t%u\t%u\t%u\t", (unsigned long long)i, "SIC?"[KMC_BUBBLE_KIND(w[6])], w[0], w[1], w[4]);
            const uint64_t au = lu - w[4] - w[5], av = lv - w[4] - w[5];
            if (au) fwrite(ub.data() + uo[u] + w[4], 1, (size_t)au, stdout); else fputc('-', stdout);
            fputc('\t', stdout);
            if (av) fwrite(arm.data() + w[4], 1, (size_t)av, stdout); else fputc('-', stdout);
            printf("\t%llu/%llu\t%llu/%llu\n", (unsigned long long)ua[u], (unsigned long long)(lu - (uint64_t)(k - 1)), (unsigned long long)ua[v],
                   (unsigned long long)(lv - (uint64_t)(k - 1)));
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (graph_stats) {
        uint64_t w[KMC_GRAPH_WORDS], n = 0;
        rc = kmc_graph(ctx, (uint64_t)min_count, (uint64_t)max_count, nullptr, 0, &n, w);
        if (rc) { int r = die("kmc_graph", kmc_last_error(ctx)); destroy_all(); return r; }
        static const char* names[KMC_GRAPH_WORDS] = {"nodes", "right_degrees", "left_degrees", "isolated", "dead_ends", "branching",
                                                     "end_sides", "single_node_unitigs"};
        for (int i = 0; i < KMC_GRAPH_WORDS; ++i) printf("%s\t%llu\n", names[i], (unsigned long long)w[i]);
        printf("unitigs\t%llu\n", (unsigned long long)(w[6] / 2));
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (graph) {
        std::vector<uint64_t> ghi(nd ? nd : 1), glo(nd ? nd : 1), gcnt(nd ? nd : 1);
        std::vector<uint16_t> adj(nd ? nd : 1);
        uint64_t n = 0;
        rc = kmc_export(ctx, ghi.data(), glo.data(), gcnt.data(), nd);
        if (rc) { int r = die("kmc_export", kmc_last_error(ctx)); destroy_all(); return r; }
        rc = kmc_graph(ctx, (uint64_t)min_count, (uint64_t)max_count, adj.data(), nd, &n, nullptr);
        if (rc) { int r = die("kmc_graph", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        char gl[128];
        for (uint64_t i = 0; i < n; ++i) {
            const unsigned a = adj[i];
            if (!KMC_GRAPH_SOLID(a)) continue;
            kmc_decode_key(ghi[i], glo[i], k, gl);
            int m = k + snprintf(gl + k, sizeof(gl) - k, "\t%llu\t", (unsigned long long)gcnt[i]);
            for (int side = 0; side < 2; ++side) {
                const unsigned nib = side ? KMC_GRAPH_LEFT(a) : KMC_GRAPH_RIGHT(a);
                if (!nib) gl[m++] = '.';
                for (int c = 0; c < 4; ++c) if ((nib >> c) & 1) gl[m++] = "ACGT"[c];
                gl[m++] = '\t';
            }
            if (KMC_GRAPH_END_L(a)) gl[m++] = 'L';
            if (KMC_GRAPH_END_R(a)) gl[m++] = 'R';
            if (!KMC_GRAPH_END_L(a) && !KMC_GRAPH_END_R(a)) gl[m++] = '.';
            gl[m++] = '\n';
            fwrite(gl, 1, (size_t)m, stdout);
        }
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (histo) {
        std::vector<uint64_t> h((size_t)histo + 1);
        rc = kmc_histogram(ctx, (uint64_t)min_count, (uint64_t)max_count, (uint32_t)histo + 1, h.data(), nullptr);
        if (rc) { int r = die("kmc_histogram", kmc_last_error(ctx)); destroy_all(); return r; }
        setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
        for (int c = 1; c <= histo; ++c)
            if (h[(size_t)c]) printf("%d\t%llu\n", c, (unsigned long long)h[(size_t)c]);
        fflush(stdout);
        destroy_all();
        return 0;
    }
    if (filtered) {   // the kept keys only: size, then copy
        rc = kmc_export_filtered(ctx, (uint64_t)min_count, (uint64_t)max_count, nullptr, nullptr, nullptr, 0, &nd);
        if (rc && !(rc == KMC_ERR_ARG && nd)) { int r = die("kmc_export_filtered", kmc_last_error(ctx)); destroy_all(); return r; }
    }
    std::vector<uint64_t> hi(nd ? nd : 1), lo(nd ? nd : 1), cnt(nd ? nd : 1);
    rc = filtered ? kmc_export_filtered(ctx, (uint64_t)min_count, (uint64_t)max_count, hi.data(), lo.data(), cnt.data(), nd, &nd)
                  : kmc_export(ctx, hi.data(), lo.data(), cnt.data(), nd);
    if (rc) { int r = die(filtered ? "kmc_export_filtered" : "kmc_export", kmc_last_error(ctx)); destroy_all(); return r; }
    const int klen = k ? k : 54;
    setvbuf(stdout, obuf.data(), _IOFBF, obuf.size());
    char line[96];
    for (uint64_t i = 0; i < nd; ++i) {
        kmc_decode_key(hi[i], lo[i], klen, line);
        if (expand) {
            line[klen] = '\n';
            for (uint64_t c = 0; c < cnt[i]; ++c) fwrite(line, 1, (size_t)klen + 1, stdout);
        } else {
            int m = snprintf(line + klen, sizeof(line) - klen, "\t%llu\n", (unsigned long long)cnt[i]);
            fwrite(line, 1, (size_t)(klen + m), stdout);
        }
    }
    fflush(stdout);
    if (stats) {
        kmc_stats s;
        kmc_get_stats(counted, &s);
        fprintf(stderr, "reads %llu bases %llu kmers %llu distinct %llu table_slots %llu spilled %llu kernel_ms %.3f algo %d\n",
                (unsigned long long)s.n_reads, (unsigned long long)s.n_bases, (unsigned long long)s.n_kmers,
                (unsigned long long)s.n_distinct, (unsigned long long)s.table_capacity, (unsigned long long)s.n_spilled,
                s.kernel_ms_last, s.algo_last);
    }
    destroy_all();
    return 0;
}
