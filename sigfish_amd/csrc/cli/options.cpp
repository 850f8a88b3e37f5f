// options.cpp -- the options of `sigfish-amd dtw` (src/dtw_main.c:125-277): table, help and the checks between options.
// Nothing here opens a file or touches a device, so -V and help may exit() from here.
#include <cmath>
#include <getopt.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../../include/sigfish_amd.h"
#include "../recal_rule.hpp"
#include "cli.hpp"

namespace cli {
namespace {

// long options without a letter (getopt_long returns these; the letters return themselves)
enum LongOpt {
    O_KMER_MODEL = 256, O_RNA, O_DEBUG_BREAK, O_DTW_STD, O_INVERT, O_FULL_REF, O_FROM_END, O_PROFILE_CPU, O_ACCEL, O_PORE, O_DEVICE,
    O_SECONDARY, O_METH_MODEL, O_HOST_EVENTS, O_STREAMS, O_HOST_PARSE, O_GPU_PARSE, O_RANKS, O_SHARD, O_READ_RANGE, O_NO_HEADER,
    O_RANK_BUFFER, O_HOST_PATHS, O_DEVICE_PATHS, O_CHANNELS, O_CHUNK_SAMPLES, O_NORM_EVENTS, O_MIN_EVENTS, O_MIN_MAPQ, O_PACE,
    O_RECALIBRATE, O_RECALIBRATE_AT_END, O_RESWEEP, O_CANDIDATES, O_SECONDARY_STRIPS, O_SPREAD, O_TARGETS, O_ENRICH, O_DEPLETE, O_MARGIN, O_BY_NAME, O_TRACE, O_QUOTA, O_TRUTH, O_DEPTH_CAP, O_GROUP_CAP, O_LEAD, O_STRANDED, O_GROUP_LEAD, O_GROUP_STRANDED
};

const option kLongOptions[] = {
    {"threads", required_argument, 0, 't'}, {"batchsize", required_argument, 0, 'K'}, {"max-bytes", required_argument, 0, 'B'},
    {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'V'},
    {"kmer-model", required_argument, 0, O_KMER_MODEL}, {"output", required_argument, 0, 'o'}, {"rna", no_argument, 0, O_RNA},
    {"prefix", required_argument, 0, 'p'}, {"query-size", required_argument, 0, 'q'}, {"debug-break", required_argument, 0, O_DEBUG_BREAK},
    {"dtw-std", no_argument, 0, O_DTW_STD}, {"invert", no_argument, 0, O_INVERT}, {"full-ref", no_argument, 0, O_FULL_REF},
    {"from-end", no_argument, 0, O_FROM_END}, {"profile-cpu", required_argument, 0, O_PROFILE_CPU}, {"accel", required_argument, 0, O_ACCEL},
    {"sam", no_argument, 0, 'a'}, {"pore", required_argument, 0, O_PORE}, {"device", required_argument, 0, O_DEVICE},
    {"secondary", required_argument, 0, O_SECONDARY}, {"window", required_argument, 0, 'w'}, {"meth-model", required_argument, 0, O_METH_MODEL},
    {"host-events", no_argument, 0, O_HOST_EVENTS}, {"streams", required_argument, 0, O_STREAMS}, {"host-parse", no_argument, 0, O_HOST_PARSE},
    {"gpu-parse", no_argument, 0, O_GPU_PARSE}, {"ranks", required_argument, 0, O_RANKS}, {"shard", required_argument, 0, O_SHARD},
    {"read-range", required_argument, 0, O_READ_RANGE}, {"no-header", no_argument, 0, O_NO_HEADER},
    {"rank-buffer", required_argument, 0, O_RANK_BUFFER}, {"host-paths", no_argument, 0, O_HOST_PATHS},
    {"device-paths", no_argument, 0, O_DEVICE_PATHS}, {"secondary-strips", no_argument, 0, O_SECONDARY_STRIPS},
    {0, 0, 0, 0}};

bool yes_or_no(const char *arg, const char *what) {  // yes_or_no(), src/dtw_main.c:92-113
    if (!strcmp(arg, "yes") || !strcmp(arg, "y")) return true;
    if (!strcmp(arg, "no") || !strcmp(arg, "n")) return false;
    die(std::string("option '--") + what + "' only accepts 'yes' or 'no'.");
}

int64_t parse_num(const char *s) {  // K/M/G suffixes as src/dtw_main.c:46-58
    char *e;
    double x = strtod(s, &e);
    if (*e == 'G' || *e == 'g')
        x *= 1e9;
    else if (*e == 'M' || *e == 'm')
        x *= 1e6;
    else if (*e == 'K' || *e == 'k')
        x *= 1e3;
    return static_cast<int64_t>(x + .499);
}

void help(FILE *fp, const Opt &o) {
    fprintf(fp, "Usage: sigfish-amd dtw [OPTIONS] genome.fa reads.blow5|reads.slow5\n\nbasic options:\n");
    fprintf(fp, "   -t INT                     number of host threads for parsing and event detection [%d]\n", o.threads);
    fprintf(fp, "   -K INT                     batch size (max number of reads loaded at once) [%d]\n", o.batch_size);
    fprintf(fp, "   -B FLOAT[K/M/G]            max number of bytes loaded at once [%.1fM]\n", o.batch_bytes / 1e6);
    fprintf(fp, "   -h                         help\n   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --verbose INT              verbosity level [%d]\n   --version                  print version\n", o.verbosity);
    fprintf(fp, "   --pore STR                 set the pore chemistry (r9, r10 or rna004) [auto]\n");
    fprintf(fp, "   --device INT[,INT...]      GPU(s) to use; batches are dealt to them in turn [0]\n   --host-events              detect events on host threads instead of the GPU\n   --gpu-parse | --host-parse decompress and parse the records on the GPU | on host threads [host threads up to 2 GPUs per process, GPU beyond]\n   --streams INT              device contexts taking batches in turn [2]\n");
    fprintf(fp, "   --ranks INT                read-shard the run over INT processes (rank r: device r of the list, -t/INT threads, the r-th\n"
                "                              byte slice of the file, which must be a regular file); output is printed in rank order = file\n"
                "                              order [one per distinct device]\n"
                "   --shard r/G                map only the records starting in the r-th of G equal byte slices of the file\n"
                "   --read-range A:B           map only records A..B-1 of the file (B omitted: to the end)\n"
                "   --rank-buffer FLOAT[K/M/G] gathered output kept in memory per rank; the rest waits in an unnamed temporary file [%.0fM]\n"
                "   --no-header                do not print the SAM header (ranks after the first)\n\nadvanced options:\n", o.rank_buffer / 1e6);
    fprintf(fp, "   --kmer-model FILE          nucleotide k-mer model file (required: builtin models are not bundled)\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA\n");
    fprintf(fp, "   -q INT                     the number of events in query signal to align [%d]\n", o.query);
    fprintf(fp, "   -p INT                     the number of events to trim at query signal start [%d]\n", o.prefix);
    fprintf(fp, "   --debug-break INT          break after processing the specified no. of batches\n");
    fprintf(fp, "   --dtw-std                  use DTW standard instead of DTW subsequence\n");
    fprintf(fp, "   --invert                   reverse the reference events instead of query\n");
    fprintf(fp, "   --full-ref                 map to the full reference\n");
    fprintf(fp, "   --from-end                 map the end portion of the query instead of the beginning\n");
    fprintf(fp, "   --sam                      output in SAM format\n");
    fprintf(fp, "   --device-paths | --host-paths  with --sam: warp paths of a whole batch on the GPU | read by read on the host threads [host threads]\n");
    fprintf(fp, "   --secondary STR            print secondary mappings. yes or no [no]\n");
    fprintf(fp, "   --secondary-strips         with --secondary yes: secondary mappings also for -q beyond 2048 events, whose reads run in row\n"
                "                              strips (the library's option \"secondary_strips\"); without it such a -q is refused [off]\n");
    fprintf(fp, "   --profile-cpu=yes|no       run the stages one after the other and report Parse/Events/Normalise/DTW time [no]\n");
    fprintf(fp, "   --accel=yes|no             run the alignment on the accelerator [yes]; 'no' is an error: this build has no CPU path\n");
}

void parse_device_list(const char *arg, std::vector<int> *devices) {
    devices->clear();
    for (const char *p = arg; *p;) {
        char *e = nullptr;
        const long d = strtol(p, &e, 10);
        if (e == p || d < 0) die("--device takes a comma separated list of GPU indices");
        devices->push_back(static_cast<int>(d));
        p = (*e == ',') ? e + 1 : e;
        if (*e && *e != ',') die("--device takes a comma separated list of GPU indices");
    }
    if (devices->empty()) die("--device takes a comma separated list of GPU indices");
}

// `realtime`: its own options, those of dtw it shares, and those of dtw it refuses by name (a session has no such mode)
const option kRealtimeOptions[] = {
    {"threads", required_argument, 0, 't'}, {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'V'},
    {"kmer-model", required_argument, 0, O_KMER_MODEL}, {"output", required_argument, 0, 'o'}, {"rna", no_argument, 0, O_RNA},
    {"prefix", required_argument, 0, 'p'}, {"query-size", required_argument, 0, 'q'}, {"invert", no_argument, 0, O_INVERT},
    {"pore", required_argument, 0, O_PORE}, {"device", required_argument, 0, O_DEVICE},
    {"channels", required_argument, 0, O_CHANNELS}, {"chunk-samples", required_argument, 0, O_CHUNK_SAMPLES},
    {"norm-events", required_argument, 0, O_NORM_EVENTS}, {"min-events", required_argument, 0, O_MIN_EVENTS},
    {"min-mapq", required_argument, 0, O_MIN_MAPQ}, {"pace", required_argument, 0, O_PACE},
    {"recalibrate", required_argument, 0, O_RECALIBRATE}, {"recalibrate-at-end", no_argument, 0, O_RECALIBRATE_AT_END},
    {"resweep", no_argument, 0, O_RESWEEP}, {"dtw-std", no_argument, 0, O_DTW_STD}, {"from-end", no_argument, 0, O_FROM_END}, {"sam", no_argument, 0, 'a'},
    {"secondary", required_argument, 0, O_SECONDARY}, {"ranks", required_argument, 0, O_RANKS},
    {"candidates", required_argument, 0, O_CANDIDATES}, {"spread", no_argument, 0, O_SPREAD},
    {"targets", required_argument, 0, O_TARGETS}, {"enrich", no_argument, 0, O_ENRICH}, {"deplete", no_argument, 0, O_DEPLETE},
    {"margin", required_argument, 0, O_MARGIN}, {"by-name", no_argument, 0, O_BY_NAME}, {"quota", required_argument, 0, O_QUOTA}, {"trace", required_argument, 0, O_TRACE},
    {"truth", required_argument, 0, O_TRUTH}, {"depth-cap", required_argument, 0, O_DEPTH_CAP}, {"group-cap", required_argument, 0, O_GROUP_CAP},
    {"lead", required_argument, 0, O_LEAD}, {"stranded", no_argument, 0, O_STRANDED}, {"group-lead", required_argument, 0, O_GROUP_LEAD}, {"group-stranded", no_argument, 0, O_GROUP_STRANDED},
    {0, 0, 0, 0}};

void realtime_help(FILE *fp, const RealtimeOpt &r) {
    fprintf(fp, "Usage: sigfish-amd realtime [OPTIONS] genome.fa reads.blow5|reads.slow5\n\n"
                "Replays the file as a flow cell would deliver it, through a raw-signal session (sfa_session_extend_raw): read i starts on\n"
                "channel i; at every tick each busy channel sends its next --chunk-samples samples, all channels in one call; a read is\n"
                "decided early (E: --min-events query events and mapq >= --min-mapq), when its query is full (F) or at its end (R), its\n"
                "PAF line is printed at that moment, and the channel takes the next read of the file.  The schedule counts ticks, not\n"
                "seconds: the output does not depend on the machine's speed.\n\n"
                "With the defaults (--norm-events = -q, never early) a read's line, without the three tags at its end, is the line\n"
                "`sigfish-amd dtw -p P -q Q` prints for it whenever the read has P + Q events: the same events, the window [P, P + Q),\n"
                "the same normalisation over that window, the same row.  The one difference: a read with fewer than P + norm events is\n"
                "never calibrated and prints nothing, where dtw shortens its window.\n"
                "With --recalibrate and --recalibrate-at-end a read may be calibrated on few events, decided early, and still print dtw's\n"
                "line when it is not: the window grows with the read, up to -q or, for a read that ends short, to all its events.\n\nbasic options:\n");
    fprintf(fp, "   -t INT                     number of host threads decoding the records ahead of need [%d]\n", r.o.threads);
    fprintf(fp, "   -h                         help\n   -o FILE                    output to file [stdout]\n");
    fprintf(fp, "   --verbose INT              verbosity level [%d]\n   --version                  print version\n", r.o.verbosity);
    fprintf(fp, "   --pore STR                 set the pore chemistry (r9, r10 or rna004) [auto]\n");
    fprintf(fp, "   --device INT[,INT...]      the GPU to use; a list needs --spread [0]\n");
    fprintf(fp, "   --spread                   deal the channels over every GPU of --device (channel i on the i %% G-th; a GPU listed twice\n"
                "                              counts twice): the session is created with SFA_SESSION_SPREAD.  Same output [off]\n");
    fprintf(fp, "   --kmer-model FILE          nucleotide k-mer model file (required: builtin models are not bundled)\n");
    fprintf(fp, "   --rna                      the dataset is direct RNA (needs --invert or --resweep: a session cannot extend a reversed query)\n");
    fprintf(fp, "   --invert                   reverse the reference events instead of query\n");
    fprintf(fp, "   --resweep                  sweep a read only when its normalisation window changes (calibration, every --recalibrate point,\n"
                "                              --recalibrate-at-end), over the window's events: with --rna the query is the events reversed,\n"
                "                              as dtw takes it without --invert; ne:i and --min-events count the window [off]\n");
    fprintf(fp, "   -q INT                     query events at which a read is full [%d]\n", r.o.query);
    fprintf(fp, "   -p INT                     the number of events to trim at query signal start, >= 0 [%d]\n\nreplay options:\n", r.o.prefix);
    fprintf(fp, "   --channels INT             channels of the flow cell = slots of the session [%d]\n", r.channels);
    fprintf(fp, "   --chunk-samples INT        samples a channel sends per tick [%ld]\n", static_cast<long>(r.chunk_samples));
    fprintf(fp, "   --norm-events INT          events the normalisation is frozen over, 25..q [the value of -q]\n");
    fprintf(fp, "   --recalibrate LIST|double  window lengths, ascending, above --norm-events and up to q: a read that reaches one is\n"
                "                              normalised over that many events and swept again from its first event inside the tick;\n"
                "                              double = 2 x norm-events, 4 x, ... below q, then q (at most twice the sweep work) [off]\n");
    fprintf(fp, "   --recalibrate-at-end       a read's last line is dtw's: a read that ends with 25 .. q - 1 events behind -p is normalised\n"
                "                              over all of them, as dtw normalises a read that is too short, and q joins the --recalibrate\n"
                "                              points (if it is not the last already), so that a full read is normalised over q events [off]\n");
    fprintf(fp, "   --min-events INT           no early decision below this many query events [the value of -q]\n");
    fprintf(fp, "   --min-mapq INT             decide early at this mapq; 61 = never [%d]\n", r.min_mapq);
    fprintf(fp, "   --candidates INT           behind every primary line, the channel's next 1..4 candidates of the sorted list of the 5 best\n"
                "                              windows (tp:A:S lines, best first, same span and tags): what dtw --secondary yes prints, for\n"
                "                              the events the read has at its decision [off]\n");
    fprintf(fp, "   --targets FILE.bed         adaptive sampling: the early decision is the class decision -- the best on-target column of the\n"
                "                              read's carried row against the best off-target one (sfa_session_classes) -- in place of mapq;\n"
                "                              needs --enrich or --deplete, and --margin; lines gain tc:A:<T|O|N> ac:A:<A|U|P> tm:f:<margin met>;\n"
                "                              an accepted or proceeding read keeps its channel until it has passed, an unblocked one frees it;\n"
                "                              not with --resweep [off]\n");
    fprintf(fp, "   --enrich | --deplete       accept on-target reads and unblock off-target ones | the other way round\n");
    fprintf(fp, "   --margin FLOAT             cost per query event by which one class must beat the other; nobody has measured a good value:\n"
                "                              no default\n");
    fprintf(fp, "   --by-name                  with --targets: column 4 of the BED file names each interval's group (at most 1023 names); lines gain\n"
                "                              tg:Z:<group of the read's best column, * for none> gm:f:<(runner-up - best) / events>, the summary\n"
                "                              one line per group; decisions stay the class decision's [off]\n");
    fprintf(fp, "   --quota INT                with --by-name --enrich: every named group wants INT accepted reads.  A group that has them is\n"
                "                              closed from the next tick on: its columns count as off target, so its reads are unblocked (one\n"
                "                              sfa_session_open_classes call per tick in place of the class call; nothing is uploaded when a\n"
                "                              group closes).  A tick decides under the groups open at its start, so a group may overshoot by the\n"
                "                              reads accepted in its closing tick.  Lines gain og:Z:<open group of the read's best on-target\n"
                "                              column, * for none>, the trace `close` lines, the summary quota= and closed_at= [off]\n");
    fprintf(fp, "   --depth-cap INT            with --targets --enrich (mask targets: not with --by-name / --quota): stop asking for reads over\n"
                "                              positions that are covered INT times.  At the end of a tick every read accepted in it (ac:A:A) adds\n"
                "                              the target interval of its PAF line to a depth track on the device, all in one\n"
                "                              sfa_session_coverage_add call; from the next tick on a target column whose coordinate has depth >=\n"
                "                              INT counts as off target.  The interval is the aligned window of the decided prefix, not the whole\n"
                "                              molecule.  The trace gains `cover` lines, the summary the open columns and the bases added [off]\n");
    fprintf(fp, "   --group-cap INT            with --targets --by-name --enrich (optionally --quota; not with --depth-cap, --deplete, --resweep): a\n"
                "                              named group stops asking for reads, column by column, where it is covered INT times.  One\n"
                "                              sfa_session_open_classes call per tick decides (lines gain og:Z:); at the end of a tick the accepted\n"
                "                              reads' intervals go into one sfa_session_coverage_add call, and from the next tick on a column whose\n"
                "                              coordinate has depth >= INT belongs to the background.  The trace gains `cover` lines and\n"
                "                              `full group=NAME` when every column of a group is capped, the summary a depth line per group [off]\n");
    fprintf(fp, "   --lead INT                 with --targets (mask targets: not with --by-name / --quota / --group-cap; allowed with --depth-cap and\n"
                "                              --truth): the INT bases in front of every target, in the read's direction, count as on target --\n"
                "                              below its begin for a '+' read, above its end for a '-' read (sfa_session_targets_reach).  With\n"
                "                              --depth-cap a lead-in closes when the first base of the target it leads to is covered.  Schedule,\n"
                "                              decision rule and tags are unchanged; the summary gains the on-target columns [off]\n");
    fprintf(fp, "   --stranded                 with --lead: column 6 of the BED file is the target's strand, '+', '-' or '.' for both [both]\n");
    fprintf(fp, "   --group-lead INT           with --targets --by-name --enrich (optionally --quota, --group-cap, --truth; not with --lead,\n"
                "                              --depth-cap, --deplete): the INT bases in front of every named target, in the read's direction, carry\n"
                "                              the label of the target the read reaches first (sfa_session_target_groups_reach); the mask gets the\n"
                "                              same lead.  With --group-cap a lead-in closes when the first base of the target it leads to is\n"
                "                              covered.  Lines, tags and trace are --by-name's; the summary gains the labelled columns [off]\n");
    fprintf(fp, "   --group-stranded           with --group-lead: column 6 of the BED file is the target's strand, '+', '-' or '.' for both [both]\n");
    fprintf(fp, "   --truth FILE.paf           with --targets: check every decision against where the read came from -- a PAF file, column 1 the\n"
                "                              read id, 6 the contig (* for a read that belongs nowhere), 8 and 9 begin and end; a read that\n"
                "                              shares a base with a target is truly on target.  Lines gain tt:A:<true class T|O, N: not in the\n"
                "                              file> tv:A:<verdict of tc: C correct, W wrong, N> and with --by-name tn:Z:<true group> gv:A:<C|W|N>,\n"
                "                              the trace `verdict` lines, the summary `truth:` lines.  Changes no decision [off]\n");
    fprintf(fp, "   --trace FILE               write the schedule's trace (take / send / hold / decide lines) to FILE [off]\n");
    fprintf(fp, "   --pace yes|no              sleep so that tick t does not start before t x chunk-samples / sampling_rate seconds;\n"
                "                              changes the timing report on stderr only, never the output [no]\n\n"
                "output: PAF as dtw prints it, then ne:i:<query events at the decision> ns:i:<samples sent> dc:A:<E|F|R>\n");
}

}  // namespace

RealtimeOpt parse_realtime_options(int argc, char **argv) {
    RealtimeOpt r;
    Opt &o = r.o;
    FILE *fp_help = stderr;
    int c, li = 0;
    bool secondary = false;
    const char *recal = nullptr, *candidates = nullptr, *margin = nullptr, *quota = nullptr, *depth_cap = nullptr, *group_cap = nullptr, *lead = nullptr, *group_lead = nullptr;
    bool enrich = false, deplete = false;
    while ((c = getopt_long(argc, argv, "p:q:t:v:o:ahV", kRealtimeOptions, &li)) >= 0) {
        switch (c) {
            case 't': o.threads = atoi(optarg); if (o.threads < 1) die("Number of threads should larger than 0."); break;
            case 'v': o.verbosity = atoi(optarg); break;
            case 'V': fprintf(stdout, "sigfish-amd %s\n", sfa_version()); exit(EXIT_SUCCESS);
            case 'h': fp_help = stdout; break;
            case 'p': o.prefix = atoi(optarg); break;
            case 'q': o.query = atoi(optarg); if (o.query < 1) die("Query size should larger than 0."); break;
            case 'o': if (strcmp(optarg, "-") != 0 && !freopen(optarg, "wb", stdout)) die(std::string("failed to write the output to file ") + optarg); break;
            case 'a': o.flag |= F_SAM; break;
            case O_KMER_MODEL: o.model_file = optarg; break;
            case O_RNA: o.flag |= F_RNA; break;
            case O_DTW_STD: o.flag |= F_DTW; break;
            case O_INVERT: o.flag |= F_INV; break;
            case O_FROM_END: o.flag |= F_END; break;
            case O_SECONDARY: secondary = yes_or_no(optarg, "secondary"); break;
            case O_RANKS: o.ranks = atoi(optarg); break;
            case O_PORE:
                o.pore = optarg;
                if (strcmp(optarg, "r9") && strcmp(optarg, "r10") && strcmp(optarg, "rna004")) die("Pore model should be r9, r10 or rna004");
                if (!strcmp(optarg, "r10")) { o.flag |= F_R10; o.pore_flag = 1; }
                if (!strcmp(optarg, "rna004")) { o.flag |= F_RNA | F_R10; o.pore_flag = 2; }
                break;
            case O_DEVICE: parse_device_list(optarg, &o.devices); break;
            case O_CHANNELS: r.channels = atoi(optarg); if (r.channels < 1) die("--channels should be larger than 0"); break;
            case O_CHUNK_SAMPLES: r.chunk_samples = parse_num(optarg); if (r.chunk_samples < 1 || r.chunk_samples > (1 << 20)) die("--chunk-samples should be 1..1048576"); break;
            case O_NORM_EVENTS: r.norm_events = atoi(optarg); if (r.norm_events < 0) die("--norm-events should be 25..q"); break;
            case O_MIN_EVENTS: r.min_events = atoi(optarg); if (r.min_events < 0) die("--min-events should not be negative"); break;
            case O_MIN_MAPQ: r.min_mapq = atoi(optarg); break;
            case O_PACE: r.pace = yes_or_no(optarg, "pace"); break;
            case O_RECALIBRATE: recal = optarg; break;
            case O_RECALIBRATE_AT_END: r.recal_at_end = true; break;
            case O_RESWEEP: r.resweep = true; break;
            case O_CANDIDATES: candidates = optarg; break;
            case O_SPREAD: r.spread = true; break;
            case O_TARGETS: r.targets = optarg; break;
            case O_ENRICH: enrich = true; break;
            case O_DEPLETE: deplete = true; break;
            case O_MARGIN: margin = optarg; break;
            case O_BY_NAME: r.by_name = true; break;
            case O_QUOTA: quota = optarg; break;
            case O_TRUTH: r.truth = optarg; break;
            case O_DEPTH_CAP: depth_cap = optarg; break;
            case O_GROUP_CAP: group_cap = optarg; break;
            case O_LEAD: lead = optarg; break;
            case O_STRANDED: r.stranded = true; break;
            case O_GROUP_LEAD: group_lead = optarg; break;
            case O_GROUP_STRANDED: r.group_stranded = true; break;
            case O_TRACE: r.trace = optarg; break;
            default: realtime_help(stderr, r); exit(EXIT_FAILURE);
        }
    }
    if (argc - optind != 2 || fp_help == stdout) {
        realtime_help(fp_help, r);
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    o.fasta = argv[optind];
    o.blow5 = argv[optind + 1];
    // what a session cannot do, by name (sfa_session_create would refuse some of it later, with a device open)
    if (o.flag & F_DTW) die("realtime: --dtw-std is not available: a session extends the subsequence DTW");
    if (o.flag & F_END) die("realtime: --from-end is not available: the end of a read is not known while it arrives");
    if (o.prefix < 0) die("realtime: -p -1 (automatic query start) is not available: -p must be >= 0");
    if (o.flag & F_SAM) die("realtime: --sam is not available: sessions keep no warp path");
    if (secondary) die("realtime: --secondary yes is not available: sessions keep one row per slot; --candidates N prints a slot's candidate list");
    if (candidates) {
        char *e = nullptr;
        const long v = strtol(candidates, &e, 10);
        if (e == candidates || *e || v < 1 || v > 4) die("realtime: --candidates should be 1..4");
        r.candidates = static_cast<int32_t>(v);
    }
    if (o.ranks != 0) die("realtime: --ranks is not available: a replay is one process on one device");
    if (o.devices.size() != 1 && !r.spread) die("realtime: --device takes exactly one GPU: a session's rows live on one device (--spread deals the channels over a list)");
    if ((o.flag & F_INV) && !(o.flag & F_RNA)) die("Inversion is only available for RNA.");
    if ((o.flag & F_RNA) && !(o.flag & F_INV) && !r.resweep) die("realtime: --rna needs --invert (or --resweep): without it the query rows are the events reversed, and a session cannot take new events as row 0");
    // adaptive sampling: everything that needs no file
    if (r.targets.empty() && (enrich || deplete || margin)) die("realtime: --enrich, --deplete and --margin belong to --targets FILE.bed");
    if (r.targets.empty() && r.by_name) die("realtime: --by-name belongs to --targets FILE.bed");
    if (r.targets.empty() && !r.truth.empty()) die("realtime: --truth checks target decisions: pass --targets FILE.bed with --enrich or --deplete and --margin with it");
    if (group_lead || r.group_stranded) {
        if (!r.by_name) die("realtime: --group-lead and --group-stranded widen named groups in the read's direction: pass --targets FILE.bed --by-name --enrich --margin X with them");
        if (lead || r.stranded) die("realtime: --group-lead and --lead are two leads: with --by-name pass --group-lead alone (the mask gets the same lead)");
        if (depth_cap) die("realtime: --group-lead with --depth-cap is not built: --depth-cap is for mask targets; the cap of named groups is --group-cap");
        if (deplete) die("realtime: --group-lead with --deplete is not built: use --enrich");
        if (!group_lead) die("realtime: --group-stranded belongs to --group-lead: pass --group-lead N (0 for no lead-in) with it");
        char *e = nullptr;
        const long long v = strtoll(group_lead, &e, 10);
        if (e == group_lead || *e || v < 0 || v > (1 << 30)) die("realtime: --group-lead should be an integer 0..1073741824");
        r.group_lead = static_cast<int32_t>(v);
    }
    if (lead || r.stranded) {
        if (r.targets.empty()) die("realtime: --lead and --stranded widen targets in the read's direction: pass --targets FILE.bed with --enrich or --deplete and --margin with them");
        if (r.by_name || quota || group_cap) die("realtime: --lead and --stranded are for mask targets: with --by-name / --quota / --group-cap they are not built (groups work from labels)");
        if (!lead) die("realtime: --stranded belongs to --lead: pass --lead N (0 for no lead-in) with it");
        char *e = nullptr;
        const long long v = strtoll(lead, &e, 10);
        if (e == lead || *e || v < 0 || v > (1 << 30)) die("realtime: --lead should be an integer 0..1073741824");
        r.lead = static_cast<int32_t>(v);
    }
    if (quota) {
        if (!r.by_name) die("realtime: --quota counts accepted reads per named group: pass --targets FILE.bed --by-name --enrich with it");
        if (deplete) die("realtime: --quota is not available with --deplete (a closed group's reads would be accepted): use --enrich");
        char *e = nullptr;
        const long long v = strtoll(quota, &e, 10);
        if (e == quota || *e || v < 1) die("realtime: --quota should be an integer >= 1 (leave the option out for no quota)");
        r.quota = v;
    }
    if (group_cap) {  // (a session of this front end always carries start columns, as for --depth-cap)
        char *e = nullptr;
        const long long v = strtoll(group_cap, &e, 10);
        if (e == group_cap || *e || v < 1 || v > (1 << 30)) die("realtime: --group-cap should be an integer 1..1073741824 (leave the option out for no cap)");
        if (deplete) die("realtime: --group-cap with --deplete is not built: a covered position would turn on target; use --enrich");
        if (!r.by_name || !enrich) die("realtime: --group-cap closes the covered columns of named groups: pass --targets FILE.bed --by-name --enrich --margin X with it");
        if (depth_cap) die("realtime: --group-cap and --depth-cap are two caps over one depth track: pass one of them (--depth-cap is for mask targets)");
        if (r.resweep) die("realtime: --group-cap is not available with --resweep: a resweep session has no target groups");
        r.group_cap = static_cast<int32_t>(v);
    }
    if (depth_cap) {  // (a session of this front end always carries start columns: the interval's other end is there)
        char *e = nullptr;
        const long long v = strtoll(depth_cap, &e, 10);
        if (e == depth_cap || *e || v < 1 || v > (1 << 30)) die("realtime: --depth-cap should be an integer 1..1073741824 (leave the option out for no cap)");
        if (deplete) die("realtime: --depth-cap with --deplete is not built: a covered position would turn on target; use --enrich");
        if (r.targets.empty() || !enrich) die("realtime: --depth-cap closes covered target positions: pass --targets FILE.bed --enrich --margin X with it");
        if (r.by_name || quota) die("realtime: --depth-cap is for mask targets: with --by-name / --quota it is not built (per-group base quotas)");
        r.depth_cap = static_cast<int32_t>(v);
    }
    if (!r.targets.empty()) {
        if (enrich == deplete) die("realtime: --targets needs exactly one of --enrich and --deplete");
        if (!margin) die("realtime: --targets needs --margin: nobody has measured a good value, there is no default");
        char *e = nullptr;
        r.margin = strtof(margin, &e);
        if (e == margin || *e || !(r.margin >= 0.0f) || !std::isfinite(r.margin)) die("realtime: --margin should be a number >= 0");
        if (r.resweep) die("realtime: --targets is not available with --resweep: a resweep session's carried row belongs to the reversed query");
        r.target_mode = enrich ? 0 : 1;
    }
    if (r.norm_events < 0) r.norm_events = o.query;
    if (r.min_events < 0) r.min_events = o.query;
    if (r.norm_events < 25 || r.norm_events > o.query) die("realtime: --norm-events should be 25..q (the value of -q)");
    if (recal && !strcmp(recal, "double")) {
        int32_t at[sfa::kRecalMaxPoints];
        r.recal_at.assign(at, at + sfa::recal_double(r.norm_events, o.query, at));
    } else if (recal) {
        for (const char *p = recal; *p;) {
            char *e = nullptr;
            const long v = strtol(p, &e, 10);
            if (e == p || (*e && *e != ',') || v < 0 || v > INT32_MAX) die("realtime: --recalibrate takes 'double' or a comma separated list of window lengths");
            if (r.recal_at.size() > static_cast<size_t>(sfa::kRecalMaxPoints)) break;  // (refused below)
            r.recal_at.push_back(static_cast<int32_t>(v));
            p = *e ? e + 1 : e;
            if (*e && !*p) die("realtime: --recalibrate takes 'double' or a comma separated list of window lengths");
        }
        if (r.recal_at.empty()) die("realtime: --recalibrate takes 'double' or a comma separated list of window lengths");
    }
    if (const char *why = sfa::recal_list_error(r.recal_at.data(), static_cast<int64_t>(r.recal_at.size()), r.norm_events, o.query))
        die(std::string("realtime: --recalibrate: ") + why + " (the list must ascend from above --norm-events up to q, at most 32 points)");
    // --recalibrate-at-end is about the line a read ends with, whichever way it ends: a read that ends short gets the session's
    // end-of-read window (SFA_RECAL_AT_END), a read that ends full must be normalised over [p, p + q), so q joins the points
    if (r.recal_at_end && o.query > r.norm_events && (r.recal_at.empty() || r.recal_at.back() != o.query)) {
        r.recal_at.push_back(o.query);
        if (const char *why = sfa::recal_list_error(r.recal_at.data(), static_cast<int64_t>(r.recal_at.size()), r.norm_events, o.query))
            die(std::string("realtime: --recalibrate with --recalibrate-at-end (which adds q as the last point): ") + why);
    }
    o.ranks = 1;
    return r;
}

Opt parse_options(int argc, char **argv) {
    Opt o;
    FILE *fp_help = stderr;
    int c, li = 0;
    while ((c = getopt_long(argc, argv, "p:q:t:B:K:v:o:w:ahV", kLongOptions, &li)) >= 0) {
        switch (c) {
            case 'B': o.batch_bytes = parse_num(optarg); if (o.batch_bytes <= 0) die("Maximum number of bytes should be larger than 0."); break;
            case 'K': o.batch_size = atoi(optarg); if (o.batch_size < 1) die("Batch size should larger than 0."); break;
            case 't': o.threads = atoi(optarg); if (o.threads < 1) die("Number of threads should larger than 0."); break;
            case 'v': o.verbosity = atoi(optarg); break;
            case 'V': fprintf(stdout, "sigfish-amd %s\n", sfa_version()); exit(EXIT_SUCCESS);
            case 'h': fp_help = stdout; break;
            case 'p': o.prefix = atoi(optarg); break;
            case 'q': o.query = atoi(optarg); if (o.query < 1) die("Query size should larger than 0."); break;
            case 'o': if (strcmp(optarg, "-") != 0 && !freopen(optarg, "wb", stdout)) die(std::string("failed to write the output to file ") + optarg); break;
            case 'a': o.flag |= F_SAM; break;
            case 'w': break;  // parsed and unused by the reference as well
            case O_KMER_MODEL: o.model_file = optarg; break;
            case O_RNA: o.flag |= F_RNA; break;
            case O_DEBUG_BREAK: o.debug_break = atoi(optarg); break;
            case O_DTW_STD: o.flag |= F_DTW; break;
            case O_INVERT: o.flag |= F_INV; break;
            case O_FULL_REF: o.flag |= F_REF; break;
            case O_FROM_END: o.flag |= F_END; break;
            case O_PROFILE_CPU: if (yes_or_no(optarg, "profile-cpu")) o.flag |= F_PRF; else o.flag &= ~F_PRF; break;  // src/dtw_main.c:213-214
            case O_ACCEL:  // src/dtw_main.c:215-220: the reference falls back to work_db(dtw_single) on its CPU; there is none here
                if (!yes_or_no(optarg, "accel"))
                    die("--accel=no: this build has no CPU alignment path (the stage only exists as gfx950 kernels); "
                        "run the reference binary for a CPU run, or drop the option");
                break;
            case O_SECONDARY:  // src/dtw_main.c:207-208 parses it; here it prints the reference's own candidate list (other values: no effect)
                if (!strcmp(optarg, "yes")) o.secondary = true;
                else if (!strcmp(optarg, "no")) o.secondary = false;
                break;
            case O_METH_MODEL: break;  // dead option of the reference (--meth-model): parsed, no effect
            case O_PORE:
                o.pore = optarg;
                if (strcmp(optarg, "r9") && strcmp(optarg, "r10") && strcmp(optarg, "rna004")) die("Pore model should be r9, r10 or rna004");
                if (!strcmp(optarg, "r10")) { o.flag |= F_R10; o.pore_flag = 1; }
                if (!strcmp(optarg, "rna004")) { o.flag |= F_RNA | F_R10; o.pore_flag = 2; }
                break;
            case O_DEVICE: parse_device_list(optarg, &o.devices); break;
            case O_HOST_EVENTS: o.host_events = true; break;
            case O_SECONDARY_STRIPS: o.secondary_strips = true; break;
            case O_HOST_PATHS: case O_DEVICE_PATHS: o.device_paths = c == O_DEVICE_PATHS; break;
            case O_HOST_PARSE: case O_GPU_PARSE: o.gpu_parse = c == O_GPU_PARSE; break;
            case O_RANKS: o.ranks = atoi(optarg); if (o.ranks < 1 || o.ranks > 64) die("--ranks should be 1..64"); break;
            case O_SHARD:
                if (sscanf(optarg, "%d/%d", &o.shard_r, &o.shard_n) != 2 || o.shard_n < 1 || o.shard_r < 0 || o.shard_r >= o.shard_n)
                    die("--shard takes r/G with 0 <= r < G");
                break;
            case O_READ_RANGE: {
                char *e = nullptr;
                o.range_a = strtoll(optarg, &e, 10);
                if (e == optarg || *e != ':' || o.range_a < 0) die("--read-range takes A:B (records A up to, not including, B; B may be omitted)");
                ++e;  // past the colon
                o.range_b = *e ? strtoll(e, &e, 10) : -1;
                if (*e || (o.range_b >= 0 && o.range_b < o.range_a)) die("--read-range takes A:B (records A up to, not including, B; B may be omitted)");
                break;
            }
            case O_NO_HEADER: o.no_header = true; break;
            case O_RANK_BUFFER: o.rank_buffer = parse_num(optarg); if (o.rank_buffer < 0) die("--rank-buffer should not be negative"); break;
            case O_STREAMS: o.streams = atoi(optarg); if (o.streams < 1 || o.streams > 8) die("--streams should be 1..8"); break;
            default: help(stderr, o); exit(EXIT_FAILURE);
        }
    }
    if (argc - optind != 2 || fp_help == stdout) {
        help(fp_help, o);
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    o.fasta = argv[optind];
    o.blow5 = argv[optind + 1];
    // same order of checks as src/dtw_main.c:248-277 (before RNA auto-detection)
    if (!(o.flag & F_RNA)) {
        if (o.flag & F_DTW) die("DTW is only available for RNA.");
        if (o.flag & F_INV) die("Inversion is only available for RNA.");
        if (o.flag & F_REF) die("--full-ref is only available for RNA.");
    }
    if (o.prefix < 0) {
        if (!(o.flag & F_RNA)) die("DNA does not support auto query start detection.");
        if (o.flag & F_INV) die("Inversion is not compatible with auto query start detection.");
        if (o.flag & F_END) die("Mapping from query end is not compatible with auto query start detection.");
    }

    if (o.shard_n > 1 && (o.range_a > 0 || o.range_b >= 0)) die("--shard and --read-range exclude each other");
    if (o.secondary_strips && !o.secondary) die("--secondary-strips needs --secondary yes");
    if (o.secondary && o.query > 2048 && !o.secondary_strips) die("--secondary yes supports -q up to 2048");
    if (o.ranks == 0) {  // one process per DISTINCT device of the list; a device listed twice is two contexts of one process
        std::vector<int> d = o.devices;
        std::sort(d.begin(), d.end());
        o.ranks = static_cast<int>(std::unique(d.begin(), d.end()) - d.begin());
    }
    if (o.ranks > 1) {
        if (o.shard_n > 1 || o.range_a > 0 || o.range_b >= 0) die("--ranks shards the whole file: it cannot be combined with --shard or --read-range");
        if (o.debug_break >= 0) die("--debug-break counts the batches of one process: use --ranks 1 with it");
    }
    return o;
}

}  // namespace cli
