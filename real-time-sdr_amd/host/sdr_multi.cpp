// sdr_multi.cpp -- multi-channel receiver CLI over the engine of include/sdr_multi.h (the reference
// program's three stage threads over nch channels, project.cpp:134-136).
//
//   sdr_multi NCH [--mode 0-3] [--in FILE|-] [--out PREFIX] [--fast] [--cus N] [--tune FILE] [--meter [--rf]]
//             [--deemph US] [--blend] [--demod ref|phase] [--rds-decode [--rds-correct N] [--rds-clock ref|track] [--rds-soft L] [--rds-carrier ref|quad]]
//   sdr_multi NROWS --scan [--mode 0-3] [--in FILE|-] [--out PREFIX] [--scan-blocks B] [--step K] [--thr DB]
//   sdr_multi NCH --wide W [--shift S] --tune FILE ...          (the receiver on wide captures)
//   sdr_multi NWIDE --wide W [--shift S] --scan ...             (the scan of wide captures)
//
// Input: u8 I/Q, block after block, each block NCH rows of 2*block_iq bytes (channel after
// channel: the [block][channel][bytes] layout of bench.py). Output: PREFIX.pcm -- per block NCH
// rows of 2*n_audio int16 (L/R interleaved per channel, stereo.cpp:100-111) -- and PREFIX.rds, the
// RDS text of every channel ("ch <c>: " + parse()'s lines, rds_utilities.cpp:172-199). --cus N: the
// two consumers' PLLs on CUs [0, N) (persistent launches when the input is a regular file), 0: no
// CU masks. --tune FILE: shared captures (include/sdr_multi_tuned.h) -- FILE is text, one "src khz"
// pair per line, NCH lines: channel c listens to capture row src and to the station khz kHz off its
// centre; the input then holds max(src) + 1 rows per block instead of NCH. A summary line goes to
// stderr. --scan: the band scan (include/sdr_scan_run.h) instead of the receiver -- the first B blocks
// (default 4) of NROWS capture rows, the --tune input layout, are scanned and the stations found are
// written to PREFIX.stations in the --tune format; --step K: the station grid in kHz (default 100),
// --thr DB: the threshold over the floor (default 10). `sdr_multi <n> --tune PREFIX.stations` with the
// n the scan printed then receives them. --meter: the reception meter (include/sdr_multi_meter.h) beside the
// receiver, with or without --tune -- PREFIX.meter (per block NCH rows of 64 bytes, sdr_meter_row) and
// PREFIX.status (per channel the run's mean readings and its STEREO / RDS / OFFTUNE / DEAD_AIR flags);
// the PCM and the RDS text are those of a run without it. --rf (needs --meter, not with --fast): the RF
// readings too (SDR_FLAG_IF_ENVELOPE, sdr_meter_rf) -- PREFIX.rf (per block NCH rows of 32 bytes,
// sdr_meter_rf_row) and PREFIX.rfstatus (per channel the run's level in dBFS, envelope ripple, C/N, deepest
// fade and crest, and WEAK); every other file is that of a run without it. --deemph US (0, 50 or 75) and --blend (needs
// --meter): the audio finishing stage (include/sdr_multi_audio.h) -- PREFIX.audio, in the layout of PREFIX.pcm,
// holds the audio de-emphasised with US microseconds (75 when only --blend is given) and, with --blend,
// blended to mono where the meter finds no pilot; every other file is that of a run without them.
// --wide W (4, 8 or 10; --shift S: the splitter's output shift, default 14, 15, 16): the input is wide
// signed 8-bit I/Q at W * rf_Fs (include/sdr_multi_wide.h, include/sdr_wide_scan.h) -- per block, rows of
// 2*W*block_iq int8 bytes, each cut by the wideband splitter into 2W-1 capture rows; capture row w*(2W-1)+r
// is row r of wide stream w. With --tune the input holds ceil((max(src) + 1) / (2W-1)) wide streams per
// block; with --scan NWIDE wide streams are scanned and PREFIX.stations names the capture rows, so
// `sdr_multi <n> --wide W --tune PREFIX.stations` receives what `sdr_multi NWIDE --wide W --scan` found.
// The summary line counts the wide bytes read; clip counts go to stderr when any are non-zero.
// --wide-format s16 (with --wide; s8 is the default): the wide input is little-endian int16 I/Q, rows of
// 4*W*block_iq bytes (include/sdr_multi_wide16.h), cut by the 16-bit splitter. --shift S is then 1-33 (default 22,
// 23, 24) and holds for every row; --wide-gain auto[:TARGET] instead takes a shift per row from block 0's peaks
// (target 1-127, default 90). A receiver run also writes PREFIX.wide, one line "stream row shift peak clips" per
// capture row.
// --demod phase: the phase discriminator (SDR_FLAG_PHASE_DEMOD, include/sdr_amd.h) instead of the
// reference's (--demod ref, the default): the audio of a loud station no longer folds, and with --meter every
// PREFIX.status line also ends with the run's peak deviation and mean offset in kHz. Not with --fast.
// --rds-decode: the RDS group decoder (include/sdr_amd.h, sdr_rds_*; mode 0) behind the RDS thread's bits --
// PREFIX.groups, one line per group ("ch <c> bits <n> AAAA BBBB CCCC DDDD", "----" for a block that was not
// received, a trailing "*" on a corrected one), and PREFIX.radio, per channel PI, PTY, TP/TA/MS, PS, RadioText,
// clock time, AF, the groups by type, block counts, BLER, slips and syncs; --rds-correct N (0-5, default 2):
// the longest error burst it corrects. Every other file is that of a run without it.
// --rds-clock track (with --rds-decode): the decoder's bits come from the RDS symbol tracker (sdr_rds_track_*: a
// continuous bit clock and a correlator over the whole bit) instead of the per-block clock recovery (ref, the
// default); PREFIX.groups and PREFIX.radio are made from them, PREFIX.radio gains a "clock:" line per channel,
// and PREFIX.rds and every other file stay those of a run without it.
// --rds-soft L (1-6, with --rds-clock track): soft decisions -- the tracker also writes every bit's reliability and
// the decoder first searches a failing block over the flips of its L least reliable raw decisions
// (sdr_rds_groups_soft); in PREFIX.groups a block placed that way ends in "~", PREFIX.radio gains a "soft:" line
// per channel, and every other file stays that of a run without it.
// --rds-carrier quad (with --rds-clock track): coherent RDS -- the RDS chain also runs with the quadrature of its
// carrier (SDR_FLAG_RDS_QUAD), the carrier-phase derotator (sdr_rds_carrier_*) turns both branches' rows onto one
// axis and the tracker reads those rows instead of rds_clean (ref, the default); PREFIX.groups and PREFIX.radio
// are made from the new bits, PREFIX.radio gains a "carrier:" line per channel, and every other file stays that
// of a run without it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_audio.h"
#include "sdr_multi_meter.h"
#include "sdr_multi_rds.h"
#include "sdr_multi_tuned.h"
#include "sdr_multi_wide.h"
#include "sdr_multi_wide16.h"
#include "sdr_scan_run.h"
#include "sdr_wide_scan.h"

namespace {
[[noreturn]] void usage() {
    std::fprintf(stderr, "usage: sdr_multi NCH [--mode 0-3] [--in FILE|-] [--out PREFIX] [--fast] [--cus N] "
                         "[--tune FILE] [--meter [--rf]] [--deemph US] [--blend] [--demod ref|phase] [--rds-decode [--rds-correct N] [--rds-clock ref|track] [--rds-soft L] [--rds-carrier ref|quad]]\n"
                         "       sdr_multi NROWS --scan [--mode 0-3] [--in FILE|-] [--out PREFIX] [--scan-blocks B] "
                         "[--step K] [--thr DB]\n"
                         "       sdr_multi NCH --wide W [--shift S] --tune FILE ...   |   sdr_multi NWIDE --wide W [--shift S] --scan ...\n"
                         "  --tune FILE: NCH lines \"src khz\"; the input holds max(src)+1 capture rows per block\n"
                         "  --meter: also write PREFIX.meter (64-byte readings per channel and block) and PREFIX.status\n"
                         "  --rf: also write PREFIX.rf (32-byte RF readings per channel and block) and PREFIX.rfstatus (level in\n"
                         "            dBFS, envelope ripple, C/N, fade, crest per channel); needs --meter, not with --fast\n"
                         "  --deemph US: also write PREFIX.audio, the PCM de-emphasised with 0, 50 or 75 microseconds\n"
                         "  --blend: PREFIX.audio blended to mono where the meter finds no pilot (needs --meter)\n"
                         "  --demod phase: the phase discriminator (fm_demod in radians, no fold above if_Fs/4 of deviation;\n"
                         "            PREFIX.status gains peak_khz and offset_khz); ref (default): the reference's; not with --fast\n"
                         "  --rds-decode: also write PREFIX.groups (one line per RDS group) and PREFIX.radio (PI, PS, RadioText,\n"
                         "            clock time, AF, block error rate per channel); --rds-correct N: bursts up to N bits (0-5, default 2)\n"
                         "  --rds-clock track: the decoder's bits from the symbol tracker (a continuous bit clock, a correlator over\n"
                         "            the whole bit) instead of the per-block clock recovery (ref, default); needs --rds-decode, mode 0\n"
                         "  --rds-soft L: soft decisions, a failing block is searched over the flips of its L (1-6) least reliable\n"
                         "            bits before the burst table; needs --rds-clock track\n"
                         "  --rds-carrier quad: coherent RDS, the chain's quadrature branch too and both turned onto one axis by the\n"
                         "            carrier phase found in them, for the tracker (ref, default: rds_clean alone); needs --rds-clock track\n"
                         "  --scan: write the stations of NROWS capture rows to PREFIX.stations (the --tune format)\n"
                         "  --wide W: the input is wide int8 I/Q at W (4, 8, 10) times rf_Fs, rows of 2*W*block_iq bytes, each\n"
                         "            split into 2W-1 capture rows (--shift S: output shift 1-24); needs --tune or --scan\n"
                         "  --wide-format s8|s16: with --wide; s16: int16 I/Q, rows of 4*W*block_iq bytes, --shift 1-33, or\n"
                         "            --wide-gain auto[:TARGET] (a shift per row from block 0's peaks, target 1-127, default 90);\n"
                         "            a receiver run also writes PREFIX.wide (stream, row, shift, peak, clips per capture row)\n");
    std::exit(1);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) usage();
    sdr_multi_opts o{};
    o.nch = std::atoi(argv[1]);
    o.pll_cus = 64;
    std::string in = "-", out = "sdr_multi", tune_path;
    if (o.nch <= 0) usage();
    bool scan = false, meter = false, blend = false, finish = false, rds_decode = false, rds_correct = false, rds_clock_set = false;
    int rds_clock = SDR_MULTI_RDS_CLOCK_REF, rds_soft = 0;
    bool rds_quad = false;
    sdr_rds_opts ro{};
    sdr_rds_opts_default(&ro);
    int wide_w = 0, wide_shift = 0;
    bool wide_format_set = false, wide_gain_set = false;
    sdr_wide_fmt wf{};
    sdr_audio_opts ao{};
    sdr_audio_opts_default(&ao);
    sdr_scan_run_opts so{};
    sdr_scan_opts_default(&so.pick);
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--mode" && i + 1 < argc) o.mode = std::atoi(argv[++i]);
        else if (a == "--in" && i + 1 < argc) in = argv[++i];
        else if (a == "--out" && i + 1 < argc) out = argv[++i];
        else if (a == "--cus" && i + 1 < argc) o.pll_cus = std::atoi(argv[++i]);
        else if (a == "--tune" && i + 1 < argc) tune_path = argv[++i];
        else if (a == "--scan") scan = true;
        else if (a == "--wide" && i + 1 < argc) {
            wide_w = std::atoi(argv[++i]);
            if (wide_w != 4 && wide_w != 8 && wide_w != 10) usage();
        }
        else if (a == "--shift" && i + 1 < argc) {
            wide_shift = std::atoi(argv[++i]);
            if (wide_shift < 1 || wide_shift > 33) usage();   // (above 24: with --wide-format s16 only, below)
        }
        else if (a == "--wide-format" && i + 1 < argc) {
            const std::string f = argv[++i];
            if (f == "s16") wf.format = SDR_WIDE_S16;
            else if (f == "s8") wf.format = SDR_WIDE_S8;
            else usage();
            wide_format_set = true;
        }
        else if (a == "--wide-gain" && i + 1 < argc) {
            const std::string g = argv[++i];
            if (g == "fixed") wf.gain = SDR_WIDE_GAIN_FIXED;
            else if (g.rfind("auto", 0) == 0 && (g.size() == 4 || g[4] == ':')) {
                wf.gain = SDR_WIDE_GAIN_AUTO;
                if (g.size() > 4) {
                    char* end = nullptr;
                    const long t = std::strtol(g.c_str() + 5, &end, 10);
                    if (g.size() == 5 || *end || t < 1 || t > 127) usage();
                    wf.target = (int)t;
                }
            }
            else usage();
            wide_gain_set = true;
        }
        else if (a == "--meter") meter = true;
        else if (a == "--rf") o.flags |= SDR_FLAG_IF_ENVELOPE;
        else if (a == "--blend") blend = finish = true;
        else if (a == "--deemph" && i + 1 < argc) {
            const std::string us = argv[++i];
            if (us != "0" && us != "50" && us != "75") usage();
            ao.tau_us = (float)std::atoi(us.c_str());
            finish = true;
        }
        else if (a == "--scan-blocks" && i + 1 < argc) so.max_blocks = std::atoi(argv[++i]);
        else if (a == "--step" && i + 1 < argc) so.pick.step_khz = std::atoi(argv[++i]);
        else if (a == "--thr" && i + 1 < argc) so.pick.thr_db = (float)std::atof(argv[++i]);
        else if (a == "--rds-decode") rds_decode = true;
        else if (a == "--rds-correct" && i + 1 < argc) {
            const std::string n = argv[++i];
            if (n.size() != 1 || n[0] < '0' || n[0] > '5') usage();
            ro.max_burst = n[0] - '0';
            rds_correct = true;
        }
        else if (a == "--rds-clock" && i + 1 < argc) {
            const std::string c = argv[++i];
            if (c == "track") rds_clock = SDR_MULTI_RDS_CLOCK_TRACK;
            else if (c == "ref") rds_clock = SDR_MULTI_RDS_CLOCK_REF;
            else usage();
            rds_clock_set = true;
        }
        else if (a == "--rds-soft" && i + 1 < argc) {
            const std::string n = argv[++i];
            if (n.size() != 1 || n[0] < '1' || n[0] > '6') usage();
            rds_soft = n[0] - '0';
        }
        else if (a == "--rds-carrier" && i + 1 < argc) {
            const std::string c = argv[++i];
            if (c == "quad") rds_quad = true;
            else if (c == "ref") rds_quad = false;
            else usage();
        }
        else if (a == "--fast") o.flags |= SDR_FLAG_FAST_FRONTEND;
        else if (a == "--demod" && i + 1 < argc) {
            const std::string d = argv[++i];
            if (d == "phase") o.flags |= SDR_FLAG_PHASE_DEMOD;
            else if (d == "ref") o.flags &= ~SDR_FLAG_PHASE_DEMOD;
            else usage();
        }
        else usage();
    }
    if ((o.flags & SDR_FLAG_FAST_FRONTEND) && (o.flags & SDR_FLAG_PHASE_DEMOD)) usage();   // the MFMA front end has none
    if (const char* dev = std::getenv("SDR_DEVICE")) o.device = std::atoi(dev);
    o.in_path = in.c_str();
    o.out_prefix = out.c_str();
    if (blend && !meter) usage();
    if ((o.flags & SDR_FLAG_IF_ENVELOPE) && (!meter || (o.flags & SDR_FLAG_FAST_FRONTEND))) usage();   // the meter reads the row
    if ((rds_correct || rds_clock_set) && !rds_decode) usage();
    if (rds_soft && (!rds_decode || rds_clock != SDR_MULTI_RDS_CLOCK_TRACK)) usage();   // only the tracker has reliabilities
    if (rds_quad && (!rds_decode || rds_clock != SDR_MULTI_RDS_CLOCK_TRACK)) usage();   // the tracker reads the rotated rows
    if (rds_decode && (scan || !sdr_rds_mode_ok(o.mode))) usage();   // a scan demodulates nothing; modes 1-3 have no RDS bit clock
    if (wide_shift && !wide_w) usage();
    if ((wide_format_set || wide_gain_set) && !wide_w) usage();
    if (wf.format != SDR_WIDE_S16 && (wide_gain_set || wide_shift > 24)) usage();   // the s8 splitter has one shift, 1-24
    if (wf.gain == SDR_WIDE_GAIN_AUTO && wide_shift) usage();                       // one or the other
    if (wide_w && !scan && tune_path.empty()) usage();        // a wide run is always tuned
    if (scan && wide_w) {
        if (!tune_path.empty() || meter || finish) usage();
        const std::string list = out + ".stations";
        sdr_wide_scan_opts wo{};
        wo.nwide = o.nch;
        wo.W = wide_w;
        wo.shift = wide_shift;
        wo.mode = o.mode;
        wo.device = o.device;
        wo.in_path = o.in_path;
        wo.out_path = list.c_str();
        wo.max_blocks = so.max_blocks;
        wo.pick = so.pick;
        sdr_wide_scan_stats ws{};
        const int rc = wf.format == SDR_WIDE_S16 ? sdr_wide_scan_run_fmt(&wo, &wf, &ws) : sdr_wide_scan_run(&wo, &ws);
        if (rc != SDR_OK) {
            std::fprintf(stderr, "sdr_multi: %d %s\n", rc, ws.error);
            return 1;
        }
        std::fprintf(stderr, "sdr_multi: scan: %d stations in %d wide streams x %d rows (%lld segments per row)\n", ws.stations,
                     wo.nwide, 2 * wide_w - 1, ws.segments);
        if (ws.clips) std::fprintf(stderr, "sdr_multi: splitter: %lld output components clipped\n", ws.clips);
        return 0;
    }
    if (scan) {
        if (!tune_path.empty() || meter || finish) usage();   // a scan writes a tuning, it does not take one (nor does it demodulate)
        const std::string list = out + ".stations";
        so.nrows = o.nch;
        so.mode = o.mode;
        so.device = o.device;
        so.in_path = o.in_path;
        so.out_path = list.c_str();
        sdr_scan_run_stats ss{};
        const int rc = sdr_scan_run(&so, &ss);
        if (rc != SDR_OK) {
            std::fprintf(stderr, "sdr_multi: %d %s\n", rc, ss.error);
            return 1;
        }
        std::fprintf(stderr, "sdr_multi: scan: %d stations in %d rows (%lld segments per row)\n", ss.stations, so.nrows,
                     ss.segments);
        return 0;
    }
    sdr_multi_stats st{};
    std::vector<int32_t> src, khz;
    sdr_multi_tuning tune{};
    if (!tune_path.empty()) {
        FILE* tf = std::fopen(tune_path.c_str(), "r");
        if (!tf) {
            std::fprintf(stderr, "sdr_multi: cannot open %s\n", tune_path.c_str());
            return 1;
        }
        int a = 0, b = 0, extra = 0;
        while ((int)src.size() < o.nch && std::fscanf(tf, "%d %d", &a, &b) == 2) {
            src.push_back(a);
            khz.push_back(b);
            tune.nsrc = a + 1 > tune.nsrc ? a + 1 : tune.nsrc;
        }
        const bool more = std::fscanf(tf, "%d", &extra) == 1;
        std::fclose(tf);
        if ((int)src.size() != o.nch || more) {
            std::fprintf(stderr, "sdr_multi: %s must hold %d lines \"src khz\"\n", tune_path.c_str(), o.nch);
            return 1;
        }
        tune.src = src.data();
        tune.khz = khz.data();
    }
    const int wide_r = 2 * wide_w - 1;
    sdr_multi_wide wd{};
    std::vector<long long> clips, wide_peaks;
    std::vector<int> wide_shifts;
    if (wide_w) {
        wd.W = wide_w;
        wd.nwide = (tune.nsrc + wide_r - 1) / wide_r;
        wd.shift = wide_shift;
        clips.assign((size_t)(wd.nwide > 0 ? wd.nwide : 1) * wide_r, 0);
        wd.clips = clips.data();
        if (wf.format == SDR_WIDE_S16) {
            wide_shifts.assign(clips.size(), 0);
            wide_peaks.assign(clips.size(), 0);
            wf.shifts_out = wide_shifts.data();
            wf.peaks_out = wide_peaks.data();
        }
    }
    const int rows = wide_w ? wd.nwide : tune_path.empty() ? o.nch : tune.nsrc;
    sdr_meter_opts mo{};
    sdr_meter_opts_default(&mo);
    const sdr_multi_tuning* tp = tune_path.empty() ? nullptr : &tune;
    const sdr_multi_rds rd{ro.max_burst, ro.loss_blocks};
    const sdr_rds_soft_opts sq{ro.max_burst, ro.loss_blocks, rds_soft};
    sdr_rds_carrier_opts cq{};
    sdr_rds_carrier_opts_default(&cq);
    const bool s16 = wide_w && wf.format == SDR_WIDE_S16;
    const int rc = s16 ? sdr_multi_run_wide_fmt(&o, &wd, tp, meter ? &mo : nullptr, finish ? &ao : nullptr, blend ? 1 : 0,
                                                rds_decode ? &rd : nullptr, rds_decode ? rds_clock : SDR_MULTI_RDS_CLOCK_REF, nullptr,
                                                rds_soft ? &sq : nullptr, rds_quad ? &cq : nullptr, &wf, &st)
                   : rds_decode ? sdr_multi_run_rds_carrier(&o, wide_w ? &wd : nullptr, tp, meter ? &mo : nullptr,
                                                          finish ? &ao : nullptr, blend ? 1 : 0, &rd, rds_clock, nullptr,
                                                          rds_soft ? &sq : nullptr, rds_quad ? &cq : nullptr, &st)
                   : wide_w ? sdr_multi_run_wide(&o, &wd, tp, meter ? &mo : nullptr, finish ? &ao : nullptr, blend ? 1 : 0, &st)
                   : finish ? sdr_multi_run_finished(&o, tp, meter ? &mo : nullptr, &ao, blend ? 1 : 0, &st)
                   : meter ? sdr_multi_run_metered(&o, tp, &mo, &st)
                           : sdr_multi_run_tuned(&o, tp, &st);
    if (rc != SDR_OK) {
        std::fprintf(stderr, "sdr_multi: %d %s%s\n", rc, sdr_last_error(),
                     tune_path.empty() ? "" : " (--tune: 0 <= src < NCH rows, -N/2 < khz <= N/2, N = rf_Fs / 1000)");
        return 1;
    }
    if (s16) {   // the gain each capture row had and what it did with it
        const std::string path = out + ".wide";
        FILE* f = std::fopen(path.c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "sdr_multi: cannot write %s\n", path.c_str());
            return 1;
        }
        for (size_t i = 0; i < clips.size(); i++)
            std::fprintf(f, "%zu %zu %d %lld %lld\n", i / (size_t)wide_r, i % (size_t)wide_r, wide_shifts[i], wide_peaks[i], clips[i]);
        std::fclose(f);
    }
    for (size_t i = 0; i < clips.size(); i++)
        if (clips[i])
            std::fprintf(stderr, "sdr_multi: splitter: wide stream %zu row %zu: %lld output components clipped\n",
                         i / (size_t)wide_r, i % (size_t)wide_r, clips[i]);
    sdr_ctx* probe = nullptr;   // sizes of the mode
    sdr_info info{};
    if (sdr_ctx_create(&probe, o.device, 1, o.mode, 0, 0) != SDR_OK || sdr_ctx_info(probe, &info) != SDR_OK) return 1;
    sdr_ctx_destroy(probe);
    const double samples = (double)st.blocks * o.nch * info.block_iq;
    const double signal_s = (double)st.blocks * info.block_iq / (double)info.rf_Fs;
    const double in_gb = (double)st.blocks * rows * (s16 ? 4.0 : 2.0) * info.block_iq * (wide_w ? wide_w : 1) / 1e9;   // (a wide run: the wide bytes)
    char after0[128] = "after block 0 n/a (fewer than 2 blocks)";
    if (st.blocks >= 2 && st.steady_seconds > 0)
        std::snprintf(after0, sizeof(after0), "after block 0 %.1f MS/s (%.1fx real time)",
                      (double)(st.blocks - 1) * o.nch * info.block_iq / st.steady_seconds / 1e6,
                      (double)(st.blocks - 1) * info.block_iq / (double)info.rf_Fs / st.steady_seconds);
    char rows_txt[64] = "";   // a tuned run reads fewer rows than it has channels
    if (wide_w) std::snprintf(rows_txt, sizeof(rows_txt), " (from %d wide streams x %d rows per block)", rows, wide_r);
    else if (!tune_path.empty()) std::snprintf(rows_txt, sizeof(rows_txt), " (from %d capture rows per block)", rows);
    std::fprintf(stderr,
                 "sdr_multi: %d channels%s x %lld blocks in %.3f s: %.1f MS/s I/Q, %.1fx real time; %s; PLLs %s "
                 "(%.4f ms per block); input read %.3f s (%.1f GB/s), H2D %.3f s GPU time (%.1f GB/s), "
                 "L/R D2H %.3f s\n",
                 o.nch, rows_txt, st.blocks, st.seconds, st.seconds > 0 ? samples / st.seconds / 1e6 : 0.0,
                 st.seconds > 0 ? signal_s / st.seconds : 0.0, after0, st.persistent ? "persistent" : "per-block dispatch",
                 st.pll_period_ms, st.read_s, st.read_s > 0 ? in_gb / st.read_s : 0.0, st.h2d_ms / 1e3,
                 st.h2d_ms > 0 ? in_gb / (st.h2d_ms / 1e3) : 0.0, st.d2h_ms / 1e3);
    return 0;
}
