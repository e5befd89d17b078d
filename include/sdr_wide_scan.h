/* sdr_wide_scan.h -- the band scan over a wide capture file: the file loop behind
 * `sdr_multi NWIDE --wide W --scan`, exported from libsdr_host.so
 * (real-time-sdr_amd/host/sdr_scan_run.cpp) on the splitter and the scanner of include/sdr_amd.h
 * (sdr_split_*, sdr_scan_*).
 *
 * The input is the byte stream sdr_multi --wide reads (include/sdr_multi_wide.h): int8 I/Q, block after
 * block, each block nwide streams of 2 * W * block_iq bytes. Up to max_blocks whole blocks are split into
 * nwide * R capture rows (R = 2 W - 1) and scanned. With N = rf_Fs / 1000, row r of a stream (k = r - (W - 1),
 * centre k N / 2 kHz off the wide capture's centre) is picked with guard_khz = N / 4, so its candidates
 * are |khz| <= N / 4, on the absolute station grid: its first_khz is (pick.first_khz - k N / 2) mod
 * pick.step_khz (N / 2 is no multiple of 100 in modes 1 and 3). A pick whose absolute frequency an
 * earlier row of the same stream already gave -- the |khz| = N / 4 tie of two neighbouring rows -- is
 * dropped. The stations are written as the text --tune takes, one "src khz" line each with
 * src = w * R + r, row after row, each row in the picker's order. */
#ifndef SDR_WIDE_SCAN_H
#define SDR_WIDE_SCAN_H

#include <stdint.h>

#include "sdr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdr_wide_scan_opts {
    int nwide, W, shift;          /* wide streams per block, width factor, splitter shift (<= 0: default) */
    int mode, device;
    const char *in_path;          /* input file, or "-" for stdin */
    const char *out_path;         /* the station list; NULL: no file */
    int max_blocks;               /* blocks to scan at most; <= 0: 4 */
    sdr_scan_opts pick;           /* the picker's options; guard_khz is replaced by N / 4 and first_khz is absolute */
    /* optional (NULL: none): the first max_stations stations found, as sdr_tuner_set takes them */
    int max_stations;
    int32_t *src, *khz;
} sdr_wide_scan_opts;

typedef struct sdr_wide_scan_stats {
    int stations;                 /* stations found over all rows */
    long long blocks, segments;   /* blocks scanned, segments accumulated per row */
    long long clips;              /* output components the splitter clipped, over all rows */
    char error[256];              /* what failed, when the return value is not SDR_OK */
} sdr_wide_scan_stats;

/* SDR_OK, or SDR_E_INVALID (bad options, an input that cannot be opened or holds no whole block, an
 * output that cannot be written) or the splitter's or scanner's error; stats->error then says what. */
int sdr_wide_scan_run(const sdr_wide_scan_opts *opts, sdr_wide_scan_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
