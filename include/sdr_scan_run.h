/* sdr_scan_run.h -- the band scan over a capture file: the file loop behind `sdr_multi NROWS --scan`,
 * exported from libsdr_host.so (real-time-sdr_amd/host/sdr_scan_run.cpp) on the scanner of
 * include/sdr_amd.h (sdr_scan_*).
 *
 * The input is the byte stream sdr_multi --tune reads (include/sdr_multi_tuned.h): u8 I/Q, block after
 * block, each block nrows capture rows of 2*block_iq bytes. Up to max_blocks whole blocks are scanned
 * (a trailing partial block is not used), every row's spectrum goes through sdr_scan_pick, and the
 * stations found are written as the text --tune takes: one "src khz" line per station, row after row,
 * each row in the picker's order (descending channel power). */
#ifndef SDR_SCAN_RUN_H
#define SDR_SCAN_RUN_H

#include <stdint.h>

#include "sdr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdr_scan_run_opts {
    int nrows, mode, device;
    const char *in_path;          /* input file, or "-" for stdin */
    const char *out_path;         /* the station list; NULL: no file */
    int max_blocks;               /* blocks to scan at most; <= 0: 4 */
    sdr_scan_opts pick;           /* the picker's options (sdr_scan_opts_default for the usual ones) */
    /* optional (NULL: none): the first max_stations stations found, as sdr_tuner_set takes them */
    int max_stations;
    int32_t *src, *khz;
} sdr_scan_run_opts;

typedef struct sdr_scan_run_stats {
    int stations;                 /* stations found over all rows */
    long long blocks, segments;   /* blocks scanned, segments accumulated per row */
    char error[256];              /* what failed, when the return value is not SDR_OK */
} sdr_scan_run_stats;

/* SDR_OK, or SDR_E_INVALID (bad options, an input that cannot be opened or holds no whole block, an
 * output that cannot be written) or the scanner's error; stats->error then says what. */
int sdr_scan_run(const sdr_scan_run_opts *opts, sdr_scan_run_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
