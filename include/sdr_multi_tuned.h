/* sdr_multi_tuned.h -- the multi-channel receiver engine (include/sdr_multi.h) on shared captures:
 * many stations from one I/Q stream per front end (include/sdr_amd.h, sdr_tuner_set /
 * sdr_frontend_tuned). Same engine, same options and statistics, exported from libsdr_host.so; the
 * CLI's --tune option calls it.
 *
 * Channel ch listens to row src[ch] of the nsrc capture rows of every block and to the station
 * khz[ch] kHz off that capture's centre. The input -- a file, a pipe or the device -- then holds
 * nsrc rows per block instead of nch: a byte stream is block after block of nsrc rows of 2*block_iq
 * bytes; a device input has row src of block b at d_iq + b*block_stride + src*row_stride. Everything
 * downstream of fm_demod, the outputs and the captures are per channel as ever. */
#ifndef SDR_MULTI_TUNED_H
#define SDR_MULTI_TUNED_H

#include <stdint.h>

#include "sdr_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdr_multi_tuning {
    int nsrc;                     /* capture rows per block, 1 <= nsrc <= nch */
    const int32_t *src, *khz;     /* [nch]: 0 <= src[ch] < nsrc, -N/2 < khz[ch] <= N/2, N = rf_Fs / 1000 */
} sdr_multi_tuning;

/* sdr_multi_run with the tuning `tune` (NULL: exactly sdr_multi_run). The tuning is checked before
 * anything starts: SDR_E_INVALID for a violated bound or a NULL array. The engine's pooled contexts
 * take the tuning of the run that uses them (an untuned run clears it). */
int sdr_multi_run_tuned(const sdr_multi_opts *opts, const sdr_multi_tuning *tune, sdr_multi_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
