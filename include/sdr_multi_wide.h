/* sdr_multi_wide.h -- the multi-channel receiver engine (include/sdr_multi.h) on wide captures: one
 * signed 8-bit I/Q stream at W * rf_Fs per antenna, cut into capture rows by the wideband splitter
 * (include/sdr_amd.h, sdr_split_*) in front of the shared-capture tuner. Same engine, same options and
 * statistics, exported from libsdr_host.so; the CLI's --wide option calls it.
 *
 * The input -- a file, a pipe or the device -- holds nwide rows of 2 * W * block_iq int8 bytes per block
 * (I then Q): a byte stream is block after block of them; a device input has stream w of block b at
 * d_iq + b*block_stride + w*row_stride (row_stride >= 2 * W * block_iq, a multiple of 4, d_iq 4-byte
 * aligned). Per block the RF thread uploads the wide block, runs sdr_split_block into one of two row
 * buffers on the front-end stream and hands that buffer to sdr_frontend_tuned: capture row w * R + r
 * (R = 2 W - 1) is row r of stream w, and the tuning names these rows. Everything downstream of the
 * front end, the outputs and the captures are those of a tuned run on the same rows. */
#ifndef SDR_MULTI_WIDE_H
#define SDR_MULTI_WIDE_H

#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_audio.h"
#include "sdr_multi_meter.h"
#include "sdr_multi_tuned.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdr_multi_wide {
    int W, nwide;                 /* width factor (4, 8 or 10) and wide streams per block */
    int shift;                    /* the splitter's output shift, 1..24; <= 0: the default of W */
    long long *clips;             /* optional (NULL: none): the run's clip counters [nwide * (2 W - 1)] */
} sdr_multi_wide;

/* wide == NULL: exactly sdr_multi_run_finished. Otherwise a wide run, always tuned; mo and ao may be
 * NULL (no meter, no finishing stage; blend != 0 needs both). SDR_E_INVALID before anything starts: a
 * NULL tuning, tune->nsrc > nwide * (2 W - 1) (or > nch, the tuner's own bound), a bad W, nwide or
 * shift, or what sdr_multi_run_finished refuses. */
int sdr_multi_run_wide(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                       const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, sdr_multi_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
