/* sdr_multi_audio.h -- the multi-channel receiver engine (include/sdr_multi.h) with the audio
 * finishing stage (include/sdr_amd.h, sdr_audio_*): de-emphasis, and a stereo blend that follows the
 * reception meter's pilot reading. Same engine, same options and statistics, exported from
 * libsdr_host.so; the CLI's --deemph and --blend options call it.
 *
 * Per block the audio thread runs sdr_stereo_post, sdr_meter_audio (a metered run),
 * sdr_audio_blend_from_meter (blend != 0) and sdr_audio_finish from the block's L/R rows into device
 * rows of its own, all on its post stream; a copy to pinned memory follows behind the L/R one. The
 * PCM, the RDS text, the meter's files and the captures are those of a run without the stage. With an
 * out_prefix the run also writes
 *   PREFIX.audio    the finished audio, in the layout of PREFIX.pcm: per block, nch rows of
 *                   2 * n_audio int16, L/R interleaved */
#ifndef SDR_MULTI_AUDIO_H
#define SDR_MULTI_AUDIO_H

#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_meter.h"
#include "sdr_multi_tuned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sdr_multi_run_metered (mo may be NULL: no meter; tune may be NULL) with the finishing stage; ao: its
 * options (sdr_audio_opts_default); blend != 0: the blend follows the meter, else it stays 1 (full
 * stereo). SDR_E_INVALID: ao NULL or refused by sdr_audio_create, blend != 0 with mo NULL. */
int sdr_multi_run_finished(const sdr_multi_opts *opts, const sdr_multi_tuning *tune, const sdr_meter_opts *mo,
                           const sdr_audio_opts *ao, int blend, sdr_multi_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
