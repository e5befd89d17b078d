/* sdr_multi_meter.h -- the multi-channel receiver engine (include/sdr_multi.h) with the reception
 * meter (include/sdr_amd.h, sdr_meter_*): which channels carry a stereo pilot, which a usable RDS
 * sub-carrier, which are tuned off, which are noise or dead air. Same engine, same options and
 * statistics, exported from libsdr_host.so; the CLI's --meter option calls it.
 *
 * The audio thread calls sdr_meter_audio after its sdr_stereo_post and the RDS thread sdr_meter_rds
 * after its sdr_rds_post, each on its own context and stream, both on one shared meter. The PCM, the
 * RDS text and the captures are those of a run without the meter. With an out_prefix the run also
 * writes
 *   PREFIX.meter    per block, nch rows of 64 bytes (sdr_meter_row, both parts of the block)
 *   PREFIX.status   at the end, one text line per channel:
 *                     ch <c>: offset <v> level_db <v> pilot_nr <v> rds_nr <v> eye_db <v> flags <F>
 *                   the run's means of sdr_meter_status's readings over its blocks (discriminator
 *                   units and ratios, not kHz of deviation) and, joined by '|', the flags STEREO, RDS,
 *                   OFFTUNE, DEAD_AIR that held on more than half the blocks ('-' when none did).
 *                   A run whose opts->flags hold SDR_FLAG_PHASE_DEMOD (the phase discriminator: the rows'
 *                   fm fields are radians) ends every line with
 *                     " peak_khz <v> offset_khz <v>"
 *                   the run's maximum of sdr_meter_deviation's peak and the mean of its offset, in kHz
 *                   of deviation; without that flag the file is byte for byte what it was. */
#ifndef SDR_MULTI_METER_H
#define SDR_MULTI_METER_H

#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_tuned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sdr_multi_run_tuned (tune may be NULL: sdr_multi_run) with the meter; mo: the thresholds of the
 * status flags (sdr_meter_opts_default), SDR_E_INVALID when NULL. */
int sdr_multi_run_metered(const sdr_multi_opts *opts, const sdr_multi_tuning *tune, const sdr_meter_opts *mo,
                          sdr_multi_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
