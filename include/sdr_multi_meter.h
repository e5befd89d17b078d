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
 *                   of deviation; without that flag the file is byte for byte what it was.
 *
 * The RF readings. A run whose opts->flags hold SDR_FLAG_IF_ENVELOPE and that has a meter (mo != NULL) --
 * through this or any later entry point that takes mo, tuned, wide, int16 or RDS-decoding runs alike -- is
 * RF-metered: the RF thread's context alone is created with the flag, and directly behind each block's
 * sdr_frontend / sdr_frontend_tuned, on the same stream, the RF thread calls sdr_meter_rf on the shared
 * meter. The flag without a meter, or with SDR_FLAG_FAST_FRONTEND, is SDR_E_INVALID before anything starts.
 * Every other file of the run is byte for byte that of the run without the flag; with an out_prefix the
 * run also writes
 *   PREFIX.rf        per block, nch rows of 32 bytes (sdr_meter_rf_row)
 *   PREFIX.rfstatus  at the end, one text line per channel:
 *                      ch <c>: level_dbfs <v> ripple <v> cnr_db <v> fade_db <v> crest_db <v> flags <WEAK|->
 *                    sdr_meter_rf_status under its default options of the channel's run-long row: env_sum,
 *                    env_sq and n of its blocks added in double (the sums stored as f32 again), the minimum
 *                    of env_min and the maximum of env_max. Each <v> is printed with %.3f (an infinity as
 *                    inf or -inf). In a wide run the level is relative to the full scale of the splitter's
 *                    output row; the row's shift in PREFIX.wide converts it. */
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
