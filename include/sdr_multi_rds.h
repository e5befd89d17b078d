/* sdr_multi_rds.h -- the multi-channel receiver engine (include/sdr_multi.h) with the RDS group decoder
 * (include/sdr_amd.h, sdr_rds_*): block synchronisation, slip recovery and burst correction on the GPU
 * where the bits are, and what every station says. Same engine, same options and statistics, exported
 * from libsdr_host.so; the CLI's --rds-decode [--rds-correct N] calls it.
 *
 * The RDS thread runs sdr_rds_groups behind its sdr_rds_bits on its post stream, copies the block's group
 * records out with the bits into pinned buffers of the engine's pool, and its frame layer feeds one
 * sdr_rds_station per channel. The PCM, the RDS text, the captures and the meter's and the finishing
 * stage's files are those of a run without the decoder. With an out_prefix the run also writes
 *   PREFIX.groups   one text line per group, block after block, the channels in order within a block:
 *                     ch <c> bits <n> AAAA BBBB CCCC DDDD
 *                   <n> = sdr_rds_group.bits; a block that is not in ok is "----", a corrected block has
 *                   a trailing "*"
 *   PREFIX.radio    at the end, every channel's sdr_rds_station_format report, each line behind
 *                   "ch <c>: ": PI, PTY (the RBDS names), TP/TA/MS, PS, RT, CT, AF, the groups by type,
 *                   blocks good/corrected/bad and BLER, slips, syncs acquired/lost.
 *
 * The bit clock (sdr_multi_run_rds_clock, the CLI's --rds-clock ref|track): with SDR_MULTI_RDS_CLOCK_REF the
 * decoder reads the bits of sdr_rds_bits, as above. With SDR_MULTI_RDS_CLOCK_TRACK the RDS thread also runs
 * the RDS symbol tracker (include/sdr_amd.h, sdr_rds_track_*) behind the block's RRC on its post stream, on the
 * context's rds_clean row, and sdr_rds_groups reads the tracker's bits: PREFIX.groups and PREFIX.radio are made
 * from them, and PREFIX.radio gains, behind every channel's report, the line
 *   ch <c>: clock: locked <0|1> phase <p> bits <n> moves <m> half_moves <h> resets <r> level <l>
 * of its sdr_rds_track_stats. PREFIX.rds, the PCM, the captures and every other file are byte for byte those
 * of a run with the reference clock. */
#ifndef SDR_MULTI_RDS_H
#define SDR_MULTI_RDS_H

#include "sdr_amd.h"
#include "sdr_multi.h"
#include "sdr_multi_tuned.h"
#include "sdr_multi_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdr_multi_rds {
    int max_burst, loss_blocks;   /* sdr_rds_opts: 0..5 and 1..64 */
} sdr_multi_rds;

/* sdr_multi_run_wide with the decoder: any of wide, tune, mo, ao may be NULL as there; rds == NULL is
 * that call. SDR_E_INVALID, before anything starts, also for options out of range and for a mode whose
 * RDS chain has no 1187.5 bit/s clock (sdr_rds_mode_ok: modes 1 to 3). */
int sdr_multi_run_rds(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                      const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, const sdr_multi_rds *rds,
                      sdr_multi_stats *stats);

#define SDR_MULTI_RDS_CLOCK_REF 0     /* the bits of sdr_rds_bits: the reference's per-block clock recovery */
#define SDR_MULTI_RDS_CLOCK_TRACK 1   /* the bits of sdr_rds_track_bits */

/* sdr_multi_run_rds with a choice of bit clock; rds_clock = SDR_MULTI_RDS_CLOCK_REF is that call. track: the
 * tracker's options, NULL for sdr_rds_track_opts_default's; only read with SDR_MULTI_RDS_CLOCK_TRACK.
 * SDR_E_INVALID, before anything starts, also for an rds_clock that is neither, for the tracker without the
 * decoder (rds == NULL), and for tracker options out of range. */
int sdr_multi_run_rds_clock(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                            const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, const sdr_multi_rds *rds,
                            int rds_clock, const sdr_rds_track_opts *track, sdr_multi_stats *stats);

/* sdr_multi_run_rds_clock with soft decisions (the CLI's --rds-soft L); soft == NULL is that call. With soft the
 * RDS thread runs sdr_rds_track_bits_soft, which also writes every bit's reliability into one more
 * [nch][SDR_MAX_BITS] u16 device row set of the engine's pool, and sdr_rds_groups_soft on a decoder of
 * sdr_rds_dec_create_soft(soft): soft->max_burst and soft->loss_blocks are the decoder's, rds only says that
 * the run decodes. In PREFIX.groups a block the soft step placed ends in "~" instead of "*", and PREFIX.radio
 * gains, behind every channel's clock line, the line
 *   ch <c>: soft: blocks <n> flips <f>
 * of its sdr_rds_soft_stats. Every other file is byte for byte that of the run without soft.
 * SDR_E_INVALID, before anything starts, also for soft without SDR_MULTI_RDS_CLOCK_TRACK or without rds, and for
 * soft options out of range (soft_bits 0..6). */
int sdr_multi_run_rds_soft(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                           const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, const sdr_multi_rds *rds,
                           int rds_clock, const sdr_rds_track_opts *track, const sdr_rds_soft_opts *soft,
                           sdr_multi_stats *stats);

/* sdr_multi_run_rds_soft on coherent rows (the CLI's --rds-carrier quad); carrier == NULL is that call. With
 * carrier the RDS thread's context is created with SDR_FLAG_RDS_QUAD, and behind the block's RRCs on its post
 * stream the thread runs sdr_rds_carrier_rotate (include/sdr_amd.h, sdr_rds_carrier_*) on the context's rds_clean
 * and rds_clean_q rows into one more [nch][n_rds] f32 row set of the engine's pool, then the tracker on those
 * rows in place of rds_clean, then the decoder. PREFIX.groups and PREFIX.radio are made from the new bits, and
 * PREFIX.radio gains, directly behind every channel's clock line (before a soft line), the line
 *   ch <c>: carrier: phase <degrees, %.2f> coherence <hypot(sr, si) / st, %.3f> windows <n> resets <r>
 * of its sdr_rds_carrier_stats. PREFIX.rds, the PCM, the captures and every other file are byte for byte those
 * of the run without carrier: sdr_rds_bits still reads rds_clean.
 * SDR_E_INVALID, before anything starts, also for carrier without SDR_MULTI_RDS_CLOCK_TRACK or without rds, and
 * for carrier options out of range (qshift 0..15, avg_shift 0..6). */
int sdr_multi_run_rds_carrier(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                              const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, const sdr_multi_rds *rds,
                              int rds_clock, const sdr_rds_track_opts *track, const sdr_rds_soft_opts *soft,
                              const sdr_rds_carrier_opts *carrier, sdr_multi_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
