/* sdr_multi_wide16.h -- the receiver engine (include/sdr_multi_wide.h) and the wide scan (include/sdr_wide_scan.h)
 * on 16-bit wide captures: the sc16 stream of a USRP, bladeRF, LimeSDR, Pluto or SDRplay, cut into capture rows by
 * the 16-bit splitter (include/sdr_amd.h, sdr_split16_*) with a shift per stream and row. Same engine, same
 * options, records and statistics, exported from libsdr_host.so; the CLI's --wide-format option calls these.
 *
 * One record says what the wide streams hold and how the rows get their gain. With format SDR_WIDE_S16 an input
 * row -- file, pipe or device -- is 4 * W * block_iq bytes: little-endian int16, I then Q; the sdr_multi_wide /
 * sdr_wide_scan_opts record's `shift` is then the 16-bit splitter's (1..33; <= 0: the default 22, 23, 24 of
 * W = 4, 8, 10) and holds for every row unless `shifts` or auto gain replaces it. Nothing downstream of the row
 * buffers changes.
 *
 * Auto gain: before the run proper the engine splits block 0 once into a row buffer nobody reads, reads the
 * peaks, gives every row sdr_split16_shift_for(peak, target, W), sets these shifts, resets the splitter and starts
 * at block 0 again: one extra launch and one sync per run, before anything is handed to the front end. The shifts
 * then hold for the run (no gain loop while receiving); a later, louder block may clip, and the clip counters say
 * so as they do today. */
#ifndef SDR_MULTI_WIDE16_H
#define SDR_MULTI_WIDE16_H

#include "sdr_multi_rds.h"
#include "sdr_multi_wide.h"
#include "sdr_wide_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDR_WIDE_S8 0
#define SDR_WIDE_S16 1
#define SDR_WIDE_GAIN_FIXED 0
#define SDR_WIDE_GAIN_AUTO 1

typedef struct sdr_wide_fmt {
    int format;                   /* SDR_WIDE_S8: the existing run, the rest of the record is not looked at */
    int gain;                     /* SDR_WIDE_GAIN_FIXED or SDR_WIDE_GAIN_AUTO */
    int target;                   /* auto gain's target, 1..127; 0: 90 */
    const int *shifts;            /* optional (NULL: none), fixed gain only: a shift per row [nwide * (2 W - 1)], 1..33 */
    int *shifts_out;              /* optional: the shifts the run used [nwide * (2 W - 1)] */
    long long *peaks_out;         /* optional: the run's peaks [nwide * (2 W - 1)] (sdr_split16_peaks) */
} sdr_wide_fmt;

/* fmt == NULL or fmt->format == SDR_WIDE_S8: exactly sdr_multi_run_rds_carrier. Otherwise the same run on int16
 * wide streams. SDR_E_INVALID before anything starts: a format, gain or target outside the above, a shift (the
 * wide record's, or one of the table's) outside 1..33, auto gain together with a shifts table, no wide record,
 * or what sdr_multi_run_rds_carrier refuses. wide->clips is filled as there. */
int sdr_multi_run_wide_fmt(const sdr_multi_opts *opts, const sdr_multi_wide *wide, const sdr_multi_tuning *tune,
                           const sdr_meter_opts *mo, const sdr_audio_opts *ao, int blend, const sdr_multi_rds *rds,
                           int rds_clock, const sdr_rds_track_opts *track, const sdr_rds_soft_opts *soft,
                           const sdr_rds_carrier_opts *carrier, const sdr_wide_fmt *fmt, sdr_multi_stats *stats);

/* fmt == NULL or fmt->format == SDR_WIDE_S8: exactly sdr_wide_scan_run. Otherwise the scan of int16 wide streams;
 * auto gain takes its shifts from block 0 and then scans max_blocks blocks from block 0 on. The same refusals,
 * with stats->error saying which. */
int sdr_wide_scan_run_fmt(const sdr_wide_scan_opts *opts, const sdr_wide_fmt *fmt, sdr_wide_scan_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
