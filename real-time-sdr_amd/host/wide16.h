// wide16.h -- what the receiver engine and the wide scan share about sdr_wide_fmt (include/sdr_multi_wide16.h):
// the record's rule, and the auto gain step on block 0.
#pragma once

#include <vector>

#include "sdr_multi_wide16.h"

namespace sdrhost {

inline bool wide16(const sdr_wide_fmt* f) { return f && f->format != SDR_WIDE_S8; }

// nullptr when a run of W, nwide and the wide record's shift takes the record, else what is wrong with it
inline const char* wide_fmt_refusal(const sdr_wide_fmt* f, int mode, int W, int nwide, int shift) {
    if (!wide16(f)) return nullptr;
    if (f->format != SDR_WIDE_S16) return "wide format not s8 (0) or s16 (1)";
    if (f->gain != SDR_WIDE_GAIN_FIXED && f->gain != SDR_WIDE_GAIN_AUTO) return "wide gain not fixed (0) or auto (1)";
    if (f->target < 0 || f->target > 127) return "wide gain target outside [1, 127]";
    if (f->gain == SDR_WIDE_GAIN_AUTO && f->shifts) return "auto gain and a shifts table";
    if (sdr_split16_check(mode, W, nwide, shift) != SDR_OK) return sdr_last_error();
    if (f->shifts)
        for (int i = 0; i < nwide * (2 * W - 1); i++)
            if (f->shifts[i] < 1 || f->shifts[i] > 33) return "a shift of the table outside [1, 33]";
    return nullptr;
}

// Auto gain: block 0 split once into `rows` (which nobody reads), its peaks through the rule into *shifts, these
// set, and the splitter reset, all on st; waits for st once. The caller then starts at block 0 again.
inline int wide16_auto_gain(sdr_split16* s, int W, int target, const int16_t* wide, size_t wide_stride, uint8_t* rows,
                            size_t row_stride, void* st, std::vector<int>* shifts) {
    std::vector<long long> peaks(shifts->size());
    int rc = sdr_split16_block(s, wide, wide_stride, rows, row_stride, st);
    if (rc == SDR_OK) rc = sdr_split16_peaks(s, peaks.data(), 0, st);
    if (rc != SDR_OK) return rc;
    for (size_t i = 0; i < peaks.size(); i++) (*shifts)[i] = sdr_split16_shift_for(peaks[i], target > 0 ? target : 90, W);
    rc = sdr_split16_set_shifts(s, shifts->data(), st);
    if (rc == SDR_OK) rc = sdr_split16_reset(s, st);
    return rc;
}

}  // namespace sdrhost
