// wide_split.h -- what the receiver engine and the wide scan share about a wide run's input: the rule of
// sdr_wide_fmt (include/sdr_multi_wide16.h), and the run's splitter of either sample width.
#pragma once

#include <algorithm>
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

// A wide run's splitter: nwide * (2 W - 1) capture rows per block from nwide wide streams of 2 * wide_iq bytes
// (int8, sdr_split_*) or 4 * wide_iq bytes (int16, sdr_split16_*: a shift per row, fixed, the caller's table, or
// from block 0's peaks). Every method returns the C ABI's code and throws nothing; behind a code that is not
// SDR_OK, `failed` names the call for the caller to put in front of sdr_last_error(). (Hidden: libsdr_host.so
// exports the C entry points, not this.)
class __attribute__((visibility("hidden"))) WideSplit {
    sdr_split* s8 = nullptr;
    sdr_split16* s16 = nullptr;
    int W = 0;
    std::vector<int> shifts;             // s16: the table in use
    int said(int rc, const char* call) {
        if (rc != SDR_OK) failed = call;
        return rc;
    }

  public:
    int rows = 0, wide_iq = 0;           // capture rows of a block; samples of a wide stream's block
    size_t in_row = 0;                   // bytes of a wide stream's block
    int auto_target = -1;                // >= 0: block 0 goes through gain_from first (0: the default target)
    const char* failed = "";

    WideSplit() = default;
    WideSplit(const WideSplit&) = delete;
    WideSplit& operator=(const WideSplit&) = delete;
    ~WideSplit() {
        if (s8) (void)sdr_split_destroy(s8);
        if (s16) (void)sdr_split16_destroy(s16);
    }
    void close() {   // the same ahead of time, for an owner that releases in an order of its own
        if (s8) (void)sdr_split_destroy(s8);
        if (s16) (void)sdr_split16_destroy(s16);
        s8 = nullptr;
        s16 = nullptr;
    }

    // f: a record that wide_fmt_refusal() took, or none. A caller's shifts table is kept for set_table()
    int create(int device, int mode, int W_, int nwide, int shift, const sdr_wide_fmt* f) {
        W = W_;
        if (const int rc = said(sdr_split_geometry(mode, W, &rows, nullptr, &wide_iq, nullptr, nullptr), "sdr_split_geometry"))
            return rc;
        rows *= nwide;
        in_row = (wide16(f) ? 4 : 2) * (size_t)wide_iq;
        if (!wide16(f)) return said(sdr_split_create(&s8, device, mode, W, nwide, shift), "sdr_split_create");
        if (const int rc = said(sdr_split16_create(&s16, device, mode, W, nwide, shift), "sdr_split16_create")) return rc;
        shifts.assign((size_t)rows, shift > 0 ? shift : sdr_split16_shift_for(0, 90, W));
        if (f->gain == SDR_WIDE_GAIN_AUTO) auto_target = f->target;
        if (f->shifts) shifts.assign(f->shifts, f->shifts + rows);
        return SDR_OK;
    }

    // behind create(), in front of block 0: the caller's shifts table, where there is one, on st
    int set_table(const sdr_wide_fmt* f, void* st) {
        if (!s16 || !f->shifts) return SDR_OK;
        return said(sdr_split16_set_shifts(s16, shifts.data(), st), "sdr_split16_set_shifts");
    }

    // both at once, for a caller whose stream exists before its splitter
    int open(int device, int mode, int W_, int nwide, int shift, const sdr_wide_fmt* f, void* st) {
        const int rc = create(device, mode, W_, nwide, shift, f);
        return rc == SDR_OK ? set_table(f, st) : rc;
    }

    // Auto gain, in front of block 0's block call: the block split once into `scratch` (rows nobody reads), its
    // peaks through the rule into the shifts, these set, and the splitter reset, all on st; waits for st once.
    int gain_from(const uint8_t* src, size_t stride, uint8_t* scratch, size_t row, void* st) {
        std::vector<long long> peaks(shifts.size());
        int rc = sdr_split16_block(s16, reinterpret_cast<const int16_t*>(src), stride, scratch, row, st);
        if (rc == SDR_OK) rc = sdr_split16_peaks(s16, peaks.data(), 0, st);
        if (rc != SDR_OK) return said(rc, "the wide run's auto gain");
        for (size_t i = 0; i < peaks.size(); i++) shifts[i] = sdr_split16_shift_for(peaks[i], auto_target > 0 ? auto_target : 90, W);
        rc = sdr_split16_set_shifts(s16, shifts.data(), st);
        if (rc == SDR_OK) rc = sdr_split16_reset(s16, st);
        return said(rc, "the wide run's auto gain");
    }

    int block(const uint8_t* src, size_t stride, uint8_t* out, size_t row, void* st) {
        if (s16) return said(sdr_split16_block(s16, reinterpret_cast<const int16_t*>(src), stride, out, row, st), "sdr_split16_block");
        return said(sdr_split_block(s8, reinterpret_cast<const int8_t*>(src), stride, out, row, st), "sdr_split_block");
    }

    // the end of a run: the clip counts [rows] where asked for, and what the record asks for (peaks_out, shifts_out)
    int report(long long* clips, const sdr_wide_fmt* f, void* st) {
        if (clips)
            if (const int rc = s16 ? said(sdr_split16_clips(s16, clips, st), "sdr_split16_clips")
                                   : said(sdr_split_clips(s8, clips, st), "sdr_split_clips"))
                return rc;
        if (!s16) return SDR_OK;
        if (f->shifts_out) std::copy(shifts.begin(), shifts.end(), f->shifts_out);
        return f->peaks_out ? said(sdr_split16_peaks(s16, f->peaks_out, 0, st), "sdr_split16_peaks") : SDR_OK;
    }
};

}  // namespace sdrhost
