// sdr_rds_text.cpp -- the host side of the RDS group decoder (include/sdr_amd.h, sdr_rds_*): the syndrome
// and the burst-correction table the kernel's create uses, and the text layer that turns 16-byte group
// records into what a station says (PI, PTY, TP/TA/MS, PS, RadioText, clock time, AF, groups by type,
// block error rate). Plain C++ without HIP: it builds and runs anywhere.
//
// Every index that comes off the air (segment address, AF count, text position) is bounded before use.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "sdr_amd.h"

namespace {

constexpr uint32_t kPoly = 0x5B9;   // g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1

// RBDS programme type names (index = 5-bit PTY code), as the receiver's frame layer prints them
const char* const kPty[32] = {"Undefined", "News", "Information", "Sports", "Talk", "Rock", "Classic Rock",
                              "Adult Hits", "Soft Rock", "Top 40", "Country", "Oldies", "Soft", "Nostalgia",
                              "Jazz", "Classical", "Rhythm & Blues", "Soft Rhythm & Blues", "Language",
                              "Religious Music", "Religious Talk", "Personality", "Public", "College",
                              "Spanish Talk", "Spanish Music", "Hip Hop", "Unassigned", "Unassigned", "Weather",
                              "Emergency Test", "Emergency"};

char printable(uint8_t c) { return (c >= 0x20 && c <= 0x7E) ? (char)c : '.'; }

struct Out {
    char* buf;
    size_t cap, len;
    void add(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char tmp[256];
        va_list ap;
        va_start(ap, fmt);
        int k = std::vsnprintf(tmp, sizeof tmp, fmt, ap);
        va_end(ap);
        if (k < 0) return;
        if ((size_t)k >= sizeof tmp) k = (int)sizeof tmp - 1;
        for (int i = 0; i < k; i++) {
            if (buf && len + 1 < cap) buf[len] = tmp[i];
            len++;
        }
    }
};

void af_code(sdr_rds_station* s, unsigned code) {
    if (code >= 224 && code <= 249) {
        const unsigned count = code - 224;          // 0..25
        if (count != s->af_expect) {
            s->af_expect = (uint8_t)count;
            s->af_n = 0;
        }
    } else if (code >= 1 && code <= 204) {
        const uint16_t f = (uint16_t)(876 + code);  // 100 kHz units
        for (unsigned i = 0; i < s->af_n && i < 25; i++)
            if (s->af[i] == f) return;
        if (s->af_n < 25) s->af[s->af_n++] = f;
    }
}

void rt_put(sdr_rds_station* s, unsigned pos, uint8_t c) {
    if (pos >= 64) return;
    s->rt[pos] = c;
    s->rt_seen |= (uint64_t)1 << pos;
}

void clock_time(sdr_rds_station* s, const sdr_rds_group* g) {
    const long mjd = ((long)(g->w[1] & 3) << 15) | (g->w[2] >> 1);
    const unsigned hour = ((g->w[2] & 1u) << 4) | (g->w[3] >> 12);
    const unsigned minute = (g->w[3] >> 6) & 0x3F;
    const int off = (int)(g->w[3] & 0x1F) * ((g->w[3] & 0x20) ? -1 : 1);
    if (mjd < 15079 || hour > 23 || minute > 59) return;
    // IEC 62106 annex G, in integers: Y' = int((MJD - 15078.2) / 365.25), M' = int((MJD - 14956.1 -
    // int(Y' 365.25)) / 30.6001), D = MJD - 14956 - int(Y' 365.25) - int(M' 30.6001)
    const long yp = (mjd * 100 - 1507820) / 36525;
    const long yd = yp * 36525 / 100;
    const long mp = ((mjd - yd) * 10000 - 149561000) / 306001;
    const long day = mjd - 14956 - yd - mp * 306001 / 10000;
    const long k = (mp == 14 || mp == 15) ? 1 : 0;
    s->ct_year = (int32_t)(1900 + yp + k);
    s->ct_month = (uint8_t)(mp - 1 - 12 * k);
    s->ct_day = (uint8_t)day;
    s->ct_hour = (uint8_t)hour;
    s->ct_minute = (uint8_t)minute;
    s->ct_offset = (int8_t)off;
    s->ct_mjd = (int32_t)mjd;
    s->ct_valid = 1;
}

}  // namespace

extern "C" {

void sdr_rds_opts_default(sdr_rds_opts* o) {
    if (!o) return;
    o->max_burst = 2;
    o->loss_blocks = 8;
}

uint32_t sdr_rds_syndrome(uint32_t w26) {
    uint32_t reg = w26 & 0x3FFFFFFu;
    for (int bit = 25; bit >= 10; bit--)
        if (reg & (1u << bit)) reg ^= kPoly << (bit - 10);
    return reg & 0x3FFu;
}

int sdr_rds_correction_table(int max_burst, uint32_t* tab1024, int* entries) {
    if (max_burst < 0 || max_burst > 5) return SDR_E_INVALID;
    if (tab1024) std::memset(tab1024, 0, 1024 * sizeof(uint32_t));
    int n = 0;
    for (int len = 1; len <= max_burst; len++) {
        const uint32_t inner = len <= 2 ? 1u : 1u << (len - 2);
        for (uint32_t mid = 0; mid < inner; mid++) {
            const uint32_t p = len == 1 ? 1u : (1u << (len - 1)) | (mid << 1) | 1u;
            for (int pos = 0; pos + len <= 26; pos++) {
                const uint32_t e = p << pos;
                if (tab1024) tab1024[sdr_rds_syndrome(e)] = e;
                n++;
            }
        }
    }
    if (entries) *entries = n;
    return SDR_OK;
}

const char* sdr_rds_pty_name(int pty) { return kPty[pty & 31]; }

void sdr_rds_station_init(sdr_rds_station* s) {
    if (!s) return;
    std::memset(s, 0, sizeof *s);
    std::memset(s->ps, ' ', sizeof s->ps);
    std::memset(s->ps_done, ' ', sizeof s->ps_done);
    std::memset(s->rt, ' ', sizeof s->rt);
    s->rt_len = 64;
}

void sdr_rds_station_update(sdr_rds_station* s, const sdr_rds_group* g) {
    if (!s || !g) return;
    s->ngroups++;
    const unsigned ok = g->ok & 15u;
    if (ok & 1u) {
        if (s->pi_seen && s->pi_last == g->w[0]) {
            s->pi = g->w[0];
            s->pi_valid = 1;
        }
        s->pi_last = g->w[0];
        s->pi_seen = 1;
    } else {
        s->pi_seen = 0;                 // "twice in a row": a group without block A breaks the run
    }
    if (!(ok & 2u)) return;             // everything else is addressed by block B
    const unsigned b = g->w[1];
    const unsigned type = (b >> 12) & 15u, ver = (b >> 11) & 1u;
    s->hist[(2 * type + ver) & 31u]++;
    s->tp = (b >> 10) & 1u;
    s->pty = (b >> 5) & 31u;
    s->have_b = 1;
    if (type == 0) {
        s->ta = (b >> 4) & 1u;
        s->ms = (b >> 3) & 1u;
        s->have_0 = 1;
        if (ok & 8u) {
            const unsigned seg = b & 3u;
            const uint8_t c0 = (uint8_t)(g->w[3] >> 8), c1 = (uint8_t)(g->w[3] & 0xFF);
            if (((s->ps_seen >> seg) & 1u) && (s->ps[2 * seg] != c0 || s->ps[2 * seg + 1] != c1)) s->ps_seen = 0;
            s->ps[2 * seg] = c0;
            s->ps[2 * seg + 1] = c1;
            s->ps_seen |= (uint8_t)(1u << seg);
            if (s->ps_seen == 15) {
                std::memcpy(s->ps_done, s->ps, 8);
                s->ps_complete = 1;
            }
        }
        if (ver == 0 && (ok & 4u) && !(g->flags & SDR_RDS_GROUP_CPRIME)) {
            af_code(s, g->w[2] >> 8);
            af_code(s, g->w[2] & 0xFFu);
        }
    } else if (type == 2) {
        const unsigned ab = (b >> 4) & 1u, seg = b & 15u;
        const uint8_t len = ver ? 32 : 64;
        if (!s->rt_have_ab || s->rt_ab != ab || s->rt_len != len) {
            std::memset(s->rt, ' ', sizeof s->rt);
            s->rt_seen = 0;
            s->rt_ab = (uint8_t)ab;
            s->rt_have_ab = 1;
            s->rt_len = len;
        }
        if (ver == 0) {
            if ((ok & 4u) && !(g->flags & SDR_RDS_GROUP_CPRIME)) {
                rt_put(s, 4 * seg, (uint8_t)(g->w[2] >> 8));
                rt_put(s, 4 * seg + 1, (uint8_t)(g->w[2] & 0xFF));
            }
            if (ok & 8u) {
                rt_put(s, 4 * seg + 2, (uint8_t)(g->w[3] >> 8));
                rt_put(s, 4 * seg + 3, (uint8_t)(g->w[3] & 0xFF));
            }
        } else if (ok & 8u) {
            rt_put(s, 2 * seg, (uint8_t)(g->w[3] >> 8));
            rt_put(s, 2 * seg + 1, (uint8_t)(g->w[3] & 0xFF));
        }
    } else if (type == 4 && ver == 0) {
        if ((ok & 12u) == 12u && !(g->flags & SDR_RDS_GROUP_CPRIME)) clock_time(s, g);
    }
}

void sdr_rds_station_stats(sdr_rds_station* s, const sdr_rds_stats* st) {
    if (!s || !st) return;
    s->good = st->good;
    s->corrected = st->corrected;
    s->bad = st->bad;
    s->slips = st->slips;
    s->acquired = st->acquired;
    s->lost = st->lost;
}

double sdr_rds_station_bler(const sdr_rds_station* s) {
    if (!s) return 0.0;
    const double all = (double)s->good + (double)s->corrected + (double)s->bad;
    return all > 0.0 ? (double)s->bad / all : 0.0;
}

size_t sdr_rds_station_format(const sdr_rds_station* s, char* buf, size_t n) {
    Out o{n ? buf : nullptr, n, 0};
    if (!s) {
        if (buf && n) buf[0] = 0;
        return 0;
    }
    if (s->pi_valid) o.add("PI: %04X\n", s->pi);
    else o.add("PI: ----\n");
    if (s->have_b) o.add("PTY: %s\nTP: %u", kPty[s->pty & 31], s->tp);
    else o.add("PTY: -\nTP: -");
    if (s->have_0) o.add(" TA: %u MS: %u\n", s->ta, s->ms);
    else o.add(" TA: - MS: -\n");
    char ps[9];
    for (int i = 0; i < 8; i++) ps[i] = printable(s->ps_complete ? s->ps_done[i] : s->ps[i]);
    ps[8] = 0;
    o.add("PS: %s%s\n", ps, s->ps_complete ? "" : " (incomplete)");
    char rt[65];
    unsigned len = s->rt_len <= 64 ? s->rt_len : 64, end = len;
    for (unsigned i = 0; i < len; i++)
        if (((s->rt_seen >> i) & 1u) && s->rt[i] == 0x0D) {
            end = i;
            break;
        }
    for (unsigned i = 0; i < end; i++) rt[i] = ((s->rt_seen >> i) & 1u) ? printable(s->rt[i]) : ' ';
    while (end > 0 && rt[end - 1] == ' ') end--;
    rt[end] = 0;
    o.add("RT: %s\n", rt);
    if (s->ct_valid)
        o.add("CT: %04d-%02u-%02u %02u:%02u UTC %c%u.%u h (MJD %d)\n", (int)s->ct_year, s->ct_month, s->ct_day, s->ct_hour,
              s->ct_minute, s->ct_offset < 0 ? '-' : '+', (unsigned)((s->ct_offset < 0 ? -s->ct_offset : s->ct_offset) / 2),
              (unsigned)((s->ct_offset < 0 ? -s->ct_offset : s->ct_offset) % 2) * 5, (int)s->ct_mjd);
    else o.add("CT: -\n");
    o.add("AF:");
    const unsigned naf = s->af_n <= 25 ? s->af_n : 25;
    for (unsigned i = 0; i < naf; i++) o.add(" %u.%u", s->af[i] / 10u, s->af[i] % 10u);
    if (!naf) o.add(" -");
    o.add("\ngroups: %u", s->ngroups);
    for (int t = 0; t < 32; t++)
        if (s->hist[t]) o.add(" %d%c:%u", t / 2, (t & 1) ? 'B' : 'A', s->hist[t]);
    o.add("\nblocks: good %u corrected %u bad %u BLER %.4f\n", s->good, s->corrected, s->bad, sdr_rds_station_bler(s));
    o.add("slips: %u sync acquired %u lost %u\n", s->slips, s->acquired, s->lost);
    if (buf && n) buf[o.len < n ? o.len : n - 1] = 0;
    return o.len;
}

}  // extern "C"
