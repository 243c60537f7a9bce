// rg_clicks.h -- internal: the click scan (include/mp3rgain_amd_clicks.h) as rg_clicks.hip (kernels, launcher, seam),
// rg_clicks_host.cpp (the serial host twin, the kernels' code walked by one host lane, the finish) and rg_file_verify.hip
// (rg_clicks) share it.  The model of a block, the residual, the flag test, the event monoid, the work of a tile and the fold of
// a plane's tiles are host and device code, written once here for an executor X that says how many lanes work (256 in a
// workgroup, 1 on the host), how they wait for one another and how they add into shared memory -- as rg_flacenc.h is.
//
// Same bytes on every route: the autocorrelation is an exact int64 sum, the recursion and the quantisation are one lane's double
// arithmetic in the encoder's order (rg_fe_levinson_step, rg_fe_quantise_to; everything that includes this header is built with
// -ffp-contract=off), the median is an exact select, and the events of a stretch of samples combine by an associative rule
// (rg_ck_combine), so a plane may be cut anywhere and its parts combined in any bracketing.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_clicks.h"
#include "rg_pcm_plane.h"
#include "rg_stereo.h"   // rg_st_q
#include "rg_flacenc.h"  // the model: rg_fe_window, rg_fe_levinson_step, rg_fe_quantise_to

#define RG_CK_HD RG_ST_HD

// ---- how a plane is cut ------------------------------------------------------------------------------------------------------
#define RG_CK_LANES 256u        // lanes of the tile kernel's workgroup
#define RG_CK_FOLD_LANES 256u   // lanes of the fold kernel's workgroup
#define RG_CK_SPAN 12288u       // samples a workgroup holds: a tile of whole blocks and one block of margin on either side
#define RG_CK_HIST 16u          // samples in front of the span: the history of its first sample (>= RG_CK_MAX_ORDER)
#define RG_CK_MAX_SPAN_BLOCKS (RG_CK_SPAN / 256u)  // 48
#define RG_CK_CHUNK 32u         // samples of one lane's piece of the autocorrelation; every block length is a multiple
#define RG_CK_DIGIT 5u          // bits of one pass of the median's radix select: 6 passes over e < 2^30
#define RG_CK_BINS (1u << RG_CK_DIGIT)
#define RG_CK_NONE 0xFFFFFFFFu

struct RgCkEv {                 // an event: samples [start, last]
    uint32_t start, last, strength, peak_at;
};
struct RgCkInner {              // the events of a stretch that can no longer change
    uint32_t clicks, bursts, widest;
    uint32_t first_click;       // RG_CK_NONE: no click
    uint32_t strongest, strongest_at;  // of the strongest click, the earliest on a tie; 0 and RG_CK_NONE: no click
};
struct RgCkSum {                // the events of a stretch of samples: the monoid
    uint32_t n;                 // events
    uint32_t flagged;           // samples
    RgCkEv first, last;         // the first and the last event (the same when n == 1): a neighbour may still widen them
    RgCkInner in;               // all the others
};  // 64 bytes
struct RgCkTile {               // a tile, and a plane as the sum of its tiles
    RgCkSum sum;
    uint32_t fallback, median_max, nonfinite, nonzero;
};  // 80 bytes
struct RgCkPlane {              // one plane of a launch
    uint64_t off;               // from the arena's base, in bytes (sample-aligned)
    uint64_t first_tile;        // of this plane among the launch's tiles
    uint32_t n;                 // N < 2^32
    uint32_t n_blocks, n_tiles;
    uint32_t format;            // rg_sample_format
};  // 32 bytes

RG_CK_HD uint32_t rg_ck_tile_blocks(uint32_t block) { return RG_CK_SPAN / block - 2u; }

// ---- the model ---------------------------------------------------------------------------------------------------------------
struct RgCkModel {
    int32_t c[RG_CK_MAX_ORDER];
    int32_t shift;
    uint32_t order;
};
RG_CK_HD void rg_ck_fallback(RgCkModel *m) {
    for (uint32_t j = 0; j < RG_CK_MAX_ORDER; ++j) m->c[j] = 0;
    m->c[0] = 2;
    m->c[1] = -1;
    m->shift = 0;
    m->order = 2;
}
// xw[i] of a block of n >= 2 samples
RG_CK_HD int32_t rg_ck_windowed(int32_t q, uint32_t i, uint32_t n) { return (int32_t)(((int64_t)q * rg_fe_window(i, n)) >> 15); }
// the model of a block of n samples from its autocorrelation acf[0 .. P]; true when it fell back
RG_CK_HD bool rg_ck_model(const int64_t *acf, uint32_t n, uint32_t P, RgCkModel *m) {
    rg_ck_fallback(m);
    if (n < 4u * P || acf[0] <= 0) return true;
    double lp[RG_CK_MAX_ORDER], tmp[RG_CK_MAX_ORDER];
    double err = (double)acf[0];
    for (uint32_t i = 0; i < P; ++i) {
        err = rg_fe_levinson_step(acf, lp, tmp, i, err);
        if (!(err > 0.0) && i + 1 < P) return true;  // the encoder's recursion stops here, before order P
    }
    int32_t qc[RG_CK_MAX_ORDER], shift;
    if (!rg_fe_quantise_to(lp, P, 12u, qc, &shift)) return true;
    for (uint32_t j = 0; j < P; ++j) m->c[j] = qc[j];
    m->shift = shift;
    m->order = P;
    return false;
}
// e[n]: q points at q[n], with the plane's samples in front of it; n >= m.order
RG_CK_HD uint32_t rg_ck_abs_res(const int16_t *q, const RgCkModel &m) {
    int64_t s = 0;
    for (uint32_t j = 0; j < m.order; ++j) s += (int64_t)m.c[j] * q[-1 - (int32_t)j];
    const int64_t r = (int64_t)q[0] - (s >> m.shift);
    return (uint32_t)(r < 0 ? -r : r);
}
// the flag test; *strength when flagged
RG_CK_HD bool rg_ck_flagged(uint32_t e, uint32_t S, uint32_t ratio_permille, uint32_t *strength) {
    const uint64_t k = 1000ull * e;
    if (k <= (uint64_t)ratio_permille * S) return false;
    const uint64_t s = k / S;
    *strength = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
    return true;
}

// ---- the event monoid --------------------------------------------------------------------------------------------------------
RG_CK_HD RgCkSum rg_ck_empty() {
    RgCkSum s;
    memset(&s, 0, sizeof s);
    s.in.first_click = s.in.strongest_at = RG_CK_NONE;
    return s;
}
RG_CK_HD RgCkTile rg_ck_empty_tile() {
    RgCkTile t;
    t.sum = rg_ck_empty();
    t.fallback = t.median_max = t.nonfinite = t.nonzero = 0u;
    return t;
}
RG_CK_HD RgCkSum rg_ck_single(uint32_t at, uint32_t strength) {
    RgCkSum s = rg_ck_empty();
    s.n = s.flagged = 1u;
    s.first = s.last = RgCkEv{at, at, strength, at};
    return s;
}
// a <- a and the later event b as one
RG_CK_HD void rg_ck_ev_merge(RgCkEv *a, const RgCkEv &b) {
    a->last = b.last;
    if (b.strength > a->strength) {
        a->strength = b.strength;
        a->peak_at = b.peak_at;
    }
}
// an event that can no longer change, into the counts
RG_CK_HD void rg_ck_inner_add(RgCkInner *in, const RgCkEv &e, uint32_t max_width) {
    const uint32_t w = e.last - e.start + 1u;
    if (w > in->widest) in->widest = w;
    if (w > max_width) {
        in->bursts += 1u;
        return;
    }
    in->clicks += 1u;
    if (e.start < in->first_click) in->first_click = e.start;
    if (e.strength > in->strongest || (e.strength == in->strongest && e.peak_at < in->strongest_at)) {
        in->strongest = e.strength;
        in->strongest_at = e.peak_at;
    }
}
RG_CK_HD void rg_ck_inner_combine(RgCkInner *a, const RgCkInner &b) {
    a->clicks += b.clicks;
    a->bursts += b.bursts;
    if (b.widest > a->widest) a->widest = b.widest;
    if (b.first_click < a->first_click) a->first_click = b.first_click;
    if (b.strongest > a->strongest || (b.strongest == a->strongest && b.strongest_at < a->strongest_at)) {
        a->strongest = b.strongest;
        a->strongest_at = b.strongest_at;
    }
}
// a <- a followed by b, two adjacent stretches; the last event of a and the first of b are one when they are within `gap`
RG_CK_HD void rg_ck_combine(RgCkSum *a, const RgCkSum &b, uint32_t gap, uint32_t max_width) {
    if (!b.n) return;
    if (!a->n) {
        *a = b;
        return;
    }
    rg_ck_inner_combine(&a->in, b.in);
    a->flagged += b.flagged;
    if (b.first.start - a->last.last <= gap) {
        RgCkEv m = a->last;
        rg_ck_ev_merge(&m, b.first);
        if (a->n == 1u) a->first = m;
        if (b.n == 1u) {
            a->last = m;
        } else {
            if (a->n > 1u) rg_ck_inner_add(&a->in, m, max_width);
            a->last = b.last;
        }
        a->n += b.n - 1u;
    } else {
        if (a->n > 1u) rg_ck_inner_add(&a->in, a->last, max_width);
        if (b.n > 1u) rg_ck_inner_add(&a->in, b.first, max_width);
        a->last = b.last;
        a->n += b.n;
    }
}
RG_CK_HD void rg_ck_combine_tile(RgCkTile *a, const RgCkTile &b, uint32_t gap, uint32_t max_width) {
    rg_ck_combine(&a->sum, b.sum, gap, max_width);
    a->fallback += b.fallback;
    if (b.median_max > a->median_max) a->median_max = b.median_max;
    a->nonfinite += b.nonfinite;
    a->nonzero |= b.nonzero;
}
// every event of a whole plane counted
RG_CK_HD RgCkInner rg_ck_close(const RgCkSum &s, uint32_t max_width) {
    RgCkInner in = s.in;
    if (s.n) rg_ck_inner_add(&in, s.first, max_width);
    if (s.n > 1u) rg_ck_inner_add(&in, s.last, max_width);
    return in;
}
// events that start in tile t of a plane: its events, less its first when that continues the tile before
RG_CK_HD uint32_t rg_ck_starts(const RgCkTile *recs, uint32_t t, uint32_t gap) {
    const RgCkSum &s = recs[t].sum;
    if (!s.n) return 0u;
    const bool joined = t > 0u && recs[t - 1u].sum.n && s.first.start - recs[t - 1u].sum.last.last <= gap;
    return s.n - (joined ? 1u : 0u);
}

// ---- samples -----------------------------------------------------------------------------------------------------------------
RG_CK_HD int32_t rg_ck_q_at(const unsigned char *plane, uint32_t format, uint64_t k, bool *finite) {
#if defined(__HIP_DEVICE_COMPILE__)  // planes are sample-aligned in device memory
    if (format == RG_FMT_S16_PLANAR) {
        *finite = true;
        return reinterpret_cast<const int16_t *>(plane)[k];
    }
    const uint32_t raw = reinterpret_cast<const uint32_t *>(plane)[k];
#else
    if (format == RG_FMT_S16_PLANAR) {
        *finite = true;
        int16_t v;
        memcpy(&v, plane + 2u * k, 2);
        return v;
    }
    uint32_t raw;
    memcpy(&raw, plane + 4u * k, 4);
#endif
    return format == RG_FMT_F32_PLANAR ? rg_st_q<RG_FMT_F32_PLANAR>(raw, finite) : rg_st_q<RG_FMT_S32_PLANAR>(raw, finite);
}

// ---- the work of a tile ------------------------------------------------------------------------------------------------------
struct RgCkWork {
    // q[RG_CK_HIST + i]: sample i of the span.  Once the residuals stand, the same bytes hold the select's histograms
    // (RG_CK_MAX_SPAN_BLOCKS x RG_CK_BINS counts) and behind them the lanes' sums (RG_CK_LANES x RgCkSum)
    alignas(16) int16_t q[RG_CK_HIST + RG_CK_SPAN];
    uint32_t e[RG_CK_SPAN];  // before the residuals: the windowed signal
    int64_t acf[RG_CK_MAX_SPAN_BLOCKS][RG_CK_MAX_ORDER + 1];
    RgCkModel model[RG_CK_MAX_SPAN_BLOCKS];
    uint32_t med[RG_CK_MAX_SPAN_BLOCKS], rank[RG_CK_MAX_SPAN_BLOCKS];
    uint32_t fallback, nonfinite, nonzero, median_max;
};
static_assert(sizeof(int16_t) * (RG_CK_HIST + RG_CK_SPAN) >= 4u * RG_CK_MAX_SPAN_BLOCKS * RG_CK_BINS + RG_CK_LANES * sizeof(RgCkSum), "the aliases fit");
#define RG_CK_LDS_BYTES ((uint32_t)sizeof(RgCkWork))

// the serial executor: one lane
struct RgCkSerial {
    RG_CK_HD uint32_t tid() const { return 0; }
    RG_CK_HD uint32_t nt() const { return 1; }
    RG_CK_HD void sync() const {}
    RG_CK_HD void add32(uint32_t *p, uint32_t v) const { *p += v; }
    RG_CK_HD void max32(uint32_t *p, uint32_t v) const { *p = v > *p ? v : *p; }
    RG_CK_HD void add64(int64_t *p, int64_t v) const { *p += v; }
};

// where tile t of a plane lies
struct RgCkCut {
    uint32_t b0, b1;    // its blocks [b0, b1)
    uint32_t sb0, nsb;  // the span's blocks [sb0, sb0 + nsb): one more on either side where the plane has one
    uint64_t s0;        // the span's first sample
    uint32_t span_len;
    uint64_t t0, t1;    // its samples [t0, t1)
};
RG_CK_HD RgCkCut rg_ck_cut(const RgCkPlane &pl, uint32_t B, uint32_t t) {
    const uint32_t tb = rg_ck_tile_blocks(B);
    RgCkCut c;
    c.b0 = t * tb;
    c.b1 = c.b0 + tb < pl.n_blocks ? c.b0 + tb : pl.n_blocks;
    c.sb0 = c.b0 ? c.b0 - 1u : 0u;
    const uint32_t sb1 = c.b1 + 1u < pl.n_blocks ? c.b1 + 1u : pl.n_blocks;
    c.nsb = sb1 - c.sb0;
    c.s0 = (uint64_t)c.sb0 * B;
    const uint64_t s1 = (uint64_t)sb1 * B < pl.n ? (uint64_t)sb1 * B : pl.n;
    c.span_len = (uint32_t)(s1 - c.s0);
    c.t0 = (uint64_t)c.b0 * B;
    c.t1 = (uint64_t)c.b1 * B < pl.n ? (uint64_t)c.b1 * B : pl.n;
    return c;
}
// samples of block `blk` of the span
RG_CK_HD uint32_t rg_ck_block_len(const RgCkPlane &pl, const RgCkCut &c, uint32_t B, uint32_t blk) {
    const uint64_t left = pl.n - (uint64_t)(c.sb0 + blk) * B;
    return left < B ? (uint32_t)left : B;
}
// S(n) for the samples of block `blk` of the span
RG_CK_HD uint32_t rg_ck_scale(const RgCkWork &w, uint32_t blk, uint32_t nsb, uint32_t floor) {
    uint32_t S = w.med[blk] > floor ? w.med[blk] : floor;
    if (blk > 0u && w.med[blk - 1u] > S) S = w.med[blk - 1u];
    if (blk + 1u < nsb && w.med[blk + 1u] > S) S = w.med[blk + 1u];
    return S;
}

// Tile t of plane `pl` (at `plane`): the residuals and the medians of its span into w, then
//   ev_out == nullptr  its record -> *out
//   ev_out != nullptr  the events that start in it -> ev_out[first_event ..], as far as they are among the plane's first
//                      o.max_events; `recs` are the plane's tile records, by which an event is followed beyond the tile
template <class X>
RG_CK_HD void rg_ck_tile(X &x, RgCkWork &w, const unsigned char *plane, const RgCkPlane &pl, const rg_clicks_opts &o, uint32_t t, RgCkTile *out,
                         const RgCkTile *recs, uint32_t first_event, RgCkEv *ev_out) {
    const uint32_t B = o.block_samples, P = o.order, tid = x.tid(), nt = x.nt();
    const RgCkCut c = rg_ck_cut(pl, B, t);
    for (uint32_t i = tid; i < c.nsb * (RG_CK_MAX_ORDER + 1u); i += nt) w.acf[i / (RG_CK_MAX_ORDER + 1u)][i % (RG_CK_MAX_ORDER + 1u)] = 0;
    if (tid == 0) w.fallback = w.nonfinite = w.nonzero = w.median_max = 0u;
    x.sync();
    // q of the span and of the history in front of it; what the tile itself counts
    {
        uint32_t nonfinite = 0, nonzero = 0;
        for (uint32_t i = tid; i < RG_CK_HIST + c.span_len; i += nt) {
            const int64_t g = (int64_t)c.s0 + (int64_t)i - (int64_t)RG_CK_HIST;
            int32_t q = 0;
            if (g >= 0) {
                bool finite;
                q = rg_ck_q_at(plane, pl.format, (uint64_t)g, &finite);
                if ((uint64_t)g >= c.t0 && (uint64_t)g < c.t1) {
                    nonfinite += finite ? 0u : 1u;
                    nonzero |= q ? 1u : 0u;
                }
            }
            w.q[i] = (int16_t)q;
        }
        if (nonfinite) x.add32(&w.nonfinite, nonfinite);
        if (nonzero) x.max32(&w.nonzero, 1u);
    }
    x.sync();
    // the windowed signal of every block that gets a model of its own
    int32_t *xw = reinterpret_cast<int32_t *>(w.e);
    for (uint32_t i = tid; i < c.span_len; i += nt) {
        const uint32_t blk = i / B, nb = rg_ck_block_len(pl, c, B, blk);
        xw[i] = nb >= 4u * P ? rg_ck_windowed(w.q[RG_CK_HIST + i], i - blk * B, nb) : 0;
    }
    x.sync();
    // its autocorrelation: exact, so the lanes may add in any order
    for (uint32_t ch = tid; ch < (c.span_len + RG_CK_CHUNK - 1u) / RG_CK_CHUNK; ch += nt) {
        const uint32_t base = ch * RG_CK_CHUNK, blk = base / B, jb = base - blk * B, nb = rg_ck_block_len(pl, c, B, blk);
        if (nb < 4u * P) continue;
        const uint32_t je = jb + RG_CK_CHUNK < nb ? jb + RG_CK_CHUNK : nb;
        int64_t r[RG_CK_MAX_ORDER + 1u];
#pragma unroll
        for (uint32_t l = 0; l <= RG_CK_MAX_ORDER; ++l) r[l] = 0;
        const int32_t *xb = xw + blk * B;
        for (uint32_t i = jb; i < je; ++i) {
            const int64_t v = xb[i];
#pragma unroll
            for (uint32_t l = 0; l <= RG_CK_MAX_ORDER; ++l)
                if (l <= P && l <= i) r[l] += v * xb[i - l];
        }
#pragma unroll
        for (uint32_t l = 0; l <= RG_CK_MAX_ORDER; ++l)
            if (l <= P && r[l]) x.add64(&w.acf[blk][l], r[l]);
    }
    x.sync();
    // one lane per block: the recursion and the quantisation
    for (uint32_t blk = tid; blk < c.nsb; blk += nt) {
        const bool fell = rg_ck_model(w.acf[blk], rg_ck_block_len(pl, c, B, blk), P, &w.model[blk]);
        if (fell && c.sb0 + blk >= c.b0 && c.sb0 + blk < c.b1) x.add32(&w.fallback, 1u);
    }
    x.sync();
    for (uint32_t i = tid; i < c.span_len; i += nt) {
        const RgCkModel &m = w.model[i / B];
        w.e[i] = c.s0 + i < m.order ? 0u : rg_ck_abs_res(&w.q[RG_CK_HIST + i], m);
    }
    // the lower median of every block: a radix select, all blocks at once (w.med: the digits found so far)
    uint32_t *hist = reinterpret_cast<uint32_t *>(w.q);
    for (uint32_t blk = tid; blk < c.nsb; blk += nt) {
        w.med[blk] = 0u;
        w.rank[blk] = (rg_ck_block_len(pl, c, B, blk) - 1u) / 2u;
    }
    for (int32_t pass = 30 / (int32_t)RG_CK_DIGIT - 1; pass >= 0; --pass) {
        const uint32_t sh = (uint32_t)pass * RG_CK_DIGIT;
        x.sync();
        for (uint32_t i = tid; i < c.nsb * RG_CK_BINS; i += nt) hist[i] = 0u;
        x.sync();
        for (uint32_t i = tid; i < c.span_len; i += nt) {
            const uint32_t blk = i / B, v = w.e[i];
            if ((v >> (sh + RG_CK_DIGIT)) == w.med[blk]) x.add32(&hist[blk * RG_CK_BINS + ((v >> sh) & (RG_CK_BINS - 1u))], 1u);
        }
        x.sync();
        for (uint32_t blk = tid; blk < c.nsb; blk += nt) {
            uint32_t r = w.rank[blk], bin = 0;
            for (; bin < RG_CK_BINS - 1u; ++bin) {
                const uint32_t h = hist[blk * RG_CK_BINS + bin];
                if (r < h) break;
                r -= h;
            }
            w.rank[blk] = r;
            w.med[blk] = (w.med[blk] << RG_CK_DIGIT) | bin;
        }
    }
    x.sync();
    if (ev_out) {  // the events that start here, by one lane
        if (tid != 0) return;
        RgCkEv cur{0u, 0u, 0u, 0u};
        bool have = false, foreign = false;
        uint32_t idx = first_event;
        const bool prev = t > 0u && recs[t - 1u].sum.n;
        for (uint64_t n = c.t0; n <= c.t1; ++n) {
            uint32_t s = 0;
            const uint32_t i = (uint32_t)(n - c.s0);
            const bool end = n == c.t1;
            if (!end && !rg_ck_flagged(w.e[i], rg_ck_scale(w, i / B, c.nsb, o.floor), o.ratio_permille, &s)) continue;
            if (!end && have && (uint32_t)n - cur.last <= o.gap) {
                rg_ck_ev_merge(&cur, RgCkEv{(uint32_t)n, (uint32_t)n, s, (uint32_t)n});
                continue;
            }
            if (have) {
                if (end)  // it may go on in the tiles that follow
                    for (uint32_t u = t + 1u; u < pl.n_tiles && recs[u].sum.n && recs[u].sum.first.start - cur.last <= o.gap; ++u) {
                        rg_ck_ev_merge(&cur, recs[u].sum.first);
                        if (recs[u].sum.n > 1u) break;
                    }
                if (!foreign) {
                    if (idx < o.max_events) ev_out[idx] = cur;
                    ++idx;
                }
            }
            if (end) break;
            foreign = !have && prev && (uint32_t)n - recs[t - 1u].sum.last.last <= o.gap;  // the tile before began it
            have = true;
            cur = RgCkEv{(uint32_t)n, (uint32_t)n, s, (uint32_t)n};
        }
        return;
    }
    for (uint32_t blk = tid; blk < c.nsb; blk += nt)
        if (c.sb0 + blk >= c.b0 && c.sb0 + blk < c.b1) x.max32(&w.median_max, w.med[blk]);
    // the flags: a lane takes a run of consecutive samples, the runs combine in order by a tree
    RgCkSum *sums = reinterpret_cast<RgCkSum *>(w.q + 2u * RG_CK_MAX_SPAN_BLOCKS * RG_CK_BINS);
    {
        const uint32_t len = (uint32_t)(c.t1 - c.t0), run = (len + nt - 1u) / nt;
        const uint32_t a = tid * run < len ? tid * run : len, b = a + run < len ? a + run : len;
        RgCkSum acc = rg_ck_empty();
        uint32_t blk_of = RG_CK_NONE, S = 0;
        for (uint32_t k = a; k < b; ++k) {
            const uint32_t i = (uint32_t)(c.t0 - c.s0) + k, blk = i / B;
            if (blk != blk_of) {
                blk_of = blk;
                S = rg_ck_scale(w, blk, c.nsb, o.floor);
            }
            uint32_t s;
            if (rg_ck_flagged(w.e[i], S, o.ratio_permille, &s)) rg_ck_combine(&acc, rg_ck_single((uint32_t)(c.t0 + k), s), o.gap, o.max_width);
        }
        sums[tid] = acc;
    }
    x.sync();
    for (uint32_t step = 1; step < nt; step <<= 1) {
        if ((tid & (2u * step - 1u)) == 0u && tid + step < nt) rg_ck_combine(&sums[tid], sums[tid + step], o.gap, o.max_width);
        x.sync();
    }
    if (tid == 0) {
        out->sum = sums[0];
        out->fallback = w.fallback;
        out->median_max = w.median_max;
        out->nonfinite = w.nonfinite;
        out->nonzero = w.nonzero;
    }
}

// ---- the fold of a plane's tiles ---------------------------------------------------------------------------------------------
struct RgCkFoldWork {
    RgCkTile acc[RG_CK_FOLD_LANES];
    uint32_t starts[RG_CK_FOLD_LANES];
};
// recs[0 .. pl.n_tiles) -> *out, the plane; tile_first[t] <- the number of events that start before tile t, and emit(t) for every
// tile in which one of the plane's first o.max_events events starts.  A lane folds a run of consecutive tiles.
template <class X, class E>
RG_CK_HD void rg_ck_fold(X &x, RgCkFoldWork &w, const RgCkPlane &pl, const rg_clicks_opts &o, const RgCkTile *recs, uint32_t *tile_first, RgCkTile *out,
                         E &emit) {
    const uint32_t tid = x.tid(), nt = x.nt();
    const uint32_t run = (pl.n_tiles + nt - 1u) / nt;
    const uint32_t a = tid * run < pl.n_tiles ? tid * run : pl.n_tiles, b = a + run < pl.n_tiles ? a + run : pl.n_tiles;
    RgCkTile acc = rg_ck_empty_tile();
    uint32_t starts = 0;
    for (uint32_t t = a; t < b; ++t) {
        starts += rg_ck_starts(recs, t, o.gap);
        rg_ck_combine_tile(&acc, recs[t], o.gap, o.max_width);
    }
    w.acc[tid] = acc;
    w.starts[tid] = starts;
    x.sync();
    if (tid == 0) {  // the lanes' runs in order, and where each run's events begin to count
        RgCkTile all = rg_ck_empty_tile();
        uint32_t before = 0;
        for (uint32_t l = 0; l < nt; ++l) {
            rg_ck_combine_tile(&all, w.acc[l], o.gap, o.max_width);
            const uint32_t s = w.starts[l];
            w.starts[l] = before;
            before += s;
        }
        *out = all;
    }
    x.sync();
    uint32_t before = w.starts[tid];
    for (uint32_t t = a; t < b; ++t) {
        const uint32_t s = rg_ck_starts(recs, t, o.gap);
        tile_first[t] = before;
        if (s && before < o.max_events) emit(t);
        before += s;
    }
}

// ---- rg_clicks_host.cpp (plain C++: no device, no context) -------------------------------------------------------------------
// NULL -> the defaults; RG_ERR_INVALID_ARG for an option outside its range
int rg_ck_options(const rg_clicks_opts *opts, rg_clicks_opts *out, char *err, size_t err_len);
// The planes of track i, described by `t`, in an arena of `arena_bytes` bytes -> out[0 .. t.channels).  RG_ERR_FORMAT unless it is
// 1 .. 8 channels of one of the three formats and fewer than 2^32 frames; RG_ERR_INVALID_ARG unless the planes lie inside the
// arena, sample-aligned.  The text goes to err[err_len].  first_tile is rg_ck_plan's to set.
int rg_ck_track_planes(size_t i, const rg_track_desc &t, const rg_clicks_opts &o, size_t arena_bytes, RgCkPlane *out, char *err, size_t err_len);
// the tiles of the `n` planes of a launch; returns their number
uint64_t rg_ck_plan(RgCkPlane *planes, size_t n);
// one plane from host memory: the definitions, serially -> the plane's sums, and its first min(events, K) events into ev[K]
RgCkTile rg_ck_serial_host(const unsigned char *arena, const RgCkPlane &pl, const rg_clicks_opts &o, RgCkEv *ev);
// ... and by the kernels' tile and fold code on one lane
RgCkTile rg_ck_folded_host(const unsigned char *arena, const RgCkPlane &pl, const rg_clicks_opts &o, RgCkEv *ev);
// the finish: the record of a track from its planes' sums po[0 .. channels) and their event slots ev[channels][K]; `events`: the
// record's row of K, or NULL
void rg_ck_fill(const rg_track_desc &t, const rg_clicks_opts &o, uint32_t dropped_frames, const RgCkTile *po, const RgCkEv *ev, rg_clicks_result *out,
                rg_clicks_event *events);
// routes 0 and 2 of rg_clicks_arena
int rg_ck_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_clicks_opts *opts, const void *arena, size_t arena_bytes, rg_clicks_result *out,
                     rg_clicks_event *events, char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` planes in the device arena at `d_arena` (allocated in whole 16-byte words): the kernels on `s`, po[i] <- plane i and
// ev[i * K ..] <- its first events (zero beyond them); `s` has been synchronised on return
int rg_ck_device(rg_ctx *c, const unsigned char *d_arena, RgCkPlane *planes, size_t n, const rg_clicks_opts &o, RgCkTile *po, RgCkEv *ev, hipStream_t s);
#endif
