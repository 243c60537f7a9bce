// rg_stats.h -- internal: the PCM defect scan (include/mp3rgain_amd_stats.h) as rg_stats.hip (kernels, launcher, seams),
// rg_stats_host.cpp (the serial host twin and the kernels' fold arithmetic on the host) and rg_file_verify.hip (rg_pcm_stats)
// share it.  What one lane's chunk comes to, how two neighbours combine and how a plane is finished is host and device code,
// written once here; the kernels and the folded host route differ only in who walks the lanes.
//
// The counts, the sum, the OR, the minimum and the maximum are commutative.  The stretches are not: a run of clipped or zero
// samples crosses whatever boundary a plane is cut at.  So a part -- a lane's chunk, a subtree, a tile, a run of tiles --
// keeps, per predicate, the stretch that touches its first sample and the one that touches its last open, and counts only the
// stretches that are closed on both sides inside it; combining two parts closes or merges what meets at the junction.  A part
// that is one stretch from end to end (pre == n) stays open on both sides, which is what lets a stretch grow across three and
// more parts.  All lengths and positions are below N < 2^32.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_stats.h"
#include "rg_pcm_plane.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_STATS_HD __host__ __device__ inline
#else
#define RG_STATS_HD inline
#endif

// ---- how a plane is cut ---------------------------------------------------------------------------------------------------
#define RG_STATS_CHUNK 32u                               // C: samples one lane walks (64 bytes of S16, 128 of S32 / F32)
#define RG_STATS_BLOCK 256u                              // lanes of a tile block = chunks of a tile
#define RG_STATS_LEVELS 8                                // log2(RG_STATS_BLOCK)
#define RG_STATS_TILE (RG_STATS_CHUNK * RG_STATS_BLOCK)  // T: samples of a tile
#define RG_STATS_FOLD_LANES 64u                          // F: lanes of the fold kernel (one wave per plane)
#define RG_STATS_FOLD_LEVELS 6                           // log2(RG_STATS_FOLD_LANES)
#define RG_STATS_ANY_TEST 1                              // the product's lanes test four samples at once first: see DESIGN 12.5
#define RG_STATS_NONE 0xFFFFFFFFu                       // "no counted stretch": a position is at most 2^32 - 2

// The stretches of one predicate over a part of n samples.  A stretch has a class (+1 / -1 for clipping, 1 for zero); class 0
// is "no stretch".  pre == n (n > 0) says the whole part is one stretch; then suf == n as well.
struct RgStatsRuns {
    uint32_t pre, suf;       // length of the stretch that starts at the part's first sample / ends at its last (0: none)
    int32_t pre_cls, suf_cls;
    uint32_t count, longest; // of the stretches closed on both sides inside the part: those at the threshold, the longest
    uint32_t first;          // where the first counted one starts, from the part's first sample (RG_STATS_NONE: none)
};  // 28 bytes
struct RgStatsPart {
    RgStatsRuns clip, zero;
    int64_t sum;
    uint32_t n;              // samples of the part
    int32_t mn, mx;          // integers: the values; float: rg_stats_fkey of the finite ones
    uint32_t or_mask, clipped, zeros, nonfinite;
    uint32_t reserved;
};  // 96 bytes

// One plane of a launch
struct RgStatsPlane {
    uint64_t off;         // from the arena's base, in bytes (sample-aligned)
    uint64_t first_tile;  // of this plane among the launch's tiles (the tiles of one format are contiguous)
    uint32_t n;           // N < 2^32
    uint32_t n_tiles;
    uint32_t run;         // tile records one lane of the fold kernel folds (>= 1)
    uint32_t format;      // rg_sample_format
    int32_t P, M;         // integer formats: class +1 when v >= P, -1 when v <= M
    uint32_t bits;        // b (W for float, where it is not used)
    uint32_t reserved;
};  // 48 bytes

// ---- samples ---------------------------------------------------------------------------------------------------------------
RG_STATS_HD float rg_stats_as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// finite floats in their own order as int32 (-0.0 sorts below +0.0), and back
RG_STATS_HD int32_t rg_stats_fkey(uint32_t bits) { return (int32_t)(bits & 0x80000000u ? bits ^ 0x7FFFFFFFu : bits); }
RG_STATS_HD float rg_stats_funkey(int32_t key) { return rg_stats_as_float(key < 0 ? (uint32_t)key ^ 0x7FFFFFFFu : (uint32_t)key); }
RG_STATS_HD int32_t rg_stats_full_scale(uint32_t format, uint32_t bits) {  // P
    const uint32_t w = rg_pcm_width(format);
    return (int32_t)((((uint32_t)1 << (bits - 1)) - 1u) << (w - bits));
}
RG_STATS_HD int32_t rg_stats_minus_full_scale(uint32_t format) { return format == RG_FMT_S16_PLANAR ? -32768 : INT32_MIN; }  // M

// What a sample is.  `raw`: the stored pattern, an S16 sample sign-extended to 32 bits.
template <int FMT>
RG_STATS_HD void rg_stats_classify(uint32_t raw, int32_t P, int32_t M, int32_t *cls, bool *zero, bool *finite) {
    if (FMT == RG_FMT_F32_PLANAR) {
        const float x = rg_stats_as_float(raw);
        *finite = (raw & 0x7F800000u) != 0x7F800000u;
        *cls = !*finite ? 0 : (x >= 1.0f ? 1 : (x <= -1.0f ? -1 : 0));
        *zero = (raw & 0x7FFFFFFFu) == 0u;
    } else {
        const int32_t v = (int32_t)raw;
        *finite = true;
        *cls = v >= P ? 1 : (v <= M ? -1 : 0);
        *zero = v == 0;
    }
}
// a sample that takes part in min, max, sum and or_mask.  q of a float: x * 2^23 is exact in float as well (a power of two,
// and no result is subnormal or overflows after the clamp), so rintf gives llrint's integer
template <int FMT>
RG_STATS_HD void rg_stats_take(uint32_t raw, RgStatsPart *p) {
    if (FMT == RG_FMT_F32_PLANAR) {
        const int32_t key = rg_stats_fkey(raw);
        p->mn = key < p->mn ? key : p->mn;
        p->mx = key > p->mx ? key : p->mx;
        p->sum += (int64_t)rintf(fminf(fmaxf(rg_stats_as_float(raw), -256.0f), 256.0f) * 8388608.0f);
    } else {
        const int32_t v = (int32_t)raw;
        p->mn = v < p->mn ? v : p->mn;
        p->mx = v > p->mx ? v : p->mx;
        p->sum += v;
        p->or_mask |= FMT == RG_FMT_S16_PLANAR ? raw & 0xFFFFu : raw;
    }
}

// ---- stretches -------------------------------------------------------------------------------------------------------------
RG_STATS_HD RgStatsRuns rg_stats_no_runs() { return RgStatsRuns{0u, 0u, 0, 0, 0u, 0u, RG_STATS_NONE}; }
RG_STATS_HD RgStatsPart rg_stats_empty() {
    RgStatsPart p;
    p.clip = rg_stats_no_runs();
    p.zero = rg_stats_no_runs();
    p.sum = 0;
    p.n = 0;
    p.mn = INT32_MAX;
    p.mx = INT32_MIN;
    p.or_mask = p.clipped = p.zeros = p.nonfinite = p.reserved = 0;
    return p;
}
// a stretch [start, start + len) that is closed on both sides inside the part (start > 0)
RG_STATS_HD void rg_stats_closed(RgStatsRuns *r, uint32_t start, uint32_t len, uint32_t min_run) {
    if (len >= min_run) {
        ++r->count;
        if (r->first == RG_STATS_NONE) r->first = start;
    }
    r->longest = len > r->longest ? len : r->longest;
}
// the stretch a walk is in: class 0 = none
struct RgStatsWalk {
    uint32_t start, len;
    int32_t cls;
};
// sample j of a chunk has class `cls`
RG_STATS_HD void rg_stats_feed(RgStatsRuns *r, RgStatsWalk *w, int32_t cls, uint32_t j, uint32_t min_run) {
    if (cls == w->cls) {
        w->len += cls != 0;
        return;
    }
    if (w->cls) {  // a stretch ends in front of j
        if (w->start == 0) {
            r->pre = w->len;
            r->pre_cls = w->cls;
        } else {
            rg_stats_closed(r, w->start, w->len, min_run);
        }
    }
    w->cls = cls;
    w->start = j;
    w->len = cls != 0;
}
// the chunk ends: the stretch the walk is in touches its last sample
RG_STATS_HD void rg_stats_walk_end(RgStatsRuns *r, const RgStatsWalk &w) {
    if (!w.cls) return;
    r->suf = w.len;
    r->suf_cls = w.cls;
    if (w.start == 0) {  // the whole chunk
        r->pre = w.len;
        r->pre_cls = w.cls;
    }
}

// ---- one lane's chunk ------------------------------------------------------------------------------------------------------
template <int FMT>
RG_STATS_HD void rg_stats_step(uint32_t raw, uint32_t j, int32_t P, int32_t M, uint32_t min_clip, uint32_t min_zero, RgStatsPart *p, RgStatsWalk *wc,
                               RgStatsWalk *wz) {
    int32_t cls;
    bool zero, finite;
    rg_stats_classify<FMT>(raw, P, M, &cls, &zero, &finite);
    if (finite) rg_stats_take<FMT>(raw, p);
    else ++p->nonfinite;
    p->clipped += cls != 0;
    p->zeros += zero;
    rg_stats_feed(&p->clip, wc, cls, j, min_clip);
    rg_stats_feed(&p->zero, wz, zero ? 1 : 0, j, min_zero);
}
// `n` samples, sample j = get(j) (the stored pattern, S16 sign-extended).  With ANY four samples that hold neither a
// full-scale, a zero nor a non-finite one end the open stretches once and skip the bookkeeping: same part either way.
template <int FMT, bool ANY, class Get>
RG_STATS_HD void rg_stats_chunk(Get get, uint32_t n, int32_t P, int32_t M, uint32_t min_clip, uint32_t min_zero, RgStatsPart *out) {
    RgStatsPart p = rg_stats_empty();
    RgStatsWalk wc{0u, 0u, 0}, wz{0u, 0u, 0};
    uint32_t j = 0;
    if (ANY) {
        for (; j + 4 <= n; j += 4) {
            uint32_t raw[4];
            bool any = false;
            for (uint32_t k = 0; k < 4; ++k) {
                int32_t cls;
                bool zero, finite;
                raw[k] = get(j + k);
                rg_stats_classify<FMT>(raw[k], P, M, &cls, &zero, &finite);
                any = any || cls != 0 || zero || !finite;
            }
            if (any) {
                for (uint32_t k = 0; k < 4; ++k) rg_stats_step<FMT>(raw[k], j + k, P, M, min_clip, min_zero, &p, &wc, &wz);
            } else {
                rg_stats_feed(&p.clip, &wc, 0, j, min_clip);
                rg_stats_feed(&p.zero, &wz, 0, j, min_zero);
                for (uint32_t k = 0; k < 4; ++k) rg_stats_take<FMT>(raw[k], &p);
            }
        }
    }
    for (; j < n; ++j) rg_stats_step<FMT>(get(j), j, P, M, min_clip, min_zero, &p, &wc, &wz);
    rg_stats_walk_end(&p.clip, wc);
    rg_stats_walk_end(&p.zero, wz);
    p.n = n;
    *out = p;
}

// ---- folding ---------------------------------------------------------------------------------------------------------------
// a (na > 0 samples) <- a || b (nb > 0 samples), one predicate
RG_STATS_HD void rg_stats_runs_combine(RgStatsRuns *a, uint32_t na, const RgStatsRuns &b, uint32_t nb, uint32_t min_run) {
    const bool whole_a = a->pre == na, whole_b = b.pre == nb;
    const uint32_t sa = a->suf;
    if (sa && b.pre && a->suf_cls == b.pre_cls) {  // one stretch across the junction
        const uint32_t m = sa + b.pre;
        if (whole_a) a->pre = m;
        if (!whole_a && !whole_b) rg_stats_closed(a, na - sa, m, min_run);
        if (whole_b) {
            a->suf = m;
        } else {
            a->suf = b.suf;
            a->suf_cls = b.suf_cls;
        }
    } else {  // the junction closes what touches it, unless that is open at the part's other end
        if (sa && !whole_a) rg_stats_closed(a, na - sa, sa, min_run);
        if (b.pre && !whole_b) rg_stats_closed(a, na, b.pre, min_run);
        a->suf = b.suf;
        a->suf_cls = b.suf_cls;
    }
    a->count += b.count;
    a->longest = b.longest > a->longest ? b.longest : a->longest;
    if (a->first == RG_STATS_NONE && b.first != RG_STATS_NONE) a->first = na + b.first;
}
// a <- a || b
RG_STATS_HD void rg_stats_combine(RgStatsPart *a, const RgStatsPart &b, uint32_t min_clip, uint32_t min_zero) {
    if (!b.n) return;
    if (!a->n) {
        *a = b;
        return;
    }
    rg_stats_runs_combine(&a->clip, a->n, b.clip, b.n, min_clip);
    rg_stats_runs_combine(&a->zero, a->n, b.zero, b.n, min_zero);
    a->sum += b.sum;
    a->n += b.n;
    a->mn = b.mn < a->mn ? b.mn : a->mn;
    a->mx = b.mx > a->mx ? b.mx : a->mx;
    a->or_mask |= b.or_mask;
    a->clipped += b.clipped;
    a->zeros += b.zeros;
    a->nonfinite += b.nonfinite;
}

// tile `t` of a plane of `n` samples: [*start, *start + return)
RG_STATS_HD uint32_t rg_stats_tile_window(uint32_t n, uint32_t t, uint32_t *start) {
    *start = t * RG_STATS_TILE;
    return n - *start < RG_STATS_TILE ? n - *start : RG_STATS_TILE;
}
// lane `lane`'s chunk of a window of `wlen` samples: [*start, *start + return) of the window
RG_STATS_HD uint32_t rg_stats_lane_chunk(uint32_t wlen, uint32_t lane, uint32_t *start) {
    *start = lane * RG_STATS_CHUNK;
    if (*start >= wlen) return 0;
    return wlen - *start < RG_STATS_CHUNK ? wlen - *start : RG_STATS_CHUNK;
}
// lane `lane` of the fold kernel folds tile records [*lo, return) of its plane
RG_STATS_HD uint32_t rg_stats_lane_run(uint32_t n_tiles, uint32_t run, uint32_t lane, uint32_t *lo) {
    const uint64_t a = (uint64_t)lane * run, b = a + run;
    *lo = (uint32_t)(a < n_tiles ? a : n_tiles);
    return (uint32_t)(b < n_tiles ? b : n_tiles);
}

// the plane's numbers from the fold of all of it: here the stretches at the plane's ends are closed (clipping) or become the
// edge silence (zero)
RG_STATS_HD rg_pcm_stats_channel rg_stats_finish(const RgStatsPart &all, uint32_t format, uint32_t min_clip) {
    rg_pcm_stats_channel c;
    const uint32_t n = all.n;
    const bool is_float = format == RG_FMT_F32_PLANAR;
    if (n == all.nonfinite) {  // nothing took part
        c.min = c.max = 0.0;
    } else if (is_float) {
        c.min = (double)rg_stats_funkey(all.mn) + 0.0;  // (-0.0 + 0.0 is +0.0)
        c.max = (double)rg_stats_funkey(all.mx) + 0.0;
    } else {
        c.min = (double)all.mn;
        c.max = (double)all.mx;
    }
    c.sum = all.sum;
    c.or_mask = all.or_mask;
    c.effective_bits = all.or_mask ? rg_pcm_width(format) - (uint32_t)__builtin_ctz(all.or_mask) : 0u;
    c.clipped = all.clipped;
    RgStatsRuns r = all.clip;
    if (n && r.pre == n) {
        r.count = n >= min_clip;
        r.longest = n;
        r.first = n >= min_clip ? 0u : RG_STATS_NONE;
    } else {
        if (r.pre) {
            r.longest = r.pre > r.longest ? r.pre : r.longest;
            if (r.pre >= min_clip) {
                ++r.count;
                r.first = 0u;
            }
        }
        if (r.suf) {
            r.longest = r.suf > r.longest ? r.suf : r.longest;
            if (r.suf >= min_clip) {
                ++r.count;
                if (r.first == RG_STATS_NONE) r.first = n - r.suf;
            }
        }
    }
    c.clip_runs = r.count;
    c.longest_clip_run = r.longest;
    c.first_clip_run = r.first == RG_STATS_NONE ? n : r.first;
    c.zeros = all.zeros;
    c.lead_zeros = all.zero.pre;
    c.trail_zeros = all.zero.suf;
    c.zero_runs = all.zero.count;
    c.longest_zero_run = all.zero.longest;
    c.nonfinite = all.nonfinite;
    return c;
}

// ---- rg_stats_host.cpp (plain C++: no device, no context) ------------------------------------------------------------------
// NULL -> the defaults; RG_ERR_INVALID_ARG for an option that is 0
int rg_stats_options(const rg_pcm_stats_opts *opts, rg_pcm_stats_opts *out, char *err, size_t err_len);
// The planes of track i, described by `t` with `bits`, in an arena of `arena_bytes` bytes: planes[0 .. t.channels).
// RG_ERR_FORMAT unless it is 1 .. 8 channels of one of the three formats and fewer than 2^32 frames, RG_ERR_INVALID_ARG unless
// the planes lie inside the arena, sample-aligned, and 1 <= bits <= W; the text goes to err[err_len].  *bits_out: what the
// record reports (0 for float).  first_tile, n_tiles and run are rg_stats_plan's to set.
int rg_stats_track_planes(size_t i, const rg_track_desc &t, uint32_t bits, size_t arena_bytes, RgStatsPlane *planes, uint32_t *bits_out, char *err,
                          size_t err_len);
// tiles and runs of the `n` planes of a launch, the tiles of each format contiguous: fmt_tile[f] .. fmt_tile[f + 1] are
// format f's; returns the number of tiles
uint64_t rg_stats_plan(RgStatsPlane *planes, size_t n, uint64_t fmt_tile[4]);
// one plane's numbers from host memory: the definitions, serially ...
rg_pcm_stats_channel rg_stats_serial_host(const unsigned char *arena, const RgStatsPlane &p, const rg_pcm_stats_opts &o);
// ... and as the kernels compute them: chunks, trees, tile records, runs (`p` has been through rg_stats_plan)
rg_pcm_stats_channel rg_stats_folded_host(const unsigned char *arena, const RgStatsPlane &p, const rg_pcm_stats_opts &o, bool any_test);
// the result record of a track that was scanned: ch[0 .. t.channels) are its planes'
void rg_stats_fill(const rg_track_desc &t, uint32_t bits_reported, uint32_t dropped_frames, const rg_pcm_stats_channel *ch, rg_pcm_stats_result *out);
// routes 0 and 2 of rg_pcm_stats_arena
int rg_stats_arena_host(int route, size_t n, const rg_track_desc *descs, const uint32_t *bits, const rg_pcm_stats_opts *opts, const void *arena,
                        size_t arena_bytes, rg_pcm_stats_result *out, char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` planes in the device arena at `d_arena` (allocated in whole 16-byte words): the two kernels on `s`, ch[i] <- plane i;
// `s` has been synchronised on return
int rg_stats_device(rg_ctx *c, const unsigned char *d_arena, RgStatsPlane *planes, size_t n, const rg_pcm_stats_opts &o, rg_pcm_stats_channel *ch,
                    hipStream_t s);
// For the rate hooks of other scans (rg_dr_rate), which time the stats pair over their own arena: the bookkeeping of a launch
// over `n` planes in an allocation of its own (uploaded on `s`), then the launches alone, then the release.
struct RgStatsBench {
    unsigned char *d;
    size_t n, map, tiles, res;
    uint64_t fmt_tile[4];
};
int rg_stats_bench_setup(rg_ctx *c, RgStatsPlane *planes, size_t n, hipStream_t s, RgStatsBench *b);
int rg_stats_bench_launch(rg_ctx *c, const unsigned char *d_arena, const RgStatsBench &b, hipStream_t s);
void rg_stats_bench_free(RgStatsBench *b);
#endif
