// rg_compare.h -- internal: the null test of two tracks (include/mp3rgain_amd_compare.h) as rg_compare.hip (kernels, launcher,
// seam) and rg_compare_host.cpp (the serial host twin, the kernels' cutting and fold arithmetic on the host, the pick and the
// finish) share it.  What a sample pair adds to the sums, how two sums combine, where a segment, a tile, a block and a piece lie
// is host and device code, written once here; the kernels and the folded host route differ only in who walks the lanes.  The
// reduced sample q, the lanes' share of a tile's strips and the piece length are the stereo scan's (rg_stereo.h), not copies.
//
// Everything in front of the pick and the finish is a sum of integers, a count, a maximum or a minimum: all commute and are exact
// in any order.  |q| <= 2^15, a product at most 2^30, and a pair has fewer than 2^32 samples in its overlap (rg_cmp_plan_pair
// refuses more): every sum stays below 2^62 in magnitude, one int64 each.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_compare.h"
#include "rg_pcm_plane.h"
#include "rg_stereo.h"

#define RG_CMP_HD RG_ST_HD

// ---- how a pair is cut -------------------------------------------------------------------------------------------------------
#define RG_CMP_LANES RG_ST_LANES        // lanes of every workgroup here
#define RG_CMP_TILE RG_ST_TILE          // reference frames of a tile of the lag kernel
#define RG_CMP_STRIP RG_ST_STRIP        // consecutive reference frames a lane holds in registers
#define RG_CMP_LAG_GROUP RG_ST_LAG_GROUP  // consecutive lags a lane accumulates
#define RG_CMP_MAX_GROUPS ((2u * RG_CMP_MAX_RADIUS + 1u + RG_CMP_LAG_GROUP - 1u) / RG_CMP_LAG_GROUP)  // 256: one per lane
// the b side of a tile in LDS: frame m of the tile (m from -R) at position m + R, so a lane's window of lag group g over strip c
// begins at 16 (c + g), aligned; the last group may reach RG_CMP_LAG_GROUP - 1 lags past +R
#define RG_CMP_B_LDS (RG_CMP_TILE + RG_CMP_LAG_GROUP * RG_CMP_MAX_GROUPS)
#define RG_CMP_LDS_SUMS (RG_CMP_LAG_GROUP * RG_CMP_MAX_GROUPS + 2u)  // the lags of every group, EA, EB
#define RG_CMP_LDS_BYTES (2u * RG_CMP_TILE + 2u * RG_CMP_B_LDS + 8u * RG_CMP_LDS_SUMS)
#define RG_CMP_MIXED_PIECE 4096u        // frames of a piece of a pair of different formats
#define RG_CMP_NONE (~(uint64_t)0)      // first_diff: no sample differs

struct RgCmpPair {           // one pair of a launch
    uint64_t off_a, off_b;   // of channel 0 of each track from the arena's base, in bytes (sample-aligned)
    uint64_t first_tile;     // of this pair among the launch's tiles
    uint64_t first_row;      // ... lag rows (row s * cc + c)
    uint64_t first_piece;    // ... pieces (the pieces of one kernel are contiguous)
    uint64_t first_block;    // ... blocks
    int64_t h;               // the hint
    int64_t lag;             // h + d*, once picked
    uint32_t na, nb;         // frames of the two tracks
    uint32_t fmt_a, fmt_b;   // rg_sample_format
    uint32_t cc;             // Cc; 0 for a pair that is not measured
    uint32_t n0, v;          // the overlap at the hint: [n0, n0 + v)
    uint32_t n_seg, seg_len; // S segments of seg_len frames each (one of v frames when the overlap is one segment)
    int32_t sigma;           // the polarity, once picked
    uint32_t m0, w;          // the overlap at the lag: [m0, m0 + w), once picked
    uint32_t block;          // B
    uint32_t n_blocks;       // ceil(w / B)
    uint32_t pieces_per_block;  // of a whole block; only the last block may have fewer
    uint32_t flags;          // RG_CMP_RATE, RG_CMP_NO_OVERLAP, RG_CMP_CHANNELS_DIFFER as planned
    uint32_t pad;
};  // 128 bytes
struct RgCmpPiece {          // the sums of one channel of a piece, of a block, of anything in between
    uint64_t aa, bb;         // the sums of qa^2 and qb^2
    int64_t ab;              // the sum of qa qb
    uint64_t first_diff;     // frame index in a, RG_CMP_NONE
    uint32_t equal;          // samples (a block has at most 384 000 frames of 8 channels)
    uint32_t max_diff;
    uint32_t nonfinite;      // samples, both sides
    uint32_t pad;
};  // 48 bytes
struct RgCmpTotals {         // the raw numbers of a pair's stage C: the same bits on every route
    uint64_t aa, bb;
    int64_t ab;
    uint64_t equal, first_diff, nonfinite;
    uint32_t blocks, differing, max_diff, pad;
};  // 64 bytes
struct RgCmpPicked {         // what the pick makes of a pair's lag rows
    int32_t d, sigma;
    uint32_t flags;          // RG_CMP_LOCKED, RG_CMP_AT_EDGE, RG_CMP_DRIFT
    uint32_t locked_segments;
    int64_t seg_lag_min, seg_lag_max;
    double lock;
};

RG_CMP_HD uint32_t rg_cmp_groups(uint32_t radius) { return rg_st_groups(radius); }
RG_CMP_HD uint32_t rg_cmp_row_len(uint32_t radius) { return 2u * radius + 3u; }
RG_CMP_HD RgCmpPiece rg_cmp_empty() { return RgCmpPiece{0u, 0u, 0, RG_CMP_NONE, 0u, 0u, 0u, 0u}; }
// which moments kernel takes a pair: its format when both tracks have it, 3 = the frame-by-frame kernel for two formats
RG_CMP_HD uint32_t rg_cmp_kind(uint32_t fmt_a, uint32_t fmt_b) { return fmt_a == fmt_b ? fmt_a : 3u; }
RG_CMP_HD uint32_t rg_cmp_piece_frames(uint32_t fmt_a, uint32_t fmt_b) { return fmt_a == fmt_b ? rg_st_piece_samples(fmt_a) : RG_CMP_MIXED_PIECE; }

// ---- samples -----------------------------------------------------------------------------------------------------------------
// one sample pair into the sums: its q, whether it is equal, its non-finite samples; `at`: the frame index in a
RG_CMP_HD void rg_cmp_add(int32_t qa, int32_t qb, bool eq, uint32_t nonfinite, int32_t sigma, uint64_t at, RgCmpPiece *p) {
    p->aa += (uint64_t)(uint32_t)(qa * qa);  // <= 2^30
    p->bb += (uint64_t)(uint32_t)(qb * qb);
    p->ab += (int64_t)(qa * qb);
    const int32_t diff = qa - sigma * qb;
    const uint32_t mag = (uint32_t)(diff < 0 ? -diff : diff);
    p->equal += eq ? 1u : 0u;
    p->max_diff = mag > p->max_diff ? mag : p->max_diff;
    if (!eq && at < p->first_diff) p->first_diff = at;
    p->nonfinite += nonfinite;
}
// ... of two tracks of format FMT.  raw: the stored patterns, an S16 sample sign-extended
template <int FMT>
RG_CMP_HD void rg_cmp_take(uint32_t raw_a, uint32_t raw_b, int32_t sigma, uint64_t at, RgCmpPiece *p) {
    bool fin_a, fin_b;
    const int32_t qa = rg_st_q<FMT>(raw_a, &fin_a), qb = rg_st_q<FMT>(raw_b, &fin_b);
    bool eq = qa == -qb;
    if (sigma > 0) {
        if (FMT == RG_FMT_F32_PLANAR) {
            float xa, xb;
            memcpy(&xa, &raw_a, 4);
            memcpy(&xb, &raw_b, 4);
            eq = xa == xb;
        } else {
            eq = raw_a == raw_b;
        }
    }
    rg_cmp_add(qa, qb, eq, (fin_a ? 0u : 1u) + (fin_b ? 0u : 1u), sigma, at, p);
}
// q of a sample of a format that is not known at compile time
RG_CMP_HD int32_t rg_cmp_q(uint32_t format, uint32_t raw, bool *finite) {
    return format == RG_FMT_F32_PLANAR ? rg_st_q<RG_FMT_F32_PLANAR>(raw, finite)
           : format == RG_FMT_S16_PLANAR ? rg_st_q<RG_FMT_S16_PLANAR>(raw, finite) : rg_st_q<RG_FMT_S32_PLANAR>(raw, finite);
}
// ... of two tracks of different formats: q against q
RG_CMP_HD void rg_cmp_take_mixed(uint32_t fmt_a, uint32_t raw_a, uint32_t fmt_b, uint32_t raw_b, int32_t sigma, uint64_t at, RgCmpPiece *p) {
    bool fin_a, fin_b;
    const int32_t qa = rg_cmp_q(fmt_a, raw_a, &fin_a), qb = rg_cmp_q(fmt_b, raw_b, &fin_b);
    rg_cmp_add(qa, qb, qa == sigma * qb, (fin_a ? 0u : 1u) + (fin_b ? 0u : 1u), sigma, at, p);
}
// a <- a + b
RG_CMP_HD void rg_cmp_combine(RgCmpPiece *a, const RgCmpPiece &b) {
    a->aa += b.aa;
    a->bb += b.bb;
    a->ab += b.ab;
    a->first_diff = b.first_diff < a->first_diff ? b.first_diff : a->first_diff;
    a->equal += b.equal;
    a->max_diff = b.max_diff > a->max_diff ? b.max_diff : a->max_diff;
    a->nonfinite += b.nonfinite;
}
// a block of `len` frames of `cc` channels, from its sums over the channels: the caller's row, and into the pair's totals
RG_CMP_HD rg_compare_block rg_cmp_block_row(const RgCmpPiece &b, uint32_t len) {
    return rg_compare_block{(int64_t)b.aa, (int64_t)b.bb, b.ab, b.first_diff, b.equal, b.max_diff, len, 0u};
}
RG_CMP_HD void rg_cmp_block_into(RgCmpTotals *t, const RgCmpPiece &b, uint32_t len, uint32_t cc) {
    t->aa += b.aa;
    t->bb += b.bb;
    t->ab += b.ab;
    t->equal += b.equal;
    t->first_diff = b.first_diff < t->first_diff ? b.first_diff : t->first_diff;
    t->nonfinite += b.nonfinite;
    t->blocks += 1u;
    t->differing += b.equal < len * cc ? 1u : 0u;
    t->max_diff = b.max_diff > t->max_diff ? b.max_diff : t->max_diff;
}

// ---- cutting -----------------------------------------------------------------------------------------------------------------
// where segment `s` of a pair starts in a (it has p.seg_len frames)
RG_CMP_HD uint64_t rg_cmp_seg_start(const RgCmpPair &p, uint32_t s) {
    return (uint64_t)p.n0 + (uint64_t)(2u * s + 1u) * (uint64_t)(p.v - p.seg_len) / (2u * p.n_seg);
}
RG_CMP_HD uint32_t rg_cmp_seg_tiles(const RgCmpPair &p) { return (p.seg_len + RG_CMP_TILE - 1u) / RG_CMP_TILE; }
RG_CMP_HD uint64_t rg_cmp_pair_tiles(const RgCmpPair &p) { return (uint64_t)p.n_seg * p.cc * rg_cmp_seg_tiles(p); }
RG_CMP_HD uint64_t rg_cmp_pair_rows(const RgCmpPair &p) { return (uint64_t)p.n_seg * p.cc; }
// tile `rel` of a pair: its segment and channel, and [*start, *start + return) in a
RG_CMP_HD uint32_t rg_cmp_tile_window(const RgCmpPair &p, uint64_t rel, uint32_t *s, uint32_t *c, uint64_t *start) {
    const uint32_t per = rg_cmp_seg_tiles(p), k = (uint32_t)(rel % per);
    const uint64_t sc = rel / per;
    *c = (uint32_t)(sc % p.cc);
    *s = (uint32_t)(sc / p.cc);
    const uint32_t at = k * RG_CMP_TILE, left = p.seg_len - at;
    *start = rg_cmp_seg_start(p, *s) + at;
    return left < RG_CMP_TILE ? left : RG_CMP_TILE;
}
// block `b` of a pair's stage C: [*start, *start + return) of the overlap
RG_CMP_HD uint32_t rg_cmp_block_window(const RgCmpPair &p, uint32_t b, uint32_t *start) {
    *start = b * p.block;  // < w < 2^32
    const uint32_t left = p.w - *start;
    return left < p.block ? left : p.block;
}
RG_CMP_HD uint32_t rg_cmp_pieces_of(uint32_t len, uint32_t piece) { return (len + piece - 1u) / piece; }
// the pieces of one channel of a pair, and of the pair
RG_CMP_HD uint64_t rg_cmp_channel_pieces(const RgCmpPair &p) {
    if (!p.n_blocks) return 0;
    uint32_t start;
    const uint32_t tail = rg_cmp_block_window(p, p.n_blocks - 1u, &start);
    return (uint64_t)(p.n_blocks - 1u) * p.pieces_per_block + rg_cmp_pieces_of(tail, rg_cmp_piece_frames(p.fmt_a, p.fmt_b));
}
RG_CMP_HD uint64_t rg_cmp_pair_pieces(const RgCmpPair &p) { return rg_cmp_channel_pieces(p) * p.cc; }
// piece `rel` of a pair: its channel and block, and [*start, *start + return) of the overlap
RG_CMP_HD uint32_t rg_cmp_piece_window(const RgCmpPair &p, uint64_t rel, uint32_t *c, uint32_t *b, uint32_t *start) {
    const uint64_t per = rg_cmp_channel_pieces(p), r = rel % per;
    *c = (uint32_t)(rel / per);
    *b = (uint32_t)(r / p.pieces_per_block);
    const uint32_t k = (uint32_t)(r % p.pieces_per_block), P = rg_cmp_piece_frames(p.fmt_a, p.fmt_b);
    uint32_t bstart;
    const uint32_t len = rg_cmp_block_window(p, *b, &bstart);
    *start = bstart + k * P;
    return len - k * P < P ? len - k * P : P;
}
// How the lanes of a tile's workgroup share it: `groups` lag groups of RG_CMP_LANES / groups lanes each, and the lanes left over
// (127 of them at the default radius, 129 groups) go one each to the first groups, so no lane idles while a group has more than
// one strip to give.  Lane `l` has group *g and takes strips [*first, return) of the `strips` there are, dealt in equal runs to
// its group's lanes.
RG_CMP_HD uint32_t rg_cmp_lane_strips(uint32_t l, uint32_t groups, uint32_t strips, uint32_t *g, uint32_t *first) {
    const uint32_t per_group = RG_CMP_LANES / groups, even = per_group * groups, extra = RG_CMP_LANES - even;
    const uint32_t r = l < even ? l / groups : per_group;
    *g = l < even ? l % groups : l - even;
    const uint32_t cnt = per_group + (*g < extra ? 1u : 0u), per_lane = (strips + cnt - 1u) / cnt;
    *first = r * per_lane;
    if (*first >= strips) {
        *first = 0;
        return 0;
    }
    return *first + per_lane < strips ? *first + per_lane : strips;
}
// where channel c of each track starts, from the arena's base
RG_CMP_HD uint64_t rg_cmp_plane_a(const RgCmpPair &p, uint32_t c) { return p.off_a + (uint64_t)c * p.na * rg_pcm_bps(p.fmt_a); }
RG_CMP_HD uint64_t rg_cmp_plane_b(const RgCmpPair &p, uint32_t c) { return p.off_b + (uint64_t)c * p.nb * rg_pcm_bps(p.fmt_b); }

// ---- rg_compare_host.cpp (plain C++: no device, no context) ---------------------------------------------------------------------
// NULL -> the defaults; RG_ERR_INVALID_ARG for an option outside its range
int rg_cmp_options(const rg_compare_opts *opts, rg_compare_opts *out, char *err, size_t err_len);
// Pair i = (a, b, h) of the `n` tracks `descs` describe in an arena of `arena_bytes` bytes: the checks of the header, and stage
// B's geometry.  A pair that is not measured (another rate, no overlap) has cc == 0 and its flag.  first_* are rg_cmp_plan's.
int rg_cmp_plan_pair(size_t i, const rg_track_desc *descs, size_t n, const rg_compare_pair &pair, const rg_compare_opts &o, bool rate_is_format,
                     size_t arena_bytes, RgCmpPair *out, char *err, size_t err_len);
// tiles and rows of the `n` pairs of a launch; returns the number of tiles, *n_rows: of rows
uint64_t rg_cmp_plan_lags(RgCmpPair *pairs, size_t n, uint64_t *n_rows);
// the pick: from the rows of a pair (rg_cmp_pair_rows of rg_cmp_row_len each)
RgCmpPicked rg_cmp_pick(const RgCmpPair &p, const rg_compare_opts &o, const int64_t *rows);
// stage C's geometry from the pick: lag, sigma, m0, w, blocks
void rg_cmp_set_lag(RgCmpPair *p, const RgCmpPicked &k);
// pieces and blocks of the `n` pairs, the pieces of each kernel contiguous: kind_piece[k] .. kind_piece[k + 1] are kernel k's
// (rg_cmp_kind); returns the number of pieces, *n_blocks: of blocks
uint64_t rg_cmp_plan_moments(RgCmpPair *pairs, size_t n, uint64_t kind_piece[5], uint64_t *n_blocks);
// one pair's lag rows from host memory: the definitions, serially, and as the kernel computes them
void rg_cmp_lags_serial(const unsigned char *arena, const RgCmpPair &p, uint32_t radius, int64_t *rows);
void rg_cmp_lags_folded(const unsigned char *arena, const RgCmpPair &p, uint32_t radius, int64_t *rows);
// one pair's stage C: blocks[p.n_blocks] and the totals, likewise
RgCmpTotals rg_cmp_moments_serial(const unsigned char *arena, const RgCmpPair &p, rg_compare_block *blocks);
RgCmpTotals rg_cmp_moments_folded(const unsigned char *arena, const RgCmpPair &p, rg_compare_block *blocks);
// the record of a pair that was not measured (p.cc == 0), and the finish of one that was
void rg_cmp_fill_skipped(const rg_track_desc *descs, const rg_compare_pair &pair, const rg_compare_opts &o, const RgCmpPair &p, uint32_t dropped_a,
                         uint32_t dropped_b, rg_compare_result *out);
void rg_cmp_fill(const rg_track_desc *descs, const rg_compare_pair &pair, const rg_compare_opts &o, const RgCmpPair &p, const RgCmpPicked &k,
                 const RgCmpTotals &tot, const rg_compare_block *blocks, uint32_t dropped_a, uint32_t dropped_b, uint32_t more_flags,
                 rg_compare_result *out);
// a pair's rows into the caller's slab (segments * RG_CMP_MAX_CHANNELS rows), and its blocks into the caller's rows
void rg_cmp_rows_out(const RgCmpPair &p, const rg_compare_opts &o, const int64_t *rows, int64_t *slab);
void rg_cmp_blocks_out(const RgCmpPair &p, const rg_compare_block *blocks, rg_compare_block *out, size_t blocks_per_pair);
// routes 0 and 2 of rg_compare_arena
int rg_cmp_arena_host(int route, size_t n, const rg_track_desc *descs, size_t n_pairs, const rg_compare_pair *pairs, const rg_compare_opts *opts,
                      const void *arena, size_t arena_bytes, rg_compare_result *out, rg_compare_block *blocks_out, size_t blocks_per_pair,
                      int64_t *lag_sums, char *err, size_t err_len);

#if defined(__HIPCC__)
#include <vector>
struct rg_ctx;
// `n` planned pairs in the device arena at `d_arena` (allocated in whole 16-byte words) on `s`: the lag kernel, rows <- every
// pair's lag rows (rg_cmp_plan_lags' order), picked[i] <- the host's pick of pair i, which sets pairs[i]'s stage C; then the
// moments kernels and the fold: tot[i] and blocks (rg_cmp_plan_moments' order) <- pair i's.  `s` has been synchronised on return.
int rg_cmp_device(rg_ctx *c, const unsigned char *d_arena, RgCmpPair *pairs, size_t n, const rg_compare_opts &o, std::vector<int64_t> *rows,
                  RgCmpPicked *picked, RgCmpTotals *tot, std::vector<rg_compare_block> *blocks, hipStream_t s);
#endif
