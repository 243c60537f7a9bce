// rg_stereo.h -- internal: the stereo image scan (include/mp3rgain_amd_stereo.h) as rg_stereo.hip (kernels, launcher, seam),
// rg_stereo_host.cpp (the serial host twin, the kernels' cutting and fold arithmetic on the host, the finish) and
// rg_file_verify.hip (rg_stereo) share it.  What a frame adds to the sums, how two sums combine, what a block adds to a track,
// which of two lags is the better and how a tile of the lag kernel is laid out is host and device code, written once here; the
// kernels and the folded host route differ only in who walks the lanes.
//
// Everything in front of the finish is a sum of integers, a count or a choice under a total order: all commute and are exact in
// any order, so a block may be cut anywhere, a track tiled anywhere and the partial sums added in any order.  |q| <= 2^15, so a
// product is at most 2^30 in magnitude and a sum over fewer than 2^32 frames below 2^62: one int64 each.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_stereo.h"
#include "rg_pcm_plane.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_ST_HD __host__ __device__ inline
#else
#define RG_ST_HD inline
#endif

// ---- how a track is cut -----------------------------------------------------------------------------------------------------
#define RG_ST_LANES 256u                                        // lanes of every workgroup here
#define RG_ST_STEPS 4u                                          // 16-byte vectors one lane takes from each plane of a whole piece
#define RG_ST_PIECE_BYTES (16u * RG_ST_LANES * RG_ST_STEPS)     // 16 KiB of each plane
#define RG_ST_TILE 4096u                                        // frames of a tile of the lag kernel
#define RG_ST_STRIP 16u                                         // consecutive frames a lane holds the left values of
#define RG_ST_LAG_GROUP 16u                                     // consecutive lags a lane accumulates
#define RG_ST_MAX_GROUPS ((2u * RG_ST_MAX_RADIUS + 1u + RG_ST_LAG_GROUP - 1u) / RG_ST_LAG_GROUP)  // 32
// the right plane of a tile in LDS: frame m of the tile (m from -R) at position m + R, so a lane's window of lag group g over
// strip c begins at 16 (c + g), aligned; the last group may reach RG_ST_LAG_GROUP - 1 lags past +R
#define RG_ST_RIGHT_LDS (RG_ST_TILE + RG_ST_LAG_GROUP * RG_ST_MAX_GROUPS)
#define RG_ST_MAX_LAGS (2u * RG_ST_MAX_RADIUS + 1u)
#define RG_ST_LDS_BYTES (2u * RG_ST_TILE + 2u * RG_ST_RIGHT_LDS + 8u * (RG_ST_LAG_GROUP * RG_ST_MAX_GROUPS))

struct RgStPiece {          // the sums of a piece, of a block, of anything in between
    uint64_t ll, rr;        // the sums of q_L^2 and q_R^2
    int64_t lr;             // the sum of q_L q_R
    uint32_t equal, opposite, zero;  // raw comparisons (a block has at most 384 000 frames)
    uint32_t nonfinite;     // samples, both channels
};  // 40 bytes
struct RgStTrack {          // one track of a launch
    uint64_t off_l, off_r;  // of channels 0 and 1 from the arena's base, in bytes (sample-aligned)
    uint64_t first_piece;   // of this track among the launch's pieces (the pieces of one format are contiguous)
    uint64_t first_tile;    // of this track among the launch's tiles
    uint32_t n;             // N < 2^32; 0 for a track of one channel, which is not measured
    uint32_t block;         // B
    uint32_t n_blocks;      // ceil(N / B)
    uint32_t pieces_per_block;  // of a whole block; only the last block may have fewer
    uint32_t format;        // rg_sample_format
    uint32_t n_tiles;       // ceil(N / RG_ST_TILE)
};  // 56 bytes
struct RgStTotals {         // the raw numbers of a track: the same bits on every route
    uint64_t ell, err;
    int64_t elr;
    uint64_t equal, opposite, zero, nonfinite;
    int64_t lag_sum, anti_sum;
    uint32_t blocks, active, neg, mono;
    int32_t lag, anti_lag;
};  // 96 bytes

// ---- samples ---------------------------------------------------------------------------------------------------------------
RG_ST_HD uint32_t rg_st_piece_samples(uint32_t format) { return RG_ST_PIECE_BYTES / rg_pcm_bps(format); }
RG_ST_HD uint32_t rg_st_groups(uint32_t radius) { return (2u * radius + 1u + RG_ST_LAG_GROUP - 1u) / RG_ST_LAG_GROUP; }

RG_ST_HD RgStPiece rg_st_empty() { return RgStPiece{0u, 0u, 0, 0u, 0u, 0u, 0u}; }

// q of a sample.  `raw`: the stored pattern, an S16 sample sign-extended to 32 bits.  clamp(x) * 2^15 is exact in float (a power
// of two; what is subnormal or becomes so rounds to 0 either way), so rintf gives the integer of the definition.
template <int FMT>
RG_ST_HD int32_t rg_st_q(uint32_t raw, bool *finite) {
    *finite = true;
    if (FMT == RG_FMT_F32_PLANAR) {
        if ((raw & 0x7F800000u) == 0x7F800000u) {
            *finite = false;
            return 0;
        }
        float x;
        memcpy(&x, &raw, 4);
        const int32_t q = (int32_t)rintf(fminf(fmaxf(x, -1.0f), 1.0f) * 32768.0f);
        return q > 32767 ? 32767 : q;
    }
    if (FMT == RG_FMT_S32_PLANAR) return (int32_t)raw >> 16;
    return (int32_t)raw;
}
// one frame into the sums
template <int FMT>
RG_ST_HD void rg_st_take(uint32_t raw_l, uint32_t raw_r, RgStPiece *p) {
    bool fin_l, fin_r;
    const int32_t ql = rg_st_q<FMT>(raw_l, &fin_l), qr = rg_st_q<FMT>(raw_r, &fin_r);
    p->ll += (uint64_t)(uint32_t)(ql * ql);  // <= 2^30
    p->rr += (uint64_t)(uint32_t)(qr * qr);
    p->lr += (int64_t)(ql * qr);
    if (FMT == RG_FMT_F32_PLANAR) {
        float xl, xr;
        memcpy(&xl, &raw_l, 4);
        memcpy(&xr, &raw_r, 4);
        p->equal += xl == xr ? 1u : 0u;
        p->opposite += (xl == -xr && xl != 0.0f) ? 1u : 0u;
        p->zero += (xl == 0.0f && xr == 0.0f) ? 1u : 0u;
        p->nonfinite += (fin_l ? 0u : 1u) + (fin_r ? 0u : 1u);
    } else {
        const int32_t vl = (int32_t)raw_l, vr = (int32_t)raw_r;
        p->equal += vl == vr ? 1u : 0u;
        p->opposite += ((int64_t)vl + (int64_t)vr == 0 && vl != 0) ? 1u : 0u;
        p->zero += (vl == 0 && vr == 0) ? 1u : 0u;
    }
}
// a <- a + b
RG_ST_HD void rg_st_combine(RgStPiece *a, const RgStPiece &b) {
    a->ll += b.ll;
    a->rr += b.rr;
    a->lr += b.lr;
    a->equal += b.equal;
    a->opposite += b.opposite;
    a->zero += b.zero;
    a->nonfinite += b.nonfinite;
}
// a block of `len` frames, from its sums, into the track's totals
RG_ST_HD void rg_st_block_into(RgStTotals *t, const RgStPiece &b, uint32_t len) {
    t->ell += b.ll;
    t->err += b.rr;
    t->elr += b.lr;
    t->equal += b.equal;
    t->opposite += b.opposite;
    t->zero += b.zero;
    t->nonfinite += b.nonfinite;
    t->blocks += 1u;
    const bool active = b.ll + b.rr > 0;
    t->active += active ? 1u : 0u;
    t->neg += b.lr < 0 ? 1u : 0u;
    t->mono += (active && b.equal == len) ? 1u : 0u;
}

// ---- lags ------------------------------------------------------------------------------------------------------------------
// the total order of the best lag: the larger sum, then the smaller |d|, then the negative d.  true when (ca, da) comes first
RG_ST_HD bool rg_st_better(int64_t ca, int32_t da, int64_t cb, int32_t db) {
    if (ca != cb) return ca > cb;
    const int32_t aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
    if (aa != ab) return aa < ab;
    return da < db;
}
// ... and of the anti-phase lag: the smaller sum, then the same
RG_ST_HD bool rg_st_lower(int64_t ca, int32_t da, int64_t cb, int32_t db) { return rg_st_better(-ca, da, -cb, db); }  // |C| < 2^62

// ---- cutting ---------------------------------------------------------------------------------------------------------------
// block `b` of a track: [*start, *start + return)
RG_ST_HD uint32_t rg_st_block_window(const RgStTrack &t, uint32_t b, uint64_t *start) {
    *start = (uint64_t)b * t.block;
    const uint64_t left = t.n - *start;
    return left < t.block ? (uint32_t)left : t.block;
}
// pieces of a block of `len` frames
RG_ST_HD uint32_t rg_st_pieces_of(uint32_t len, uint32_t format) {
    const uint32_t P = rg_st_piece_samples(format);
    return (len + P - 1) / P;
}
// piece `k` of a block of `len` frames: [*start, *start + return) of the block
RG_ST_HD uint32_t rg_st_piece_window(uint32_t len, uint32_t k, uint32_t format, uint32_t *start) {
    const uint32_t P = rg_st_piece_samples(format);
    *start = k * P;
    return len - *start < P ? len - *start : P;
}
// all the pieces of a track
RG_ST_HD uint64_t rg_st_track_pieces(const RgStTrack &t) {
    if (!t.n_blocks) return 0;
    uint64_t start;
    const uint32_t tail = rg_st_block_window(t, t.n_blocks - 1, &start);
    return (uint64_t)(t.n_blocks - 1) * t.pieces_per_block + rg_st_pieces_of(tail, t.format);
}
// tile `k` of a track: [*start, *start + return)
RG_ST_HD uint32_t rg_st_tile_window(const RgStTrack &t, uint32_t k, uint64_t *start) {
    *start = (uint64_t)k * RG_ST_TILE;
    const uint64_t left = t.n - *start;
    return left < RG_ST_TILE ? (uint32_t)left : RG_ST_TILE;
}
// How the lanes of a tile's workgroup share it: `groups` lag groups, lanes_per_group = RG_ST_LANES / groups lanes each (lane l has
// group l % groups and is the l / groups-th of them; the lanes left over idle), and the strips of the tile dealt to a group's
// lanes in runs of *strips_per_lane.  Lane `l` takes strips [*first, return) of the `strips` there are.
RG_ST_HD uint32_t rg_st_lane_strips(uint32_t l, uint32_t groups, uint32_t strips, uint32_t *first) {
    const uint32_t per_group = RG_ST_LANES / groups, r = l / groups;
    const uint32_t per_lane = (strips + per_group - 1) / per_group;
    *first = r * per_lane;
    if (r >= per_group || *first >= strips) {
        *first = 0;
        return 0;
    }
    return *first + per_lane < strips ? *first + per_lane : strips;
}

// ---- rg_stereo_host.cpp (plain C++: no device, no context) -----------------------------------------------------------------
// NULL -> the defaults; RG_ERR_INVALID_ARG for a radius, a block length or a threshold outside its range
int rg_st_options(const rg_stereo_opts *opts, rg_stereo_opts *out, char *err, size_t err_len);
// Track i, described by `t`, in an arena of `arena_bytes` bytes.  RG_ERR_FORMAT unless it is 1 .. 8 channels of one of the three
// formats and fewer than 2^32 frames, and -- when the block length comes from the sample rate -- 1 <= sample_rate <=
// RG_ST_MAX_BLOCK_FRAMES where `rate_is_format` (the file route: such a stream fails alone), RG_ERR_INVALID_ARG otherwise;
// RG_ERR_INVALID_ARG unless the planes lie inside the arena, sample-aligned.  The text goes to err[err_len].  first_piece and
// first_tile are rg_st_plan's to set.
int rg_st_track(size_t i, const rg_track_desc &t, const rg_stereo_opts &o, bool rate_is_format, size_t arena_bytes, RgStTrack *out, char *err,
                size_t err_len);
// pieces and tiles of the `n` tracks of a launch, the pieces of each format contiguous: fmt_piece[f] .. fmt_piece[f + 1] are
// format f's; returns the number of pieces, *n_tiles: of tiles
uint64_t rg_st_plan(RgStTrack *tracks, size_t n, uint64_t fmt_piece[4], uint64_t *n_tiles);
// one track's raw numbers and its 2 * radius + 1 lag sums from host memory: the definitions, serially ...
RgStTotals rg_st_serial_host(const unsigned char *arena, const RgStTrack &t, uint32_t radius, int64_t *sums);
// ... and as the kernels compute them: pieces, blocks, tiles of strips and lag groups in double, the choice by a tree
RgStTotals rg_st_folded_host(const unsigned char *arena, const RgStTrack &t, uint32_t radius, int64_t *sums);
// the finish: the result record of a track that was scanned, block = B
void rg_st_fill(const rg_track_desc &t, const rg_stereo_opts &o, uint32_t block, uint32_t dropped_frames, const RgStTotals &tot, rg_stereo_result *out);
// routes 0 and 2 of rg_stereo_arena
int rg_st_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_stereo_opts *opts, const void *arena, size_t arena_bytes,
                     rg_stereo_result *out, int64_t *lag_sums, char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` tracks in the device arena at `d_arena` (allocated in whole 16-byte words): the kernels on `s`, tot[i] <- track i, and when
// `sums` is not NULL its rows i <- the 2 * radius + 1 lag sums of track i; `s` has been synchronised on return
int rg_st_device(rg_ctx *c, const unsigned char *d_arena, RgStTrack *tracks, size_t n, uint32_t radius, RgStTotals *tot, int64_t *sums, hipStream_t s);
#endif
