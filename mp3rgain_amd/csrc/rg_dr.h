// rg_dr.h -- internal: the dynamic range scan (include/mp3rgain_amd_dr.h) as rg_dr.hip (kernels, launcher, seams),
// rg_dr_host.cpp (the serial host twin, the kernels' cutting and fold arithmetic on the host, the finish) and
// rg_file_verify.hip (rg_dynamic_range) share it.  What a sample adds to a sum, how two sums combine, what a block's sums
// come to in double, how the k-th largest is found digit by digit and how a plane is finished is host and device code,
// written once here; the kernels and the folded host route differ only in who walks the lanes.
//
// A block's energy is a sum of integers and its peak a maximum: both commute and are exact in any order, so a block may be
// cut anywhere and its pieces folded in any fixed tree.  The energy reaches 2^82, so it is kept as two 64-bit sums, of the
// low and of the high 32 bits of every square: a block has at most 1 152 000 < 2^21 samples, so neither limb overflows
// (< 2^53), and a piece record can be added to another limb by limb without a carry between them.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_dr.h"
#include "rg_pcm_plane.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_DR_HD __host__ __device__ inline
#else
#define RG_DR_HD inline
#endif

// ---- how a block is cut ---------------------------------------------------------------------------------------------------
#define RG_DR_LANES 256u                                        // lanes of a piece's workgroup
#define RG_DR_STEPS 8u                                          // 16-byte vectors one lane takes from a whole piece
#define RG_DR_PIECE_BYTES (16u * RG_DR_LANES * RG_DR_STEPS)     // 32 KiB of samples
#define RG_DR_FOLD_LANES 256u                                   // lanes of the fold kernel (one workgroup per plane)
#define RG_DR_RADIX_BITS 8u                                     // the selection takes the doubles' patterns 8 bits a pass
#define RG_DR_BINS (1u << RG_DR_RADIX_BITS)
#define RG_DR_PASSES (64u / RG_DR_RADIX_BITS)

struct RgDrPiece {          // the sums of a piece, of a block, of anything in between
    uint64_t hi, lo;        // the sums of q^2 >> 32 and of q^2 & 0xFFFFFFFF
    uint32_t peak;          // max |q|
    uint32_t nonfinite;
};  // 24 bytes
struct RgDrBlock {          // one block of a plane, as the fold leaves it for the selection and the walk
    double ms, e;
    uint32_t peak;
    uint32_t reserved;
};  // 24 bytes
struct RgDrPlane {          // one plane of a launch
    uint64_t off;           // from the arena's base, in bytes (sample-aligned)
    uint64_t first_piece;   // of this plane among the launch's pieces (the pieces of one format are contiguous)
    uint64_t first_block;   // of this plane among the launch's block records
    uint32_t n;             // N < 2^32
    uint32_t block;         // B
    uint32_t n_blocks;      // ceil(N / B)
    uint32_t pieces_per_block;  // of a whole block; only the last block may have fewer
    uint32_t k;             // max(1, floor(n_blocks * top_permille / 1000)); 0 when there is no block
    uint32_t format;        // rg_sample_format
};  // 48 bytes
struct RgDrPlaneOut {       // the raw numbers of a plane: the same bits on every route
    double top_ms, mean_square;
    uint32_t peak, peak2, blocks, top_blocks, nonfinite, reserved;
};  // 40 bytes

// ---- samples ---------------------------------------------------------------------------------------------------------------
RG_DR_HD uint32_t rg_dr_step_samples(uint32_t format) { return 16u / rg_pcm_bps(format); }
RG_DR_HD uint32_t rg_dr_piece_samples(uint32_t format) { return RG_DR_PIECE_BYTES / rg_pcm_bps(format); }
// s^2
RG_DR_HD double rg_dr_scale2(uint32_t format) {
    return format == RG_FMT_S16_PLANAR ? 1073741824.0 : (format == RG_FMT_S32_PLANAR ? 4611686018427387904.0 : 70368744177664.0);
}
RG_DR_HD double rg_dr_scale(uint32_t format) { return format == RG_FMT_S16_PLANAR ? 32768.0 : (format == RG_FMT_S32_PLANAR ? 2147483648.0 : 8388608.0); }

RG_DR_HD RgDrPiece rg_dr_empty() { return RgDrPiece{0u, 0u, 0u, 0u}; }

// |q| of a sample.  `raw`: the stored pattern, an S16 sample sign-extended to 32 bits.  |q| <= 2^31 fits an unsigned word where q
// = +2^31 (a float at or beyond +256) fits no int32.  x * 2^23 is exact in float (a power of two, and after the clamp nothing
// overflows; what is subnormal or becomes so rounds to 0 either way), so rintf gives llrint's integer.
template <int FMT>
RG_DR_HD uint32_t rg_dr_abs_q(uint32_t raw, bool *finite) {
    *finite = true;
    if (FMT == RG_FMT_F32_PLANAR) {
        if ((raw & 0x7F800000u) == 0x7F800000u) {
            *finite = false;
            return 0u;
        }
        float x;
        const uint32_t mag = raw & 0x7FFFFFFFu;
        memcpy(&x, &mag, 4);
        return (uint32_t)rintf(fminf(x, 256.0f) * 8388608.0f);
    }
    const int32_t v = (int32_t)raw;
    return v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
}
// one sample into the sums
template <int FMT>
RG_DR_HD void rg_dr_take(uint32_t raw, RgDrPiece *p) {
    bool finite;
    const uint32_t a = rg_dr_abs_q<FMT>(raw, &finite);
    if (FMT == RG_FMT_S16_PLANAR) {
        p->lo += a * a;  // <= 2^30
    } else {
        const uint64_t sq = (uint64_t)a * a;
        p->lo += sq & 0xFFFFFFFFu;
        p->hi += sq >> 32;
    }
    p->peak = a > p->peak ? a : p->peak;
    p->nonfinite += finite ? 0u : 1u;
}
// a <- a + b
RG_DR_HD void rg_dr_combine(RgDrPiece *a, const RgDrPiece &b) {
    a->hi += b.hi;
    a->lo += b.lo;
    a->peak = b.peak > a->peak ? b.peak : a->peak;
    a->nonfinite += b.nonfinite;
}
// e: E = hi * 2^32 + lo rounded once to double.  H < 2^54 and L < 2^32 convert exactly and H * 2^32 is exact, so the one
// rounding is the addition's (and a fused multiply-add rounds the same exact sum once: contraction cannot change it)
RG_DR_HD double rg_dr_energy(const RgDrPiece &p) {
    const uint64_t H = p.hi + (p.lo >> 32), L = p.lo & 0xFFFFFFFFu;
    return (double)H * 4294967296.0 + (double)L;
}
RG_DR_HD double rg_dr_mean_square(double e, uint32_t n, uint32_t format) { return 2.0 * e / ((double)n * rg_dr_scale2(format)); }
// a block of `n` samples from its sums
RG_DR_HD RgDrBlock rg_dr_block(const RgDrPiece &p, uint32_t n, uint32_t format) {
    RgDrBlock b;
    b.e = rg_dr_energy(p);
    b.ms = rg_dr_mean_square(b.e, n, format);
    b.peak = p.peak;
    b.reserved = 0;
    return b;
}

// ---- cutting ---------------------------------------------------------------------------------------------------------------
// block `b` of a plane: [*start, *start + return)
RG_DR_HD uint32_t rg_dr_block_window(const RgDrPlane &p, uint32_t b, uint64_t *start) {
    *start = (uint64_t)b * p.block;
    const uint64_t left = p.n - *start;
    return left < p.block ? (uint32_t)left : p.block;
}
// pieces of a block of `len` samples
RG_DR_HD uint32_t rg_dr_pieces_of(uint32_t len, uint32_t format) {
    const uint32_t T = rg_dr_piece_samples(format);
    return (len + T - 1) / T;
}
// piece `k` of a block of `len` samples: [*start, *start + return) of the block
RG_DR_HD uint32_t rg_dr_piece_window(uint32_t len, uint32_t k, uint32_t format, uint32_t *start) {
    const uint32_t T = rg_dr_piece_samples(format);
    *start = k * T;
    return len - *start < T ? len - *start : T;
}

// all the pieces of a plane
RG_DR_HD uint64_t rg_dr_plane_pieces(const RgDrPlane &p) {
    if (!p.n_blocks) return 0;
    uint64_t start;
    const uint32_t tail = rg_dr_block_window(p, p.n_blocks - 1, &start);
    return (uint64_t)(p.n_blocks - 1) * p.pieces_per_block + rg_dr_pieces_of(tail, p.format);
}

// ---- selection -------------------------------------------------------------------------------------------------------------
// ms >= 0 (never -0.0: a quotient of non-negative numbers), so the doubles order as their patterns do, unsigned
RG_DR_HD uint64_t rg_dr_key(double ms) {
    uint64_t u;
    memcpy(&u, &ms, 8);
    return u;
}
RG_DR_HD double rg_dr_unkey(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}
// pass `pass` (0 = the top digit) looks at keys whose digits above it equal `prefix`'s
RG_DR_HD bool rg_dr_in_prefix(uint64_t key, uint64_t prefix, uint32_t pass) {
    return pass == 0 || (key >> (64u - RG_DR_RADIX_BITS * pass)) == prefix;
}
RG_DR_HD uint32_t rg_dr_digit(uint64_t key, uint32_t pass) { return (uint32_t)(key >> (64u - RG_DR_RADIX_BITS * (pass + 1))) & (RG_DR_BINS - 1u); }
// hist: the digits of the keys in the prefix.  The `need`-th largest of them (1 <= need <= their number) has the returned
// digit; *above: how many have a larger one
template <class Hist>
RG_DR_HD uint32_t rg_dr_pick(const Hist &hist, uint32_t need, uint32_t *above) {
    uint32_t cum = 0;
    for (uint32_t d = RG_DR_BINS - 1u; d > 0; --d) {
        const uint32_t h = hist[d];
        if (cum + h >= need) {
            *above = cum;
            return d;
        }
        cum += h;
    }
    *above = cum;
    return 0u;
}

// ---- a plane from its blocks -----------------------------------------------------------------------------------------------
// block(b) for b in [0, n_blocks), t = the k-th largest ms and g = the blocks with ms > t.  One walk in ascending block index.
template <class GetBlock>
RG_DR_HD RgDrPlaneOut rg_dr_plane(GetBlock block, const RgDrPlane &p, double t, uint32_t g, uint32_t nonfinite) {
    RgDrPlaneOut o;
    o.top_ms = o.mean_square = 0.0;
    o.peak = o.peak2 = 0u;
    o.blocks = p.n_blocks;
    o.top_blocks = p.k;
    o.nonfinite = nonfinite;
    o.reserved = 0;
    if (!p.n_blocks) return o;
    double S = 0.0, e = 0.0;
    uint32_t p1 = 0, p2 = 0;
    for (uint32_t b = 0; b < p.n_blocks; ++b) {
        const RgDrBlock r = block(b);
        if (r.ms > t) S += r.ms;
        e += r.e;
        if (b == 0) {
            p1 = p2 = r.peak;  // one block: it is the second element too
        } else if (b == 1) {
            p2 = r.peak < p1 ? r.peak : p1;
            p1 = r.peak > p1 ? r.peak : p1;
        } else if (r.peak > p1) {
            p2 = p1;
            p1 = r.peak;
        } else if (r.peak > p2) {
            p2 = r.peak;
        }
    }
    for (uint32_t j = g; j < p.k; ++j) S += t;
    o.top_ms = S / (double)p.k;
    o.mean_square = rg_dr_mean_square(e, p.n, p.format);
    o.peak = p1;
    o.peak2 = p2;
    return o;
}

// ---- rg_dr_host.cpp (plain C++: no device, no context) ---------------------------------------------------------------------
// NULL -> the defaults; RG_ERR_INVALID_ARG for top_permille outside 1 .. 1000 or block_frames beyond RG_DR_MAX_BLOCK_FRAMES
int rg_dr_options(const rg_dr_opts *opts, rg_dr_opts *out, char *err, size_t err_len);
// The planes of track i, described by `t`, in an arena of `arena_bytes` bytes: planes[0 .. t.channels).  RG_ERR_FORMAT unless
// it is 1 .. 8 channels of one of the three formats and fewer than 2^32 frames, and -- when the block length comes from the
// sample rate -- 1 <= 3 * sample_rate <= RG_DR_MAX_BLOCK_FRAMES where `rate_is_format` (the file route: such a stream fails
// alone), RG_ERR_INVALID_ARG otherwise; RG_ERR_INVALID_ARG unless the planes lie inside the arena, sample-aligned.  The text
// goes to err[err_len].  first_piece and first_block are rg_dr_plan's to set.
int rg_dr_track_planes(size_t i, const rg_track_desc &t, const rg_dr_opts &o, bool rate_is_format, size_t arena_bytes, RgDrPlane *planes, char *err,
                       size_t err_len);
// pieces and block records of the `n` planes of a launch, the pieces of each format contiguous: fmt_piece[f] ..
// fmt_piece[f + 1] are format f's; returns the number of pieces, *n_blocks: of block records
uint64_t rg_dr_plan(RgDrPlane *planes, size_t n, uint64_t fmt_piece[4], uint64_t *n_blocks);
// one plane's raw numbers from host memory: the definitions, serially ...
RgDrPlaneOut rg_dr_serial_host(const unsigned char *arena, const RgDrPlane &p);
// ... and as the kernels compute them: pieces, block records, the radix select, the walk
RgDrPlaneOut rg_dr_folded_host(const unsigned char *arena, const RgDrPlane &p);
// the finish: the result record of a track that was scanned; po[0 .. t.channels) are its planes', block = B
void rg_dr_fill(const rg_track_desc &t, uint32_t block, uint32_t dropped_frames, const RgDrPlaneOut *po, rg_dr_result *out);
// routes 0 and 2 of rg_dr_arena
int rg_dr_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_dr_opts *opts, const void *arena, size_t arena_bytes, rg_dr_result *out,
                     char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` planes in the device arena at `d_arena` (allocated in whole 16-byte words): the kernels on `s`, po[i] <- plane i; `s`
// has been synchronised on return
int rg_dr_device(rg_ctx *c, const unsigned char *d_arena, RgDrPlane *planes, size_t n, RgDrPlaneOut *po, hipStream_t s);
#endif
