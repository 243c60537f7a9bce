// rg_ancestry.h -- internal: the lossy ancestry scan (include/mp3rgain_amd_ancestry.h) as rg_ancestry.hip (kernels, launcher,
// seams), rg_ancestry_host.cpp (the serial host twin, the kernels' cutting walked by the host, the finish) and
// rg_file_verify.hip (rg_ancestry) share it.  What a sample is worth, the windowing, the matrixing, the MDCT, the butterflies
// and the group statistic are host and device code, written once here as chains of explicit fused multiply-adds in a fixed
// order; every file that includes this header is built with -ffp-contract=off.  The counts are integers, so the order in
// which workgroups add them does not matter: same input, same bits on every route.
//
// The cutting.  Alignments r and r + 32 see the same subband sequence shifted by one slot, so per (view, segment) there are 32
// polyphase phases p = r mod 32; alignment r = 32 q + p, granule g, slot t is slot u = q + 18 g + t of phase p, whose newest
// sample is a + p + 32 u + 31.  A workgroup takes one phase of one TILE of up to RG_ANC_TILE granules of one segment of one
// view: the samples into LDS, 18 ng + 35 slots x 32 subbands into LDS (the slots of the granule before the tile for the MDCT's
// history and 17 more for q = 1 .. 17), then the MDCT, the butterflies and the statistic at each of the 18 slot alignments.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mp3rgain_amd_ancestry.h"
#include "rg_pcm_plane.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_ANC_HD __host__ __device__ __forceinline__
#else
#define RG_ANC_HD inline
#endif

#define RG_ANC_LANES 256u
#define RG_ANC_PHASES 32u
#define RG_ANC_TILE 4u                                         // granules of a workgroup's tile
#define RG_ANC_TILE_SLOTS (18u * RG_ANC_TILE + 35u)            // 179
#define RG_ANC_TILE_SAMPLES (32u * RG_ANC_TILE_SLOTS + 480u)   // 6208
#define RG_ANC_GROUP 12u
#define RG_ANC_INV12 0.083333336f                              // (float)(1.0 / 12)

struct RgAncTables {      // built once on the host in double and rounded (rg_anc_tables), the same bits on the device
    float c[512];         // C = D / 32
    float mt[64][32];     // mt[j][k] = M[k][j]
    float wt[36][18];     // wt[i][l] = W[l][i]
    float cs[8], ca[8];
};
struct RgAncView {        // one view of a launch
    uint64_t off_a, off_b;  // the plane(s), from the arena's base, in bytes (sample-aligned); off_b for mid and side
    uint32_t n;             // N < 2^32
    uint32_t format;        // rg_sample_format
    uint32_t mix;           // 0 = the plane, 1 = mid, 2 = side
    uint32_t reserved;
};  // 32 bytes
struct RgAncJob {         // one tile of one segment of one view; 32 workgroups, one per phase
    uint64_t a;           // the segment's first frame
    uint32_t view;
    uint32_t g0, ng;      // granules g0 .. g0 + ng - 1, g0 >= 1, 1 <= ng <= RG_ANC_TILE
    uint32_t reserved;
};  // 24 bytes

RG_ANC_HD float rg_anc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---- samples ---------------------------------------------------------------------------------------------------------------
RG_ANC_HD bool rg_anc_nonfinite(uint32_t bits) { return (bits & 0x7F800000u) == 0x7F800000u; }
RG_ANC_HD float rg_anc_plane_sample(const unsigned char *arena, uint64_t off, uint32_t format, uint32_t k) {
    if (format == RG_FMT_S16_PLANAR) {
        int16_t s;
#if defined(__HIP_DEVICE_COMPILE__)
        s = *reinterpret_cast<const int16_t *>(arena + off + 2ull * k);
#else
        memcpy(&s, arena + off + 2ull * k, 2);
#endif
        return (float)s;
    }
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = *reinterpret_cast<const uint32_t *>(arena + off + 4ull * k);
#else
    memcpy(&u, arena + off + 4ull * k, 4);
#endif
    if (format == RG_FMT_S32_PLANAR) return (float)(int32_t)u * 1.52587890625e-05f;
    if (rg_anc_nonfinite(u)) return 0.0f;
    float x;
    memcpy(&x, &u, 4);
    return x * 32768.0f;
}
RG_ANC_HD float rg_anc_sample(const unsigned char *arena, const RgAncView &v, int64_t idx) {
    if (idx < 0 || idx >= (int64_t)v.n) return 0.0f;
    const float l = rg_anc_plane_sample(arena, v.off_a, v.format, (uint32_t)idx);
    if (v.mix == 0) return l;
    const float r = rg_anc_plane_sample(arena, v.off_b, v.format, (uint32_t)idx);
    return v.mix == 1 ? 0.5f * (l + r) : 0.5f * (l - r);
}

// ---- the filterbank: X(i), Y(j), Z(i) are callables -----------------------------------------------------------------------
template <class GetX>
RG_ANC_HD float rg_anc_window(const RgAncTables &t, GetX X, uint32_t j) {
    float acc = 0.0f;
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) acc = rg_anc_fma(t.c[j + 64u * m], X(j + 64u * m), acc);
    return acc;
}
template <class GetY>
RG_ANC_HD float rg_anc_matrix(const RgAncTables &t, GetY Y, uint32_t k) {
    float acc = 0.0f;
#pragma unroll 8
    for (uint32_t j = 0; j < 64; ++j) acc = rg_anc_fma(t.mt[j][k], Y(j), acc);
    return acc;
}
// the 32 subbands of one slot at once (host routes): the same 32 chains, walked side by side so that a compiler may use vectors
inline void rg_anc_matrix32(const RgAncTables &t, const float y[64], float out[32]) {
    for (uint32_t k = 0; k < 32; ++k) out[k] = 0.0f;
    for (uint32_t j = 0; j < 64; ++j)
        for (uint32_t k = 0; k < 32; ++k) out[k] = rg_anc_fma(t.mt[j][k], y[j], out[k]);
}
// the 18 lines of one subband from its 36 slots; Z(i) is already negated where the inversion asks
template <class GetZ>
RG_ANC_HD void rg_anc_mdct(const RgAncTables &t, GetZ Z, float x[18]) {
#pragma unroll
    for (uint32_t l = 0; l < 18; ++l) x[l] = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 36; ++i) {
        const float z = Z(i);
#pragma unroll
        for (uint32_t l = 0; l < 18; ++l) x[l] = rg_anc_fma(t.wt[i][l], z, x[l]);
    }
}
RG_ANC_HD float rg_anc_invert(float s, uint32_t sb, uint32_t i) { return (sb & 1u) && (i & 1u) ? -s : s; }
RG_ANC_HD float rg_anc_bfly_lo(float a, float b, float cs, float ca) { return rg_anc_fma(b, ca, a * cs); }
RG_ANC_HD float rg_anc_bfly_up(float a, float b, float cs, float ca) { return rg_anc_fma(-a, ca, b * cs); }

// ---- the statistic ---------------------------------------------------------------------------------------------------------
RG_ANC_HD float rg_anc_ssq(float acc, float c) { return rg_anc_fma(c, c, acc); }
RG_ANC_HD float rg_anc_ms(float q) { return q * RG_ANC_INV12; }
RG_ANC_HD bool rg_anc_is_small(float c, float ms) { return 256.0f * (c * c) < ms; }

// the 576 lines of one granule at one alignment, in place: butterflies, then the counts (the host routes; the kernel does the
// same steps across the lanes of a half-wave)
inline void rg_anc_granule_counts(const RgAncTables &t, float x[576], float floor_, uint32_t *small_, uint32_t *active_) {
    for (uint32_t sb = 1; sb < 32; ++sb)
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t lo = 18u * sb - 1u - i, up = 18u * sb + i;
            const float a = x[lo], b = x[up];
            x[lo] = rg_anc_bfly_lo(a, b, t.cs[i], t.ca[i]);
            x[up] = rg_anc_bfly_up(a, b, t.cs[i], t.ca[i]);
        }
    uint32_t s = 0, a = 0;
    for (uint32_t g = 0; g < 48; ++g) {
        float q = 0.0f;
        for (uint32_t i = 0; i < RG_ANC_GROUP; ++i) q = rg_anc_ssq(q, x[RG_ANC_GROUP * g + i]);
        const float ms = rg_anc_ms(q);
        if (!(ms >= floor_)) continue;
        a += RG_ANC_GROUP;
        for (uint32_t i = 0; i < RG_ANC_GROUP; ++i) s += rg_anc_is_small(x[RG_ANC_GROUP * g + i], ms) ? 1u : 0u;
    }
    *small_ = s;
    *active_ = a;
}

// ---- segments --------------------------------------------------------------------------------------------------------------
// S and G as they are used for a plane of N frames (S = 0: nothing is analysed)
inline void rg_anc_cut(uint64_t N, uint32_t want_s, uint32_t want_g, uint32_t *S, uint32_t *G) {
    *S = 0;
    *G = 0;
    if (N < 3u * 576u) return;
    const uint64_t whole = N / 576u - 2u;
    if (want_s == 0 || (uint64_t)want_g > whole) {
        *S = 1;
        *G = (uint32_t)whole;
        return;
    }
    const uint64_t L = 576ull * (want_g + 2ull), fit = N / L;
    *S = (uint32_t)(fit < want_s ? fit : want_s);
    *G = want_g;
}
inline uint64_t rg_anc_start(uint64_t N, uint32_t S, uint32_t G, uint32_t j) {
    if (S <= 1) return 0;
    const uint64_t L = 576ull * (G + 2ull);
    return 576ull * (uint64_t)(((unsigned __int128)j * (N - L)) / (576ull * (S - 1ull)));
}

// ---- rg_ancestry_host.cpp (plain C++: no device, no context) ------------------------------------------------------------------
const RgAncTables &rg_anc_tables();
// NULL -> the defaults, zeros -> the defaults; RG_ERR_INVALID_ARG as the header says
int rg_anc_options(const rg_ancestry_opts *opts, rg_ancestry_opts *out, char *err, size_t err_len);
// the views of track `i` into views[0 .. *n_views): checks format, channels (1 .. 8), frames < 2^32 (RG_ERR_FORMAT), alignment
// and that the planes lie inside the arena (RG_ERR_INVALID_ARG); the text goes to err[err_len]
int rg_anc_track_views(size_t i, const rg_track_desc &t, size_t arena_bytes, RgAncView *views, uint32_t *n_views, char *err, size_t err_len);
// the tiles of view `view` of a track of N frames, appended to *jobs; *S and *G as they are used
void rg_anc_jobs(uint64_t N, const rg_ancestry_opts &o, uint32_t view, std::vector<RgAncJob> *jobs, uint32_t *S, uint32_t *G);
// route 0: small[576] and active[576] of one view, alignment by alignment; *nonfinite over the whole plane
void rg_anc_serial_host(const unsigned char *arena, const RgAncView &v, const rg_ancestry_opts &o, uint64_t *small_, uint64_t *active_, uint64_t *nonfinite);
// route 2: one phase of one tile, added to small[576] / active[576]
void rg_anc_tile_host(const unsigned char *arena, const RgAncView &v, const RgAncJob &job, uint32_t phase, float floor_, uint64_t *small_, uint64_t *active_);
uint64_t rg_anc_count_nonfinite(const unsigned char *arena, const RgAncView &v);
// the finish: counts[v] = small[576] then active[576] of view v
void rg_anc_fill(const rg_track_desc &t, const rg_ancestry_opts &o, uint32_t S, uint32_t G, uint32_t dropped_frames, uint32_t n_views, const RgAncView *views,
                 const uint64_t *counts, const uint64_t *nonfinite, rg_ancestry_result *out);
int rg_anc_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_ancestry_opts *opts, const void *arena, size_t arena_bytes,
                      rg_ancestry_result *out, uint64_t *counts, char *err, size_t err_len);
double rg_anc_fma_per_sample(uint32_t G);

// ---- rg_ancestry.hip ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct rg_ctx;
// the kernels over `n_views` views and their jobs on stream `s`; counts[v * 1152 ..) and nonfinite[v] come back.  The callers
// have checked every view against the arena.
int rg_anc_device(rg_ctx *c, const unsigned char *d_arena, const RgAncView *views, size_t n_views, const std::vector<RgAncJob> &jobs, float floor_,
                  uint64_t *counts, uint64_t *nonfinite, hipStream_t s);
#endif
