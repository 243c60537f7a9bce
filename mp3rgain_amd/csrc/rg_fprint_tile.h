// rg_fprint_tile.h -- internal, HIP only: the tile walk that the fingerprint kernel (rg_fprint.hip) and the onset kernel of the
// tempo scan (rg_tempo.hip) share.  Both make, per tile of RG_FP_TILE_CODES = 7 hops of one track, the band energies of its 8
// frames of 4096 samples at hop 512, and differ only in the bands (33 or 32, the edges in the track record) and in what they
// make of two neighbouring rows.  rg_fp_tile_bands is the whole of that: the tile's samples are read from the arena once,
// down-mixed ((ch0 + ch1) * 0.5f) and staged in LDS, consecutive lanes reading consecutive samples; every frame is windowed from
// there; frames are transformed two at a time, as the real and imaginary part of one 4096-point complex transform (the spectral
// scan's three radix-16 passes in registers, its exchange buffer and padding); lanes 0 .. BANDS - 1 sum the bands of the first
// frame, lanes 64 .. 64 + BANDS - 1 (another wave) those of the second, in bin order, and the rows stay in LDS.  A unit that
// includes this is compiled without contraction: same input, same bits as rg_fp_tile_bands_host (rg_fprint.h).
#pragma once

#include <string.h>

#include <vector>

#include "rg_fprint.h"

#define RG_FP_ROW 18u   // complex per row of 16 in the exchange buffer (as rg_spectrum.hip)
#define RG_FP_K0 306u   // complex per k0
#define RG_FP_XCH (16u * RG_FP_K0)
// the dynamic LDS of a tile kernel of `bands` bands: [exchange | staged samples | band energies | edges]
#define RG_FP_TILE_LDS(bands) (RG_FP_XCH * 8u + RG_FP_STAGE * 4u + RG_FP_TILE_FRAMES * (bands) * 4u + ((bands) + 1u) * 4u)

__device__ __forceinline__ uint32_t fp_pos(uint32_t k) { return k + ((k + 7u) >> 3); }

template <int FMT>
__device__ __forceinline__ float fp_load(const unsigned char *plane, uint64_t k) {
    if (FMT == RG_FMT_S16_PLANAR) return rg_spec_value<FMT>((uint32_t)(int32_t) reinterpret_cast<const int16_t *>(plane)[k]);
    return rg_spec_value<FMT>(reinterpret_cast<const uint32_t *>(plane)[k]);
}

// where the rows of band energies of a tile kernel's LDS start
__device__ __forceinline__ float *rg_fp_tile_rows(unsigned char *s_raw) {
    return reinterpret_cast<float *>(s_raw + RG_FP_XCH * 8u) + RG_FP_STAGE;
}

// Tile t of track p by a workgroup of RG_FP_LANES lanes, every lane calling it: on return (after a barrier) the rows
// E[i * BANDS + m], i < nf, lie at rg_fp_tile_rows; -> nf, the tile's frames (frame f0 = t * 7 is row 0).  *nonfinite: the
// non-finite frames among those the tile owns (the same value in every lane).  `edges`: BANDS + 1 edges to take instead of p.e.
template <int FMT, uint32_t BANDS>
__device__ __forceinline__ uint32_t rg_fp_tile_bands(const unsigned char *__restrict__ arena, const RgSpecTables *__restrict__ tables, const RgFpTrack &p,
                                                     uint32_t t, unsigned char *s_raw, uint32_t *nonfinite_out,
                                                     const uint32_t *__restrict__ edges = nullptr) {
    RgSpecC *s_x = reinterpret_cast<RgSpecC *>(s_raw);
    float *s_pcm = reinterpret_cast<float *>(s_raw + RG_FP_XCH * 8u);
    float *s_E = s_pcm + RG_FP_STAGE;
    uint32_t *s_e = reinterpret_cast<uint32_t *>(s_E + RG_FP_TILE_FRAMES * BANDS);
    const uint32_t tid = threadIdx.x, hi = tid >> 4, lo = tid & 15u;
    const uint32_t f0 = t * RG_FP_TILE_CODES;
    const uint32_t left = p.frames - f0, nf = left < RG_FP_TILE_FRAMES ? left : RG_FP_TILE_FRAMES;
    const uint32_t count = (nf - 1u) * RG_FP_HOP + RG_FP_FRAME;  // f0 + nf <= F: the last sample is below N
    {
        const unsigned char *p0 = arena + p.off0, *p1 = arena + p.off1;
        const uint64_t base = (uint64_t)f0 * RG_FP_HOP;
        const bool two = p.channels >= 2;
        for (uint32_t k = tid; k < count; k += RG_FP_LANES) {
            const float a = fp_load<FMT>(p0, base + k);
            s_pcm[k] = two ? (a + fp_load<FMT>(p1, base + k)) * 0.5f : a;
        }
        if (tid <= BANDS) s_e[tid] = edges ? edges[tid] : p.e[tid];  // (the key scan's 61 edges do not fit the record)
    }
    float win[16];
#pragma unroll
    for (uint32_t n2 = 0; n2 < 16; ++n2) win[n2] = tables->window[256u * n2 + tid];
    uint32_t nonfinite = 0;
    __syncthreads();
    for (uint32_t pr = 0; pr < nf; pr += 2) {
        const bool has_b = pr + 1 < nf;
        const float *fa = s_pcm + pr * RG_FP_HOP + tid, *fb = has_b ? fa + RG_FP_HOP : fa;
        RgSpecC v[16];
#pragma unroll
        for (uint32_t n2 = 0; n2 < 16; ++n2) {
            v[n2].x = fa[256u * n2];
            v[n2].y = fb[256u * n2];
        }
        bool use_a = true, use_b = has_b;
        if (FMT == RG_FMT_F32_PLANAR) {
            int bad_a = 0, bad_b = 0;
#pragma unroll
            for (uint32_t n2 = 0; n2 < 16; ++n2) {
                bad_a |= rg_fp_nonfinite(v[n2].x) ? 1 : 0;
                bad_b |= rg_fp_nonfinite(v[n2].y) ? 1 : 0;
            }
            bad_a = __syncthreads_or(bad_a);
            bad_b = __syncthreads_or(bad_b);
            use_a = !bad_a;
            use_b = has_b && !bad_b;
            // a tile owns every frame but its first, which is the last of the tile before; tile 0 owns that too
            nonfinite += (bad_a && (pr || !t) ? 1u : 0u) + (has_b && bad_b ? 1u : 0u);
        }
#pragma unroll
        for (uint32_t n2 = 0; n2 < 16; ++n2) {
            v[n2].x = use_a ? v[n2].x * win[n2] : 0.0f;
            v[n2].y = use_b ? v[n2].y * win[n2] : 0.0f;
        }
        rg_spec_pass1(v, tid, tables->tw1);  // lane = 16 n1 + n0
#pragma unroll
        for (uint32_t k0 = 0; k0 < 16; ++k0) s_x[k0 * RG_FP_K0 + hi * RG_FP_ROW + lo] = v[k0];
        __syncthreads();
        {  // pass 2: lane = 16 k0 + n0, in its own 16 places
            RgSpecC *col = s_x + hi * RG_FP_K0 + lo;
#pragma unroll
            for (uint32_t n1 = 0; n1 < 16; ++n1) v[n1] = col[n1 * RG_FP_ROW];
            rg_spec_pass2(v, lo, tables->tw2);
#pragma unroll
            for (uint32_t k1 = 0; k1 < 16; ++k1) col[k1 * RG_FP_ROW] = v[k1];
        }
        __syncthreads();
        {  // pass 3: lane = 16 k1 + k0
            const float4 *row = reinterpret_cast<const float4 *>(s_x + lo * RG_FP_K0 + hi * RG_FP_ROW);
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) {
                const float4 f = row[q];
                v[2 * q] = RgSpecC{f.x, f.y};
                v[2 * q + 1] = RgSpecC{f.z, f.w};
            }
        }
        __syncthreads();  // every lane has read: Z takes the buffer
        rg_spec_dft16(v);
#pragma unroll
        for (uint32_t k2 = 0; k2 < 16; ++k2) s_x[fp_pos(tid + 256u * k2)] = v[k2];
        __syncthreads();
        {
            const uint32_t which = tid >> 6, m = tid & 63u;  // wave 0: the first frame's bands, wave 1: the second's
            if (which < 2 && m < BANDS && (which == 0 || has_b)) {
                const float s = rg_fp_band([&](uint32_t k) { return s_x[fp_pos(k)]; }, s_e[m], s_e[m + 1], which);
                s_E[(pr + which) * BANDS + m] = (which ? use_b : use_a) ? s : 0.0f;
            }
        }
        __syncthreads();  // the bands have been read: the next pair's pass 1 may write
    }
    *nonfinite_out = nonfinite;
    return nf;
}

// one workgroup per track: the non-finite frames its tiles counted, summed (a template, so that each unit that launches it has it)
template <int UNIT>
__global__ __launch_bounds__(256) void rg_fp_fold_kernel(const RgFpTrack *__restrict__ tracks, const uint32_t *__restrict__ tile_nonfinite,
                                                         uint32_t *__restrict__ out) {
    __shared__ uint32_t s_sum[256];
    const uint32_t tid = threadIdx.x;
    const RgFpTrack &p = tracks[blockIdx.x];
    uint32_t sum = 0;
    for (uint32_t t = tid; t < p.n_tiles; t += 256u) sum += tile_nonfinite[p.first_tile + t];
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t w = 128; w; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = s_sum[0];
}

// ---- one call's launches ---------------------------------------------------------------------------------------------------
// Device layout of the work buffer, every part 16-byte aligned: [tables | track records | tile -> track | tile counts | track counts]
struct FpJob {
    uint64_t fmt_tile[4];
    std::vector<unsigned char> head;  // the device buffer's bytes [0, counts_at)
    size_t tracks_at, map_at, counts_at, res_at, end, n;
};
static inline size_t fp_a16(size_t x) { return (x + 15) & ~(size_t)15; }

// `tracks` have been planned (rg_fp_plan)
static inline void fp_job(const RgFpTrack *tracks, size_t n, const uint64_t fmt_tile[4], FpJob *job) {
    memcpy(job->fmt_tile, fmt_tile, sizeof job->fmt_tile);
    const uint64_t tiles = fmt_tile[3];
    job->n = n;
    job->tracks_at = fp_a16(sizeof(RgSpecTables));
    job->map_at = fp_a16(job->tracks_at + n * sizeof(RgFpTrack));
    job->counts_at = fp_a16(job->map_at + (size_t)tiles * sizeof(uint32_t));
    job->res_at = fp_a16(job->counts_at + (size_t)tiles * sizeof(uint32_t));
    job->end = fp_a16(job->res_at + n * sizeof(uint32_t));
    job->head.assign(job->counts_at, 0);
    memcpy(job->head.data(), &rg_spec_tables(), sizeof(RgSpecTables));
    memcpy(job->head.data() + job->tracks_at, tracks, n * sizeof(RgFpTrack));
    uint32_t *map = reinterpret_cast<uint32_t *>(job->head.data() + job->map_at);
    for (size_t i = 0; i < n; ++i)
        for (uint32_t t = 0; t < tracks[i].n_tiles; ++t) map[tracks[i].first_tile + t] = (uint32_t)i;
}
