// rg_tempo.hip -- the tempo scan on the device (include/mp3rgain_amd_tempo.h, rg_tempo.h): per track an onset curve of one
// integer per 512 samples from the planes of the analysis arena, its windowed autocorrelation, and the all-integer finish.
//
//   rg_tp_tiles_kernel   stage 1: one workgroup of 256 lanes per tile of 7 onsets of one track, many tracks per launch, one launch
//                        per format.  The tile walk is the fingerprint's (rg_fprint_tile.h: the tile's down-mixed samples staged
//                        in LDS once, 8 frames windowed from there, two per transform through the spectral scan's passes), here
//                        with 32 bands from 60 to 8000 Hz; the 8 x 32 band energies stay in LDS and lanes 0 .. 6 make the
//                        onsets (rg_tp_onset: a shift of the f32 bit pattern for a logarithm, the rises summed).  69 KB of LDS.
//   rg_tp_acf_kernel     stage 2: one workgroup per (track, window).  The window's 2W onsets lie in LDS as 32-bit words; lanes
//                        own lags, four consecutive ones each (256 x 4 = the largest W): per step of four i a lane reads four
//                        o[i ..] (one 16-byte broadcast) and four new o[i + d ..] (one 16-byte read, consecutive lanes 16 bytes
//                        apart) and does 16 multiply-adds on a sliding register window of 8 values.  B_w[d] comes from a prefix
//                        sum of the window in LDS.  c_w goes to LDS, from where the lanes score their candidates (lanes own
//                        periods; a tree with rg_tp_better closes the window's P16_w), and into the track's C by 64-bit integer
//                        atomic additions: whatever their order, the sum is the same.
//   rg_tp_finish_kernel  one workgroup per track: C in LDS, lanes own periods (the track's P16), then windows (stability), then
//                        phases of the beat grid, each closed by a tree in LDS with the host's total orders.
// No float after stage 1; this unit is compiled without contraction: same input, same bytes as the host twins.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_fprint_tile.h"
#include "rg_pcm_seam.h"
#include "rg_tempo.h"

#define RG_TP_LDS_BYTES RG_FP_TILE_LDS(RG_TEMPO_BANDS)

template <int FMT>
__global__ __launch_bounds__(RG_FP_LANES) void rg_tp_tiles_kernel(const unsigned char *__restrict__ arena, const RgSpecTables *__restrict__ tables,
                                                                  const RgFpTrack *__restrict__ tracks, const uint32_t *__restrict__ tile_track,
                                                                  uint64_t tile_base, uint16_t *__restrict__ onsets, float *__restrict__ bands,
                                                                  uint32_t *__restrict__ tile_nonfinite) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const float *s_E = rg_fp_tile_rows(s_raw);
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = tile_base + blockIdx.x;
    const RgFpTrack &p = tracks[tile_track[tile]];
    const uint32_t t = (uint32_t)(tile - p.first_tile), f0 = t * RG_TP_TILE_ONSETS;
    uint32_t nonfinite;
    const uint32_t nf = rg_fp_tile_bands<FMT, RG_TEMPO_BANDS>(arena, tables, p, t, s_raw, &nonfinite);
    // f0 + tid + 1 < f0 + nf <= F: onset f0 + tid is below K = F - 1
    if (tid + 1 < nf) onsets[p.codes_at + f0 + tid] = rg_tp_onset(s_E + tid * RG_TEMPO_BANDS, s_E + (tid + 1) * RG_TEMPO_BANDS);
    if (bands) {
        float *dst = bands + (p.frames_at + f0) * RG_TEMPO_BANDS;
        for (uint32_t k = tid + (t ? RG_TEMPO_BANDS : 0u); k < nf * RG_TEMPO_BANDS; k += RG_FP_LANES) dst[k] = s_E[k];
    }
    if (tid == 0) tile_nonfinite[tile] = nonfinite;
}

// the best of s[0 .. 256) by `better`, to s[0]; every lane calls it, s[tid] written before
template <class T, class Better>
__device__ __forceinline__ void tp_tree(T *s, uint32_t tid, Better better) {
    __syncthreads();
    for (uint32_t w = RG_TP_ACF_LANES / 2; w; w >>= 1) {
        if (tid < w) {
            const T other = s[tid + w];
            if (better(other, s[tid])) s[tid] = other;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RG_TP_ACF_LANES) void rg_tp_acf_kernel(const uint16_t *__restrict__ onsets, const RgTpTrack *__restrict__ tracks,
                                                                    const uint32_t *__restrict__ win_track, uint32_t W, uint32_t hop,
                                                                    uint32_t *__restrict__ p16_w, unsigned long long *__restrict__ acf) {
    __shared__ __attribute__((aligned(16))) uint32_t s_a[RG_TEMPO_MAX_WINDOW];      // o[s_w + i], zeros from W on
    __shared__ __attribute__((aligned(16))) uint32_t s_b[2u * RG_TEMPO_MAX_WINDOW]; // o[s_w + j], zeros from 2W on
    __shared__ uint32_t s_p[2u * RG_TEMPO_MAX_WINDOW + 1u];                         // s_p[j] = s_b[0] + .. + s_b[j - 1]
    __shared__ int32_t s_c[RG_TEMPO_MAX_WINDOW];
    __shared__ uint32_t s_part[RG_TP_ACF_LANES];
    __shared__ RgTpBest s_best[RG_TP_ACF_LANES];
    const uint32_t tid = threadIdx.x, win = blockIdx.x, ti = win_track[win];
    const RgTpTrack t = tracks[ti];
    const uint32_t w = win - (uint32_t)t.first_win;
    const uint16_t *x = onsets + t.onsets_at + (uint64_t)w * hop;  // w hop + 2W <= K: x[0 .. 2W) are the track's
    for (uint32_t j = tid; j < 2u * RG_TEMPO_MAX_WINDOW; j += RG_TP_ACF_LANES) s_b[j] = j < 2u * W ? x[j] : 0u;
    for (uint32_t i = tid; i < RG_TEMPO_MAX_WINDOW; i += RG_TP_ACF_LANES) s_a[i] = i < W ? x[i] : 0u;
    __syncthreads();
    {  // the prefix sums: eight words per lane, a scan of the 256 partial sums between
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) sum += s_b[8u * tid + q];
        s_part[tid] = sum;
        __syncthreads();
        for (uint32_t off = 1; off < RG_TP_ACF_LANES; off <<= 1) {
            const uint32_t v = tid >= off ? s_part[tid - off] : 0u;
            __syncthreads();
            s_part[tid] += v;
            __syncthreads();
        }
        uint32_t run = tid ? s_part[tid - 1] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            s_p[8u * tid + q] = run;
            run += s_b[8u * tid + q];
        }
        if (tid == RG_TP_ACF_LANES - 1u) s_p[2u * RG_TEMPO_MAX_WINDOW] = run;
    }
    __syncthreads();
    const uint32_t d0 = RG_TP_LAGS_PER_LANE * tid;
    if (d0 < W) {
        const uint32_t W4 = (W + 3u) & ~3u;  // s_a is zero from W on
        uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        uint4 lo = *reinterpret_cast<const uint4 *>(&s_b[d0]);
        for (uint32_t i = 0; i < W4; i += 4) {
            const uint4 a = *reinterpret_cast<const uint4 *>(&s_a[i]);
            const uint4 hi = *reinterpret_cast<const uint4 *>(&s_b[i + d0 + 4u]);  // i + d0 + 7 <= 2 W4 - 1 <= 2047
            r0 += __umul24(a.x, lo.x) + __umul24(a.y, lo.y) + __umul24(a.z, lo.z) + __umul24(a.w, lo.w);
            r1 += __umul24(a.x, lo.y) + __umul24(a.y, lo.z) + __umul24(a.z, lo.w) + __umul24(a.w, hi.x);
            r2 += __umul24(a.x, lo.z) + __umul24(a.y, lo.w) + __umul24(a.z, hi.x) + __umul24(a.w, hi.y);
            r3 += __umul24(a.x, lo.w) + __umul24(a.y, hi.x) + __umul24(a.z, hi.y) + __umul24(a.w, hi.z);
            lo = hi;
        }
        const uint32_t R[RG_TP_LAGS_PER_LANE] = {r0, r1, r2, r3};
        const uint64_t A = s_p[W];
#pragma unroll
        for (uint32_t r = 0; r < RG_TP_LAGS_PER_LANE; ++r) {
            const uint32_t d = d0 + r;
            if (d >= W) continue;
            const uint64_t B = s_p[d + W] - s_p[d];
            const int32_t cw = (int32_t)((int64_t)R[r] - (int64_t)(A * B / W));
            s_c[d] = cw;
            if (cw) atomicAdd(&acf[(uint64_t)ti * W + d], (unsigned long long)(long long)cw);
        }
    }
    __syncthreads();
    RgTpBest best{0, 0u, 0u};
    for (uint32_t p = t.pmax / 2u + 1u + tid; p <= t.pmax; p += RG_TP_ACF_LANES) {
        const RgTpBest cand{rg_tp_score(s_c, p, t.kh), p, 0u};  // (kh p >> 4) + 1 <= W - 1
        if (rg_tp_better(cand, best)) best = cand;
    }
    s_best[tid] = best;
    tp_tree(s_best, tid, [](const RgTpBest &a, const RgTpBest &b) { return rg_tp_better(a, b); });
    if (tid == 0) p16_w[win] = s_best[0].p16;
}

__global__ __launch_bounds__(RG_TP_ACF_LANES) void rg_tp_finish_kernel(const uint16_t *__restrict__ onsets, const RgTpTrack *__restrict__ tracks, uint32_t W,
                                                                       const uint32_t *__restrict__ p16_w, const long long *__restrict__ acf,
                                                                       RgTpFinish *__restrict__ out) {
    __shared__ int64_t s_C[RG_TEMPO_MAX_WINDOW];
    __shared__ RgTpBest s_best[RG_TP_ACF_LANES];
    __shared__ RgTpPhase s_phase[RG_TP_ACF_LANES];
    __shared__ uint32_t s_count[RG_TP_ACF_LANES];
    const uint32_t tid = threadIdx.x;
    const RgTpTrack t = tracks[blockIdx.x];
    const long long *C = acf + (uint64_t)blockIdx.x * W;
    if (!t.windows || !t.kh || C[0] <= 0) {  // the same in every lane
        if (tid == 0) out[blockIdx.x] = RgTpFinish{0u, 0u, 0u, 0u};
        return;
    }
    for (uint32_t d = tid; d < W; d += RG_TP_ACF_LANES) s_C[d] = C[d];
    __syncthreads();
    RgTpBest best{0, 0u, 0u};
    for (uint32_t p = t.pmax / 2u + 1u + tid; p <= t.pmax; p += RG_TP_ACF_LANES) {
        const RgTpBest cand{rg_tp_score(s_C, p, t.kh), p, 0u};
        if (rg_tp_better(cand, best)) best = cand;
    }
    s_best[tid] = best;
    tp_tree(s_best, tid, [](const RgTpBest &a, const RgTpBest &b) { return rg_tp_better(a, b); });
    best = s_best[0];
    uint32_t stable = 0;
    for (uint32_t w = tid; w < t.windows; w += RG_TP_ACF_LANES) stable += rg_tp_window_stable(p16_w[t.first_win + w], best.p16) ? 1u : 0u;
    s_count[tid] = stable;
    __syncthreads();
    for (uint32_t w = RG_TP_ACF_LANES / 2; w; w >>= 1) {
        if (tid < w) s_count[tid] += s_count[tid + w];
        __syncthreads();
    }
    RgTpPhase phase{0u, 0u, 0u};
    const uint16_t *x = onsets + t.onsets_at;
    for (uint32_t phi = tid; phi < best.p16; phi += RG_TP_ACF_LANES) {
        const RgTpPhase cand = rg_tp_phase(x, t.k, best.p16, phi);  // every index is below K
        if (rg_tp_phase_better(cand, phase)) phase = cand;
    }
    s_phase[tid] = phase;
    tp_tree(s_phase, tid, [](const RgTpPhase &a, const RgTpPhase &b) { return rg_tp_phase_better(a, b); });
    if (tid == 0) rg_tp_close(best, s_C[0], t.kh, s_count[0], t.windows, s_phase[0], &out[blockIdx.x]);
}

// ---- stage 1: one call's launches -------------------------------------------------------------------------------------------
template <int FMT>
static hipError_t tp_launch_format(const unsigned char *d_arena, unsigned char *d, const FpJob &job, uint16_t *d_onsets, float *d_bands, hipStream_t s) {
    const uint64_t base = job.fmt_tile[FMT == RG_FMT_F32_PLANAR ? 0 : FMT == RG_FMT_S16_PLANAR ? 1 : 2];
    const uint64_t count = job.fmt_tile[(FMT == RG_FMT_F32_PLANAR ? 0 : FMT == RG_FMT_S16_PLANAR ? 1 : 2) + 1] - base;
    if (!count) return hipSuccess;
    // more than 64 KB of LDS has to be asked for
    const hipError_t e = hipFuncSetAttribute((const void *)rg_tp_tiles_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize, RG_TP_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rg_tp_tiles_kernel<FMT>), dim3((uint32_t)count), dim3(RG_FP_LANES), RG_TP_LDS_BYTES, s, d_arena,
                       reinterpret_cast<const RgSpecTables *>(d), reinterpret_cast<const RgFpTrack *>(d + job.tracks_at),
                       reinterpret_cast<const uint32_t *>(d + job.map_at), base, d_onsets, d_bands, reinterpret_cast<uint32_t *>(d + job.counts_at));
    return hipGetLastError();
}

static int tp_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const FpJob &job, uint16_t *d_onsets, float *d_bands, hipStream_t s) {
    RG_HIP(c, tp_launch_format<RG_FMT_F32_PLANAR>(d_arena, d, job, d_onsets, d_bands, s));
    RG_HIP(c, tp_launch_format<RG_FMT_S16_PLANAR>(d_arena, d, job, d_onsets, d_bands, s));
    RG_HIP(c, tp_launch_format<RG_FMT_S32_PLANAR>(d_arena, d, job, d_onsets, d_bands, s));
    hipLaunchKernelGGL(rg_fp_fold_kernel<1>, dim3((uint32_t)job.n), dim3(256), 0, s, reinterpret_cast<const RgFpTrack *>(d + job.tracks_at),
                       reinterpret_cast<const uint32_t *>(d + job.counts_at), reinterpret_cast<uint32_t *>(d + job.res_at));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_tempo_onsets_device(rg_ctx *c, const unsigned char *d_arena, RgFpTrack *tracks, size_t n, uint16_t *d_onsets, float *d_bands, uint32_t *nonfinite,
                           hipStream_t s) {
    if (!n) return RG_OK;
    uint64_t fmt_tile[4], at = 0;
    for (uint32_t f = 0; f < 3; ++f) {  // the tiles of one format contiguous; codes_at and frames_at are the caller's
        fmt_tile[f] = at;
        for (size_t i = 0; i < n; ++i)
            if (tracks[i].format == f) {
                tracks[i].first_tile = at;
                at += tracks[i].n_tiles;
            }
    }
    fmt_tile[3] = at;
    if (n > 0x7fffffffu || at > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks, %llu tiles", n, (unsigned long long)at);
    FpJob job;
    fp_job(tracks, n, fmt_tile, &job);
    RG_HIP(c, c->d_tempo.reserve(job.end));
    unsigned char *d = c->d_tempo.p;
    RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    const int rc = tp_launch(c, d_arena, d, job, d_onsets, d_bands, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(nonfinite, d + job.res_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- stage 2: one call's launches -------------------------------------------------------------------------------------------
// Device layout of the work buffer, every part 16-byte aligned: [track records | window -> track | P16_w | C | finish records]
struct TpJob {
    std::vector<unsigned char> head;  // the device buffer's bytes [0, pw_at)
    size_t map_at, pw_at, acf_at, fin_at, end, n, windows;
    uint32_t W, hop;
};

// `tracks` have been planned (rg_tp_stage2_plan)
static void tp_job(const RgTpTrack *tracks, size_t n, uint64_t windows, const rg_tempo_opts &o, TpJob *job) {
    job->n = n;
    job->windows = (size_t)windows;
    job->W = o.window;
    job->hop = o.hop;
    job->map_at = fp_a16(n * sizeof(RgTpTrack));
    job->pw_at = fp_a16(job->map_at + (size_t)windows * sizeof(uint32_t));
    job->acf_at = fp_a16(job->pw_at + (size_t)windows * sizeof(uint32_t));
    job->fin_at = fp_a16(job->acf_at + n * (size_t)o.window * sizeof(int64_t));
    job->end = fp_a16(job->fin_at + n * sizeof(RgTpFinish));
    job->head.assign(job->pw_at, 0);
    memcpy(job->head.data(), tracks, n * sizeof(RgTpTrack));
    uint32_t *map = reinterpret_cast<uint32_t *>(job->head.data() + job->map_at);
    for (size_t i = 0; i < n; ++i)
        if (tracks[i].kh)
            for (uint32_t w = 0; w < tracks[i].windows; ++w) map[tracks[i].first_win + w] = (uint32_t)i;
}

static int tp_launch_acf(rg_ctx *c, const uint16_t *d_onsets, unsigned char *d, const TpJob &job, hipStream_t s) {
    RG_HIP(c, hipMemsetAsync(d + job.acf_at, 0, job.n * (size_t)job.W * sizeof(int64_t), s));
    if (!job.windows) return RG_OK;
    hipLaunchKernelGGL(rg_tp_acf_kernel, dim3((uint32_t)job.windows), dim3(RG_TP_ACF_LANES), 0, s, d_onsets, reinterpret_cast<const RgTpTrack *>(d),
                       reinterpret_cast<const uint32_t *>(d + job.map_at), job.W, job.hop, reinterpret_cast<uint32_t *>(d + job.pw_at),
                       reinterpret_cast<unsigned long long *>(d + job.acf_at));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

static int tp_launch_finish(rg_ctx *c, const uint16_t *d_onsets, unsigned char *d, const TpJob &job, hipStream_t s) {
    hipLaunchKernelGGL(rg_tp_finish_kernel, dim3((uint32_t)job.n), dim3(RG_TP_ACF_LANES), 0, s, d_onsets, reinterpret_cast<const RgTpTrack *>(d), job.W,
                       reinterpret_cast<const uint32_t *>(d + job.pw_at), reinterpret_cast<const long long *>(d + job.acf_at),
                       reinterpret_cast<RgTpFinish *>(d + job.fin_at));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_tempo_stage2_device(rg_ctx *c, const uint16_t *d_onsets, RgTpTrack *tracks, size_t n, const rg_tempo_opts &o, RgTpFinish *finish, int64_t *acf,
                           hipStream_t s) {
    if (!n) return RG_OK;
    const uint64_t windows = rg_tp_stage2_plan(tracks, n);
    if (n > 0x7fffffffu || windows > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks, %llu windows", n, (unsigned long long)windows);
    TpJob job;
    tp_job(tracks, n, windows, o, &job);
    RG_HIP(c, c->d_tempo.reserve(job.end));
    unsigned char *d = c->d_tempo.p;
    RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    int rc = tp_launch_acf(c, d_onsets, d, job, s);
    if (rc == RG_OK) rc = tp_launch_finish(c, d_onsets, d, job, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(finish, d + job.fin_at, n * sizeof(RgTpFinish), hipMemcpyDeviceToHost, s));
    if (acf) RG_HIP(c, hipMemcpyAsync(acf, d + job.acf_at, n * (size_t)o.window * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seams (include/mp3rgain_amd_tempo.h) -------------------------------------------------------------------------------
extern "C" int rg_tempo_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_tempo_opts *opts,
                              rg_tempo_result *out, uint16_t *onsets_out, float *bands_out) {
    std::vector<RgFpTrack> tracks;
    rg_tempo_opts o;
    uint64_t n_onsets = 0, n_frames = 0;
    const auto host = [&](char *err, size_t err_len) {
        const int rc = rg_tp_options(opts, &o, err, err_len);
        return rc != RG_OK ? rc : rg_tp_arena_host(route, n, descs, arena, arena_bytes, o, out, onsets_out, bands_out, err, err_len);
    };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_tp_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        tracks = std::vector<RgFpTrack>(n + 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_tp_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        uint64_t fmt_tile[4];
        (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
        for (size_t i = 0; i < n; ++i) {
            n_onsets += tracks[i].frames ? tracks[i].frames - 1u : 0u;
            n_frames += tracks[i].frames;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        // the onsets, then the band energies when they are asked for
        const size_t bands_at = ((size_t)n_onsets + 7) & ~(size_t)7, halves = bands_at + (bands_out ? (size_t)n_frames * RG_TEMPO_BANDS * 2 : 0);
        RG_HIP(c, c->d_tp_onsets.reserve(halves + 8));
        uint16_t *d_onsets = c->d_tp_onsets.p;
        float *d_bands = bands_out ? reinterpret_cast<float *>(d_onsets + bands_at) : nullptr;
        std::vector<uint32_t> nonfinite(n ? n : 1);
        int rc = rg_tempo_onsets_device(c, c->d_arena.p, tracks.data(), n, d_onsets, d_bands, nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        std::vector<RgTpTrack> s2(n + 1);
        std::vector<RgTpFinish> fin(n + 1);
        for (size_t i = 0; i < n; ++i) {
            rg_tp_stage2_track(descs[i].sample_rate, tracks[i].frames ? tracks[i].frames - 1u : 0u, o, &s2[i]);
            s2[i].onsets_at = tracks[i].codes_at;
        }
        rc = rg_tempo_stage2_device(c, d_onsets, s2.data(), n, o, fin.data(), nullptr, s);
        if (rc != RG_OK) return rc;
        if (onsets_out && n_onsets) RG_HIP(c, hipMemcpyAsync(onsets_out, d_onsets, (size_t)n_onsets * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
        if (bands_out && n_frames) RG_HIP(c, hipMemcpyAsync(bands_out, d_bands, (size_t)n_frames * RG_TEMPO_BANDS * sizeof(float), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i)
            rg_tp_fill(&descs[i], descs[i].sample_rate, tracks[i].frames, s2[i], fin[i], 0, nonfinite[i], tracks[i].codes_at, &out[i]);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_tempo_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

extern "C" int rg_tempo_from_onsets(void *ctx, int route, size_t n, const uint32_t *counts, const uint32_t *rates, const uint16_t *onsets,
                                    const rg_tempo_opts *opts, rg_tempo_result *out, int64_t *acf_out) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    char err[256] = "";
    if (!c && route == 1) return RG_ERR_INVALID_ARG;
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_from_onsets: route %d (0 = serial host twin, 1 = kernels)", route);
    if (n && (!counts || !rates || !out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_from_onsets: null array");
    rg_tempo_opts o;
    int rc = rg_tp_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    try {
        uint64_t total = 0;
        for (size_t i = 0; i < n; ++i) total += counts[i];
        if (total && !onsets) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_from_onsets: null array");
        rc = rg_tp_from_onsets_check(n, counts, onsets, err, sizeof err);
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
        if (route == 0) return rg_tp_from_onsets_host(n, counts, rates, onsets, o, out, acf_out);
        if (!n) return RG_OK;
        std::vector<RgTpTrack> s2(n);
        std::vector<RgTpFinish> fin(n);
        uint64_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_tp_stage2_track(rates[i], counts[i], o, &s2[i]);
            s2[i].onsets_at = at;
            at += counts[i];
        }
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        RG_HIP(c, c->d_tp_onsets.reserve((size_t)total + 8));
        if (total) RG_HIP(c, hipMemcpyAsync(c->d_tp_onsets.p, onsets, (size_t)total * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        rc = rg_tempo_stage2_device(c, c->d_tp_onsets.p, s2.data(), n, o, fin.data(), acf_out, s);
        RG_HIP(c, hipStreamSynchronize(s));
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) rg_tp_fill(nullptr, rates[i], 0, s2[i], fin[i], 0, 0, s2[i].onsets_at, &out[i]);
        return RG_OK;
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

// ---- measurement hook (tools/tempo_rate.py) ----------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per word: word w <- a mix of its index (as rg_fprint.hip fills its arena)
__global__ __launch_bounds__(256) void rg_tp_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}
// the read-only pass the onset stage is compared with: every 16-byte word of the planes once, one sum per workgroup
__global__ __launch_bounds__(256) void rg_tp_read_kernel(const uint4 *__restrict__ src, uint64_t words, uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_sum[256];
    uint32_t sum = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        const uint4 v = src[w];
        sum += v.x ^ v.y ^ v.z ^ v.w;
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t k = 128; k; k >>= 1) {
        if (threadIdx.x < k) s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = s_sum[0];
}

extern "C" int rg_tempo_rate(void *ctx, size_t n, uint64_t frames, const rg_tempo_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                             double warm_ms, double *onset_ms, double *read_ms, double *acf_ms, double *finish_ms, double *host_onset_ms,
                             double *host_finish_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || n > 65535 || !frames || frames >= ((uint64_t)1 << 32) || !reps || !onset_ms || !read_ms || !acf_ms || !finish_ms ||
        (host_tracks && (!host_onset_ms || !host_finish_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_rate: bad arguments");
    rg_tempo_opts o;
    char err[256] = "";
    int rc = rg_tp_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 2 * 2, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d1 = nullptr, *d2 = nullptr;
    uint16_t *d_onsets = nullptr;
    uint32_t *d_sums = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgFpTrack> tracks(n);
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)RG_FMT_S16_PLANAR;
            if (rg_tp_track(i, t, total, &tracks[i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_rate: %s", err);
        }
        uint64_t fmt_tile[4];
        (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
        FpJob job;
        fp_job(tracks.data(), n, fmt_tile, &job);
        const uint32_t k = tracks[0].frames ? tracks[0].frames - 1u : 0u;
        std::vector<RgTpTrack> s2(n);
        for (size_t i = 0; i < n; ++i) {
            rg_tp_stage2_track(44100u, k, o, &s2[i]);
            s2[i].onsets_at = tracks[i].codes_at;
        }
        const uint64_t windows = rg_tp_stage2_plan(s2.data(), n);
        if (windows > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_tempo_rate: %llu windows", (unsigned long long)windows);
        TpJob job2;
        tp_job(s2.data(), n, windows, o, &job2);
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d1, job.end));
        RG_HIP(c, hipMalloc((void **)&d2, job2.end));
        RG_HIP(c, hipMalloc((void **)&d_onsets, ((size_t)k * n + 8) * sizeof(uint16_t)));
        RG_HIP(c, hipMalloc((void **)&d_sums, 4096 * sizeof(uint32_t)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_tp_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d1, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemcpyAsync(d2, job2.head.data(), job2.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<uint16_t> host_onsets((size_t)k * host_tracks + 1);
        std::vector<RgTpFinish> host_fin(host_tracks + 1), dev_fin(n);
        const auto pool_run = [&](size_t items, auto fn) {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < items; i = next.fetch_add(1)) fn(i);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        enum { kOnset, kRead, kAcf, kFinish, kStages };
        const auto launch = [&](int what) -> int {
            if (what == kOnset) return tp_launch(c, d_arena, d1, job, d_onsets, nullptr, s);
            if (what == kRead) {
                hipLaunchKernelGGL(rg_tp_read_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<const uint4 *>(d_arena), (uint64_t)(total / 16), d_sums);
                RG_HIP(c, hipGetLastError());
                return RG_OK;
            }
            if (what == kAcf) return tp_launch_acf(c, d_onsets, d2, job2, s);
            return tp_launch_finish(c, d_onsets, d2, job2, s);
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            for (int what = kOnset; what < kStages; ++what) {
                const int lr = launch(what);
                if (lr != RG_OK) return lr;
            }
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            double *const dst[kStages] = {onset_ms, read_ms, acf_ms, finish_ms};
            for (int what = kOnset; what < kStages; ++what) {  // the four alternate within a round
                float ms = 0.0f;
                RG_HIP(c, hipEventRecord(e0, s));
                const int lr = launch(what);
                if (lr != RG_OK) return lr;
                RG_HIP(c, hipEventRecord(e1, s));
                RG_HIP(c, hipStreamSynchronize(s));
                RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
                dst[what][r] = ms;
            }
            if (host_tracks) {
                auto t0 = std::chrono::steady_clock::now();
                pool_run(host_tracks, [&](size_t i) { (void)rg_tp_folded_host(h.data(), tracks[i], host_onsets.data() + tracks[i].codes_at, nullptr); });
                host_onset_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                t0 = std::chrono::steady_clock::now();
                pool_run(host_tracks, [&](size_t i) { rg_tp_stage2_host(host_onsets.data(), s2[i], o, &host_fin[i], nullptr); });
                host_finish_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            std::vector<uint16_t> dev_onsets((size_t)k * host_tracks + 1);
            RG_HIP(c, hipMemcpy(dev_onsets.data(), d_onsets, (size_t)k * host_tracks * sizeof(uint16_t), hipMemcpyDeviceToHost));
            RG_HIP(c, hipMemcpy(dev_fin.data(), d2 + job2.fin_at, n * sizeof(RgTpFinish), hipMemcpyDeviceToHost));
            *mismatches = 0;
            for (size_t i = 0; i < (size_t)k * host_tracks; ++i) *mismatches += dev_onsets[i] != host_onsets[i];
            for (size_t i = 0; i < host_tracks; ++i) *mismatches += memcmp(&dev_fin[i], &host_fin[i], sizeof(RgTpFinish)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_tempo_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_sums) (void)hipFree(d_sums);
    if (d_onsets) (void)hipFree(d_onsets);
    if (d2) (void)hipFree(d2);
    if (d1) (void)hipFree(d1);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
