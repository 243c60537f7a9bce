// rg_key.hip -- the key scan on the device (include/mp3rgain_amd_key.h, rg_key.h): per track the signal decimated to 5 .. 10 kHz,
// a chroma row of twelve integers per 512 decimated samples, and the all-integer match against the key profiles.
//
//   rg_key_decimate_kernel  stage 1a, the hot path: one workgroup of 256 lanes per run of 256 consecutive outputs of one track,
//                           many tracks per launch, one launch per format.  The run's (255 + 16) D + 1 input frames are read from
//                           the arena once, consecutive lanes reading consecutive samples of a plane (each lane only its own
//                           sample: nothing outside the plane is touched, whatever its alignment), down-mixed and staged in LDS
//                           polyphase-transposed, [k mod D][k / D]: lane j then reads x[j D + k] at column j + k / D of row
//                           k mod D, consecutive lanes consecutive words, instead of words D apart (an 8-way bank conflict at
//                           D = 8).  Every lane sums its output in ascending k; the taps are the same for every lane and come
//                           through scalar loads.
//   rg_key_tiles_kernel     stage 1b: the fingerprint's tile walk (rg_fprint_tile.h) over the decimated buffer as an arena of
//                           mono f32 tracks, 60 bands whose edges come from the key track's record; one lane per frame the tile
//                           owns turns its 60 energies into the row (rg_key_row).  72 KB of LDS.
//   rg_key_finish_kernel    stage 2, one workgroup per track: lanes sum rows into H (a tree in LDS: integers, so any order), 24
//                           lanes score the keys, lane 0 closes with the host's total order; then lanes own segments.
// No float after the rows; this unit is compiled without contraction: same input, same bytes as the host twins.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_fprint_tile.h"
#include "rg_key.h"
#include "rg_pcm_seam.h"

// where a stage-2 launch finds a track's rows
struct KeyRows {
    uint64_t rows_at;
    uint32_t rows, reserved;
};

#define KEY_STAGE_LOADS 5u  // at D = 8 a run is 2169 samples: two rounds of 5 x 256

// sample k of a plane as the stored pattern, S16 sign-extended (what rg_spec_value takes)
template <int FMT>
__device__ __forceinline__ uint32_t key_raw(const unsigned char *plane, uint32_t k) {
    if (FMT == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(plane)[k];
    return reinterpret_cast<const uint32_t *>(plane)[k];
}

template <int FMT>
__global__ __launch_bounds__(RG_KEY_DECIM_LANES) void rg_key_decimate_kernel(const unsigned char *__restrict__ arena, const RgKeyTrack *__restrict__ tracks,
                                                                             const uint64_t *__restrict__ run_first, const uint32_t *__restrict__ run_track,
                                                                             uint32_t n_runs, uint64_t wg_base, const float *__restrict__ taps,
                                                                             float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = wg_base + blockIdx.x;
    uint32_t lo = 0, hi = n_runs;  // the last run that starts at or before this workgroup: the same in every lane
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (run_first[mid] <= wg) lo = mid; else hi = mid;
    }
    const RgKeyTrack &p = tracks[run_track[lo]];
    const uint32_t D = p.decim, j0 = (uint32_t)(wg - p.first_wg) * RG_KEY_DECIM_OUTPUTS;
    const uint32_t left = p.m - j0, no = left < RG_KEY_DECIM_OUTPUTS ? left : RG_KEY_DECIM_OUTPUTS;  // j0 < M
    const unsigned char *p0 = arena + p.off0, *p1 = arena + p.off1;
    const bool two = p.channels >= 2;
    float *out = y + p.y_at + j0;
    if (D == 1u) {  // y = x
        if (tid < no) {
            const float a = fp_load<FMT>(p0, (uint64_t)j0 + tid);
            out[tid] = two ? (a + fp_load<FMT>(p1, (uint64_t)j0 + tid)) * 0.5f : a;
        }
        return;
    }
    // (j0 + no - 1) D + 16 D <= (M - 1) D + 16 D < N: every sample read is the track's
    const uint32_t count = (no - 1u) * D + RG_KEY_TAPS_PER_DECIM * D + 1u, recip = p.recip;
    const uint64_t base = (uint64_t)j0 * D * (FMT == RG_FMT_S16_PLANAR ? 2u : 4u);
    const unsigned char *q0 = p0 + base, *q1 = p1 + base;  // the run's first sample in each plane: the same in every lane
    // KEY_STAGE_LOADS samples of each plane per lane are asked for before the first is waited for: one at a time, the run's
    // nine rounds of two dependent loads were most of the kernel's time
    for (uint32_t i0 = tid; i0 < count; i0 += KEY_STAGE_LOADS * RG_KEY_DECIM_LANES) {
        uint32_t ra[KEY_STAGE_LOADS], rb[KEY_STAGE_LOADS];
#pragma unroll
        for (uint32_t u = 0; u < KEY_STAGE_LOADS; ++u) {
            // without a branch, or each load would be waited for in a block of its own: beyond the run, its last sample
            // again; of a single channel, p1 is p0
            const uint32_t i = i0 + u * RG_KEY_DECIM_LANES, ic = i < count ? i : count - 1u;
            ra[u] = key_raw<FMT>(q0, ic);
            rb[u] = key_raw<FMT>(q1, ic);
        }
#pragma unroll
        for (uint32_t u = 0; u < KEY_STAGE_LOADS; ++u) {
            const uint32_t i = i0 + u * RG_KEY_DECIM_LANES, ic = i < count ? i : count - 1u;  // (beyond the run: the last sample's place, its value)
            const float a = rg_spec_value<FMT>(ra[u]);
            const uint32_t col = __umulhi(ic, recip), row = ic - col * D;  // i / D, i mod D (i D < 2^32)
            s_x[row * RG_KEY_DECIM_COLS + col] = two ? (a + rg_spec_value<FMT>(rb[u])) * 0.5f : a;
        }
    }
    __syncthreads();
    if (tid < no) {
        const float *h = taps + p.taps_at, *x = s_x + tid;
        float s = 0.0f;
        for (uint32_t q = 0; q < RG_KEY_TAPS_PER_DECIM; ++q) {
            const float *xq = x + q;
            for (uint32_t r = 0; r < D; ++r) {
                const float prod = h[r] * xq[r * RG_KEY_DECIM_COLS];
                s += prod;
            }
            h += D;
        }
        const float prod = h[0] * x[RG_KEY_TAPS_PER_DECIM];
        s += prod;
        out[tid] = s;
    }
}

__global__ __launch_bounds__(RG_FP_LANES) void rg_key_tiles_kernel(const unsigned char *__restrict__ ybuf, const RgSpecTables *__restrict__ tables,
                                                                   const RgFpTrack *__restrict__ fp_tracks, const RgKeyTrack *__restrict__ tracks,
                                                                   const uint32_t *__restrict__ tile_track, uint16_t *__restrict__ rows,
                                                                   float *__restrict__ bands, uint32_t *__restrict__ tile_nonfinite) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const float *s_E = rg_fp_tile_rows(s_raw);
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, ti = tile_track[tile];
    const RgFpTrack &p = fp_tracks[ti];
    const uint32_t t = (uint32_t)(tile - p.first_tile), f0 = t * RG_KEY_TILE_ROWS, first = t ? 1u : 0u;
    uint32_t nonfinite;
    const uint32_t nf = rg_fp_tile_bands<RG_FMT_F32_PLANAR, RG_KEY_BANDS>(ybuf, tables, p, t, s_raw, &nonfinite, tracks[ti].e);
    // a tile owns every frame but its first; tile 0 owns that too.  f0 + tid < f0 + nf <= F
    if (tid >= first && tid < nf) rg_key_row(s_E + tid * RG_KEY_BANDS, rows + (p.frames_at + f0 + tid) * RG_KEY_CHROMA);
    if (bands) {
        float *dst = bands + (p.frames_at + f0) * RG_KEY_BANDS;
        for (uint32_t k = tid + first * RG_KEY_BANDS; k < nf * RG_KEY_BANDS; k += RG_FP_LANES) dst[k] = s_E[k];
    }
    if (tid == 0) tile_nonfinite[tile] = nonfinite;
}

// the sum of s[0 .. 256) to s[0]; every lane calls it, s[tid] written before
template <class T>
__device__ __forceinline__ void key_tree_sum(T *s, uint32_t tid) {
    __syncthreads();
    for (uint32_t w = RG_KEY_FINISH_LANES / 2; w; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
}

__global__ __launch_bounds__(RG_KEY_FINISH_LANES) void rg_key_finish_kernel(const uint16_t *__restrict__ rows, const KeyRows *__restrict__ tracks, uint32_t S,
                                                                            RgKeyFinish *__restrict__ out) {
    __shared__ uint64_t s_red[RG_KEY_FINISH_LANES];
    __shared__ uint32_t s_count[RG_KEY_FINISH_LANES];
    __shared__ uint64_t s_H[12];
    __shared__ uint32_t s_h[12];
    __shared__ int64_t s_score[24];
    __shared__ RgKeyPick s_pick;
    __shared__ uint32_t s_silent;
    const uint32_t tid = threadIdx.x;
    const KeyRows t = tracks[blockIdx.x];
    const uint16_t *r = rows + t.rows_at * RG_KEY_CHROMA;
    uint64_t H[12];
    uint32_t silent = 0;
    for (uint32_t p = 0; p < 12; ++p) H[p] = 0;
    for (uint32_t n = tid; n < t.rows; n += RG_KEY_FINISH_LANES) {
        const uint16_t *row = r + (uint64_t)n * RG_KEY_CHROMA;
        for (uint32_t p = 0; p < 12; ++p) H[p] += row[p];
        silent += rg_key_row_silent(row) ? 1u : 0u;
    }
    for (uint32_t p = 0; p < 12; ++p) {
        s_red[tid] = H[p];
        key_tree_sum(s_red, tid);
        if (tid == 0) s_H[p] = s_red[0];
        __syncthreads();
    }
    s_count[tid] = silent;
    key_tree_sum(s_count, tid);
    if (tid == 0) {
        s_silent = s_count[0];
        rg_key_scale(s_H, s_h);
    }
    __syncthreads();
    if (tid < 24) s_score[tid] = rg_key_score(s_h, tid);
    __syncthreads();
    if (tid == 0) rg_key_close(s_h, s_score, &s_pick);
    __syncthreads();
    const RgKeyPick pick = s_pick;
    const uint32_t G = t.rows / S;
    uint32_t nonzero = 0, agreeing = 0;
    for (uint32_t g = tid; g < G; g += RG_KEY_FINISH_LANES) {  // (g + 1) S <= F: every row read is the track's
        uint64_t Hg[12];
        if (!rg_key_segment_sums(r, g, S, Hg)) continue;
        RgKeyPick sp;
        rg_key_pick(Hg, &sp);
        ++nonzero;
        agreeing += !sp.none && sp.key == pick.key ? 1u : 0u;
    }
    s_red[tid] = ((uint64_t)nonzero << 32) | agreeing;  // both below 2^23
    key_tree_sum(s_red, tid);
    if (tid == 0) rg_key_finish(pick, s_silent, G, (uint32_t)(s_red[0] >> 32), (uint32_t)s_red[0], &out[blockIdx.x]);
}

// ---- one call's launches -----------------------------------------------------------------------------------------------------
// Device layout of the work buffer, every part 16-byte aligned: the tile walk's job (rg_fprint_tile.h) over the decimated
// signals, then [key track records | run starts | run -> track | taps | rows records | finish records]
struct KeyJob {
    FpJob fp;
    std::vector<unsigned char> head;  // the device buffer's bytes [fp.end, fin_at)
    uint64_t fmt_wg[4];
    size_t tracks_at, first_at, run_at, taps_at, rows_at, fin_at, end, n, n_runs;
    uint64_t y_floats, rows;
    uint32_t max_decim, segment;
};

// tracks: rg_key_track'ed; they are planned here
static int key_job(rg_ctx *c, RgKeyTrack *tracks, size_t n, const rg_key_opts &o, KeyJob *job) {
    std::vector<float> taps;
    job->n = n;
    job->segment = o.segment;
    job->y_floats = rg_key_plan(tracks, n, job->fmt_wg, &taps, &job->rows);
    std::vector<RgFpTrack> fp(n + 1);
    uint64_t tiles = 0;
    job->max_decim = 1;
    std::vector<uint64_t> first;
    std::vector<uint32_t> run;
    for (size_t i = 0; i < n; ++i) {
        rg_key_fp_track(tracks[i], tracks[i].y_at * sizeof(float), &fp[i]);
        fp[i].first_tile = tiles;
        fp[i].frames_at = tracks[i].rows_at;
        tiles += fp[i].n_tiles;
        job->max_decim = std::max(job->max_decim, tracks[i].decim);
    }
    for (uint32_t f = 0; f < 3; ++f)  // the runs in the order of their workgroups
        for (size_t i = 0; i < n; ++i)
            if (tracks[i].format == f && tracks[i].n_wg) {
                first.push_back(tracks[i].first_wg);
                run.push_back((uint32_t)i);
            }
    if (n > 0x7fffffffu || tiles > 0x7fffffffu || job->fmt_wg[3] > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks, %llu tiles, %llu decimation workgroups", n, (unsigned long long)tiles,
                          (unsigned long long)job->fmt_wg[3]);
    const uint64_t fmt_tile[4] = {0, tiles, tiles, tiles};  // every decimated signal is f32
    fp_job(fp.data(), n, fmt_tile, &job->fp);
    job->n_runs = run.size();
    job->tracks_at = job->fp.end;
    job->first_at = fp_a16(job->tracks_at + n * sizeof(RgKeyTrack));
    job->run_at = fp_a16(job->first_at + first.size() * sizeof(uint64_t));
    job->taps_at = fp_a16(job->run_at + run.size() * sizeof(uint32_t));
    job->rows_at = fp_a16(job->taps_at + taps.size() * sizeof(float));
    job->fin_at = fp_a16(job->rows_at + n * sizeof(KeyRows));
    job->end = fp_a16(job->fin_at + n * sizeof(RgKeyFinish));
    job->head.assign(job->fin_at - job->tracks_at, 0);
    const auto at = [&](size_t off) { return job->head.data() + (off - job->tracks_at); };
    memcpy(at(job->tracks_at), tracks, n * sizeof(RgKeyTrack));
    if (!first.empty()) memcpy(at(job->first_at), first.data(), first.size() * sizeof(uint64_t));
    if (!run.empty()) memcpy(at(job->run_at), run.data(), run.size() * sizeof(uint32_t));
    if (!taps.empty()) memcpy(at(job->taps_at), taps.data(), taps.size() * sizeof(float));
    KeyRows *kr = reinterpret_cast<KeyRows *>(at(job->rows_at));
    for (size_t i = 0; i < n; ++i) kr[i] = KeyRows{tracks[i].rows_at, tracks[i].rows, 0u};
    return RG_OK;
}

template <int FMT>
static hipError_t key_launch_decim_format(const unsigned char *d_arena, unsigned char *d, const KeyJob &job, float *d_y, hipStream_t s) {
    const uint64_t base = job.fmt_wg[FMT], count = job.fmt_wg[FMT + 1] - base;
    if (!count) return hipSuccess;
    const uint32_t lds = job.max_decim * RG_KEY_DECIM_COLS * (uint32_t)sizeof(float);  // at most 87 KB: more than 64 KB has to be asked for
    const hipError_t e = hipFuncSetAttribute((const void *)rg_key_decimate_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             RG_KEY_MAX_DECIM * RG_KEY_DECIM_COLS * (uint32_t)sizeof(float));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rg_key_decimate_kernel<FMT>), dim3((uint32_t)count), dim3(RG_KEY_DECIM_LANES), lds, s, d_arena,
                       reinterpret_cast<const RgKeyTrack *>(d + job.tracks_at), reinterpret_cast<const uint64_t *>(d + job.first_at),
                       reinterpret_cast<const uint32_t *>(d + job.run_at), (uint32_t)job.n_runs, base, reinterpret_cast<const float *>(d + job.taps_at), d_y);
    return hipGetLastError();
}

static int key_launch_decim(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const KeyJob &job, float *d_y, hipStream_t s) {
    static_assert(RG_FMT_F32_PLANAR == 0 && RG_FMT_S16_PLANAR == 1 && RG_FMT_S32_PLANAR == 2, "fmt_wg is indexed by the format");
    RG_HIP(c, key_launch_decim_format<RG_FMT_F32_PLANAR>(d_arena, d, job, d_y, s));
    RG_HIP(c, key_launch_decim_format<RG_FMT_S16_PLANAR>(d_arena, d, job, d_y, s));
    RG_HIP(c, key_launch_decim_format<RG_FMT_S32_PLANAR>(d_arena, d, job, d_y, s));
    return RG_OK;
}

static int key_launch_tiles(rg_ctx *c, unsigned char *d, const KeyJob &job, const float *d_y, uint16_t *d_rows, float *d_bands, hipStream_t s) {
    const uint64_t tiles = job.fp.fmt_tile[3];
    if (tiles) {
        RG_HIP(c, hipFuncSetAttribute((const void *)rg_key_tiles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RG_KEY_TILE_LDS_BYTES));
        hipLaunchKernelGGL(rg_key_tiles_kernel, dim3((uint32_t)tiles), dim3(RG_FP_LANES), RG_KEY_TILE_LDS_BYTES, s, reinterpret_cast<const unsigned char *>(d_y),
                           reinterpret_cast<const RgSpecTables *>(d), reinterpret_cast<const RgFpTrack *>(d + job.fp.tracks_at),
                           reinterpret_cast<const RgKeyTrack *>(d + job.tracks_at), reinterpret_cast<const uint32_t *>(d + job.fp.map_at), d_rows, d_bands,
                           reinterpret_cast<uint32_t *>(d + job.fp.counts_at));
        RG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(rg_fp_fold_kernel<2>, dim3((uint32_t)job.n), dim3(256), 0, s, reinterpret_cast<const RgFpTrack *>(d + job.fp.tracks_at),
                       reinterpret_cast<const uint32_t *>(d + job.fp.counts_at), reinterpret_cast<uint32_t *>(d + job.fp.res_at));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

static int key_launch_finish(rg_ctx *c, const uint16_t *d_rows, const KeyRows *d_recs, size_t n, uint32_t segment, RgKeyFinish *d_fin, hipStream_t s) {
    hipLaunchKernelGGL(rg_key_finish_kernel, dim3((uint32_t)n), dim3(RG_KEY_FINISH_LANES), 0, s, d_rows, d_recs, segment, d_fin);
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

static_assert(RG_KEY_TILE_LDS_BYTES == RG_FP_TILE_LDS(RG_KEY_BANDS), "rg_key_kernel_shape tells the tile kernel's LDS");

int rg_key_device(rg_ctx *c, const unsigned char *d_arena, RgKeyTrack *tracks, size_t n, const rg_key_opts &o, bool want_bands, RgKeyFinish *finish,
                  uint32_t *nonfinite, hipStream_t s) {
    if (!n) return RG_OK;
    KeyJob job;
    int rc = key_job(c, tracks, n, o, &job);
    if (rc != RG_OK) return rc;
    const size_t bands_at = (size_t)job.y_floats;
    RG_HIP(c, c->d_key.reserve(job.end));
    RG_HIP(c, c->d_key_decim.reserve(bands_at + (want_bands ? (size_t)job.rows * RG_KEY_BANDS : 0) + 16));
    RG_HIP(c, c->d_key_rows.reserve((size_t)job.rows * RG_KEY_CHROMA + 16));
    unsigned char *d = c->d_key.p;
    float *d_y = c->d_key_decim.p;
    RG_HIP(c, hipMemcpyAsync(d, job.fp.head.data(), job.fp.head.size(), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipMemcpyAsync(d + job.tracks_at, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    rc = key_launch_decim(c, d_arena, d, job, d_y, s);
    if (rc == RG_OK) rc = key_launch_tiles(c, d, job, d_y, c->d_key_rows.p, want_bands ? d_y + bands_at : nullptr, s);
    if (rc == RG_OK)
        rc = key_launch_finish(c, c->d_key_rows.p, reinterpret_cast<const KeyRows *>(d + job.rows_at), n, job.segment, reinterpret_cast<RgKeyFinish *>(d + job.fin_at), s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (the heads are on their way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(finish, d + job.fin_at, n * sizeof(RgKeyFinish), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipMemcpyAsync(nonfinite, d + job.fp.res_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- stage 1a alone: the L = 1 path of the rational resampler (rg_resample.hip) ------------------------------------------------
struct RgKeyDecimJob : KeyJob {};

int rg_key_decimate_prepare(rg_ctx *c, RgKeyTrack *tracks, const uint64_t *y_at, size_t n, hipStream_t s, RgKeyDecimJob **out) {
    *out = nullptr;
    std::unique_ptr<RgKeyDecimJob> owner(new RgKeyDecimJob);
    RgKeyDecimJob &job = *owner;
    std::vector<float> taps;
    std::vector<uint64_t> first;
    std::vector<uint32_t> run;
    (void)rg_key_plan(tracks, n, job.fmt_wg, &taps, &job.rows);
    job.max_decim = 1;
    for (size_t i = 0; i < n; ++i) {
        tracks[i].y_at = y_at[i];
        job.max_decim = std::max(job.max_decim, tracks[i].decim);
    }
    for (uint32_t f = 0; f < 3; ++f)  // the runs in the order of their workgroups
        for (size_t i = 0; i < n; ++i)
            if (tracks[i].format == f && tracks[i].n_wg) {
                first.push_back(tracks[i].first_wg);
                run.push_back((uint32_t)i);
            }
    if (n > 0x7fffffffu || job.fmt_wg[3] > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks, %llu decimation workgroups", n, (unsigned long long)job.fmt_wg[3]);
    if (run.empty()) return RG_OK;  // nothing to launch: *out stays NULL
    job.n = n;
    job.n_runs = run.size();
    job.tracks_at = 0;
    job.first_at = fp_a16(n * sizeof(RgKeyTrack));
    job.run_at = fp_a16(job.first_at + first.size() * sizeof(uint64_t));
    job.taps_at = fp_a16(job.run_at + run.size() * sizeof(uint32_t));
    job.end = fp_a16(job.taps_at + taps.size() * sizeof(float));
    job.head.assign(job.end, 0);
    memcpy(job.head.data(), tracks, n * sizeof(RgKeyTrack));
    memcpy(job.head.data() + job.first_at, first.data(), first.size() * sizeof(uint64_t));
    memcpy(job.head.data() + job.run_at, run.data(), run.size() * sizeof(uint32_t));
    if (!taps.empty()) memcpy(job.head.data() + job.taps_at, taps.data(), taps.size() * sizeof(float));
    RG_HIP(c, c->d_key.reserve(job.end));
    RG_HIP(c, hipMemcpyAsync(c->d_key.p, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipStreamSynchronize(s));
    *out = owner.release();
    return RG_OK;
}

int rg_key_decimate_launch(rg_ctx *c, const unsigned char *d_arena, const RgKeyDecimJob *job, float *d_y, hipStream_t s) {
    return job ? key_launch_decim(c, d_arena, c->d_key.p, *job, d_y, s) : RG_OK;
}

void rg_key_decimate_free(RgKeyDecimJob *job) { delete job; }

// ---- test seams (include/mp3rgain_amd_key.h) ---------------------------------------------------------------------------------
extern "C" int rg_key_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_key_opts *opts,
                            rg_key_result *out, float *decim_out, float *bands_out, uint16_t *chroma_out) {
    std::vector<RgKeyTrack> tracks;
    rg_key_opts o;
    const auto host = [&](char *err, size_t err_len) {
        const int rc = rg_key_options(opts, &o, err, err_len);
        return rc != RG_OK ? rc : rg_key_arena_host(route, n, descs, arena, arena_bytes, o, out, decim_out, bands_out, chroma_out, err, err_len);
    };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_key_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        tracks = std::vector<RgKeyTrack>(n + 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_key_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        if (!n) return RG_OK;
        std::vector<uint32_t> nonfinite(n);
        std::vector<RgKeyFinish> fin(n);
        const int rc = rg_key_device(c, c->d_arena.p, tracks.data(), n, o, bands_out != nullptr, fin.data(), nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        uint64_t y_out = 0, y_end = 0, rows = 0;
        for (size_t i = 0; i < n; ++i) {
            const RgKeyTrack &t = tracks[i];
            if (decim_out && t.m) RG_HIP(c, hipMemcpyAsync(decim_out + y_out, c->d_key_decim.p + t.y_at, (size_t)t.m * sizeof(float), hipMemcpyDeviceToHost, s));
            y_out += t.m;
            y_end = t.y_at + (((uint64_t)t.m + 3u) & ~(uint64_t)3);
            rows += t.rows;
        }
        if (chroma_out && rows) RG_HIP(c, hipMemcpyAsync(chroma_out, c->d_key_rows.p, (size_t)rows * RG_KEY_CHROMA * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
        if (bands_out && rows)
            RG_HIP(c, hipMemcpyAsync(bands_out, c->d_key_decim.p + y_end, (size_t)rows * RG_KEY_BANDS * sizeof(float), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) rg_key_fill(&descs[i], &tracks[i], tracks[i].rows, fin[i], 0, nonfinite[i], tracks[i].rows_at, &out[i]);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_key_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

extern "C" int rg_key_from_chroma(void *ctx, int route, size_t n, const uint32_t *counts, const uint16_t *chroma, const rg_key_opts *opts, rg_key_result *out) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    char err[256] = "";
    if (!c && route == 1) return RG_ERR_INVALID_ARG;
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_key_from_chroma: route %d (0 = serial host twin, 1 = kernels)", route);
    if (n && (!counts || !out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_key_from_chroma: null array");
    rg_key_opts o;
    int rc = rg_key_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    try {
        uint64_t total = 0;
        for (size_t i = 0; i < n; ++i) total += counts[i];
        if (total && !chroma) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_key_from_chroma: null array");
        rc = rg_key_from_chroma_check(n, counts, chroma, err, sizeof err);
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
        if (route == 0) return rg_key_from_chroma_host(n, counts, chroma, o, out);
        if (!n) return RG_OK;
        if (n > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks", n);
        std::vector<KeyRows> recs(n);
        std::vector<RgKeyFinish> fin(n);
        uint64_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            recs[i] = KeyRows{at, counts[i], 0u};
            at += counts[i];
        }
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        const size_t fin_at = fp_a16(n * sizeof(KeyRows));
        RG_HIP(c, c->d_key.reserve(fin_at + n * sizeof(RgKeyFinish)));
        RG_HIP(c, c->d_key_rows.reserve((size_t)total * RG_KEY_CHROMA + 16));
        RG_HIP(c, hipMemcpyAsync(c->d_key.p, recs.data(), n * sizeof(KeyRows), hipMemcpyHostToDevice, s));
        if (total) RG_HIP(c, hipMemcpyAsync(c->d_key_rows.p, chroma, (size_t)total * RG_KEY_CHROMA * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        rc = key_launch_finish(c, c->d_key_rows.p, reinterpret_cast<const KeyRows *>(c->d_key.p), n, o.segment, reinterpret_cast<RgKeyFinish *>(c->d_key.p + fin_at), s);
        if (rc == RG_OK) {
            const hipError_t e = hipMemcpyAsync(fin.data(), c->d_key.p + fin_at, n * sizeof(RgKeyFinish), hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) rc = rg_set_err(c, RG_ERR_DEVICE, "rg_key_from_chroma: %s", hipGetErrorString(e));
        }
        RG_HIP(c, hipStreamSynchronize(s));
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) rg_key_fill(nullptr, nullptr, counts[i], fin[i], 0, 0, recs[i].rows_at, &out[i]);
        return RG_OK;
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

// ---- measurement hook (tools/key_rate.py) ------------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per word: word w <- a mix of its index (as rg_tempo.hip fills its arena)
__global__ __launch_bounds__(256) void rg_key_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}
// the read-only pass the decimation is compared with: every 16-byte word of the planes once, one sum per workgroup
__global__ __launch_bounds__(256) void rg_key_read_kernel(const uint4 *__restrict__ src, uint64_t words, uint32_t *__restrict__ sums) {
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

extern "C" int rg_key_rate(void *ctx, size_t n, uint64_t frames, const rg_key_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                           double *decim_ms, double *read_ms, double *tiles_ms, double *finish_ms, double *host_stage1_ms, double *host_finish_ms,
                           size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || n > 65535 || !frames || frames >= ((uint64_t)1 << 32) || !reps || !decim_ms || !read_ms || !tiles_ms || !finish_ms ||
        (host_tracks && (!host_stage1_ms || !host_finish_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_key_rate: bad arguments");
    rg_key_opts o;
    char err[256] = "";
    int rc = rg_key_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 2 * 2, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d = nullptr;
    float *d_y = nullptr;
    uint16_t *d_rows = nullptr;
    uint32_t *d_sums = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgKeyTrack> tracks(n);
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)RG_FMT_S16_PLANAR;
            if (rg_key_track(i, t, total, &tracks[i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_key_rate: %s", err);
        }
        KeyJob job;
        int jr = key_job(c, tracks.data(), n, o, &job);
        if (jr != RG_OK) return jr;
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d, job.end));
        RG_HIP(c, hipMalloc((void **)&d_y, ((size_t)job.y_floats + 16) * sizeof(float)));
        RG_HIP(c, hipMalloc((void **)&d_rows, ((size_t)job.rows * RG_KEY_CHROMA + 16) * sizeof(uint16_t)));
        RG_HIP(c, hipMalloc((void **)&d_sums, 4096 * sizeof(uint32_t)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_key_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, job.fp.head.data(), job.fp.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemcpyAsync(d + job.tracks_at, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const uint32_t M = tracks[0].m, F = tracks[0].rows;
        std::vector<float> host_y((size_t)M * host_tracks + 1);
        std::vector<uint16_t> host_rows((size_t)F * RG_KEY_CHROMA * host_tracks + 1);
        std::vector<RgKeyFinish> host_fin(host_tracks + 1), dev_fin(n);
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
        enum { kDecim, kRead, kTiles, kFinish, kStages };
        const auto launch = [&](int what) -> int {
            if (what == kDecim) return key_launch_decim(c, d_arena, d, job, d_y, s);
            if (what == kRead) {
                hipLaunchKernelGGL(rg_key_read_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<const uint4 *>(d_arena), (uint64_t)(total / 16), d_sums);
                RG_HIP(c, hipGetLastError());
                return RG_OK;
            }
            if (what == kTiles) return key_launch_tiles(c, d, job, d_y, d_rows, nullptr, s);
            return key_launch_finish(c, d_rows, reinterpret_cast<const KeyRows *>(d + job.rows_at), n, job.segment, reinterpret_cast<RgKeyFinish *>(d + job.fin_at), s);
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            for (int what = kDecim; what < kStages; ++what) {
                const int lr = launch(what);
                if (lr != RG_OK) return lr;
            }
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            double *const dst[kStages] = {decim_ms, read_ms, tiles_ms, finish_ms};
            for (int what = kDecim; what < kStages; ++what) {  // the four alternate within a round
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
                pool_run(host_tracks, [&](size_t i) {
                    (void)rg_key_folded_host(h.data(), tracks[i], host_y.data() + (size_t)M * i, nullptr, host_rows.data() + (size_t)F * RG_KEY_CHROMA * i);
                });
                host_stage1_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                t0 = std::chrono::steady_clock::now();
                pool_run(host_tracks, [&](size_t i) { rg_key_stage2_host(host_rows.data() + (size_t)F * RG_KEY_CHROMA * i, F, o, &host_fin[i]); });
                host_finish_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            std::vector<float> dev_y(M + 1u);
            std::vector<uint16_t> dev_rows((size_t)F * RG_KEY_CHROMA * host_tracks + 1);
            RG_HIP(c, hipMemcpy(dev_rows.data(), d_rows, (size_t)F * RG_KEY_CHROMA * host_tracks * sizeof(uint16_t), hipMemcpyDeviceToHost));
            RG_HIP(c, hipMemcpy(dev_fin.data(), d + job.fin_at, n * sizeof(RgKeyFinish), hipMemcpyDeviceToHost));
            *mismatches = 0;
            for (size_t i = 0; i < host_tracks; ++i) {
                RG_HIP(c, hipMemcpy(dev_y.data(), d_y + tracks[i].y_at, (size_t)M * sizeof(float), hipMemcpyDeviceToHost));
                *mismatches += memcmp(dev_y.data(), host_y.data() + (size_t)M * i, (size_t)M * sizeof(float)) != 0;
                *mismatches += memcmp(&dev_fin[i], &host_fin[i], sizeof(RgKeyFinish)) != 0;
            }
            for (size_t i = 0; i < (size_t)F * RG_KEY_CHROMA * host_tracks; ++i) *mismatches += dev_rows[i] != host_rows[i];
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_key_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_sums) (void)hipFree(d_sums);
    if (d_rows) (void)hipFree(d_rows);
    if (d_y) (void)hipFree(d_y);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
