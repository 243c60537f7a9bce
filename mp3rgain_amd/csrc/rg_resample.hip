// rg_resample.hip -- the rational resampler on the device and the cross-rate fingerprint on top of it
// (include/mp3rgain_amd_resample.h, rg_resample.h): per track the signal brought to 11025 Hz, then the fingerprint's tile walk
// (rg_fprint.hip: rg_fprint_device) over the resampled buffer as an arena of mono f32 tracks with the 11025 Hz edges.
//
//   rg_resample_kernel  the hot path for L >= 2: one workgroup of 256 lanes per run of 256 consecutive outputs of one track,
//                       many tracks per launch, one launch per format; the workgroup finds its track as the key scan's
//                       decimation kernel does.  Where the run starts (b_{j0}, p_{j0}, j0 mod L) comes from a record the host
//                       made in 64 bits; from there lane t goes on in 32: b = b_{j0} + (t M + L - 1 - p_{j0}) / L, the
//                       division a multiplication by a reciprocal.  The run's input span, b_{j0} .. b_{j0 + 255} + P - 1
//                       (1185 samples at 48 kHz, at most 8673), is read from the arena once, consecutive lanes reading
//                       consecutive samples of a plane (each lane only its own sample: nothing outside the plane is touched,
//                       whatever its alignment), down-mixed and staged in LDS as f32.  Every lane then sums its own window in
//                       ascending k.  Unlike the decimator's, the phase differs from lane to lane, but it depends on j mod L
//                       only: the table lies tap-major and by output residue, hq[k][j mod L], so consecutive lanes read
//                       consecutive words of row k with one wrap, instead of 64 scattered rows.  The table (41 KB at 48 kHz,
//                       164 KB at 192 kHz) is shared by every workgroup of that rate and stays in L2.  No scratch memory.
//   L = 1               (and the identity) is the key scan's decimation kernel (rg_key.hip: rg_key_decimate_launch), not a copy.
// This unit is compiled without contraction: same input, same bytes as the host's route 2.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_fprint_tile.h"
#include "rg_key.h"
#include "rg_pcm_seam.h"
#include "rg_resample.h"

#define RS_STAGE_LOADS 5u  // at 48 kHz a run is 1185 samples: one round of 5 x 256

// sample k of a plane as the stored pattern, S16 sign-extended (what rg_spec_value takes)
template <int FMT>
__device__ __forceinline__ uint32_t rs_raw(const unsigned char *plane, uint32_t k) {
    if (FMT == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(plane)[k];
    return reinterpret_cast<const uint32_t *>(plane)[k];
}

template <int FMT>
__global__ __launch_bounds__(RG_RS_LANES) void rg_resample_kernel(const unsigned char *__restrict__ arena, const RgRsTrack *__restrict__ tracks,
                                                                  const uint64_t *__restrict__ run_first, const uint32_t *__restrict__ run_track,
                                                                  uint32_t n_runs, uint64_t wg_base, const RgRsStart *__restrict__ starts,
                                                                  const float *__restrict__ tables, float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = wg_base + blockIdx.x;
    uint32_t lo = 0, hi = n_runs;  // the last run that starts at or before this workgroup: the same in every lane
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (run_first[mid] <= wg) lo = mid; else hi = mid;
    }
    const RgRsTrack &p = tracks[run_track[lo]];
    const RgRsStart st = starts[wg];
    const uint32_t L = p.up, M = p.down, P = p.taps, recip = p.recip;
    const uint32_t j0 = (uint32_t)(wg - p.first_wg) * RG_RS_OUTPUTS;
    const uint32_t left = p.m - j0, no = left < RG_RS_OUTPUTS ? left : RG_RS_OUTPUTS;  // j0 < M_out
    const uint32_t p0j = st.phase_resid & 0xFFFFu, r0 = st.phase_resid >> 16;
    // output j0 + t starts b_{j0} + ceil((t M - p_{j0}) / L) samples in: (t M + L - 1 - p) L <= (255 * 32 L + L) L < 2^32
    const uint32_t slack = L - 1u - p0j;
    const uint32_t count = __umulhi((no - 1u) * M + slack, recip) + P;  // b_{j0 + no - 1} + P <= N: every sample read is the track's
    const bool two = p.channels >= 2;
    const uint64_t base = (uint64_t)st.first * (FMT == RG_FMT_S16_PLANAR ? 2u : 4u);
    const unsigned char *q0 = arena + p.off0 + base, *q1 = arena + p.off1 + base;  // the run's first sample in each plane
    // RS_STAGE_LOADS samples of each plane per lane are asked for before the first is waited for (as the decimation kernel does)
    for (uint32_t i0 = tid; i0 < count; i0 += RS_STAGE_LOADS * RG_RS_LANES) {
        uint32_t ra[RS_STAGE_LOADS], rb[RS_STAGE_LOADS];
#pragma unroll
        for (uint32_t u = 0; u < RS_STAGE_LOADS; ++u) {
            // without a branch: beyond the run, its last sample again; of a single channel, p1 is p0
            const uint32_t i = i0 + u * RG_RS_LANES, ic = i < count ? i : count - 1u;
            ra[u] = rs_raw<FMT>(q0, ic);
            rb[u] = rs_raw<FMT>(q1, ic);
        }
#pragma unroll
        for (uint32_t u = 0; u < RS_STAGE_LOADS; ++u) {
            const uint32_t i = i0 + u * RG_RS_LANES, ic = i < count ? i : count - 1u;  // (beyond the run: the last sample's place, its value)
            const float a = rg_spec_value<FMT>(ra[u]);
            s_x[ic] = two ? (a + rg_spec_value<FMT>(rb[u])) * 0.5f : a;
        }
    }
    __syncthreads();
    if (tid < no) {
        const uint32_t db = __umulhi(tid * M + slack, recip);  // db + P <= count
        const uint32_t rr = r0 + tid, r = rr - __umulhi(rr, recip) * L;  // (j0 + t) mod L
        const float *h = tables + p.hq_at + r, *x = s_x + db;
        float s = 0.0f;
        for (uint32_t k = 0; k < P; ++k) {
            const float prod = h[k * L] * x[k];
            s += prod;
        }
        y[p.y_at + j0 + tid] = s;
    }
}

// ---- one call's launches -----------------------------------------------------------------------------------------------------
// Device layout of the work buffer, every part 16-byte aligned: [track records | run starts | run -> track | workgroup starts |
// tap tables]; the L = 1 tracks are a job of the key scan's (c->d_key)
struct RsJob {
    std::vector<unsigned char> head;
    uint64_t fmt_wg[4];
    size_t tracks_at, first_at, run_at, starts_at, tables_at, end, n, n_runs;
    uint64_t y_floats;
    uint32_t fmt_lds[3];  // the dynamic LDS of each format's launch
    RgKeyDecimJob *decim = nullptr;
    ~RsJob() { rg_key_decimate_free(decim); }
};

// tracks: rg_rs_track'ed; they are planned here
static int rs_job(rg_ctx *c, RgRsTrack *tracks, size_t n, hipStream_t s, RsJob *job) {
    std::vector<float> tables;
    std::vector<RgRsStart> starts;
    std::vector<uint64_t> first;
    std::vector<uint32_t> run;
    job->n = n;
    job->y_floats = rg_rs_plan(tracks, n, job->fmt_wg, &tables, &starts);
    for (uint32_t f = 0; f < 3; ++f) {  // the runs in the order of their workgroups
        uint32_t span = 0;
        for (size_t i = 0; i < n; ++i)
            if (tracks[i].format == f && tracks[i].n_wg) {
                first.push_back(tracks[i].first_wg);
                run.push_back((uint32_t)i);
                span = std::max(span, tracks[i].span);
            }
        job->fmt_lds[f] = span * (uint32_t)sizeof(float);
    }
    if (n > 0x7fffffffu || job->fmt_wg[3] > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu tracks, %llu resampler workgroups", n, (unsigned long long)job->fmt_wg[3]);
    job->n_runs = run.size();
    job->tracks_at = 0;
    job->first_at = fp_a16(n * sizeof(RgRsTrack));
    job->run_at = fp_a16(job->first_at + first.size() * sizeof(uint64_t));
    job->starts_at = fp_a16(job->run_at + run.size() * sizeof(uint32_t));
    job->tables_at = fp_a16(job->starts_at + starts.size() * sizeof(RgRsStart));
    job->end = fp_a16(job->tables_at + tables.size() * sizeof(float));
    job->head.assign(job->end, 0);
    unsigned char *h = job->head.data();
    memcpy(h, tracks, n * sizeof(RgRsTrack));
    if (!first.empty()) memcpy(h + job->first_at, first.data(), first.size() * sizeof(uint64_t));
    if (!run.empty()) memcpy(h + job->run_at, run.data(), run.size() * sizeof(uint32_t));
    if (!starts.empty()) memcpy(h + job->starts_at, starts.data(), starts.size() * sizeof(RgRsStart));
    if (!tables.empty()) memcpy(h + job->tables_at, tables.data(), tables.size() * sizeof(float));
    // the L = 1 tracks (and y = x) as the key scan's decimation of factor M
    std::vector<RgKeyTrack> kt;
    std::vector<uint64_t> y_at;
    for (size_t i = 0; i < n; ++i) {
        const RgRsTrack &t = tracks[i];
        if (t.up != 1 || !t.m) continue;
        RgKeyTrack k;
        memset(&k, 0, sizeof k);
        k.off0 = t.off0;
        k.off1 = t.off1;
        k.n = t.n;
        k.m = t.m;
        k.decim = t.down;
        k.format = t.format;
        k.channels = t.channels;
        k.n_wg = (t.m + RG_KEY_DECIM_OUTPUTS - 1u) / RG_KEY_DECIM_OUTPUTS;
        k.recip = (uint32_t)(0xFFFFFFFFu / t.down) + 1u;
        kt.push_back(k);
        y_at.push_back(t.y_at);
    }
    return kt.empty() ? RG_OK : rg_key_decimate_prepare(c, kt.data(), y_at.data(), kt.size(), s, &job->decim);
}

template <int FMT>
static hipError_t rs_launch_format(const unsigned char *d_arena, unsigned char *d, const RsJob &job, float *d_y, hipStream_t s) {
    const uint64_t base = job.fmt_wg[FMT], count = job.fmt_wg[FMT + 1] - base;
    if (!count) return hipSuccess;
    hipLaunchKernelGGL((rg_resample_kernel<FMT>), dim3((uint32_t)count), dim3(RG_RS_LANES), job.fmt_lds[FMT], s, d_arena,
                       reinterpret_cast<const RgRsTrack *>(d + job.tracks_at), reinterpret_cast<const uint64_t *>(d + job.first_at),
                       reinterpret_cast<const uint32_t *>(d + job.run_at), (uint32_t)job.n_runs, base, reinterpret_cast<const RgRsStart *>(d + job.starts_at),
                       reinterpret_cast<const float *>(d + job.tables_at), d_y);
    return hipGetLastError();
}

static int rs_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const RsJob &job, float *d_y, hipStream_t s) {
    static_assert(RG_FMT_F32_PLANAR == 0 && RG_FMT_S16_PLANAR == 1 && RG_FMT_S32_PLANAR == 2, "fmt_wg is indexed by the format");
    static_assert(RG_RS_MAX_SPAN * sizeof(float) <= 65536, "the staged span fits the LDS a kernel gets without asking");
    RG_HIP(c, rs_launch_format<RG_FMT_F32_PLANAR>(d_arena, d, job, d_y, s));
    RG_HIP(c, rs_launch_format<RG_FMT_S16_PLANAR>(d_arena, d, job, d_y, s));
    RG_HIP(c, rs_launch_format<RG_FMT_S32_PLANAR>(d_arena, d, job, d_y, s));
    return rg_key_decimate_launch(c, d_arena, job.decim, d_y, s);
}

int rg_resample_device(rg_ctx *c, const unsigned char *d_arena, RgRsTrack *tracks, size_t n, hipStream_t s) {
    if (!n) return RG_OK;
    RsJob job;
    int rc = rs_job(c, tracks, n, s, &job);
    if (rc != RG_OK) return rc;
    RG_HIP(c, c->d_rs.reserve(job.end));
    RG_HIP(c, c->d_rs_y.reserve((size_t)job.y_floats + 16));
    RG_HIP(c, hipMemcpyAsync(c->d_rs.p, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    rc = rs_launch(c, d_arena, c->d_rs.p, job, c->d_rs_y.p, s);
    const hipError_t e = hipStreamSynchronize(s);  // (the head is on its way)
    if (rc != RG_OK) return rc;
    RG_HIP(c, e);
    return RG_OK;
}

int rg_xrate_device(rg_ctx *c, const unsigned char *d_arena, RgRsTrack *tracks, RgFpTrack *fp, size_t n, uint64_t codes_base, uint32_t *d_codes, float *d_bands,
                    uint32_t *nonfinite, hipStream_t s) {
    if (!n) return RG_OK;
    const int rc = rg_resample_device(c, d_arena, tracks, n, s);
    if (rc != RG_OK) return rc;
    for (size_t i = 0; i < n; ++i) rg_xr_fp_track(tracks[i], tracks[i].y_at * sizeof(float), &fp[i]);
    uint64_t fmt_tile[4];
    (void)rg_fp_plan(fp, n, fmt_tile, codes_base, 0);
    return rg_fprint_device(c, reinterpret_cast<const unsigned char *>(c->d_rs_y.p), fp, n, d_codes, d_bands, nonfinite, s);
}

// ---- test seams (include/mp3rgain_amd_resample.h) ----------------------------------------------------------------------------
static int rs_plan_tracks(size_t n, const rg_track_desc *descs, size_t arena_bytes, std::vector<RgRsTrack> *tracks, char *err, size_t err_len) {
    *tracks = std::vector<RgRsTrack>(n + 1);
    for (size_t i = 0; i < n; ++i) {
        const int rc = rg_rs_track(i, descs[i], arena_bytes, &(*tracks)[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    return RG_OK;
}

// y of every track, packed in track order, to y_out (enqueued on `s`)
static int rs_copy_y(rg_ctx *c, const std::vector<RgRsTrack> &tracks, size_t n, float *y_out, hipStream_t s) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const RgRsTrack &t = tracks[i];
        if (y_out && t.m) RG_HIP(c, hipMemcpyAsync(y_out + at, c->d_rs_y.p + t.y_at, (size_t)t.m * sizeof(float), hipMemcpyDeviceToHost, s));
        at += t.m;
    }
    return RG_OK;
}

extern "C" int rg_resample_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_resample_result *out,
                                 float *y_out) {
    std::vector<RgRsTrack> tracks;
    const auto host = [&](char *err, size_t err_len) { return rg_rs_arena_host(route, n, descs, arena, arena_bytes, out, y_out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) { return rs_plan_tracks(n, descs, arena_bytes, &tracks, err, err_len); };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        if (!n) return RG_OK;
        int rc = rg_resample_device(c, c->d_arena.p, tracks.data(), n, s);
        if (rc == RG_OK) rc = rs_copy_y(c, tracks, n, y_out, s);
        if (rc != RG_OK) return rc;
        RG_HIP(c, hipStreamSynchronize(s));
        uint64_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_rs_fill(descs[i], tracks[i], at, &out[i]);
            at += tracks[i].m;
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_resample_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

extern "C" int rg_xrate_fingerprint_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes,
                                          rg_xrate_result *out, uint32_t *codes_out, float *bands_out, float *y_out) {
    std::vector<RgRsTrack> tracks;
    const auto host = [&](char *err, size_t err_len) {
        return rg_xr_arena_host(route, n, descs, arena, arena_bytes, out, codes_out, bands_out, y_out, err, err_len);
    };
    const auto plan = [&](char *err, size_t err_len) { return rs_plan_tracks(n, descs, arena_bytes, &tracks, err, err_len); };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        if (!n) return RG_OK;
        std::vector<RgFpTrack> fp(n + 1);
        uint64_t n_codes = 0, n_frames = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_xr_fp_track(tracks[i], 0, &fp[i]);
            n_codes += fp[i].frames ? fp[i].frames - 1u : 0u;
            n_frames += fp[i].frames;
        }
        // the codes, then the band energies when they are asked for
        const size_t bands_at = ((size_t)n_codes + 3) & ~(size_t)3, words = bands_at + (bands_out ? (size_t)n_frames * RG_FP_BANDS : 0);
        RG_HIP(c, c->d_fp_codes.reserve(words + 4));
        uint32_t *d_codes = c->d_fp_codes.p;
        float *d_bands = bands_out ? reinterpret_cast<float *>(d_codes + bands_at) : nullptr;
        std::vector<uint32_t> nonfinite(n);
        int rc = rg_xrate_device(c, c->d_arena.p, tracks.data(), fp.data(), n, 0, d_codes, d_bands, nonfinite.data(), s);
        if (rc == RG_OK) rc = rs_copy_y(c, tracks, n, y_out, s);
        if (rc != RG_OK) return rc;
        if (codes_out && n_codes) RG_HIP(c, hipMemcpyAsync(codes_out, d_codes, (size_t)n_codes * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (bands_out && n_frames) RG_HIP(c, hipMemcpyAsync(bands_out, d_bands, (size_t)n_frames * RG_FP_BANDS * sizeof(float), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        uint64_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_xr_fill(descs[i], tracks[i], fp[i], 0, nonfinite[i], (uint32_t)i, at, &out[i]);
            at += tracks[i].m;
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_xrate_fingerprint_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/resample_rate.py) -------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per word: word w <- a mix of its index (as rg_key.hip fills its arena)
__global__ __launch_bounds__(256) void rg_rs_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}
// the read-only pass the resampler is compared with: every 16-byte word of the planes once, one sum per workgroup
__global__ __launch_bounds__(256) void rg_rs_read_kernel(const uint4 *__restrict__ src, uint64_t words, uint32_t *__restrict__ sums) {
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

extern "C" int rg_resample_rate(void *ctx, size_t n, uint64_t frames, uint32_t sample_rate, size_t host_tracks, uint32_t threads, uint32_t reps,
                                double warm_ms, double *resample_ms, double *read_ms, double *host_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || n > 65535 || !frames || frames >= ((uint64_t)1 << 32) || !reps || !resample_ms || !read_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_resample_rate: bad arguments");
    char err[256] = "";
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 2 * 2, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d = nullptr;
    float *d_y = nullptr;
    uint32_t *d_sums = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgRsTrack> tracks(n);
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = sample_rate;
            t.channels = 2;
            t.format = (uint16_t)RG_FMT_S16_PLANAR;
            if (rg_rs_track(i, t, total, &tracks[i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_resample_rate: %s", err);
        }
        if (!tracks[0].up) return rg_set_err(c, RG_ERR_UNSUPPORTED_RATE, "rg_resample_rate: %u Hz is not supported", sample_rate);
        RsJob job;
        const int jr = rs_job(c, tracks.data(), n, s, &job);
        if (jr != RG_OK) return jr;
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d, job.end + 16));
        RG_HIP(c, hipMalloc((void **)&d_y, ((size_t)job.y_floats + 16) * sizeof(float)));
        RG_HIP(c, hipMalloc((void **)&d_sums, 4096 * sizeof(uint32_t)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_rs_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const uint32_t M = tracks[0].m;
        std::vector<float> host_y((size_t)M * host_tracks + 1);
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
        enum { kResample, kRead, kStages };
        const auto launch = [&](int what) -> int {
            if (what == kResample) return rs_launch(c, d_arena, d, job, d_y, s);
            hipLaunchKernelGGL(rg_rs_read_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<const uint4 *>(d_arena), (uint64_t)(total / 16), d_sums);
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            for (int what = kResample; what < kStages; ++what) {
                const int lr = launch(what);
                if (lr != RG_OK) return lr;
            }
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            double *const dst[kStages] = {resample_ms, read_ms};
            for (int what = kResample; what < kStages; ++what) {  // the two alternate within a round
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
                const auto t0 = std::chrono::steady_clock::now();
                pool_run(host_tracks, [&](size_t i) { rg_rs_folded_host(h.data(), tracks[i], host_y.data() + (size_t)M * i); });
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            std::vector<float> dev_y(M + 1u);
            *mismatches = 0;
            for (size_t i = 0; i < host_tracks; ++i) {
                RG_HIP(c, hipMemcpy(dev_y.data(), d_y + tracks[i].y_at, (size_t)M * sizeof(float), hipMemcpyDeviceToHost));
                *mismatches += memcmp(dev_y.data(), host_y.data() + (size_t)M * i, (size_t)M * sizeof(float)) != 0;
            }
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_resample_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_sums) (void)hipFree(d_sums);
    if (d_y) (void)hipFree(d_y);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
