// rg_fprint.hip -- stage 1 of the duplicate finder on the device (include/mp3rgain_amd_fingerprint.h, rg_fprint.h): per track a
// 32-bit sub-band-difference code per 512 samples, from the planes of the analysis arena in any of its three formats.
//
// The tile walk itself (staging, pairs of frames, the passes, the band sums) is rg_fprint_tile.h's, shared with the tempo scan.
//   rg_fp_tiles_kernel  one workgroup of 256 lanes per tile of RG_FP_TILE_CODES = 7 codes of one track, many tracks per launch,
//                       one launch per format; the workgroup finds its track in a tile -> track table.  A tile needs 8 frames
//                       (the first is the last frame of the tile before: a code is a difference of two frames), which at hop
//                       512 are 7680 samples: they are read from the arena once, down-mixed ((ch0 + ch1) * 0.5f), and staged
//                       in 30 KB of LDS, consecutive lanes reading consecutive samples; every frame is windowed from there.
//                       Frames are transformed two at a time, as the real and imaginary part of one 4096-point complex
//                       transform: the spectral scan's three radix-16 passes in registers (rg_spectrum.h) with its exchange
//                       buffer and padding (38 KB of LDS).  Lanes 0 .. 32 sum the 33 bands of the first frame, lanes 64 .. 96
//                       (another wave) those of the second, in bin order; the 8 x 33 band energies stay in LDS, and lanes
//                       0 .. 6 make the codes.  69 KB of LDS in all: two workgroups per CU (160 KB), so one workgroup's
//                       barriers overlap the other's butterflies; 15 codes per tile would save half of the 1/8 of frames that
//                       are transformed twice and leave one workgroup per CU.  The last pass is not pruned: every lane's
//                       DFT16 yields bins on both sides of the 2 kHz edge.
//   rg_fp_fold_kernel   one workgroup per track: the non-finite frames its tiles counted, summed.
// No atomics, no transcendental in the kernels, and this unit is compiled without contraction: same input, same bits as the
// host's route 2.  The launcher's callers check every track against the arena first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_fprint.h"
#include "rg_fprint_tile.h"
#include "rg_pcm_seam.h"

#define RG_FP_LDS_BYTES RG_FP_TILE_LDS(RG_FP_BANDS)

template <int FMT>
__global__ __launch_bounds__(RG_FP_LANES) void rg_fp_tiles_kernel(const unsigned char *__restrict__ arena, const RgSpecTables *__restrict__ tables,
                                                                  const RgFpTrack *__restrict__ tracks, const uint32_t *__restrict__ tile_track,
                                                                  uint64_t tile_base, uint32_t *__restrict__ codes, float *__restrict__ bands,
                                                                  uint32_t *__restrict__ tile_nonfinite) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const float *s_E = rg_fp_tile_rows(s_raw);
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = tile_base + blockIdx.x;
    const RgFpTrack &p = tracks[tile_track[tile]];
    const uint32_t t = (uint32_t)(tile - p.first_tile), f0 = t * RG_FP_TILE_CODES;
    uint32_t nonfinite;
    const uint32_t nf = rg_fp_tile_bands<FMT, RG_FP_BANDS>(arena, tables, p, t, s_raw, &nonfinite);
    if (tid + 1 < nf) codes[p.codes_at + f0 + tid] = rg_fp_code(s_E + tid * RG_FP_BANDS, s_E + (tid + 1) * RG_FP_BANDS);
    if (bands) {
        float *dst = bands + (p.frames_at + f0) * RG_FP_BANDS;
        for (uint32_t k = tid + (t ? RG_FP_BANDS : 0u); k < nf * RG_FP_BANDS; k += RG_FP_LANES) dst[k] = s_E[k];
    }
    if (tid == 0) tile_nonfinite[tile] = nonfinite;
}

static size_t a16(size_t x) { return fp_a16(x); }

template <int FMT>
static hipError_t fp_launch_format(const unsigned char *d_arena, unsigned char *d, const FpJob &job, uint32_t *d_codes, float *d_bands, hipStream_t s) {
    const uint64_t base = job.fmt_tile[FMT == RG_FMT_F32_PLANAR ? 0 : FMT == RG_FMT_S16_PLANAR ? 1 : 2];
    const uint64_t count = job.fmt_tile[(FMT == RG_FMT_F32_PLANAR ? 0 : FMT == RG_FMT_S16_PLANAR ? 1 : 2) + 1] - base;
    if (!count) return hipSuccess;
    // more than 64 KB of LDS has to be asked for
    const hipError_t e = hipFuncSetAttribute((const void *)rg_fp_tiles_kernel<FMT>, hipFuncAttributeMaxDynamicSharedMemorySize, RG_FP_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rg_fp_tiles_kernel<FMT>), dim3((uint32_t)count), dim3(RG_FP_LANES), RG_FP_LDS_BYTES, s, d_arena,
                       reinterpret_cast<const RgSpecTables *>(d), reinterpret_cast<const RgFpTrack *>(d + job.tracks_at),
                       reinterpret_cast<const uint32_t *>(d + job.map_at), base, d_codes, d_bands, reinterpret_cast<uint32_t *>(d + job.counts_at));
    return hipGetLastError();
}

static int fp_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const FpJob &job, uint32_t *d_codes, float *d_bands, hipStream_t s) {
    RG_HIP(c, fp_launch_format<RG_FMT_F32_PLANAR>(d_arena, d, job, d_codes, d_bands, s));
    RG_HIP(c, fp_launch_format<RG_FMT_S16_PLANAR>(d_arena, d, job, d_codes, d_bands, s));
    RG_HIP(c, fp_launch_format<RG_FMT_S32_PLANAR>(d_arena, d, job, d_codes, d_bands, s));
    hipLaunchKernelGGL(rg_fp_fold_kernel<0>, dim3((uint32_t)job.n), dim3(256), 0, s, reinterpret_cast<const RgFpTrack *>(d + job.tracks_at),
                       reinterpret_cast<const uint32_t *>(d + job.counts_at), reinterpret_cast<uint32_t *>(d + job.res_at));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_fprint_device(rg_ctx *c, const unsigned char *d_arena, RgFpTrack *tracks, size_t n, uint32_t *d_codes, float *d_bands, uint32_t *nonfinite,
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
    RG_HIP(c, c->d_fprint.reserve(job.end));
    unsigned char *d = c->d_fprint.p;
    RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    const int rc = fp_launch(c, d_arena, d, job, d_codes, d_bands, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(nonfinite, d + job.res_at, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_fingerprint.h) --------------------------------------------------------------------------
extern "C" int rg_fingerprint_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes,
                                    rg_fingerprint_result *out, uint32_t *codes_out, float *bands_out) {
    std::vector<RgFpTrack> tracks;
    uint64_t n_codes = 0, n_frames = 0;
    const auto host = [&](char *err, size_t err_len) { return rg_fp_arena_host(route, n, descs, arena, arena_bytes, out, codes_out, bands_out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        tracks = std::vector<RgFpTrack>(n + 1);
        for (size_t i = 0; i < n; ++i) {
            const int rc = rg_fp_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        uint64_t fmt_tile[4];
        (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
        for (size_t i = 0; i < n; ++i) {
            n_codes += tracks[i].frames ? tracks[i].frames - 1u : 0u;
            n_frames += tracks[i].frames;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        // the codes, then the band energies when they are asked for
        const size_t bands_at = ((size_t)n_codes + 3) & ~(size_t)3, words = bands_at + (bands_out ? (size_t)n_frames * RG_FP_BANDS : 0);
        RG_HIP(c, c->d_fp_codes.reserve(words + 4));
        uint32_t *d_codes = c->d_fp_codes.p;
        float *d_bands = bands_out ? reinterpret_cast<float *>(d_codes + bands_at) : nullptr;
        std::vector<uint32_t> nonfinite(n ? n : 1);
        const int rc = rg_fprint_device(c, c->d_arena.p, tracks.data(), n, d_codes, d_bands, nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        if (codes_out && n_codes) RG_HIP(c, hipMemcpyAsync(codes_out, d_codes, (size_t)n_codes * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (bands_out && n_frames) RG_HIP(c, hipMemcpyAsync(bands_out, d_bands, (size_t)n_frames * RG_FP_BANDS * sizeof(float), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) rg_fp_fill(descs[i], tracks[i], 0, nonfinite[i], (uint32_t)i, &out[i]);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_fingerprint_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/fingerprint_rate.py) ----------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per word: word w <- a mix of its index (as rg_spectrum.hip fills its arena)
__global__ __launch_bounds__(256) void rg_fp_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}
// the read-only pass the fingerprint stage is compared with: every 16-byte word of the planes once, one sum per workgroup
__global__ __launch_bounds__(256) void rg_fp_read_kernel(const uint4 *__restrict__ src, uint64_t words, uint32_t *__restrict__ sums) {
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

extern "C" int rg_fingerprint_rate(void *ctx, size_t n, uint64_t frames, const rg_fingerprint_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                                   double warm_ms, double *fp_ms, double *read_ms, double *match_ms, double *host_fp_ms, double *host_match_ms,
                                   size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || n > 65535 || !frames || frames >= ((uint64_t)1 << 32) || !reps || !fp_ms || !read_ms || !match_ms ||
        (host_tracks && (!host_fp_ms || !host_match_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_rate: bad arguments");
    rg_fingerprint_opts o;
    char err[256] = "";
    int rc = rg_fp_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 2 * 2, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d = nullptr, *d_match = nullptr;
    uint32_t *d_codes = nullptr, *d_sums = nullptr;
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
            if (rg_fp_track(i, t, total, &tracks[i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_rate: %s", err);
        }
        uint64_t fmt_tile[4];
        (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
        FpJob job;
        fp_job(tracks.data(), n, fmt_tile, &job);
        const uint32_t k = tracks[0].frames ? tracks[0].frames - 1u : 0u;
        std::vector<uint32_t> counts(n, k), rates(n, 44100u);
        std::vector<uint64_t> at(n);
        for (size_t i = 0; i < n; ++i) at[i] = tracks[i].codes_at;
        const size_t n_rec = n * (n - 1) / 2;
        std::vector<rg_fingerprint_pair_record> host_rec(n_rec + 1), dev_rec(n_rec + 1);
        std::vector<RgFpPair> pairs;
        rg_fp_pairs(n, counts.data(), rates.data(), at.data(), o, &pairs, dev_rec.data());
        const size_t rec_at = a16(pairs.size() * sizeof(RgFpPair));
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d, job.end));
        RG_HIP(c, hipMalloc((void **)&d_codes, ((size_t)k * n + 4) * sizeof(uint32_t)));
        RG_HIP(c, hipMalloc((void **)&d_sums, 4096 * sizeof(uint32_t)));
        RG_HIP(c, hipMalloc((void **)&d_match, rec_at + (n_rec + 1) * sizeof(rg_fingerprint_pair_record)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_fp_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
        if (!pairs.empty()) RG_HIP(c, hipMemcpyAsync(d_match, pairs.data(), pairs.size() * sizeof(RgFpPair), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const RgFpPair *d_pairs = reinterpret_cast<const RgFpPair *>(d_match);
        rg_fingerprint_pair_record *d_rec = reinterpret_cast<rg_fingerprint_pair_record *>(d_match + rec_at);
        std::vector<uint32_t> host_codes((size_t)k * host_tracks + 1);
        std::vector<RgFpPair> host_pairs;  // those among the first host_tracks tracks
        for (const RgFpPair &p : pairs)
            if (p.a_at < (uint64_t)k * host_tracks && p.b_at < (uint64_t)k * host_tracks) host_pairs.push_back(p);
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
        enum { kFp, kRead, kMatch };
        const auto launch = [&](int what) -> int {
            if (what == kFp) return fp_launch(c, d_arena, d, job, d_codes, nullptr, s);
            if (what == kRead) {
                hipLaunchKernelGGL(rg_fp_read_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<const uint4 *>(d_arena), (uint64_t)(total / 16), d_sums);
                RG_HIP(c, hipGetLastError());
                return RG_OK;
            }
            return pairs.empty() ? RG_OK : rg_fprint_match_launch(c, d_codes, d_pairs, pairs.size(), o, d_rec, s);
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            for (int what = kFp; what <= kMatch; ++what) {
                const int lr = launch(what);
                if (lr != RG_OK) return lr;
            }
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            double *const dst[3] = {fp_ms, read_ms, match_ms};
            for (int what = kFp; what <= kMatch; ++what) {  // the three alternate within a round
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
                pool_run(host_tracks, [&](size_t i) { (void)rg_fp_folded_host(h.data(), tracks[i], host_codes.data() + tracks[i].codes_at, nullptr); });
                host_fp_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                t0 = std::chrono::steady_clock::now();
                pool_run(host_pairs.size(), [&](size_t i) { rg_fp_match_host(host_codes.data(), host_pairs[i], o, &host_rec[host_pairs[i].rec]); });
                host_match_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            std::vector<uint32_t> dev_codes((size_t)k * host_tracks + 1);
            RG_HIP(c, hipMemcpy(dev_codes.data(), d_codes, (size_t)k * host_tracks * sizeof(uint32_t), hipMemcpyDeviceToHost));
            RG_HIP(c, hipMemcpy(dev_rec.data(), d_rec, n_rec * sizeof(rg_fingerprint_pair_record), hipMemcpyDeviceToHost));
            *mismatches = 0;
            for (size_t i = 0; i < (size_t)k * host_tracks; ++i) *mismatches += dev_codes[i] != host_codes[i];
            for (const RgFpPair &p : host_pairs) *mismatches += memcmp(&dev_rec[p.rec], &host_rec[p.rec], sizeof(rg_fingerprint_pair_record)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_fingerprint_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_match) (void)hipFree(d_match);
    if (d_sums) (void)hipFree(d_sums);
    if (d_codes) (void)hipFree(d_codes);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
