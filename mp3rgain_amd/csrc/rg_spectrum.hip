// rg_spectrum.hip -- the spectral scan on the device (include/mp3rgain_amd_spectrum.h, rg_spectrum.h): per plane the energy in
// 256 bands of a short-time Fourier transform (frames of 4096 samples, hop 2048, periodic Hann), from the planes of the analysis
// arena in any of its three formats.
//
//   rg_spec_tiles_kernel  one block of 256 lanes per run of RG_SPEC_TILE_FRAMES consecutive frames of one plane, many planes per
//                         launch, one launch per format; the block finds its plane in a tile -> plane table.  Frames are
//                         transformed two at a time, as the real and imaginary part of one 4096-point complex transform: three
//                         radix-16 passes in registers (rg_spectrum.h) with two exchanges through 38 KB of LDS.  A lane's 16
//                         points of pass 1 lie 256 samples apart, so a wave reads 64 consecutive samples with every load: the
//                         plane is read where it lies, element by element, with no alignment to respect and nothing outside
//                         the plane touched; the half a pair's two frames share is loaded once, and the hop two pairs share
//                         comes from the cache the second time.  The exchange buffer is [k0][k1 or n1][n0] with 18 complex per
//                         row of 16 and 306 per k0: pass 2 reads and writes its own 16 places (no barrier between), pass 3 reads 16
//                         contiguous complex per lane with 16-byte reads whose lanes lie 36 (mod 64) dwords apart.  Z goes back
//                         in natural order, one bump per eight bins; lane j separates the two spectra over band j's bins, sums
//                         the eight powers of each in f32 and adds them to its double accumulator in frame order.  A frame of
//                         a float plane with a NaN or Inf goes in as zeros and is not added.  One record of 256 doubles per
//                         tile.
//   rg_spec_fold_kernel   one block of 256 lanes per plane: lane j adds band j of the plane's tile records in tile order.
// No atomics, no transcendental in the kernels, and this unit is compiled without contraction: same input, same bits as the host's
// route 2.  The launcher's callers check every plane against the arena first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_pcm_seam.h"
#include "rg_spectrum.h"

#define RG_SPEC_ROW 18u    // complex per row of 16 in the exchange buffer
#define RG_SPEC_K0 306u    // complex per k0: 16 rows and 18 more, 612 dwords = 36 (mod 64)
#define RG_SPEC_LDS (16u * RG_SPEC_K0)

// where Z[k] lies after pass 3: natural order with one complex of padding per eight bins, so that the band lanes' runs of eight
// start 18 dwords apart
__device__ __forceinline__ uint32_t spec_pos(uint32_t k) { return k + ((k + 7u) >> 3); }

template <int FMT>
__device__ __forceinline__ uint32_t spec_load(const unsigned char *plane, uint64_t k) {
    if (FMT == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(plane)[k];
    return reinterpret_cast<const uint32_t *>(plane)[k];
}

template <int FMT>
__global__ __launch_bounds__(RG_SPEC_BLOCK) void rg_spec_tiles_kernel(const unsigned char *__restrict__ arena, const RgSpecTables *__restrict__ tables,
                                                                      const RgSpecPlane *__restrict__ planes, const uint32_t *__restrict__ tile_plane,
                                                                      uint64_t tile_base, double *__restrict__ tile_out, uint32_t *__restrict__ tile_skipped) {
    __shared__ __attribute__((aligned(16))) RgSpecC s_x[RG_SPEC_LDS];
    const uint32_t tid = threadIdx.x, hi = tid >> 4, lo = tid & 15u;
    const uint64_t tile = tile_base + blockIdx.x;
    const RgSpecPlane &p = planes[tile_plane[tile]];
    const unsigned char *plane = arena + p.off;
    const uint32_t f0 = (uint32_t)(tile - p.first_tile) * RG_SPEC_TILE_FRAMES;
    const uint32_t left = p.frames - f0, nf = left < RG_SPEC_TILE_FRAMES ? left : RG_SPEC_TILE_FRAMES;
    float win[16];
#pragma unroll
    for (uint32_t n2 = 0; n2 < 16; ++n2) win[n2] = tables->window[256u * n2 + tid];
    double acc = 0.0;
    uint32_t skipped = 0;
    for (uint32_t pr = 0; pr < nf; pr += 2) {
        const bool has_b = pr + 1 < nf;
        const uint64_t at = (uint64_t)(f0 + pr) * RG_SPEC_HOP + tid;
        // samples at, at + 256, ...: frame a takes the first 16, frame b the last 16 of 24
        uint32_t raw[24];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) raw[i] = spec_load<FMT>(plane, at + 256u * i);
#pragma unroll
        for (uint32_t i = 16; i < 24; ++i) raw[i] = has_b ? spec_load<FMT>(plane, at + 256u * i) : 0u;
        bool use_a = true, use_b = has_b;
        if (FMT == RG_FMT_F32_PLANAR) {
            int bad_a = 0, bad_b = 0;
#pragma unroll
            for (uint32_t i = 0; i < 24; ++i) {
                const int bad = rg_spec_nonfinite<FMT>(raw[i]) ? 1 : 0;
                if (i < 16) bad_a |= bad;
                if (i >= 8) bad_b |= bad;
            }
            bad_a = __syncthreads_or(bad_a);
            bad_b = __syncthreads_or(bad_b);
            use_a = !bad_a;
            use_b = has_b && !bad_b;
            skipped += (bad_a ? 1u : 0u) + (has_b && bad_b ? 1u : 0u);
        }
        RgSpecC v[16];
#pragma unroll
        for (uint32_t n2 = 0; n2 < 16; ++n2) {
            v[n2].x = use_a ? rg_spec_value<FMT>(raw[n2]) * win[n2] : 0.0f;
            v[n2].y = use_b ? rg_spec_value<FMT>(raw[n2 + 8]) * win[n2] : 0.0f;
        }
        rg_spec_pass1(v, tid, tables->tw1);  // lane = 16 n1 + n0
#pragma unroll
        for (uint32_t k0 = 0; k0 < 16; ++k0) s_x[k0 * RG_SPEC_K0 + hi * RG_SPEC_ROW + lo] = v[k0];
        __syncthreads();
        {  // pass 2: lane = 16 k0 + n0, in its own 16 places
            RgSpecC *col = s_x + hi * RG_SPEC_K0 + lo;
#pragma unroll
            for (uint32_t n1 = 0; n1 < 16; ++n1) v[n1] = col[n1 * RG_SPEC_ROW];
            rg_spec_pass2(v, lo, tables->tw2);
#pragma unroll
            for (uint32_t k1 = 0; k1 < 16; ++k1) col[k1 * RG_SPEC_ROW] = v[k1];
        }
        __syncthreads();
        {  // pass 3: lane = 16 k1 + k0
            const float4 *row = reinterpret_cast<const float4 *>(s_x + lo * RG_SPEC_K0 + hi * RG_SPEC_ROW);
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
        for (uint32_t k2 = 0; k2 < 16; ++k2) s_x[spec_pos(tid + 256u * k2)] = v[k2];
        __syncthreads();
        float sa, sb;
        rg_spec_band([&](uint32_t k) { return s_x[spec_pos(k)]; }, tid, &sa, &sb);
        if (use_a) acc += (double)sa;
        if (use_b) acc += (double)sb;
        __syncthreads();  // the bands have been read: the next pair's pass 1 may write
    }
    tile_out[tile * RG_SPEC_BANDS + tid] = acc;
    if (tid == 0) tile_skipped[tile] = skipped;
}

__global__ __launch_bounds__(RG_SPEC_BLOCK) void rg_spec_fold_kernel(const RgSpecPlane *__restrict__ planes, const double *__restrict__ tile_in,
                                                                     const uint32_t *__restrict__ tile_skipped, RgSpecPlaneOut *__restrict__ out) {
    const uint32_t tid = threadIdx.x;
    const RgSpecPlane &p = planes[blockIdx.x];
    const uint64_t first = p.first_tile;
    double e = 0.0;
    for (uint32_t t = 0; t < p.n_tiles; ++t) e += tile_in[(first + t) * RG_SPEC_BANDS + tid];
    out[blockIdx.x].E[tid] = e;
    if (tid == 0) {
        uint32_t skipped = 0;
        for (uint32_t t = 0; t < p.n_tiles; ++t) skipped += tile_skipped[first + t];
        out[blockIdx.x].analysed = p.frames - skipped;
        out[blockIdx.x].skipped = skipped;
        out[blockIdx.x].reserved[0] = out[blockIdx.x].reserved[1] = 0u;
    }
}

// ---- one call's launches ---------------------------------------------------------------------------------------------------
// The planes are cut into runs whose tile records fit RG_SPEC_MAX_LAUNCH_TILES (a run holds at least one plane), so the tile
// records of 1000 long tracks take 64 MiB and not 0.5 GB: the runs are launched one after the other on one stream and share
// the records' memory.  Device layout, every part 16-byte aligned:
//   [tables | per run: plane records, tile -> plane | tile records | skipped counts | per-plane results]
struct SpecRun {
    size_t first, count;  // planes
    uint64_t fmt_tile[4];
    size_t planes_at, map_at;
};
struct SpecJob {
    std::vector<SpecRun> runs;
    std::vector<unsigned char> head;  // the device buffer's bytes [0, tiles_at)
    size_t tiles_at, skipped_at, res_at, end;
};
static size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

static void spec_job(RgSpecPlane *planes, size_t n, SpecJob *job) {
    job->runs.clear();
    size_t at = a16(sizeof(RgSpecTables));
    uint64_t most = 0;
    for (size_t i = 0; i < n;) {
        SpecRun r;
        r.first = i;
        uint64_t tiles = 0;
        do {
            const uint64_t t = (planes[i].frames + RG_SPEC_TILE_FRAMES - 1) / RG_SPEC_TILE_FRAMES;
            if (i > r.first && tiles + t > RG_SPEC_MAX_LAUNCH_TILES) break;
            tiles += t;
            ++i;
        } while (i < n);
        r.count = i - r.first;
        (void)rg_spec_plan(planes + r.first, r.count, r.fmt_tile);
        r.planes_at = at;
        r.map_at = a16(at + r.count * sizeof(RgSpecPlane));
        at = a16(r.map_at + (size_t)tiles * sizeof(uint32_t));
        most = std::max(most, tiles);
        job->runs.push_back(r);
    }
    job->tiles_at = at;
    job->skipped_at = a16(job->tiles_at + (size_t)most * RG_SPEC_BANDS * sizeof(double));
    job->res_at = a16(job->skipped_at + (size_t)most * sizeof(uint32_t));
    job->end = a16(job->res_at + n * sizeof(RgSpecPlaneOut));
    job->head.assign(job->tiles_at, 0);
    memcpy(job->head.data(), &rg_spec_tables(), sizeof(RgSpecTables));
    for (const SpecRun &r : job->runs) {
        memcpy(job->head.data() + r.planes_at, planes + r.first, r.count * sizeof(RgSpecPlane));
        uint32_t *map = reinterpret_cast<uint32_t *>(job->head.data() + r.map_at);
        for (size_t i = 0; i < r.count; ++i) {
            const RgSpecPlane &p = planes[r.first + i];
            for (uint32_t t = 0; t < p.n_tiles; ++t) map[p.first_tile + t] = (uint32_t)i;
        }
    }
}

template <int FMT>
static void spec_launch_format(const unsigned char *d_arena, unsigned char *d, const SpecJob &job, const SpecRun &r, uint64_t base, uint64_t count,
                               hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL((rg_spec_tiles_kernel<FMT>), dim3((uint32_t)count), dim3(RG_SPEC_BLOCK), 0, s, d_arena, reinterpret_cast<const RgSpecTables *>(d),
                       reinterpret_cast<const RgSpecPlane *>(d + r.planes_at), reinterpret_cast<const uint32_t *>(d + r.map_at), base,
                       reinterpret_cast<double *>(d + job.tiles_at), reinterpret_cast<uint32_t *>(d + job.skipped_at));
}

static int spec_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const SpecJob &job, hipStream_t s) {
    for (const SpecRun &r : job.runs) {
        spec_launch_format<RG_FMT_F32_PLANAR>(d_arena, d, job, r, r.fmt_tile[0], r.fmt_tile[1] - r.fmt_tile[0], s);
        spec_launch_format<RG_FMT_S16_PLANAR>(d_arena, d, job, r, r.fmt_tile[1], r.fmt_tile[2] - r.fmt_tile[1], s);
        spec_launch_format<RG_FMT_S32_PLANAR>(d_arena, d, job, r, r.fmt_tile[2], r.fmt_tile[3] - r.fmt_tile[2], s);
        RG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(rg_spec_fold_kernel, dim3((uint32_t)r.count), dim3(RG_SPEC_BLOCK), 0, s, reinterpret_cast<const RgSpecPlane *>(d + r.planes_at),
                           reinterpret_cast<const double *>(d + job.tiles_at), reinterpret_cast<const uint32_t *>(d + job.skipped_at),
                           reinterpret_cast<RgSpecPlaneOut *>(d + job.res_at) + r.first);
        RG_HIP(c, hipGetLastError());
    }
    return RG_OK;
}

int rg_spectrum_device(rg_ctx *c, const unsigned char *d_arena, RgSpecPlane *planes, size_t n, RgSpecPlaneOut *out, hipStream_t s) {
    if (!n) return RG_OK;
    if (n > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one call: %zu planes", n);
    SpecJob job;
    spec_job(planes, n, &job);
    RG_HIP(c, c->d_spectrum.reserve(job.end));
    unsigned char *d = c->d_spectrum.p;
    RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
    const int rc = spec_launch(c, d_arena, d, job, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(out, d + job.res_at, n * sizeof(RgSpecPlaneOut), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_spectrum.h) ---------------------------------------------------------------------------
extern "C" int rg_spectrum_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_spectrum_opts *opts, const void *arena,
                                 size_t arena_bytes, rg_spectrum_result *out, double *bands_out) {
    rg_spectrum_opts o;
    std::vector<RgSpecPlane> planes;
    size_t n_planes = 0;
    const auto host = [&](char *err, size_t err_len) { return rg_spec_arena_host(route, n, descs, opts, arena, arena_bytes, out, bands_out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_spec_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        planes = std::vector<RgSpecPlane>(n * RG_SPEC_MAX_CHANNELS + 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_spec_track_planes(i, descs[i], arena_bytes, &planes[n_planes], err, err_len);
            if (rc != RG_OK) return rc;
            n_planes += descs[i].channels;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        std::vector<RgSpecPlaneOut> po(n_planes ? n_planes : 1);
        const int rc = rg_spectrum_device(c, c->d_arena.p, planes.data(), n_planes, po.data(), s);
        if (rc != RG_OK) return rc;
        if (!n_planes) RG_HIP(c, hipStreamSynchronize(s));
        size_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_spec_fill(descs[i], 0, &po[at], o, &out[i], bands_out ? bands_out + i * RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS : nullptr);
            at += descs[i].channels;
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_spectrum_arena", "the kernels' arithmetic", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/spectrum_rate.py) ------------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, 32-bit integers, or floats in [-1, 1); word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_spec_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.0f / 2147483648.0f)) : u;
    }
}

extern "C" int rg_spectrum_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                                double *kernel_ms, double *host_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || format > RG_FMT_S32_PLANAR || !reps || !kernel_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_spectrum_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_width(format) / 8;
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgSpecPlane> planes(2 * n);
        char err[256] = "";
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)format;
            if (rg_spec_track_planes(i, t, total, &planes[2 * i], err, sizeof err) != RG_OK)
                return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_spectrum_rate: %s", err);
        }
        SpecJob job;
        spec_job(planes.data(), planes.size(), &job);
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d, job.end));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_spec_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, job.head.data(), job.head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<RgSpecPlaneOut> host_out(host_tracks ? 2 * host_tracks : 1), dev_out(2 * host_tracks ? 2 * host_tracks : 1);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < 2 * host_tracks; i = next.fetch_add(1)) rg_spec_folded_host(h.data(), planes[i], &host_out[i]);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            const int lr = spec_launch(c, d_arena, d, job, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        if (host_tracks) host_pass();
        for (uint32_t r = 0; r < reps; ++r) {
            float ms = 0.0f;
            RG_HIP(c, hipEventRecord(e0, s));
            const int lr = spec_launch(c, d_arena, d, job, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            kernel_ms[r] = ms;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            RG_HIP(c, hipMemcpy(dev_out.data(), d + job.res_at, 2 * host_tracks * sizeof(RgSpecPlaneOut), hipMemcpyDeviceToHost));
            *mismatches = 0;
            for (size_t i = 0; i < 2 * host_tracks; ++i) *mismatches += memcmp(&dev_out[i], &host_out[i], sizeof(RgSpecPlaneOut)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_spectrum_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
