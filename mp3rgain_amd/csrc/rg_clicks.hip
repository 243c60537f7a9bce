// rg_clicks.hip -- the click scan on the device (include/mp3rgain_amd_clicks.h, rg_clicks.h): every plane of the analysis arena,
// in any of its three formats, predicted block by block by the FLAC encoder's model, and the samples whose residual stands far
// above the median residual around them gathered into events.
//
//   rg_ck_tile_kernel  one workgroup per tile of one plane, found in a tile -> plane table: a run of whole blocks, and one block of
//                      margin on either side, so that the medians of the neighbouring blocks and the history of the first sample
//                      are the workgroup's own.  q goes into LDS once, as 16-bit values.  The windowed signal, then its exact
//                      autocorrelation (a lane takes 32 samples of one block and adds its 64-bit partial sums into the block's in
//                      LDS); then ONE LANE PER BLOCK runs the short recursion and the quantisation, all blocks of the span side
//                      by side; the residuals; the lower median of every block by a radix select in LDS (6 passes of 5 bits over
//                      all blocks at once, exact); the flags, a lane a run of consecutive samples, and the runs' event sums
//                      combined in order by a tree.  One 80-byte record per tile.
//   rg_ck_fold_kernel  one workgroup per plane: a lane folds a run of consecutive tile records, lane 0 the lanes' runs in order.
//                      It also counts the events that start before every tile and lists the tiles in which one of the plane's
//                      first max_events events starts.
//   rg_ck_emit_kernel  one workgroup per listed tile: the tile's residuals and medians again, and one lane writes the events that
//                      start in it into the plane's max_events slots, following an event beyond the tile by the tile records.
//                      Nothing on the device grows with max_events x tiles.
// The arithmetic is rg_clicks.h's, the very code the host routes run.  The launcher's callers check every track against the arena.
#include <string.h>

#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_clicks.h"
#include "rg_ctx.h"
#include "rg_pcm_seam.h"

// the workgroup as an executor of rg_clicks.h
struct CkLanes {
    __device__ uint32_t tid() const { return threadIdx.x; }
    __device__ uint32_t nt() const { return blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void add32(uint32_t *p, uint32_t v) const { atomicAdd(p, v); }
    __device__ void max32(uint32_t *p, uint32_t v) const { atomicMax(p, v); }
    __device__ void add64(int64_t *p, int64_t v) const { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }
};

__global__ __launch_bounds__(RG_CK_LANES) void rg_ck_tile_kernel(const unsigned char *__restrict__ arena, const RgCkPlane *__restrict__ planes,
                                                                const uint32_t *__restrict__ tile_plane, rg_clicks_opts o, RgCkTile *__restrict__ recs) {
    __shared__ RgCkWork w;
    CkLanes x;
    const RgCkPlane pl = planes[tile_plane[blockIdx.x]];
    rg_ck_tile(x, w, arena + pl.off, pl, o, (uint32_t)(blockIdx.x - pl.first_tile), &recs[blockIdx.x], nullptr, 0u, nullptr);
}

// the fold's way of listing a tile: its number among the launch's tiles into the next free place
struct CkList {
    uint32_t *list, *count;
    uint32_t first_tile;
    __device__ void operator()(uint32_t t) const { list[atomicAdd(count, 1u)] = first_tile + t; }
};

__global__ __launch_bounds__(RG_CK_FOLD_LANES) void rg_ck_fold_kernel(const RgCkPlane *__restrict__ planes, rg_clicks_opts o, const RgCkTile *__restrict__ recs,
                                                                     uint32_t *__restrict__ tile_first, RgCkTile *__restrict__ out, uint32_t *__restrict__ list,
                                                                     uint32_t *__restrict__ count) {
    __shared__ RgCkFoldWork w;
    CkLanes x;
    const RgCkPlane pl = planes[blockIdx.x];
    CkList emit{list, count, (uint32_t)pl.first_tile};
    rg_ck_fold(x, w, pl, o, recs + pl.first_tile, tile_first + pl.first_tile, &out[blockIdx.x], emit);
}

__global__ __launch_bounds__(RG_CK_LANES) void rg_ck_emit_kernel(const unsigned char *__restrict__ arena, const RgCkPlane *__restrict__ planes,
                                                                const uint32_t *__restrict__ tile_plane, rg_clicks_opts o, const RgCkTile *__restrict__ recs,
                                                                const uint32_t *__restrict__ tile_first, const uint32_t *__restrict__ list, RgCkEv *__restrict__ ev) {
    __shared__ RgCkWork w;
    CkLanes x;
    const uint32_t tile = list[blockIdx.x], pi = tile_plane[tile];
    const RgCkPlane pl = planes[pi];
    rg_ck_tile(x, w, arena + pl.off, pl, o, (uint32_t)(tile - pl.first_tile), nullptr, recs + pl.first_tile, tile_first[tile], ev + (size_t)pi * o.max_events);
}

// Device layout of one launch's bookkeeping, every part 16-byte aligned:
// [plane records | tile -> plane | tile records | events before a tile | listed tiles | their count | per-plane results | event slots]
struct CkLayout {
    size_t tmap, recs, first, list, count, res, ev, end;
};
static CkLayout ck_layout(size_t n, uint64_t n_tiles, uint32_t K) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    CkLayout l;
    l.tmap = a16(n * sizeof(RgCkPlane));
    l.recs = a16(l.tmap + (size_t)n_tiles * sizeof(uint32_t));
    l.first = a16(l.recs + (size_t)n_tiles * sizeof(RgCkTile));
    l.list = a16(l.first + (size_t)n_tiles * sizeof(uint32_t));
    l.count = a16(l.list + (size_t)n_tiles * sizeof(uint32_t));
    l.res = l.count + 16;
    l.ev = a16(l.res + n * sizeof(RgCkTile));
    l.end = a16(l.ev + n * K * sizeof(RgCkEv)) + 16;
    return l;
}
// the head of the bookkeeping as the host builds it: the planned records and the table
static void ck_head(const RgCkPlane *planes, size_t n, const CkLayout &l, std::vector<unsigned char> *head) {
    head->assign(l.recs, 0);
    if (n) memcpy(head->data(), planes, n * sizeof(RgCkPlane));
    uint32_t *tmap = reinterpret_cast<uint32_t *>(head->data() + l.tmap);
    for (size_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < planes[i].n_tiles; ++k) tmap[planes[i].first_tile + k] = (uint32_t)i;
}

struct CkPtrs {
    const RgCkPlane *planes;
    const uint32_t *tmap;
    RgCkTile *recs, *res;
    uint32_t *first, *list, *count;
    RgCkEv *ev;
};
static CkPtrs ck_ptrs(unsigned char *d, const CkLayout &l) {
    return CkPtrs{reinterpret_cast<const RgCkPlane *>(d), reinterpret_cast<const uint32_t *>(d + l.tmap), reinterpret_cast<RgCkTile *>(d + l.recs),
                  reinterpret_cast<RgCkTile *>(d + l.res), reinterpret_cast<uint32_t *>(d + l.first), reinterpret_cast<uint32_t *>(d + l.list),
                  reinterpret_cast<uint32_t *>(d + l.count), reinterpret_cast<RgCkEv *>(d + l.ev)};
}

int rg_ck_device(rg_ctx *c, const unsigned char *d_arena, RgCkPlane *planes, size_t n, const rg_clicks_opts &o, RgCkTile *po, RgCkEv *ev, hipStream_t s) {
    if (!n) return RG_OK;
    const uint64_t n_tiles = rg_ck_plan(planes, n);
    if (n > 0x7fffffffu || n_tiles > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu planes, %llu tiles", n, (unsigned long long)n_tiles);
    const uint32_t K = o.max_events;
    const CkLayout l = ck_layout(n, n_tiles, K);
    std::vector<unsigned char> head;
    ck_head(planes, n, l, &head);
    RG_HIP(c, c->d_clicks.reserve(l.end));
    unsigned char *d = c->d_clicks.p;
    const CkPtrs p = ck_ptrs(d, l);
    uint32_t listed = 0;
    const auto run = [&]() -> int {
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemsetAsync(d + l.count, 0, l.end - l.count, s));
        if (n_tiles) {
            hipLaunchKernelGGL(rg_ck_tile_kernel, dim3((uint32_t)n_tiles), dim3(RG_CK_LANES), 0, s, d_arena, p.planes, p.tmap, o, p.recs);
            RG_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(rg_ck_fold_kernel, dim3((uint32_t)n), dim3(RG_CK_FOLD_LANES), 0, s, p.planes, o, p.recs, p.first, p.res, p.list, p.count);
        RG_HIP(c, hipGetLastError());
        RG_HIP(c, hipMemcpyAsync(&listed, p.count, sizeof listed, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        if (listed > n_tiles) return rg_set_err(c, RG_ERR_DEVICE, "clicks: %u tiles listed of %llu", listed, (unsigned long long)n_tiles);
        if (listed) {
            hipLaunchKernelGGL(rg_ck_emit_kernel, dim3(listed), dim3(RG_CK_LANES), 0, s, d_arena, p.planes, p.tmap, o, p.recs, p.first, p.list, p.ev);
            RG_HIP(c, hipGetLastError());
        }
        RG_HIP(c, hipMemcpyAsync(po, p.res, n * sizeof(RgCkTile), hipMemcpyDeviceToHost, s));
        if (K) RG_HIP(c, hipMemcpyAsync(ev, p.ev, n * K * sizeof(RgCkEv), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        return RG_OK;
    };
    const int rc = run();
    if (rc != RG_OK) (void)hipStreamSynchronize(s);  // (`head` and `listed` may be on their way)
    return rc;
}

// ---- test seam (include/mp3rgain_amd_clicks.h) -----------------------------------------------------------------------------
extern "C" int rg_clicks_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_clicks_opts *opts, const void *arena, size_t arena_bytes,
                               rg_clicks_result *out, rg_clicks_event *events) {
    std::vector<RgCkPlane> planes;
    std::vector<size_t> first;
    rg_clicks_opts o;
    const auto host = [&](char *err, size_t err_len) { return rg_ck_arena_host(route, n, descs, opts, arena, arena_bytes, out, events, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_ck_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        planes = std::vector<RgCkPlane>(n * RG_CK_MAX_CHANNELS + 1);
        first.assign(n + 1, 0);
        size_t n_planes = 0;
        for (size_t i = 0; i < n; ++i) {
            rc = rg_ck_track_planes(i, descs[i], o, arena_bytes, &planes[n_planes], err, err_len);
            if (rc != RG_OK) return rc;
            first[i] = n_planes;
            n_planes += descs[i].channels;
        }
        first[n] = n_planes;
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        const size_t n_planes = first[n];
        const uint32_t K = o.max_events;
        std::vector<RgCkTile> po(n_planes + 1);
        std::vector<RgCkEv> ev(n_planes * K + 1);
        const int rc = rg_ck_device(c, c->d_arena.p, planes.data(), n_planes, o, po.data(), ev.data(), s);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) rg_ck_fill(descs[i], o, 0, &po[first[i]], &ev[first[i] * K], &out[i], events ? events + i * K : nullptr);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_clicks_arena", "the kernels' code", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/clicks_rate.py) -------------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, or 32-bit integers; word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_ck_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.001f / 2147483648.0f)) : u;
    }
}

extern "C" int rg_clicks_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, const rg_clicks_opts *opts, size_t host_tracks, uint32_t threads,
                              uint32_t reps, double warm_ms, double *scan_ms, double *fold_ms, double *emit_ms, double *host_ms, size_t *mismatches,
                              uint64_t *bytes, uint64_t *macs) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || format > RG_FMT_S32_PLANAR || !reps || !scan_ms || !fold_ms || !emit_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_clicks_rate: bad arguments");
    rg_clicks_opts o;
    char oerr[256] = "";
    int rc = rg_ck_options(opts, &o, oerr, sizeof oerr);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", oerr);
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_bps(format), K = o.max_events;
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    if (bytes) *bytes = (uint64_t)n * track_bytes;
    if (macs) *macs = (uint64_t)n * 2u * frames * (2u * o.order + 1u);
    unsigned char *d_arena = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        const size_t n_planes = 2 * n;
        std::vector<RgCkPlane> planes(n_planes);
        std::vector<rg_track_desc> descs(n);
        char err[256] = "";
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc &t = descs[i];
            memset(&t, 0, sizeof t);
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)format;
            if (rg_ck_track_planes(i, t, o, total, &planes[2 * i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_clicks_rate: %s", err);
        }
        const uint64_t n_tiles = rg_ck_plan(planes.data(), n_planes);
        if (n_planes > 0x7fffffffu || n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_clicks_rate: too many tiles");
        const CkLayout l = ck_layout(n_planes, n_tiles, K);
        std::vector<unsigned char> head;
        ck_head(planes.data(), n_planes, l, &head);
        RG_HIP(c, hipMalloc((void **)&d_arena, total + 16));
        RG_HIP(c, hipMalloc((void **)&d, l.end));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_ck_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemsetAsync(d + l.recs, 0, l.end - l.recs, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const CkPtrs p = ck_ptrs(d, l);
        uint32_t listed = 0;
        const auto scan_leg = [&]() -> int {
            hipLaunchKernelGGL(rg_ck_tile_kernel, dim3((uint32_t)n_tiles), dim3(RG_CK_LANES), 0, s, d_arena, p.planes, p.tmap, o, p.recs);
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        const auto fold_leg = [&]() -> int {
            RG_HIP(c, hipMemsetAsync(d + l.count, 0, 16, s));
            hipLaunchKernelGGL(rg_ck_fold_kernel, dim3((uint32_t)n_planes), dim3(RG_CK_FOLD_LANES), 0, s, p.planes, o, p.recs, p.first, p.res, p.list, p.count);
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        const auto emit_leg = [&]() -> int {
            if (!listed) return RG_OK;
            hipLaunchKernelGGL(rg_ck_emit_kernel, dim3(listed), dim3(RG_CK_LANES), 0, s, d_arena, p.planes, p.tmap, o, p.recs, p.first, p.list, p.ev);
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        // one timed leg: HIP events around the launches alone
        const auto timed = [&](const auto &launch, double *ms_out) -> int {
            float ms = 0.0f;
            RG_HIP(c, hipEventRecord(e0, s));
            const int r = launch();
            if (r != RG_OK) return r;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            *ms_out = ms;
            return RG_OK;
        };
        const auto round = [&](double *a, double *b, double *e) -> int {
            int r;
            if ((r = timed(scan_leg, a)) != RG_OK || (r = timed(fold_leg, b)) != RG_OK) return r;
            RG_HIP(c, hipMemcpyAsync(&listed, p.count, sizeof listed, hipMemcpyDeviceToHost, s));
            RG_HIP(c, hipStreamSynchronize(s));
            if (listed > n_tiles) return rg_set_err(c, RG_ERR_DEVICE, "rg_clicks_rate: %u tiles listed of %llu", listed, (unsigned long long)n_tiles);
            return timed(emit_leg, e);
        };
        std::vector<rg_clicks_result> host_res(host_tracks ? host_tracks : 1), dev_res(host_tracks ? host_tracks : 1);
        std::vector<rg_clicks_event> host_ev((host_tracks ? host_tracks : 1) * (size_t)K + 1), dev_ev((host_tracks ? host_tracks : 1) * (size_t)K + 1);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                std::vector<RgCkEv> ev(2 * (size_t)K + 1);
                for (size_t i = next.fetch_add(1); i < host_tracks; i = next.fetch_add(1)) {
                    RgCkTile po[2];
                    for (uint32_t ch = 0; ch < 2; ++ch) po[ch] = rg_ck_serial_host(h.data(), planes[2 * i + ch], o, &ev[(size_t)ch * K]);
                    rg_ck_fill(descs[i], o, 0, po, ev.data(), &host_res[i], &host_ev[i * K]);
                }
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        int lr;
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            double a, b, e;
            if ((lr = round(&a, &b, &e)) != RG_OK) return lr;
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            if ((lr = round(&scan_ms[r], &fold_ms[r], &emit_ms[r])) != RG_OK) return lr;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            std::vector<RgCkTile> po(2 * host_tracks);
            std::vector<RgCkEv> ev(2 * host_tracks * (size_t)K + 1);
            RG_HIP(c, hipMemcpyAsync(po.data(), p.res, po.size() * sizeof(RgCkTile), hipMemcpyDeviceToHost, s));
            if (K) RG_HIP(c, hipMemcpyAsync(ev.data(), p.ev, 2 * host_tracks * (size_t)K * sizeof(RgCkEv), hipMemcpyDeviceToHost, s));
            RG_HIP(c, hipStreamSynchronize(s));
            *mismatches = 0;
            for (size_t i = 0; i < host_tracks; ++i) {
                rg_ck_fill(descs[i], o, 0, &po[2 * i], &ev[2 * i * K], &dev_res[i], &dev_ev[i * K]);
                *mismatches += (memcmp(&dev_res[i], &host_res[i], sizeof(rg_clicks_result)) != 0 || (K && memcmp(&dev_ev[i * K], &host_ev[i * K], K * sizeof(rg_clicks_event)) != 0)) ? 1 : 0;
            }
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_clicks_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
