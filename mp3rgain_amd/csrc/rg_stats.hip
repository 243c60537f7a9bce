// rg_stats.hip -- the PCM defect scan on the device (include/mp3rgain_amd_stats.h, rg_stats.h): per plane the clipped samples
// and clip runs, the zero runs inside the audio and at its edges, the sum, the OR of the bit patterns, minimum and maximum, from
// the planes of the analysis arena in any of its three formats.
//
// A plane is cut into chunks of RG_STATS_CHUNK samples, every chunk walked by its own lane and the lanes' parts folded in order
// (rg_stats.h says what a part keeps so that stretches survive the cuts).  Chunks and tiles are counted from the plane's first
// sample; only the last of each is short, and a missing one is the empty part.
//
//   rg_stats_tiles_kernel  one block per tile of RG_STATS_BLOCK chunks, many planes per launch, one launch per format; the block
//                          finds its plane in a tile -> plane table.  It stages its stretch of the plane into LDS with aligned
//                          16-byte loads, coalesced across the wave -- the aligned cover may reach up to 15 bytes outside the
//                          plane on either side, never outside the arena's allocation of whole 16-byte words, and what it holds
//                          beyond the plane is never read back (the vector two tiles share is the only one fetched twice) --
//                          skewed by one dword per chunk so that the lanes, whose chunks lie a power of two apart, walk
//                          different banks.  Each lane walks its chunk from LDS (rg_stats_chunk), and a fixed tree over LDS
//                          folds the 256 parts (rg_stats_combine), which lie there at an odd stride in dwords.  One 96-byte record per tile.
//   rg_stats_fold_kernel   one block (a wave) per plane: each lane folds a run of `run` tile records in order, then the same
//                          tree, then the plane's ends are closed (rg_stats_finish).
// No atomics, and the only floating point is exact (a float scaled by 2^23 and rounded): same input, same bits.  The launcher's
// callers check every plane against the arena first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_pcm_seam.h"
#include "rg_rip.h"
#include "rg_stats.h"

template <int FMT>
struct StatsLds {
    static constexpr uint32_t bps = FMT == RG_FMT_S16_PLANAR ? 2u : 4u;
    static constexpr uint32_t skew_shift = FMT == RG_FMT_S16_PLANAR ? 4u : 5u;  // log2 of a chunk's dwords
    static constexpr uint32_t win_dwords = bps * RG_STATS_TILE / 4u + 8u;       // the aligned cover of a tile: at most 30 bytes more
    static constexpr uint32_t dwords = win_dwords + (win_dwords >> skew_shift) + 4u;
    static constexpr uint32_t part_bytes = RG_STATS_BLOCK * (uint32_t)(sizeof(RgStatsPart) + 4);  // StatsLdsPart
    static constexpr uint32_t bytes = 4u * dwords > part_bytes ? 4u * dwords : part_bytes;
    // LDS image of the cover: its dword d at d + (d >> skew_shift)
    static __device__ __forceinline__ uint32_t skew(uint32_t d) { return d + (d >> skew_shift); }
};

// A part in LDS: its 24 dwords and one of padding.  With the record's own 96-byte stride the lanes of a tree level meet on
// two banks (and on one from the second level on); an odd stride in dwords spreads neighbouring records over all of them.
struct StatsLdsPart {
    uint32_t w[sizeof(RgStatsPart) / 4 + 1];
};
__device__ __forceinline__ void stats_put(StatsLdsPart *v, uint32_t i, const RgStatsPart &p) { memcpy(v[i].w, &p, sizeof p); }
__device__ __forceinline__ RgStatsPart stats_get(const StatsLdsPart *v, uint32_t i) {
    RgStatsPart p;
    memcpy(&p, v[i].w, sizeof p);
    return p;
}

// the fixed tree: v[0] <- the fold of v[0 .. 2^levels) in order.  Level by level lane i folds records 2i and 2i + 1 and, when
// every lane has read, writes the result to record i: the records stay packed, so reads are 2 records and writes 1 record
// apart at every level, and the lanes that work are the first ones, so whole waves drop out as the levels go up.
__device__ __forceinline__ void rg_stats_tree(StatsLdsPart *v, uint32_t levels, uint32_t min_clip, uint32_t min_zero, uint32_t tid) {
    for (uint32_t j = 0; j < levels; ++j) {
        const bool works = tid < ((1u << levels) >> (j + 1));
        RgStatsPart a;
        __syncthreads();
        if (works) {
            a = stats_get(v, 2 * tid);
            rg_stats_combine(&a, stats_get(v, 2 * tid + 1), min_clip, min_zero);
        }
        __syncthreads();
        if (works) stats_put(v, tid, a);
    }
    __syncthreads();
}

template <int FMT, bool ANY>
__global__ __launch_bounds__(RG_STATS_BLOCK) void rg_stats_tiles_kernel(const unsigned char *__restrict__ arena, const RgStatsPlane *__restrict__ planes,
                                                                        const uint32_t *__restrict__ tile_plane, uint64_t tile_base, uint32_t min_clip,
                                                                        uint32_t min_zero, RgStatsPart *__restrict__ tile_out) {
    typedef StatsLds<FMT> L;
    // the cover and, once every lane has walked its chunk, the parts in the same LDS: 6 blocks a CU for S16, 4 for the 32-bit formats
    __shared__ uint4 s_raw[(L::bytes + 15u) / 16u];
    uint32_t *s_data = reinterpret_cast<uint32_t *>(s_raw);
    StatsLdsPart *s_part = reinterpret_cast<StatsLdsPart *>(s_raw);
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = tile_base + blockIdx.x;
    const RgStatsPlane &p = planes[tile_plane[tile]];  // (read field by field)
    const uint64_t off = p.off;
    const int32_t P = p.P, M = p.M;
    uint32_t wstart;
    const uint32_t wlen = rg_stats_tile_window(p.n, (uint32_t)(tile - p.first_tile), &wstart);
    // the aligned cover of [wstart, wstart + wlen) into s_data
    const uint64_t g0 = off + (uint64_t)L::bps * wstart, ab = g0 & ~(uint64_t)15;
    const uint32_t mis = (uint32_t)(g0 - ab) / L::bps;  // where the stretch begins in the cover, in samples
    const uint32_t nvec = ((uint32_t)(g0 - ab) + L::bps * wlen + 15u) / 16u;
    const uint4 *src = reinterpret_cast<const uint4 *>(arena + ab);
    for (uint32_t v = tid; v < nvec; v += RG_STATS_BLOCK) {
        const uint4 q = src[v];
        const uint32_t at = L::skew(4 * v);  // (4v .. 4v + 3 share one skew)
        s_data[at] = q.x;
        s_data[at + 1] = q.y;
        s_data[at + 2] = q.z;
        s_data[at + 3] = q.w;
    }
    __syncthreads();
    uint32_t a;
    const uint32_t n = rg_stats_lane_chunk(wlen, tid, &a);
    const uint32_t m = mis + a;
    RgStatsPart part;
    rg_stats_chunk<FMT, ANY>(
        [&](uint32_t j) -> uint32_t {
            const uint32_t s = m + j;  // sample s of the cover
            if (FMT == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t)(int16_t)(s_data[L::skew(s >> 1)] >> (16 * (s & 1u)));
            return s_data[L::skew(s)];
        },
        n, P, M, min_clip, min_zero, &part);
    __syncthreads();  // the cover has been read: the parts take its place
    stats_put(s_part, tid, part);
    rg_stats_tree(s_part, RG_STATS_LEVELS, min_clip, min_zero, tid);
    if (tid == 0) tile_out[tile] = stats_get(s_part, 0);
}

__global__ __launch_bounds__(RG_STATS_FOLD_LANES) void rg_stats_fold_kernel(const RgStatsPlane *__restrict__ planes, const RgStatsPart *__restrict__ tile_in,
                                                                            uint32_t min_clip, uint32_t min_zero, rg_pcm_stats_channel *__restrict__ out) {
    __shared__ StatsLdsPart s_part[RG_STATS_FOLD_LANES];
    const uint32_t tid = threadIdx.x;
    const RgStatsPlane &p = planes[blockIdx.x];
    const uint64_t first = p.first_tile;
    uint32_t lo;
    const uint32_t hi = rg_stats_lane_run(p.n_tiles, p.run, tid, &lo);
    RgStatsPart acc = rg_stats_empty();
    for (uint32_t t = lo; t < hi; ++t) rg_stats_combine(&acc, tile_in[first + t], min_clip, min_zero);
    stats_put(s_part, tid, acc);
    rg_stats_tree(s_part, RG_STATS_FOLD_LEVELS, min_clip, min_zero, tid);
    if (tid == 0) out[blockIdx.x] = rg_stats_finish(stats_get(s_part, 0), p.format, min_clip);
}

// Device layout of one launch's bookkeeping, every part 16-byte aligned: [plane records | tile -> plane | tile records | results]
struct StatsLayout {
    size_t map, tiles, res, end;
};
static StatsLayout stats_layout(size_t n, uint64_t n_tiles) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    StatsLayout l;
    l.map = a16(n * sizeof(RgStatsPlane));
    l.tiles = a16(l.map + (size_t)n_tiles * sizeof(uint32_t));
    l.res = a16(l.tiles + (size_t)n_tiles * sizeof(RgStatsPart));
    l.end = a16(l.res + n * sizeof(rg_pcm_stats_channel));
    return l;
}
// the head of the bookkeeping as the host builds it: the planned records and the table
static void stats_head(const RgStatsPlane *planes, size_t n, const StatsLayout &l, std::vector<unsigned char> *head) {
    head->assign(l.tiles, 0);
    if (n) memcpy(head->data(), planes, n * sizeof(RgStatsPlane));
    uint32_t *map = reinterpret_cast<uint32_t *>(head->data() + l.map);
    for (size_t i = 0; i < n; ++i)
        for (uint32_t t = 0; t < planes[i].n_tiles; ++t) map[planes[i].first_tile + t] = (uint32_t)i;
}

template <int FMT>
static void stats_launch_format(const unsigned char *d_arena, const RgStatsPlane *d_planes, const uint32_t *d_map, uint64_t base, uint64_t count,
                                const rg_pcm_stats_opts &o, bool any_test, RgStatsPart *d_tiles, hipStream_t s) {
    if (!count) return;
    if (any_test)
        hipLaunchKernelGGL((rg_stats_tiles_kernel<FMT, true>), dim3((uint32_t)count), dim3(RG_STATS_BLOCK), 0, s, d_arena, d_planes, d_map, base,
                           o.min_clip_run, o.min_zero_run, d_tiles);
    else
        hipLaunchKernelGGL((rg_stats_tiles_kernel<FMT, false>), dim3((uint32_t)count), dim3(RG_STATS_BLOCK), 0, s, d_arena, d_planes, d_map, base,
                           o.min_clip_run, o.min_zero_run, d_tiles);
}

static int stats_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const StatsLayout &l, size_t n, const uint64_t fmt_tile[4],
                        const rg_pcm_stats_opts &o, bool any_test, hipStream_t s) {
    const RgStatsPlane *d_planes = reinterpret_cast<const RgStatsPlane *>(d);
    const uint32_t *d_map = reinterpret_cast<const uint32_t *>(d + l.map);
    RgStatsPart *d_tiles = reinterpret_cast<RgStatsPart *>(d + l.tiles);
    stats_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_planes, d_map, fmt_tile[0], fmt_tile[1] - fmt_tile[0], o, any_test, d_tiles, s);
    stats_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_planes, d_map, fmt_tile[1], fmt_tile[2] - fmt_tile[1], o, any_test, d_tiles, s);
    stats_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_planes, d_map, fmt_tile[2], fmt_tile[3] - fmt_tile[2], o, any_test, d_tiles, s);
    RG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(rg_stats_fold_kernel, dim3((uint32_t)n), dim3(RG_STATS_FOLD_LANES), 0, s, d_planes, d_tiles, o.min_clip_run, o.min_zero_run,
                       reinterpret_cast<rg_pcm_stats_channel *>(d + l.res));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_stats_device(rg_ctx *c, const unsigned char *d_arena, RgStatsPlane *planes, size_t n, const rg_pcm_stats_opts &o, rg_pcm_stats_channel *ch,
                    hipStream_t s) {
    if (!n) return RG_OK;
    uint64_t fmt_tile[4];
    const uint64_t n_tiles = rg_stats_plan(planes, n, fmt_tile);
    if (n > 0x7fffffffu || n_tiles > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu planes, %llu tiles", n, (unsigned long long)n_tiles);
    const StatsLayout l = stats_layout(n, n_tiles);
    std::vector<unsigned char> head;
    stats_head(planes, n, l, &head);
    RG_HIP(c, c->d_stats.reserve(l.end));
    unsigned char *d = c->d_stats.p;
    RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    const int rc = stats_launch(c, d_arena, d, l, n, fmt_tile, o, RG_STATS_ANY_TEST != 0, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(ch, d + l.res, n * sizeof(rg_pcm_stats_channel), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- for other scans' rate hooks (rg_stats.h) ---------------------------------------------------------------------------------
int rg_stats_bench_setup(rg_ctx *c, RgStatsPlane *planes, size_t n, hipStream_t s, RgStatsBench *b) {
    const uint64_t n_tiles = rg_stats_plan(planes, n, b->fmt_tile);
    if (n > 0x7fffffffu || n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many tiles for one launch");
    const StatsLayout l = stats_layout(n, n_tiles);
    std::vector<unsigned char> head;
    stats_head(planes, n, l, &head);
    RG_HIP(c, hipMalloc((void **)&b->d, l.end));
    b->n = n;
    b->map = l.map;
    b->tiles = l.tiles;
    b->res = l.res;
    RG_HIP(c, hipMemcpyAsync(b->d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipStreamSynchronize(s));  // (`head` goes away)
    return RG_OK;
}
int rg_stats_bench_launch(rg_ctx *c, const unsigned char *d_arena, const RgStatsBench &b, hipStream_t s) {
    const StatsLayout l{b.map, b.tiles, b.res, 0};
    return stats_launch(c, d_arena, b.d, l, b.n, b.fmt_tile, rg_pcm_stats_opts{RG_STATS_MIN_CLIP_RUN, RG_STATS_MIN_ZERO_RUN}, RG_STATS_ANY_TEST != 0, s);
}
void rg_stats_bench_free(RgStatsBench *b) {
    if (b->d) (void)hipFree(b->d);
    b->d = nullptr;
}

// ---- test seam (include/mp3rgain_amd_stats.h) -------------------------------------------------------------------------------
extern "C" int rg_pcm_stats_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bits, const rg_pcm_stats_opts *opts,
                                  const void *arena, size_t arena_bytes, rg_pcm_stats_result *out) {
    rg_pcm_stats_opts o;
    std::vector<RgStatsPlane> planes;
    std::vector<uint32_t> reported;
    size_t n_planes = 0;
    const auto host = [&](char *err, size_t err_len) { return rg_stats_arena_host(route, n, descs, bits, opts, arena, arena_bytes, out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_stats_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        planes = std::vector<RgStatsPlane>(n * RG_STATS_MAX_CHANNELS + 1);
        reported = std::vector<uint32_t>(n ? n : 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_stats_track_planes(i, descs[i], bits ? bits[i] : rg_pcm_width(descs[i].format), arena_bytes, &planes[n_planes], &reported[i], err, err_len);
            if (rc != RG_OK) return rc;
            n_planes += descs[i].channels;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        std::vector<rg_pcm_stats_channel> ch(n_planes ? n_planes : 1);
        const int rc = rg_stats_device(c, c->d_arena.p, planes.data(), n_planes, o, ch.data(), s);
        if (rc != RG_OK) return rc;
        size_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_stats_fill(descs[i], reported[i], 0, &ch[at], &out[i]);
            at += descs[i].channels;
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_pcm_stats_arena", "folded", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/pcm_stats_rate.py) -----------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, or 32-bit integers; word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_stats_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        // floats in [-1.001, 1.001]: one in a thousand beyond full scale, as an MP3 that decodes hot has them
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.001f / 2147483648.0f)) : u;
    }
}

extern "C" int rg_pcm_stats_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, int any_test, size_t host_tracks, uint32_t threads, uint32_t reps,
                                 double warm_ms, double *stats_ms, double *rip_ms, double *host_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || format > RG_FMT_S32_PLANAR || any_test < 0 || any_test > 1 || !reps || !stats_ms ||
        (rip_ms && format != RG_FMT_S16_PLANAR) || (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_pcm_stats_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_width(format) / 8;
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    const rg_pcm_stats_opts o{RG_STATS_MIN_CLIP_RUN, RG_STATS_MIN_ZERO_RUN};
    unsigned char *d_arena = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgStatsPlane> planes(2 * n);
        std::vector<RgRipTrack> recs(rip_ms ? n : 0);
        char err[256] = "";
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)format;
            uint32_t reported;
            if (rg_stats_track_planes(i, t, rg_pcm_width(format), total, &planes[2 * i], &reported, err, sizeof err) != RG_OK ||
                (rip_ms && rg_rip_track_record(i, t, (i == 0 ? RG_RIP_FIRST_TRACK : 0u) | (i + 1 == n ? RG_RIP_LAST_TRACK : 0u), total, &recs[i], err,
                                               sizeof err) != RG_OK))
                return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_pcm_stats_rate: %s", err);
        }
        uint64_t fmt_tile[4];
        const uint64_t n_tiles = rg_stats_plan(planes.data(), planes.size(), fmt_tile);
        const uint64_t rip_tiles = rip_ms ? rg_rip_plan(recs.data(), n) : 0;
        if (planes.size() > 0x7fffffffu || n_tiles > 0x7fffffffu || rip_tiles > 0x7fffffffu)
            return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_pcm_stats_rate: too many tiles");
        const StatsLayout l = stats_layout(planes.size(), n_tiles);
        std::vector<unsigned char> head;
        stats_head(planes.data(), planes.size(), l, &head);
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipMalloc((void **)&d, l.end));  // (its own: the rip kernels' bookkeeping stays in the context's)
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_stats_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        if (rip_ms) {
            const int ur = rg_rip_kernels(c, d_arena, recs.data(), n, rip_tiles, true, s);
            if (ur != RG_OK) return ur;
        }
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<rg_pcm_stats_channel> host_ch(host_tracks ? 2 * host_tracks : 1), dev_ch(planes.size());
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < 2 * host_tracks; i = next.fetch_add(1)) host_ch[i] = rg_stats_serial_host(h.data(), planes[i], o);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            const int lr = stats_launch(c, d_arena, d, l, planes.size(), fmt_tile, o, any_test != 0, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        if (host_tracks) host_pass();
        for (uint32_t r = 0; r < reps; ++r) {
            float ms = 0.0f;
            RG_HIP(c, hipEventRecord(e0, s));
            int lr = stats_launch(c, d_arena, d, l, planes.size(), fmt_tile, o, any_test != 0, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            stats_ms[r] = ms;
            if (rip_ms) {
                RG_HIP(c, hipEventRecord(e0, s));
                lr = rg_rip_kernels(c, d_arena, recs.data(), n, rip_tiles, false, s);
                if (lr != RG_OK) return lr;
                RG_HIP(c, hipEventRecord(e1, s));
                RG_HIP(c, hipStreamSynchronize(s));
                RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
                rip_ms[r] = ms;
            }
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        RG_HIP(c, hipMemcpy(dev_ch.data(), d + l.res, planes.size() * sizeof(rg_pcm_stats_channel), hipMemcpyDeviceToHost));
        if (host_tracks) {
            *mismatches = 0;
            for (size_t i = 0; i < 2 * host_tracks; ++i) *mismatches += memcmp(&dev_ch[i], &host_ch[i], sizeof(rg_pcm_stats_channel)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_pcm_stats_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
