// rg_rip_crc.hip -- the rip checksums on the device (include/mp3rgain_amd_rip.h, rg_rip.h, rg_crc32.h): per track the CRC-32
// of the PCM, the CRC-32 of its non-null samples, the null-sample count and the AccurateRip v1 / v2 sums, from the 16-bit
// planes of the analysis arena.
//
// A CRC's raw register (initial value 0, no final XOR) is linear, and the AccurateRip sums are sums, so a track is parallel
// inside: it is cut into chunks of RG_RIP_CHUNK frames, every chunk hashed by its own lane and the lanes' parts folded in
// order.  Chunks and tiles are counted from the track's END: only the first of each is short, a missing one in front is a
// zero, and every step of one tree level multiplies the plain CRC by one constant.  The non-null CRC's message has the
// data's own lengths, so its parts fold as (crc, len) pairs with the power taken from a table of x^(8 2^j).
//
//   rg_rip_tiles_kernel  one block per tile of RG_RIP_BLOCK chunks, many tracks per launch; the block finds its track by
//                        bisection over the tracks' first tiles.  It stages its stretch of both planes into LDS with
//                        aligned 16-byte loads -- the aligned cover may reach up to 14 bytes outside the track on either
//                        side, never outside the arena's allocation of whole 16-byte words, and what it holds beyond the
//                        track is never read back -- skewed by one dword per 16 so that lanes 64 bytes apart read
//                        different banks.  Each lane hashes its chunk from LDS with the tables in LDS (rg_rip_chunk), and
//                        a fixed tree over LDS folds the 256 parts (rg_rip_combine).  One 32-byte record per tile.
//   rg_rip_fold_kernel   one block (a wave) per track: each lane folds a run of `run` tile records in order, then the same
//                        tree with the track's powers, then the initial-value fix-up of both CRCs (rg_rip_finish).
// No atomics and no floating point anywhere: same input, same bits.  The launcher checks every record against the arena first.
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

// LDS image of one plane's stretch: dword d of the aligned cover at d + (d >> 4)
#define RG_RIP_WIN_DWORDS ((2u * RG_RIP_TILE + 32u) / 4u)
#define RG_RIP_LDS_DWORDS (RG_RIP_WIN_DWORDS + RG_RIP_WIN_DWORDS / 16u + 4u)
__device__ __forceinline__ uint32_t rg_rip_skew(uint32_t d) { return d + (d >> 4); }

// the fixed tree: v[0] <- the fold of v[0 .. 2^levels) in order, level j multiplying the plain CRC by pw[j].  The lanes
// that work are the first ones, so whole waves drop out as the levels go up.
__device__ __forceinline__ void rg_rip_tree(RgRipPart *v, uint32_t levels, const uint32_t *pw, const uint32_t *x2, uint32_t tid) {
    for (uint32_t j = 0; j < levels; ++j) {
        const uint32_t s = 1u << j;
        __syncthreads();
        if (tid < ((1u << levels) >> (j + 1))) {
            const uint32_t at = tid * 2 * s;
            RgRipPart a = v[at];
            rg_rip_combine(&a, v[at + s], pw[j], x2);
            v[at] = a;
        }
    }
    __syncthreads();
}

template <bool SLICE4>
__global__ __launch_bounds__(RG_RIP_BLOCK) void rg_rip_tiles_kernel(const unsigned char *__restrict__ arena, const RgRipTrack *__restrict__ recs,
                                                                    uint32_t n_tracks, RgRipPowers P, RgRipPart *__restrict__ tile_out) {
    __shared__ uint32_t s_data[2][RG_RIP_LDS_DWORDS];
    __shared__ uint32_t s_tab[SLICE4 ? 1024 : 256];
    __shared__ uint32_t s_x2[RG_CRC32_X2_ENTRIES];
    __shared__ RgRipPart s_part[RG_RIP_BLOCK];
    __shared__ uint32_t s_track;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    for (uint32_t k = 0; k < (SLICE4 ? 4u : 1u); ++k) s_tab[256 * k + tid] = rg_crc32_slice_entry(k, tid);
    if (tid < RG_CRC32_X2_ENTRIES) s_x2[tid] = P.x2[tid];
    if (tid == 0) {  // the last track whose first tile is not behind this one (tracks without tiles share their successor's)
        uint32_t lo = 0, hi = n_tracks - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (recs[mid].first_tile <= tile) lo = mid;
            else hi = mid - 1;
        }
        while (recs[lo].n_tiles == 0 && lo > 0) --lo;  // (only behind the last tile's track; never taken for a valid launch)
        s_track = lo;
    }
    __syncthreads();
    const RgRipTrack r = recs[s_track];
    uint64_t wstart;
    const uint32_t wlen = rg_rip_tile_window(r.frames, r.n_tiles, tile - r.first_tile, &wstart);
    // the aligned cover of [wstart, wstart + wlen) of plane p into s_data[p]; returns where the stretch begins in it, in samples
    auto stage = [&](uint32_t p) -> uint32_t {
        const uint64_t g0 = r.off + 2 * (p * r.frames + wstart), ab = g0 & ~(uint64_t)15;
        const uint32_t nvec = ((uint32_t)(g0 - ab) + 2 * wlen + 15) / 16;
        const uint4 *src = reinterpret_cast<const uint4 *>(arena + ab);
        for (uint32_t v = tid; v < nvec; v += RG_RIP_BLOCK) {
            const uint4 q = src[v];
            const uint32_t at = rg_rip_skew(4 * v);  // (4v .. 4v + 3 share one skew)
            s_data[p][at] = q.x;
            s_data[p][at + 1] = q.y;
            s_data[p][at + 2] = q.z;
            s_data[p][at + 3] = q.w;
        }
        return (uint32_t)(g0 - ab) >> 1;
    };
    const uint32_t mis0 = stage(0), mis1 = stage(1);
    __syncthreads();
    uint32_t a;
    const uint32_t n = rg_rip_lane_chunk(wlen, tid, &a);
    const uint32_t m0 = mis0 + a, m1 = mis1 + a;
    RgRipPart part;
    rg_rip_chunk<SLICE4>(
        [&](uint32_t p, uint32_t j) -> uint32_t {
            const uint32_t s = (p ? m1 : m0) + j;  // sample s of the cover: half (s & 1) of dword s >> 1
            return (s_data[p][rg_rip_skew(s >> 1)] >> (16 * (s & 1u))) & 0xFFFFu;
        },
        wstart + a, n, r.from, r.to, s_tab, &part);
    s_part[tid] = part;
    rg_rip_tree(s_part, RG_RIP_LEVELS, P.pw, s_x2, tid);
    if (tid == 0) tile_out[tile] = s_part[0];
}

__global__ __launch_bounds__(RG_RIP_FOLD_LANES) void rg_rip_fold_kernel(const RgRipTrack *__restrict__ recs, const RgRipPart *__restrict__ tile_in,
                                                                        RgRipPowers P, RgRipSums *__restrict__ out) {
    __shared__ RgRipPart s_part[RG_RIP_FOLD_LANES];
    __shared__ uint32_t s_x2[RG_CRC32_X2_ENTRIES];
    __shared__ uint32_t s_pw[RG_RIP_FOLD_LEVELS];
    const uint32_t tid = threadIdx.x;
    const RgRipTrack &r = recs[blockIdx.x];  // (read field by field: a copy indexed by lane would live in scratch)
    if (tid < RG_CRC32_X2_ENTRIES) s_x2[tid] = P.x2[tid];
    if (tid < RG_RIP_FOLD_LEVELS) s_pw[tid] = r.pw[tid];
    __syncthreads();
    int64_t lo;
    const int64_t hi = rg_rip_lane_run(r.n_tiles, r.run, tid, &lo);
    RgRipPart acc = rg_rip_empty();
    for (int64_t t = lo; t < hi; ++t) rg_rip_combine(&acc, tile_in[r.first_tile + (uint64_t)t], P.x_tile, s_x2);
    s_part[tid] = acc;
    rg_rip_tree(s_part, RG_RIP_FOLD_LEVELS, s_pw, s_x2, tid);
    if (tid == 0) out[blockIdx.x] = rg_rip_finish(s_part[0], r.frames, s_x2);
}

// Device layout of one launch's bookkeeping (c->d_rip), every part 16-byte aligned: [track records | tile records | sums]
struct RipLayout {
    size_t tiles, sums, end;
};
static RipLayout rip_layout(size_t n, uint64_t n_tiles) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    RipLayout l;
    l.tiles = a16(n * sizeof(RgRipTrack));
    l.sums = a16(l.tiles + (size_t)n_tiles * sizeof(RgRipPart));
    l.end = a16(l.sums + n * sizeof(RgRipSums));
    return l;
}

static int rip_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const RipLayout &l, size_t n, uint64_t n_tiles, int table_layout,
                      hipStream_t s) {
    const RgRipPowers P = rg_rip_powers();
    const RgRipTrack *d_recs = reinterpret_cast<const RgRipTrack *>(d);
    RgRipPart *d_tiles = reinterpret_cast<RgRipPart *>(d + l.tiles);
    if (n_tiles) {
        if (table_layout)
            hipLaunchKernelGGL(rg_rip_tiles_kernel<true>, dim3((uint32_t)n_tiles), dim3(RG_RIP_BLOCK), 0, s, d_arena, d_recs, (uint32_t)n, P, d_tiles);
        else
            hipLaunchKernelGGL(rg_rip_tiles_kernel<false>, dim3((uint32_t)n_tiles), dim3(RG_RIP_BLOCK), 0, s, d_arena, d_recs, (uint32_t)n, P, d_tiles);
        RG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(rg_rip_fold_kernel, dim3((uint32_t)n), dim3(RG_RIP_FOLD_LANES), 0, s, d_recs, d_tiles, P, reinterpret_cast<RgRipSums *>(d + l.sums));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

// the plain CRC's table layout of the product: see DESIGN 12.2 for the readings
#define RG_RIP_TABLE_LAYOUT 1

int rg_rip_device(rg_ctx *c, const unsigned char *d_arena, RgRipTrack *recs, size_t n, RgRipSums *sums, hipStream_t s) {
    if (!n) return RG_OK;
    const uint64_t n_tiles = rg_rip_plan(recs, n);
    if (n > 0x7fffffffu || n_tiles > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu tracks, %llu tiles", n, (unsigned long long)n_tiles);
    const RipLayout l = rip_layout(n, n_tiles);
    RG_HIP(c, c->d_rip.reserve(l.end));
    unsigned char *d = c->d_rip.p;
    RG_HIP(c, hipMemcpyAsync(d, recs, n * sizeof(RgRipTrack), hipMemcpyHostToDevice, s));
    const int rc = rip_launch(c, d_arena, d, l, n, n_tiles, RG_RIP_TABLE_LAYOUT, s);
    if (rc != RG_OK) return rc;
    RG_HIP(c, hipMemcpyAsync(sums, d + l.sums, n * sizeof(RgRipSums), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

int rg_rip_kernels(rg_ctx *c, const unsigned char *d_arena, const RgRipTrack *recs, size_t n, uint64_t n_tiles, bool upload, hipStream_t s) {
    const RipLayout l = rip_layout(n, n_tiles);
    if (upload) {
        RG_HIP(c, c->d_rip.reserve(l.end));
        RG_HIP(c, hipMemcpyAsync(c->d_rip.p, recs, n * sizeof(RgRipTrack), hipMemcpyHostToDevice, s));
        return RG_OK;
    }
    return rip_launch(c, d_arena, c->d_rip.p, l, n, n_tiles, RG_RIP_TABLE_LAYOUT, s);
}

// ---- test seam (include/mp3rgain_amd_rip.h) ---------------------------------------------------------------------------------
extern "C" int rg_rip_checksums_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, const void *arena,
                                      size_t arena_bytes, rg_rip_result *out) {
    std::vector<RgRipTrack> recs;
    const auto host = [&](char *err, size_t err_len) { return rg_rip_arena_host(route, n, descs, track_flags, arena, arena_bytes, out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        recs = std::vector<RgRipTrack>(n ? n : 1);
        for (size_t i = 0; i < n; ++i) {
            const int rc = rg_rip_track_record(i, descs[i], track_flags ? track_flags[i] : 0u, arena_bytes, &recs[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        std::vector<RgRipSums> sums(n ? n : 1);
        const int rc = rg_rip_device(c, c->d_arena.p, recs.data(), n, sums.data(), s);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) rg_rip_fill(sums[i], descs[i].frames, descs[i].sample_rate, 0, &out[i]);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_rip_checksums_arena", "folded", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/rip_crc_rate.py) -------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per 32-bit word: word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_rip_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}

extern "C" int rg_rip_rate(void *ctx, size_t n, uint64_t frames, int table_layout, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                           double *dev_ms, double *host_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || table_layout < 0 || table_layout > 1 || !reps || !dev_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 4, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgRipTrack> recs(n);
        for (size_t i = 0; i < n; ++i) {
            memset(&recs[i], 0, sizeof recs[i]);
            recs[i].off = i * stride;
            recs[i].frames = frames;
            recs[i].from = i == 0 ? RG_RIP_AR_SKIP : 0u;  // a disc: the first and the last track flagged
            recs[i].to = i + 1 == n ? (int64_t)frames - (int64_t)RG_RIP_AR_SKIP : (int64_t)frames;
        }
        const uint64_t n_tiles = rg_rip_plan(recs.data(), n);
        if (n > 0x7fffffffu || n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_rate: too many tiles");
        const RipLayout l = rip_layout(n, n_tiles);
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, c->d_rip.reserve(l.end));
        unsigned char *d = c->d_rip.p;
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_rip_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, recs.data(), n * sizeof(RgRipTrack), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<RgRipSums> host_sums(host_tracks ? host_tracks : 1), dev_sums(n);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < host_tracks; i = next.fetch_add(1)) host_sums[i] = rg_rip_serial_host(h.data(), recs[i]);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            const int lr = rip_launch(c, d_arena, d, l, n, n_tiles, table_layout, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        if (host_tracks) host_pass();
        for (uint32_t r = 0; r < reps; ++r) {
            RG_HIP(c, hipEventRecord(e0, s));
            const int lr = rip_launch(c, d_arena, d, l, n, n_tiles, table_layout, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            float ms = 0.0f;
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            dev_ms[r] = ms;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        RG_HIP(c, hipMemcpy(dev_sums.data(), d + l.sums, n * sizeof(RgRipSums), hipMemcpyDeviceToHost));
        if (host_tracks) {
            *mismatches = 0;
            for (size_t i = 0; i < host_tracks; ++i) *mismatches += memcmp(&dev_sums[i], &host_sums[i], sizeof(RgRipSums)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_rip_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
