// rg_rip_offsets.hip -- the AccurateRip signatures of a disc at every drive offset of a window (include/mp3rgain_amd_rip.h,
// DRIVE OFFSETS; rg_rip.h): per track and offset o the sums of lo32(p) and hi32(p), p = W[B + i - 1 + o] * i, over the
// positions i that count.  v1 slides from one offset to the next; v2's hi32 is a floor of a product and does not, so every
// (frame, offset) pair is a 32 x 32 -> 64 multiply: the one integer-ALU-bound kernel of the project.
//
//   rg_rip_offsets_kernel  one block per (track, tile of RG_RIP_OFF_TILE frames), from a table the host lays out
//                          (rg_rip_offsets_plan: only tiles that hold a frame that counts).
//     staging   the disc words W of positions B + k0 - radius .. B + k0 + T + radius go into LDS as packed 32-bit words.  This
//               is the only place that maps a disc position to (track, frame): one bisection over the tracks' bases per lane,
//               then a walk forward, so a halo may span any number of short tracks; outside the disc it is zeros.  Samples
//               are read with 2-byte loads, so a track needs only sample alignment, and nothing but the tracks' own planes is
//               read.
//     products  lane l holds the J = RG_RIP_OFF_J = 23 consecutive offsets l J .. l J + J - 1 (as indices o + radius) in registers:
//               2 J accumulators and a window of J words, of which one is new per frame, so LDS is read once per J products
//               (lanes read words J apart: J is odd, no bank conflicts).  The frame loop is unrolled J times so that the
//               window's rotation is a renaming.  The position i is uniform across the block -- a scalar operand -- and
//               from..to are in the loop's bounds, not in a mask.  BLOCK * J = 5888 covers the largest window in one pass;
//               waves whose offsets all lie beyond the window skip the loop.
//     fold      each lane adds its sums into the zeroed tables with vector atomic adds: arv1 += lo, arv2 += lo + hi.  Adds
//               of integers commute: same input, same bits.
// No floating point, no scratch.  The launcher's callers check every record against the arena first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_rip.h"

// J: consecutive offsets a lane holds in registers.  The product runs J = RG_RIP_OFF_J, one pass over the window; J = 1 (a
// lane per offset, one LDS read per product, 23 passes) is there to be measured against it (rg_rip_offsets_rate).
template <uint32_t J>
__global__ __launch_bounds__(RG_RIP_OFF_BLOCK) void rg_rip_offsets_kernel(const unsigned char *__restrict__ arena, const RgRipDiscTrack *__restrict__ tr,
                                                                          uint32_t n_tracks, const RgRipOffTile *__restrict__ tiles, uint32_t radius,
                                                                          uint32_t *__restrict__ arv1, uint32_t *__restrict__ arv2) {
    constexpr uint32_t SPAN = RG_RIP_OFF_BLOCK * J;  // offsets of one pass
    static_assert((2u * RG_RIP_OFFSET_MAX + SPAN) / SPAN * SPAN <= RG_RIP_OFF_SPAN, "a lane's window would leave the staged words");
    __shared__ uint32_t s_w[RG_RIP_OFF_LDS];
    const uint32_t tid = threadIdx.x;
    const RgRipOffTile tile = tiles[blockIdx.x];
    const uint64_t base = tr[tile.track].base, total = tr[n_tracks].base;
    const int64_t to = tr[tile.track].to;
    const uint32_t from = tr[tile.track].from;
    const uint32_t n_off = 2 * radius + 1, staged = RG_RIP_OFF_TILE + 2 * radius;  // s_w[x] = W[base + k0 - radius + x]

    {
        const int64_t pos0 = (int64_t)(base + tile.k0) - (int64_t)radius;
        uint32_t u = 0;
        bool found = false;
        for (uint32_t x = tid; x < RG_RIP_OFF_LDS; x += RG_RIP_OFF_BLOCK) {
            const int64_t pos = pos0 + x;
            uint32_t w = 0;
            if (x < staged && pos >= 0 && (uint64_t)pos < total) {
                if (!found) u = rg_rip_disc_find(tr, n_tracks, (uint64_t)pos);
                found = true;
                while ((uint64_t)pos >= tr[u + 1].base) ++u;  // (tr[n_tracks].base = total > pos)
                const uint64_t f = (uint64_t)pos - tr[u].base, frames = tr[u].frames;
                const unsigned char *p = arena + tr[u].off;
                const uint32_t l = *reinterpret_cast<const uint16_t *>(p + 2 * f), r = *reinterpret_cast<const uint16_t *>(p + 2 * (frames + f));
                w = l | (r << 16);
            }
            s_w[x] = w;
        }
    }
    __syncthreads();

    // frames [ka, ke) of the tile count: position i = k0 + k + 1 in from..to
    const int64_t lo_k = (from > 1u ? (int64_t)from - 1 : 0) - (int64_t)tile.k0, hi_k = to - (int64_t)tile.k0;
    const uint32_t ka = (uint32_t)(lo_k > 0 ? lo_k : 0), ke = (uint32_t)(hi_k < (int64_t)RG_RIP_OFF_TILE ? (hi_k > 0 ? hi_k : 0) : RG_RIP_OFF_TILE);
    if (ka >= ke) return;
    const size_t row = (size_t)tile.track * n_off;
    for (uint32_t first = tid * J; first < n_off; first += SPAN) {  // `first`: of this lane's J offsets, as o + radius
        uint32_t lo[J], hi[J], win[J];
#pragma unroll
        for (uint32_t j = 0; j < J; ++j) lo[j] = hi[j] = 0;
        // frame k, offset first + j reads s_w[k + first + j]: the word is win[(g + j) % J] at step g = k - ka
#pragma unroll
        for (uint32_t j = 0; j + 1 < J; ++j) win[j] = s_w[ka + first + j];
        win[J - 1] = 0;
        for (uint32_t kb = ka; kb < ke; kb += J) {
#pragma unroll
            for (uint32_t s = 0; s < J; ++s) {
                const uint32_t k = kb + s;
                if (k < ke) {  // uniform
                    win[(s + J - 1) % J] = s_w[k + first + J - 1];  // <= T - 1 + RG_RIP_OFF_SPAN - 1: the assert above
                    const uint32_t i = tile.k0 + k + 1;
#pragma unroll
                    for (uint32_t j = 0; j < J; ++j) rg_rip_off_product(win[(s + j) % J], i, &lo[j], &hi[j]);
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < J; ++j) {
            if (first + j < n_off) {
                if (arv1) atomicAdd(&arv1[row + first + j], lo[j]);
                if (arv2) atomicAdd(&arv2[row + first + j], lo[j] + hi[j]);
            }
        }
    }
}

// Device layout of one launch's bookkeeping (c->d_rip), every part 16-byte aligned: [disc records | tiles | arv1 | arv2]
struct OffLayout {
    size_t tiles, v1, v2, end, table_bytes;
};
static OffLayout off_layout(size_t n, size_t n_tiles, int32_t radius) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    OffLayout l;
    l.table_bytes = n * (2 * (size_t)radius + 1) * sizeof(uint32_t);
    l.tiles = a16((n + 1) * sizeof(RgRipDiscTrack));
    l.v1 = a16(l.tiles + n_tiles * sizeof(RgRipOffTile));
    l.v2 = a16(l.v1 + l.table_bytes);
    l.end = a16(l.v2 + l.table_bytes);
    return l;
}

// the tables zeroed and the kernel over `n_tiles` tiles (> 0), on `s`
static int off_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const OffLayout &l, size_t n, size_t n_tiles, int32_t radius, bool want1,
                      bool want2, hipStream_t s, uint32_t lane_offsets = RG_RIP_OFF_J) {
    RG_HIP(c, hipMemsetAsync(d + l.v1, 0, l.end - l.v1, s));
    if (!n_tiles) return RG_OK;
    const auto kernel = lane_offsets == 1 ? rg_rip_offsets_kernel<1> : rg_rip_offsets_kernel<RG_RIP_OFF_J>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)n_tiles), dim3(RG_RIP_OFF_BLOCK), 0, s, d_arena, reinterpret_cast<const RgRipDiscTrack *>(d), (uint32_t)n,
                       reinterpret_cast<const RgRipOffTile *>(d + l.tiles), (uint32_t)radius, want1 ? reinterpret_cast<uint32_t *>(d + l.v1) : nullptr,
                       want2 ? reinterpret_cast<uint32_t *>(d + l.v2) : nullptr);
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_rip_offsets_device(rg_ctx *c, const unsigned char *d_arena, const RgRipDiscTrack *tr, size_t n, int32_t radius, uint32_t *arv1, uint32_t *arv2,
                          hipStream_t s) {
    if (!n || (!arv1 && !arv2)) return RG_OK;
    if (radius < 0 || radius > RG_RIP_OFFSET_MAX || n > RG_RIP_DISC_MAX_TRACKS)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rip offsets: radius %d, %zu tracks", (int)radius, n);
    std::vector<RgRipOffTile> tiles;
    rg_rip_offsets_plan(tr, n, &tiles);
    if (tiles.size() > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu tiles", tiles.size());
    const OffLayout l = off_layout(n, tiles.size(), radius);
    RG_HIP(c, c->d_rip.reserve(l.end));
    unsigned char *d = c->d_rip.p;
    RG_HIP(c, hipMemcpyAsync(d, tr, (n + 1) * sizeof(RgRipDiscTrack), hipMemcpyHostToDevice, s));
    if (!tiles.empty()) RG_HIP(c, hipMemcpyAsync(d + l.tiles, tiles.data(), tiles.size() * sizeof(RgRipOffTile), hipMemcpyHostToDevice, s));
    const int rc = off_launch(c, d_arena, d, l, n, tiles.size(), radius, arv1 != nullptr, arv2 != nullptr, s);
    if (rc != RG_OK) return rc;
    if (arv1) RG_HIP(c, hipMemcpyAsync(arv1, d + l.v1, l.table_bytes, hipMemcpyDeviceToHost, s));
    if (arv2) RG_HIP(c, hipMemcpyAsync(arv2, d + l.v2, l.table_bytes, hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));  // (`tiles` and the caller's records live until here)
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_rip.h) ---------------------------------------------------------------------------------
extern "C" int rg_rip_offsets_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, int32_t radius,
                                    const void *arena, size_t arena_bytes, uint32_t *arv1, uint32_t *arv2) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    char err[256] = "";
    if (!c && route == 1) return RG_ERR_INVALID_ARG;  // the host routes need no context (their error text: rg_last_error(NULL))
    try {
        std::vector<RgRipDiscTrack> recs;
        int rc = rg_rip_offsets_check(route, n, descs, track_flags, radius, arena, arena_bytes, arv2, &recs, err, sizeof err);
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
        if (!n) return RG_OK;
        if (route != 1) return rg_rip_offsets_host(route, recs, radius, arena, arv1, arv2);
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        RG_HIP(c, c->d_arena.reserve(((arena_bytes + 15) & ~(size_t)15) + 16));
        hipStream_t s = c->slots[0].stream;
        if (arena_bytes) RG_HIP(c, hipMemcpyAsync(c->d_arena.p, arena, arena_bytes, hipMemcpyHostToDevice, s));
        return rg_rip_offsets_device(c, c->d_arena.p, recs.data(), n, radius, arv1, arv2, s);
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

// ---- measurement hook (tools/rip_offsets_rate.py) ----------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per 32-bit word: word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_rip_offsets_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}

extern "C" int rg_rip_offsets_rate(void *ctx, size_t n, uint64_t frames, int32_t radius, uint32_t lane_offsets, uint32_t host_offsets, uint32_t threads,
                                   uint32_t reps, double warm_ms, double *dev_ms, double *host_ms, uint64_t *host_products, uint64_t *disc_products, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    const uint32_t n_off = 2 * (uint32_t)(radius < 0 ? 0 : radius) + 1;
    if ((lane_offsets != 1 && lane_offsets != RG_RIP_OFF_J) || !n || n > RG_RIP_DISC_MAX_TRACKS || !frames || frames >= ((uint64_t)1 << 32) || radius < 0 || radius > RG_RIP_OFFSET_MAX || !reps || !dev_ms ||
        host_offsets > n_off || (host_offsets && (!host_ms || !host_products || !threads || !mismatches)) || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_offsets_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 4, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgRipTrack> tracks(n);
        for (size_t i = 0; i < n; ++i) {
            memset(&tracks[i], 0, sizeof tracks[i]);
            tracks[i].off = i * stride;
            tracks[i].frames = frames;
            tracks[i].from = i == 0 ? RG_RIP_AR_SKIP : 0u;
            tracks[i].to = i + 1 == n ? (int64_t)frames - (int64_t)RG_RIP_AR_SKIP : (int64_t)frames;
        }
        std::vector<RgRipDiscTrack> recs(n + 1);
        rg_rip_disc(tracks.data(), n, recs.data());
        uint64_t counted = 0;
        for (size_t i = 0; i < n; ++i) {
            const int64_t f = recs[i].from > 1u ? recs[i].from : 1;
            if (recs[i].to >= f) counted += (uint64_t)(recs[i].to - f + 1);
        }
        if (disc_products) *disc_products = counted * n_off;
        std::vector<RgRipOffTile> tiles;
        rg_rip_offsets_plan(recs.data(), n, &tiles);
        if (tiles.size() > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_rip_offsets_rate: too many tiles");
        const OffLayout l = off_layout(n, tiles.size(), radius);
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, c->d_rip.reserve(l.end));
        unsigned char *d = c->d_rip.p;
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_rip_offsets_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        RG_HIP(c, hipMemcpyAsync(d, recs.data(), (n + 1) * sizeof(RgRipDiscTrack), hipMemcpyHostToDevice, s));
        if (!tiles.empty()) RG_HIP(c, hipMemcpyAsync(d + l.tiles, tiles.data(), tiles.size() * sizeof(RgRipOffTile), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            const int lr = off_launch(c, d_arena, d, l, n, tiles.size(), radius, true, true, s, lane_offsets);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipStreamSynchronize(s));
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            RG_HIP(c, hipEventRecord(e0, s));
            const int lr = off_launch(c, d_arena, d, l, n, tiles.size(), radius, true, true, s, lane_offsets);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            float ms = 0.0f;
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            dev_ms[r] = ms;
        }
        if (!host_offsets) return RG_OK;
        std::vector<uint32_t> v1(n * (size_t)n_off), v2(n * (size_t)n_off), W;
        RG_HIP(c, hipMemcpy(v1.data(), d + l.v1, l.table_bytes, hipMemcpyDeviceToHost));
        RG_HIP(c, hipMemcpy(v2.data(), d + l.v2, l.table_bytes, hipMemcpyDeviceToHost));
        {
            std::vector<unsigned char> h(total);
            RG_HIP(c, hipMemcpy(h.data(), d_arena, total, hipMemcpyDeviceToHost));
            rg_rip_disc_words(h.data(), recs.data(), n, &W);
        }
        // the host's share: offsets spread evenly over the window, both of its ends among them
        std::vector<int32_t> offs(host_offsets);
        for (uint32_t q = 0; q < host_offsets; ++q)
            offs[q] = host_offsets == 1 ? 0 : (int32_t)((uint64_t)q * (n_off - 1) / (host_offsets - 1)) - radius;
        std::atomic<size_t> next{0}, bad{0};
        const size_t cells = n * (size_t)host_offsets;
        auto work = [&]() {
            for (size_t q = next.fetch_add(1); q < cells; q = next.fetch_add(1)) {
                const size_t t = q / host_offsets;
                const int32_t o = offs[q % host_offsets];
                uint32_t a, b;
                rg_rip_offsets_cell(W, recs[t], o, &a, &b);
                const size_t at = t * n_off + (size_t)(o + radius);
                if (a != v1[at] || b != v2[at]) bad.fetch_add(1);
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *host_products = counted * host_offsets;
        *mismatches = bad.load();
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_rip_offsets_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
