// rg_dr.hip -- the dynamic range scan on the device (include/mp3rgain_amd_dr.h, rg_dr.h): per plane the exact energy and the peak
// of every block, the k-th largest block by mean square, the mean of the blocks above it and the second-highest block peak, from
// the planes of the analysis arena in any of its three formats.
//
//   rg_dr_pieces_kernel  one workgroup per piece of RG_DR_PIECE_BYTES of one block of one plane, many planes per launch, one
//                        launch per format; the workgroup finds its plane in a piece -> plane table and its block and piece from
//                        its place among the plane's pieces.  The lanes take interleaved, coalesced 16-byte vectors of the
//                        piece's aligned cover straight into registers, all of a lane's loads issued before the first is used;
//                        there is no LDS staging, because a sum of squares and a maximum do not care which lane saw a sample.
//                        Planes and blocks are only sample-aligned, so the first and the last vector of the cover are taken
//                        sample by sample under a mask, by two lanes; the cover reaches at most 15 bytes outside the plane on
//                        either side, never outside the arena's allocation of whole 16-byte words.  Lane shuffles and four LDS
//                        records reduce the workgroup; one 24-byte record per piece.
//   rg_dr_fold_kernel    one workgroup per plane.  Lane l folds the pieces of blocks l, l + 256, ... in ascending order into the
//                        block's sums and leaves (ms, e, peak) per block in device memory; a radix select on the bit patterns of
//                        the ms (8 bits a pass, integer counters in LDS) finds the k-th largest whatever the number of blocks;
//                        lane 0 walks the block records in ascending index (rg_dr_plane).  One 40-byte record per plane.
// The sums are integers and the only atomics are integer counters in LDS; the doubles are added by one lane in a fixed order:
// same input, same bits.  The launcher's callers check every plane against the arena first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_dr.h"
#include "rg_pcm_seam.h"
#include "rg_stats.h"

// sample j of a vector as the stored pattern, S16 sign-extended
template <int FMT>
__device__ __forceinline__ uint32_t dr_sample(const uint4 &w, uint32_t j) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    if (FMT == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t)(int16_t)(d[j >> 1] >> (16u * (j & 1u)));
    return d[j];
}
// a whole vector into the sums
template <int FMT>
__device__ __forceinline__ void dr_take_vec(const uint4 &w, RgDrPiece *acc) {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    if (FMT == RG_FMT_S16_PLANAR) {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {  // two squares are at most 2^31: one 64-bit addition per pair
            const int32_t v0 = (int32_t)(int16_t)d[i], v1 = (int32_t)d[i] >> 16;
            const uint32_t a0 = (uint32_t)(v0 < 0 ? -v0 : v0), a1 = (uint32_t)(v1 < 0 ? -v1 : v1);
            acc->lo += a0 * a0 + a1 * a1;
            const uint32_t m = a0 > a1 ? a0 : a1;
            acc->peak = m > acc->peak ? m : acc->peak;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) rg_dr_take<FMT>(d[i], acc);
    }
}

// the workgroup's sums in lane 0: shuffles inside a wave, then the four waves' records in order
template <int FMT>
__device__ __forceinline__ RgDrPiece dr_reduce(RgDrPiece acc, RgDrPiece *s_wave, uint32_t tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        RgDrPiece o;
        o.lo = __shfl_xor((unsigned long long)acc.lo, d, 64);
        o.hi = FMT == RG_FMT_S16_PLANAR ? 0ull : __shfl_xor((unsigned long long)acc.hi, d, 64);
        o.peak = __shfl_xor(acc.peak, d, 64);
        o.nonfinite = FMT == RG_FMT_F32_PLANAR ? __shfl_xor(acc.nonfinite, d, 64) : 0u;
        rg_dr_combine(&acc, o);
    }
    if ((tid & 63u) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        for (uint32_t w = 1; w < RG_DR_LANES / 64u; ++w) rg_dr_combine(&acc, s_wave[w]);
    return acc;
}

// where a workgroup's piece lies
struct DrCover {
    const uint4 *src;  // the aligned cover
    uint32_t nvec;     // its vectors
    uint32_t mis;      // where the piece begins in it, in samples
    uint32_t plen;     // samples of the piece
};
template <int FMT>
__device__ __forceinline__ DrCover dr_cover(const unsigned char *arena, const RgDrPlane &p, uint64_t piece) {
    constexpr uint32_t bps = FMT == RG_FMT_S16_PLANAR ? 2u : 4u;
    const uint32_t rel = (uint32_t)(piece - p.first_piece);
    const uint32_t b = rel / p.pieces_per_block, k = rel - b * p.pieces_per_block;
    uint64_t bstart;
    const uint32_t len = rg_dr_block_window(p, b, &bstart);
    uint32_t pstart;
    DrCover c;
    c.plen = rg_dr_piece_window(len, k, FMT, &pstart);
    const uint64_t g0 = p.off + (uint64_t)bps * (bstart + pstart), ab = g0 & ~(uint64_t)15;
    c.mis = (uint32_t)(g0 - ab) / bps;
    c.nvec = ((uint32_t)(g0 - ab) + bps * c.plen + 15u) / 16u;
    c.src = reinterpret_cast<const uint4 *>(arena + ab);
    return c;
}

template <int FMT>
__global__ __launch_bounds__(RG_DR_LANES) void rg_dr_pieces_kernel(const unsigned char *__restrict__ arena, const RgDrPlane *__restrict__ planes,
                                                                  const uint32_t *__restrict__ piece_plane, uint64_t piece_base,
                                                                  RgDrPiece *__restrict__ piece_out) {
    constexpr uint32_t C = FMT == RG_FMT_S16_PLANAR ? 8u : 4u;  // samples of a vector
    __shared__ RgDrPiece s_wave[RG_DR_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t piece = piece_base + blockIdx.x;
    const DrCover c = dr_cover<FMT>(arena, planes[piece_plane[piece]], piece);
    RgDrPiece acc = rg_dr_empty();
    // the two vectors that may hold samples of a neighbour: lane 0 the first, lane 1 the last, sample by sample
    if (tid < 2 && (tid == 0 || c.nvec > 1)) {
        const uint32_t v = tid ? c.nvec - 1 : 0u;
        const uint4 w = c.src[v];
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            const uint32_t at = v * C + j;
            if (at >= c.mis && at < c.mis + c.plen) rg_dr_take<FMT>(dr_sample<FMT>(w, j), &acc);
        }
    }
    // the vectors in between are whole: RG_DR_STEPS loads in flight per lane (a vector of zeros adds nothing)
    const uint32_t end = c.nvec - 1;
    for (uint32_t v = 1 + tid; v < end; v += RG_DR_STEPS * RG_DR_LANES) {
        uint4 w[RG_DR_STEPS];
#pragma unroll
        for (uint32_t u = 0; u < RG_DR_STEPS; ++u) {
            const uint32_t at = v + u * RG_DR_LANES;
            w[u] = at < end ? c.src[at] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (uint32_t u = 0; u < RG_DR_STEPS; ++u) dr_take_vec<FMT>(w[u], &acc);
    }
    acc = dr_reduce<FMT>(acc, s_wave, tid);
    if (tid == 0) piece_out[piece] = acc;
}

// blocks: written and read back by the same workgroup (no __restrict__, and a workgroup barrier in between)
__global__ __launch_bounds__(RG_DR_FOLD_LANES) void rg_dr_fold_kernel(const RgDrPlane *__restrict__ planes, const RgDrPiece *__restrict__ piece_in,
                                                                      RgDrBlock *blocks, RgDrPlaneOut *__restrict__ out) {
    __shared__ uint32_t s_hist[RG_DR_BINS];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_above, s_nonfinite;
    const uint32_t tid = threadIdx.x;
    const RgDrPlane p = planes[blockIdx.x];
    RgDrBlock *const mine = blocks + p.first_block;
    if (tid == 0) s_nonfinite = 0;
    __syncthreads();
    // the pieces of a block in ascending order, the block's record
    uint32_t nonfinite = 0;
    for (uint32_t b = tid; b < p.n_blocks; b += RG_DR_FOLD_LANES) {
        uint64_t bstart;
        const uint32_t len = rg_dr_block_window(p, b, &bstart);
        const RgDrPiece *in = piece_in + p.first_piece + (uint64_t)b * p.pieces_per_block;
        const uint32_t cnt = rg_dr_pieces_of(len, p.format);
        RgDrPiece acc = rg_dr_empty();
        for (uint32_t k = 0; k < cnt; ++k) rg_dr_combine(&acc, in[k]);
        mine[b] = rg_dr_block(acc, len, p.format);
        nonfinite += acc.nonfinite;
    }
    if (nonfinite) atomicAdd(&s_nonfinite, nonfinite);
    // the k-th largest ms: its pattern, a digit a pass
    uint64_t prefix = 0;
    uint32_t above = 0;
    if (p.n_blocks)  // uniform over the workgroup
        for (uint32_t pass = 0; pass < RG_DR_PASSES; ++pass) {
            for (uint32_t i = tid; i < RG_DR_BINS; i += RG_DR_FOLD_LANES) s_hist[i] = 0;
            __syncthreads();  // (in the first pass: the block records are written as well)
            for (uint32_t b = tid; b < p.n_blocks; b += RG_DR_FOLD_LANES) {
                const uint64_t key = rg_dr_key(mine[b].ms);
                if (rg_dr_in_prefix(key, prefix, pass)) atomicAdd(&s_hist[rg_dr_digit(key, pass)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t more;
                const uint32_t d = rg_dr_pick(s_hist, p.k - above, &more);
                s_above = above + more;
                s_prefix = (prefix << RG_DR_RADIX_BITS) | d;
            }
            __syncthreads();
            above = s_above;
            prefix = s_prefix;
        }
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = rg_dr_plane([&](uint32_t b) { return mine[b]; }, p, rg_dr_unkey(prefix), above, s_nonfinite);
}

// Device layout of one launch's bookkeeping, every part 16-byte aligned:
// [plane records | piece -> plane | piece records | block records | results]
struct DrLayout {
    size_t map, pieces, blocks, res, end;
};
static DrLayout dr_layout(size_t n, uint64_t n_pieces, uint64_t n_blocks) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    DrLayout l;
    l.map = a16(n * sizeof(RgDrPlane));
    l.pieces = a16(l.map + (size_t)n_pieces * sizeof(uint32_t));
    l.blocks = a16(l.pieces + (size_t)n_pieces * sizeof(RgDrPiece));
    l.res = a16(l.blocks + (size_t)n_blocks * sizeof(RgDrBlock));
    l.end = a16(l.res + n * sizeof(RgDrPlaneOut));
    return l;
}
// the head of the bookkeeping as the host builds it: the planned records and the table
static void dr_head(const RgDrPlane *planes, size_t n, const DrLayout &l, std::vector<unsigned char> *head) {
    head->assign(l.pieces, 0);
    if (n) memcpy(head->data(), planes, n * sizeof(RgDrPlane));
    uint32_t *map = reinterpret_cast<uint32_t *>(head->data() + l.map);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t cnt = rg_dr_plane_pieces(planes[i]);
        for (uint64_t t = 0; t < cnt; ++t) map[planes[i].first_piece + t] = (uint32_t)i;
    }
}

template <int FMT>
static void dr_launch_format(const unsigned char *d_arena, const RgDrPlane *d_planes, const uint32_t *d_map, uint64_t base, uint64_t count,
                             RgDrPiece *d_pieces, hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL((rg_dr_pieces_kernel<FMT>), dim3((uint32_t)count), dim3(RG_DR_LANES), 0, s, d_arena, d_planes, d_map, base, d_pieces);
}

static int dr_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const DrLayout &l, size_t n, const uint64_t fmt_piece[4], hipStream_t s) {
    const RgDrPlane *d_planes = reinterpret_cast<const RgDrPlane *>(d);
    const uint32_t *d_map = reinterpret_cast<const uint32_t *>(d + l.map);
    RgDrPiece *d_pieces = reinterpret_cast<RgDrPiece *>(d + l.pieces);
    dr_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_planes, d_map, fmt_piece[0], fmt_piece[1] - fmt_piece[0], d_pieces, s);
    dr_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_planes, d_map, fmt_piece[1], fmt_piece[2] - fmt_piece[1], d_pieces, s);
    dr_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_planes, d_map, fmt_piece[2], fmt_piece[3] - fmt_piece[2], d_pieces, s);
    RG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(rg_dr_fold_kernel, dim3((uint32_t)n), dim3(RG_DR_FOLD_LANES), 0, s, d_planes, d_pieces, reinterpret_cast<RgDrBlock *>(d + l.blocks),
                       reinterpret_cast<RgDrPlaneOut *>(d + l.res));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_dr_device(rg_ctx *c, const unsigned char *d_arena, RgDrPlane *planes, size_t n, RgDrPlaneOut *po, hipStream_t s) {
    if (!n) return RG_OK;
    uint64_t fmt_piece[4], n_blocks;
    const uint64_t n_pieces = rg_dr_plan(planes, n, fmt_piece, &n_blocks);
    if (n > 0x7fffffffu || n_pieces > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu planes, %llu pieces", n, (unsigned long long)n_pieces);
    const DrLayout l = dr_layout(n, n_pieces, n_blocks);
    std::vector<unsigned char> head;
    dr_head(planes, n, l, &head);
    RG_HIP(c, c->d_dr.reserve(l.end));
    unsigned char *d = c->d_dr.p;
    RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    const int rc = dr_launch(c, d_arena, d, l, n, fmt_piece, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(po, d + l.res, n * sizeof(RgDrPlaneOut), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_dr.h) ---------------------------------------------------------------------------------
extern "C" int rg_dr_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_dr_opts *opts, const void *arena, size_t arena_bytes,
                           rg_dr_result *out) {
    std::vector<RgDrPlane> planes;
    size_t n_planes = 0;
    const auto host = [&](char *err, size_t err_len) { return rg_dr_arena_host(route, n, descs, opts, arena, arena_bytes, out, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        rg_dr_opts o;
        int rc = rg_dr_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        planes = std::vector<RgDrPlane>(n * RG_DR_MAX_CHANNELS + 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_dr_track_planes(i, descs[i], o, false, arena_bytes, &planes[n_planes], err, err_len);
            if (rc != RG_OK) return rc;
            n_planes += descs[i].channels;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        std::vector<RgDrPlaneOut> po(n_planes ? n_planes : 1);
        const int rc = rg_dr_device(c, c->d_arena.p, planes.data(), n_planes, po.data(), s);
        if (rc != RG_OK) return rc;
        size_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_dr_fill(descs[i], planes[at].block, 0, &po[at], &out[i]);
            at += descs[i].channels;
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_dr_arena", "folded", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/dr_rate.py) -----------------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, or 32-bit integers; word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_dr_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        // floats in [-1.001, 1.001]: one in a thousand beyond full scale, as an MP3 that decodes hot has them
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.001f / 2147483648.0f)) : u;
    }
}

// the read floor: the pieces kernel's loads -- the same table, the same covers, the same loads in flight -- and one addition
// per dword; one word per piece so that nothing is optimised away
template <int FMT>
__global__ __launch_bounds__(RG_DR_LANES) void rg_dr_floor_kernel(const unsigned char *__restrict__ arena, const RgDrPlane *__restrict__ planes,
                                                                 const uint32_t *__restrict__ piece_plane, uint64_t piece_base,
                                                                 uint32_t *__restrict__ sink) {
    __shared__ uint32_t s_wave[RG_DR_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t piece = piece_base + blockIdx.x;
    const DrCover c = dr_cover<FMT>(arena, planes[piece_plane[piece]], piece);
    uint32_t sum = 0;
    for (uint32_t v = tid; v < c.nvec; v += RG_DR_STEPS * RG_DR_LANES) {
        uint4 w[RG_DR_STEPS];
#pragma unroll
        for (uint32_t u = 0; u < RG_DR_STEPS; ++u) {
            const uint32_t at = v + u * RG_DR_LANES;
            w[u] = at < c.nvec ? c.src[at] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (uint32_t u = 0; u < RG_DR_STEPS; ++u) sum += w[u].x + w[u].y + w[u].z + w[u].w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((tid & 63u) == 0) s_wave[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) sink[piece] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

template <int FMT>
static void dr_floor_format(const unsigned char *d_arena, const RgDrPlane *d_planes, const uint32_t *d_map, uint64_t base, uint64_t count, uint32_t *sink,
                            hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL((rg_dr_floor_kernel<FMT>), dim3((uint32_t)count), dim3(RG_DR_LANES), 0, s, d_arena, d_planes, d_map, base, sink);
}

extern "C" int rg_dr_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                          double *dr_ms, double *stats_ms, double *floor_ms, double *host_ms, size_t *mismatches, uint64_t *bytes) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || format > RG_FMT_S32_PLANAR || !reps || !dr_ms || !stats_ms || !floor_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_dr_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_bps(format);
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    if (bytes) *bytes = (uint64_t)n * track_bytes;
    unsigned char *d_arena = nullptr, *d = nullptr;
    uint32_t *d_sink = nullptr;
    RgStatsBench sb{};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        const rg_dr_opts o{0u, RG_DR_TOP_PERMILLE};
        std::vector<RgDrPlane> planes(2 * n);
        std::vector<RgStatsPlane> splanes(2 * n);
        char err[256] = "";
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)format;
            uint32_t reported;
            if (rg_dr_track_planes(i, t, o, false, total, &planes[2 * i], err, sizeof err) != RG_OK ||
                rg_stats_track_planes(i, t, rg_pcm_width(format), total, &splanes[2 * i], &reported, err, sizeof err) != RG_OK)
                return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_dr_rate: %s", err);
        }
        uint64_t fmt_piece[4], n_blocks;
        const uint64_t n_pieces = rg_dr_plan(planes.data(), planes.size(), fmt_piece, &n_blocks);
        if (planes.size() > 0x7fffffffu || n_pieces > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_dr_rate: too many pieces");
        const DrLayout l = dr_layout(planes.size(), n_pieces, n_blocks);
        std::vector<unsigned char> head;
        dr_head(planes.data(), planes.size(), l, &head);
        RG_HIP(c, hipMalloc((void **)&d_arena, total + 16));
        RG_HIP(c, hipMalloc((void **)&d, l.end));
        RG_HIP(c, hipMalloc((void **)&d_sink, (size_t)(n_pieces ? n_pieces : 1) * sizeof(uint32_t)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_dr_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        int lr = rg_stats_bench_setup(c, splanes.data(), splanes.size(), s, &sb);
        if (lr != RG_OK) return lr;
        RG_HIP(c, hipStreamSynchronize(s));
        const RgDrPlane *d_planes = reinterpret_cast<const RgDrPlane *>(d);
        const uint32_t *d_map = reinterpret_cast<const uint32_t *>(d + l.map);
        const auto floor_launch = [&]() -> int {
            dr_floor_format<RG_FMT_F32_PLANAR>(d_arena, d_planes, d_map, fmt_piece[0], fmt_piece[1] - fmt_piece[0], d_sink, s);
            dr_floor_format<RG_FMT_S16_PLANAR>(d_arena, d_planes, d_map, fmt_piece[1], fmt_piece[2] - fmt_piece[1], d_sink, s);
            dr_floor_format<RG_FMT_S32_PLANAR>(d_arena, d_planes, d_map, fmt_piece[2], fmt_piece[3] - fmt_piece[2], d_sink, s);
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        std::vector<RgDrPlaneOut> host_po(host_tracks ? 2 * host_tracks : 1), dev_po(planes.size());
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < 2 * host_tracks; i = next.fetch_add(1)) host_po[i] = rg_dr_serial_host(h.data(), planes[i]);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
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
        const auto dr_leg = [&]() { return dr_launch(c, d_arena, d, l, planes.size(), fmt_piece, s); };
        const auto stats_leg = [&]() { return rg_stats_bench_launch(c, d_arena, sb, s); };
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            double ms;
            if ((lr = timed(dr_leg, &ms)) != RG_OK || (lr = timed(stats_leg, &ms)) != RG_OK || (lr = timed(floor_launch, &ms)) != RG_OK) return lr;
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        if (host_tracks) host_pass();
        for (uint32_t r = 0; r < reps; ++r) {  // the legs alternate inside every round
            if ((lr = timed(dr_leg, &dr_ms[r])) != RG_OK || (lr = timed(stats_leg, &stats_ms[r])) != RG_OK || (lr = timed(floor_launch, &floor_ms[r])) != RG_OK)
                return lr;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        RG_HIP(c, hipMemcpy(dev_po.data(), d + l.res, planes.size() * sizeof(RgDrPlaneOut), hipMemcpyDeviceToHost));
        if (host_tracks) {
            *mismatches = 0;
            for (size_t i = 0; i < 2 * host_tracks; ++i) *mismatches += memcmp(&dev_po[i], &host_po[i], sizeof(RgDrPlaneOut)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_dr_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    rg_stats_bench_free(&sb);
    if (d_sink) (void)hipFree(d_sink);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
