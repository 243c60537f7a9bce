// rg_stereo.hip -- the stereo image scan on the device (include/mp3rgain_amd_stereo.h, rg_stereo.h): the exact moments of
// channels 0 and 1 of every block, the raw comparisons, and the cross-correlation of the two channels at every lag within the
// radius, from the planes of the analysis arena in any of its three formats.
//
//   rg_st_moments_kernel  one workgroup per piece of RG_ST_PIECE_BYTES of each plane of one block of one track, many tracks per
//                         launch, one launch per format; the workgroup finds its track in a piece -> track table.  The lanes take
//                         interleaved, coalesced 16-byte vectors of the LEFT plane's aligned cover straight into registers, and
//                         for each of them the two vectors of the RIGHT plane's aligned cover that hold the same frames: the two
//                         planes are only sample-aligned and their alignments modulo 16 bytes are independent, so the right pair
//                         is shifted into place by a workgroup-uniform number of samples (selects and a funnel shift, no indexed
//                         registers).  All of a lane's loads are issued before the first is used.  The first and the last vector
//                         of the left cover are taken frame by frame under a mask, by two lanes; a cover reaches at most 15 bytes
//                         outside its plane, never outside the arena's allocation of whole 16-byte words.  Lane shuffles and four
//                         LDS records reduce the workgroup; one 40-byte record per piece.  No float sums.
//   rg_st_lags_kernel     one workgroup per tile of RG_ST_TILE frames of one track, found in a tile -> track table.  Both planes'
//                         q go into LDS once, as 16-bit values, the right plane with `radius` frames of margin in front and up to
//                         radius + 15 behind, zero where the margin leaves the track, so the inner loop has no edge branch.  A
//                         lane owns a lag group (16 consecutive lags) and a run of strips (16 consecutive frames each): per strip
//                         it converts 16 left values and 16 new right values to double (the other 16 of its 32-value window slide
//                         over from the strip before) and makes 256 fused multiply-adds in double.  A lane's partial is a sum of at
//                         most 2^12 products of at most 2^30: below 2^53, so the double IS the integer, whatever the order.  The
//                         partials go as 64-bit integers into the tile's sums in LDS and from there into the track's by integer
//                         atomic adds.
//   rg_st_fold_kernel     one workgroup per track.  Lane l folds the pieces of blocks l, l + 256, ... into block sums and those
//                         into the track's totals and block counts (integer atomics in LDS); the two lags are chosen by a tree
//                         under the host's total order.  One 96-byte record per track.
// Integers and a total order: same input, same bits.  The launcher's callers check every track against the arena first.
#include <string.h>

#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_pcm_seam.h"
#include "rg_st_device.h"
#include "rg_stereo.h"

// ---- the moments -----------------------------------------------------------------------------------------------------------
// (st_sample and st_shift: rg_st_device.h)
// where a workgroup's piece lies
struct StCover {
    const uint4 *l, *r;      // the aligned covers of the two planes
    uint32_t nvec_l, nvec_r; // their vectors
    uint32_t mis;            // where the piece begins in the left cover, in samples
    int32_t back;            // 0, or -1 when a left vector's frames begin in the right vector before it
    uint32_t ws, bits;       // the shift of the right pair: whole dwords, and 0 or 16 bits
    uint32_t plen;           // frames of the piece
};
template <int FMT>
__device__ __forceinline__ StCover st_cover(const unsigned char *arena, const RgStTrack &t, uint64_t piece) {
    constexpr uint32_t bps = FMT == RG_FMT_S16_PLANAR ? 2u : 4u, C = 16u / bps;
    const uint32_t rel = (uint32_t)(piece - t.first_piece);
    const uint32_t b = rel / t.pieces_per_block, k = rel - b * t.pieces_per_block;
    uint64_t bstart;
    const uint32_t len = rg_st_block_window(t, b, &bstart);
    uint32_t pstart;
    StCover c;
    c.plen = rg_st_piece_window(len, k, FMT, &pstart);
    const uint64_t gl = t.off_l + (uint64_t)bps * (bstart + pstart), al = gl & ~(uint64_t)15;
    const uint64_t gr = t.off_r + (uint64_t)bps * (bstart + pstart), ar = gr & ~(uint64_t)15;
    const uint32_t mis_r = (uint32_t)(gr - ar) / bps;
    c.mis = (uint32_t)(gl - al) / bps;
    c.nvec_l = ((uint32_t)(gl - al) + bps * c.plen + 15u) / 16u;
    c.nvec_r = ((uint32_t)(gr - ar) + bps * c.plen + 15u) / 16u;
    // sample j of left vector v is frame v C + j - mis, which is sample v C + j + (mis_r - mis) of the right cover
    const int32_t delta = (int32_t)mis_r - (int32_t)c.mis;
    c.back = delta < 0 ? -1 : 0;
    const uint32_t sh = (uint32_t)(delta < 0 ? delta + (int32_t)C : delta);  // 0 .. C - 1 samples
    c.ws = sh * bps / 4u;
    c.bits = 8u * (sh * bps % 4u);
    c.l = reinterpret_cast<const uint4 *>(arena + al);
    c.r = reinterpret_cast<const uint4 *>(arena + ar);
    return c;
}
// the right vector of a pair, zeros where the cover ends
__device__ __forceinline__ uint4 st_right(const StCover &c, int32_t at) { return (uint32_t)at < c.nvec_r ? c.r[at] : uint4{0u, 0u, 0u, 0u}; }

// the workgroup's sums in lane 0: shuffles inside a wave, then the four waves' records in order
template <int FMT>
__device__ __forceinline__ RgStPiece st_reduce(RgStPiece acc, RgStPiece *s_wave, uint32_t tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        RgStPiece o;
        o.ll = __shfl_xor((unsigned long long)acc.ll, d, 64);
        o.rr = __shfl_xor((unsigned long long)acc.rr, d, 64);
        o.lr = (int64_t)__shfl_xor((unsigned long long)acc.lr, d, 64);
        o.equal = __shfl_xor(acc.equal, d, 64);
        o.opposite = __shfl_xor(acc.opposite, d, 64);
        o.zero = __shfl_xor(acc.zero, d, 64);
        o.nonfinite = FMT == RG_FMT_F32_PLANAR ? __shfl_xor(acc.nonfinite, d, 64) : 0u;
        rg_st_combine(&acc, o);
    }
    if ((tid & 63u) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        for (uint32_t w = 1; w < RG_ST_LANES / 64u; ++w) rg_st_combine(&acc, s_wave[w]);
    return acc;
}

template <int FMT>
__global__ __launch_bounds__(RG_ST_LANES) void rg_st_moments_kernel(const unsigned char *__restrict__ arena, const RgStTrack *__restrict__ tracks,
                                                                   const uint32_t *__restrict__ piece_track, uint64_t piece_base,
                                                                   RgStPiece *__restrict__ piece_out) {
    constexpr uint32_t C = FMT == RG_FMT_S16_PLANAR ? 8u : 4u;  // samples of a vector
    __shared__ RgStPiece s_wave[RG_ST_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t piece = piece_base + blockIdx.x;
    const StCover c = st_cover<FMT>(arena, tracks[piece_track[piece]], piece);
    RgStPiece acc = rg_st_empty();
    // the two left vectors that may hold samples of a neighbour: lane 0 the first, lane 1 the last, frame by frame
    if (tid < 2 && (tid == 0 || c.nvec_l > 1)) {
        const uint32_t v = tid ? c.nvec_l - 1 : 0u;
        const uint4 wl = c.l[v];
        const uint4 wr = st_shift(st_right(c, (int32_t)v + c.back), st_right(c, (int32_t)v + c.back + 1), c.ws, c.bits);
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            const uint32_t at = v * C + j;
            if (at >= c.mis && at < c.mis + c.plen) rg_st_take<FMT>(st_sample<FMT>(wl, j), st_sample<FMT>(wr, j), &acc);
        }
    }
    // the vectors in between are whole: RG_ST_STEPS loads of each plane in flight per lane (a frame of zeros adds nothing to the
    // sums and is taken back from the counts of equal and zero frames below)
    const uint32_t end = c.nvec_l - 1;
    uint32_t padded = 0;
    for (uint32_t v = 1 + tid; v < end; v += RG_ST_STEPS * RG_ST_LANES) {
        uint4 wl[RG_ST_STEPS], wa[RG_ST_STEPS], wb[RG_ST_STEPS];
#pragma unroll
        for (uint32_t u = 0; u < RG_ST_STEPS; ++u) {
            const uint32_t at = v + u * RG_ST_LANES;
            const bool in = at < end;
            wl[u] = in ? c.l[at] : uint4{0u, 0u, 0u, 0u};
            wa[u] = in ? st_right(c, (int32_t)at + c.back) : uint4{0u, 0u, 0u, 0u};
            wb[u] = in ? st_right(c, (int32_t)at + c.back + 1) : uint4{0u, 0u, 0u, 0u};
            padded += in ? 0u : C;
        }
#pragma unroll
        for (uint32_t u = 0; u < RG_ST_STEPS; ++u) {
            const uint4 wr = st_shift(wa[u], wb[u], c.ws, c.bits);
#pragma unroll
            for (uint32_t j = 0; j < C; ++j) rg_st_take<FMT>(st_sample<FMT>(wl[u], j), st_sample<FMT>(wr, j), &acc);
        }
    }
    acc.equal -= padded;
    acc.zero -= padded;
    acc = st_reduce<FMT>(acc, s_wave, tid);
    if (tid == 0) piece_out[piece] = acc;
}

// ---- the lags --------------------------------------------------------------------------------------------------------------
// (st_q_at and st_load16: rg_st_device.h)
__global__ __launch_bounds__(RG_ST_LANES) void rg_st_lags_kernel(const unsigned char *__restrict__ arena, const RgStTrack *__restrict__ tracks,
                                                                const uint32_t *__restrict__ tile_track, uint32_t radius,
                                                                unsigned long long *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) int16_t s_left[RG_ST_TILE];
    __shared__ __attribute__((aligned(16))) int16_t s_right[RG_ST_RIGHT_LDS];
    __shared__ unsigned long long s_sums[RG_ST_LAG_GROUP * RG_ST_MAX_GROUPS];
    const uint32_t tid = threadIdx.x;
    const uint32_t ti = tile_track[blockIdx.x];
    const RgStTrack t = tracks[ti];
    uint64_t tstart;
    const uint32_t len = rg_st_tile_window(t, (uint32_t)(blockIdx.x - t.first_tile), &tstart);
    const uint32_t strips = (len + RG_ST_STRIP - 1u) / RG_ST_STRIP, groups = rg_st_groups(radius), W = 2u * radius + 1u;
    const unsigned char *pl = arena + t.off_l, *pr = arena + t.off_r;
    // both planes into LDS, zeros behind the tile's last frame and wherever the right margin leaves the track
    for (uint32_t i = tid; i < strips * RG_ST_STRIP; i += RG_ST_LANES) s_left[i] = i < len ? st_q_at(pl, t.format, tstart + i) : (int16_t)0;
    for (uint32_t p = tid; p < RG_ST_STRIP * (strips + groups); p += RG_ST_LANES) {
        const int64_t m = (int64_t)tstart + (int64_t)p - (int64_t)radius;
        s_right[p] = (m >= 0 && m < (int64_t)t.n) ? st_q_at(pr, t.format, (uint64_t)m) : (int16_t)0;
    }
    for (uint32_t i = tid; i < RG_ST_LAG_GROUP * RG_ST_MAX_GROUPS; i += RG_ST_LANES) s_sums[i] = 0ull;
    __syncthreads();
    uint32_t first;
    const uint32_t end = rg_st_lane_strips(tid, groups, strips, &first), g = tid % groups;
    if (first < end) {
        double acc[RG_ST_LAG_GROUP], w[2 * RG_ST_LAG_GROUP];
#pragma unroll
        for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j) acc[j] = 0.0;
        st_load16(s_right + RG_ST_STRIP * (first + g), w);
        for (uint32_t c = first; c < end; ++c) {
            double l[RG_ST_STRIP];
            st_load16(s_right + RG_ST_STRIP * (c + g + 1u), w + RG_ST_LAG_GROUP);
            st_load16(s_left + RG_ST_STRIP * c, l);
#pragma unroll
            for (uint32_t i = 0; i < RG_ST_STRIP; ++i)
#pragma unroll
                for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j) acc[j] = fma(l[i], w[i + j], acc[j]);
#pragma unroll
            for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j) w[j] = w[RG_ST_LAG_GROUP + j];
        }
#pragma unroll
        for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j)
            if (acc[j] != 0.0) atomicAdd(&s_sums[RG_ST_LAG_GROUP * g + j], (unsigned long long)(long long)acc[j]);
    }
    __syncthreads();
    for (uint32_t i = tid; i < W; i += RG_ST_LANES) {
        const unsigned long long v = s_sums[i];
        if (v) atomicAdd(&sums[(uint64_t)ti * W + i], v);
    }
}

// ---- the fold --------------------------------------------------------------------------------------------------------------
struct StPick {
    int64_t c;
    int32_t d;
};
__device__ __forceinline__ StPick st_pick_shfl(const StPick &p, int d) {
    StPick o;
    o.c = (int64_t)__shfl_xor((unsigned long long)p.c, d, 64);
    o.d = __shfl_xor(p.d, d, 64);
    return o;
}

__global__ __launch_bounds__(RG_ST_LANES) void rg_st_fold_kernel(const RgStTrack *__restrict__ tracks, const RgStPiece *__restrict__ piece_in,
                                                                const long long *__restrict__ sums, uint32_t radius, RgStTotals *__restrict__ out) {
    __shared__ unsigned long long s_u64[7];  // ell, err, elr, equal, opposite, zero, nonfinite
    __shared__ uint32_t s_u32[4];            // blocks, active, neg, mono
    __shared__ StPick s_hi[RG_ST_LANES / 64u], s_lo[RG_ST_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const RgStTrack t = tracks[blockIdx.x];
    if (tid < 7) s_u64[tid] = 0ull;
    if (tid < 4) s_u32[tid] = 0u;
    __syncthreads();
    // the pieces of a block in ascending order, the block into the lane's totals
    RgStTotals acc;
    memset(&acc, 0, sizeof acc);
    for (uint32_t b = tid; b < t.n_blocks; b += RG_ST_LANES) {
        uint64_t bstart;
        const uint32_t len = rg_st_block_window(t, b, &bstart);
        const RgStPiece *in = piece_in + t.first_piece + (uint64_t)b * t.pieces_per_block;
        const uint32_t cnt = rg_st_pieces_of(len, t.format);
        RgStPiece blk = rg_st_empty();
        for (uint32_t k = 0; k < cnt; ++k) rg_st_combine(&blk, in[k]);
        rg_st_block_into(&acc, blk, len);
    }
    if (acc.blocks) {
        atomicAdd(&s_u64[0], (unsigned long long)acc.ell);
        atomicAdd(&s_u64[1], (unsigned long long)acc.err);
        atomicAdd(&s_u64[2], (unsigned long long)acc.elr);
        atomicAdd(&s_u64[3], (unsigned long long)acc.equal);
        atomicAdd(&s_u64[4], (unsigned long long)acc.opposite);
        atomicAdd(&s_u64[5], (unsigned long long)acc.zero);
        atomicAdd(&s_u64[6], (unsigned long long)acc.nonfinite);
        atomicAdd(&s_u32[0], acc.blocks);
        atomicAdd(&s_u32[1], acc.active);
        atomicAdd(&s_u32[2], acc.neg);
        atomicAdd(&s_u32[3], acc.mono);
    }
    // the two lags: a lane's candidates (a lane without one repeats the first), the wave, the four waves
    const uint32_t W = 2u * radius + 1u;
    const long long *mine = sums + (uint64_t)blockIdx.x * W;
    const uint32_t a = tid < W ? tid : 0u, b2 = tid + RG_ST_LANES;
    StPick hi{mine[a], (int32_t)a - (int32_t)radius}, lo = hi;
    if (b2 < W) {
        const StPick p{mine[b2], (int32_t)b2 - (int32_t)radius};
        if (rg_st_better(p.c, p.d, hi.c, hi.d)) hi = p;
        if (rg_st_lower(p.c, p.d, lo.c, lo.d)) lo = p;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const StPick oh = st_pick_shfl(hi, d), ol = st_pick_shfl(lo, d);
        if (rg_st_better(oh.c, oh.d, hi.c, hi.d)) hi = oh;
        if (rg_st_lower(ol.c, ol.d, lo.c, lo.d)) lo = ol;
    }
    if ((tid & 63u) == 0) {
        s_hi[tid >> 6] = hi;
        s_lo[tid >> 6] = lo;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < RG_ST_LANES / 64u; ++w) {
            if (rg_st_better(s_hi[w].c, s_hi[w].d, hi.c, hi.d)) hi = s_hi[w];
            if (rg_st_lower(s_lo[w].c, s_lo[w].d, lo.c, lo.d)) lo = s_lo[w];
        }
        RgStTotals o;
        o.ell = s_u64[0];
        o.err = s_u64[1];
        o.elr = (int64_t)s_u64[2];
        o.equal = s_u64[3];
        o.opposite = s_u64[4];
        o.zero = s_u64[5];
        o.nonfinite = s_u64[6];
        o.lag_sum = hi.c;
        o.anti_sum = lo.c;
        o.blocks = s_u32[0];
        o.active = s_u32[1];
        o.neg = s_u32[2];
        o.mono = s_u32[3];
        o.lag = hi.d;
        o.anti_lag = lo.d;
        out[blockIdx.x] = o;
    }
}

// Device layout of one launch's bookkeeping, every part 16-byte aligned:
// [track records | piece -> track | tile -> track | piece records | lag sums | results]
struct StLayout {
    size_t pmap, tmap, pieces, sums, res, end;
};
static StLayout st_layout(size_t n, uint64_t n_pieces, uint64_t n_tiles, uint32_t W) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    StLayout l;
    l.pmap = a16(n * sizeof(RgStTrack));
    l.tmap = a16(l.pmap + (size_t)n_pieces * sizeof(uint32_t));
    l.pieces = a16(l.tmap + (size_t)n_tiles * sizeof(uint32_t));
    l.sums = a16(l.pieces + (size_t)n_pieces * sizeof(RgStPiece));
    l.res = a16(l.sums + n * W * sizeof(int64_t));
    l.end = a16(l.res + n * sizeof(RgStTotals));
    return l;
}
// the head of the bookkeeping as the host builds it: the planned records and the two tables
static void st_head(const RgStTrack *tracks, size_t n, const StLayout &l, std::vector<unsigned char> *head) {
    head->assign(l.pieces, 0);
    if (n) memcpy(head->data(), tracks, n * sizeof(RgStTrack));
    uint32_t *pmap = reinterpret_cast<uint32_t *>(head->data() + l.pmap), *tmap = reinterpret_cast<uint32_t *>(head->data() + l.tmap);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t cnt = rg_st_track_pieces(tracks[i]);
        for (uint64_t k = 0; k < cnt; ++k) pmap[tracks[i].first_piece + k] = (uint32_t)i;
        for (uint32_t k = 0; k < tracks[i].n_tiles; ++k) tmap[tracks[i].first_tile + k] = (uint32_t)i;
    }
}

template <int FMT>
static void st_launch_format(const unsigned char *d_arena, const RgStTrack *d_tracks, const uint32_t *d_map, uint64_t base, uint64_t count,
                             RgStPiece *d_pieces, hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL((rg_st_moments_kernel<FMT>), dim3((uint32_t)count), dim3(RG_ST_LANES), 0, s, d_arena, d_tracks, d_map, base, d_pieces);
}

static int st_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const StLayout &l, size_t n, const uint64_t fmt_piece[4], uint64_t n_tiles,
                     uint32_t radius, hipStream_t s) {
    const RgStTrack *d_tracks = reinterpret_cast<const RgStTrack *>(d);
    const uint32_t *d_pmap = reinterpret_cast<const uint32_t *>(d + l.pmap), *d_tmap = reinterpret_cast<const uint32_t *>(d + l.tmap);
    RgStPiece *d_pieces = reinterpret_cast<RgStPiece *>(d + l.pieces);
    RG_HIP(c, hipMemsetAsync(d + l.sums, 0, l.res - l.sums, s));
    st_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[0], fmt_piece[1] - fmt_piece[0], d_pieces, s);
    st_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[1], fmt_piece[2] - fmt_piece[1], d_pieces, s);
    st_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[2], fmt_piece[3] - fmt_piece[2], d_pieces, s);
    RG_HIP(c, hipGetLastError());
    if (n_tiles) {
        hipLaunchKernelGGL(rg_st_lags_kernel, dim3((uint32_t)n_tiles), dim3(RG_ST_LANES), 0, s, d_arena, d_tracks, d_tmap, radius,
                           reinterpret_cast<unsigned long long *>(d + l.sums));
        RG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(rg_st_fold_kernel, dim3((uint32_t)n), dim3(RG_ST_LANES), 0, s, d_tracks, d_pieces, reinterpret_cast<const long long *>(d + l.sums), radius,
                       reinterpret_cast<RgStTotals *>(d + l.res));
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_st_device(rg_ctx *c, const unsigned char *d_arena, RgStTrack *tracks, size_t n, uint32_t radius, RgStTotals *tot, int64_t *sums, hipStream_t s) {
    if (!n) return RG_OK;
    if (radius > RG_ST_MAX_RADIUS) return rg_set_err(c, RG_ERR_INVALID_ARG, "stereo: radius %u is more than %u", radius, RG_ST_MAX_RADIUS);
    uint64_t fmt_piece[4], n_tiles;
    const uint64_t n_pieces = rg_st_plan(tracks, n, fmt_piece, &n_tiles);
    if (n > 0x7fffffffu || n_pieces > 0x7fffffffu || n_tiles > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu tracks, %llu pieces, %llu tiles", n, (unsigned long long)n_pieces,
                          (unsigned long long)n_tiles);
    const uint32_t W = 2u * radius + 1u;
    const StLayout l = st_layout(n, n_pieces, n_tiles, W);
    std::vector<unsigned char> head;
    st_head(tracks, n, l, &head);
    RG_HIP(c, c->d_stereo.reserve(l.end));
    unsigned char *d = c->d_stereo.p;
    RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    const int rc = st_launch(c, d_arena, d, l, n, fmt_piece, n_tiles, radius, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(tot, d + l.res, n * sizeof(RgStTotals), hipMemcpyDeviceToHost, s));
    if (sums) RG_HIP(c, hipMemcpyAsync(sums, d + l.sums, n * W * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_stereo.h) -----------------------------------------------------------------------------
extern "C" int rg_stereo_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_stereo_opts *opts, const void *arena, size_t arena_bytes,
                               rg_stereo_result *out, int64_t *lag_sums) {
    std::vector<RgStTrack> tracks;
    rg_stereo_opts o;
    const auto host = [&](char *err, size_t err_len) { return rg_st_arena_host(route, n, descs, opts, arena, arena_bytes, out, lag_sums, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_st_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        tracks = std::vector<RgStTrack>(n + 1);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_st_track(i, descs[i], o, false, arena_bytes, &tracks[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        std::vector<RgStTotals> tot(n ? n : 1);
        const int rc = rg_st_device(c, c->d_arena.p, tracks.data(), n, o.radius, tot.data(), lag_sums, s);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) rg_st_fill(descs[i], o, tracks[i].block, 0, tot[i], &out[i]);
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_stereo_arena", "folded", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/stereo_rate.py) -------------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, or 32-bit integers; word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_st_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        // floats in [-1.001, 1.001]: one in a thousand beyond full scale, as an MP3 that decodes hot has them
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.001f / 2147483648.0f)) : u;
    }
}

extern "C" int rg_stereo_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, uint32_t radius, size_t host_tracks, uint32_t threads, uint32_t reps,
                              double warm_ms, double *moments_ms, double *lags_ms, double *host_ms, size_t *mismatches, uint64_t *bytes, uint64_t *macs) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || format > RG_FMT_S32_PLANAR || radius > RG_ST_MAX_RADIUS || !reps || !moments_ms || !lags_ms ||
        (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_stereo_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_bps(format), W = 2u * radius + 1u;
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    if (bytes) *bytes = (uint64_t)n * track_bytes;
    if (macs) {
        uint64_t per = 0;
        for (int64_t d = -(int64_t)radius; d <= (int64_t)radius; ++d) per += frames > (uint64_t)(d < 0 ? -d : d) ? frames - (uint64_t)(d < 0 ? -d : d) : 0;
        *macs = per * n;
    }
    unsigned char *d_arena = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        const rg_stereo_opts o{0u, radius, RG_ST_DEFAULT_PHASE_PERMILLE, RG_ST_DEFAULT_DELAY_PERMILLE, RG_ST_DEFAULT_MONO_DB, RG_ST_DEFAULT_BALANCE_DB};
        std::vector<RgStTrack> tracks(n);
        char err[256] = "";
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = (uint16_t)format;
            if (rg_st_track(i, t, o, false, total, &tracks[i], err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_stereo_rate: %s", err);
        }
        uint64_t fmt_piece[4], n_tiles;
        const uint64_t n_pieces = rg_st_plan(tracks.data(), n, fmt_piece, &n_tiles);
        if (n > 0x7fffffffu || n_pieces > 0x7fffffffu || n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_stereo_rate: too many pieces");
        const StLayout l = st_layout(n, n_pieces, n_tiles, W);
        std::vector<unsigned char> head;
        st_head(tracks.data(), n, l, &head);
        RG_HIP(c, hipMalloc((void **)&d_arena, total + 16));
        RG_HIP(c, hipMalloc((void **)&d, l.end));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_st_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemsetAsync(d + l.sums, 0, l.end - l.sums, s));  // (the first fold runs before the first lag leg)
        RG_HIP(c, hipStreamSynchronize(s));
        const RgStTrack *d_tracks = reinterpret_cast<const RgStTrack *>(d);
        const uint32_t *d_pmap = reinterpret_cast<const uint32_t *>(d + l.pmap), *d_tmap = reinterpret_cast<const uint32_t *>(d + l.tmap);
        RgStPiece *d_pieces = reinterpret_cast<RgStPiece *>(d + l.pieces);
        const auto fold_launch = [&]() -> int {
            hipLaunchKernelGGL(rg_st_fold_kernel, dim3((uint32_t)n), dim3(RG_ST_LANES), 0, s, d_tracks, d_pieces, reinterpret_cast<const long long *>(d + l.sums),
                               radius, reinterpret_cast<RgStTotals *>(d + l.res));
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        const auto moments_leg = [&]() -> int {
            st_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[0], fmt_piece[1] - fmt_piece[0], d_pieces, s);
            st_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[1], fmt_piece[2] - fmt_piece[1], d_pieces, s);
            st_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_tracks, d_pmap, fmt_piece[2], fmt_piece[3] - fmt_piece[2], d_pieces, s);
            RG_HIP(c, hipGetLastError());
            return fold_launch();
        };
        const auto lags_leg = [&]() -> int {
            RG_HIP(c, hipMemsetAsync(d + l.sums, 0, l.res - l.sums, s));
            hipLaunchKernelGGL(rg_st_lags_kernel, dim3((uint32_t)n_tiles), dim3(RG_ST_LANES), 0, s, d_arena, d_tracks, d_tmap, radius,
                               reinterpret_cast<unsigned long long *>(d + l.sums));
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        std::vector<RgStTotals> host_tot(host_tracks ? host_tracks : 1), dev_tot(n);
        std::vector<int64_t> host_sums((host_tracks ? host_tracks : 1) * (size_t)W), dev_sums((host_tracks ? host_tracks : 1) * (size_t)W);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < host_tracks; i = next.fetch_add(1)) host_tot[i] = rg_st_serial_host(h.data(), tracks[i], radius, &host_sums[i * W]);
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
        int lr;
        // the warm-up: a fresh process runs slower for a while after a large allocation
        const auto w0 = std::chrono::steady_clock::now();
        do {
            double ms;
            if ((lr = timed(moments_leg, &ms)) != RG_OK || (lr = timed(lags_leg, &ms)) != RG_OK) return lr;
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {  // the legs alternate inside every round
            if ((lr = timed(moments_leg, &moments_ms[r])) != RG_OK || (lr = timed(lags_leg, &lags_ms[r])) != RG_OK) return lr;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if ((lr = fold_launch()) != RG_OK) return lr;  // the totals of the last round's pieces and sums
        RG_HIP(c, hipMemcpyAsync(dev_tot.data(), d + l.res, n * sizeof(RgStTotals), hipMemcpyDeviceToHost, s));
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(dev_sums.data(), d + l.sums, host_tracks * W * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        if (host_tracks) {
            *mismatches = 0;
            for (size_t i = 0; i < host_tracks; ++i)
                *mismatches += (memcmp(&dev_tot[i], &host_tot[i], sizeof(RgStTotals)) != 0 || memcmp(&dev_sums[i * W], &host_sums[i * W], W * sizeof(int64_t)) != 0) ? 1 : 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_stereo_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
