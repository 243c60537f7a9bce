// rg_compare.hip -- the null test of two tracks on the device (include/mp3rgain_amd_compare.h, rg_compare.h): the cross-correlation
// of one track against another at every lag within the radius of a hint, over a few segments, and -- at the lag and polarity the
// host picks from those sums -- the exact moments, the count of equal samples, the largest difference and the first differing
// frame of every block of the overlap, from planes of the analysis arena in any of its three formats, the two tracks of a pair
// in the same format or not.
//
//   rg_cmp_lags_kernel     one workgroup per (pair, segment, channel, tile of RG_CMP_TILE reference frames), found in a tile ->
//                          pair table.  The stereo lag kernel's plan for planes of two tracks: both sides' q go into LDS once, as
//                          16-bit values, the b side from `hint - radius` frames before the tile's first frame to radius + 15
//                          behind its last, zero wherever that leaves the track, so the inner loop has no edge branch.  A lane
//                          owns a lag group (16 consecutive lags) and a run of strips (16 consecutive frames each): per strip 16
//                          new values of each side become doubles (the other half of its 32-value window slides over from the
//                          strip before) and 256 fused multiply-adds in double.  A lane's partial is a sum of at most 2^12
//                          products of at most 2^30: below 2^53, so the double IS the integer, whatever the order.  At radius 2047
//                          there are 256 groups for 256 lanes and a lane walks the whole tile; at radius 0 there is one group and
//                          the strips are dealt over the lanes; where the groups do not divide the lanes (129 at the default
//                          radius) the lanes left over go one each to the first groups (rg_cmp_lane_strips).  EA and EB are integer
//                          sums, the tile's frames dealt over all the lanes (one more pass over the staged values in LDS).  The partials go as 64-bit
//                          integers into the tile's sums in LDS and from there into the pair's rows by integer atomic adds.
//   rg_cmp_moments_kernel  the stereo moments kernel's plan: one workgroup per piece of RG_ST_PIECE_BYTES of one channel of one
//                          block of one pair whose tracks share a format, one launch per format.  The lanes take interleaved
//                          16-byte vectors of a's aligned cover straight into registers and for each the two vectors of b's cover
//                          that hold the same frames, shifted into place by a workgroup-uniform amount (the two planes are only
//                          sample-aligned, and `lag` moves them against each other as well); all of a lane's loads are issued
//                          before the first is used; the cover's first and last vector are taken frame by frame under a mask.
//   rg_cmp_mixed_kernel    pairs of two formats: one workgroup per piece of RG_CMP_MIXED_PIECE frames, a lane takes frames
//                          lane, lane + 256, ... one sample of each side at a time.  The plain path: such pairs are rare.
//   rg_cmp_fold_kernel     one workgroup per pair.  Lane l folds the pieces of blocks l, l + 256, ... over the channels into block
//                          rows and those into the pair's totals (integer atomics in LDS: sums, a maximum, a minimum).
// Integer sums only, and one 48-byte record per piece whose combine is associative and commutative: same input, same bits.  The
// pick between the two stages runs on the host from the rows (rg_cmp_pick), one function for every route.
#include <string.h>

#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_compare.h"
#include "rg_ctx.h"
#include "rg_pcm_seam.h"
#include "rg_st_device.h"

// ---- the lags ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_CMP_LANES) void rg_cmp_lags_kernel(const unsigned char *__restrict__ arena, const RgCmpPair *__restrict__ pairs,
                                                                  const uint32_t *__restrict__ tile_pair, uint32_t radius,
                                                                  unsigned long long *__restrict__ rows) {
    __shared__ __attribute__((aligned(16))) int16_t s_a[RG_CMP_TILE];
    __shared__ __attribute__((aligned(16))) int16_t s_b[RG_CMP_B_LDS];
    __shared__ unsigned long long s_sums[RG_CMP_LDS_SUMS];
    const uint32_t tid = threadIdx.x;
    const RgCmpPair p = pairs[tile_pair[blockIdx.x]];
    uint32_t seg, ch;
    uint64_t tstart;
    const uint32_t len = rg_cmp_tile_window(p, (uint64_t)blockIdx.x - p.first_tile, &seg, &ch, &tstart);
    const uint32_t strips = (len + RG_CMP_STRIP - 1u) / RG_CMP_STRIP, groups = rg_cmp_groups(radius), W = 2u * radius + 1u;
    const unsigned char *pa = arena + rg_cmp_plane_a(p, ch), *pb = arena + rg_cmp_plane_b(p, ch);
    // both sides into LDS, zeros behind the tile's last frame and wherever b's window leaves its track
    for (uint32_t i = tid; i < strips * RG_CMP_STRIP; i += RG_CMP_LANES) s_a[i] = i < len ? st_q_at(pa, p.fmt_a, tstart + i) : (int16_t)0;
    for (uint32_t k = tid; k < RG_CMP_STRIP * (strips + groups); k += RG_CMP_LANES) {
        const int64_t m = (int64_t)tstart + p.h + (int64_t)k - (int64_t)radius;
        s_b[k] = (m >= 0 && m < (int64_t)p.nb) ? st_q_at(pb, p.fmt_b, (uint64_t)m) : (int16_t)0;
    }
    for (uint32_t i = tid; i < RG_CMP_LDS_SUMS; i += RG_CMP_LANES) s_sums[i] = 0ull;
    __syncthreads();
    uint32_t first, g;
    const uint32_t end = rg_cmp_lane_strips(tid, groups, strips, &g, &first);
    if (first < end) {
        double acc[RG_CMP_LAG_GROUP], w[2 * RG_CMP_LAG_GROUP];
#pragma unroll
        for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j) acc[j] = 0.0;
        st_load16(s_b + RG_CMP_STRIP * (first + g), w);
        for (uint32_t c = first; c < end; ++c) {
            double l[RG_CMP_STRIP];
            st_load16(s_b + RG_CMP_STRIP * (c + g + 1u), w + RG_CMP_LAG_GROUP);
            st_load16(s_a + RG_CMP_STRIP * c, l);
#pragma unroll
            for (uint32_t i = 0; i < RG_CMP_STRIP; ++i)
#pragma unroll
                for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j) acc[j] = fma(l[i], w[i + j], acc[j]);
#pragma unroll
            for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j) w[j] = w[RG_CMP_LAG_GROUP + j];
        }
#pragma unroll
        for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j)
            if (acc[j] != 0.0) atomicAdd(&s_sums[RG_CMP_LAG_GROUP * g + j], (unsigned long long)(long long)acc[j]);
    }
    // EA and EB of the tile: the d = 0 window of b is the staged value `radius` places on
    unsigned long long ea = 0ull, eb = 0ull;
    for (uint32_t i = tid; i < len; i += RG_CMP_LANES) {
        const int32_t a = s_a[i], b = s_b[i + radius];
        ea += (unsigned long long)(uint32_t)(a * a);
        eb += (unsigned long long)(uint32_t)(b * b);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ea += __shfl_xor(ea, d, 64);
        eb += __shfl_xor(eb, d, 64);
    }
    if ((tid & 63u) == 0) {
        if (ea) atomicAdd(&s_sums[RG_CMP_LDS_SUMS - 2u], ea);
        if (eb) atomicAdd(&s_sums[RG_CMP_LDS_SUMS - 1u], eb);
    }
    __syncthreads();
    unsigned long long *row = rows + (p.first_row + (uint64_t)seg * p.cc + ch) * rg_cmp_row_len(radius);
    for (uint32_t i = tid; i < W + 2u; i += RG_CMP_LANES) {
        const unsigned long long v = s_sums[i < W ? i : RG_CMP_LDS_SUMS - 2u + (i - W)];
        if (v) atomicAdd(&row[i], v);
    }
}

// ---- the moments -------------------------------------------------------------------------------------------------------------
// where a workgroup's piece lies
struct CmpCover {
    const uint4 *a, *b;      // the aligned covers of the two planes
    uint32_t nvec_a, nvec_b; // their vectors
    uint32_t mis;            // where the piece begins in a's cover, in samples
    int32_t back;            // 0, or -1 when an a vector's frames begin in the b vector before it
    uint32_t ws, bits;       // the shift of the b pair: whole dwords, and 0 or 16 bits
    uint32_t plen;           // frames of the piece
    uint64_t first;          // the piece's first frame, in a
};
template <int FMT>
__device__ __forceinline__ CmpCover cmp_cover(const unsigned char *arena, const RgCmpPair &p, uint64_t rel) {
    constexpr uint32_t bps = FMT == RG_FMT_S16_PLANAR ? 2u : 4u, C = 16u / bps;
    uint32_t ch, blk, start;
    CmpCover c;
    c.plen = rg_cmp_piece_window(p, rel, &ch, &blk, &start);
    c.first = (uint64_t)p.m0 + start;
    const uint64_t ga = rg_cmp_plane_a(p, ch) + (uint64_t)bps * c.first, al = ga & ~(uint64_t)15;
    const uint64_t gb = rg_cmp_plane_b(p, ch) + (uint64_t)bps * (uint64_t)((int64_t)c.first + p.lag), ar = gb & ~(uint64_t)15;
    const uint32_t mis_b = (uint32_t)(gb - ar) / bps;
    c.mis = (uint32_t)(ga - al) / bps;
    c.nvec_a = ((uint32_t)(ga - al) + bps * c.plen + 15u) / 16u;
    c.nvec_b = ((uint32_t)(gb - ar) + bps * c.plen + 15u) / 16u;
    // sample j of a's vector v is frame v C + j - mis of the piece, which is sample v C + j + (mis_b - mis) of b's cover
    const int32_t delta = (int32_t)mis_b - (int32_t)c.mis;
    c.back = delta < 0 ? -1 : 0;
    const uint32_t sh = (uint32_t)(delta < 0 ? delta + (int32_t)C : delta);  // 0 .. C - 1 samples
    c.ws = sh * bps / 4u;
    c.bits = 8u * (sh * bps % 4u);
    c.a = reinterpret_cast<const uint4 *>(arena + al);
    c.b = reinterpret_cast<const uint4 *>(arena + ar);
    return c;
}
// the b vector of a pair, zeros where the cover ends
__device__ __forceinline__ uint4 cmp_b(const CmpCover &c, int32_t at) { return (uint32_t)at < c.nvec_b ? c.b[at] : uint4{0u, 0u, 0u, 0u}; }

// the workgroup's sums in lane 0: shuffles inside a wave, then the four waves' records in order
__device__ __forceinline__ RgCmpPiece cmp_reduce(RgCmpPiece acc, RgCmpPiece *s_wave, uint32_t tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        RgCmpPiece o;
        o.aa = __shfl_xor((unsigned long long)acc.aa, d, 64);
        o.bb = __shfl_xor((unsigned long long)acc.bb, d, 64);
        o.ab = (int64_t)__shfl_xor((unsigned long long)acc.ab, d, 64);
        o.first_diff = __shfl_xor((unsigned long long)acc.first_diff, d, 64);
        o.equal = __shfl_xor(acc.equal, d, 64);
        o.max_diff = __shfl_xor(acc.max_diff, d, 64);
        o.nonfinite = __shfl_xor(acc.nonfinite, d, 64);
        rg_cmp_combine(&acc, o);
    }
    if ((tid & 63u) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        for (uint32_t w = 1; w < RG_CMP_LANES / 64u; ++w) rg_cmp_combine(&acc, s_wave[w]);
    return acc;
}

template <int FMT>
__global__ __launch_bounds__(RG_CMP_LANES) void rg_cmp_moments_kernel(const unsigned char *__restrict__ arena, const RgCmpPair *__restrict__ pairs,
                                                                     const uint32_t *__restrict__ piece_pair, uint64_t piece_base,
                                                                     RgCmpPiece *__restrict__ piece_out) {
    constexpr uint32_t C = FMT == RG_FMT_S16_PLANAR ? 8u : 4u;  // samples of a vector
    __shared__ RgCmpPiece s_wave[RG_CMP_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t piece = piece_base + blockIdx.x;
    const RgCmpPair p = pairs[piece_pair[piece]];
    const CmpCover c = cmp_cover<FMT>(arena, p, piece - p.first_piece);
    const int32_t sigma = p.sigma;
    const uint64_t origin = c.first - c.mis;  // the frame of sample 0 of a's cover (it may lie before the piece: only a difference is used)
    RgCmpPiece acc = rg_cmp_empty();
    // the two a vectors that may hold samples of a neighbour: lane 0 the first, lane 1 the last, frame by frame
    if (tid < 2 && (tid == 0 || c.nvec_a > 1)) {
        const uint32_t v = tid ? c.nvec_a - 1 : 0u;
        const uint4 wa = c.a[v];
        const uint4 wb = st_shift(cmp_b(c, (int32_t)v + c.back), cmp_b(c, (int32_t)v + c.back + 1), c.ws, c.bits);
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            const uint32_t at = v * C + j;
            if (at >= c.mis && at < c.mis + c.plen) rg_cmp_take<FMT>(st_sample<FMT>(wa, j), st_sample<FMT>(wb, j), sigma, origin + at, &acc);
        }
    }
    // the vectors in between are whole: RG_ST_STEPS loads of each plane in flight per lane (a pair of zeros adds nothing to the
    // sums, differs in nothing and is taken back from the count of equal samples below)
    const uint32_t end = c.nvec_a - 1;
    uint32_t padded = 0;
    for (uint32_t v = 1 + tid; v < end; v += RG_ST_STEPS * RG_CMP_LANES) {
        uint4 wa[RG_ST_STEPS], wl[RG_ST_STEPS], wh[RG_ST_STEPS];
#pragma unroll
        for (uint32_t u = 0; u < RG_ST_STEPS; ++u) {
            const uint32_t at = v + u * RG_CMP_LANES;
            const bool in = at < end;
            wa[u] = in ? c.a[at] : uint4{0u, 0u, 0u, 0u};
            wl[u] = in ? cmp_b(c, (int32_t)at + c.back) : uint4{0u, 0u, 0u, 0u};
            wh[u] = in ? cmp_b(c, (int32_t)at + c.back + 1) : uint4{0u, 0u, 0u, 0u};
            padded += in ? 0u : C;
        }
#pragma unroll
        for (uint32_t u = 0; u < RG_ST_STEPS; ++u) {
            const uint4 wb = st_shift(wl[u], wh[u], c.ws, c.bits);
            const uint64_t at = origin + (uint64_t)(v + u * RG_CMP_LANES) * C;
#pragma unroll
            for (uint32_t j = 0; j < C; ++j) rg_cmp_take<FMT>(st_sample<FMT>(wa[u], j), st_sample<FMT>(wb, j), sigma, at + j, &acc);
        }
    }
    acc.equal -= padded;
    acc = cmp_reduce(acc, s_wave, tid);
    if (tid == 0) piece_out[piece] = acc;
}

// sample k of a plane as the stored pattern, S16 sign-extended
__device__ __forceinline__ uint32_t cmp_raw_at(const unsigned char *plane, uint32_t format, uint64_t k) {
    if (format == RG_FMT_S16_PLANAR) return (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(plane)[k];
    return reinterpret_cast<const uint32_t *>(plane)[k];
}

__global__ __launch_bounds__(RG_CMP_LANES) void rg_cmp_mixed_kernel(const unsigned char *__restrict__ arena, const RgCmpPair *__restrict__ pairs,
                                                                   const uint32_t *__restrict__ piece_pair, uint64_t piece_base,
                                                                   RgCmpPiece *__restrict__ piece_out) {
    __shared__ RgCmpPiece s_wave[RG_CMP_LANES / 64u];
    const uint32_t tid = threadIdx.x;
    const uint64_t piece = piece_base + blockIdx.x;
    const RgCmpPair p = pairs[piece_pair[piece]];
    uint32_t ch, blk, start;
    const uint32_t plen = rg_cmp_piece_window(p, piece - p.first_piece, &ch, &blk, &start);
    const unsigned char *pa = arena + rg_cmp_plane_a(p, ch), *pb = arena + rg_cmp_plane_b(p, ch);
    RgCmpPiece acc = rg_cmp_empty();
    for (uint32_t j = tid; j < plen; j += RG_CMP_LANES) {
        const uint64_t fa = (uint64_t)p.m0 + start + j, fb = (uint64_t)((int64_t)fa + p.lag);
        rg_cmp_take_mixed(p.fmt_a, cmp_raw_at(pa, p.fmt_a, fa), p.fmt_b, cmp_raw_at(pb, p.fmt_b, fb), p.sigma, fa, &acc);
    }
    acc = cmp_reduce(acc, s_wave, tid);
    if (tid == 0) piece_out[piece] = acc;
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_CMP_LANES) void rg_cmp_fold_kernel(const RgCmpPair *__restrict__ pairs, const RgCmpPiece *__restrict__ piece_in,
                                                                  rg_compare_block *__restrict__ blocks_out, RgCmpTotals *__restrict__ out) {
    __shared__ unsigned long long s_u64[6];  // aa, bb, ab, equal, nonfinite, first_diff
    __shared__ uint32_t s_u32[3];            // blocks, differing, max_diff
    const uint32_t tid = threadIdx.x;
    const RgCmpPair p = pairs[blockIdx.x];
    if (tid < 6) s_u64[tid] = tid == 5 ? RG_CMP_NONE : 0ull;
    if (tid < 3) s_u32[tid] = 0u;
    __syncthreads();
    RgCmpTotals acc;
    memset(&acc, 0, sizeof acc);
    acc.first_diff = RG_CMP_NONE;
    const uint32_t n_blocks = p.cc ? p.n_blocks : 0u;
    const uint64_t per = n_blocks ? rg_cmp_channel_pieces(p) : 0;
    const uint32_t P = rg_cmp_piece_frames(p.fmt_a, p.fmt_b);
    for (uint32_t b = tid; b < n_blocks; b += RG_CMP_LANES) {
        uint32_t start;
        const uint32_t len = rg_cmp_block_window(p, b, &start), cnt = rg_cmp_pieces_of(len, P);
        RgCmpPiece blk = rg_cmp_empty();
        for (uint32_t c = 0; c < p.cc; ++c) {
            const RgCmpPiece *in = piece_in + p.first_piece + c * per + (uint64_t)b * p.pieces_per_block;
            for (uint32_t k = 0; k < cnt; ++k) rg_cmp_combine(&blk, in[k]);
        }
        blocks_out[p.first_block + b] = rg_cmp_block_row(blk, len);
        rg_cmp_block_into(&acc, blk, len, p.cc);
    }
    if (acc.blocks) {
        atomicAdd(&s_u64[0], (unsigned long long)acc.aa);
        atomicAdd(&s_u64[1], (unsigned long long)acc.bb);
        atomicAdd(&s_u64[2], (unsigned long long)acc.ab);
        atomicAdd(&s_u64[3], (unsigned long long)acc.equal);
        atomicAdd(&s_u64[4], (unsigned long long)acc.nonfinite);
        atomicMin(&s_u64[5], (unsigned long long)acc.first_diff);
        atomicAdd(&s_u32[0], acc.blocks);
        atomicAdd(&s_u32[1], acc.differing);
        atomicMax(&s_u32[2], acc.max_diff);
    }
    __syncthreads();
    if (tid == 0) {
        RgCmpTotals o;
        o.aa = s_u64[0];
        o.bb = s_u64[1];
        o.ab = (int64_t)s_u64[2];
        o.equal = s_u64[3];
        o.nonfinite = s_u64[4];
        o.first_diff = s_u64[5];
        o.blocks = s_u32[0];
        o.differing = s_u32[1];
        o.max_diff = s_u32[2];
        o.pad = 0u;
        out[blockIdx.x] = o;
    }
}

// ---- the launcher ------------------------------------------------------------------------------------------------------------
static size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

template <int FMT>
static void cmp_launch_format(const unsigned char *d_arena, const RgCmpPair *d_pairs, const uint32_t *d_map, uint64_t base, uint64_t count,
                              RgCmpPiece *d_pieces, hipStream_t s) {
    if (!count) return;
    hipLaunchKernelGGL((rg_cmp_moments_kernel<FMT>), dim3((uint32_t)count), dim3(RG_CMP_LANES), 0, s, d_arena, d_pairs, d_map, base, d_pieces);
}

int rg_cmp_device(rg_ctx *c, const unsigned char *d_arena, RgCmpPair *pairs, size_t n, const rg_compare_opts &o, std::vector<int64_t> *rows,
                  RgCmpPicked *picked, RgCmpTotals *tot, std::vector<rg_compare_block> *blocks, hipStream_t s) {
    rows->clear();
    blocks->clear();
    if (!n) return RG_OK;
    if (o.radius > RG_CMP_MAX_RADIUS) return rg_set_err(c, RG_ERR_INVALID_ARG, "compare: radius %u is more than %u", o.radius, RG_CMP_MAX_RADIUS);
    const uint32_t RL = rg_cmp_row_len(o.radius);
    // stage B: [pair records | tile -> pair | lag rows]
    uint64_t n_rows;
    const uint64_t n_tiles = rg_cmp_plan_lags(pairs, n, &n_rows);
    if (n > 0x7fffffffu || n_tiles > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu pairs, %llu tiles", n, (unsigned long long)n_tiles);
    const size_t tmap_at = a16(n * sizeof(RgCmpPair)), rows_at = a16(tmap_at + (size_t)n_tiles * sizeof(uint32_t));
    const size_t rows_bytes = (size_t)n_rows * RL * sizeof(int64_t);
    std::vector<unsigned char> head(rows_at, 0);
    memcpy(head.data(), pairs, n * sizeof(RgCmpPair));
    {
        uint32_t *tmap = reinterpret_cast<uint32_t *>(head.data() + tmap_at);
        for (size_t i = 0; i < n; ++i)
            if (pairs[i].cc)
                for (uint64_t k = 0, cnt = rg_cmp_pair_tiles(pairs[i]); k < cnt; ++k) tmap[pairs[i].first_tile + k] = (uint32_t)i;
    }
    rows->assign((size_t)n_rows * RL, 0);
    if (n_tiles) {
        RG_HIP(c, c->d_compare.reserve(a16(rows_at + rows_bytes)));
        unsigned char *d = c->d_compare.p;
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemsetAsync(d + rows_at, 0, rows_bytes, s));
        hipLaunchKernelGGL(rg_cmp_lags_kernel, dim3((uint32_t)n_tiles), dim3(RG_CMP_LANES), 0, s, d_arena, reinterpret_cast<const RgCmpPair *>(d),
                           reinterpret_cast<const uint32_t *>(d + tmap_at), o.radius, reinterpret_cast<unsigned long long *>(d + rows_at));
        if (hipGetLastError() != hipSuccess) {
            (void)hipStreamSynchronize(s);  // (`head` is on its way)
            return rg_set_err(c, RG_ERR_DEVICE, "rg_cmp_lags_kernel: launch failed");
        }
        RG_HIP(c, hipMemcpyAsync(rows->data(), d + rows_at, rows_bytes, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
    }
    // the pick, on the host
    for (size_t i = 0; i < n; ++i) {
        memset(&picked[i], 0, sizeof picked[i]);
        memset(&tot[i], 0, sizeof tot[i]);
        if (!pairs[i].cc) continue;
        picked[i] = rg_cmp_pick(pairs[i], o, rows->data() + pairs[i].first_row * RL);
        rg_cmp_set_lag(&pairs[i], picked[i]);
    }
    // stage C: [pair records | piece -> pair | piece records | block rows | totals]
    uint64_t kind_piece[5], n_blocks;
    const uint64_t n_pieces = rg_cmp_plan_moments(pairs, n, kind_piece, &n_blocks);
    if (n_pieces > 0x7fffffffu || n_blocks > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %llu pieces, %llu blocks", (unsigned long long)n_pieces, (unsigned long long)n_blocks);
    const size_t pmap_at = a16(n * sizeof(RgCmpPair)), pieces_at = a16(pmap_at + (size_t)n_pieces * sizeof(uint32_t));
    const size_t blocks_at = a16(pieces_at + (size_t)n_pieces * sizeof(RgCmpPiece)), tot_at = a16(blocks_at + (size_t)n_blocks * sizeof(rg_compare_block));
    const size_t end_at = a16(tot_at + n * sizeof(RgCmpTotals));
    head.assign(pieces_at, 0);
    memcpy(head.data(), pairs, n * sizeof(RgCmpPair));
    {
        uint32_t *pmap = reinterpret_cast<uint32_t *>(head.data() + pmap_at);
        for (size_t i = 0; i < n; ++i)
            if (pairs[i].cc)
                for (uint64_t k = 0, cnt = rg_cmp_pair_pieces(pairs[i]); k < cnt; ++k) pmap[pairs[i].first_piece + k] = (uint32_t)i;
    }
    blocks->assign((size_t)n_blocks, rg_compare_block{});
    RG_HIP(c, c->d_compare.reserve(end_at));
    unsigned char *d = c->d_compare.p;
    const RgCmpPair *d_pairs = reinterpret_cast<const RgCmpPair *>(d);
    const uint32_t *d_pmap = reinterpret_cast<const uint32_t *>(d + pmap_at);
    RgCmpPiece *d_pieces = reinterpret_cast<RgCmpPiece *>(d + pieces_at);
    RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    cmp_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[0], kind_piece[1] - kind_piece[0], d_pieces, s);
    cmp_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[1], kind_piece[2] - kind_piece[1], d_pieces, s);
    cmp_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[2], kind_piece[3] - kind_piece[2], d_pieces, s);
    if (kind_piece[4] > kind_piece[3])
        hipLaunchKernelGGL(rg_cmp_mixed_kernel, dim3((uint32_t)(kind_piece[4] - kind_piece[3])), dim3(RG_CMP_LANES), 0, s, d_arena, d_pairs, d_pmap, kind_piece[3],
                           d_pieces);
    hipLaunchKernelGGL(rg_cmp_fold_kernel, dim3((uint32_t)n), dim3(RG_CMP_LANES), 0, s, d_pairs, d_pieces, reinterpret_cast<rg_compare_block *>(d + blocks_at),
                       reinterpret_cast<RgCmpTotals *>(d + tot_at));
    if (hipGetLastError() != hipSuccess) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rg_set_err(c, RG_ERR_DEVICE, "the compare moments kernels: launch failed");
    }
    RG_HIP(c, hipMemcpyAsync(tot, d + tot_at, n * sizeof(RgCmpTotals), hipMemcpyDeviceToHost, s));
    if (n_blocks) RG_HIP(c, hipMemcpyAsync(blocks->data(), d + blocks_at, (size_t)n_blocks * sizeof(rg_compare_block), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_compare.h) --------------------------------------------------------------------------------
extern "C" int rg_compare_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, size_t n_pairs, const rg_compare_pair *pairs,
                                const rg_compare_opts *opts, const void *arena, size_t arena_bytes, rg_compare_result *out, rg_compare_block *blocks_out,
                                size_t blocks_per_pair, int64_t *lag_sums) {
    std::vector<RgCmpPair> plan_recs;
    rg_compare_opts o;
    const auto host = [&](char *err, size_t err_len) {
        return rg_cmp_arena_host(route, n, descs, n_pairs, pairs, opts, arena, arena_bytes, out, blocks_out, blocks_per_pair, lag_sums, err, err_len);
    };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_cmp_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        if (n_pairs && !descs) {
            snprintf(err, err_len, "rg_compare_arena: null array");
            return RG_ERR_INVALID_ARG;
        }
        plan_recs = std::vector<RgCmpPair>(n_pairs + 1);
        for (size_t i = 0; i < n_pairs; ++i) {
            rc = rg_cmp_plan_pair(i, descs, n, pairs[i], o, false, arena_bytes, &plan_recs[i], err, err_len);
            if (rc != RG_OK) return rc;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        const size_t slab = (size_t)o.segments * RG_CMP_MAX_CHANNELS * rg_cmp_row_len(o.radius);
        if (lag_sums && n_pairs) memset(lag_sums, 0, n_pairs * slab * sizeof(int64_t));
        if (blocks_out && n_pairs && blocks_per_pair) memset(blocks_out, 0, n_pairs * blocks_per_pair * sizeof *blocks_out);
        std::vector<RgCmpPicked> picked(n_pairs + 1);
        std::vector<RgCmpTotals> tot(n_pairs + 1);
        std::vector<int64_t> rows;
        std::vector<rg_compare_block> blocks;
        const int rc = rg_cmp_device(c, c->d_arena.p, plan_recs.data(), n_pairs, o, &rows, picked.data(), tot.data(), &blocks, s);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n_pairs; ++i) {
            const RgCmpPair &p = plan_recs[i];
            if (!p.cc) {
                rg_cmp_fill_skipped(descs, pairs[i], o, p, 0, 0, &out[i]);
                continue;
            }
            const rg_compare_block *mine = blocks.data() + p.first_block;
            rg_cmp_fill(descs, pairs[i], o, p, picked[i], tot[i], mine, 0, 0, 0, &out[i]);
            if (lag_sums) rg_cmp_rows_out(p, o, rows.data() + p.first_row * rg_cmp_row_len(o.radius), lag_sums + i * slab);
            if (blocks_out) rg_cmp_blocks_out(p, mine, blocks_out + i * blocks_per_pair, blocks_per_pair);
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_compare_arena", "folded", n_pairs, pairs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/compare_rate.py) ----------------------------------------------------------------------------------
// pseudo-random words: 16-bit samples two per word, or floats in [-1.001, 1.001]; word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_cmp_fill_kernel(uint32_t *__restrict__ dst, uint64_t words, int as_float) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        dst[w] = as_float ? __float_as_uint(((float)(int32_t)u) * (1.001f / 2147483648.0f)) : u;
    }
}

extern "C" int rg_compare_rate(void *ctx, size_t n_tracks, size_t n_pairs, uint64_t frames, uint32_t format, const rg_compare_opts *opts, size_t host_pairs,
                               uint32_t threads, uint32_t reps, double warm_ms, double *moments_ms, double *lags_ms, double *host_ms, size_t *mismatches,
                               uint64_t *bytes, uint64_t *macs) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    rg_compare_opts o;
    char err[256] = "";
    int rc = rg_cmp_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    if (!n_pairs || 2 * n_pairs > n_tracks || !frames || frames >= ((uint64_t)1 << 31) || format > RG_FMT_S32_PLANAR || !reps || !moments_ms || !lags_ms ||
        (host_pairs && (!host_ms || !threads || !mismatches)) || host_pairs > n_pairs || !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_compare_rate: bad arguments");
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const uint32_t bps = rg_pcm_bps(format), RL = rg_cmp_row_len(o.radius);
    const size_t track_bytes = (size_t)frames * 2 * bps, stride = (track_bytes + 15) & ~(size_t)15, total = n_tracks * stride;
    if (bytes) *bytes = (uint64_t)n_pairs * 2 * track_bytes;
    unsigned char *d_arena = nullptr, *dl = nullptr, *dm = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        // pair p is tracks 2p (the reference copy) and 2p + 1, the hint 0
        std::vector<rg_track_desc> descs(n_tracks);
        for (size_t i = 0; i < n_tracks; ++i) {
            descs[i] = rg_track_desc{};
            descs[i].offset_bytes = i * stride;
            descs[i].frames = frames;
            descs[i].sample_rate = 44100;
            descs[i].channels = 2;
            descs[i].format = (uint16_t)format;
        }
        std::vector<RgCmpPair> pairs(n_pairs);
        for (size_t p = 0; p < n_pairs; ++p) {
            const rg_compare_pair pr{(uint32_t)(2 * p), (uint32_t)(2 * p + 1), 0};
            if (rg_cmp_plan_pair(p, descs.data(), n_tracks, pr, o, false, total, &pairs[p], err, sizeof err) != RG_OK)
                return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_compare_rate: %s", err);
        }
        uint64_t n_rows;
        const uint64_t n_tiles = rg_cmp_plan_lags(pairs.data(), n_pairs, &n_rows);
        if (n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_compare_rate: too many tiles");
        if (macs) {
            uint64_t per = 0;  // of the definition: every segment frame at every lag whose partner lies in b
            for (const RgCmpPair &p : pairs)
                for (uint32_t sg = 0; sg < p.n_seg; ++sg) {
                    const int64_t st = (int64_t)rg_cmp_seg_start(p, sg), en = st + p.seg_len;
                    for (int64_t d = -(int64_t)o.radius; d <= (int64_t)o.radius; ++d) {
                        const int64_t lo = st > -(p.h + d) ? st : -(p.h + d), hi = en < (int64_t)p.nb - p.h - d ? en : (int64_t)p.nb - p.h - d;
                        per += hi > lo ? (uint64_t)(hi - lo) * p.cc : 0;
                    }
                }
            *macs = per;
        }
        // the lag launch's bookkeeping
        const size_t tmap_at = a16(n_pairs * sizeof(RgCmpPair)), rows_at = a16(tmap_at + (size_t)n_tiles * sizeof(uint32_t));
        const size_t rows_bytes = (size_t)n_rows * RL * sizeof(int64_t);
        std::vector<unsigned char> head(rows_at, 0);
        memcpy(head.data(), pairs.data(), n_pairs * sizeof(RgCmpPair));
        {
            uint32_t *tmap = reinterpret_cast<uint32_t *>(head.data() + tmap_at);
            for (size_t i = 0; i < n_pairs; ++i)
                for (uint64_t k = 0, cnt = rg_cmp_pair_tiles(pairs[i]); k < cnt; ++k) tmap[pairs[i].first_tile + k] = (uint32_t)i;
        }
        RG_HIP(c, hipMalloc((void **)&d_arena, total + 16));
        RG_HIP(c, hipMalloc((void **)&dl, a16(rows_at + rows_bytes)));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_cmp_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4),
                           format == RG_FMT_F32_PLANAR ? 1 : 0);
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(2 * host_pairs * stride);
        if (host_pairs) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(dl, head.data(), head.size(), hipMemcpyHostToDevice, s));
        const auto lags_leg = [&]() -> int {
            RG_HIP(c, hipMemsetAsync(dl + rows_at, 0, rows_bytes, s));
            hipLaunchKernelGGL(rg_cmp_lags_kernel, dim3((uint32_t)n_tiles), dim3(RG_CMP_LANES), 0, s, d_arena, reinterpret_cast<const RgCmpPair *>(dl),
                               reinterpret_cast<const uint32_t *>(dl + tmap_at), o.radius, reinterpret_cast<unsigned long long *>(dl + rows_at));
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        // once: the rows, the host's pick, and the moments launch's bookkeeping from it
        int lr = lags_leg();
        if (lr != RG_OK) return lr;
        std::vector<int64_t> rows((size_t)n_rows * RL);
        RG_HIP(c, hipMemcpyAsync(rows.data(), dl + rows_at, rows_bytes, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<RgCmpPicked> picked(n_pairs);
        for (size_t i = 0; i < n_pairs; ++i) {
            picked[i] = rg_cmp_pick(pairs[i], o, rows.data() + pairs[i].first_row * RL);
            rg_cmp_set_lag(&pairs[i], picked[i]);
        }
        uint64_t kind_piece[5], n_blocks;
        const uint64_t n_pieces = rg_cmp_plan_moments(pairs.data(), n_pairs, kind_piece, &n_blocks);
        if (n_pieces > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_compare_rate: too many pieces");
        const size_t pmap_at = a16(n_pairs * sizeof(RgCmpPair)), pieces_at = a16(pmap_at + (size_t)n_pieces * sizeof(uint32_t));
        const size_t blocks_at = a16(pieces_at + (size_t)n_pieces * sizeof(RgCmpPiece)), tot_at = a16(blocks_at + (size_t)n_blocks * sizeof(rg_compare_block));
        const size_t end_at = a16(tot_at + n_pairs * sizeof(RgCmpTotals));
        head.assign(pieces_at, 0);
        memcpy(head.data(), pairs.data(), n_pairs * sizeof(RgCmpPair));
        {
            uint32_t *pmap = reinterpret_cast<uint32_t *>(head.data() + pmap_at);
            for (size_t i = 0; i < n_pairs; ++i)
                for (uint64_t k = 0, cnt = rg_cmp_pair_pieces(pairs[i]); k < cnt; ++k) pmap[pairs[i].first_piece + k] = (uint32_t)i;
        }
        RG_HIP(c, hipMalloc((void **)&dm, end_at));
        RG_HIP(c, hipMemcpyAsync(dm, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const RgCmpPair *d_pairs = reinterpret_cast<const RgCmpPair *>(dm);
        const uint32_t *d_pmap = reinterpret_cast<const uint32_t *>(dm + pmap_at);
        RgCmpPiece *d_pieces = reinterpret_cast<RgCmpPiece *>(dm + pieces_at);
        const auto moments_leg = [&]() -> int {
            cmp_launch_format<RG_FMT_F32_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[0], kind_piece[1] - kind_piece[0], d_pieces, s);
            cmp_launch_format<RG_FMT_S16_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[1], kind_piece[2] - kind_piece[1], d_pieces, s);
            cmp_launch_format<RG_FMT_S32_PLANAR>(d_arena, d_pairs, d_pmap, kind_piece[2], kind_piece[3] - kind_piece[2], d_pieces, s);
            hipLaunchKernelGGL(rg_cmp_fold_kernel, dim3((uint32_t)n_pairs), dim3(RG_CMP_LANES), 0, s, d_pairs, d_pieces,
                               reinterpret_cast<rg_compare_block *>(dm + blocks_at), reinterpret_cast<RgCmpTotals *>(dm + tot_at));
            RG_HIP(c, hipGetLastError());
            return RG_OK;
        };
        // the serial twin over the first host pairs: rows, pick, blocks, totals
        std::vector<int64_t> host_rows((size_t)(host_pairs ? pairs[host_pairs - 1].first_row + rg_cmp_pair_rows(pairs[host_pairs - 1]) : 0) * RL);
        std::vector<RgCmpPair> host_plan(pairs.begin(), pairs.begin() + host_pairs);
        std::vector<RgCmpTotals> host_tot(host_pairs ? host_pairs : 1);
        std::vector<std::vector<rg_compare_block>> host_blocks(host_pairs);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < host_pairs; i = next.fetch_add(1)) {
                    RgCmpPair &p = host_plan[i];
                    int64_t *mine = host_rows.data() + p.first_row * RL;
                    rg_cmp_lags_serial(h.data(), p, o.radius, mine);
                    rg_cmp_set_lag(&p, rg_cmp_pick(p, o, mine));
                    host_blocks[i].assign(p.n_blocks + 1, rg_compare_block{});
                    host_tot[i] = rg_cmp_moments_serial(h.data(), p, host_blocks[i].data());
                }
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
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
        const auto w0 = std::chrono::steady_clock::now();
        do {
            double ms;
            if ((lr = timed(moments_leg, &ms)) != RG_OK || (lr = timed(lags_leg, &ms)) != RG_OK) return lr;
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {  // the legs alternate inside every round
            if ((lr = timed(moments_leg, &moments_ms[r])) != RG_OK || (lr = timed(lags_leg, &lags_ms[r])) != RG_OK) return lr;
            if (host_pairs) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (!host_pairs) return RG_OK;
        // the last round's rows, totals and blocks against the twin's
        std::vector<RgCmpTotals> dev_tot(n_pairs);
        std::vector<rg_compare_block> dev_blocks((size_t)n_blocks);
        RG_HIP(c, hipMemcpyAsync(rows.data(), dl + rows_at, host_rows.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(dev_tot.data(), dm + tot_at, n_pairs * sizeof(RgCmpTotals), hipMemcpyDeviceToHost, s));
        if (n_blocks) RG_HIP(c, hipMemcpyAsync(dev_blocks.data(), dm + blocks_at, (size_t)n_blocks * sizeof(rg_compare_block), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        *mismatches = 0;
        for (size_t i = 0; i < host_pairs; ++i) {
            const RgCmpPair &p = pairs[i], &q = host_plan[i];
            const size_t at = p.first_row * RL, len = rg_cmp_pair_rows(p) * RL;
            const bool same = q.lag == p.lag && q.sigma == p.sigma && q.n_blocks == p.n_blocks && memcmp(&rows[at], &host_rows[at], len * sizeof(int64_t)) == 0 &&
                              memcmp(&dev_tot[i], &host_tot[i], sizeof(RgCmpTotals)) == 0 &&
                              memcmp(&dev_blocks[p.first_block], host_blocks[i].data(), p.n_blocks * sizeof(rg_compare_block)) == 0;
            *mismatches += same ? 0 : 1;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_compare_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (dm) (void)hipFree(dm);
    if (dl) (void)hipFree(dl);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
