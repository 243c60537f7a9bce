// rg_r128_inl.h -- the device helpers the kernels of the EBU R 128 path share (rg_r128.hip, rg_r128_range.hip,
// rg_r128_albums.hip): a block's value, the fixed fold tree, the radix select's steps.  Every summation order has its one
// definition here, so that a track's kernels and an album's, in different translation units, agree to the bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rg_r128.h"

// ---- a gating block's value (rg_r128_gate_kernel, rg_r128a_gate_kernel), and the fold of every gate pass ------------------
namespace {

__device__ __forceinline__ double r128_block_z(const RgR128TrackDev &T, const uint32_t b) {
    const double *e0 = T.e + b;
    double s;
    if (T.nch >= 2) {
        const double *e1 = e0 + T.H;
        s = (((e0[0] + e1[0]) + (e0[1] + e1[1])) + (e0[2] + e1[2])) + (e0[3] + e1[3]);
    } else {
        s = ((e0[0] + e0[1]) + e0[2]) + e0[3];
    }
    return s / (4.0 * (double)T.hop);
}

// sum and count over the workgroup (256 threads), in a fixed tree
__device__ __forceinline__ void r128_fold(double *sh_sum, uint32_t *sh_cnt, double &sum, uint32_t &cnt) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh_sum[tid] = sum;
    sh_cnt[tid] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sh_sum[tid] += sh_sum[tid + s];
            sh_cnt[tid] += sh_cnt[tid + s];
        }
        __syncthreads();
    }
    sum = sh_sum[0];
    cnt = sh_cnt[0];
}

}  // namespace

// ---- loudness range (rg_r128r_*, rg_r128a_*) ------------------------------------------------------------------------------
#define RG_R128R_ST_HOPS 30
#define RG_R128R_BINS 4096      // 12-bit digit: two histograms are 32 KiB of LDS
#define RG_R128R_PASSES 6       // 5 x 12 bits + 4 bits
#define RG_R128R_WIDE 256       // slices of a wide album's threshold sum; its counting workgroups at most
#define RG_R128R_WIDE_FROM 16384u  // measured: one workgroup is ahead at 7 k blocks, level at 18 k, 0.4 ms behind at 66 k

struct RgR128RangeTrack {
    const double *e;     // hop energies [nch][H]
    uint64_t st_base;    // first short-term block of the track in the block array
    uint32_t chunk_base; // first workgroup of the track in stage 1
    uint32_t H, nch, hop, st_count, pad;
};

struct RgR128RangeSel {  // the state of a wide album selection, on the device
    double thr;
    uint64_t prefix[2], mask;
    uint32_t rank[2];
    uint32_t n, pad;
};

// one wide selection's device state: RgR128RangeSel[PASSES + 1] | psum[2][WIDE] | pcnt[2][WIDE] | ghist[PASSES][2 * BINS]
constexpr size_t kWideSel = 0, kWidePsum = 512, kWidePcnt = kWidePsum + 2 * RG_R128R_WIDE * sizeof(double),
                 kWideHist = kWidePcnt + 2 * RG_R128R_WIDE * sizeof(uint32_t),
                 kWideBytes = kWideHist + (size_t)RG_R128R_PASSES * 2 * RG_R128R_BINS * sizeof(uint32_t);
static_assert((RG_R128R_PASSES + 1) * sizeof(RgR128RangeSel) <= kWidePsum, "the selection states fit their slot");

namespace {

__device__ __forceinline__ unsigned long long r128r_umax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__device__ __forceinline__ int r128r_shift(const int pass) { return pass < RG_R128R_PASSES - 1 ? 52 - 12 * pass : 0; }
__device__ __forceinline__ int r128r_width(const int pass) { return pass < RG_R128R_PASSES - 1 ? 12 : 4; }

// hist: RG_R128R_BINS counters in LDS.  The bin that holds the element of rank `rank` (0-based, below the counters' sum) and
// its rank within that bin go to pick[0], pick[1]; every thread may read them after the call.
__device__ __forceinline__ void r128r_find_bin(const uint32_t *hist, uint32_t *scan, uint32_t *pick, const uint32_t rank) {
    constexpr int PER = RG_R128R_BINS / 256;
    const int tid = threadIdx.x;
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) t += hist[tid * PER + k];
    __syncthreads();  // the last call's readers of pick are through
    scan[tid] = t;
    if (tid == 0) pick[0] = pick[1] = 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t v = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const uint32_t incl = scan[tid], excl = incl - t;
    if (rank >= excl && rank < incl) {  // one thread at most
        uint32_t r = rank - excl;
        for (int k = 0; k < PER; ++k) {
            const uint32_t cnt = hist[tid * PER + k];
            if (r < cnt) {
                pick[0] = (uint32_t)(tid * PER + k);
                pick[1] = r;
                break;
            }
            r -= cnt;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void r128r_ranks(const uint32_t n, uint32_t *rank) {
    rank[0] = (uint32_t)((10ull * (n - 1u) + 50ull) / 100ull);
    rank[1] = (uint32_t)((95ull * (n - 1u) + 50ull) / 100ull);
}

// the state of a selection before its first counting pass
__device__ __forceinline__ void r128r_start(RgR128RangeSel &s, const double thr, const uint32_t n) {
    s.thr = thr;
    s.prefix[0] = s.prefix[1] = s.mask = 0;
    s.rank[0] = s.rank[1] = 0;
    s.n = n;
    s.pad = 0;
    if (n) r128r_ranks(n, s.rank);
}

// One value for a histogram.  The values of a wave are neighbours in time and often share a digit (the upper passes see one
// or two exponents): the first two distinct digits of a wave are added once per wave, what is left lane by lane.  The wave
// is converged here (the callers' loops are uniform).
__device__ __forceinline__ void r128r_count(uint32_t *hist, const uint32_t digit, bool pred) {
    unsigned long long todo = __ballot(pred);
    for (int it = 0; it < 2 && todo; ++it) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t d = __shfl(digit, leader, 64);
        const bool mine = pred && digit == d;
        const unsigned long long m = __ballot(mine);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[d], (uint32_t)__popcll(m));
        pred = pred && !mine;
        todo &= ~m;
    }
    if (pred) atomicAdd(&hist[digit], 1u);
}

// Counting pass `pass` over v[i0, i1): the digit of every value both gates keep and whose upper bits are a percentile's
// prefix so far, into that percentile's histogram (hist, hist + BINS).  While both percentiles share their prefix the two
// histograms would be equal: only the first is counted then, and r128r_advance reads it for both.
__device__ __forceinline__ void r128r_count_slice(uint32_t *hist, const double *__restrict__ v, const uint64_t i0, const uint64_t i1,
                                                  const double abs_gate, const RgR128RangeSel &s, const int pass) {
    const int shift = r128r_shift(pass), width = r128r_width(pass);
    const bool same = s.prefix[0] == s.prefix[1];
    for (uint64_t base = i0; base < i1; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const double x = i < i1 ? v[i] : 0.0;
        const bool kept = i < i1 && x >= abs_gate && x >= s.thr;
        const uint64_t bits = (uint64_t)__double_as_longlong(x);
        const uint32_t digit = (uint32_t)(bits >> shift) & ((1u << width) - 1u);
        r128r_count(hist, digit, kept && (bits & s.mask) == s.prefix[0]);
        if (!same) r128r_count(hist + RG_R128R_BINS, digit, kept && (bits & s.mask) == s.prefix[1]);
    }
}

// after counting pass `pass`: the digit of both percentiles, their ranks within it
__device__ __forceinline__ void r128r_advance(RgR128RangeSel &s, const uint32_t *hist, uint32_t *scan, uint32_t *pick, const int pass) {
    const int shift = r128r_shift(pass), width = r128r_width(pass);
    const bool same = s.prefix[0] == s.prefix[1];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        r128r_find_bin(hist + (q && !same ? RG_R128R_BINS : 0), scan, pick, s.rank[q]);
        s.prefix[q] |= (uint64_t)pick[0] << shift;
        s.rank[q] = pick[1];
    }
    s.mask |= (uint64_t)((1u << width) - 1u) << shift;
}

__device__ __forceinline__ double r128r_lufs(const double ms) { return ms > 0.0 ? -0.691 + 10.0 * log10(ms) : -__builtin_inf(); }

__device__ __forceinline__ void r128r_finish(rg_r128_dynamics &d, const uint32_t total, const uint32_t n, const uint64_t low_bits,
                                             const uint64_t high_bits, const unsigned long long m_bits, const unsigned long long s_bits) {
    const double low = __longlong_as_double((long long)low_bits), high = __longlong_as_double((long long)high_bits);
    d.loudness_range_lu = n ? 10.0 * log10(high / low) : 0.0;
    d.range_low_lufs = n ? r128r_lufs(low) : -__builtin_inf();
    d.range_high_lufs = n ? r128r_lufs(high) : -__builtin_inf();
    d.max_momentary_lufs = r128r_lufs(__longlong_as_double((long long)m_bits));
    d.max_short_term_lufs = r128r_lufs(__longlong_as_double((long long)s_bits));
    d.st_blocks = total;
    d.st_blocks_gated = n;
}

// max over the tracks' maxima, by the whole workgroup; the result is in sh_max[0] (momentary) and sh_max[1] (short-term)
__device__ __forceinline__ void r128r_album_maxima(const unsigned long long *__restrict__ max_bits, const uint32_t n_tracks,
                                                   unsigned long long *sh_max /* 512 */) {
    const int tid = threadIdx.x;
    unsigned long long m = 0, s = 0;
    for (uint32_t i = tid; i < n_tracks; i += 256) {
        m = r128r_umax(m, max_bits[2 * i]);
        s = r128r_umax(s, max_bits[2 * i + 1]);
    }
    __syncthreads();
    sh_max[2 * tid] = m;
    sh_max[2 * tid + 1] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            sh_max[2 * tid] = r128r_umax(sh_max[2 * tid], sh_max[2 * (tid + k)]);
            sh_max[2 * tid + 1] = r128r_umax(sh_max[2 * tid + 1], sh_max[2 * (tid + k) + 1]);
        }
        __syncthreads();
    }
}

}  // namespace
