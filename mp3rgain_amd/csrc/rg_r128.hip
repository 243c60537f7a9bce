// rg_r128.hip -- EBU R 128 / ReplayGain 2.0 analysis on gfx950: K-weighted hop energies and sample peak (main kernel),
// gating and the logarithm (gate kernel), true peak (polyphase interpolator), and the host driver behind
// include/mp3rgain_amd_r128.h.  DESIGN.md section 14 has the reasoning and the numbers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rg_ctx.h"
#include "rg_r128.h"
#include "rg_r128_inl.h"

namespace {

typedef uint32_t __attribute__((ext_vector_type(4))) r128_u32x4;
typedef uint32_t __attribute__((ext_vector_type(4), aligned(4))) r128_u32x4u;  // 16-byte load, 4-byte aligned
typedef short __attribute__((ext_vector_type(4), aligned(2))) r128_s16x4u;     // 8-byte load, 2-byte aligned

// ---- per-format sample access.  A staged sample is a 32-bit LDS word (float bits, or the sign-extended integer); the
// ---- power-of-two full-scale factor is folded into the stage-1 numerator, so value() is the raw number.
template <int FMT> struct R128Fmt;
template <> struct R128Fmt<RG_FMT_F32_PLANAR> {
    typedef float elem;
    typedef float peak_t;
    static __device__ __forceinline__ uint32_t word(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ double value(uint32_t w) { return (double)__uint_as_float(w); }
    // max over FINITE values: v * 0 is NaN for an infinite v and fmaxf drops NaNs, so Inf and NaN both leave pk alone
    static __device__ __forceinline__ void peak(uint32_t w, float &pk) {
        const float v = __uint_as_float(w);
        pk = fmaxf(pk, fmaf(v, 0.0f, fabsf(v)));
    }
    static __device__ __forceinline__ uint32_t peak_bits(float pk) { return __float_as_uint(pk); }
    static __device__ __forceinline__ double peak_value(uint32_t bits) { return (double)__uint_as_float(bits); }
    static __device__ __forceinline__ float sample(float v) { return v; }
};
template <> struct R128Fmt<RG_FMT_S16_PLANAR> {
    typedef int16_t elem;
    typedef uint32_t peak_t;
    static __device__ __forceinline__ uint32_t word(int16_t v) { return (uint32_t)(int32_t)v; }
    static __device__ __forceinline__ double value(uint32_t w) { return (double)(int32_t)w; }
    static __device__ __forceinline__ void peak(uint32_t w, uint32_t &pk) {
        const int32_t v = (int32_t)w;
        const uint32_t m = (uint32_t)(v < 0 ? -v : v);
        pk = m > pk ? m : pk;
    }
    static __device__ __forceinline__ uint32_t peak_bits(uint32_t pk) { return pk; }
    static __device__ __forceinline__ double peak_value(uint32_t bits) { return (double)bits / 32768.0; }
    static __device__ __forceinline__ float sample(int16_t v) { return (float)v * (1.0f / 32768.0f); }
};
template <> struct R128Fmt<RG_FMT_S32_PLANAR> {
    typedef int32_t elem;
    typedef uint32_t peak_t;
    static __device__ __forceinline__ uint32_t word(int32_t v) { return (uint32_t)v; }
    static __device__ __forceinline__ double value(uint32_t w) { return (double)(int32_t)w; }
    static __device__ __forceinline__ void peak(uint32_t w, uint32_t &pk) {
        const int32_t v = (int32_t)w;
        const uint32_t m = v < 0 ? (uint32_t)0 - (uint32_t)v : (uint32_t)v;
        pk = m > pk ? m : pk;
    }
    static __device__ __forceinline__ uint32_t peak_bits(uint32_t pk) { return pk; }
    static __device__ __forceinline__ double peak_value(uint32_t bits) { return (double)bits / 2147483648.0; }
    static __device__ __forceinline__ float sample(int32_t v) { return (float)v * (1.0f / 2147483648.0f); }
};

__device__ __forceinline__ uint32_t r128_find_track(const RgR128TrackDev *__restrict__ tracks, uint32_t n, uint64_t key,
                                                    uint64_t RgR128TrackDev::*base) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (tracks[mid].*base <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace

// =================================================================================================
// Main kernel: PCM -> hop energies e[channel][hop] (f64) and the sample peak, one pass over the arena.
//
// One lane = one channel x a run of S consecutive hops, started RG_R128_WARM_HOPS hops early from the zero state (nothing
// is accumulated there).  The cascade's memory decays by a factor of ten every tenth of a hop at every rate, so what a lane
// has not seen is below 1e-30 of what came before its start: under f64 rounding for any input.  Every hop of every channel
// has exactly one owner lane, which writes its energy with a plain store: nothing depends on scheduling.
//
// Loader: a wave owns 64 rows (the lanes' runs), strided far apart in the arena.  Per tile of RG_R128_TILE = 32 frames every
// lane issues 8 loads of 4 frames: instruction q, lane j fetches one piece of row 8q + (j >> 3), so an instruction reads 8
// contiguous 128-byte runs (64-byte runs for 16-bit samples) instead of 64 scattered pieces.  The pieces go through registers
// into the wave's private 8 KiB tile, one tile ahead of their use (the loads of tile t + 1 are in flight while tile t is
// consumed); the piece a lane fetches is XOR-swizzled with (row >> 1) & 7 so that the consumer's row-per-lane 16-byte LDS
// reads of 16 neighbouring rows (128 bytes apart) fall on 16 distinct slots of the 256-byte bank row.  The tile is
// wave-private: no block barrier.  The lanes of a wave need not share a track, a rate or a channel: every constant is per lane.
#define RG_R128_TILE 32
#define RG_R128_BLOCK 256
#define RG_R128_WAVE_TILE_BYTES (64 * RG_R128_TILE * 4)

template <int FMT>
__global__ void __launch_bounds__(RG_R128_BLOCK)
rg_r128_main_kernel(const RgR128TrackDev *__restrict__ tracks, const uint32_t n_tracks, const uint64_t n_lanes,
                    uint32_t *__restrict__ peak_bits, uint32_t *__restrict__ flags) {
    typedef R128Fmt<FMT> F;
    typedef const __attribute__((address_space(1))) typename F::elem gelem;
    __shared__ __attribute__((aligned(16))) char tiles[RG_R128_BLOCK / 64][RG_R128_WAVE_TILE_BYTES];
    const int lane = threadIdx.x & 63;
    char *const wtile = tiles[threadIdx.x >> 6];
    const uint64_t g = (uint64_t)blockIdx.x * RG_R128_BLOCK + threadIdx.x;
    if (g - (uint64_t)lane >= n_lanes) return;  // the whole wave is past the end
    const bool live = g < n_lanes;
    const uint32_t ti = r128_find_track(tracks, n_tracks, live ? g : n_lanes - 1, &RgR128TrackDev::lane_base);
    const RgR128TrackDev &T = tracks[ti];
    const uint32_t hop = T.hop, H = T.H, runs = T.runs, S = T.S;
    const uint32_t local = live ? (uint32_t)(g - T.lane_base) : 0u;
    const uint32_t c = local / runs, r = local - c * runs;
    const uint32_t first_hop = r * S;
    const uint32_t warm = first_hop < RG_R128_WARM_HOPS ? first_hop : RG_R128_WARM_HOPS;
    const uint64_t start = (uint64_t)(first_hop - warm) * hop;
    const int own = H > first_hop ? (int)(H - first_hop < S ? H - first_hop : S) : 0;
    // the track's last run reads on to the end of the channel: the partial last hop counts for the peak (and for the
    // non-finite flag), not for any energy
    uint32_t len = r + 1 == runs ? (uint32_t)(T.frames - start) : (warm + (uint32_t)own) * hop;
    if (!live) len = 0;
    gelem *const rowp = (gelem *)(uintptr_t)(T.ch[c] + start * sizeof(typename F::elem));
    double *const eout = T.e + (size_t)c * H + first_hop;
    const double b0 = T.b[0], b1 = T.b[1], b2 = T.b[2];
    const double na11 = -T.a1[0], na12 = -T.a1[1], na21 = -T.a2[0], na22 = -T.a2[1];

    // loader role: instruction q covers rows 8q .. 8q+7; this lane fetches for row 8q + (lane >> 3) the piece that belongs
    // in LDS slot (lane & 7) of that row
    gelem *lfirst[8];
    uint32_t llen[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int row = 8 * q + (lane >> 3);
        const int piece = (lane & 7) ^ ((row >> 1) & 7);
        const unsigned long long base = __shfl((unsigned long long)(uintptr_t)rowp, row, 64);
        lfirst[q] = (gelem *)(uintptr_t)base + 4 * piece;
        llen[q] = __shfl(len, row, 64);
    }
    uint32_t maxlen = len;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(maxlen, d, 64);
        maxlen = o > maxlen ? o : maxlen;
    }
    const uint32_t ntiles = (maxlen + RG_R128_TILE - 1) / RG_R128_TILE;

    r128_u32x4 stage[8];
    auto load_tile = [&](const uint32_t tile) {
        const uint32_t n0 = tile * RG_R128_TILE;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = 8 * q + (lane >> 3);
            const int piece = (lane & 7) ^ ((row >> 1) & 7);
            const uint32_t pn = n0 + 4u * piece;  // frame index of the piece within its row
            gelem *src = lfirst[q] + n0;
            if (pn + 4u <= llen[q]) {
                if constexpr (FMT == RG_FMT_S16_PLANAR) {
                    const r128_s16x4u v = *(const __attribute__((address_space(1))) r128_s16x4u *)src;
                    stage[q] = r128_u32x4{(uint32_t)(int32_t)v.x, (uint32_t)(int32_t)v.y, (uint32_t)(int32_t)v.z, (uint32_t)(int32_t)v.w};
                } else {
                    stage[q] = *(const __attribute__((address_space(1))) r128_u32x4u *)src;
                }
            } else {  // the end of a row: element by element, nothing is read past it
                stage[q].x = pn + 0u < llen[q] ? F::word(src[0]) : 0u;
                stage[q].y = pn + 1u < llen[q] ? F::word(src[1]) : 0u;
                stage[q].z = pn + 2u < llen[q] ? F::word(src[2]) : 0u;
                stage[q].w = pn + 3u < llen[q] ? F::word(src[3]) : 0u;
            }
        }
    };
    auto store_tile = [&] {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 8; ++q)
            *reinterpret_cast<uint4 *>(wtile + q * 1024 + lane * 16) = make_uint4(stage[q].x, stage[q].y, stage[q].z, stage[q].w);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    // consumer role: row == lane
    const char *const rrow = wtile + lane * (RG_R128_TILE * 4);
    const int rswz = (lane >> 1) & 7;
    auto read_piece = [&](const int p) -> uint4 { return *reinterpret_cast<const uint4 *>(rrow + 16 * (p ^ rswz)); };

    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, acc = 0.0;
    typename F::peak_t pk = 0;
    uint32_t cnt = 0;
    int hidx = -(int)warm;
    // both biquads in transposed direct form II, as the checker's lfilter runs them: 10 FP64 operations per sample
    auto step = [&](const uint32_t w) {
        const double x = F::value(w);
        const double y = fma(b0, x, s1);
        s1 = fma(na11, y, fma(b1, x, s2));
        s2 = fma(na12, y, b2 * x);
        const double z = y + t1;
        t1 = fma(na21, z, fma(-2.0, y, t2));
        t2 = fma(na22, z, y);
        acc = fma(z, z, acc);
    };
    auto flush = [&] {
        if (hidx >= 0 && hidx < own) eout[hidx] = acc;
        acc = 0.0;
        cnt = 0;
        ++hidx;
    };

    if (ntiles) load_tile(0);
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        store_tile();
        if (tile + 1 < ntiles) load_tile(tile + 1);
        const uint32_t n0 = tile * RG_R128_TILE;
        if (n0 < len) {
            uint4 cur = read_piece(0);
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const uint4 nxt = read_piece((p + 1) & 7);
                const uint32_t f[4] = {cur.x, cur.y, cur.z, cur.w};
                const uint32_t n = n0 + 4u * p;
                if (n + 4u <= len && cnt + 4u <= hop) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) F::peak(f[u], pk);
#pragma unroll
                    for (int u = 0; u < 4; ++u) step(f[u]);
                    cnt += 4u;
                    if (cnt == hop) flush();
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (n + u < len) {
                            F::peak(f[u], pk);
                            step(f[u]);
                            if (++cnt == hop) flush();
                        }
                }
                cur = nxt;
            }
        }
    }
    if (live) {
        const uint32_t bits = F::peak_bits(pk);
        if (bits) atomicMax(&peak_bits[T.index], bits);
        // a sample that is not finite never leaves the recursion's state again
        if (!(fabs(s1) + fabs(s2) + fabs(t1) + fabs(t2) < __builtin_inf())) atomicOr(&flags[T.index], RG_TRACK_FLAG_NONFINITE);
    }
}

// =================================================================================================
// True peak: the 49-tap interpolator on the zero-stuffed signal, as F phases of 13 / 12 (F = 4) or 25 / 24 (F = 2) taps, in
// f32.  A block walks RG_R128_TP_CHUNK consecutive tiles of RG_R128_TP_TILE frames of one channel: a tile plus 48 / F frames
// of history is staged in LDS (zeros before the track's start and after its end, which also produces the tail after the last
// sample), the next tile's samples are already on their way in registers while this one is computed (two LDS buffers, one
// barrier per tile); a thread computes every phase of four consecutive frames from a register window.  Per-track max through
// an integer atomic max on the bits of the non-negative float.  Values that are not finite do not count.
#define RG_R128_TP_TILE 1024
#define RG_R128_TP_CHUNK 16
struct RgR128Taps { float h[RG_R128_TP_TAPS]; };

template <int FMT, int FACTOR>
__global__ void __launch_bounds__(256)
rg_r128_truepeak_kernel(const RgR128TrackDev *__restrict__ tracks, const uint32_t n_tracks, const RgR128Taps taps,
                        uint32_t *__restrict__ tp_bits) {
    typedef R128Fmt<FMT> F;
    constexpr int HIST = 48 / FACTOR;
    constexpr int NLD = (RG_R128_TP_TILE + HIST + 255) / 256;
    __shared__ __attribute__((aligned(16))) float xs[2][RG_R128_TP_TILE + HIST];
    const uint32_t ti = r128_find_track(tracks, n_tracks, blockIdx.x, &RgR128TrackDev::tile_base);
    const RgR128TrackDev &T = tracks[ti];
    const uint32_t c = blockIdx.y;
    if (c >= T.nch) return;
    const uint64_t N = T.frames;
    const uint64_t chunk0 = (uint64_t)(blockIdx.x - T.tile_base) * (RG_R128_TP_CHUNK * RG_R128_TP_TILE);  // first output frame
    const uint64_t left = N + HIST - chunk0;  // output frames from here to the end of the tail
    const uint32_t ntiles = left >= (uint64_t)RG_R128_TP_CHUNK * RG_R128_TP_TILE ? RG_R128_TP_CHUNK
                                                                                 : (uint32_t)((left + RG_R128_TP_TILE - 1) / RG_R128_TP_TILE);
    const typename F::elem *const x = reinterpret_cast<const typename F::elem *>(T.ch[c]);
    float r[NLD];
    auto fetch = [&](const uint32_t tile) {
        const uint64_t base = chunk0 + (uint64_t)tile * RG_R128_TP_TILE;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const uint32_t i = threadIdx.x + 256u * k;
            const uint64_t gi = base + i;  // frame gi - HIST
            r[k] = (i < RG_R128_TP_TILE + HIST && gi >= (uint64_t)HIST && gi - HIST < N) ? F::sample(x[gi - HIST]) : 0.0f;
        }
    };
    fetch(0);
    float m = 0.0f;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
        float *const buf = xs[tile & 1];
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const uint32_t i = threadIdx.x + 256u * k;
            if (i < RG_R128_TP_TILE + HIST) buf[i] = r[k];
        }
        __syncthreads();
        if (tile + 1 < ntiles) fetch(tile + 1);
        // w[k] = x[first frame of the tile + 4 tid - HIST + k]; output frame n = ... + 4 tid + u, phase p: sum_i h[p + F i] x[n - i]
        float w[HIST + 4];
#pragma unroll
        for (int k = 0; k < HIST + 4; k += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(&buf[4 * threadIdx.x + k]);
            w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int p = 0; p < FACTOR; ++p) {
                float y = 0.0f;
#pragma unroll
                for (int i = 0; p + FACTOR * i < RG_R128_TP_TAPS; ++i) y = fmaf(taps.h[p + FACTOR * i], w[u + HIST - i], y);
                m = fmaxf(m, fmaf(y, 0.0f, fabsf(y)));
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(&tp_bits[T.index], __float_as_uint(m));
}

// =================================================================================================
// Gate kernel: one workgroup per track.  Block values from hop energies in a fixed order, both gates, the logarithm.  Every
// thread sums its blocks in ascending order and the workgroup folds the 256 partial sums in a fixed tree: the same input
// gives the same bits on every run.  (An album's union of blocks is rg_r128a_gate_kernel's, rg_r128_albums.hip.)
__global__ void __launch_bounds__(256)
rg_r128_gate_kernel(const RgR128TrackDev *__restrict__ tracks, const double abs_gate, const uint32_t *__restrict__ peak_bits,
                    const uint32_t *__restrict__ tp_bits /* nullptr: true peak not asked for */, const uint32_t *__restrict__ flags,
                    rg_r128_track_result *__restrict__ out, double *__restrict__ block_z /* nullptr, or every track's blocks */) {
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256];
    const RgR128TrackDev &T = tracks[blockIdx.x];
    const uint32_t nb = T.H > 3u ? T.H - 3u : 0u;
    double thr = abs_gate;
    double sum = 0.0;
    uint32_t cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        sum = 0.0;
        cnt = 0;
        for (uint32_t b = threadIdx.x; b < nb; b += 256) {
            const double z = r128_block_z(T, b);
            if (pass == 0 && block_z) block_z[T.z_base + b] = z;
            if (z >= abs_gate && z >= thr) {
                sum += z;
                ++cnt;
            }
        }
        r128_fold(sh_sum, sh_cnt, sum, cnt);
        if (pass == 0) thr = cnt ? 0.1 * (sum / (double)cnt) : abs_gate;
    }
    if (threadIdx.x) return;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    double lufs = -inf, gain = 0.0;
    if (cnt) {
        lufs = -0.691 + 10.0 * log10(sum / (double)cnt);
        gain = RG_R128_REFERENCE_LUFS - lufs;
    }
    rg_r128_track_result r;
    const uint32_t fl = flags[T.index];
    r.loudness_lufs = fl ? nan : lufs;
    r.gain_db = fl ? nan : gain;
    const uint32_t pb = peak_bits[T.index];
    r.sample_peak = T.format == RG_FMT_F32_PLANAR   ? R128Fmt<RG_FMT_F32_PLANAR>::peak_value(pb)
                    : T.format == RG_FMT_S16_PLANAR ? R128Fmt<RG_FMT_S16_PLANAR>::peak_value(pb)
                                                    : R128Fmt<RG_FMT_S32_PLANAR>::peak_value(pb);
    r.true_peak = !tp_bits ? nan : T.tp_factor == 1 ? r.sample_peak : (double)__uint_as_float(tp_bits[T.index]);
    r.sample_rate = T.sample_rate;
    r.blocks = nb;
    r.blocks_gated = cnt;
    r.flags = fl;
    out[T.index] = r;
}

// =================================================================================================
// host driver
namespace {

struct R128State {
    uint32_t tune_S = 0;
    int tune_album_select = 0;
    int channel_mode = RG_R128_CHANNELS_PAIR;
    void *range = nullptr;  // rg_r128_range.hip's buffers
    void *albums = nullptr;  // rg_r128_albums.hip's
    DevBuf<unsigned char> d_desc;
    DevBuf<uint32_t> d_words;  // [sample peak | true peak | flags] x n
    DevBuf<rg_r128_track_result> d_res;
    DevBuf<double> d_e, d_z;
    DevBuf<double> d_ce;  // weighted tracks: the per-channel hop energies in front of the fold
    // an album in progress: every group's tracks in input order, their hop energies still on the device
    std::vector<double *> kept_e;
    std::vector<RgR128TrackDev> kept;
    std::vector<rg_r128_track_result> kept_res;
    void drop_album() {
        for (double *p : kept_e) (void)hipFree(p);
        kept_e.clear();
        kept.clear();
        kept_res.clear();
    }
};

R128State &state(rg_ctx *c) {
    if (!c->r128) {
        c->r128 = new R128State();
        c->r128_free = [](void *p) {
            R128State *s = static_cast<R128State *>(p);
            s->drop_album();
            rg_r128_range_free(s->range);
            rg_r128_albums_free(s->albums);
            s->d_desc.release();
            s->d_words.release();
            s->d_res.release();
            s->d_e.release();
            s->d_z.release();
            s->d_ce.release();
            delete s;
        };
    }
    return *static_cast<R128State *>(c->r128);
}

int r128_validate(rg_ctx *c, const rg_track_desc *tracks, size_t n, size_t pcm_bytes) {
    if (n > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many tracks");
    for (size_t t = 0; t < n; ++t) {
        const rg_track_desc &d = tracks[t];
        if (!rg_r128_supported_rate(d.sample_rate))
            return rg_set_err(c, RG_ERR_UNSUPPORTED_RATE, "Unsupported sample rate: %u Hz. Supported rates: %u to %u", d.sample_rate,
                              RG_R128_MIN_RATE, RG_R128_MAX_RATE);
        if (d.channels == 0) return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: channels == 0", t);
        if (d.format > RG_FMT_S32_PLANAR) return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: unknown format %u", t, d.format);
        const size_t bps = rg_bytes_per_sample(d.format);
        if (d.offset_bytes % bps) return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: offset not sample-aligned", t);
        if (d.frames / ((d.sample_rate + 5u) / 10u) > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: too long", t);
        const uint64_t need = d.offset_bytes + (uint64_t)d.channels * d.frames * bps;
        if (need > pcm_bytes)
            return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: extends past the PCM arena (%llu > %zu)", t, (unsigned long long)need,
                              pcm_bytes);
    }
    return RG_OK;
}

template <int FMT>
void launch_main(const RgR128TrackDev *d_list, uint32_t n, uint64_t lanes, uint32_t *peak, uint32_t *flags, hipStream_t s) {
    const uint64_t blocks = (lanes + RG_R128_BLOCK - 1) / RG_R128_BLOCK;
    hipLaunchKernelGGL(rg_r128_main_kernel<FMT>, dim3((uint32_t)blocks), dim3(RG_R128_BLOCK), 0, s, d_list, n, lanes, peak, flags);
}

template <int FMT>
void launch_tp(uint32_t factor, const RgR128TrackDev *d_list, uint32_t n, uint64_t tiles, uint32_t ny, uint32_t *tp, hipStream_t s) {
    RgR128Taps taps;
    rg_r128_tp_table(factor, taps.h);
    if (factor == 4)
        hipLaunchKernelGGL((rg_r128_truepeak_kernel<FMT, 4>), dim3((uint32_t)tiles, ny), dim3(256), 0, s, d_list, n, taps, tp);
    else
        hipLaunchKernelGGL((rg_r128_truepeak_kernel<FMT, 2>), dim3((uint32_t)tiles, ny), dim3(256), 0, s, d_list, n, taps, tp);
}

// hops per lane: enough lanes for about three waves on every SIMD of the chip, few enough that the three warm-up hops of a
// lane stay a small share of what it reads
uint32_t choose_S(const R128State &st, uint64_t channel_hops) {
    if (st.tune_S) return st.tune_S;
    const uint64_t target_lanes = 256ull * 4 * 3 * 64;
    const uint64_t s = (channel_hops + target_lanes - 1) / target_lanes;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(s, 4), 64);
}

}  // namespace

double rg_r128_abs_gate() { return pow(10.0, (-70.0 + 0.691) / 10.0); }

extern "C" int rg_r128_set_tuning(rg_ctx *c, int key, int64_t value) {
    if (!c) return RG_ERR_INVALID_ARG;
    if (key == 2) {
        if (value < 0 || value > 2) return rg_set_err(c, RG_ERR_INVALID_ARG, "album selection must be 0..2");
        state(c).tune_album_select = (int)value;
        return RG_OK;
    }
    if (key != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "unknown R 128 tuning key %d", key);
    if (value < 0 || value > RG_R128_MAX_S) return rg_set_err(c, RG_ERR_INVALID_ARG, "hops per lane must be 0..%d", RG_R128_MAX_S);
    state(c).tune_S = (uint32_t)value;
    return RG_OK;
}

extern "C" int rg_r128_set_channel_mode(rg_ctx *c, int mode) {
    if (!c) return RG_ERR_INVALID_ARG;
    if (mode != RG_R128_CHANNELS_PAIR && mode != RG_R128_CHANNELS_LAYOUT)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "unknown R 128 channel mode %d", mode);
    state(c).channel_mode = mode;
    return RG_OK;
}

int rg_r128_channel_mode(rg_ctx *c) { return state(c).channel_mode; }

int rg_r128_check_weights(rg_ctx *c, size_t t, uint32_t channels, const rg_r128_channel_weights *w) {
    if (channels < 1 || channels > 8)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: Unsupported channel count for layout analysis: %u (1 to 8)", t, channels);
    for (uint32_t k = 0; w && k < channels; ++k)
        if (!(w->w[k] >= 0.0) || !(w->w[k] < INFINITY))
            return rg_set_err(c, RG_ERR_INVALID_ARG, "track %zu: channel weight %u is not a finite number >= 0", t, k);
    return RG_OK;
}

void rg_r128_album_reset(rg_ctx *c) { state(c).drop_album(); }

int rg_r128_album_select(rg_ctx *c) { return state(c).tune_album_select; }
void **rg_r128_range_slot(rg_ctx *c) { return &state(c).range; }
void **rg_r128_albums_slot(rg_ctx *c) { return &state(c).albums; }

int rg_r128_run(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *d_base, size_t pcm_bytes, int want_tp, int keep,
                rg_r128_track_result *out, double *block_z_out, rg_r128_dynamics *dyn_out, double *st_z_out, RgR128TrackDev *tr_out,
                double **e_out, const rg_r128_channel_weights *weights) {
    if (e_out) *e_out = nullptr;
    if (!c) return RG_ERR_INVALID_ARG;
    if (n && (!tracks || !out || !d_base)) return rg_set_err(c, RG_ERR_INVALID_ARG, "null argument");
    int rc = r128_validate(c, tracks, n, pcm_bytes);
    if (rc != RG_OK) return rc;
    // the weights of every track: the caller's, or the layout rule's in LAYOUT mode; neither: the pair of channels 0 and 1
    std::vector<rg_r128_channel_weights> layout_w;
    if (!weights && n && state(c).channel_mode == RG_R128_CHANNELS_LAYOUT) {
        layout_w.resize(n);
        for (size_t i = 0; i < n; ++i) {
            rc = rg_r128_check_weights(c, i, tracks[i].channels, nullptr);
            if (rc != RG_OK) return rc;
            (void)rg_r128_layout_weights(tracks[i].channels, 0, &layout_w[i]);
        }
        weights = layout_w.data();
    }
    for (size_t i = 0; weights && i < n; ++i) {
        rc = rg_r128_check_weights(c, i, tracks[i].channels, &weights[i]);
        if (rc != RG_OK) return rc;
    }
    if (n == 0) return RG_OK;
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    // the arena may be the context's own, still read by an earlier batch of the other path; this path is synchronous
    for (int k = 0; k < RG_SLOT_STREAMS; ++k) RG_HIP(c, hipStreamSynchronize(c->slots[k].stream));
    hipStream_t s = c->slot().stream;
    R128State &st = state(c);

    std::vector<RgR128TrackDev> tr(n);
    uint64_t total_e = 0, total_z = 0, channel_hops = 0, total_ce = 0;
    // a weighted track: every channel goes through the main kernel into d_ce (main_nch rows from ce_off on) and is folded
    // into the track's one row of d_e; 0: a plain track
    std::vector<uint32_t> main_nch(n, 0);
    std::vector<uint64_t> ce_off(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const rg_track_desc &d = tracks[i];
        RgR128Design ds;
        rg_r128_design(d.sample_rate, &ds);
        RgR128TrackDev &o = tr[i];
        memset(&o, 0, sizeof o);
        const size_t bps = rg_bytes_per_sample(d.format);
        o.nch = d.channels >= 2 ? 2 : 1;
        if (weights) {
            bool plain = d.channels <= 2;
            for (uint32_t k = 0; plain && k < d.channels; ++k) plain = weights[i].w[k] == 1.0;
            if (!plain) main_nch[i] = d.channels;
        }
        const uint32_t planes = main_nch[i] ? main_nch[i] : o.nch;
        for (uint32_t k = 0; k < planes; ++k) o.ch[k] = (const unsigned char *)d_base + d.offset_bytes + (uint64_t)k * d.frames * bps;
        if (main_nch[i]) o.nch = 1;
        o.frames = d.frames;
        o.hop = ds.hop;
        o.H = (uint32_t)(d.frames / ds.hop);
        o.index = (uint32_t)i;
        o.tp_factor = ds.tp_factor;
        o.sample_rate = d.sample_rate;
        o.format = d.format;
        const double scale = d.format == RG_FMT_F32_PLANAR ? 1.0 : d.format == RG_FMT_S16_PLANAR ? 1.0 / 32768.0 : 1.0 / 2147483648.0;
        for (int k = 0; k < 3; ++k) o.b[k] = ds.b1[k] * scale;
        o.a1[0] = ds.a1[1]; o.a1[1] = ds.a1[2];
        o.a2[0] = ds.a2[1]; o.a2[1] = ds.a2[2];
        o.z_base = total_z;
        total_z += o.H > 3 ? o.H - 3 : 0;
        o.e = (double *)(uintptr_t)(total_e * sizeof(double));  // offset for now
        total_e += (uint64_t)o.nch * o.H;
        channel_hops += (uint64_t)planes * o.H;
        if (main_nch[i]) {
            ce_off[i] = total_ce;
            total_ce += (uint64_t)planes * o.H;
        }
    }
    const uint32_t S = choose_S(st, channel_hops);
    double *d_e = nullptr;
    if (keep) {
        RG_HIP(c, hipMalloc((void **)&d_e, (total_e ? total_e : 1) * sizeof(double)));
        st.kept_e.push_back(d_e);
    } else if (e_out) {  // (an error below leaves it to the caller, which frees what it was given)
        RG_HIP(c, hipMalloc((void **)&d_e, (total_e ? total_e : 1) * sizeof(double)));
        *e_out = d_e;
    } else {
        RG_HIP(c, st.d_e.reserve(total_e ? total_e : 1));
        d_e = st.d_e.p;
    }
    if (total_ce) RG_HIP(c, st.d_ce.reserve(total_ce));
    for (size_t i = 0; i < n; ++i) {
        RgR128TrackDev &o = tr[i];
        o.e = d_e + (uintptr_t)o.e / sizeof(double);
        o.S = S;
        o.runs = o.frames ? std::max<uint32_t>(1u, (o.H + S - 1) / S) : 0u;
    }
    // launch lists: the loudness kernel per sample format, the true-peak kernel per (format, factor)
    std::vector<RgR128TrackDev> blob(tr);
    struct List { size_t first = 0, count = 0; uint64_t units = 0; uint32_t ny = 2; };
    List main_l[3], tp_l[3][2];
    for (int f = 0; f < 3; ++f) {
        main_l[f].first = blob.size();
        for (size_t i = 0; i < n; ++i)
            if ((int)tr[i].format == f && tr[i].runs) {
                RgR128TrackDev o = tr[i];
                if (main_nch[i]) {
                    o.nch = main_nch[i];
                    o.e = st.d_ce.p + ce_off[i];
                }
                o.lane_base = main_l[f].units;
                main_l[f].units += (uint64_t)o.nch * o.runs;
                blob.push_back(o);
                ++main_l[f].count;
            }
    }
    if (want_tp)
        for (int f = 0; f < 3; ++f)
            for (int k = 0; k < 2; ++k) {
                const uint32_t factor = k ? 2 : 4;
                tp_l[f][k].first = blob.size();
                for (size_t i = 0; i < n; ++i)
                    if ((int)tr[i].format == f && tr[i].tp_factor == factor && tr[i].frames) {
                        RgR128TrackDev o = tr[i];
                        if (main_nch[i]) o.nch = main_nch[i];  // peaks are over every channel, whatever its weight
                        tp_l[f][k].ny = std::max(tp_l[f][k].ny, o.nch);
                        o.tile_base = tp_l[f][k].units;
                        const uint64_t chunk = (uint64_t)RG_R128_TP_CHUNK * RG_R128_TP_TILE;
                        tp_l[f][k].units += (o.frames + 48 / factor + chunk - 1) / chunk;
                        blob.push_back(o);
                        ++tp_l[f][k].count;
                    }
                if (tp_l[f][k].units > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "batch too long for one true-peak launch");
            }
    for (int f = 0; f < 3; ++f)
        if (main_l[f].units > 0x7FFFFFFFull * RG_R128_BLOCK) return rg_set_err(c, RG_ERR_INVALID_ARG, "batch too long for one launch");

    std::vector<RgR128FoldItem> fold;
    uint64_t fold_blocks = 0;
    for (size_t i = 0; i < n; ++i)
        if (main_nch[i] && tr[i].H) {
            RgR128FoldItem it;
            memset(&it, 0, sizeof it);
            it.src = st.d_ce.p + ce_off[i];
            it.dst = tr[i].e;
            it.block_base = fold_blocks;
            it.H = tr[i].H;
            it.nch = main_nch[i];
            for (uint32_t k = 0; k < it.nch; ++k) it.w[k] = weights[i].w[k];
            fold_blocks += (it.H + RG_R128_FOLD_BLOCK - 1) / RG_R128_FOLD_BLOCK;
            fold.push_back(it);
        }
    if (fold_blocks > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "batch too long for one launch");
    const size_t desc_bytes = blob.size() * sizeof(RgR128TrackDev);  // (a multiple of 8: the fold's items follow)
    RG_HIP(c, st.d_desc.reserve(desc_bytes + fold.size() * sizeof(RgR128FoldItem)));
    RG_HIP(c, st.d_words.reserve(3 * n));
    RG_HIP(c, st.d_res.reserve(n));
    if (block_z_out) RG_HIP(c, st.d_z.reserve(total_z ? total_z : 1));
    const RgR128TrackDev *d_tr = reinterpret_cast<const RgR128TrackDev *>(st.d_desc.p);
    uint32_t *d_peak = st.d_words.p, *d_tp = st.d_words.p + n, *d_flags = st.d_words.p + 2 * n;
    RG_HIP(c, hipMemcpyAsync(st.d_desc.p, blob.data(), desc_bytes, hipMemcpyHostToDevice, s));
    if (!fold.empty())
        RG_HIP(c, hipMemcpyAsync(st.d_desc.p + desc_bytes, fold.data(), fold.size() * sizeof(RgR128FoldItem), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipMemsetAsync(st.d_words.p, 0, 3 * n * sizeof(uint32_t), s));
    for (int f = 0; f < 3; ++f) {
        if (!main_l[f].count) continue;
        const RgR128TrackDev *l = d_tr + main_l[f].first;
        if (f == RG_FMT_F32_PLANAR) launch_main<RG_FMT_F32_PLANAR>(l, (uint32_t)main_l[f].count, main_l[f].units, d_peak, d_flags, s);
        else if (f == RG_FMT_S16_PLANAR) launch_main<RG_FMT_S16_PLANAR>(l, (uint32_t)main_l[f].count, main_l[f].units, d_peak, d_flags, s);
        else launch_main<RG_FMT_S32_PLANAR>(l, (uint32_t)main_l[f].count, main_l[f].units, d_peak, d_flags, s);
        RG_HIP(c, hipGetLastError());
    }
    if (!fold.empty())
        RG_HIP(c, (hipError_t)rg_r128_fold_launch(reinterpret_cast<const RgR128FoldItem *>(st.d_desc.p + desc_bytes), (uint32_t)fold.size(),
                                                  fold_blocks, s));
    if (want_tp)
        for (int f = 0; f < 3; ++f)
            for (int k = 0; k < 2; ++k) {
                if (!tp_l[f][k].count) continue;
                const RgR128TrackDev *l = d_tr + tp_l[f][k].first;
                const uint32_t factor = k ? 2 : 4, cnt = (uint32_t)tp_l[f][k].count;
                if (f == RG_FMT_F32_PLANAR) launch_tp<RG_FMT_F32_PLANAR>(factor, l, cnt, tp_l[f][k].units, tp_l[f][k].ny, d_tp, s);
                else if (f == RG_FMT_S16_PLANAR) launch_tp<RG_FMT_S16_PLANAR>(factor, l, cnt, tp_l[f][k].units, tp_l[f][k].ny, d_tp, s);
                else launch_tp<RG_FMT_S32_PLANAR>(factor, l, cnt, tp_l[f][k].units, tp_l[f][k].ny, d_tp, s);
                RG_HIP(c, hipGetLastError());
            }
    hipLaunchKernelGGL(rg_r128_gate_kernel, dim3((uint32_t)n), dim3(256), 0, s, d_tr, rg_r128_abs_gate(), (const uint32_t *)d_peak,
                       (const uint32_t *)(want_tp ? d_tp : nullptr), (const uint32_t *)d_flags, st.d_res.p,
                       block_z_out ? st.d_z.p : (double *)nullptr);
    RG_HIP(c, hipGetLastError());
    RG_HIP(c, hipMemcpyAsync(out, st.d_res.p, n * sizeof(rg_r128_track_result), hipMemcpyDeviceToHost, s));
    if (block_z_out && total_z) RG_HIP(c, hipMemcpyAsync(block_z_out, st.d_z.p, total_z * sizeof(double), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    if (tr_out) std::copy(tr.begin(), tr.end(), tr_out);
    if (keep)
        for (size_t i = 0; i < n; ++i) {
            st.kept.push_back(tr[i]);
            st.kept_res.push_back(out[i]);
        }
    else if (dyn_out)
        return rg_r128_dynamics_run(c, &st.range, tr.data(), out, n, dyn_out, st_z_out);
    return RG_OK;
}

// One album is the many-albums stage with n_albums == 1: the empty album's record, the gates over the union, the peaks, the
// NaN rule and the dynamics are all rg_r128_albums_stage's.
int rg_r128_album_end(rg_ctx *c, int want_tp, rg_r128_album_result *album_out, rg_r128_dynamics *dyn_out,
                      rg_r128_dynamics *album_dyn_out, double *st_z_out) {
    if (!c || !album_out) return RG_ERR_INVALID_ARG;
    R128State &st = state(c);
    const size_t n = st.kept.size(), first[2] = {0, n};
    int rc = n ? rg_bind_device(c) : RG_OK;
    if (rc == RG_OK)
        rc = rg_r128_albums_stage(c, st.kept.data(), st.kept_res.data(), n, first, 1, want_tp, album_out, dyn_out, album_dyn_out, st_z_out);
    st.drop_album();
    return rc;
}

namespace {

int pcm_batch(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes, int on_device, int want_tp,
              rg_r128_track_result *out, double *block_z_out, rg_r128_dynamics *dyn_out, double *st_z_out) {
    if (!c) return RG_ERR_INVALID_ARG;
    if (n && !pcm_base) return rg_set_err(c, RG_ERR_INVALID_ARG, "null pcm_base");
    int rc = r128_validate(c, tracks, n, pcm_bytes);  // before anything is copied
    if (rc != RG_OK) return rc;
    const void *d_base = nullptr;
    rc = rg_stage_pcm(c, pcm_base, pcm_bytes, on_device, &d_base);
    if (rc != RG_OK) return rc;
    return rg_r128_run(c, tracks, n, d_base, pcm_bytes, want_tp, 0, out, block_z_out, dyn_out, st_z_out);
}

int album_pcm(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes, int on_device, int want_tp,
              rg_r128_track_result *tracks_out, rg_r128_album_result *album_out, double *block_z_out, rg_r128_dynamics *dyn_out,
              rg_r128_dynamics *album_dyn_out, double *st_z_out) {
    if (!c || !album_out) return RG_ERR_INVALID_ARG;
    if (n && !pcm_base) return rg_set_err(c, RG_ERR_INVALID_ARG, "null pcm_base");
    int rc = r128_validate(c, tracks, n, pcm_bytes);
    if (rc != RG_OK) return rc;
    const void *d_base = nullptr;
    rc = rg_stage_pcm(c, pcm_base, pcm_bytes, on_device, &d_base);
    if (rc != RG_OK) return rc;
    rg_r128_album_reset(c);
    rc = rg_r128_run(c, tracks, n, d_base, pcm_bytes, want_tp, 1, tracks_out, block_z_out);
    if (rc != RG_OK) {
        rg_r128_album_reset(c);
        return rc;
    }
    return rg_r128_album_end(c, want_tp, album_out, dyn_out, album_dyn_out, st_z_out);
}

}  // namespace

extern "C" int rg_r128_analyze_pcm_batch(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                                         int on_device, int want_tp, rg_r128_track_result *out, double *block_z_out) {
    return pcm_batch(c, tracks, n, pcm_base, pcm_bytes, on_device, want_tp, out, block_z_out, nullptr, nullptr);
}

extern "C" int rg_r128_analyze_album_pcm(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                                         int on_device, int want_tp, rg_r128_track_result *tracks_out,
                                         rg_r128_album_result *album_out, double *block_z_out) {
    return album_pcm(c, tracks, n, pcm_base, pcm_bytes, on_device, want_tp, tracks_out, album_out, block_z_out, nullptr, nullptr, nullptr);
}

extern "C" int rg_r128_analyze_pcm_batch_dynamics(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base,
                                                  size_t pcm_bytes, int on_device, int want_tp, rg_r128_track_result *out,
                                                  double *block_z_out, rg_r128_dynamics *dyn_out, double *st_z_out) {
    if (c && n && !dyn_out) return rg_set_err(c, RG_ERR_INVALID_ARG, "null dyn_out");
    return pcm_batch(c, tracks, n, pcm_base, pcm_bytes, on_device, want_tp, out, block_z_out, dyn_out, st_z_out);
}

extern "C" int rg_r128_analyze_album_pcm_dynamics(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *pcm_base,
                                                  size_t pcm_bytes, int on_device, int want_tp, rg_r128_track_result *tracks_out,
                                                  rg_r128_album_result *album_out, double *block_z_out, rg_r128_dynamics *dyn_out,
                                                  rg_r128_dynamics *album_dyn_out, double *st_z_out) {
    if (c && ((n && !dyn_out) || !album_dyn_out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "null dynamics output");
    return album_pcm(c, tracks, n, pcm_base, pcm_bytes, on_device, want_tp, tracks_out, album_out, block_z_out, dyn_out, album_dyn_out,
                     st_z_out);
}
