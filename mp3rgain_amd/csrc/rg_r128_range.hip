// rg_r128_range.hip -- loudness range (EBU Tech 3342) and the momentary / short-term maxima of the EBU R 128 path on gfx950,
// from the hop energies the loudness kernel of rg_r128.hip leaves on the device.  No PCM is read again.  The definitions
// are in include/mp3rgain_amd_r128.h; DESIGN.md section 14.1 has the shapes, the bytes and the measured time.
//
// Stage 1 (rg_r128r_blocks_kernel): a wide launch over (track, chunk of 1024 block positions).  A workgroup sums the two
//   channels' hop energies of its chunk (+ 29 hops) into LDS once, forms every short-term block by a direct 30-term sum in
//   ascending hop order and stores it, forms the momentary blocks exactly as the gate kernel does, and folds both maxima
//   into the track's two 64-bit words by an integer max on the bits of the non-negative doubles.
// Stage 2 (rg_r128r_select_kernel): one workgroup per track.  Two gate passes (fixed per-thread order, fixed fold tree),
//   then a radix select on the values' bit patterns, 12 bits a pass (the last one 4), for both percentiles at once: counting
//   into two LDS histograms of 4096 integers, a prefix scan, the digit, the rank within it.  What comes out are two elements
//   of the block list, bit for bit.
// An album's selection runs over its range of the block array these stages leave on the device (tracks are laid out one
//   after another): rg_r128_albums.hip, for one album as for many.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "rg_ctx.h"
#include "rg_r128.h"
#include "rg_r128_inl.h"

#define RG_R128R_CHUNK 1024

// =================================================================================================
// Stage 1: short-term blocks and the two maxima.
__global__ void __launch_bounds__(256)
rg_r128r_blocks_kernel(const RgR128RangeTrack *__restrict__ tracks, const uint32_t n_tracks, double *__restrict__ st,
                       unsigned long long *__restrict__ max_bits /* [n_tracks][2]: momentary, short-term */) {
    __shared__ double c[RG_R128R_CHUNK + 32];
    const int tid = threadIdx.x;
    uint32_t lo = 0, hi = n_tracks - 1;
    while (lo < hi) {  // the last track whose first workgroup is not past this one (a track without blocks has none)
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (tracks[mid].chunk_base <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const RgR128RangeTrack T = tracks[lo];
    const uint32_t h0 = (blockIdx.x - T.chunk_base) * RG_R128R_CHUNK;
    for (uint32_t i = tid; i < RG_R128R_CHUNK + RG_R128R_ST_HOPS - 1; i += 256) {
        const uint32_t h = h0 + i;
        double v = 0.0;
        if (h < T.H) {
            v = T.e[h];
            if (T.nch >= 2) v += T.e[(size_t)T.H + h];
        }
        c[i] = v;
    }
    __syncthreads();
    const double dm = 4.0 * (double)T.hop, ds = (double)RG_R128R_ST_HOPS * (double)T.hop;
    unsigned long long mm = 0, sm = 0;
    for (uint32_t j = tid; j < RG_R128R_CHUNK; j += 256) {
        const uint32_t b = h0 + j;
        if (b + 4u <= T.H) {  // the gate kernel's order (rg_r128.hip: r128_block_z)
            const double z = (((c[j] + c[j + 1]) + c[j + 2]) + c[j + 3]) / dm;
            mm = r128r_umax(mm, (unsigned long long)__double_as_longlong(z));
        }
        if (b + (uint32_t)RG_R128R_ST_HOPS <= T.H) {
            double s = c[j];
#pragma unroll
            for (int k = 1; k < RG_R128R_ST_HOPS; ++k) s += c[j + k];
            const double v = s / ds;
            st[T.st_base + b] = v;
            sm = r128r_umax(sm, (unsigned long long)__double_as_longlong(v));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mm = r128r_umax(mm, __shfl_xor(mm, d, 64));
        sm = r128r_umax(sm, __shfl_xor(sm, d, 64));
    }
    if ((tid & 63) == 0) {
        if (mm) atomicMax(&max_bits[2 * lo], mm);
        if (sm) atomicMax(&max_bits[2 * lo + 1], sm);
    }
}

// =================================================================================================
// Stage 2: both gates and the two percentiles, one workgroup per track.
__global__ void __launch_bounds__(256)
rg_r128r_select_kernel(const RgR128RangeTrack *__restrict__ tracks, const double *__restrict__ st, const double abs_gate,
                       const unsigned long long *__restrict__ max_bits, rg_r128_dynamics *__restrict__ out /* [n_tracks] */) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256], scan[256], pick[2];
    const int tid = threadIdx.x;
    const double *const v = st + tracks[blockIdx.x].st_base;
    const uint32_t N = tracks[blockIdx.x].st_count;

    double sum = 0.0;
    uint32_t cnt = 0;
    for (uint32_t i = tid; i < N; i += 256) {
        const double x = v[i];
        if (x >= abs_gate) {
            sum += x;
            ++cnt;
        }
    }
    r128_fold(sh_sum, sh_cnt, sum, cnt);
    const double thr = cnt ? 0.01 * (sum / (double)cnt) : abs_gate;
    sum = 0.0;
    cnt = 0;
    for (uint32_t i = tid; i < N; i += 256) {
        const double x = v[i];
        if (x >= abs_gate && x >= thr) ++cnt;
    }
    r128_fold(sh_sum, sh_cnt, sum, cnt);
    RgR128RangeSel sel;
    r128r_start(sel, thr, cnt);
    if (sel.n)  // uniform over the workgroup
        for (int pass = 0; pass < RG_R128R_PASSES; ++pass) {
            for (int b = tid; b < 2 * RG_R128R_BINS; b += 256) hist[b] = 0;
            __syncthreads();
            r128r_count_slice(hist, v, 0, N, abs_gate, sel, pass);
            __syncthreads();
            r128r_advance(sel, hist, scan, pick, pass);
        }
    if (tid == 0) {
        rg_r128_dynamics d;
        r128r_finish(d, N, sel.n, sel.prefix[0], sel.prefix[1], max_bits[2 * blockIdx.x], max_bits[2 * blockIdx.x + 1]);
        out[blockIdx.x] = d;
    }
}

// =================================================================================================
// host driver
namespace {

struct RangeState {
    DevBuf<RgR128RangeTrack> d_tr;
    DevBuf<double> d_st;
    DevBuf<unsigned long long> d_max;
    DevBuf<rg_r128_dynamics> d_dyn;
};

}  // namespace

extern "C" int rg_r128_album_select_form(int album_select, uint64_t st_blocks) {
    return album_select == 2 || (album_select == 0 && st_blocks >= RG_R128R_WIDE_FROM) ? 2 : 1;
}

void rg_r128_range_free(void *p) {
    RangeState *s = static_cast<RangeState *>(p);
    if (!s) return;
    s->d_tr.release();
    s->d_st.release();
    s->d_max.release();
    s->d_dyn.release();
    delete s;
}

void rg_r128_dynamics_none(rg_r128_dynamics *d) {
    memset(d, 0, sizeof *d);
    d->range_low_lufs = d->range_high_lufs = d->max_momentary_lufs = d->max_short_term_lufs = -INFINITY;
}

void rg_r128_dynamics_nan(rg_r128_dynamics *d) {
    d->loudness_range_lu = d->range_low_lufs = d->range_high_lufs = d->max_momentary_lufs = d->max_short_term_lufs = NAN;
    d->st_blocks_gated = 0;
}

// Both stages over n tracks: the track list and the block array's layout, the buffers, the two launches.
int rg_r128_range_tracks(rg_ctx *c, void **slot, const RgR128TrackDev *tr, size_t n, RgR128RangeDev *dev) {
    if (!*slot) *slot = new RangeState();
    RangeState &st = *static_cast<RangeState *>(*slot);
    hipStream_t s = c->slot().stream;
    std::vector<RgR128RangeTrack> list(n);
    dev->st_base.resize(n + 1);
    uint64_t total = 0, chunks = 0;
    for (size_t i = 0; i < n; ++i) {
        RgR128RangeTrack &o = list[i];
        memset(&o, 0, sizeof o);
        o.e = tr[i].e;
        o.H = tr[i].H;
        o.nch = tr[i].nch;
        o.hop = tr[i].hop;
        o.st_base = dev->st_base[i] = total;
        o.st_count = o.H >= RG_R128R_ST_HOPS ? o.H - (RG_R128R_ST_HOPS - 1) : 0u;
        o.chunk_base = (uint32_t)chunks;
        total += o.st_count;
        chunks += o.H > 3u ? (o.H - 3u + RG_R128R_CHUNK - 1) / RG_R128R_CHUNK : 0u;
        if (total > 0x7FFFFFFFull || chunks > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "batch too long for the loudness range");
    }
    dev->st_base[n] = total;
    RG_HIP(c, st.d_tr.reserve(n));
    RG_HIP(c, st.d_st.reserve(total ? total : 1));
    RG_HIP(c, st.d_max.reserve(2 * n));
    RG_HIP(c, st.d_dyn.reserve(n));
    RG_HIP(c, hipMemcpyAsync(st.d_tr.p, list.data(), n * sizeof(RgR128RangeTrack), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipMemsetAsync(st.d_max.p, 0, 2 * n * sizeof(unsigned long long), s));
    if (chunks) {
        hipLaunchKernelGGL(rg_r128r_blocks_kernel, dim3((uint32_t)chunks), dim3(256), 0, s, (const RgR128RangeTrack *)st.d_tr.p,
                           (uint32_t)n, st.d_st.p, st.d_max.p);
        RG_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(rg_r128r_select_kernel, dim3((uint32_t)n), dim3(256), 0, s, (const RgR128RangeTrack *)st.d_tr.p,
                       (const double *)st.d_st.p, rg_r128_abs_gate(), (const unsigned long long *)st.d_max.p, st.d_dyn.p);
    RG_HIP(c, hipGetLastError());
    dev->st = st.d_st.p;
    dev->max_bits = st.d_max.p;
    dev->dyn = st.d_dyn.p;
    dev->total = total;
    return RG_OK;
}

// The tracks-only call: the two stages, one copy back, the NaN rule.
int rg_r128_dynamics_run(rg_ctx *c, void **slot, const RgR128TrackDev *tr, const rg_r128_track_result *res, size_t n,
                         rg_r128_dynamics *out, double *st_z_out) {
    if (n == 0) return RG_OK;
    RgR128RangeDev dev;
    const int rc = rg_r128_range_tracks(c, slot, tr, n, &dev);
    if (rc != RG_OK) return rc;
    hipStream_t s = c->slot().stream;
    RG_HIP(c, hipMemcpyAsync(out, dev.dyn, n * sizeof(rg_r128_dynamics), hipMemcpyDeviceToHost, s));
    if (st_z_out && dev.total) RG_HIP(c, hipMemcpyAsync(st_z_out, dev.st, dev.total * sizeof(double), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i)
        if (res[i].flags & RG_TRACK_FLAG_NONFINITE) rg_r128_dynamics_nan(&out[i]);
    return RG_OK;
}
