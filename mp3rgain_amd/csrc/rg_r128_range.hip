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
// An album's union of blocks is the whole block array (tracks are laid out one after another).  It is selected either by one
//   more workgroup of stage 2, or, from RG_R128R_WIDE_FROM blocks on, by the same passes as wide launches
//   (rg_r128r_album_*_kernel): RG_R128R_WIDE workgroups count their fixed slice into LDS and add to a global integer
//   histogram; the next launch picks the digits from it.  Integer counts and fixed slices: nothing depends on scheduling.
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
// Stage 2: both gates and the two percentiles, one workgroup per track; workgroup n_tracks, if launched, takes the album.
__global__ void __launch_bounds__(256)
rg_r128r_select_kernel(const RgR128RangeTrack *__restrict__ tracks, const uint32_t n_tracks, const double *__restrict__ st,
                       const uint32_t album_total, const double abs_gate, const unsigned long long *__restrict__ max_bits,
                       rg_r128_dynamics *__restrict__ out /* [n_tracks], then the album's */) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ double sh_sum[256];
    __shared__ unsigned long long sh_max[512];
    __shared__ uint32_t sh_cnt[256], scan[256], pick[2];
    const int tid = threadIdx.x;
    const bool album = blockIdx.x >= n_tracks;
    const double *const v = album ? st : st + tracks[blockIdx.x].st_base;
    const uint32_t N = album ? album_total : tracks[blockIdx.x].st_count;

    double sum = 0.0;
    uint32_t cnt = 0;
    for (uint32_t i = tid; i < N; i += 256) {
        const double x = v[i];
        if (x >= abs_gate) {
            sum += x;
            ++cnt;
        }
    }
    r128r_fold(sh_sum, sh_cnt, sum, cnt);
    const double thr = cnt ? 0.01 * (sum / (double)cnt) : abs_gate;
    sum = 0.0;
    cnt = 0;
    for (uint32_t i = tid; i < N; i += 256) {
        const double x = v[i];
        if (x >= abs_gate && x >= thr) ++cnt;
    }
    r128r_fold(sh_sum, sh_cnt, sum, cnt);
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
    unsigned long long m_bits, s_bits;
    if (album) {
        r128r_album_maxima(max_bits, n_tracks, sh_max);
        m_bits = sh_max[0];
        s_bits = sh_max[1];
    } else {
        m_bits = max_bits[2 * blockIdx.x];
        s_bits = max_bits[2 * blockIdx.x + 1];
    }
    if (tid == 0) {
        rg_r128_dynamics d;
        r128r_finish(d, N, sel.n, sel.prefix[0], sel.prefix[1], m_bits, s_bits);
        out[blockIdx.x] = d;
    }
}

// =================================================================================================
// The album's selection as wide passes.  Workgroup g owns the fixed slice [g * slice, (g + 1) * slice) of the block array.
// Every launch first brings the selection's state up to date from what the launch before it left in global memory (the
// partial sums, the histogram) -- every workgroup for itself, all with the same result -- and workgroup 0 stores that state for
// the next launch: sel[0] holds the threshold, sel[p + 1] the state before counting pass p.  No launch reads what it writes.
__global__ void __launch_bounds__(256)
rg_r128r_album_gate_kernel(const double *__restrict__ v, const uint32_t N, const double abs_gate, const int pass,
                           RgR128RangeSel *__restrict__ sel, double *__restrict__ psum /* [2][WIDE] */,
                           uint32_t *__restrict__ pcnt /* [2][WIDE] */) {
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256];
    double thr = abs_gate;
    if (pass) {
        double sum = psum[threadIdx.x];  // RG_R128R_WIDE == the workgroup's size
        uint32_t cnt = pcnt[threadIdx.x];
        r128r_fold(sh_sum, sh_cnt, sum, cnt);
        thr = cnt ? 0.01 * (sum / (double)cnt) : abs_gate;
        if (blockIdx.x == 0 && threadIdx.x == 0) sel[0].thr = thr;
    }
    const uint32_t slice = (N + RG_R128R_WIDE - 1) / RG_R128R_WIDE;
    const uint64_t i0 = (uint64_t)blockIdx.x * slice;
    const uint64_t i1 = i0 + slice < N ? i0 + slice : N;
    double sum = 0.0;
    uint32_t cnt = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const double x = v[i];
        if (x >= abs_gate && x >= thr) {
            sum += x;
            ++cnt;
        }
    }
    r128r_fold(sh_sum, sh_cnt, sum, cnt);
    if (threadIdx.x == 0) {
        psum[pass * RG_R128R_WIDE + blockIdx.x] = sum;
        pcnt[pass * RG_R128R_WIDE + blockIdx.x] = cnt;
    }
}

__global__ void __launch_bounds__(256)
rg_r128r_album_count_kernel(const double *__restrict__ v, const uint32_t N, const double abs_gate, const int pass,
                            RgR128RangeSel *__restrict__ sel, const uint32_t *__restrict__ pcnt,
                            uint32_t *__restrict__ ghist /* [PASSES][2 * BINS], zero */) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256], scan[256], pick[2];
    const int tid = threadIdx.x;
    RgR128RangeSel s;
    if (pass == 0) {
        double sum = 0.0;
        uint32_t cnt = pcnt[RG_R128R_WIDE + tid];
        r128r_fold(sh_sum, sh_cnt, sum, cnt);
        r128r_start(s, sel[0].thr, cnt);
    } else {
        s = sel[pass];
        const uint32_t *const g = ghist + (size_t)(pass - 1) * 2 * RG_R128R_BINS;
        for (int b = tid; b < 2 * RG_R128R_BINS; b += 256) hist[b] = g[b];
        __syncthreads();
        r128r_advance(s, hist, scan, pick, pass - 1);
    }
    if (blockIdx.x == 0 && tid == 0) sel[pass + 1] = s;
    __syncthreads();
    for (int b = tid; b < 2 * RG_R128R_BINS; b += 256) hist[b] = 0;
    __syncthreads();
    const uint32_t slice = (N + RG_R128R_WIDE - 1) / RG_R128R_WIDE;
    const uint64_t i0 = (uint64_t)blockIdx.x * slice;
    const uint64_t i1 = i0 + slice < N ? i0 + slice : N;
    if (s.n) r128r_count_slice(hist, v, i0, i1, abs_gate, s, pass);
    __syncthreads();
    uint32_t *const g = ghist + (size_t)pass * 2 * RG_R128R_BINS;
    const int used = s.prefix[0] == s.prefix[1] ? RG_R128R_BINS : 2 * RG_R128R_BINS;
    for (int b = tid; b < used; b += 256)
        if (hist[b]) atomicAdd(&g[b], hist[b]);
}

// one workgroup after the last counting pass: the last digits, the album's maxima, its values
__global__ void __launch_bounds__(256)
rg_r128r_album_finish_kernel(const RgR128RangeSel *__restrict__ sel, const uint32_t *__restrict__ ghist,
                             const unsigned long long *__restrict__ max_bits, const uint32_t n_tracks, const uint32_t total,
                             rg_r128_dynamics *__restrict__ album_out) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ unsigned long long sh_max[512];
    __shared__ uint32_t scan[256], pick[2];
    const int tid = threadIdx.x;
    RgR128RangeSel s = sel[RG_R128R_PASSES];
    const uint32_t *const g = ghist + (size_t)(RG_R128R_PASSES - 1) * 2 * RG_R128R_BINS;
    for (int b = tid; b < 2 * RG_R128R_BINS; b += 256) hist[b] = g[b];
    __syncthreads();
    r128r_advance(s, hist, scan, pick, RG_R128R_PASSES - 1);
    r128r_album_maxima(max_bits, n_tracks, sh_max);
    if (tid == 0) {
        rg_r128_dynamics d;
        r128r_finish(d, total, s.n, s.prefix[0], s.prefix[1], sh_max[0], sh_max[1]);
        *album_out = d;
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
    // the wide album selection: RgR128RangeSel[PASSES + 1] | psum[2][WIDE] | pcnt[2][WIDE] | ghist[PASSES][2 * BINS]
    DevBuf<unsigned char> d_wide;
};

double r128r_abs_gate() { return pow(10.0, (-70.0 + 0.691) / 10.0); }

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
    s->d_wide.release();
    delete s;
}

void rg_r128_dynamics_none(rg_r128_dynamics *d) {
    memset(d, 0, sizeof *d);
    d->range_low_lufs = d->range_high_lufs = d->max_momentary_lufs = d->max_short_term_lufs = -INFINITY;
}

namespace {

// Stage 1 over n tracks: the track list and the block array's layout, the buffers, the launch.  *total_out: short-term blocks.
int range_blocks(rg_ctx *c, RangeState &st, const RgR128TrackDev *tr, size_t n, size_t dyn_slots, uint64_t *total_out,
                 std::vector<RgR128RangeTrack> *list_out) {
    hipStream_t s = c->slot().stream;
    std::vector<RgR128RangeTrack> &list = *list_out;
    list.resize(n);
    uint64_t total = 0, chunks = 0;
    for (size_t i = 0; i < n; ++i) {
        RgR128RangeTrack &o = list[i];
        memset(&o, 0, sizeof o);
        o.e = tr[i].e;
        o.H = tr[i].H;
        o.nch = tr[i].nch;
        o.hop = tr[i].hop;
        o.st_base = total;
        o.st_count = o.H >= RG_R128R_ST_HOPS ? o.H - (RG_R128R_ST_HOPS - 1) : 0u;
        o.chunk_base = (uint32_t)chunks;
        total += o.st_count;
        chunks += o.H > 3u ? (o.H - 3u + RG_R128R_CHUNK - 1) / RG_R128R_CHUNK : 0u;
        if (total > 0x7FFFFFFFull || chunks > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "batch too long for the loudness range");
    }
    RG_HIP(c, st.d_tr.reserve(n));
    RG_HIP(c, st.d_st.reserve(total ? total : 1));
    RG_HIP(c, st.d_max.reserve(2 * n));
    RG_HIP(c, st.d_dyn.reserve(dyn_slots));
    RG_HIP(c, hipMemcpyAsync(st.d_tr.p, list.data(), n * sizeof(RgR128RangeTrack), hipMemcpyHostToDevice, s));
    RG_HIP(c, hipMemsetAsync(st.d_max.p, 0, 2 * n * sizeof(unsigned long long), s));
    if (chunks) {
        hipLaunchKernelGGL(rg_r128r_blocks_kernel, dim3((uint32_t)chunks), dim3(256), 0, s, (const RgR128RangeTrack *)st.d_tr.p,
                           (uint32_t)n, st.d_st.p, st.d_max.p);
        RG_HIP(c, hipGetLastError());
    }
    *total_out = total;
    return RG_OK;
}

}  // namespace

int rg_r128_range_tracks(rg_ctx *c, void **slot, const RgR128TrackDev *tr, size_t n, RgR128RangeDev *dev) {
    if (!*slot) *slot = new RangeState();
    RangeState &st = *static_cast<RangeState *>(*slot);
    hipStream_t s = c->slot().stream;
    std::vector<RgR128RangeTrack> list;
    uint64_t total = 0;
    const int rc = range_blocks(c, st, tr, n, n, &total, &list);
    if (rc != RG_OK) return rc;
    hipLaunchKernelGGL(rg_r128r_select_kernel, dim3((uint32_t)n), dim3(256), 0, s, (const RgR128RangeTrack *)st.d_tr.p, (uint32_t)n,
                       (const double *)st.d_st.p, (uint32_t)total, r128r_abs_gate(), (const unsigned long long *)st.d_max.p, st.d_dyn.p);
    RG_HIP(c, hipGetLastError());
    dev->st = st.d_st.p;
    dev->max_bits = st.d_max.p;
    dev->dyn = st.d_dyn.p;
    dev->total = total;
    dev->st_base.resize(n + 1);
    for (size_t i = 0; i < n; ++i) dev->st_base[i] = list[i].st_base;
    dev->st_base[n] = total;
    return RG_OK;
}

void rg_r128_dynamics_nan(rg_r128_dynamics *d) {
    d->loudness_range_lu = d->range_low_lufs = d->range_high_lufs = d->max_momentary_lufs = d->max_short_term_lufs = NAN;
    d->st_blocks_gated = 0;
}

int rg_r128_dynamics_run(rg_ctx *c, void **slot, int album_select, const RgR128TrackDev *tr, const rg_r128_track_result *res,
                         size_t n, rg_r128_dynamics *out, rg_r128_dynamics *album_out, double *st_z_out) {
    if (album_out) rg_r128_dynamics_none(album_out);
    if (n == 0) return RG_OK;
    if (!*slot) *slot = new RangeState();
    RangeState &st = *static_cast<RangeState *>(*slot);
    hipStream_t s = c->slot().stream;

    std::vector<RgR128RangeTrack> list;
    uint64_t total = 0;
    const int rc = range_blocks(c, st, tr, n, n + 1, &total, &list);
    if (rc != RG_OK) return rc;
    const bool wide = album_out && rg_r128_album_select_form(album_select, total) == 2;
    const double gate = r128r_abs_gate();
    hipLaunchKernelGGL(rg_r128r_select_kernel, dim3((uint32_t)n + (album_out && !wide ? 1u : 0u)), dim3(256), 0, s,
                       (const RgR128RangeTrack *)st.d_tr.p, (uint32_t)n, (const double *)st.d_st.p, (uint32_t)total, gate,
                       (const unsigned long long *)st.d_max.p, st.d_dyn.p);
    RG_HIP(c, hipGetLastError());
    if (wide) {
        RG_HIP(c, st.d_wide.reserve(kWideBytes));
        RgR128RangeSel *sel = reinterpret_cast<RgR128RangeSel *>(st.d_wide.p + kWideSel);
        double *psum = reinterpret_cast<double *>(st.d_wide.p + kWidePsum);
        uint32_t *pcnt = reinterpret_cast<uint32_t *>(st.d_wide.p + kWidePcnt);
        uint32_t *ghist = reinterpret_cast<uint32_t *>(st.d_wide.p + kWideHist);
        RG_HIP(c, hipMemsetAsync(st.d_wide.p, 0, kWideBytes, s));
        for (int pass = 0; pass < 2; ++pass)
            hipLaunchKernelGGL(rg_r128r_album_gate_kernel, dim3(RG_R128R_WIDE), dim3(256), 0, s, (const double *)st.d_st.p,
                               (uint32_t)total, gate, pass, sel, psum, pcnt);
        RG_HIP(c, hipGetLastError());
        for (int pass = 0; pass < RG_R128R_PASSES; ++pass)
            hipLaunchKernelGGL(rg_r128r_album_count_kernel, dim3(RG_R128R_WIDE), dim3(256), 0, s, (const double *)st.d_st.p,
                               (uint32_t)total, gate, pass, sel, (const uint32_t *)pcnt, ghist);
        RG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(rg_r128r_album_finish_kernel, dim3(1), dim3(256), 0, s, (const RgR128RangeSel *)sel, (const uint32_t *)ghist,
                           (const unsigned long long *)st.d_max.p, (uint32_t)n, (uint32_t)total, st.d_dyn.p + n);
        RG_HIP(c, hipGetLastError());
    }
    std::vector<rg_r128_dynamics> host(n + 1);
    RG_HIP(c, hipMemcpyAsync(host.data(), st.d_dyn.p, (n + (album_out ? 1 : 0)) * sizeof(rg_r128_dynamics), hipMemcpyDeviceToHost, s));
    if (st_z_out && total) RG_HIP(c, hipMemcpyAsync(st_z_out, st.d_st.p, total * sizeof(double), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    bool bad = false;
    for (size_t i = 0; i < n; ++i) {
        if (res[i].flags & RG_TRACK_FLAG_NONFINITE) {
            bad = true;
            rg_r128_dynamics_nan(&host[i]);
        }
        if (out) out[i] = host[i];
    }
    if (album_out) {
        *album_out = host[n];
        if (bad) rg_r128_dynamics_nan(album_out);
    }
    return RG_OK;
}
