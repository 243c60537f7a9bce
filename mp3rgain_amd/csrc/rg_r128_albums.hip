// rg_r128_albums.hip -- the album stage of the EBU R 128 path: every album of a call (of a group of files) in the same
// launches, segmented over the arrays the track stage leaves on the device.  The single-album entry points come here too
// (rg_r128.hip: rg_r128_album_end, one album over every kept track), so there is one album stage and an album's record
// does not depend on how many albums share its call.  The pieces shared with the track kernels (a block's value, the fold
// tree, the radix select's steps) are in rg_r128_inl.h.  DESIGN.md section 14.2.
//
//  rg_r128a_gate_kernel         integrated loudness: one workgroup per album walks the album's tracks.
//  rg_r128a_select_kernel       loudness range of the small albums: one workgroup per album over its range of the
//                               short-term block array (tracks lie one after another there, so an album is contiguous).
//  rg_r128a_wide_gate_kernel    loudness range of the wide albums (from RG_R128R_WIDE_FROM blocks on): grid = (slices, album).
//  rg_r128a_wide_count_kernel   The threshold's sum is over RG_R128R_WIDE fixed slices of the album's own block list (a
//  rg_r128a_wide_finish_kernel  workgroup takes one, or several one after another, never merged), whatever the grid; the
//                               counting passes are integer counts and take at least RG_R128A_COUNT_MIN values per workgroup.
// Integer atomics only; every launch reads what the launch before it left in global memory and no launch reads what it writes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rg_ctx.h"
#include "rg_r128.h"
#include "rg_r128_inl.h"

#define RG_R128A_GATE_SLICES 4      // slices of the threshold's sum one workgroup takes, from that many albums in a round on
#define RG_R128A_COUNT_MIN 4096u    // values of a counting workgroup, at least (two 4096-bin histograms are cleared and flushed)

struct RgR128AlbumDev {
    uint64_t st_off;                    // the album's first short-term block in the block array
    uint32_t st_count;                  // its short-term blocks
    uint32_t track_first, track_count;  // its tracks in the track array
    uint32_t out;                       // its record in the output arrays
    uint32_t count_wgs;                 // wide: the workgroups that count, each over ceil(st_count / count_wgs) blocks
    uint32_t pad;
};

// =================================================================================================
// Integrated loudness: one workgroup per album over the union of its tracks' gating blocks, in track order; the passes, the
// per-thread order and the fold are rg_r128_gate_kernel's.  Peaks, and the NaN of an album with a track that is not finite,
// are the host's (it has the tracks' results).
__global__ void __launch_bounds__(256)
rg_r128a_gate_kernel(const RgR128TrackDev *__restrict__ tracks, const RgR128AlbumDev *__restrict__ albums, const double abs_gate,
                     rg_r128_album_result *__restrict__ out) {
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256];
    const uint32_t t0 = albums[blockIdx.x].track_first, n_list = albums[blockIdx.x].track_count;
    double thr = abs_gate;
    double sum = 0.0;
    uint32_t cnt = 0, total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        sum = 0.0;
        cnt = 0;
        total = 0;
        for (uint32_t k = 0; k < n_list; ++k) {
            const RgR128TrackDev &T = tracks[t0 + k];
            const uint32_t nb = T.H > 3u ? T.H - 3u : 0u;
            total += nb;
            for (uint32_t b = threadIdx.x; b < nb; b += 256) {
                const double z = r128_block_z(T, b);
                if (z >= abs_gate && z >= thr) {
                    sum += z;
                    ++cnt;
                }
            }
        }
        r128_fold(sh_sum, sh_cnt, sum, cnt);
        if (pass == 0) thr = cnt ? 0.1 * (sum / (double)cnt) : abs_gate;
    }
    if (threadIdx.x) return;
    double lufs = -__builtin_inf(), gain = 0.0;
    if (cnt) {
        lufs = -0.691 + 10.0 * log10(sum / (double)cnt);
        gain = RG_R128_REFERENCE_LUFS - lufs;
    }
    rg_r128_album_result a;
    a.loudness_lufs = lufs;
    a.gain_db = gain;
    a.sample_peak = 0.0;
    a.true_peak = __builtin_nan("");
    a.blocks = total;
    a.blocks_gated = cnt;
    out[albums[blockIdx.x].out] = a;
}

// =================================================================================================
// Loudness range, small albums: rg_r128r_select_kernel's gates and radix select, one workgroup per album over the album's
// range of the block array; the maxima are the integer max over its tracks' words.
__global__ void __launch_bounds__(256)
rg_r128a_select_kernel(const RgR128AlbumDev *__restrict__ albums, const double *__restrict__ st, const double abs_gate,
                       const unsigned long long *__restrict__ max_bits, rg_r128_dynamics *__restrict__ out) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ double sh_sum[256];
    __shared__ unsigned long long sh_max[512];
    __shared__ uint32_t sh_cnt[256], scan[256], pick[2];
    const int tid = threadIdx.x;
    const RgR128AlbumDev A = albums[blockIdx.x];
    const double *const v = st + A.st_off;
    const uint32_t N = A.st_count;

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
    r128r_album_maxima(max_bits + 2 * (size_t)A.track_first, A.track_count, sh_max);
    if (tid == 0) {
        rg_r128_dynamics d;
        r128r_finish(d, N, sel.n, sel.prefix[0], sel.prefix[1], sh_max[0], sh_max[1]);
        out[A.out] = d;
    }
}

// =================================================================================================
// Loudness range, wide albums: every pass of the selection is a launch, the album is the grid's second dimension, and album y
// of the round has its selection state at wide + y * kWideBytes.  Slice g of the threshold's sum is the fixed range
// [g * slice, (g + 1) * slice) of the album's blocks; a counting workgroup takes the fixed range its index gives.  Every
// launch first brings the selection's state up to date from what the launch before it left in global memory (the partial
// sums, the histogram) -- every workgroup for itself, all with the same result -- and workgroup 0 stores that state for the
// next launch: sel[0] holds the threshold, sel[p + 1] the state before counting pass p.
__global__ void __launch_bounds__(256)
rg_r128a_wide_gate_kernel(const RgR128AlbumDev *__restrict__ albums, const double *__restrict__ st, const double abs_gate,
                          const int pass, const uint32_t slices /* a workgroup walks: gridDim.x * slices == RG_R128R_WIDE */,
                          unsigned char *__restrict__ wide) {
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256];
    const RgR128AlbumDev A = albums[blockIdx.y];
    unsigned char *const w = wide + (size_t)blockIdx.y * kWideBytes;
    RgR128RangeSel *const sel = reinterpret_cast<RgR128RangeSel *>(w + kWideSel);
    double *const psum = reinterpret_cast<double *>(w + kWidePsum);
    uint32_t *const pcnt = reinterpret_cast<uint32_t *>(w + kWidePcnt);
    const double *const v = st + A.st_off;
    const uint32_t N = A.st_count;
    double thr = abs_gate;
    if (pass) {
        double sum = psum[threadIdx.x];  // RG_R128R_WIDE == the workgroup's size
        uint32_t cnt = pcnt[threadIdx.x];
        r128_fold(sh_sum, sh_cnt, sum, cnt);
        thr = cnt ? 0.01 * (sum / (double)cnt) : abs_gate;
        if (blockIdx.x == 0 && threadIdx.x == 0) sel[0].thr = thr;
    }
    const uint32_t slice = (N + RG_R128R_WIDE - 1) / RG_R128R_WIDE;
    for (uint32_t g = blockIdx.x * slices; g < (blockIdx.x + 1) * slices; ++g) {
        const uint64_t i0 = (uint64_t)g * slice;
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
        r128_fold(sh_sum, sh_cnt, sum, cnt);
        if (threadIdx.x == 0) {
            psum[pass * RG_R128R_WIDE + g] = sum;
            pcnt[pass * RG_R128R_WIDE + g] = cnt;
        }
    }
}

__global__ void __launch_bounds__(256)
rg_r128a_wide_count_kernel(const RgR128AlbumDev *__restrict__ albums, const double *__restrict__ st, const double abs_gate,
                           const int pass, unsigned char *__restrict__ wide) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ double sh_sum[256];
    __shared__ uint32_t sh_cnt[256], scan[256], pick[2];
    const int tid = threadIdx.x;
    const RgR128AlbumDev A = albums[blockIdx.y];
    if (blockIdx.x >= A.count_wgs) return;  // the grid is as wide as the round's largest album needs
    unsigned char *const w = wide + (size_t)blockIdx.y * kWideBytes;
    RgR128RangeSel *const sel = reinterpret_cast<RgR128RangeSel *>(w + kWideSel);
    const uint32_t *const pcnt = reinterpret_cast<const uint32_t *>(w + kWidePcnt);
    uint32_t *const ghist = reinterpret_cast<uint32_t *>(w + kWideHist);
    RgR128RangeSel s;
    if (pass == 0) {
        double sum = 0.0;
        uint32_t cnt = pcnt[RG_R128R_WIDE + tid];
        r128_fold(sh_sum, sh_cnt, sum, cnt);
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
    const uint32_t chunk = (A.st_count + A.count_wgs - 1) / A.count_wgs;
    const uint64_t i0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t i1 = i0 + chunk < A.st_count ? i0 + chunk : A.st_count;
    if (s.n) r128r_count_slice(hist, st + A.st_off, i0, i1, abs_gate, s, pass);
    __syncthreads();
    uint32_t *const g = ghist + (size_t)pass * 2 * RG_R128R_BINS;
    const int used = s.prefix[0] == s.prefix[1] ? RG_R128R_BINS : 2 * RG_R128R_BINS;
    for (int b = tid; b < used; b += 256)
        if (hist[b]) atomicAdd(&g[b], hist[b]);
}

__global__ void __launch_bounds__(256)
rg_r128a_wide_finish_kernel(const RgR128AlbumDev *__restrict__ albums, const unsigned char *__restrict__ wide,
                            const unsigned long long *__restrict__ max_bits, rg_r128_dynamics *__restrict__ out) {
    __shared__ uint32_t hist[2 * RG_R128R_BINS];
    __shared__ unsigned long long sh_max[512];
    __shared__ uint32_t scan[256], pick[2];
    const int tid = threadIdx.x;
    const RgR128AlbumDev A = albums[blockIdx.x];
    const unsigned char *const w = wide + (size_t)blockIdx.x * kWideBytes;
    RgR128RangeSel s = reinterpret_cast<const RgR128RangeSel *>(w + kWideSel)[RG_R128R_PASSES];
    const uint32_t *const g = reinterpret_cast<const uint32_t *>(w + kWideHist) + (size_t)(RG_R128R_PASSES - 1) * 2 * RG_R128R_BINS;
    for (int b = tid; b < 2 * RG_R128R_BINS; b += 256) hist[b] = g[b];
    __syncthreads();
    r128r_advance(s, hist, scan, pick, RG_R128R_PASSES - 1);
    r128r_album_maxima(max_bits + 2 * (size_t)A.track_first, A.track_count, sh_max);
    if (tid == 0) {
        rg_r128_dynamics d;
        r128r_finish(d, A.st_count, s.n, s.prefix[0], s.prefix[1], sh_max[0], sh_max[1]);
        out[A.out] = d;
    }
}

// =================================================================================================
// host driver
namespace {

static_assert(RG_R128R_WIDE % RG_R128A_GATE_SLICES == 0, "a gate workgroup takes whole slices");
static_assert(kWideBytes % 8 == 0, "the albums' selection states lie one after another");

struct AlbumsState {
    DevBuf<RgR128TrackDev> d_tr;
    DevBuf<RgR128AlbumDev> d_albums;  // every album with tracks | the small ones | the wide ones
    DevBuf<rg_r128_album_result> d_res;
    DevBuf<rg_r128_dynamics> d_dyn;
    DevBuf<unsigned char> d_wide;     // RG_R128A_ROUND selection states at most
};

}  // namespace

void rg_r128_albums_free(void *p) {
    AlbumsState *s = static_cast<AlbumsState *>(p);
    if (!s) return;
    s->d_tr.release();
    s->d_albums.release();
    s->d_res.release();
    s->d_dyn.release();
    s->d_wide.release();
    delete s;
}

extern "C" uint32_t rg_r128_albums_count_workgroups(uint64_t st_blocks) {
    const uint64_t w = st_blocks / RG_R128A_COUNT_MIN;  // every workgroup's share is RG_R128A_COUNT_MIN values or more
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(w, 1), RG_R128R_WIDE);
}

extern "C" size_t rg_r128_albums_wide_rounds(size_t wide_albums, size_t *state_bytes) {
    if (state_bytes) *state_bytes = std::min<size_t>(wide_albums, RG_R128A_ROUND) * kWideBytes;
    return (wide_albums + RG_R128A_ROUND - 1) / RG_R128A_ROUND;
}

int rg_r128_albums_stage(rg_ctx *c, const RgR128TrackDev *tr, const rg_r128_track_result *res, size_t n, const size_t *first,
                         size_t n_albums, int want_tp, rg_r128_album_result *albums_out, rg_r128_dynamics *dyn_out,
                         rg_r128_dynamics *albums_dyn_out, double *st_z_out) {
    for (size_t a = 0; a < n_albums; ++a) {  // what an album without tracks keeps
        memset(&albums_out[a], 0, sizeof albums_out[a]);
        albums_out[a].loudness_lufs = -INFINITY;
        albums_out[a].true_peak = want_tp ? 0.0 : NAN;
        if (albums_dyn_out) rg_r128_dynamics_none(&albums_dyn_out[a]);
    }
    if (n == 0) return RG_OK;
    if (n > 0x7FFFFFFFull || n_albums > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many tracks or albums");
    void **slot = rg_r128_albums_slot(c);
    if (!*slot) *slot = new AlbumsState();
    AlbumsState &st = *static_cast<AlbumsState *>(*slot);
    hipStream_t s = c->slot().stream;
    const double gate = rg_r128_abs_gate();

    RgR128RangeDev dev;
    if (albums_dyn_out) {  // stage 1 and the per-track selection over all n tracks, as the track call launches them
        const int rc = rg_r128_range_tracks(c, rg_r128_range_slot(c), tr, n, &dev);
        if (rc != RG_OK) return rc;
    }
    std::vector<RgR128AlbumDev> all, small, wide;
    const int select = rg_r128_album_select(c);
    for (size_t a = 0; a < n_albums; ++a) {
        if (first[a + 1] == first[a]) continue;
        RgR128AlbumDev d;
        memset(&d, 0, sizeof d);
        d.track_first = (uint32_t)first[a];
        d.track_count = (uint32_t)(first[a + 1] - first[a]);
        d.out = (uint32_t)a;
        if (albums_dyn_out) {
            d.st_off = dev.st_base[first[a]];
            d.st_count = (uint32_t)(dev.st_base[first[a + 1]] - d.st_off);
            d.count_wgs = rg_r128_albums_count_workgroups(d.st_count);
            (rg_r128_album_select_form(select, d.st_count) == 2 ? wide : small).push_back(d);
        }
        all.push_back(d);
    }
    const size_t n_all = all.size(), n_small = small.size(), n_wide = wide.size();
    if (n_all) {
        all.insert(all.end(), small.begin(), small.end());
        all.insert(all.end(), wide.begin(), wide.end());
        RG_HIP(c, st.d_tr.reserve(n));
        RG_HIP(c, st.d_albums.reserve(all.size()));
        RG_HIP(c, st.d_res.reserve(n_albums));
        if (albums_dyn_out) RG_HIP(c, st.d_dyn.reserve(n_albums));
        RG_HIP(c, hipMemcpyAsync(st.d_tr.p, tr, n * sizeof(RgR128TrackDev), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemcpyAsync(st.d_albums.p, all.data(), all.size() * sizeof(RgR128AlbumDev), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(rg_r128a_gate_kernel, dim3((uint32_t)n_all), dim3(256), 0, s, (const RgR128TrackDev *)st.d_tr.p,
                           (const RgR128AlbumDev *)st.d_albums.p, gate, st.d_res.p);
        RG_HIP(c, hipGetLastError());
    }
    if (n_small) {
        hipLaunchKernelGGL(rg_r128a_select_kernel, dim3((uint32_t)n_small), dim3(256), 0, s, (const RgR128AlbumDev *)st.d_albums.p + n_all,
                           dev.st, gate, dev.max_bits, st.d_dyn.p);
        RG_HIP(c, hipGetLastError());
    }
    if (n_wide) RG_HIP(c, st.d_wide.reserve(std::min<size_t>(n_wide, RG_R128A_ROUND) * kWideBytes));
    for (size_t r0 = 0; r0 < n_wide; r0 += RG_R128A_ROUND) {  // the wide albums, RG_R128A_ROUND selection states at a time
        const uint32_t nr = (uint32_t)std::min<size_t>(n_wide - r0, RG_R128A_ROUND);
        const RgR128AlbumDev *d_round = st.d_albums.p + n_all + n_small + r0;
        uint32_t wgs = 1;
        for (uint32_t k = 0; k < nr; ++k) wgs = std::max(wgs, wide[r0 + k].count_wgs);
        // a few albums: a workgroup per slice, so that the launch still fills the chip (measured: one album of 1.77 M blocks,
        // 8.6 us a pass by 256 workgroups, 27 us by 64); the slices themselves do not change, nor do the bits
        const uint32_t slices = nr < RG_R128A_GATE_SLICES ? 1u : RG_R128A_GATE_SLICES;
        RG_HIP(c, hipMemsetAsync(st.d_wide.p, 0, (size_t)nr * kWideBytes, s));
        for (int pass = 0; pass < 2; ++pass)
            hipLaunchKernelGGL(rg_r128a_wide_gate_kernel, dim3(RG_R128R_WIDE / slices, nr), dim3(256), 0, s, d_round, dev.st, gate, pass,
                               slices, st.d_wide.p);
        RG_HIP(c, hipGetLastError());
        for (int pass = 0; pass < RG_R128R_PASSES; ++pass)
            hipLaunchKernelGGL(rg_r128a_wide_count_kernel, dim3(wgs, nr), dim3(256), 0, s, d_round, dev.st, gate, pass, st.d_wide.p);
        RG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(rg_r128a_wide_finish_kernel, dim3(nr), dim3(256), 0, s, d_round, (const unsigned char *)st.d_wide.p,
                           dev.max_bits, st.d_dyn.p);
        RG_HIP(c, hipGetLastError());
    }
    std::vector<rg_r128_album_result> h_res(n_albums);
    std::vector<rg_r128_dynamics> h_dyn(albums_dyn_out ? n : 0), h_adyn(albums_dyn_out ? n_albums : 0);
    if (n_all) RG_HIP(c, hipMemcpyAsync(h_res.data(), st.d_res.p, n_albums * sizeof(rg_r128_album_result), hipMemcpyDeviceToHost, s));
    if (albums_dyn_out) {
        RG_HIP(c, hipMemcpyAsync(h_dyn.data(), dev.dyn, n * sizeof(rg_r128_dynamics), hipMemcpyDeviceToHost, s));
        if (n_all) RG_HIP(c, hipMemcpyAsync(h_adyn.data(), st.d_dyn.p, n_albums * sizeof(rg_r128_dynamics), hipMemcpyDeviceToHost, s));
        if (st_z_out && dev.total) RG_HIP(c, hipMemcpyAsync(st_z_out, dev.st, dev.total * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    RG_HIP(c, hipStreamSynchronize(s));
    if (albums_dyn_out && dyn_out)
        for (size_t i = 0; i < n; ++i) {
            dyn_out[i] = h_dyn[i];
            if (res[i].flags & RG_TRACK_FLAG_NONFINITE) rg_r128_dynamics_nan(&dyn_out[i]);
        }
    for (size_t a = 0; a < n_albums; ++a) {
        if (first[a + 1] == first[a]) continue;
        bool bad = false;
        double sp = 0.0, tp = 0.0;
        for (size_t i = first[a]; i < first[a + 1]; ++i) {
            bad = bad || (res[i].flags & RG_TRACK_FLAG_NONFINITE);
            sp = std::max(sp, res[i].sample_peak);
            if (want_tp) tp = std::max(tp, res[i].true_peak);
        }
        albums_out[a] = h_res[a];
        albums_out[a].sample_peak = sp;
        albums_out[a].true_peak = want_tp ? tp : NAN;
        if (bad) albums_out[a].loudness_lufs = albums_out[a].gain_db = NAN;
        if (albums_dyn_out) {
            albums_dyn_out[a] = h_adyn[a];
            if (bad) rg_r128_dynamics_nan(&albums_dyn_out[a]);
        }
    }
    return RG_OK;
}

// =================================================================================================
// PCM entry points
namespace {

int albums_pcm(rg_ctx *c, const char *fn, const rg_track_desc *tracks, size_t n, const size_t *album_first, size_t n_albums,
               const void *pcm_base, size_t pcm_bytes, int on_device, int want_tp, rg_r128_track_result *tracks_out,
               rg_r128_album_result *albums_out, double *block_z_out, bool dynamics, rg_r128_dynamics *dyn_out,
               rg_r128_dynamics *albums_dyn_out, double *st_z_out, const rg_r128_channel_weights *weights = nullptr) {
    if (!c) return RG_ERR_INVALID_ARG;
    if ((n && (!tracks || !pcm_base || !tracks_out || (dynamics && !dyn_out))) || (n_albums && (!albums_out || (dynamics && !albums_dyn_out))))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: null input or output array", fn);
    std::string why;
    if (rg_albums_check(album_first, n_albums, n, &why) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: %s", fn, why.c_str());
    const void *d_base = nullptr;
    int rc = rg_stage_pcm(c, pcm_base, pcm_bytes, on_device, &d_base);
    if (rc != RG_OK) return rc;
    // one pass over all n tracks (S from the whole batch), their hop energies stay in the context's buffer for the album stage
    std::vector<RgR128TrackDev> tr(n);
    rc = rg_r128_run(c, tracks, n, d_base, pcm_bytes, want_tp, 0, tracks_out, block_z_out, nullptr, nullptr, tr.data(), nullptr, weights);
    if (rc != RG_OK) return rc;
    rg_r128_dynamics none;  // (n_albums == 0 with dynamics: the stage still wants to know that they were asked for)
    return rg_r128_albums_stage(c, tr.data(), tracks_out, n, album_first, n_albums, want_tp, albums_out, dyn_out,
                                dynamics ? (albums_dyn_out ? albums_dyn_out : &none) : nullptr, st_z_out);
}

}  // namespace

extern "C" int rg_r128_analyze_albums_pcm(rg_ctx *c, const rg_track_desc *tracks, size_t n, const size_t *album_first, size_t n_albums,
                                          const void *pcm_base, size_t pcm_bytes, int pcm_on_device, int want_true_peak,
                                          rg_r128_track_result *tracks_out, rg_r128_album_result *albums_out, double *block_z_out) {
    return albums_pcm(c, "rg_r128_analyze_albums_pcm", tracks, n, album_first, n_albums, pcm_base, pcm_bytes, pcm_on_device,
                      want_true_peak, tracks_out, albums_out, block_z_out, false, nullptr, nullptr, nullptr);
}

extern "C" int rg_r128_analyze_albums_pcm_dynamics(rg_ctx *c, const rg_track_desc *tracks, size_t n, const size_t *album_first,
                                                   size_t n_albums, const void *pcm_base, size_t pcm_bytes, int pcm_on_device,
                                                   int want_true_peak, rg_r128_track_result *tracks_out,
                                                   rg_r128_album_result *albums_out, double *block_z_out, rg_r128_dynamics *dyn_out,
                                                   rg_r128_dynamics *albums_dyn_out, double *st_z_out) {
    return albums_pcm(c, "rg_r128_analyze_albums_pcm_dynamics", tracks, n, album_first, n_albums, pcm_base, pcm_bytes, pcm_on_device,
                      want_true_peak, tracks_out, albums_out, block_z_out, true, dyn_out, albums_dyn_out, st_z_out);
}

// The most general PCM call: per-track channel weights (nullptr: by the context's channel mode), albums or none, dynamics
// or none.
extern "C" int rg_r128_analyze_pcm_weighted(rg_ctx *c, const rg_track_desc *tracks, const rg_r128_channel_weights *weights, size_t n,
                                            const size_t *album_first, size_t n_albums, const void *pcm_base, size_t pcm_bytes,
                                            int pcm_on_device, int want_true_peak, rg_r128_track_result *tracks_out,
                                            rg_r128_album_result *albums_out, double *block_z_out, rg_r128_dynamics *dyn_out,
                                            rg_r128_dynamics *albums_dyn_out, double *st_z_out) {
    const char *fn = "rg_r128_analyze_pcm_weighted";
    if (!c) return RG_ERR_INVALID_ARG;
    if (album_first || n_albums)
        return albums_pcm(c, fn, tracks, n, album_first, n_albums, pcm_base, pcm_bytes, pcm_on_device, want_true_peak, tracks_out, albums_out,
                          block_z_out, dyn_out != nullptr || albums_dyn_out != nullptr, dyn_out, albums_dyn_out, st_z_out, weights);
    if (n && (!tracks || !pcm_base || !tracks_out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: null input or output array", fn);
    const void *d_base = nullptr;
    const int rc = rg_stage_pcm(c, pcm_base, pcm_bytes, pcm_on_device, &d_base);
    if (rc != RG_OK) return rc;
    return rg_r128_run(c, tracks, n, d_base, pcm_bytes, want_true_peak, 0, tracks_out, block_z_out, dyn_out, st_z_out, nullptr, nullptr, weights);
}
