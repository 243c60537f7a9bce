// rg_albums.hip -- many albums in one call (rg_analyze_albums, rg_files.hip): the per-album folds and read-outs.
//
// A batch of the file route holds the tracks of one group of files, in any order and from any number of albums; an album
// may straddle batches and groups.  Every album that has files in the current group owns a live pack (the [histogram | peak]
// of RG_ALBUM_PACK_WORDS words, padded to RG_ALBUMS_PACK_STRIDE so that each pack starts on 16 bytes for the percentile's
// 16-byte loads).  The fold adds every track's bins to its album's pack (u32, wrapping: LoudnessHistogram::accumulate,
// src/replaygain.rs:658-662) and takes the max of the peak bits (album_peak.max, :1056; the peaks are >= 0, so the bit
// pattern orders like the value).  Exact integer adds and a max commute: the packs do not depend on how the work was cut.
#include <hip/hip_runtime.h>

#include "rg_device.h"
#include "rg_device_inl.h"
#include "rg_albums.h"

// ---------------------------------------------------------------------------------------------
// Segmented fold.  blockIdx.x < 47: bins [256 x, 256 x + 256) of runs of RG_ALBUMS_FOLD_TRACKS tracks (blockIdx.y, striding
// by gridDim.y); a thread sums its bin over consecutive tracks of the same album in a register and adds the sum to the pack
// when the album changes (a batch in input order: one atomic per album and bin).  blockIdx.x == 47: the peaks, one track per
// thread.  album_of[t] < 0: track t is not folded.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rg_album_fold_kernel(const uint32_t *__restrict__ hist, const unsigned long long *__restrict__ peak_bits,
                     const int32_t *__restrict__ album_of, uint32_t n_tracks, uint32_t *__restrict__ packs) {
    const int nb = (RG_HISTOGRAM_SIZE + 255) / 256;
    for (uint32_t t0 = blockIdx.y * RG_ALBUMS_FOLD_TRACKS; t0 < n_tracks; t0 += gridDim.y * RG_ALBUMS_FOLD_TRACKS) {
        const uint32_t t1 = min(t0 + (uint32_t)RG_ALBUMS_FOLD_TRACKS, n_tracks);
        if ((int)blockIdx.x < nb) {
            const int b = blockIdx.x * 256 + threadIdx.x;
            if (b >= RG_HISTOGRAM_SIZE) continue;
            int32_t cur = -1;
            uint32_t s = 0;
            for (uint32_t t = t0; t < t1; ++t) {
                const int32_t a = album_of[t];
                if (a != cur) {
                    if (cur >= 0 && s) atomicAdd(packs + (size_t)cur * RG_ALBUMS_PACK_STRIDE + b, s);
                    cur = a;
                    s = 0;
                }
                if (a >= 0) s += hist[(size_t)t * RG_HISTOGRAM_SIZE + b];
            }
            if (cur >= 0 && s) atomicAdd(packs + (size_t)cur * RG_ALBUMS_PACK_STRIDE + b, s);
        } else {
            const uint32_t t = t0 + threadIdx.x;
            if (threadIdx.x < RG_ALBUMS_FOLD_TRACKS && t < t1) {
                const int32_t a = album_of[t];
                if (a >= 0)
                    atomicMax(reinterpret_cast<unsigned long long *>(packs + (size_t)a * RG_ALBUMS_PACK_STRIDE + RG_HISTOGRAM_SIZE),
                              peak_bits[t]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// rg_album_result_kernel for packs [first, first + gridDim.x): one workgroup per finished album, the same percentile
// (rg_block_loudness) and the same tail (PINK_REF - loudness, rounded steps).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RG_PCT_THREADS)
rg_album_results_kernel(const uint32_t *__restrict__ packs, uint32_t first, rg_album_result *__restrict__ out) {
    __shared__ uint64_t scan[RG_PCT_THREADS];
    const uint32_t *p = packs + (size_t)(first + blockIdx.x) * RG_ALBUMS_PACK_STRIDE;
    const RgLoudness l = rg_block_loudness(p, scan);
    if (threadIdx.x == 0) {
        rg_album_result r;
        r.album_loudness_db = l.loudness_db;
        r.album_gain_db = RG_PINK_REF - l.loudness_db;
        r.album_peak = __longlong_as_double(*reinterpret_cast<const long long *>(p + RG_HISTOGRAM_SIZE));
        r.album_gain_steps = rg_round_steps(r.album_gain_db);
        r.windows = (uint32_t)l.total;
        out[blockIdx.x] = r;
    }
}

extern "C" hipError_t rg_launch_album_fold(const uint32_t *d_hist, const unsigned long long *d_peak_bits, const int32_t *d_album_of,
                                           uint32_t n_tracks, uint32_t *d_packs, hipStream_t s) {
    if (n_tracks == 0) return hipSuccess;
    const uint32_t runs = (n_tracks + RG_ALBUMS_FOLD_TRACKS - 1) / RG_ALBUMS_FOLD_TRACKS;
    const int nb = (RG_HISTOGRAM_SIZE + 255) / 256;
    hipLaunchKernelGGL(rg_album_fold_kernel, dim3(nb + 1, runs < 4096 ? runs : 4096), dim3(256), 0, s, d_hist, d_peak_bits,
                       d_album_of, n_tracks, d_packs);
    return hipGetLastError();
}

extern "C" hipError_t rg_launch_album_results(const uint32_t *d_packs, uint32_t first, uint32_t count, rg_album_result *d_out,
                                              hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rg_album_results_kernel, dim3(count), dim3(RG_PCT_THREADS), 0, s, d_packs, first, d_out);
    return hipGetLastError();
}
