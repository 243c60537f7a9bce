// rg_albums.h -- the device side of rg_analyze_albums (rg_albums.hip): live per-album packs, their fold and read-out.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mp3rgain_amd.h"

// words from one live pack to the next: RG_ALBUM_PACK_WORDS rounded up to 16 bytes (the percentile reads 16 bytes at a time)
#define RG_ALBUMS_PACK_STRIDE (((RG_ALBUM_PACK_WORDS) + 3) & ~3)
// tracks one workgroup of the fold walks per bin
#define RG_ALBUMS_FOLD_TRACKS 16

extern "C" {
// packs[album_of[t]] += track t's [histogram | peak] (sum of bins, max of peak bits), t < n_tracks; album_of[t] < 0: skipped.
// d_hist: [n_tracks][RG_HISTOGRAM_SIZE], d_peak_bits: [n_tracks] (the layout of a batch's accumulators, rg_ctx.h RgSlot)
hipError_t rg_launch_album_fold(const uint32_t *d_hist, const unsigned long long *d_peak_bits, const int32_t *d_album_of,
                                uint32_t n_tracks, uint32_t *d_packs, hipStream_t s);
// d_out[k] = the album result of pack first + k, k < count
hipError_t rg_launch_album_results(const uint32_t *d_packs, uint32_t first, uint32_t count, rg_album_result *d_out, hipStream_t s);
}
