/* mp3rgain_amd_dr.h -- the dynamic range (DR) value on the GPU: per channel the energy and the peak of every 3-second block,
 * the mean of the loudest fifth of the blocks, the second-highest block peak, and from them the "DR" figure that collectors
 * post next to the rip log -- from the planes the file route has put into the analysis arena: one decode, on the device, one
 * more read of every sample, and only a fixed-size record per file comes back.
 *
 * THE DEFINITIONS BELOW ARE A CONVENTION OF THIS HEADER.  They follow the published description of the TT DR Offline Meter
 * (3-second blocks, RMS with the factor 2, the loudest 20 % of blocks, the second-highest block peak).  NOBODY HERE CAN CHECK
 * THEM AGAINST THE TT METER OR FOOBAR2000: the figure follows the published description and is unverified against either.
 *
 * DEFINITIONS (the contract).  A plane is one channel of one track: N < 2^32 samples in one of the three arena formats.
 *
 * Sample value: every sample becomes an integer q with a scale s.
 *   RG_FMT_S16_PLANAR  q = v, s = 2^15.
 *   RG_FMT_S32_PLANAR  q = v, s = 2^31.  The container is left-justified, so the stream's bits per sample are not needed.
 *   RG_FMT_F32_PLANAR  q = llrint(clamp(x, -256, 256) * 2^23), round half to even, s = 2^23: the quantisation of
 *                      rg_pcm_stats' `sum`.  The product is exact in float, so the device needs no double.  A NaN or Inf
 *                      sample counts in `nonfinite`, has q = 0 and stays in its block's length.
 *
 * Blocks: B = opts.block_frames when that is non-zero, otherwise 3 * sample_rate.  Block i is samples [iB, min((i+1)B, N)); a
 * non-empty remainder is a last block of its own, so blocks = ceil(N / B).  1 <= B <= 1 152 000 (3 s at 384 kHz).
 *
 * Per block i of n_i samples
 *   E_i   the sum of q^2, EXACT (it reaches 2^82: two limbs, never a float sum)
 *   e_i   E_i rounded once to double: (double)(E >> 32) * 2^32 + (double)(E & 0xFFFFFFFF) (both conversions and the product
 *         are exact)
 *   ms_i  2.0 * e_i / ((double)n_i * s^2); s^2 is a power of two, so this is one rounding
 *   p_i   max |q|, an unsigned 32-bit integer
 *
 * Per plane (the raw part of rg_dr_channel)
 *   top_blocks   k = max(1, floor(blocks * top_permille / 1000))
 *   t, g         t = the k-th largest ms_i, with multiplicity; g = the number of blocks with ms_i > t
 *   top_ms       S / k, where S is the double sum of the ms_i > t in ASCENDING BLOCK INDEX, then t added k - g times, one
 *                addition each: no product anywhere in the sum, so no fused multiply-add can make two routes differ
 *   mean_square  2.0 * (the sum of the e_i in ascending block index) / ((double)N * s^2)
 *   peak         max p_i
 *   peak2        the second element of the p_i sorted descending: equal to `peak` when two blocks share the maximum, and the
 *                only element when there is one block
 *   With N = 0 all of them are 0.
 *
 * The finish is host arithmetic on those numbers, one function for every route (log10 is not the same bits on host and device).
 *   per channel  dr = 20 * log10((peak2 / s) / sqrt(top_ms)) when peak2 and top_ms are both positive, else 0
 *                peak_db = 20 * log10(peak / s), rms_db = 10 * log10(mean_square); WHEN THE ARGUMENT IS 0 THE STORED VALUE
 *                IS -INFINITY (silence has no level)
 *   per track    dr_mean = the mean of the channels' dr, all channels (1 to 8) weighing the same; dr = llrint(dr_mean), half
 *                to even; peak_db = the maximum over the channels; rms_db = 10 * log10 of the mean of the channels' mean_square
 *
 * Options: rg_dr_opts {block_frames, top_permille}; NULL means {0, 200}.  top_permille is 1 .. 1000.
 *
 * flags:
 *   RG_DR_COMPLETE   dropped_frames == 0
 *   RG_DR_SILENT     no channel has both a positive top_ms and a positive peak2, or N = 0
 *   RG_DR_NONFINITE  some channel has nonfinite > 0
 *   RG_DR_SHORT      N < B: the figure of a clip shorter than one block is reported, but it is not a DR value
 *
 * Not here: the node and multi-GPU calls, DR tags or log files, a loudness-based PLR figure (the R 128 path has LUFS and true
 * peak).
 */
#ifndef MP3RGAIN_AMD_DR_H
#define MP3RGAIN_AMD_DR_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_DR_COMPLETE   1u
#define RG_DR_SILENT     2u
#define RG_DR_NONFINITE  4u
#define RG_DR_SHORT      8u
#define RG_DR_MAX_CHANNELS 8u
#define RG_DR_TOP_PERMILLE 200u        /* the default of rg_dr_opts.top_permille */
#define RG_DR_MAX_BLOCK_FRAMES 1152000u /* 3 s at 384 kHz */

typedef struct rg_dr_opts {
    uint32_t block_frames; /* 0 = 3 * sample_rate */
    uint32_t top_permille; /* 1 .. 1000 */
} rg_dr_opts;

typedef struct rg_dr_channel {
    double dr, peak_db, rms_db;   /* the finish                                        */
    double top_ms, mean_square;   /* the raw numbers, the same bits on every route     */
    uint32_t peak, peak2;         /* in units of q                                     */
    uint32_t blocks, top_blocks;  /* ceil(N / B) and k                                 */
    uint32_t nonfinite;
    uint32_t reserved;
} rg_dr_channel; /* 5 * 8 + 6 * 4 = 64 bytes */

typedef struct rg_dr_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel that were scanned                              */
    uint32_t sample_rate;
    uint32_t channels;       /* ch[0 .. channels) are filled, the others zero                            */
    uint32_t format;         /* rg_sample_format of the planes                                           */
    uint32_t dropped_frames; /* frames the decode route dropped, as the rip and verify records count them */
    uint32_t block_frames;   /* B                                                                        */
    int32_t dr;              /* llrint(dr_mean)                                                          */
    double dr_mean, peak_db, rms_db;
    rg_dr_channel ch[RG_DR_MAX_CHANNELS];
} rg_dr_result;              /* 64 + 8 * 64 = 576 bytes */

/* The files are decoded by the very route rg_pcm_stats uses -- the same loaders, the same groups (tuning key 13) for lists
 * larger than the device, the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0); no decoder command is
 * run -- and measured where the PCM lies, in the analysis arena, by the kernels of rg_dr.hip on the stream the decode ran on.
 * RIFF/WAVE of 8, 16, 24 and 32-bit integer and 32-bit float samples, native FLAC, and MPEG Layer III (as f32) take part.
 * opts: NULL = the defaults.  A failing file fails alone: RG_ERR_IO (it cannot be opened), RG_ERR_FORMAT (not such a stream,
 * more than 8 channels, or a sample rate whose 3-second block is longer than RG_DR_MAX_BLOCK_FRAMES), its record zero apart
 * from `status`.  A file with dropped frames gets the numbers of what the route decoded, with dropped_frames set and
 * RG_DR_COMPLETE clear.  RG_OK whenever the call itself worked.  `out` is byte for byte the same for tuning key 14 = 1 and 0. */
int rg_dynamic_range(rg_ctx *ctx, const char *const *paths, size_t n, const rg_dr_opts *opts, rg_dr_result *out);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_DR_COMPLETE set.
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' cutting and fold arithmetic run on the host; `ctx` may be NULL
 * A track needs only sample alignment.  RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not
 * sample-aligned, for top_permille outside 1 .. 1000 and for a block length outside 1 .. RG_DR_MAX_BLOCK_FRAMES (also when it
 * comes from the track's sample rate).  With a NULL ctx the error text is rg_last_error(NULL)'s. */
int rg_dr_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_dr_opts *opts, const void *arena, size_t arena_bytes,
                rg_dr_result *out);

/* Test seam: how the kernels cut a block of `format` and a plane.  step_samples: samples of one 16-byte vector, what one lane
 * takes per step; piece_samples: samples of one workgroup's piece (pieces are counted from the BLOCK's first sample, so only a
 * block's last piece is short); fold_lanes: lanes of the fold kernel, lane l folding the pieces of blocks l, l + fold_lanes, ...;
 * select_bins: the counters of one pass of the selection (a radix select on the bit patterns of the ms_i: the blocks stay in
 * device memory, so a plane may hold any number of them).  Any pointer may be NULL.  RG_ERR_FORMAT for a format that is none
 * of the three. */
int rg_dr_kernel_shape(uint32_t format, uint32_t *step_samples, uint32_t *piece_samples, uint32_t *fold_lanes, uint32_t *select_bins);

/* Measurement hook (tools/dr_rate.py): `n` tracks of `frames` frames of 2 channels of `format` at 44.1 kHz, filled on the
 * device, each at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of launches, `reps` rounds
 * of: the DR kernels over all planes (dr_ms[r], HIP events around the launches alone); the two rg_pcm_stats kernels over the
 * same arena (stats_ms[r]); a kernel that only sums the 16-byte words of the same planes, cut as the DR pieces are
 * (floor_ms[r]: the read floor of this access pattern); then the serial host twin over a host copy of the first `host_tracks`
 * (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host plane records that differ from the kernels' (it
 * must be 0).  *bytes: the bytes of PCM one round of a leg reads.  `ctx` is an rg_ctx. */
int rg_dr_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
               double *dr_ms, double *stats_ms, double *floor_ms, double *host_ms, size_t *mismatches, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
