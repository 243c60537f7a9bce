/* mp3rgain_amd_stats.h -- PCM defect scan on the GPU: per channel the clipped samples and clip runs, runs of digital silence
 * inside the audio (dropouts), the DC sum, the bits that are really used, and the digital silence at the edges, from the
 * planes the file route has put into the analysis arena -- one decode, on the device, one more read of every sample, and only
 * a fixed-size record per file comes back.
 *
 * rg_flac_verify, rg_mp3_verify and rg_rip_checksums answer "is this the audio that was encoded or ripped".  These numbers
 * answer "is the audio itself damaged": what `sox stats`, `ffmpeg astats` and mastering QC tools report.
 *
 * DEFINITIONS (the contract).  A plane is one channel of one track: N samples s_0 .. s_{N-1}, N < 2^32, in one of the three
 * arena formats.  For the integer formats W is 16 (RG_FMT_S16_PLANAR) or 32 (RG_FMT_S32_PLANAR), and `bits` = b is given per
 * track, 1 <= b <= W: the samples are left-justified in the container, as the WAV and FLAC routes stage them (the file route
 * passes the WAV's bits per sample or the FLAC stream's).  For RG_FMT_F32_PLANAR `bits` is ignored and reported as 0.
 *
 * Sample class and zero test
 *   integer  v_k is the stored value.  P = (2^(b-1) - 1) * 2^(W-b), M = -2^(W-1).  class(k) = +1 when v_k >= P, -1 when
 *            v_k <= M, otherwise 0.
 *   float    x_k.  A NaN or Inf sample counts in `nonfinite` and has class 0; it is not zero and takes no part in min, max or
 *            sum.  class = +1 when x >= 1.0, -1 when x <= -1.0, otherwise 0.
 *   zero(k)  v_k == 0; for float x_k == 0.0, either sign.
 *
 * Per plane (rg_pcm_stats_channel)
 *   min, max          over the stored values (the finite ones for float), exact; both 0 when nothing takes part (a zero is
 *                     always +0.0)
 *   sum               integer: the sum of v_k.  Float: the sum of q_k = llrint(clamp(x_k, -256, 256) * 2^23), round half to
 *                     even: the product is exact in double, so q is well defined and the sum independent of order.
 *                     |sum| < 2^63 always.  The DC offset is sum / N / 2^(W-1) for integers and sum / N / 2^23 for float.
 *   or_mask           the OR of the samples' W-bit patterns, zero-extended; float gives 0
 *   effective_bits    0 when or_mask is 0, else W - ctz(or_mask)
 *   clipped           the number of samples with class != 0
 *   clip stretches    a clip stretch is a maximal run of consecutive samples with the same non-zero class; +FS followed by -FS
 *                     is two stretches.  clip_runs: the stretches of length >= min_clip_run.  longest_clip_run: the longest
 *                     stretch of any length, 0 when there is none.  first_clip_run: the index of the first sample of the first
 *                     counted stretch, N when there is none.
 *   zeros             the number of zero samples
 *   zero stretches    a zero stretch is a maximal run of zero samples.  lead_zeros: the length of the stretch that starts at
 *                     sample 0 (0 when s_0 != 0); trail_zeros: of the one that ends at sample N - 1; an all-zero plane gives N
 *                     for both.  zero_runs: the stretches that touch neither end and are at least min_zero_run long;
 *                     longest_zero_run: the longest stretch that touches neither end.
 *   nonfinite         the number of non-finite samples; integer formats give 0
 *
 * Options: rg_pcm_stats_opts {min_clip_run, min_zero_run}, both >= 1; NULL means {3, 64} (RG_STATS_MIN_CLIP_RUN,
 * RG_STATS_MIN_ZERO_RUN).  THE DEFAULTS ARE A CONVENTION OF THIS HEADER: three equal full-scale samples are rarely music, and
 * 64 zero samples are 1.5 ms at 44.1 kHz.  NOBODY MEASURED THEM AGAINST ANOTHER TOOL.
 *
 * Per track (rg_pcm_stats_result): lead_silence_frames = the minimum over the channels of lead_zeros, trail_silence_frames
 * likewise -- exactly the frames at the edge in which every channel is zero.  flags:
 *   RG_STATS_CLIPPED    some channel has clip_runs > 0
 *   RG_STATS_DROPOUT    some channel has zero_runs > 0
 *   RG_STATS_PADDED     integer format, some or_mask != 0, and the largest effective_bits of the channels < bits
 *   RG_STATS_NONFINITE  some channel has nonfinite > 0
 *   RG_STATS_SILENT     every sample is zero, or N = 0
 *   RG_STATS_COMPLETE   dropped_frames == 0
 *
 * Not here: RMS or loudness (the R 128 path has LUFS, loudness range and true peak; the per-block RMS, the peaks and the DR value
 * are rg_dynamic_range, mp3rgain_amd_dr.h), the node and multi-GPU calls.  Spectral detection of lossy transcodes
 * and upsampled files is rg_spectrum (mp3rgain_amd_spectrum.h).  Clicks and glitches -- neither full-scale nor zero -- are
 * rg_clicks (mp3rgain_amd_clicks.h).
 * Nothing is written to files.
 */
#ifndef MP3RGAIN_AMD_STATS_H
#define MP3RGAIN_AMD_STATS_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_STATS_CLIPPED    1u
#define RG_STATS_DROPOUT    2u
#define RG_STATS_PADDED     4u
#define RG_STATS_NONFINITE  8u
#define RG_STATS_SILENT    16u
#define RG_STATS_COMPLETE  32u
#define RG_STATS_MAX_CHANNELS 8u
#define RG_STATS_MIN_CLIP_RUN 3u  /* the defaults of rg_pcm_stats_opts: see above */
#define RG_STATS_MIN_ZERO_RUN 64u

typedef struct rg_pcm_stats_opts {
    uint32_t min_clip_run, min_zero_run; /* both >= 1 */
} rg_pcm_stats_opts;

typedef struct rg_pcm_stats_channel {
    double min, max;
    int64_t sum;
    uint32_t or_mask, effective_bits;
    uint32_t clipped, clip_runs, longest_clip_run, first_clip_run;
    uint32_t zeros, lead_zeros, trail_zeros, zero_runs, longest_zero_run;
    uint32_t nonfinite;
} rg_pcm_stats_channel; /* 72 bytes */

typedef struct rg_pcm_stats_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel that were scanned                              */
    uint32_t sample_rate;
    uint32_t channels;       /* ch[0 .. channels) are filled, the others zero                            */
    uint32_t format;         /* rg_sample_format of the planes                                           */
    uint32_t bits;           /* b; 0 for float                                                           */
    uint32_t dropped_frames; /* frames the decode route dropped, as the rip and verify records count them */
    uint32_t lead_silence_frames, trail_silence_frames;
    uint32_t reserved;
    rg_pcm_stats_channel ch[RG_STATS_MAX_CHANNELS];
} rg_pcm_stats_result;       /* 48 + 8 * 72 = 624 bytes */

/* The files are decoded by the very route the analysis uses -- the same loaders, the same groups (tuning key 13) for lists
 * larger than the device, the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0); no decoder command is
 * run -- and scanned where the PCM lies, in the analysis arena, by two kernels on the stream the decode ran on.  Every input
 * the library decodes itself takes part: RIFF/WAVE of 8, 16, 24 and 32-bit integer and 32-bit float samples, native FLAC, and
 * MPEG Layer III (as f32, so a stream that decodes beyond +-1.0 shows as clipped).  opts: NULL = the defaults.  A failing file
 * fails alone: RG_ERR_IO (it cannot be opened), RG_ERR_FORMAT (not such a stream, or more than 8 channels), its record zero
 * apart from `status`.  A file with dropped frames gets the numbers of what the route decoded, with dropped_frames set and
 * RG_STATS_COMPLETE clear.  RG_OK whenever the call itself worked.  `out` is byte for byte the same for tuning key 14 = 1 and
 * 14 = 0. */
int rg_pcm_stats(rg_ctx *ctx, const char *const *paths, size_t n, const rg_pcm_stats_opts *opts, rg_pcm_stats_result *out);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT), bits[i] = b of track i (ignored for float; bits = NULL means b = W everywhere).
 * out[i].dropped_frames is 0 and RG_STATS_COMPLETE set.
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' chunking and fold arithmetic run on the host; `ctx` may be NULL
 * A track needs only sample alignment.  RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not
 * sample-aligned, for bits outside 1 .. W, and for an option that is 0.  With a NULL ctx the error text is
 * rg_last_error(NULL)'s. */
int rg_pcm_stats_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bits, const rg_pcm_stats_opts *opts,
                       const void *arena, size_t arena_bytes, rg_pcm_stats_result *out);

/* Test seam: how the kernels cut a plane.  chunk_samples: samples one lane walks; tile_samples: samples of one block of the
 * tile kernel (chunks and tiles are counted from the plane's first sample, so only the last of each is short); fold_lanes:
 * lanes of the fold kernel, each folding a run of ceil(tiles / fold_lanes) tile records.  Any pointer may be NULL. */
int rg_pcm_stats_kernel_shape(uint32_t *chunk_samples, uint32_t *tile_samples, uint32_t *fold_lanes);

/* Measurement hook (tools/pcm_stats_rate.py): `n` tracks of `frames` frames of 2 channels of `format` (bits = the container's
 * width), filled on the device, each at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of
 * launches, `reps` rounds of: the two stats kernels over all planes (stats_ms[r], HIP events around the launches), with
 * (any_test = 1) or without (0) the any-test in front of a lane's stretch bookkeeping; then, when rip_ms is not NULL (S16
 * only), the two rip CRC kernels over the same arena (rip_ms[r]); then the serial host twin over a host copy of the first
 * `host_tracks` (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host records that differ from the
 * kernels' (it must be 0).  `ctx` is an rg_ctx. */
int rg_pcm_stats_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, int any_test, size_t host_tracks, uint32_t threads, uint32_t reps,
                      double warm_ms, double *stats_ms, double *rip_ms, double *host_ms, size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
