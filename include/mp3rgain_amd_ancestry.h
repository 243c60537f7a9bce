/* mp3rgain_amd_ancestry.h -- lossy ancestry scan on the GPU: is this "lossless" PCM a decoded MPEG Layer III stream?
 *
 * Decoded MP3 audio, put through the encoder's own hybrid filterbank (32-band polyphase analysis, a 36-point MDCT per
 * subband, the alias butterflies) ON THE STREAM'S GRANULE GRID, falls back onto the values the encoder quantised its lines
 * to, many of them exactly 0.  One sample off the grid nothing shows.  The grid of a file in a FLAC or WAV container is
 * unknown, so all 576 alignments are tried, per view, from the planes the file route has put into the analysis arena: one
 * decode, on the device, and only a fixed-size record per file comes back.
 *
 * THE VERDICT IS A CONVENTION OF THIS PROJECT.  It was tried on streams from this tree's own encoder (oracle/mp3_encoder.py)
 * only, and NOTHING HERE WAS HELD TO ANOTHER ANCESTRY CHECKER.
 *
 * DEFINITIONS (the contract).  All sample arithmetic is IEEE binary32 in the order given, every "fma" one rounding.
 *
 * Sample values y[n], in 16-bit LSB units:
 *   RG_FMT_S16_PLANAR  (float)v
 *   RG_FMT_S32_PLANAR  (float)v * 2^-16 (the container is left-justified)
 *   RG_FMT_F32_PLANAR  x * 32768; a NaN or Inf sample reads as 0 and counts in the channel view's `nonfinite` (counted over
 *                      the whole plane, analysed or not)
 *   An index outside [0, N) reads as 0.
 *
 * Views: every channel is a view (up to 8, kind = the channel's index).  A track of EXACTLY two channels has two more, mid
 * 0.5f * (l + r) (kind 8) and side 0.5f * (l - r) (kind 9): a frame coded mid/side carries its zeros there and not in L or
 * R.  A result holds up to RG_ANC_MAX_VIEWS = 10 view records; `nonfinite` of mid and side is 0.
 *
 * Segments: a segment of G granules begins at frame a, a multiple of 576, and needs L = 576 (G + 2) frames.  With
 * opts.segments = S >= 1 and opts.granules = G >= 1: S is reduced to floor(N / L) when that is smaller (never overlapping),
 * and when even one segment does not fit (N < L) there is one segment at a = 0 with G = floor(N / 576) - 2.  Segment j of S
 * begins at a_j = 576 * floor(j (N - L) / (576 (S - 1))) (a_0 = 0 when S = 1).  S = 0 is the whole plane as one segment:
 * a = 0, G = floor(N / 576) - 2.  A plane of fewer than 3 * 576 frames has no segment: RG_ANC_SHORT and zero counts.  The
 * record carries the S and G that were used.
 *
 * Analysis at alignment r (0 <= r < 576) of a segment at a.  Granule g (0 <= g <= G) has as its 576 samples
 * y[a + r + 576 g .. a + r + 576 g + 575]; granule 0 is only the MDCT's history of granule 1, and lines are counted for
 * 1 <= g <= G.  Slot t (0 <= t < 18) of granule g has the newest sample at e = a + r + 576 g + 32 t + 31 and X[i] = y[e - i],
 * 0 <= i < 512, so the first slot reads 480 samples of history before its granule, before frame 0 zeros.
 *   windowing   Y[j] = fma chain over m = 0 .. 7 (ascending, from 0) of C[j + 64 m] * X[j + 64 m], 0 <= j < 64, where
 *               C = D / 32 and D is the standard's synthesis window (exact in binary32)
 *   matrixing   S[k] = fma chain over j = 0 .. 63 of M[k][j] * Y[j], M[k][j] = (float)cos((2k + 1)(j - 16) pi / 64)
 *   inversion   odd time slots of odd subbands are negated
 *   MDCT        with Z[i], 0 <= i < 36, the 18 slots of granule g - 1 and then those of g, of subband k:
 *               x[18 k + l] = fma chain over i = 0 .. 35 of W[l][i] * Z[i],
 *               W[l][i] = (float)(cos(pi / 72 (2i + 19)(2l + 1)) * sin(pi / 36 (i + 0.5)) / 9): the long window, scaled as
 *               this tree's encoder scales it
 *   butterflies for subband k = 1 .. 31 and i = 0 .. 7, with a = x[18 k - 1 - i], b = x[18 k + i], cs_i = 1 / sqrt(1 + c_i^2),
 *               ca_i = c_i / sqrt(1 + c_i^2) (the standard's c_i, rounded to binary32 from double):
 *               x[18 k - 1 - i] = fma(b, ca_i, a * cs_i), x[18 k + i] = fma(-a, ca_i, b * cs_i): the encoder's direction
 * ONLY THE LONG WINDOW IS TRIED.  Granules coded with short blocks (and start / stop windows) contribute nothing and dilute
 * the count.
 *
 * Statistic, per view and alignment: the 576 lines fall into 48 groups of 12 consecutive lines.  For a group,
 *   q  = fma chain over its 12 lines, ascending, from 0, of c * c;   ms = q * (float)(1.0 / 12)
 * The group is ACTIVE when ms >= active_floor; then its 12 lines count in active[r], and each line with
 * 256.0f * (c * c) < ms (theta = 1/16) counts in small[r].  Both are exact 64-bit counts, summed over the granules and
 * segments, and the same on every route, byte for byte.
 *
 * active_floor (0 = the default RG_ANC_ACTIVE_FLOOR): 16 times the line variance that the rounding of 16-bit PCM alone
 * produces.  Rounding noise is white with variance 1/12 LSB^2; the mean over the 576 lines of the squared norm of the
 * analysis functional (windowing, matrixing, MDCT; the butterflies are rotations and leave the mean alone) is, computed in
 * float64, 0.0034722238 = 1/288; so the line variance is 1 / (12 * 288) and the floor 16 / 3456 = 1/216 = 0.00462963.
 *
 * Per view, from the counts, in integers and doubles on the host (one function for every route):
 *   r*      maximises small[r] / active[r] among the alignments with active[r] >= 1, compared by cross-multiplication in
 *           128-bit integers; ties go to the lowest r
 *   ratio   small[r*] / active[r*];  second = the largest ratio of any other alignment with active >= 1, else 0
 *   p0      the pooled ratio of all other alignments: (sum small - small[r*]) / (sum active - active[r*]), 0 when that
 *           denominator is 0
 *   z       (small* - p0 active*) / sqrt(p0 (1 - p0) active*), 0 when the square root's argument is not positive
 *   iso     ratio / second; when second is 0: +infinity if ratio > 0, else 0
 *   The view is FLAGGED when z >= z_min and iso >= iso_min.  A view with no active group has zeros everywhere.
 * z alone is not enough: tonal and periodic material is not binomial and reaches a large z at many neighbouring alignments;
 * at a true grid the neighbours are back at the baseline, which is what iso asks.
 *
 * Per track: RG_ANC_MP3_GRID when any view is flagged; grid_offset is the r* of the flagged view with the largest z (ties:
 * the first view), `z` and `iso` are that view's, `best_view` its index; RG_ANC_MIDSIDE when that view is mid or side.
 * Without a flagged view grid_offset, z, iso are 0 and best_view is RG_ANC_NO_VIEW.  A file that is a decoded MP3 of 1057
 * samples of codec delay, untrimmed, has grid_offset 481; with k leading samples trimmed, (481 - k) mod 576.
 *
 * Defaults of z_min and iso_min (0 = the default): tools/ancestry_refcheck.py --record runs a float64 reference over the
 * case list of tests/ancestry_cases.py and records in tests/golden/ancestry_measured.json the largest z and iso of any
 * never-coded case and the smallest of any coded case that is expected to be found; each default is the geometric mean of
 * its two sides.  Recorded (3 segments of 3 granules per case, 16-bit and float input):
 *   never coded   white and pink noise, a music-like signal (mono, stereo, padded to 24 bits, floats with NaN and Inf), two
 *                 tones, a 300 Hz square wave, a sweep, a clipped sine, silence: largest z 7.3931 (the two tones), largest
 *                 iso 1.0559 (the stereo music-like signal)
 *   coded, found  the short cut at 47 % and 20 % of the lines sent to 0; streams of 64 and 128 kb/s, mono, left/right and
 *                 mid/side, with and without short blocks, as floats and rounded to 16 bits, 0 to 2000 samples trimmed; a
 *                 mid/side stream of 320 kb/s (its weak side channel falls to 0 at any bitrate): smallest z 48.8816 (the
 *                 short cut at 20 %), smallest iso 2.6564 (64 kb/s left/right)
 *   RG_ANC_Z_MIN = sqrt(7.3931 * 48.8816) = 19.01, RG_ANC_ISO_MIN = sqrt(1.0559 * 2.6564) = 1.675.  The two sides do not
 *   overlap for any case of the list.
 *   KNOWN MISSES, by design and in the list as such: the short cut at 3 % of the lines sent to 0 (z 3.3) and a mono stream of
 *   320 kb/s (z 3.3) read like never-coded audio.
 * The z of a grid grows with the square root of the lines analysed, so the defaults (16 segments of 32 granules, 57 times the
 * lines of the recorded cases) leave far more room on the coded side; tonal never-coded material grows too, which is why iso
 * is asked as well.
 *
 * flags:
 *   RG_ANC_COMPLETE   dropped_frames == 0
 *   RG_ANC_MP3_GRID   some view is flagged
 *   RG_ANC_MIDSIDE    the view that gave grid_offset is mid or side
 *   RG_ANC_NONFINITE  some channel has nonfinite > 0
 *   RG_ANC_SHORT      N < 3 * 576: nothing was analysed
 *   RG_ANC_SILENT     no view has an active group at any alignment
 *
 * WHAT THE SCAN DOES NOT FIND: streams coded so finely that few lines quantise to 0 (a lattice fit on the non-zero lines
 * would; it is not here); passages coded with short blocks; AAC, Vorbis, Opus or any other codec's ancestry; audio that was
 * resampled, re-dithered, scaled or otherwise processed after decoding.  "No grid found" is no proof of lossless origin.
 *
 * Not here: the node and multi-GPU calls, the short-window transform, other codecs' grids, tagging files with the verdict.
 */
#ifndef MP3RGAIN_AMD_ANCESTRY_H
#define MP3RGAIN_AMD_ANCESTRY_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_ANC_COMPLETE   1u
#define RG_ANC_MP3_GRID   2u
#define RG_ANC_MIDSIDE    4u
#define RG_ANC_NONFINITE  8u
#define RG_ANC_SHORT      16u
#define RG_ANC_SILENT     32u
#define RG_ANC_MAX_CHANNELS 8u
#define RG_ANC_MAX_VIEWS 10u
#define RG_ANC_ALIGNMENTS 576u
#define RG_ANC_VIEW_MID 8u
#define RG_ANC_VIEW_SIDE 9u
#define RG_ANC_NO_VIEW 0xFFFFFFFFu
#define RG_ANC_SEGMENTS 16u                 /* the defaults of rg_ancestry_opts (what NULL means) */
#define RG_ANC_GRANULES 32u
#define RG_ANC_ACTIVE_FLOOR 0.00462963f     /* 1/216, see above */
#define RG_ANC_Z_MIN 19.01                  /* sqrt(7.3931 * 48.8816), see above */
#define RG_ANC_ISO_MIN 1.675                /* sqrt(1.0559 * 2.6564) */

typedef struct rg_ancestry_opts {
    uint32_t segments;   /* S; 0 = the whole plane as one segment */
    uint32_t granules;   /* G >= 1 (ignored when segments is 0) */
    double z_min;        /* 0 = RG_ANC_Z_MIN; otherwise positive and finite */
    double iso_min;      /* 0 = RG_ANC_ISO_MIN; otherwise positive and finite */
    float active_floor;  /* 0 = RG_ANC_ACTIVE_FLOOR; otherwise positive and finite */
    uint32_t reserved;   /* 0 */
} rg_ancestry_opts;      /* 32 bytes */

typedef struct rg_ancestry_view {
    double ratio, second, p0, z, iso;
    uint64_t small, active;       /* the counts at r*                                     */
    uint64_t active_total;        /* the sum of active[r] over all alignments             */
    uint32_t offset;              /* r*                                                   */
    uint32_t kind;                /* the channel's index, RG_ANC_VIEW_MID or _SIDE        */
    uint32_t flagged;             /* 1 when z >= z_min and iso >= iso_min                 */
    uint32_t nonfinite;
} rg_ancestry_view; /* 5 * 8 + 3 * 8 + 4 * 4 = 80 bytes */

typedef struct rg_ancestry_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel of the track                                    */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;         /* rg_sample_format of the planes                                            */
    uint32_t dropped_frames; /* frames the decode route dropped, as the rip and verify records count them */
    uint32_t views;          /* view[0 .. views) are filled, the others zero                              */
    uint32_t grid_offset;
    uint32_t segments;       /* S and G as they were used                                                 */
    uint32_t granules;
    uint32_t best_view;      /* the view that gave grid_offset, or RG_ANC_NO_VIEW                         */
    uint32_t reserved;
    double z, iso;           /* of that view                                                              */
    rg_ancestry_view view[RG_ANC_MAX_VIEWS];
} rg_ancestry_result;        /* 72 + 10 * 80 = 872 bytes */

/* The files are decoded by the very route rg_pcm_stats uses -- the same loaders, the same groups (tuning key 13) for lists
 * larger than the device, the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0); no decoder command is
 * run -- and analysed where the PCM lies, in the analysis arena, by the kernels of rg_ancestry.hip on the stream the decode
 * ran on.  RIFF/WAVE of 8, 16, 24 and 32-bit integer and 32-bit float samples, native FLAC, and MPEG Layer III (as f32: an
 * .mp3 is flagged at 481) take part.  opts: NULL = the defaults.  A failing file fails alone: RG_ERR_IO, RG_ERR_FORMAT (not
 * such a stream, more than 8 channels), its record zero apart from `status`.  A file with dropped frames gets the numbers of
 * what the route decoded, with dropped_frames set and RG_ANC_COMPLETE clear.  RG_OK whenever the call itself worked.  `out`
 * is byte for byte the same for tuning key 14 = 1 and 0. */
int rg_ancestry(rg_ctx *ctx, const char *const *paths, size_t n, const rg_ancestry_opts *opts, rg_ancestry_result *out);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_ANC_COMPLETE set.
 *   route 0  the serial host twin: the definitions above, alignment by alignment; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' cutting (phases and granule tiles) run on the host; `ctx` may be NULL
 * counts: NULL, or n * RG_ANC_MAX_VIEWS * 2 * 576 uint64_t: for track i and view v, small[576] and then active[576] at
 * counts + ((i * RG_ANC_MAX_VIEWS + v) * 2) * 576; views a track does not have are zero.
 * RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not sample-aligned, for granules = 0 with
 * segments >= 1, for a negative or non-finite z_min, iso_min or active_floor, and for a non-zero `reserved`.  With a NULL
 * ctx the error text is rg_last_error(NULL)'s. */
int rg_ancestry_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_ancestry_opts *opts, const void *arena,
                      size_t arena_bytes, rg_ancestry_result *out, uint64_t *counts);

/* Test seam: how the kernels cut the work.  phases: polyphase phases per (view, segment), r mod 32, one workgroup each per
 * tile; tile_granules: granules of one workgroup's tile (a segment's last tile may be shorter); lanes: lanes of a workgroup;
 * lds_bytes: LDS of a workgroup.  Any pointer may be NULL. */
int rg_ancestry_kernel_shape(uint32_t *phases, uint32_t *tile_granules, uint32_t *lanes, uint32_t *lds_bytes);

/* Measurement hook (tools/ancestry_rate.py): `n` tracks of `frames` frames of 2 channels of 16-bit PCM at 44.1 kHz, filled on
 * the device, each at its own offset of one device arena, scanned with `opts` (NULL = the defaults).  After a warm-up of
 * `warm_ms` milliseconds of launches, `reps` rounds of the kernels over all tracks (kernel_ms[r], HIP events around the
 * launches alone), then the serial host twin over a host copy of the first `host_tracks` (<= n) tracks on `threads` host
 * threads (host_ms[r]).  *mismatches: host views whose counts differ from the kernels' (it must be 0).  *fma_per_sample: the
 * fused multiply-adds the kernels execute per sample of a view, counted from the tile structure.  `ctx` is an rg_ctx. */
int rg_ancestry_rate(void *ctx, size_t n, uint64_t frames, const rg_ancestry_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                     double warm_ms, double *kernel_ms, double *host_ms, size_t *mismatches, double *fma_per_sample);

#ifdef __cplusplus
}
#endif
#endif
