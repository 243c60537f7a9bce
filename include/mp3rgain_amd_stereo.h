/* mp3rgain_amd_stereo.h -- the stereo image of a file on the GPU: how channels 0 and 1 relate.  Whether they are the same samples
 * (dual mono), one the negated other, nearly mono, lopsided, or the same signal a few samples apart -- from the planes the file
 * route has put into the analysis arena: one decode, on the device, one more read of every sample for the moments and a
 * cross-correlation at every lag within a radius, and only a fixed-size record per file comes back.
 *
 * THE DEFINITIONS BELOW ARE A CONVENTION OF THIS PROJECT.  They were tried on synthetic material only and are held to no other
 * tool: nobody here has compared a correlation, a balance or a delay of this header with a correlation meter, a DAW or a rip
 * checker.
 *
 * DEFINITIONS (the contract).  A track takes part with its channels 0 and 1, L and R: N < 2^32 frames in one of the three arena
 * formats.  A track of one channel is RG_OK with RG_ST_MONO set and every number zero; of a track with more than two channels,
 * channels 0 and 1 are measured and RG_ST_MORE_CHANNELS is set.
 *
 * Reduced sample q, a 16-bit integer; every sum below is a sum over q.
 *   RG_FMT_S16_PLANAR  q = v.
 *   RG_FMT_S32_PLANAR  q = v >> 16, an arithmetic shift (floor).
 *   RG_FMT_F32_PLANAR  a NaN or Inf sample has q = 0 and counts in `nonfinite` (per sample, both channels into one count).
 *                      Otherwise q = min(rintf(clamp(x, -1, 1) * 32768), 32767), round half to even; the product is exact in float.
 *
 * Raw comparisons use the stored values, not q.
 *   integer frames  equal: v_L == v_R.  opposite: v_L + v_R == 0 in 64 bits and v_L != 0.  zero: both are 0.
 *   float frames    equal: x_L == x_R (-0 equals +0, a NaN never equals).  opposite: x_L == -x_R and x_L != 0.  zero: both are 0.
 *   equal_frames, opposite_frames, zero_frames: the counts over the track.
 *
 * Blocks: B = opts.block_frames when that is non-zero, otherwise sample_rate (1 s); 1 <= B <= RG_ST_MAX_BLOCK_FRAMES.  Block b is
 * frames [bB, min((b+1)B, N)); a non-empty remainder is a last block of its own.  Per block, exact int64: ELL_b = sum q_L^2,
 * ERR_b = sum q_R^2, ELR_b = sum q_L q_R, and the block's count of equal frames.  |q| <= 2^15 and N < 2^32, so every sum stays
 * below 2^62 in magnitude.  Per track
 *   ell, err, elr   the sums of the blocks'
 *   blocks          ceil(N / B)
 *   active_blocks   blocks with ELL_b + ERR_b > 0
 *   neg_blocks      blocks with ELR_b < 0
 *   mono_blocks     active blocks in which every frame is equal
 *
 * Lags: R = opts.radius, 0 .. RG_ST_MAX_RADIUS.  For d = -R .. R, C_d = sum of q_L[n] * q_R[n+d] over the n with 0 <= n < N and
 * 0 <= n+d < N, an exact int64; a lag beyond the track sums nothing and is 0.  C_0 == elr.
 *   lag, lag_sum        the d with the largest C_d and that C_d; ties go to the smaller |d|, then to the negative d.  A positive
 *                       lag means the right channel is late.
 *   anti_lag, anti_sum  the d with the smallest C_d, under the same tie rule, and that C_d.
 *
 * The finish is host arithmetic in double on those exact integers, one function for every route.
 *   correlation       elr / (sqrt(ell) * sqrt(err)); 0 WHEN ell OR err IS 0 (one silent channel correlates with nothing)
 *   lag_correlation   lag_sum / (sqrt(ell) * sqrt(err)), anti_correlation the same with anti_sum; 0 when ell or err is 0
 *   balance_db        10 * log10(ell / err): -INFINITY when ell is 0 and err is not (all right), +INFINITY when err is 0 and ell
 *                     is not (all left), 0 when both are 0
 *   side_db           10 * log10(ESS / EMM) with EMM = ell + err + 2 elr and ESS = ell + err - 2 elr, formed exactly (they need
 *                     65 bits) and rounded to double once each: -INFINITY when ESS is 0 and EMM is not (no side signal),
 *                     +INFINITY when EMM is 0 and ESS is not (the mono sum cancels), 0 when both are 0
 *
 * Options: rg_stereo_opts; NULL means RG_ST_DEFAULT_*.  phase_permille and delay_permille are 1 .. 1000, mono_db and
 * balance_db_limit 1 .. 1000.
 *
 * flags:
 *   RG_ST_COMPLETE       dropped_frames == 0
 *   RG_ST_SILENT         ell + err == 0
 *   RG_ST_NONFINITE      nonfinite > 0
 *   RG_ST_DUAL_MONO      N > 0 and equal_frames == N
 *   RG_ST_INVERTED_COPY  opposite_frames > 0 and opposite_frames + zero_frames == N
 *   RG_ST_OUT_OF_PHASE   correlation <= -phase_permille / 1000
 *   RG_ST_NEAR_MONO      not dual mono, and side_db <= -mono_db
 *   RG_ST_ONE_SIDED      |balance_db| >= balance_db_limit, or exactly one of ell and err is 0
 *   RG_ST_DELAYED        lag != 0, lag_sum > C_0 and lag_correlation >= delay_permille / 1000
 *   RG_ST_MONO           the track has one channel: nothing was measured
 *   RG_ST_MORE_CHANNELS  the track has more than two channels: channels 0 and 1 were measured
 *
 * The thresholds.  mono_db (40) and balance_db_limit (12) are stated conventions.  delay_permille and phase_permille are measured
 * by tools/stereo_refcheck.py on the serial host twin over synthetic material at radius 64 and recorded in
 * tests/golden/stereo_measured.json; each default is the geometric mean of its two sides.
 *   delay_permille 420  Never delayed (rg_synth.h tracks with independent channels, panned tones, two-tone mixes, partly
 *                       correlated mixes, and inverted copies): the largest lag_correlation of a file whose best lag is not 0 is
 *                       0.181 (an inverted copy of material with a 440 Hz tone, which correlates half a period off; independent
 *                       channels of 3 s reach 0.034).  Delayed by +-1, +-2, +-17, +-64 frames, as 16-bit, as float, re-dithered
 *                       to 16 bits and after the project's own MP3 encoder at 128 and 320 kb/s: the smallest is 0.973 (128 kb/s,
 *                       d = -64), and every one of them reads lag == d.  A panned tone correlates at 0.9999 one frame off and
 *                       better in place: the condition lag_sum > C_0 is what keeps it unflagged, not the threshold.
 *   phase_permille 587  Never inverted: the lowest correlation is -0.344, of a mix whose side is 3 dB above its mid (a wide mix,
 *                       not a fault).  Inverted copies through the same five treatments: -1.000.
 * The classes separated for every kind of material tried.
 *
 * Not found: a delay beyond the radius; Haas-style delays of tens of milliseconds; frequency-dependent phase (an all-pass between
 * the channels, a polarity flip of one band); anything about channels 2 and up.  Not told apart: an inverted pure tone IS that
 * tone delayed by half its period; such a file reads RG_ST_INVERTED_COPY or RG_ST_OUT_OF_PHASE, and RG_ST_DELAYED only when the
 * shifted sum beats the threshold.  Short files: the chance correlation of independent channels grows as the track shrinks
 * (about 4 / sqrt(N)), so below a few thousand frames RG_ST_DELAYED means little.
 */
#ifndef MP3RGAIN_AMD_STEREO_H
#define MP3RGAIN_AMD_STEREO_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_ST_COMPLETE       1u
#define RG_ST_SILENT         2u
#define RG_ST_NONFINITE      4u
#define RG_ST_DUAL_MONO      8u
#define RG_ST_INVERTED_COPY  16u
#define RG_ST_OUT_OF_PHASE   32u
#define RG_ST_NEAR_MONO      64u
#define RG_ST_ONE_SIDED      128u
#define RG_ST_DELAYED        256u
#define RG_ST_MONO           512u
#define RG_ST_MORE_CHANNELS  1024u
#define RG_ST_MAX_CHANNELS   8u
#define RG_ST_MAX_RADIUS     255u
#define RG_ST_MAX_BLOCK_FRAMES 384000u /* 1 s at 384 kHz */
#define RG_ST_DEFAULT_RADIUS 64u
#define RG_ST_DEFAULT_PHASE_PERMILLE 587u /* measured, see above */
#define RG_ST_DEFAULT_DELAY_PERMILLE 420u /* measured, see above */
#define RG_ST_DEFAULT_MONO_DB 40u
#define RG_ST_DEFAULT_BALANCE_DB 12u

typedef struct rg_stereo_opts {
    uint32_t block_frames;     /* 0 = sample_rate */
    uint32_t radius;           /* 0 .. RG_ST_MAX_RADIUS */
    uint32_t phase_permille;   /* 1 .. 1000 */
    uint32_t delay_permille;   /* 1 .. 1000 */
    uint32_t mono_db;          /* 1 .. 1000 */
    uint32_t balance_db_limit; /* 1 .. 1000 */
} rg_stereo_opts;

typedef struct rg_stereo_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel that were scanned                              */
    uint32_t sample_rate;
    uint32_t channels;       /* of the track; channels 0 and 1 were measured                             */
    uint32_t format;         /* rg_sample_format of the planes                                           */
    uint32_t dropped_frames; /* frames the decode route dropped, as the rip and verify records count them */
    uint32_t block_frames;   /* B */
    uint32_t radius;         /* R */
    uint32_t blocks, active_blocks, neg_blocks, mono_blocks;
    int32_t lag, anti_lag;
    uint64_t equal_frames, opposite_frames, zero_frames, nonfinite;
    int64_t ell, err, elr;       /* exact, the same bits on every route */
    int64_t lag_sum, anti_sum;
    double correlation, lag_correlation, anti_correlation, balance_db, side_db; /* the finish */
} rg_stereo_result;          /* 64 + 32 + 40 + 40 = 176 bytes */

/* The files are decoded by the very route rg_pcm_stats uses -- the same loaders, the same groups (tuning key 13), the device FLAC
 * decoder (tuning key 14 = 1) or the host decoder (key 14 = 0) -- and measured where the PCM lies, in the analysis arena, by the
 * kernels of rg_stereo.hip on the stream the decode ran on.  opts: NULL = the defaults.  lag_sums: NULL, or n rows of
 * 2 * radius + 1 sums, row i the C_d of file i from d = -radius up (zero for a file that takes no part or has one channel); it is
 * filled group by group.  A failing file fails alone: RG_ERR_IO, RG_ERR_FORMAT (not such a stream, more than 8 channels, or a
 * sample rate beyond RG_ST_MAX_BLOCK_FRAMES when the block length comes from it), its record zero apart from `status`.  A file
 * with dropped frames gets the numbers of what the route decoded, with dropped_frames set and RG_ST_COMPLETE clear.  RG_OK
 * whenever the call itself worked.  `out` and `lag_sums` are byte for byte the same for tuning key 14 = 1 and 0. */
int rg_stereo(rg_ctx *ctx, const char *const *paths, size_t n, const rg_stereo_opts *opts, rg_stereo_result *out, int64_t *lag_sums);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_ST_COMPLETE set.  lag_sums as above.
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' cutting and fold arithmetic run on the host; `ctx` may be NULL
 * A track needs only sample alignment.  RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not
 * sample-aligned, for a radius beyond RG_ST_MAX_RADIUS, a threshold outside its range and a block length outside
 * 1 .. RG_ST_MAX_BLOCK_FRAMES (also when it comes from the track's sample rate).  With a NULL ctx the error text is
 * rg_last_error(NULL)'s. */
int rg_stereo_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_stereo_opts *opts, const void *arena, size_t arena_bytes,
                    rg_stereo_result *out, int64_t *lag_sums);

/* Test seam: how the kernels cut a track of `format`.  piece_samples: frames of one workgroup's piece of the moments kernel
 * (pieces are counted from the BLOCK's first frame, so only a block's last piece is short); tile_frames: frames of one workgroup's
 * tile of the lag kernel (tiles are counted from the track's first frame); strip_frames: consecutive frames whose left values a
 * lane holds in registers at a time; lag_group: consecutive lags a lane accumulates; lds_bytes: the lag kernel's LDS.  Any
 * pointer may be NULL.  RG_ERR_FORMAT for a format that is none of the three. */
int rg_stereo_kernel_shape(uint32_t format, uint32_t *piece_samples, uint32_t *tile_frames, uint32_t *strip_frames, uint32_t *lag_group,
                           uint32_t *lds_bytes);

/* Measurement hook (tools/stereo_rate.py): `n` tracks of `frames` frames of 2 channels of `format` at 44.1 kHz, filled on the
 * device with pseudo-random samples, each at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of
 * launches, `reps` rounds of: the moments kernels and the fold over all tracks (moments_ms[r], HIP events around the launches
 * alone); the clearing of the lag sums and the lag kernel at `radius` (lags_ms[r]); then the serial host twin over a host copy of
 * the first `host_tracks` (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host tracks whose raw numbers or lag
 * sums differ from the kernels' (it must be 0).  *bytes: the bytes of PCM one round of a leg reads (the lag kernel reads its
 * margins on top of them).  *macs: the multiply-adds of the definition in one round of the lag leg, frames * (2 radius + 1) per
 * track less the ends.  `ctx` is an rg_ctx.  The DR pair and its read floor over such an arena are rg_dr_rate's, the tempo scan's
 * window kernel is rg_tempo_rate's: the tool calls them in the same process. */
int rg_stereo_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, uint32_t radius, size_t host_tracks, uint32_t threads, uint32_t reps,
                   double warm_ms, double *moments_ms, double *lags_ms, double *host_ms, size_t *mismatches, uint64_t *bytes, uint64_t *macs);

#ifdef __cplusplus
}
#endif
#endif
