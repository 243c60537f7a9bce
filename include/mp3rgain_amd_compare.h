/* mp3rgain_amd_compare.h -- a null test of two copies of a recording on the GPU: line the copies up to the sample, fit one gain,
 * subtract, and size what is left.  Whether two files are the same samples a few hundred frames apart or padded at the ends, the
 * same master after a gain change and a re-dither, a lossy-coded copy or a different master, and where they differ -- from planes
 * that lie side by side in the analysis arena: a cross-correlation of the two files at every lag within a radius of a hint, one
 * more read of every overlapping sample for the moments, and only a fixed-size record per pair comes back.  The unit of work is a
 * pair of tracks, not a track.
 *
 * THE DEFINITIONS BELOW ARE A CONVENTION OF THIS PROJECT.  No other null-test tool was at hand: nobody here has compared a lag, a
 * gain or a residual of this header with a DAW, an audio-diff tool or a rip checker.
 *
 * DEFINITIONS (the contract; byte for byte the same on every route).
 *
 * Input.  A call has n tracks and n_pairs pairs (a, b, hint): a != b are indices into the tracks and a is the reference copy.  A
 * pair is measured when the sample rates of its two tracks are equal -- otherwise the pair gets RG_CMP_RATE, no numbers and no
 * error -- and each track has fewer than 2^32 frames.  The channels compared are Cc = min(channels_a, channels_b), channel c of
 * the one against channel c of the other, at most RG_CMP_MAX_CHANNELS; RG_CMP_CHANNELS_DIFFER is set when the counts differ.
 * Cc * min(Na, Nb) must be below 2^32 (RG_ERR_FORMAT otherwise), so every total below is an int64 below 2^62.
 *
 * Reduced sample q: exactly the stereo header's (mp3rgain_amd_stereo.h): a 16-bit integer from any of the three arena formats,
 * with the same rounding, clamp and non-finite rule (a NaN or Inf has q = 0 and counts in `nonfinite`).
 *
 * Equality of two samples.  When both tracks have the same format and the polarity is +1 the stored values are compared (integer
 * v_a == v_b; float x_a == x_b, so -0 equals +0 and a NaN never equals) and RG_CMP_RAW is set.  Otherwise -- tracks of different
 * formats, or polarity -1 -- the test is q_a == sigma * q_b.
 *
 * Stage A, the coarse hint h (frames; b[n + h] is expected beside a[n]).  The arena seam takes the pair's `hint` as h.
 *
 * Stage B, the fine lag.  The overlap at the hint is [n0, n1) = [max(0, -h), min(Na, Nb - h)), V = n1 - n0; V <= 0 gives
 * RG_CMP_NO_OVERLAP and nothing more.  S = opts.segments (1 .. 16) segments of G = opts.segment_frames frames; G = 0 or V <= S * G
 * means one segment that is the whole overlap, otherwise segment s starts at n0 + (2s + 1)(V - G) / (2S) (integer division).
 * R = opts.radius, 0 .. RG_CMP_MAX_RADIUS.  For every segment s, channel c and d = -R .. R
 *   C[s][c][d] = sum over the segment's n of qa_c[n] * qb_c[n + h + d], over the n with 0 <= n + h + d < Nb   (an exact int64)
 *   EA[s][c] = sum qa_c[n]^2,  EB[s][c] = sum qb_c[n + h]^2 (the d = 0 window, in range)
 * A lag row is these 2R + 3 numbers: the C from d = -R up, then EA, then EB.
 * The pick is host arithmetic on the rows, one function for every route.  T[d] is the sum over s and c of C[s][c][d], formed in
 * 128 bits.  d* maximises |T[d]|; ties go to the smaller |d|, then to the negative d, whatever the signs of the two sums (the
 * positive T would come next, and two sums at one d cannot tie).  polarity sigma is the sign of T[d*], +1 when it is 0;
 * lag = h + d*.  RG_CMP_AT_EDGE when R > 0 and |d*| == R.  lock = |T[d*]| / sqrt(sum EA * sum EB) in double (each sum rounded
 * once), 0 when either sum is 0; RG_CMP_LOCKED when lock >= lock_permille / 1000.  Per segment the same pick and ratio on that
 * segment's rows alone: locked_segments, and seg_lag_min, seg_lag_max over the locked segments' lags (0 when there is none).
 * RG_CMP_DRIFT when two locked segments' lags differ by more than opts.drift_frames: a resampled or analogue-transferred copy.
 *
 * Stage C, the aligned moments at `lag` and sigma.  The overlap is [m0, m1) = [max(0, -lag), min(Na, Nb - lag)), W = m1 - m0
 * (`overlap`); a_head = m0, a_tail = Na - m1, b_head = m0 + lag, b_tail = Nb - m1 - lag.  Blocks of B frames (opts.block_frames,
 * 0 = sample_rate, 1 .. RG_CMP_MAX_BLOCK_FRAMES) are counted from m0; a non-empty remainder is a block of its own.  Per block,
 * summed over the channels, exact: aa = sum qa^2, bb = sum qb^2, ab = sum qa qb, `equal` the samples that are equal as defined
 * above, max_diff = max |qa - sigma qb|, first_diff the smallest frame index in a at which a sample is not equal (all ones when
 * there is none).  The record's aa, bb, ab, equal, max_diff and first_diff are the blocks' sums, maximum and minimum.
 *
 * The finish is in double on the exact integers, one function for every route, nothing contracted.
 *   gamma           ab / bb, so that a ~ gamma * b; gain_db = 20 log10 |gamma|, 0 when ab or bb is 0
 *   null_unity_db   10 log10((aa - 2 sigma ab + bb) / aa), the numerator formed exactly; -INFINITY when it is 0; 0 when aa is 0
 *   null_db         10 log10((aa bb - ab^2) / (aa bb)), numerator and denominator formed exactly in 128 bits and rounded once
 *                   each; -INFINITY when the numerator is 0; 0 when aa or bb is 0
 *   residual_lsb2   (aa bb - ab^2) / bb / (W Cc) / max(1, gamma^2), aa / (W Cc) when bb is 0: the mean square of what is left, in
 *                   steps of q, referred to the copy that was quantised
 *   differing_blocks  blocks whose `equal` is short of their samples
 *   worst_block, worst_block_db   per block with aa_b > 0 the residual at the pair's gamma is (aa_b - (2 gamma) ab_b) +
 *                   (gamma gamma) bb_b and its level 10 log10(residual / aa_b), -INFINITY when the residual is not positive;
 *                   the block with the highest level, the first of equals; 0 and 0 when no block has aa_b > 0
 *   gain_min_db, gain_max_db   of 20 log10 |ab_b / bb_b| over the blocks with 100 aa_b * blocks >= aa (a hundredth of the mean
 *                   block) and ab_b, bb_b not 0; both 0 when there is none.  A wide spread with a good lock is a different
 *                   master, not a gain change.
 *
 * flags:
 *   RG_CMP_COMPLETE         neither file dropped frames
 *   RG_CMP_IDENTICAL        W > 0, sigma = +1, every overlapping sample equal
 *   RG_CMP_SHIFTED          lag != 0
 *   RG_CMP_LENGTHS          any of the four head and tail counts is not 0
 *   RG_CMP_INVERTED         sigma = -1
 *   RG_CMP_NONFINITE        a non-finite sample in the overlap, on either side
 *   RG_CMP_LOCKED, RG_CMP_AT_EDGE, RG_CMP_DRIFT   stage B, above
 *   RG_CMP_SAME_MASTER      locked, not identical, residual_lsb2 <= requant_millilsb2 / 1000
 *   RG_CMP_DIFFERS          locked, not identical, and above that
 *   RG_CMP_UNRELATED        not locked
 *   RG_CMP_RATE, RG_CMP_NO_OVERLAP   not measured, above
 *   RG_CMP_NO_COARSE        no coarse match was to be had: h = 0 (set by a file route only)
 *   RG_CMP_CHANNELS_DIFFER, RG_CMP_RAW   above
 *
 * Integer bounds.  |q| <= 2^15, so a product is at most 2^30.  A lane of the lag kernel sums at most 4096 products in double:
 * below 2^53, so the double IS the integer.  Every int64 row, block sum and total is below 2^62 (fewer than 2^32 samples).  The
 * sums over channels and segments, aa bb and ab^2 are 128-bit on the host.
 *
 * The two thresholds are measured by tools/compare_refcheck.py on the serial host twin over synthetic material at the defaults
 * (3 s at 44.1 kHz, one channel) and recorded in tests/golden/compare_measured.json; each default is the geometric mean of its two
 * sides.  THIS IS SYNTHETIC MATERIAL AND THE PROJECT'S OWN MP3 ENCODER ONLY; no other null-test tool was at hand.
 *   lock_permille 606         Unrelated pairs: rg_synth.h tracks of different seeds reach a lock of 0.019 (all seeds share the
 *                             generator's steady tones); music-like signals of different seeds that share two tones (440 and
 *                             1318.5 Hz, a third of their power) reach 0.383, which is the side that counts.  Same-recording
 *                             pairs: copies +-1, +-17, +-588 and +-1023 frames from the hint (0.993 at +-1023, where a hundredth
 *                             of the segment has nothing beside it), 16-bit, float and 24-bit copies, -6 dB of gain and an
 *                             inverted copy (1.000), the project's MP3 encoder at 64, 128 and 320 kb/s decoded by this library
 *                             (0.980, 0.997, 1.000; the hint is the codec's delay of 1057 frames), and a remaster made in the
 *                             tool, a +-3 dB shelf and a 2:1 compressor: 0.958, the smallest.  Every one of them read its lag and
 *                             polarity.
 *   requant_millilsb2 18156   Same-master treatments: gains of -6, -3 and +1 dB then rounding to 16 bits (0.17, 0.25, 0.40 LSB^2)
 *                             and with TPDF dither (0.33, 0.41, 0.53); 24 bits to 16 by truncation (0.002: q floors) and by
 *                             dithered rounding (0.58, the largest); float to 16 bits (0.0001).  Everything else that locks: the
 *                             320 kb/s stream 566 LSB^2 (the smallest), 128 kb/s 61 000, 64 kb/s 363 000, the remaster 336 000.
 * The classes separated for every kind of material tried, and nothing was dropped from it.  A threshold of 18 LSB^2 is nearer
 * to the dithers than to the coder in decibels only because the geometric mean is: 15 dB above the one, 15 dB below the other.
 *
 * RATES.  tools/compare_rate.py on an MI355X (profiles/compare_rate.json), 500 pairs out of 1000 device-filled tracks of 3 min of
 * 16-bit stereo, HIP events around the launches alone after a warm-up, medians of 5: the lag kernel at the defaults 117 ms = 18.3 T
 * multiply-adds per second (47 % of the FP64 vector FMA peak, 1.18 times the stereo scan's lag kernel at radius 64 in the same
 * process), at radius 64 14.9 ms = 9.1 T/s; moments and fold 10.6 ms = 3.0 TB/s, half of the read floor over such an arena (the
 * stereo scan's pair: 81 %); float 125 ms, 16.3 ms and 17.3 ms.  The serial twin on 16 threads, scaled: 59 s.  No lag row, block
 * row or total of 32 host pairs differed.
 *
 * Not found: copies at different sample rates (the cross-rate duplicate search finds them; this does not compare them); offsets
 * beyond +-RG_CMP_MAX_RADIUS frames of the hint; drift, which is flagged and not corrected; gain that varies over time (one gamma
 * per pair; gain_min_db and gain_max_db only show that it happened); differences below the 16th bit, which are visible only
 * through `equal` and `first_diff`; anything across more than RG_CMP_MAX_CHANNELS channels or in channels one file lacks;
 * channels in a different order.
 */
#ifndef MP3RGAIN_AMD_COMPARE_H
#define MP3RGAIN_AMD_COMPARE_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_CMP_COMPLETE        (1u << 0)
#define RG_CMP_IDENTICAL       (1u << 1)
#define RG_CMP_SHIFTED         (1u << 2)
#define RG_CMP_LENGTHS         (1u << 3)
#define RG_CMP_INVERTED        (1u << 4)
#define RG_CMP_NONFINITE       (1u << 5)
#define RG_CMP_LOCKED          (1u << 6)
#define RG_CMP_AT_EDGE         (1u << 7)
#define RG_CMP_DRIFT           (1u << 8)
#define RG_CMP_SAME_MASTER     (1u << 9)
#define RG_CMP_DIFFERS         (1u << 10)
#define RG_CMP_UNRELATED       (1u << 11)
#define RG_CMP_RATE            (1u << 12)
#define RG_CMP_NO_OVERLAP      (1u << 13)
#define RG_CMP_NO_COARSE       (1u << 14)
#define RG_CMP_CHANNELS_DIFFER (1u << 15)
#define RG_CMP_RAW             (1u << 16)

#define RG_CMP_ALIGN_FINGERPRINT 0u
#define RG_CMP_ALIGN_HINT        1u
#define RG_CMP_MAX_CHANNELS      8u
#define RG_CMP_MAX_RADIUS        2047u
#define RG_CMP_MAX_COARSE_RADIUS 2047u
#define RG_CMP_MAX_SEGMENTS      16u
#define RG_CMP_MAX_BLOCK_FRAMES  384000u /* 1 s at 384 kHz, the stereo scan's limit */
#define RG_CMP_MAX_HINT          ((int64_t)1 << 32) /* |hint| beyond this is RG_ERR_INVALID_ARG */
#define RG_CMP_DEFAULT_COARSE_RADIUS 512u
#define RG_CMP_DEFAULT_RADIUS        1024u
#define RG_CMP_DEFAULT_SEGMENTS      4u
#define RG_CMP_DEFAULT_SEGMENT_FRAMES 262144u
#define RG_CMP_DEFAULT_DRIFT_FRAMES  1u
#define RG_CMP_DEFAULT_LOCK_PERMILLE 606u        /* measured, see above */
#define RG_CMP_DEFAULT_REQUANT_MILLILSB2 18156u /* measured, see above */

typedef struct rg_compare_pair {
    uint32_t a, b; /* indices into the tracks; a is the reference copy */
    int64_t hint;  /* frames: b[n + hint] is expected beside a[n] */
} rg_compare_pair;  /* 16 bytes */

typedef struct rg_compare_opts {
    uint32_t align;             /* RG_CMP_ALIGN_*; the arena seam takes hints whatever this says */
    uint32_t coarse_radius;     /* 1 .. RG_CMP_MAX_COARSE_RADIUS codes of 512 frames */
    uint32_t radius;            /* R: 0 .. RG_CMP_MAX_RADIUS */
    uint32_t segments;          /* S: 1 .. RG_CMP_MAX_SEGMENTS */
    uint32_t segment_frames;    /* G; 0 = the whole overlap */
    uint32_t block_frames;      /* B; 0 = sample_rate */
    uint32_t drift_frames;
    uint32_t lock_permille;     /* 1 .. 1000 */
    uint32_t requant_millilsb2; /* 1 .. 2^31 */
} rg_compare_opts;  /* 36 bytes */

typedef struct rg_compare_block {
    int64_t aa, bb, ab;  /* summed over the channels */
    uint64_t first_diff; /* frame index in a; all ones = none */
    uint32_t equal;      /* samples, all channels */
    uint32_t max_diff;
    uint32_t frames;     /* of the block */
    uint32_t reserved;
} rg_compare_block;  /* 48 bytes */

typedef struct rg_compare_result {
    int32_t status; /* RG_OK, or why there are no numbers */
    uint32_t flags;
    uint32_t a, b;
    uint64_t frames_a, frames_b; /* Na, Nb */
    uint32_t sample_rate;
    uint32_t channels;           /* Cc */
    uint32_t format_a, format_b;
    uint32_t dropped_a, dropped_b; /* frames the decode route dropped */
    uint32_t block_frames;       /* B */
    uint32_t radius;             /* R */
    uint32_t segments, locked_segments; /* segments measured, and those that locked */
    int32_t polarity;            /* sigma */
    uint32_t max_diff;
    int64_t hint, lag;           /* h and h + d* */
    int64_t seg_lag_min, seg_lag_max;
    uint64_t overlap;            /* W */
    uint64_t a_head, a_tail, b_head, b_tail;
    uint32_t blocks, differing_blocks, worst_block, reserved;
    uint64_t equal, first_diff, nonfinite;
    int64_t aa, bb, ab;          /* exact, the same bits on every route */
    double lock, gain_db, null_unity_db, null_db, residual_lsb2, worst_block_db, gain_min_db, gain_max_db; /* the finish */
} rg_compare_result;  /* 80 + 32 + 40 + 16 + 48 + 64 = 280 bytes */

/* The n files are decoded by the very route rg_pcm_stats uses -- the same loaders, the device FLAC decoder (tuning key 14 = 1) or
 * the host decoder (key 14 = 0) -- and the n_pairs pairs of them measured where the PCM lies, in the analysis arena, by the kernels
 * of rg_compare.hip on the stream the decode ran on.  All of a call's files must be resident together: when the list would be
 * decoded in more than one group (tuning key 13 sets the group's size) the call is refused as a whole, RG_ERR_REFUSED, with a text
 * that says so.  Stage A: with opts.align == RG_CMP_ALIGN_FINGERPRINT (the default) the fingerprint kernels
 * (mp3rgain_amd_fingerprint.h) run on the files and the match kernel on the requested pairs only, at the fingerprint's defaults
 * with the radius opts.coarse_radius; h = 512 * lag, its sign brought to "b behind a"; a pair the match skips (a short file, a
 * rate the fingerprint does not support) gets h = 0 and RG_CMP_NO_COARSE.  With RG_CMP_ALIGN_HINT h is the pair's `hint`.
 * opts, blocks_out, blocks_per_pair and lag_sums as the seam's below.  A failing file fails its own pairs only: RG_ERR_IO or
 * RG_ERR_FORMAT in the pair's `status` (text: rg_tracks_error(ctx, file)), the record otherwise zero.  A pair whose files both
 * loaded and which still cannot be measured (2^32 samples or more, a sample rate beyond RG_CMP_MAX_BLOCK_FRAMES as the block
 * length) gets RG_ERR_FORMAT alone, and its text is the pair's: rg_compare_error(ctx, pair); no file's text changes.  dropped_a and dropped_b are
 * the frames the route dropped, RG_CMP_COMPLETE clear when there are any.  RG_ERR_INVALID_ARG for an option out of range, a == b,
 * an index that is not a file and a hint beyond RG_CMP_MAX_HINT.  `out`, `blocks_out` and `lag_sums` are byte for byte the same for
 * tuning key 14 = 1 and 0. */
int rg_compare(rg_ctx *ctx, const char *const *paths, size_t n, const rg_compare_pair *pairs, size_t n_pairs, const rg_compare_opts *opts,
               rg_compare_result *out, rg_compare_block *blocks_out, size_t blocks_per_pair, int64_t *lag_sums);

/* The text of pair `pair` of the last rg_compare call: why it was not compared although both its files loaded; "" otherwise. */
const char *rg_compare_error(const rg_ctx *ctx, size_t pair);

/* Test seam: the n_pairs pairs of the n tracks that descs[i] describe in the host arena `arena`.  opts: NULL = the defaults.
 * out[p] is pair p's record (dropped_a and dropped_b 0, RG_CMP_COMPLETE set).  blocks_out: NULL, or n_pairs * blocks_per_pair
 * rows, row p * blocks_per_pair + k block k of pair p (blocks beyond blocks_per_pair are not written, rows that are not a block
 * are zero).  lag_sums: NULL, or n_pairs slabs of segments * RG_CMP_MAX_CHANNELS lag rows of 2 * radius + 3 int64 each, row
 * s * RG_CMP_MAX_CHANNELS + c of slab p the row of segment s and channel c of pair p (rows of what was not measured are zero).
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the kernels of rg_compare.hip (`ctx` is an rg_ctx)
 *   route 2  the kernels' cutting and fold arithmetic run on the host; `ctx` may be NULL
 * A track needs only sample alignment, and the two tracks of a pair may have different formats.  RG_ERR_INVALID_ARG for an option
 * out of range, a == b, an index that is not a track, a hint beyond RG_CMP_MAX_HINT, a track whose planes are not wholly inside the
 * arena or not sample-aligned, and a block length outside 1 .. RG_CMP_MAX_BLOCK_FRAMES (also when it comes from the sample rate);
 * RG_ERR_FORMAT for a track that is not 1 .. 8 channels of one of the three formats with fewer than 2^32 frames.  With a NULL ctx
 * the error text is rg_last_error(NULL)'s. */
int rg_compare_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, size_t n_pairs, const rg_compare_pair *pairs,
                     const rg_compare_opts *opts, const void *arena, size_t arena_bytes, rg_compare_result *out, rg_compare_block *blocks_out,
                     size_t blocks_per_pair, int64_t *lag_sums);

/* Test seam: how the kernels cut a pair whose tracks have formats format_a and format_b.  piece_frames: frames of one
 * workgroup's piece of the moments kernel (pieces are counted from the block's first frame); tile_frames: reference frames of one
 * workgroup's tile of the lag kernel (tiles are counted from the segment's first frame); strip_frames, lag_group: as the stereo
 * scan's; lds_bytes: the lag kernel's LDS.  Any pointer may be NULL.  RG_ERR_FORMAT for a format that is none of the three. */
int rg_compare_kernel_shape(uint32_t format_a, uint32_t format_b, uint32_t *piece_frames, uint32_t *tile_frames, uint32_t *strip_frames,
                            uint32_t *lag_group, uint32_t *lds_bytes);

/* Measurement hook (tools/compare_rate.py): n_tracks tracks of `frames` frames of 2 channels of `format` at 44.1 kHz, filled on the
 * device with pseudo-random samples, each at its own offset of one device arena; pair p is tracks 2p (the reference copy) and
 * 2p + 1 with hint 0, n_pairs <= n_tracks / 2 of them.  opts: NULL = the defaults.  Once: the lag kernel, the host's pick and the
 * plan of stage C from it.  After a warm-up of `warm_ms` milliseconds of launches, `reps` rounds of: the moments kernels and the
 * fold over all pairs (moments_ms[r], HIP events around the launches alone); the clearing of the lag rows and the lag kernel
 * (lags_ms[r]); then the serial host twin -- lag rows, pick, blocks and totals -- over a host copy of the first host_pairs pairs on
 * `threads` host threads (host_ms[r]).  *mismatches: host pairs whose lag rows, lag, polarity, block rows or totals differ from
 * the kernels' (it must be 0).  *bytes: the bytes of PCM the pairs' tracks hold (stage C reads the overlap of both once).  *macs:
 * the multiply-adds of the definition in one round of the lag leg.  `ctx` is an rg_ctx.  The read floor over such an arena is
 * rg_dr_rate's and the stereo scan's pair and lag kernel are rg_stereo_rate's: the tool calls them in the same process. */
int rg_compare_rate(void *ctx, size_t n_tracks, size_t n_pairs, uint64_t frames, uint32_t format, const rg_compare_opts *opts, size_t host_pairs,
                    uint32_t threads, uint32_t reps, double warm_ms, double *moments_ms, double *lags_ms, double *host_ms, size_t *mismatches,
                    uint64_t *bytes, uint64_t *macs);

#ifdef __cplusplus
}
#endif
#endif
