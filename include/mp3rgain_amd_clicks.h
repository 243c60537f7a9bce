/* mp3rgain_amd_clicks.h -- clicks and glitches in a file, found on the GPU: a read glitch that passed without a log, a skipped or
 * repeated sector, a stuck sample, a tick of a vinyl transfer.  Every channel is predicted from its own past by the FLAC encoder's
 * linear model, block by block; a sample whose prediction error stands far above the median error around it is flagged, flagged
 * samples close to one another make an event, and a narrow event is a click.  One decode, on the device, one more read of every
 * sample from the planes the file route has put into the analysis arena, and a fixed-size record per file comes back, with an
 * optional list of the first events.
 *
 * THE DEFINITIONS BELOW ARE A CONVENTION OF THIS PROJECT.  They were tried on synthetic material only and are held to no other
 * tool: nobody here has run them over real music, and no other declicker was at hand to compare with.
 *
 * DEFINITIONS (the contract).
 *
 * Plane: one channel of one track, N < 2^32 samples in one of the three arena formats, reduced to a 16-bit integer q exactly as
 * the stereo scan reduces a sample (mp3rgain_amd_stereo.h): S16 q = v; S32 q = v >> 16 (floor); F32 a NaN or Inf sample has q = 0
 * and counts in `nonfinite`, otherwise q = min(rintf(clamp(x, -1, 1) * 32768), 32767).  Every channel of a track is scanned, 1 to
 * RG_CK_MAX_CHANNELS.
 *
 * Options: rg_clicks_opts; NULL means RG_CK_DEFAULT_*.
 *   block_samples B   256, 512, 1024, 2048 or 4096                                 default 1024
 *   order P           even, 2 .. 12                                                default 8
 *   ratio_permille    1000 .. 1 000 000                                            default MEASURED, see below
 *   floor             1 .. 32767       A STATED CONVENTION                         default 4
 *   gap               1 .. 255         A STATED CONVENTION                         default 16
 *   max_width         1 .. 4095        A STATED CONVENTION                         default 32
 *   max_events K      0 .. 256                                                     default 16
 *
 * Model of block b.  Block b is samples [bB, min((b+1)B, N)), n_b of them.  Its model is the FLAC encoder's (mp3rgain_amd_flacenc.h)
 * of that block's q at order P and coefficient precision 12: xw[i] = (q[bB + i] * w(i, n_b)) >> 15 with the encoder's integer
 * Welch window w; the exact int64 autocorrelation of xw at lags 0 .. P; the Levinson-Durbin recursion in double in the encoder's
 * operation order, with no contraction; the encoder's quantisation to 12 bits with its shift rule (from the largest coefficient's
 * exponent, at most 15) and error feedback.  A block FALLS BACK to the fixed second-order predictor c = (2, -1), shift 0, order 2
 * when n_b < 4P, when its lag-0 sum is 0, when the recursion stops before order P (the error is no longer positive) or when the
 * quantisation fails; it then counts in `fallback_blocks`.
 *
 * Residual: r[n] = q[n] - ((sum over j < order of c_j * q[n-1-j]) >> shift), in int64, an arithmetic shift, with the coefficients
 * of the block that holds n.  The history is the plane's own samples, across the block's start; r[n] = 0 for n below the order in
 * use, where the plane has no history.  e[n] = |r[n]| < 2^30.
 *
 * Scale: m_b is the lower median of the block's e, the element of rank floor((n_b - 1) / 2) counted from 0, exactly.
 * S(n) = max(m_(b-1), m_b, m_(b+1), floor) for n in block b, a neighbour that does not exist left out.  THREE BLOCKS, because music
 * that starts late in a block after digital silence has a median of 0 there, and its first samples must not read as a click
 * against the floor: the block that follows vouches for them.  The same holds where music ends.
 *
 * Flagged sample: 1000 * e[n] > ratio_permille * S(n) in 64-bit integers.  Its strength is min(floor(1000 * e[n] / S(n)), 2^32 - 1).
 *
 * Event: a maximal set of flagged samples of one plane in which consecutive members are at most `gap` samples apart.  start = its
 * first sample, width = last - first + 1, strength = the largest strength of its members, peak_at = the first sample that reaches
 * it.  An event with width <= max_width is a CLICK (RG_CK_KIND_CLICK), a wider one a BURST (RG_CK_KIND_BURST): a hard onset or a
 * scratch, not a tick.
 *
 * Per channel (rg_clicks_channel): flagged (samples), clicks, bursts (events), widest (the largest width of any event),
 * first_click (the start of the first click; N when there is none), strongest_permille and strongest_at (strength and peak_at of
 * the strongest click, the earliest on a tie; 0 and N when there is none), fallback_blocks, median_max (the largest m_b).
 *
 * flags:
 *   RG_CK_COMPLETE    dropped_frames == 0
 *   RG_CK_SILENT      every q of every channel is 0 (or N is 0)
 *   RG_CK_NONFINITE   nonfinite > 0
 *   RG_CK_CLICKS      some channel has a click
 *   RG_CK_BURSTS      some channel has a burst
 *   RG_CK_TRUNCATED   the file has more events than max_events, so more than its list shows
 *
 * Event list (optional): n rows of K = max_events records rg_clicks_event.  Row i holds the first K events of file i ordered by
 * (start, channel); unused records are zero.  `events` (in the result) = the events of all channels, `listed` = min(events, K).
 * The device delivers each plane's first K events; the merge across channels is host code shared by every route.
 *
 * THE DEFAULT RATIO is measured by tools/clicks_refcheck.py on the serial host twin over SYNTHETIC MATERIAL ONLY and recorded in
 * tests/golden/clicks_measured.json; it is the geometric mean of the two sides below.  Nobody has tried it on real music.
 *   ratio_permille 8371
 *     Undamaged side, 6.67 x (rg_synth.h tracks of 12 s, one of them hot, with their one-second silence gap; tone mixes over a
 *     noise floor of 2^-13 of full scale; partly tonal mixes of coloured noise and tones; both as 24-bit and as float, and
 *     through the project's MP3 encoder at 128 and 320 kb/s).  Each is scanned at every ratio of a ladder from 4 upwards until
 *     nothing is flagged, and the figure is the strongest click read at any of them: 4.8 .. 6.7 x the scale, simply the tail of
 *     a Gaussian residual over 3 to 12 seconds.  The tail grows with the length: a noise-like file of minutes comes closer to
 *     the default than these.  At the default every one of these reads no clicks; the tool checks that.
 *     Damaged side, 10.51 x.  Found (claimed: each of ten planted defects found within `gap` of its place, the weakest at least
 *     1.5 x the undamaged side, and all ten found again at the default).  IN THE TONE MIX: single-sample impulses of 1/64 .. 1/2
 *     of full scale (the weakest reads 35.6 x), a run of 4 stuck samples (39.6 x), skips of 1, 10 and 588 samples (22.7 x,
 *     44.1 x, 34.6 x), a repeated 588-sample sector (42.3 x).  IN THE PARTLY TONAL MIX, whose residual is noise of 700 LSB:
 *     impulses of 1/2 and 1/4 of full scale (22.8 x, 10.5 x).  A larger impulse does not read stronger: it also spoils the model
 *     of its own block.
 * FALSE POSITIVES: THE TEMPO CASES' DRUM PATTERN IS NOT COUNTED AS UNDAMAGED MATERIAL, by a rule the tool states.  Its snare and
 * hat are noise that starts at full level within one sample, which is what this header calls a click: its strongest click reads
 * 104.6 x, and at the default it reads 47 clicks and 21 bursts in 3 seconds of two channels.  Percussion with such onsets -- a
 * drum machine -- reads as clicks; hard onsets are told from ticks and scratches by width alone.
 * Not found (not claimed; the numbers are in clicks_measured.json), all in the partly tonal mix: impulses of 1/8 of full scale
 * (8 of 10 found), of 1/16 (1 of 10), of 1/32 and 1/64 (none), a run of 4 stuck samples (none), skips of 1, 10 and 588 samples
 * (1, 2 and 2 of 10), a repeated 588-sample sector (1 of 10): they stay inside the noise's own tail.  Crackle below the ratio.
 * A stream that starts or stops in mid-wave has a click there.  A block in which music stops or starts abruptly is modelled on
 * mostly silence, and the music's few samples in it may be flagged against the neighbours' scale.  Events that coincide across
 * channels are not declared one class: each channel lists its own.
 * Not here: repairing or interpolating a click; the node and multi-GPU calls; any comparison with another declicker (none was at
 * hand).
 */
#ifndef MP3RGAIN_AMD_CLICKS_H
#define MP3RGAIN_AMD_CLICKS_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_CK_COMPLETE   1u
#define RG_CK_SILENT     2u
#define RG_CK_NONFINITE  4u
#define RG_CK_CLICKS     8u
#define RG_CK_BURSTS     16u
#define RG_CK_TRUNCATED  32u
#define RG_CK_KIND_CLICK 1u
#define RG_CK_KIND_BURST 2u
#define RG_CK_MAX_CHANNELS 8u
#define RG_CK_MAX_ORDER 12u
#define RG_CK_MAX_EVENTS 256u
#define RG_CK_DEFAULT_BLOCK 1024u
#define RG_CK_DEFAULT_ORDER 8u
#define RG_CK_DEFAULT_RATIO_PERMILLE 8371u /* measured, see above */
#define RG_CK_DEFAULT_FLOOR 4u
#define RG_CK_DEFAULT_GAP 16u
#define RG_CK_DEFAULT_MAX_WIDTH 32u
#define RG_CK_DEFAULT_MAX_EVENTS 16u

typedef struct rg_clicks_opts {
    uint32_t block_samples;  /* 256, 512, 1024, 2048, 4096 */
    uint32_t order;          /* even, 2 .. 12 */
    uint32_t ratio_permille; /* 1000 .. 1000000 */
    uint32_t floor;          /* 1 .. 32767 */
    uint32_t gap;            /* 1 .. 255 */
    uint32_t max_width;      /* 1 .. 4095 */
    uint32_t max_events;     /* 0 .. 256 */
} rg_clicks_opts;

typedef struct rg_clicks_channel {
    uint32_t flagged, clicks, bursts, widest;
    uint32_t first_click;        /* N when there is none */
    uint32_t strongest_at;       /* N when there is none */
    uint32_t strongest_permille; /* 0 when there is none */
    uint32_t fallback_blocks;
    uint32_t median_max;
    uint32_t reserved;
} rg_clicks_channel;             /* 40 bytes */

typedef struct rg_clicks_event {
    uint32_t start, width, peak_at, strength_permille;
    uint16_t channel, kind;      /* kind: RG_CK_KIND_*; 0 in an unused record */
} rg_clicks_event;               /* 20 bytes */

typedef struct rg_clicks_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: samples per channel that were scanned */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;         /* rg_sample_format of the planes */
    uint32_t dropped_frames; /* frames the decode route dropped, as the rip and verify records count them */
    uint32_t block_samples, order, ratio_permille, floor, gap, max_width, max_events; /* the options in force */
    uint32_t listed;         /* min(events, max_events) */
    uint64_t nonfinite;      /* samples, all channels */
    uint64_t events;         /* clicks and bursts of all channels */
    rg_clicks_channel ch[RG_CK_MAX_CHANNELS];
} rg_clicks_result;          /* 32 + 32 + 16 + 320 = 400 bytes */

/* The files are decoded by the very route rg_pcm_stats uses -- the same loaders, the same groups (tuning key 13), the device FLAC
 * decoder (tuning key 14 = 1) or the host decoder (key 14 = 0) -- and scanned where the PCM lies, in the analysis arena, by the
 * kernels of rg_clicks.hip on the stream the decode ran on.  WAV, FLAC and MPEG Layer III.  opts: NULL = the defaults.  events:
 * NULL, or n rows of max_events records, filled group by group.  A failing file fails alone: RG_ERR_IO, RG_ERR_FORMAT (not such a
 * stream, more than 8 channels), its record zero apart from `status`.  A file with dropped frames gets the numbers of what the
 * route decoded, with dropped_frames set and RG_CK_COMPLETE clear.  RG_OK whenever the call itself worked.  `out` and `events` are
 * byte for byte the same for tuning key 14 = 1 and 0. */
int rg_clicks(rg_ctx *ctx, const char *const *paths, size_t n, const rg_clicks_opts *opts, rg_clicks_result *out, rg_clicks_event *events);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames: anything
 * else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_CK_COMPLETE set.  events as above.
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' cutting, tile and fold code run on the host by one lane; `ctx` may be NULL
 * A track needs only sample alignment.  RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not
 * sample-aligned, and for an option outside its range.  With a NULL ctx the error text is rg_last_error(NULL)'s. */
int rg_clicks_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_clicks_opts *opts, const void *arena, size_t arena_bytes,
                    rg_clicks_result *out, rg_clicks_event *events);

/* Test seam: how the kernels cut a plane at block length `block_samples`.  tile_samples: samples of one workgroup's tile (whole
 * blocks; tiles are counted from the plane's first sample, and the workgroup reads one more block on either side);
 * tile_blocks: blocks of a tile; fold_lanes: lanes of the fold kernel's workgroup, each folding a run of consecutive tiles;
 * lds_bytes: the tile kernel's LDS.  Any pointer may be NULL.  RG_ERR_INVALID_ARG for a block length that is none of the five. */
int rg_clicks_kernel_shape(uint32_t block_samples, uint32_t *tile_samples, uint32_t *tile_blocks, uint32_t *fold_lanes, uint32_t *lds_bytes);

/* Measurement hook (tools/clicks_rate.py): `n` tracks of `frames` frames of 2 channels of `format` at 44.1 kHz, filled on the
 * device with pseudo-random samples, each at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of
 * launches, `reps` rounds of: the tile kernel over all planes (scan_ms[r], HIP events around the launch alone); the fold kernel
 * (fold_ms[r]); the emit kernel over the tiles the fold listed (emit_ms[r]); then the serial host twin over a host copy of the
 * first `host_tracks` (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host tracks whose records or event
 * lists differ from the kernels' (it must be 0).  *bytes: the bytes of PCM one round of the scan leg covers (it reads its margin
 * blocks on top of them).  *macs: the multiply-adds of the definition in one round, samples * (2 * order + 1): the window, the
 * autocorrelation and the residual.  `opts`: NULL = the defaults.  `ctx` is an rg_ctx.  DR's read floor over such an arena is
 * rg_dr_rate's: the tool calls it in the same process. */
int rg_clicks_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, const rg_clicks_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                   double warm_ms, double *scan_ms, double *fold_ms, double *emit_ms, double *host_ms, size_t *mismatches, uint64_t *bytes, uint64_t *macs);

#ifdef __cplusplus
}
#endif
#endif
