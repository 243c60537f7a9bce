/* mp3rgain_amd_r128.h -- C ABI of the EBU R 128 / ReplayGain 2.0 analysis path: integrated loudness after ITU-R BS.1770
 * (K-weighting, 400 ms blocks every 100 ms, absolute gate at -70 LUFS, relative gate at -10 LU), gain to -18 LUFS, sample
 * peak and, on request, true peak.  It sits beside the ReplayGain 1.0 path of mp3rgain_amd.h and shares its contexts, track
 * descriptors, status codes, loaders and device decoders; nothing of that path changes (RG_ABI_VERSION stays).
 *
 * The algorithm, as this library and its checker (tests/r128ref.py) both implement it:
 *  - channels 0 and 1 of a track only, each with weight 1.0 (one channel = BS.1770 mono, not "dual mono"); samples are
 *    normalised to full scale 1.0 (F32 as is, S16 / 32768, S32 / 2^31);
 *  - K-weighting: two biquads in f64 whose coefficients are derived per rate, in long double, from the analogue prototypes
 *    (rg_r128_design_info), any rate from 8000 to 384000 Hz;
 *  - hop = (rate + 5) / 10 frames; hop energy e[h] = sum over the channels of the sum of squared K-weighted samples of hop h,
 *    a partial last hop is dropped; block b = hops b..b+3, z[b] = (e[b] + e[b+1] + e[b+2] + e[b+3]) / (4 hop); a track of H
 *    whole hops has max(H - 3, 0) blocks;
 *  - absolute gate z >= 10^((-70 + 0.691) / 10); relative gate z >= 0.1 * mean of the blocks the absolute gate kept;
 *    L = -0.691 + 10 log10(mean of the blocks both gates kept); no such block: loudness -inf, gain 0; else
 *    gain = RG_R128_REFERENCE_LUFS - L;
 *  - an album gates the union of its tracks' blocks (it is not a mean of track values); album peaks = max over tracks;
 *  - true peak: oversampling by 4 below 96 kHz, by 2 below 192 kHz, sample peak from there on; 49-tap Hann-windowed sinc
 *    h[j] = sinc((j - 24) / F) * 0.5 (1 - cos(2 pi j / 48)) on the zero-stuffed signal, zero history at the start of a track,
 *    the tail after its last sample included; max |value| over channels 0 and 1 (f32 arithmetic);
 *  - a track with samples that are not finite carries RG_TRACK_FLAG_NONFINITE, its loudness and gain are NaN, its peaks are
 *    the max over finite values; an album with such a track has NaN loudness; other tracks of the batch are unaffected.
 *
 * Loudness range (EBU Tech 3342) and the momentary / short-term maxima (rg_r128_dynamics, the *_dynamics entry points), as
 * this library and their checker (tests/r128range_ref.py) both implement them, from the same hop energies:
 *  - maximum momentary loudness: -0.691 + 10 log10(max over b of z[b]) over all max(H - 3, 0) gating blocks, ungated; no
 *    block, or a maximum of 0: -inf;
 *  - short-term blocks: st[s] = (e[s] + ... + e[s+29]) / (30 hop) for s = 0 .. H-30, one every 100 ms (3 s blocks that
 *    overlap by 2.9 s); a track of H whole hops has max(H - 29, 0) of them (rg_r128_short_term_count); e[h] is the sum over
 *    channels 0 and 1 of hop h, and the 30 terms are added one after another in ascending h: the value depends on nothing
 *    but the 30 energies;
 *  - maximum short-term loudness: -0.691 + 10 log10(max over s of st[s]), -inf as above;
 *  - loudness range: A = the blocks with st >= 10^((-70 + 0.691) / 10); thr = 0.01 * mean(A) (-20 LU); K = the blocks of A
 *    with st >= thr, sorted ascending, n = |K|; low = K[(10 (n - 1) + 50) / 100], high = K[(95 (n - 1) + 50) / 100], both
 *    in integer division; LRA = 10 log10(high / low) LU; range_low and range_high are low and high in LUFS; n = 0: LRA 0.0
 *    and both bounds -inf.  low and high are elements of the block list, bit for bit: selected, not interpolated and not
 *    read from a histogram;
 *  - an album: the union of its tracks' short-term blocks in track order (a block never spans two tracks), the same two
 *    gates and the same selection; its maxima are the maxima over its tracks;
 *  - a track that carries RG_TRACK_FLAG_NONFINITE has NaN in all five values (and st_blocks_gated 0), an album with such a
 *    track too; other tracks of the batch are unaffected.
 *
 * Out of scope here: many albums in one call, node / multi-GPU and asynchronous variants, surround channel weights, writing
 * R128_* Opus tags or range tags.
 */
#ifndef MP3RGAIN_AMD_R128_H
#define MP3RGAIN_AMD_R128_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_R128_REFERENCE_LUFS (-18.0)
#define RG_R128_MIN_RATE 8000u
#define RG_R128_MAX_RATE 384000u

typedef struct rg_r128_track_result {
    double loudness_lufs;
    double gain_db;
    double sample_peak;
    double true_peak;      /* NaN when not asked for */
    uint32_t sample_rate;
    uint32_t blocks;       /* gating blocks of the track */
    uint32_t blocks_gated; /* those both gates kept */
    uint32_t flags;        /* RG_TRACK_FLAG_NONFINITE */
} rg_r128_track_result;

typedef struct rg_r128_album_result {
    double loudness_lufs;
    double gain_db;
    double sample_peak;
    double true_peak;      /* NaN when not asked for */
    uint32_t blocks;
    uint32_t blocks_gated;
} rg_r128_album_result;

typedef struct rg_r128_dynamics {
    double loudness_range_lu;
    double range_low_lufs;      /* the 10th percentile of the gated short-term blocks */
    double range_high_lufs;     /* the 95th */
    double max_momentary_lufs;
    double max_short_term_lufs;
    uint32_t st_blocks;         /* short-term blocks of the track (of the album: of all its tracks) */
    uint32_t st_blocks_gated;   /* those both gates of the loudness range kept (n above) */
} rg_r128_dynamics;

/* ---- pure helpers (host) ---------------------------------------------------------------- */
int rg_r128_supported_rate(uint32_t sample_rate); /* 8000 .. 384000 Hz */
/* The K-weighting of one rate: stage 1 (shelf) b1 / a1, stage 2 (RLB high-pass) b2 / a2, three values each, a[0] = 1;
 * hop in frames, true-peak oversampling factor.  Any pointer may be NULL.  RG_ERR_UNSUPPORTED_RATE outside the range. */
int rg_r128_design_info(uint32_t sample_rate, double *b1, double *a1, double *b2, double *a2, uint32_t *hop, uint32_t *tp_factor);
/* gating blocks of a track of `frames` frames (0 for an unsupported rate) */
uint64_t rg_r128_block_count(uint32_t sample_rate, uint64_t frames);
/* short-term (3 s) blocks of a track of `frames` frames (0 for an unsupported rate) */
uint64_t rg_r128_short_term_count(uint32_t sample_rate, uint64_t frames);

/* key 1 = hops per lane S of the loudness kernel (0 = chosen from the batch; at most 4096).  A lane runs the recursion over S
 * consecutive hops of one channel and starts three hops early from the zero state; results do not depend on S beyond f64
 * rounding of what a lane has not seen (below 1e-30 of the signal before its start).
 * key 2 = how an album's loudness range is selected: 0 = chosen from the album's size (wide from 16384 short-term blocks),
 * 1 = one workgroup makes every pass over the album's short-term blocks, 2 = every pass is a wide launch counting into an
 * integer histogram.  Both select the same elements; the threshold's sum is rounded in another order, which shows only for
 * a block within an ulp of it. */
int rg_r128_set_tuning(rg_ctx *ctx, int key, int64_t value);

/* ---- analysis (synchronous) ----------------------------------------------------------------- */
/* n independent tracks of a planar PCM arena (rg_track_desc, mp3rgain_amd.h: sample alignment only, any storage order,
 * descriptors may alias, nothing outside a track's bytes counts).  block_z_out: NULL, or room for the sum of
 * rg_r128_block_count over the tracks: every block's mean square z, track after track.
 * pcm_on_device = 1: pcm_base is a device pointer and the kernels read it on the context's own stream, which is not ordered
 * behind any stream of the caller's: the PCM must be complete (the producing stream synchronised) before the call. */
int rg_r128_analyze_pcm_batch(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                              int pcm_on_device, int want_true_peak, rg_r128_track_result *out, double *block_z_out);
/* the same, and the n tracks as one album */
int rg_r128_analyze_album_pcm(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                              int pcm_on_device, int want_true_peak, rg_r128_track_result *tracks_out,
                              rg_r128_album_result *album_out, double *block_z_out);
/* Files, through the loaders and device decoders of rg_analyze_tracks / rg_analyze_album (MP3, FLAC, WAV, decoder command,
 * groups that fit the device), with their per-file status and error texts (rg_tracks_error); only the rate check differs:
 * "Unsupported sample rate: {} Hz. Supported rates: 8000 to 384000".  An album taken in several groups keeps its hop
 * energies and is gated once at the end: the same result as in one group. */
int rg_r128_analyze_tracks(rg_ctx *ctx, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                           rg_r128_track_result *out, int32_t *status_out);
int rg_r128_analyze_album(rg_ctx *ctx, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                          rg_r128_track_result *tracks_out, rg_r128_album_result *album_out);

/* ---- the same four, and loudness range and momentary / short-term maxima ------------------------------------------------ */
/* Everything the call of the same name without _dynamics returns is returned bit for bit; dyn_out has one entry per track
 * (per file: zeroed where the file failed), album_dyn_out is the album's.  st_z_out: NULL, or room for the sum of
 * rg_r128_short_term_count over the tracks: every short-term block's mean square st, track after track. */
int rg_r128_analyze_pcm_batch_dynamics(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                                       int pcm_on_device, int want_true_peak, rg_r128_track_result *out, double *block_z_out,
                                       rg_r128_dynamics *dyn_out, double *st_z_out);
int rg_r128_analyze_album_pcm_dynamics(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const void *pcm_base, size_t pcm_bytes,
                                       int pcm_on_device, int want_true_peak, rg_r128_track_result *tracks_out,
                                       rg_r128_album_result *album_out, double *block_z_out, rg_r128_dynamics *dyn_out,
                                       rg_r128_dynamics *album_dyn_out, double *st_z_out);
int rg_r128_analyze_tracks_dynamics(rg_ctx *ctx, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                    rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out);
int rg_r128_analyze_album_dynamics(rg_ctx *ctx, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                   rg_r128_track_result *tracks_out, rg_r128_album_result *album_out, rg_r128_dynamics *dyn_out,
                                   rg_r128_dynamics *album_dyn_out);

#ifdef __cplusplus
}
#endif
#endif /* MP3RGAIN_AMD_R128_H */
