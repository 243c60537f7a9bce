/* mp3rgain_amd_r128.h -- C ABI of the EBU R 128 / ReplayGain 2.0 analysis path: integrated loudness after ITU-R BS.1770
 * (K-weighting, 400 ms blocks every 100 ms, absolute gate at -70 LUFS, relative gate at -10 LU), gain to -18 LUFS, sample
 * peak and, on request, true peak.  It sits beside the ReplayGain 1.0 path of mp3rgain_amd.h and shares its contexts, track
 * descriptors, status codes, loaders and device decoders; nothing of that path changes (RG_ABI_VERSION stays).
 *
 * The algorithm, as this library and its checker (tests/r128ref.py) both implement it:
 *  - channels 0 and 1 of a track only, each with weight 1.0 (one channel = BS.1770 mono, not "dual mono"), unless the
 *    track is weighted (channel weights, below); samples are normalised to full scale 1.0 (F32 as is, S16 / 32768,
 *    S32 / 2^31);
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
 * Many albums in one call (rg_r128_analyze_albums*, below) gate every album on the device in the same launches, and the node
 * entry points deal whole albums (or files) out over the GPUs of a node.
 *
 * Channel weights (BS.1770 multichannel loudness).  A context has a channel mode (rg_r128_set_channel_mode):
 *  - RG_R128_CHANNELS_PAIR, the default: everything above as it stands, channels 0 and 1 with weight 1.0;
 *  - RG_R128_CHANNELS_LAYOUT: every track is weighted by its channel layout (rg_r128_layout_weights).  The PCM calls use
 *    rg_r128_layout_weights(channels, 0); the file calls, and the node calls through each device's context, use the
 *    container's channel mask where it has one (WAVE_FORMAT_EXTENSIBLE, also from a decoder command's pipe; FLAC and
 *    everything else: the default of the channel count).  MP3 never has more than two channels.
 *  - rg_r128_analyze_pcm_weighted takes explicit weights per track; they override the mode.
 * A weighted track (rg_r128_channel_weights):
 *  - has 1 to 8 channels; entries of w at and beyond the channel count are ignored, every used entry must be finite and
 *    >= 0; otherwise the call returns RG_ERR_INVALID_ARG and names the track before any output is touched (a file fails
 *    alone: "Unsupported channel count for layout analysis: {n} (1 to 8)");
 *  - hop energy e[h] = sum over the channels c with w[c] != 0 of w[c] * e_c[h], e_c[h] the sum of squared K-weighted samples
 *    of hop h of channel c: in ascending channel order, starting from the first such channel, every product rounded on its
 *    own (no fused multiply-add across the sum); all weights zero: every e[h] is 0.  From there on blocks, gates, albums,
 *    short-term blocks, range and maxima are what is specified above for a one-channel e[h] (block_z_out and st_z_out carry
 *    the weighted values);
 *  - sample peak and true peak are the maximum over ALL channels of the track whatever their weight (a clipping LFE still
 *    clips), and a sample that is not finite in any channel raises RG_TRACK_FLAG_NONFINITE;
 *  - with at most two channels whose used weights are all exactly 1.0 it is not weighted at all: it takes the path above
 *    and returns its bits.
 * Weighted and plain tracks may share a batch; the plain ones run exactly as without the others.
 * The layout rule (BS.1770-4 table 4: 1.41 for |azimuth| 60 to 120 degrees at low elevation, 1.0 elsewhere, LFE not
 * counted): channel i is the i-th set bit of the WAVE dwChannelMask in ascending bit order.  A mask of 0, or one whose
 * population count is not the channel count, is replaced by the default of the count, the FLAC channel order: 1: 0x4,
 * 2: 0x3, 3: 0x7, 4: 0x33, 5: 0x37, 6: 0x3F, 7: 0x70F, 8: 0x63F.  LFE (0x8): 0.  SL and SR (0x200, 0x400): 1.41.  BL and
 * BR (0x10, 0x20): 1.41 when the mask has neither SL nor SR, else 1.0.  Every other position: 1.0.
 *
 * Out of scope here: one album across several GPUs (it would need an exchange of hop energies), asynchronous variants,
 * writing R128_* Opus tags or range tags.
 */
#ifndef MP3RGAIN_AMD_R128_H
#define MP3RGAIN_AMD_R128_H

#include "mp3rgain_amd.h"
#include "mp3rgain_amd_node.h"

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

#define RG_R128_CHANNELS_PAIR 0
#define RG_R128_CHANNELS_LAYOUT 1

typedef struct rg_r128_channel_weights {
    double w[8];
} rg_r128_channel_weights;

/* ---- pure helpers (host) ---------------------------------------------------------------- */
/* the weights of a layout of 1 to 8 channels (the rule above); RG_ERR_INVALID_ARG for any other count or out == NULL */
int rg_r128_layout_weights(uint32_t channels, uint32_t channel_mask, rg_r128_channel_weights *out);
int rg_r128_supported_rate(uint32_t sample_rate); /* 8000 .. 384000 Hz */
/* The K-weighting of one rate: stage 1 (shelf) b1 / a1, stage 2 (RLB high-pass) b2 / a2, three values each, a[0] = 1;
 * hop in frames, true-peak oversampling factor.  Any pointer may be NULL.  RG_ERR_UNSUPPORTED_RATE outside the range. */
int rg_r128_design_info(uint32_t sample_rate, double *b1, double *a1, double *b2, double *a2, uint32_t *hop, uint32_t *tp_factor);
/* gating blocks of a track of `frames` frames (0 for an unsupported rate) */
uint64_t rg_r128_block_count(uint32_t sample_rate, uint64_t frames);
/* short-term (3 s) blocks of a track of `frames` frames (0 for an unsupported rate) */
uint64_t rg_r128_short_term_count(uint32_t sample_rate, uint64_t frames);

/* How an album of st_blocks short-term blocks is selected under tuning key 2 = album_select: 1 = one workgroup, 2 = wide
 * passes.  rg_r128_albums_count_workgroups: the workgroups of one wide counting pass over such an album (each takes at
 * least 4096 values, 256 at most).  rg_r128_albums_wide_rounds: a call's wide albums are selected 64 at a time, the rounds
 * that many albums take; *state_bytes (may be NULL): the device memory of their selection states (203264 bytes per album
 * of a round, 12.4 MiB at most). */
int rg_r128_album_select_form(int album_select, uint64_t st_blocks);
uint32_t rg_r128_albums_count_workgroups(uint64_t st_blocks);
size_t rg_r128_albums_wide_rounds(size_t wide_albums, size_t *state_bytes);

/* key 1 = hops per lane S of the loudness kernel (0 = chosen from the batch; at most 4096).  A lane runs the recursion over S
 * consecutive hops of one channel and starts three hops early from the zero state; results do not depend on S beyond f64
 * rounding of what a lane has not seen (below 1e-30 of the signal before its start).
 * key 2 = how an album's loudness range is selected: 0 = chosen from the album's size (wide from 16384 short-term blocks),
 * 1 = one workgroup makes every pass over the album's short-term blocks, 2 = every pass is a wide launch counting into an
 * integer histogram.  Both select the same elements; the threshold's sum is rounded in another order, which shows only for
 * a block within an ulp of it. */
int rg_r128_set_tuning(rg_ctx *ctx, int key, int64_t value);

/* RG_R128_CHANNELS_PAIR (the default) or RG_R128_CHANNELS_LAYOUT; anything else: RG_ERR_INVALID_ARG */
int rg_r128_set_channel_mode(rg_ctx *ctx, int mode);

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

/* ---- many albums in one call ------------------------------------------------------------------------------------------------ */
/* Albums as in rg_analyze_albums: album a is tracks (files) [album_first[a], album_first[a + 1]); album_first[n_albums + 1]
 * ascends from 0 to n.  A malformed album_first is refused with RG_ERR_INVALID_ARG and the function's name in front of the
 * reason, before any output is touched.  One pass over all n tracks, then every album's gates (and, with _dynamics, every
 * album's loudness range) in the same launches: for a PCM call whose wide albums fit one round of 64, the number of kernel
 * launches does not depend on n_albums.
 *  - Equality: album a's record, every track's record and, with _dynamics, both rg_r128_dynamics are bit for bit what the
 *    single-album call of the same kind returns on that album's tracks or files under the same tuning: the same hops per
 *    lane (key 1 set, or both batches small enough that the library chooses S = 4) and the same album selection mode
 *    (key 2; with key 2 = 0 the form is chosen per album from that album's own short-term block count, as the single-album
 *    call does).
 *  - An album without tracks gets what rg_r128_analyze_album gives for n = 0.
 *  - An album with a track that is not finite has NaN loudness and NaN dynamics; other albums are unaffected.
 * block_z_out, st_z_out: as in rg_r128_analyze_pcm_batch[_dynamics], over all n tracks. */
int rg_r128_analyze_albums_pcm(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const size_t *album_first, size_t n_albums,
                               const void *pcm_base, size_t pcm_bytes, int pcm_on_device, int want_true_peak,
                               rg_r128_track_result *tracks_out, rg_r128_album_result *albums_out, double *block_z_out);
int rg_r128_analyze_albums_pcm_dynamics(rg_ctx *ctx, const rg_track_desc *tracks, size_t n, const size_t *album_first,
                                        size_t n_albums, const void *pcm_base, size_t pcm_bytes, int pcm_on_device,
                                        int want_true_peak, rg_r128_track_result *tracks_out, rg_r128_album_result *albums_out,
                                        double *block_z_out, rg_r128_dynamics *dyn_out, rg_r128_dynamics *albums_dyn_out,
                                        double *st_z_out);
/* The most general PCM call, with channel weights: weights[n], or NULL = by the context's channel mode.  album_first = NULL
 * with n_albums = 0: no albums (albums_out and albums_dyn_out are not used); dyn_out = NULL (and albums_dyn_out = NULL): no
 * dynamics.  With weights = NULL in PAIR mode it returns bit for bit what rg_r128_analyze_albums_pcm[_dynamics] returns
 * (without albums: rg_r128_analyze_pcm_batch[_dynamics]). */
int rg_r128_analyze_pcm_weighted(rg_ctx *ctx, const rg_track_desc *tracks, const rg_r128_channel_weights *weights, size_t n,
                                 const size_t *album_first, size_t n_albums, const void *pcm_base, size_t pcm_bytes,
                                 int pcm_on_device, int want_true_peak, rg_r128_track_result *tracks_out,
                                 rg_r128_album_result *albums_out, double *block_z_out, rg_r128_dynamics *dyn_out,
                                 rg_r128_dynamics *albums_dyn_out, double *st_z_out);
/* Files: the groups of rg_r128_analyze_tracks over the whole list, with its per-file status and texts (rg_tracks_error; a
 * WAV of a format no de-interleave reads fails alone with "Failed to probe format").  After each group every album whose
 * last file lies in the groups taken so far is gated, all of them in one album stage; an album that goes on into the next
 * group keeps its hop energies on the device until then.  album_status_out[a]: RG_OK, or the code of the album's first
 * failing file in input order -- code and text are what rg_r128_analyze_album reports for that album; albums_out[a] and
 * albums_dyn_out[a] are then zero.  A failing file or album does not stop the others, a file's result is valid whenever its
 * status is RG_OK, and the return value is RG_OK when the call itself worked.  When it did not (a device error), everything
 * not finished carries the call's code and text, as in rg_analyze_albums. */
int rg_r128_analyze_albums(rg_ctx *ctx, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                           int32_t track_index, int want_true_peak, rg_r128_track_result *tracks_out, int32_t *status_out,
                           rg_r128_album_result *albums_out, int32_t *album_status_out);
int rg_r128_analyze_albums_dynamics(rg_ctx *ctx, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                                    int32_t track_index, int want_true_peak, rg_r128_track_result *tracks_out, int32_t *status_out,
                                    rg_r128_album_result *albums_out, int32_t *album_status_out, rg_r128_dynamics *dyn_out,
                                    rg_r128_dynamics *albums_dyn_out);

/* ---- all GPUs of a node (mp3rgain_amd_node.h) ---------------------------------------------------------------------------- */
/* Files (rg_r128_analyze_tracks_node) or whole albums (rg_r128_analyze_albums_node) are dealt out by their bytes with
 * rg_node_partition; every device makes one rg_r128_analyze_tracks[_dynamics] / rg_r128_analyze_albums[_dynamics] call on
 * its share and the results go back to input order: bit for bit those of one context.  There is no exchange: an album is
 * never split.  dyn_out / albums_dyn_out may be NULL (both, for the albums): without dynamics.  rg_node_last_partition and
 * rg_node_tracks_error work as for rg_analyze_albums_node.  A node made by rg_node_create_backend has no R 128 entries:
 * RG_ERR_STATE. */
int rg_r128_analyze_tracks_node(rg_node *node, const char *const *paths, size_t n, int32_t track_index, int want_true_peak,
                                rg_r128_track_result *out, int32_t *status_out, rg_r128_dynamics *dyn_out);
int rg_r128_analyze_albums_node(rg_node *node, const char *const *paths, size_t n, const size_t *album_first, size_t n_albums,
                                int32_t track_index, int want_true_peak, rg_r128_track_result *tracks_out, int32_t *status_out,
                                rg_r128_album_result *albums_out, int32_t *album_status_out, rg_r128_dynamics *dyn_out,
                                rg_r128_dynamics *albums_dyn_out);

#ifdef __cplusplus
}
#endif
#endif /* MP3RGAIN_AMD_R128_H */
