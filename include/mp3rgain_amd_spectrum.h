/* mp3rgain_amd_spectrum.h -- spectral scan on the GPU: per channel the long-term power spectrum in 256 bands and, derived from
 * it on the host, the frequency above which there is nothing, the steepness of the edge there, and flags, from the planes the
 * file route has put into the analysis arena -- one decode, on the device, one more read of every sample, and a fixed-size
 * record per file comes back.
 *
 * rg_flac_verify, rg_mp3_verify, rg_rip_checksums and rg_pcm_stats all pass a FLAC that was transcoded from a 128 kb/s MP3, or
 * a 96 kHz file that was upsampled from a CD.  A lossy encoder's low-pass, or a resampler's, leaves a steep edge in the
 * spectrum with nothing but quantisation noise above it; this call reports where that edge is.
 *
 * DEFINITIONS (the contract).  A plane is one channel of one track: N samples, N < 2^32, sample rate fs, in one of the three
 * arena formats.
 *
 * Sample value  An integer sample v in a container of width W (16 or 32) becomes (float)v * 2^-(W-1): exact for S16 and for up
 *               to 24 bits in S32, otherwise the one rounding of the int -> float conversion.  A float sample is taken as it is.
 * Frames        L = 4096 (RG_SPEC_FRAME), hop H = 2048 (RG_SPEC_HOP).  K = 0 when N < L, otherwise K = (N - L) / H + 1 (integer
 *               division): the tail that fills no frame is not analysed and nothing is padded.  Frame k holds samples
 *               kH .. kH + L - 1 times the periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / L), a float table computed in
 *               double and rounded once.  A frame of a float plane that holds a NaN or Inf is skipped and counted in
 *               skipped_frames: it contributes nothing, and it does not disturb any other frame.
 * Band energy   P_k[b] = |X_k[b]|^2 for bins b = 1 .. 2048 of the frame's 4096-point DFT; bin 0 is dropped.  Band j,
 *               0 <= j < 256 (RG_SPEC_BANDS), holds bins 8j + 1 .. 8j + 8.  E[j] is the sum of P_k[b] over the analysed frames
 *               (the K frames less the skipped ones) and the band's bins, accumulated in double; p[j] = E[j] / (8 * analysed
 *               frames).
 * Verdict       one function in plain double on the host (rg_spectrum_verdict), the same code for every route.  Options
 *               rg_spectrum_opts {edge_db, min_cutoff_hz}, both > 0; NULL means {30, 4000} (RG_SPEC_EDGE_DB,
 *               RG_SPEC_MIN_CUTOFF_HZ).  Fixed: w = 8 bands, floor = max_j p[j] * 1e-12.  For every j with
 *               w - 1 <= j <= 255 - w whose upper edge f_hi(j) = (8j + 8.5) * fs / L is >= min_cutoff_hz:
 *                 below(j) = the mean of p[j-w+1 .. j]
 *                 above(j) = max(the mean of p[j+1 .. j+w], floor)
 *                 D(j)     = 10 log10(below / above)
 *               j qualifies when D(j) >= edge_db and max(max p[j+1 .. 255], floor) <= below(j) * 10^(-edge_db / 10): nothing
 *               comes back above the edge.  The cutoff is the qualifying j with the largest D, the lowest j on a tie; then
 *               cutoff_hz = f_hi(j) and edge_db = D(j).  When no j qualifies, cutoff_hz = fs / 2 and edge_db = 0.  A plane with
 *               no analysed frame or with max p == 0 has no verdict: cutoff_hz = 0, edge_db = 0, no flag.
 * Channel flags RG_SPEC_BANDLIMITED: a cutoff was found.  RG_SPEC_UPSAMPLED: bandlimited, fs >= 64000 and cutoff_hz <= 24500.
 * Track flags   the OR of the channel flags, plus RG_SPEC_SHORT (K = 0), RG_SPEC_NONFINITE (some frame was skipped) and
 *               RG_SPEC_COMPLETE (dropped_frames == 0, as in the stats record).  The track's cutoff_hz is the maximum over its
 *               channels.
 *
 * THE 30 dB, THE 4000 Hz, w = 8 AND THE 24500 Hz ARE A CONVENTION OF THIS HEADER.  NOBODY CHECKED THEM AGAINST ANOTHER TOOL OR
 * AGAINST REAL TRANSCODES; they were tried on synthetic noise only.  A CD master that its own mastering chain low-passed at
 * 20 kHz reads BANDLIMITED at 20 kHz, which is why the call reports the frequency and leaves the interpretation to the user.
 *
 * Not here: a spectrogram, time-varying detection (the holes an MP3's highest scalefactor band leaves), naming the codec or
 * bitrate, the node and multi-GPU calls.  Nothing is written to files.
 */
#ifndef MP3RGAIN_AMD_SPECTRUM_H
#define MP3RGAIN_AMD_SPECTRUM_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SPEC_BANDLIMITED 1u
#define RG_SPEC_UPSAMPLED   2u
#define RG_SPEC_SHORT       4u
#define RG_SPEC_NONFINITE   8u
#define RG_SPEC_COMPLETE   16u
#define RG_SPEC_MAX_CHANNELS 8u
#define RG_SPEC_FRAME 4096u
#define RG_SPEC_HOP   2048u
#define RG_SPEC_BANDS 256u
#define RG_SPEC_EDGE_DB 30.0           /* the defaults of rg_spectrum_opts: see above */
#define RG_SPEC_MIN_CUTOFF_HZ 4000.0
#define RG_SPEC_UPSAMPLED_MIN_RATE 64000u
#define RG_SPEC_UPSAMPLED_MAX_CUTOFF_HZ 24500.0

typedef struct rg_spectrum_opts {
    double edge_db, min_cutoff_hz; /* both > 0 */
} rg_spectrum_opts;

typedef struct rg_spectrum_channel {
    double cutoff_hz, edge_db;
    uint32_t analysed_frames, skipped_frames;
    uint32_t flags;          /* RG_SPEC_BANDLIMITED, RG_SPEC_UPSAMPLED */
    uint32_t reserved;
} rg_spectrum_channel;       /* 32 bytes */

typedef struct rg_spectrum_result {
    int32_t status;          /* RG_OK, or why there are no numbers (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel                                          */
    uint32_t sample_rate;
    uint32_t channels;       /* ch[0 .. channels) are filled, the others zero                      */
    uint32_t format;         /* rg_sample_format of the planes                                     */
    uint32_t dropped_frames; /* frames the decode route dropped, as the stats record counts them   */
    double cutoff_hz;        /* the maximum over the channels                                      */
    rg_spectrum_channel ch[RG_SPEC_MAX_CHANNELS];
} rg_spectrum_result;        /* 40 + 8 * 32 = 296 bytes */

/* The files are decoded by the very route the analysis uses -- the same loaders, the same groups (tuning key 13), the device
 * FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0); no decoder command is run -- and transformed where the PCM
 * lies, in the analysis arena, by two kernels on the stream the decode ran on.  Inputs: RIFF/WAVE of 8, 16, 24 and 32-bit
 * integer and 32-bit float samples, native FLAC, and MPEG Layer III (as f32).  opts: NULL = the defaults.  bands_out may be
 * NULL; otherwise it holds n * 8 * 256 doubles, E[j] of channel c of file i at bands_out[(i * 8 + c) * 256 + j], zero for the
 * channels a file does not have and for a failing file.  A failing file fails alone: RG_ERR_IO (it cannot be opened),
 * RG_ERR_FORMAT (not such a stream, or more than 8 channels), its record zero apart from `status`.  A file with dropped frames
 * gets the numbers of what the route decoded, with dropped_frames set and RG_SPEC_COMPLETE clear.  RG_OK whenever the call
 * itself worked.  `out` and `bands_out` are byte for byte the same for tuning key 14 = 1 and 14 = 0. */
int rg_spectrum(rg_ctx *ctx, const char *const *paths, size_t n, const rg_spectrum_opts *opts, rg_spectrum_result *out, double *bands_out);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_SPEC_COMPLETE set.  bands_out as above, or NULL.
 *   route 0  the serial host twin in double: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' arithmetic on the host: the same f32 butterflies in the same order, the same tables, the same tile
 *            and fold order; `ctx` may be NULL.  Routes 1 and 2 give byte-equal records and bands.
 * A track needs only sample alignment.  RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not
 * sample-aligned, and for an option that is not > 0.  With a NULL ctx the error text is rg_last_error(NULL)'s. */
int rg_spectrum_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_spectrum_opts *opts, const void *arena,
                      size_t arena_bytes, rg_spectrum_result *out, double *bands_out);

/* The verdict alone, on a caller's 256 numbers: p[j], or E[j] -- the verdict depends on ratios only, apart from rounding.
 * out->analysed_frames = analysed_frames, skipped_frames = 0; cutoff_hz, edge_db and flags as defined above (all zero when
 * analysed_frames is 0 or every p[j] is 0).  RG_ERR_INVALID_ARG for a NULL pointer, sample_rate 0 or an option not > 0. */
int rg_spectrum_verdict(const double *p, uint32_t analysed_frames, uint32_t sample_rate, const rg_spectrum_opts *opts, rg_spectrum_channel *out);

/* Test seam: how the kernels cut a plane.  frame = L, hop = H, bands = 256, frames_per_tile = T: one block of the tile kernel
 * transforms frames tT .. tT + T - 1 of its plane, two at a time.  Any pointer may be NULL. */
int rg_spectrum_kernel_shape(uint32_t *frame, uint32_t *hop, uint32_t *bands, uint32_t *frames_per_tile);

/* Measurement hook (tools/spectrum_rate.py): `n` tracks of `frames` frames of 2 channels of `format`, filled on the device, each
 * at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of launches, `reps` rounds of: the two
 * spectrum kernels over all planes (kernel_ms[r], HIP events around the launches alone); then, when host_tracks > 0, route 2
 * over a host copy of the first `host_tracks` (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host band
 * records that differ from the kernels' in any byte (it must be 0).  `ctx` is an rg_ctx. */
int rg_spectrum_rate(void *ctx, size_t n, uint64_t frames, uint32_t format, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                     double *kernel_ms, double *host_ms, size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
