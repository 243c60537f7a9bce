/* mp3rgain_amd_key.h -- in which key is a track?  The musical key (one of 12 major and 12 minor keys) in two stages on the GPU:
 * the signal low-passed and decimated to 5 .. 10 kHz and a chroma row per 512 decimated samples (twelve integers, one per pitch
 * class, from 60 semitone bands C2 .. B6), then the rows summed and matched against the Krumhansl-Kessler key profiles, all in
 * integers.  The key field of a tagger or a DJ library otherwise takes a second decode of every file in another program.
 *
 * THE ESTIMATOR IS A CONVENTION OF THIS PROJECT, TRIED ON SYNTHETIC MATERIAL ONLY (chord progressions; see THE MEASUREMENTS
 * below).  NOBODY HAS COMPARED IT WITH ANOTHER KEY FINDER OR RUN IT ON REAL MUSIC.  A4 = 440 Hz, equal temperament.
 *
 * STAGE 1a: DECIMATION (the contract).  A track has N frames of PCM per channel, N < 2^32, at sample rate fs.
 *
 * Signal        The fingerprint's (mp3rgain_amd_fingerprint.h): x is one channel as it is, otherwise (ch0 + ch1) * 0.5f in f32.
 * Factor        D = floor(fs / 5000): 44100 -> 8, 48000 -> 9, 96000 -> 19, 192000 -> 38, 8000 -> 1; fd = fs / D lies in
 *               [5000, 10000).  D = 0 or D > RG_KEY_MAX_DECIM (80: up to 404999 Hz): the track gets RG_KEY_RATE (with RG_KEY_SHORT),
 *               no chroma, no key, and no error.
 * Filter        D = 1: y = x, M = N.  Otherwise a Blackman-windowed sinc of 16 D + 1 taps: half = 8 D, n = k - half,
 *               fc = 0.45 / D, h[k] = 2 fc sinc(2 fc n) (0.42 + 0.5 cos(pi n / half) + 0.08 cos(2 pi n / half)) with
 *               sinc(t) = sin(pi t) / (pi t), normalised to sum 1 in double on the host and then rounded to f32: one table per D
 *               (rg_key_filter), which the kernel, its host arithmetic and route 0 all read, so libm has no part in their
 *               agreement.
 * Output        M = N < 16 D + 1 ? 0 : (N - (16 D + 1)) / D + 1, and y[j] = sum over k = 0 .. 16 D of h[k] * x[j D + k] in f32,
 *               in ascending k from 0.0f, the multiplication and the addition rounded separately (no contraction).  "Valid"
 *               only: nothing is padded at the edges.
 *
 * STAGE 1b: CHROMA ROWS, on y as a mono f32 track at rate fd.
 *
 * Frames        L = 4096, hop 512, the periodic Hann table of the spectral scan; F = M < L ? 0 : (M - L) / 512 + 1.
 * Bands         60 semitone bands (RG_KEY_BANDS), C2 .. B6: e[s] = floor(440 * 2^((s - 33.5) / 12) * L / fd + 0.5), s = 0 .. 60,
 *               in double on the host, then forced to increase as rg_tempo_bands does: e[0] = max(e[0], 1),
 *               e[s] = max(e[s], e[s-1] + 1) (rg_key_bands).  The bands are valid when e[60] <= 2048, which every D in 1 .. 80
 *               meets.  E[n][s] is the f32 sum of |Y|^2 over bins e[s] .. e[s+1] - 1 of frame n's 4096-point DFT, in bin order.
 *               A frame in which some y is a NaN or Inf (a float track) has all energies 0 and is counted in nonfinite_frames.
 * Compression   q(E) is the tempo scan's: the IEEE-754 bit pattern of (E > 2^-16f ? E : 2^-16f), shifted right by 18: one step
 *               is 1/32 of an octave of power.  qmax[n] = max over s of q(E[n][s]).  The frame is SILENT when
 *               qmax[n] == q(2^-16f), and its row is 0 (a non-finite frame is silent).  Otherwise
 *               v[n][s] = max(0, q(E[n][s]) - (qmax[n] - R)), R = RG_KEY_RANGE = 160: five octaves of power, about 15 dB.
 * Row           c[n][p] = sum over o < 5 of v[n][12 o + p], a uint16, at most 800; p = 0 is C.  A row is all zero exactly when
 *               its frame is silent (the loudest band of any other frame has v = R).  FROM HERE ON NOTHING IS A FLOAT.
 * Routes        Route 0 is these definitions with the FIR sum, the transform and the band sums in double, each y and each E
 *               rounded to f32.  The kernels (route 1) and their arithmetic on the host (route 2) work in f32 (the fingerprint's
 *               tile walk on y): routes 1 and 2 give byte-equal y, band energies and rows; route 0 differs from them in a small
 *               share of row entries by a step of q (tests/golden/key_measured.json).
 *
 * STAGE 2: DEFINITIONS (all integer).  rg_key_opts {segment S}; NULL or 0 means RG_KEY_SEGMENT = 128 rows (about 12 s);
 * 8 <= S <= 4096.
 *
 * Histogram     H[p] = sum over n of c[n][p], u64.  F == 0: RG_KEY_SHORT.  H all zero: RG_KEY_NONE.
 * Scaling       sh is the smallest shift with max over p of (H[p] >> sh) < 65536, and h = H >> sh.
 * Profiles      Krumhansl-Kessler, zero mean, scaled to a norm of about 1000 (sum of squares 1000902 and 998654), the zero sum
 *               restored at the largest entry:   major {656, -286, -1, -263, 205, 139, -220, 390, -250, 41, -273, -138}
 *                                                minor {654, -257, -47, 418, -277, -45, -292, 260, 68, -255, -92, -135}
 * Score         score(mode, tonic) = sum over p of h[p] * P_mode[(p - tonic) mod 12], i64.  key = 12 mode + tonic, mode 0 =
 *               major.  The largest score wins (`best`), a tie to the smaller key; `second` is the largest score of the 23 others.
 * Confidence    Vh = 12 sum h^2 - (sum h)^2;  den = isqrt(floor(1000000 Vh / 12));  correlation_permille =
 *               clamp(floor(1000 best / den), 0, 1000): Pearson's r of h and the profile.  den == 0 (a flat H) or best <= 0:
 *               RG_KEY_NONE, key 0 and all three fields 0.  margin_permille = clamp(floor(1000 (best - second) / best), 0, 1000)
 *               (`second` may be negative, hence the clamp).
 *               Bounds: h < 2^16, so sum h^2 < 12 * 2^32 and Vh < 144 * 2^32 < 2^40, 1000000 Vh < 2^60; |score| <=
 *               65535 * sum |P| < 2^16 * 3200 < 2^28, 1000 |score| < 2^38, best - second < 2^29.  Everything fits i64.
 * Segments      Segment g is rows g S .. g S + S - 1 and exists while it is whole: G = floor(F / S).  A segment whose rows are
 *               not all zero picks its key from its own sums in the same way (its own sh); it AGREES when it has a key (no
 *               RG_KEY_NONE of its own) and that key is the track's.  stable_permille = floor(1000 * agreeing / non-zero
 *               segments), 0 when there are none or the track has no key.  `segments` is G.
 *
 * All of stage 2 is integer arithmetic: the serial host twin (route 0 of rg_key_from_chroma) and the finish kernel (route 1)
 * agree byte for byte.
 *
 * THE MEASUREMENTS (tools/key_refcheck.py, tests/golden/key_measured.json): chord progressions I-IV-V-I-vi-IV-V-I (minor:
 * i-iv-v-i-VI-iv-v-i) with a bass root, six harmonics at 1/k, a scale-tone melody, decaying envelopes and a little noise, 40 s
 * each, in all 24 keys at 44100, 48000 and 96000 Hz.  All 72 must read their generating key (a condition of the tests); the file
 * holds the ranges of correlation, margin and stability, the correlation of white noise, and how far route 2's y, band energies
 * and rows lie from a float64 restatement.
 *
 * RATES.  tools/key_rate.py on an MI355X (profiles/key_rate.json), 1000 tracks of 3 min of 16-bit stereo at 44.1 kHz (31.8 GB),
 * HIP events around the launches alone after a warm-up, medians of 5: the decimation kernel 18.3 ms = 1.73 TB/s of PCM (a
 * read-only pass over the same planes: 6.2 ms, so 34 % of its rate; the DR kernel reads the same planes in 5.7 ms); it is
 * bound by its tap loop, not by memory: 258 unfused multiply and add instructions and 129 four-byte LDS reads per output keep the
 * vector ALUs and the LDS busy at once, and about 200 instructions more stage the 8.5 sample pairs an output costs; two samples
 * per load over an aligned body were tried and gained nothing (DESIGN 12.12 has the account).  The tiles kernel 28.8 ms (the
 * fingerprint stage, with eight times the frames and 33 bands, takes 160 ms), the finish 0.08 ms; the three together 47 ms =
 * 3.8 million seconds of audio per second, 104 times route 2 on 16 host threads for stage 1 and 421 times the host's stage 2,
 * with no decimated sample, no row and no record different from the host's.
 *
 * Not here: tuning other than A4 = 440 Hz; key changes (only flagged, through stable_permille); modes other than major and
 * minor; the node and multi-GPU calls; agreement with any other key finder or with real music; using the decimated signal for
 * duplicates across sample rates.
 */
#ifndef MP3RGAIN_AMD_KEY_H
#define MP3RGAIN_AMD_KEY_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_KEY_SHORT      1u /* F == 0: no chroma row */
#define RG_KEY_RATE       2u /* D = 0 or D > 80: nothing was decimated */
#define RG_KEY_NONFINITE  4u /* some frame held a NaN or Inf */
#define RG_KEY_COMPLETE   8u /* dropped_frames == 0 */
#define RG_KEY_NONE      16u /* H all zero, flat, or no positive score */

#define RG_KEY_MAX_CHANNELS 8u
#define RG_KEY_FRAME 4096u
#define RG_KEY_HOP    512u
#define RG_KEY_BANDS   60u
#define RG_KEY_CHROMA  12u
#define RG_KEY_RANGE  160u
#define RG_KEY_TARGET_RATE 5000u
#define RG_KEY_MAX_DECIM 80u
#define RG_KEY_TAPS_PER_DECIM 16u /* the filter has 16 D + 1 taps */
#define RG_KEY_SEGMENT 128u      /* the default of rg_key_opts */
#define RG_KEY_MIN_SEGMENT 8u
#define RG_KEY_MAX_SEGMENT 4096u
#define RG_KEY_ROW_MAX 800u

typedef struct rg_key_opts {
    uint32_t segment; /* 0 = the default */
} rg_key_opts;

typedef struct rg_key_result {
    int32_t status;            /* RG_OK, or why there is no reading (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;           /* N: PCM frames per channel                                          */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;           /* rg_sample_format of the planes                                     */
    uint32_t dropped_frames;   /* frames the decode route dropped, as the stats record counts them   */
    uint32_t decim;            /* D (0 with RG_KEY_RATE)                                             */
    uint32_t decimated;        /* M                                                                  */
    uint32_t rows;             /* F                                                                  */
    uint32_t silent_rows;      /* rows that are all zero                                             */
    uint32_t nonfinite_frames;
    uint32_t key;              /* 12 mode + tonic; meaningful without SHORT, RATE and NONE           */
    uint32_t tonic;            /* 0 = C .. 11 = B                                                    */
    uint32_t mode;             /* 0 = major, 1 = minor                                               */
    uint32_t correlation_permille;
    uint32_t margin_permille;
    uint32_t segments;         /* G                                                                  */
    uint32_t stable_permille;
    uint64_t chroma_at;        /* where the track's rows start in chroma_out, in rows of 12          */
} rg_key_result;               /* 88 bytes */

/* The decimation factor and the band edges of a rate: *decim = D, edges[0 .. 60] (for fd = fs / D).  RG_ERR_UNSUPPORTED_RATE
 * (*decim still set, the edges untouched) when D = 0 or D > 80, RG_ERR_INVALID_ARG for a NULL pointer or rate 0.  Plain host
 * arithmetic in double. */
int rg_key_bands(uint32_t sample_rate, uint32_t *decim, uint32_t *edges);

/* The filter of factor D, 2 <= D <= 80: taps[0 .. 16 D].  RG_ERR_INVALID_ARG otherwise. */
int rg_key_filter(uint32_t decim, float *taps);

/* The files (RIFF/WAVE, native FLAC, MPEG Layer III) are decoded by the very route the analysis uses and both stages run where
 * the PCM lies.  out[i]: the file's record.  chroma_out may be NULL; otherwise it holds chroma_cap rows of 12 and receives file
 * i's rows at out[i].chroma_at, as many files as fit whole in the order the groups ran (a file that did not fit, and every file
 * when chroma_out is NULL, has chroma_at = UINT64_MAX).  A failing file fails alone (RG_ERR_IO, RG_ERR_FORMAT; its record zero
 * apart from `status`).  RG_OK whenever the call itself worked.  The records are byte for byte the same for tuning key 14 = 1
 * and 0. */
int rg_key(rg_ctx *ctx, const char *const *paths, size_t n, const rg_key_opts *opts, rg_key_result *out, uint16_t *chroma_out, size_t chroma_cap);

/* Test seam, both stages: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32
 * frames: anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_KEY_COMPLETE set.  All three arrays may be NULL and
 * are packed in track order: decim_out holds the sum of M floats (y), bands_out the sum of F rows of 60 floats, chroma_out the
 * sum of F rows of 12.
 *   route 0  the serial host twin, the FIR sum and the transform in double; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' arithmetic on the host, and the host's stage 2; `ctx` may be NULL.
 *            Routes 1 and 2 give byte-equal records, y, bands and rows.
 * RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not sample-aligned, or an option out of range. */
int rg_key_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_key_opts *opts,
                 rg_key_result *out, float *decim_out, float *bands_out, uint16_t *chroma_out);

/* Test seam, stage 2, on constructed rows: track t has counts[t] rows of 12 (each entry at most 800, fewer than 2^32 / 512 rows),
 * packed in track order in `chroma`.  out[t]: the stage-2 fields (rows, silent_rows, key .. stable_permille, chroma_at), with
 * frames, rate, channels, format, decim and decimated 0.  Route 0 is the host (`ctx` may be NULL), route 1 the finish kernel. */
int rg_key_from_chroma(void *ctx, int route, size_t n, const uint32_t *counts, const uint16_t *chroma, const rg_key_opts *opts, rg_key_result *out);

/* Test seam: how the kernels cut their work.  One workgroup of decim_lanes lanes makes decim_outputs consecutive y of a track;
 * tile_rows = T: one workgroup of tile_lanes lanes makes rows tT + 1 .. tT + T (tile 0: row 0 too) from T + 1 frames, two per
 * transform, in tile_lds_bytes of LDS.  Any pointer may be NULL. */
int rg_key_kernel_shape(uint32_t *decim_outputs, uint32_t *decim_lanes, uint32_t *tile_rows, uint32_t *tile_lanes, uint32_t *tile_lds_bytes);

/* Measurement hook (tools/key_rate.py): `n` tracks of `frames` frames of 2 channels of S16 at 44100 Hz, filled on the device.
 * After a warm-up of `warm_ms` milliseconds, `reps` rounds of: the decimation kernel over all tracks (decim_ms[r]), a read-only
 * pass over the same planes (read_ms[r]), the tiles kernel (tiles_ms[r]) and the finish kernel (finish_ms[r]) at `opts`, HIP
 * events around the launches alone; when host_tracks > 0, route 2 over the first host_tracks tracks and the host's stage 2 on
 * `threads` host threads (host_stage1_ms[r], host_finish_ms[r]).  *mismatches: y, rows or records of those tracks that differ
 * (must be 0). */
int rg_key_rate(void *ctx, size_t n, uint64_t frames, const rg_key_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                double *decim_ms, double *read_ms, double *tiles_ms, double *finish_ms, double *host_stage1_ms, double *host_finish_ms, size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
