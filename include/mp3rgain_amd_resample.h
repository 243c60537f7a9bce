/* mp3rgain_amd_resample.h -- duplicates across sample rates.  The duplicate finder (mp3rgain_amd_fingerprint.h) compares two
 * files only when their rates are equal: its band edges depend on the rate and a code step is 512 samples of whatever rate the
 * file has.  Here every track is first brought to one common rate, 11025 Hz, by a rational (L/M) polyphase resampler on the
 * GPU; the fingerprint's stage 1 then runs on the resampled signal as a mono f32 track at 11025 Hz, and the match is the
 * existing stage 2, unchanged, with every track's rate given as 11025.  So the CD rip at 44.1 kHz, the 48 / 96 / 192 kHz
 * download of the same master and an 8 kHz telephone copy land in one group.
 *
 * THE RESAMPLER: DEFINITIONS (the contract).  The common rate is fc = 11025 Hz (RG_RS_RATE_OUT).  A track has N frames, N < 2^32,
 * at rate fs.
 *
 * Ratio         g = gcd(fs, fc), L = fc / g, M = fs / g.
 * Supported     fs >= 8000, L <= 441 (RG_RS_MAX_PHASES) and M <= 32 L: 8, 16, 22.05, 24, 32, 37.8, 44.1, 48, 64, 88.2, 96, 176.4,
 *               192 and 352.8 kHz among others; not 384000 Hz (M > 32 L), not 44056 Hz (L = 11025).  An unsupported track gets
 *               RG_RS_RATE, no output, and no error.
 * Signal        The fingerprint's: one channel as it is, otherwise (ch0 + ch1) * 0.5f in f32; only the first two channels count.
 * Identity      L = M = 1: y = x, M_out = N (P = 1, the single tap 1).
 * Prototype     Otherwise W = max(L, M), half = 8 W, c = 0.45 / W, and for |n| <= half
 *               G[n] = 2c sinc(2c n) (0.42 + 0.5 cos(pi n / half) + 0.08 cos(2 pi n / half)), sinc(t) = sin(pi t) / (pi t); 0 beyond.
 * Window        Output j reads x from b_j = ceil(j M / L) on, at phase p_j = b_j L - j M in [0, L), P = floor(2 half / L) + 1 taps.
 *               j M is formed in 64 bits everywhere.
 * Tap table     h[p][k] = G[p + k L - half], k = 0 .. P - 1 (0 where the argument leaves +-half); each phase is normalised to sum
 *               1 in double on the host, then rounded to f32 (rg_resample_filter: taps[p * P + k]).  One table per (L, M); the
 *               kernel, its host arithmetic and route 0 all read it, so libm has no part in their agreement.
 * Output        y[j] = sum over k = 0 .. P - 1 of h[p_j][k] x[b_j + k], in f32, in ascending k from 0.0f, the multiplication and
 *               the addition rounded separately (no contraction).
 * Count         "Valid" only: M_out is the number of j >= 0 with b_j + P <= N: 0 when N < P, otherwise
 *               floor((N - P) L / M) + 1.  Nothing is padded.  (A track whose M_out would reach 2^32 is RG_ERR_FORMAT.)
 * Key scan      For L = 1 this is exactly the key scan's decimation of factor D = M (mp3rgain_amd_key.h: 16 D + 1 taps, fc
 *               0.45 / D, y[j] = sum h[k] x[j D + k]): rg_resample_filter(1, D) equals rg_key_filter(D) byte for byte, and on the
 *               device the L = 1 tracks of a launch go through the key scan's decimation kernel, not a copy of it.
 * Routes        Route 0: these definitions with the sum in double, each y rounded to f32.  Route 1: the kernels.  Route 2: the
 *               kernels' arithmetic on the host.  Routes 1 and 2 give byte-equal y and records.
 *
 * THE CROSS-RATE FINGERPRINT.  Stage 1 of mp3rgain_amd_fingerprint.h (frames of 4096, hop 512, 33 bands, codes) on y as a mono
 * f32 track at 11025 Hz: the edges are rg_fingerprint_edges(11025), one set for every track, and a code step is 512 / 11025 s
 * (46.4 ms) for every file.  F, K, the codes and the band energies are what rg_fingerprint_arena gives for y.
 *
 * THE CROSS-RATE MATCH.  Stage 2 of that header with every rate given as 11025.  NULL or a zero field of rg_fingerprint_opts
 * means the default of THIS call, {block 64, probes 8, radius 128, max_ber_permille RG_XR_MAX_BER_PERMILLE}: about 3 s blocks
 * and +-5.9 s, close in seconds to the same-rate finder's 256 / 512 codes at 44.1 kHz.  A file needs K >= block codes (about
 * 3.4 s at the default) to take part in a pair.
 *
 * THE THRESHOLD.  tools/xrate_refcheck.py --record measured it (tests/golden/xrate_measured.json) on: the 20 seeds of the
 * same-rate finder's material (tests/fingerprint_cases.py) with its degradations at 44100 Hz, and copies of each seed resampled
 * to 48000 and 96000 Hz; and continuous-time pieces (decaying harmonic notes, rendered to 16 bits) at 44100, 48000, 96000, 32000,
 * 22050 and 8000 Hz, one of them again delayed by 133.7 ms.  The figures, and which degradation (if any) had to be left out of
 * the same-recording set, are under MEASURED below.  NOBODY HAS TRIED THIS ON REAL MUSIC OR A REAL LIBRARY.
 *
 * MEASURED (tests/golden/xrate_measured.json).  At the call's defaults the largest best-lag bit error rate over same-recording
 * pairs across rates was 179 per mille (a 64 kb/s stream of the project's encoder against the 48 and 96 kHz copies of its
 * original; the coarse codings 162 .. 176; the clean renderings of a piece at six rates 3 .. 13, the delayed one 20 .. 25), the
 * smallest over unrelated pairs 428 per mille; RG_XR_MAX_BER_PERMILLE = 303 is the rounded midpoint and no degradation had to be
 * left out.  Every same-recording pair's lag was one of the two whole codes next to the true shift; 22 pairs of coded copies,
 * whose 1057 samples of delay are 0.516 codes, took the farther of the two.  y of route 2 differs from a float64 restatement by
 * at most 4.4e-7 of a track's largest |y|; 0.45 per mille of the code bits differ between route 0 and route 2.
 *
 * RATES.  tools/resample_rate.py on an MI355X (profiles/resample_rate.json), 1000 tracks of 3 min of 16-bit stereo, HIP events
 * around the launches alone after a warm-up, medians of 5: at 48 kHz (L = 147, M = 640, 70 taps) the resampler kernel 31.8 ms =
 * 1.09 TB/s of PCM (a read-only pass over the same planes is 20 % of it; 179 times route 2 on 16 host threads); at 44.1 kHz
 * (L = 1: the key scan's decimation kernel at D = 4, 65 taps) 43.2 ms, beside that kernel's 18.3 ms at the key scan's D = 8;
 * no sample different from the host's.  The tap table is read from L2, not staged in LDS: DESIGN 12.13.
 *
 * Not here: time-stretched or pitch-shifted copies; excerpts offset by more than the radius; the node and multi-GPU calls;
 * rates outside the supported set; resampled audio as an output format (y is a test seam's by-product, band-limited to
 * 0.45 of the lower rate and "valid" only: 8 W / M samples shorter at either end than the input's duration); any change to
 * rg_same_recording, its defaults or its records; compatibility with any other resampler's output.
 */
#ifndef MP3RGAIN_AMD_RESAMPLE_H
#define MP3RGAIN_AMD_RESAMPLE_H

#include "mp3rgain_amd.h"
#include "mp3rgain_amd_fingerprint.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_RS_SHORT 1u /* M_out = 0 (the cross-rate record: K = 0) */
#define RG_RS_RATE  2u /* the rate is not supported: no output     */

#define RG_RS_RATE_OUT   11025u
#define RG_RS_MAX_PHASES   441u /* L at most                        */
#define RG_RS_MAX_RATIO     32u /* M <= 32 L                        */
#define RG_RS_MIN_RATE    8000u
#define RG_RS_HALF_PER_W     8u /* half = 8 max(L, M)               */
#define RG_RS_MAX_CHANNELS   8u

#define RG_XR_BLOCK   64u /* the defaults of rg_same_recording_xrate */
#define RG_XR_PROBES   8u
#define RG_XR_RADIUS 128u
#define RG_XR_MAX_BER_PERMILLE 303u

typedef struct rg_resample_result {
    int32_t status;
    uint32_t flags;            /* RG_RS_*                                                  */
    uint64_t frames;           /* N                                                        */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;
    uint32_t up;               /* L (still set with RG_RS_RATE)                            */
    uint32_t down;             /* M                                                        */
    uint32_t taps;             /* P (0 with RG_RS_RATE)                                    */
    uint32_t resampled;        /* M_out                                                    */
    uint32_t reserved;
    uint64_t y_at;             /* where the track's y starts in y_out, in floats           */
} rg_resample_result;          /* 56 bytes */

typedef struct rg_xrate_result {
    int32_t status;            /* rg_fingerprint_result's fields, for y at 11025 Hz ...    */
    uint32_t flags;            /* RG_FP_* (RG_FP_RATE is RG_RS_RATE)                       */
    uint64_t frames;           /* N of the file, at its own rate                           */
    uint32_t sample_rate;      /* the file's own                                           */
    uint32_t channels;
    uint32_t format;
    uint32_t dropped_frames;
    uint32_t fp_frames;        /* F of y                                                   */
    uint32_t codes;            /* K                                                        */
    uint32_t nonfinite_frames;
    uint32_t group;
    uint32_t matches;
    uint32_t reserved;
    uint64_t codes_at;
    uint64_t frames_at;
    uint32_t up;               /* ... plus L,                                              */
    uint32_t down;             /* M                                                        */
    uint32_t resampled;        /* and M_out                                                */
    uint32_t reserved2;
    uint64_t y_at;             /* the seam: where the track's y starts in y_out, in floats */
} rg_xrate_result;             /* 96 bytes */

/* The ratio and the taps per phase of a rate: *up = L, *down = M, *taps = P.  RG_ERR_UNSUPPORTED_RATE (L and M still set,
 * *taps = 0) for a rate outside the supported set, RG_ERR_INVALID_ARG for a NULL pointer or rate 0.  Plain host arithmetic. */
int rg_resample_plan(uint32_t sample_rate, uint32_t *up, uint32_t *down, uint32_t *taps);

/* The tap table of (L, M), coprime, L <= 441, M <= 32 L: taps[p * P + k] = h[p][k], L * P floats (L = M = 1: the one tap 1).
 * RG_ERR_INVALID_ARG otherwise. */
int rg_resample_filter(uint32_t up, uint32_t down, float *taps);

/* The window of output j at a supported rate: *first = b_j, *phase = p_j.  j M is formed in 64 bits: any j < 2^32 is taken. */
int rg_resample_window(uint32_t sample_rate, uint64_t j, uint64_t *first, uint32_t *phase);

/* Test seam: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32 frames:
 * anything else is RG_ERR_FORMAT), resampled to 11025 Hz.  y_out (may be NULL) holds the sum of M_out floats, packed in track
 * order (out[i].y_at).
 *   route 0  the definitions with the sum in double; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' arithmetic on the host; `ctx` may be NULL.  Routes 1 and 2 give byte-equal records and y.
 * RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not sample-aligned. */
int rg_resample_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_resample_result *out,
                      float *y_out);

/* Test seam: the resampler and stage 1 of the fingerprint on y.  codes_out (may be NULL) holds the sum of K codes, bands_out (may
 * be NULL) the sum of F frames of 33 floats, y_out (may be NULL) the sum of M_out floats, all packed in track order.  Routes as
 * above (route 0: y of route 0, then the fingerprint's route 0); out[i].group = i, matches = 0, dropped_frames = 0. */
int rg_xrate_fingerprint_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_xrate_result *out,
                               uint32_t *codes_out, float *bands_out, float *y_out);

/* The files (RIFF/WAVE, native FLAC, MPEG Layer III) are decoded by the very route the analysis uses, resampled and
 * fingerprinted where the PCM lies; the codes stay on the device from group to group and one match runs after the last group.
 * Everything else is rg_same_recording's: pairs, *n_pairs, codes_out and codes_cap, a failing file failing alone, the records
 * byte for byte the same for tuning key 14 = 1 and 0.  pairs[].lag is in codes of 512 / 11025 s. */
int rg_same_recording_xrate(rg_ctx *ctx, const char *const *paths, size_t n, const rg_fingerprint_opts *opts, rg_xrate_result *out,
                            rg_fingerprint_pair *pairs, size_t max_pairs, size_t *n_pairs, uint32_t *codes_out, size_t codes_cap);

/* Test seam: how the kernel cuts its work.  One workgroup of `lanes` lanes makes `outputs` consecutive y of a track from at
 * most max_span staged samples (LDS: 4 max_span bytes at most).  Any pointer may be NULL. */
int rg_resample_kernel_shape(uint32_t *outputs, uint32_t *lanes, uint32_t *max_span);

/* Measurement hook (tools/resample_rate.py): `n` tracks of `frames` frames of 2 channels of S16 at `sample_rate`, filled on the
 * device.  After a warm-up of `warm_ms` milliseconds, `reps` rounds of: the resampler's launches over all tracks (resample_ms[r])
 * and a read-only pass over the same planes (read_ms[r]), HIP events around the launches alone; when host_tracks > 0, route 2
 * over the first host_tracks tracks on `threads` host threads (host_ms[r]).  *mismatches: tracks among those whose y differs
 * (must be 0). */
int rg_resample_rate(void *ctx, size_t n, uint64_t frames, uint32_t sample_rate, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                     double *resample_ms, double *read_ms, double *host_ms, size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
