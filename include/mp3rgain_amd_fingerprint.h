/* mp3rgain_amd_fingerprint.h -- which files of a library are the same recording?  Two stages on the GPU: a fingerprint per track
 * (a sub-band-difference code per 512 samples, from the planes the file route has put into the analysis arena), and a match of
 * every pair of tracks of a call at every lag within a radius, by Hamming distance.  rg_rip_checksums finds bit-identical PCM
 * only; this finds the same audio after a lossy codec, a gain change, some samples of encoder delay or a second of silence in
 * front.  The match stage is quadratic in the number of tracks and exact: every pair, every lag, no index and no heuristic.
 *
 * THE FINGERPRINT IS A CONVENTION OF THIS PROJECT.  It follows the idea of Haitsma and Kalker's sub-band-difference code, with
 * frames, bands and rounding of its own, and it is COMPATIBLE WITH NO OTHER FINGERPRINT: not with Chromaprint or AcoustID, not
 * with the original Philips system.  Codes are comparable only with codes this header's calls made.
 *
 * STAGE 1: DEFINITIONS (the contract).  A track has N frames of PCM per channel, N < 2^32, at sample rate fs.
 *
 * Signal        One channel: that channel.  Two or more: x = (ch0 + ch1) * 0.5f in f32, the sample values as the spectral scan
 *               defines them ((float)v * 2^-(W-1) for an integer of container width W, a float as it is); only the first two
 *               channels count, as in the gain analysis.
 * Frames        L = 4096 (RG_FP_FRAME), hop H = 512 (RG_FP_HOP), the periodic Hann table of the spectral scan.  F = 0 when
 *               N < L, otherwise F = (N - L) / 512 + 1.  A frame of a float track in which some x is a NaN or Inf has all band
 *               energies 0 and is counted in nonfinite_frames (the code bits next to it follow from those zeros).
 * Bands         33 bands (RG_FP_BANDS) between 300 and 2000 Hz, logarithmically spaced: the edges are
 *               e[m] = floor(300 * (2000/300)^(m/33) * L / fs + 0.5), m = 0 .. 33, computed in double on the host
 *               (rg_fingerprint_edges).  Band m is bins e[m] .. e[m+1] - 1 of the frame's 4096-point DFT; E[n][m] is the f32 sum
 *               of |X|^2 over them in bin order.  A rate is supported when the edges strictly increase and e[33] <= 2048: every
 *               rate from 4000 to 74372 Hz is (at 44100 and 48000 the narrowest band is one bin), and so is 88200 Hz; from
 *               74373 Hz up two edges can round to the same bin, and 96000 Hz is among the rates that fail.  A track at an
 *               unsupported rate gets RG_FP_RATE, no code, and no error.
 * Codes         K = max(F - 1, 0) codes of 32 bits.  Bit m of code n (n = 1 .. F-1, m = 0 .. 31; stored at index n - 1) is 1 when
 *               (E[n][m] - E[n][m+1]) - (E[n-1][m] - E[n-1][m+1]) > 0, in f32 in exactly that order.
 * Routes        Route 0 is these definitions in double.  The kernels (route 1) and their arithmetic on the host (route 2) work
 *               in f32, two frames per complex transform, a tile of 7 codes per workgroup whose first frame is the last
 *               of the tile before: routes 1 and 2 give byte-equal codes and band energies; route 0 differs from them in a small
 *               share of bits, each where the reference's margin is tiny (tests/golden/fingerprint_measured.json).
 *
 * STAGE 2: DEFINITIONS.  Inputs: the code arrays of n tracks with their rates, and rg_fingerprint_opts {block, probes, radius,
 * max_ber_permille}; NULL or a zero field means the default {256, 8, 512, RG_FP_MAX_BER_PERMILLE}.  1 <= block <= 4096,
 * 1 <= probes <= 64, 1 <= radius <= 2047 (512 codes are about +-6 s at 44.1 kHz), 1 <= max_ber_permille <= 1000.
 *
 * Compared      A pair (i, j), i < j, is compared when both rates are equal and supported and both have K >= block; otherwise
 *               it gets RG_FP_PAIR_SKIPPED.  The probe side a is the track with fewer codes, on a tie the lower index
 *               (RG_FP_PAIR_PROBE_J when it is j); b is the other.
 * Probes, lags  Probe p starts at s_p = (2p + 1)(K_a - block) / (2 probes), integer division.  Lags d run from -radius to radius.
 *               Probe p counts at lag d when 0 <= s_p + d and s_p + d + block <= K_b; its distance is the sum over i < block of
 *               popcount(A[s_p + i] ^ B[s_p + d + i]).  A lag qualifies when at least ceil(probes / 2) probes count; errors(d)
 *               and bits(d) are the sums over the counting probes (32 block bits each).
 * Best lag      The qualifying lag with the smallest errors / bits, compared by 64-bit cross-multiplication; on a tie the smaller
 *               |d|, then the negative d.  No qualifying lag: RG_FP_PAIR_SKIPPED.  lag = d: B runs d codes (512 d samples)
 *               behind A.
 * Match         errors * 1000 <= bits * max_ber_permille: RG_FP_PAIR_MATCH.  All of it is integer arithmetic: the serial host
 *               twin (route 0) and the kernel (route 1) agree byte for byte.
 * Groups        The matching pairs joined by a union-find: a file's group is the smallest index of its component.
 *
 * THE THRESHOLD.  tools/fingerprint_refcheck.py measured it on this project's own material (tests/golden/
 * fingerprint_measured.json): 20 seeds of synthetic music of 6.5 s, each with copies degraded by the project's coarse MP3-like
 * coding (tests/ancestry_cases.short_cut, zero shares 0.5 and 0.8, 1057 samples of delay), white noise at 20 dB SNR, -6 dB of
 * gain, 16-bit quantisation, leading trims of 137, 256 and 1105 samples and 1 s of silence in front, alone and in two
 * combinations; four of the seeds also as a real stream of the project's own MP3 encoder (128 and 64 kb/s), decoded by this
 * library.  At the default block, probes and radius the largest best-lag bit error rate over same-recording pairs was 167 per
 * mille (a copy trimmed by 256 samples, half a hop, against a coarsely coded one; 39 and 82 per mille for the 128 and 64 kb/s
 * streams against their originals), the smallest over unrelated pairs 466 per mille, every same-recording pair at its expected
 * lag, and no degradation had to be dropped; RG_FP_MAX_BER_PERMILLE = 316 is the rounded midpoint.  Over the 4.4 million code
 * bits of that material the kernels' f32 arithmetic flipped none against the float64 reference; the band energies differ from
 * it by at most 3e-7 of a frame's largest band.  NOBODY HAS TRIED THIS ON REAL MUSIC, A REAL LIBRARY OR ANOTHER ENCODER: all
 * seeds share the generator (and two steady tones), which the unrelated reading reflects.
 *
 * RATES.  tools/fingerprint_rate.py on an MI355X (profiles/fingerprint_rate.json), 1000 tracks of 3 min of 16-bit stereo, HIP
 * events around the launches alone after a warm-up, medians of 5: the fingerprint kernels 160 ms (119 times route 2 on 16 host
 * threads; a read-only pass over the same planes is 4 % of it), the match kernel over all 499500 pairs at the defaults 92 ms =
 * 1.1e13 word operations per second (249 times the host match on 16 threads, 43.7 % of the integer vector peak at three
 * operations per word), with no code and no pair record different from the host's.
 *
 * Not here: matching across sample rates; rates from 96 kHz up; time-stretched or pitch-shifted copies; excerpts offset by
 * more than the radius; the node and multi-GPU calls; any index kept between calls; compatibility with Chromaprint or AcoustID.
 */
#ifndef MP3RGAIN_AMD_FINGERPRINT_H
#define MP3RGAIN_AMD_FINGERPRINT_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_FP_SHORT      1u /* K = 0: fewer than L + H samples */
#define RG_FP_RATE       2u /* the rate is not supported: no code */
#define RG_FP_NONFINITE  4u /* some frame held a NaN or Inf */
#define RG_FP_COMPLETE   8u /* dropped_frames == 0 */

#define RG_FP_PAIR_COMPARED 1u
#define RG_FP_PAIR_MATCH    2u
#define RG_FP_PAIR_SKIPPED  4u
#define RG_FP_PAIR_PROBE_J  8u

#define RG_FP_MAX_CHANNELS 8u
#define RG_FP_FRAME 4096u
#define RG_FP_HOP    512u
#define RG_FP_BANDS   33u
#define RG_FP_BLOCK  256u /* the defaults of rg_fingerprint_opts */
#define RG_FP_PROBES   8u
#define RG_FP_RADIUS 512u
#define RG_FP_MAX_BER_PERMILLE 316u
#define RG_FP_MAX_BLOCK  4096u
#define RG_FP_MAX_PROBES   64u
#define RG_FP_MAX_RADIUS 2047u

typedef struct rg_fingerprint_opts {
    uint32_t block, probes, radius, max_ber_permille; /* 0 = the default */
} rg_fingerprint_opts;

typedef struct rg_fingerprint_result {
    int32_t status;            /* RG_OK, or why there is no fingerprint (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;           /* N: PCM frames per channel                                          */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;           /* rg_sample_format of the planes                                     */
    uint32_t dropped_frames;   /* frames the decode route dropped, as the stats record counts them   */
    uint32_t fp_frames;        /* F (0 at an unsupported rate)                                       */
    uint32_t codes;            /* K                                                                  */
    uint32_t nonfinite_frames;
    uint32_t group;            /* rg_same_recording: the smallest index of the file's component; the seam: the track's index */
    uint32_t matches;          /* rg_same_recording: matching pairs this file is part of             */
    uint32_t reserved;
    uint64_t codes_at;         /* where the track's codes start in codes_out, in codes               */
    uint64_t frames_at;        /* where its band energies start in bands_out, in frames of 33 floats */
} rg_fingerprint_result;       /* 72 bytes */

typedef struct rg_fingerprint_pair_record {
    uint32_t errors, bits;
    int32_t lag;
    uint32_t flags;            /* RG_FP_PAIR_* */
} rg_fingerprint_pair_record;  /* 16 bytes */

typedef struct rg_fingerprint_pair {
    uint32_t i, j, errors, bits;
    int32_t lag;               /* of the longer track against the shorter, in codes of 512 samples */
    uint32_t flags;
} rg_fingerprint_pair;         /* 24 bytes */

/* The band edges of a rate: edges[0 .. 33].  RG_ERR_UNSUPPORTED_RATE (edges still filled) when they do not strictly increase or
 * e[33] > 2048, RG_ERR_INVALID_ARG for a NULL pointer or rate 0.  Plain host arithmetic in double. */
int rg_fingerprint_edges(uint32_t sample_rate, uint32_t *edges);

/* The files (RIFF/WAVE, native FLAC, MPEG Layer III) are decoded by the very route the analysis uses -- the same loaders, the
 * same groups (tuning key 13), the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0) -- and fingerprinted
 * where the PCM lies.  The codes stay on the device from group to group; the match stage runs once after the last group.
 * out[i]: the file's record.  pairs[0 .. min(*n_pairs, max_pairs)): the matching pairs only, in (i, j) order; *n_pairs is
 * their true number even when max_pairs is smaller (pairs may be NULL when max_pairs is 0).  codes_out may be NULL; otherwise
 * it holds codes_cap codes and receives file i's codes at out[i].codes_at, as many files as fit whole (a file that did not
 * fit, and every file when codes_out is NULL, has codes_at = UINT64_MAX).  A failing file fails alone (RG_ERR_IO, RG_ERR_FORMAT; its record zero apart from `status`)
 * and takes part in no pair.  RG_OK whenever the call itself worked.  The records are byte for byte the same for tuning key
 * 14 = 1 and 14 = 0. */
int rg_same_recording(rg_ctx *ctx, const char *const *paths, size_t n, const rg_fingerprint_opts *opts, rg_fingerprint_result *out,
                      rg_fingerprint_pair *pairs, size_t max_pairs, size_t *n_pairs, uint32_t *codes_out, size_t codes_cap);

/* Test seam, stage 1: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32
 * frames: anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0, RG_FP_COMPLETE set, group = i, matches = 0.  The tracks'
 * codes are packed in track order: codes_out (may be NULL) holds the sum of K codes, bands_out (may be NULL) the sum of F
 * frames of 33 floats (E[n][m] at bands_out[(frames_at + n) * 33 + m]).
 *   route 0  the serial host twin in double: the definitions above; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' arithmetic on the host: the same f32 butterflies, pairs of frames and tiles; `ctx` may be NULL.
 *            Routes 1 and 2 give byte-equal records, codes and bands.
 * RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not sample-aligned. */
int rg_fingerprint_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes,
                         rg_fingerprint_result *out, uint32_t *codes_out, float *bands_out);

/* Test seam, stage 2, on constructed codes: track t has counts[t] codes at rate rates[t], packed in track order in `codes`.
 * pair_records receives n (n - 1) / 2 records in (i, j) order: (0,1), (0,2), .. (1,2), ..  Route 0 is the host (`ctx` may be
 * NULL), route 1 the kernel.  RG_ERR_INVALID_ARG for an option out of its range. */
int rg_fingerprint_match_codes(void *ctx, int route, size_t n, const uint32_t *counts, const uint32_t *rates, const uint32_t *codes,
                               const rg_fingerprint_opts *opts, rg_fingerprint_pair_record *pair_records);

/* The host's finish on pair records in (i, j) order: groups[t] = the smallest index of t's component, matches[t] = matching
 * pairs t is part of (either may be NULL); -> the number of matching pairs. */
size_t rg_fingerprint_groups(size_t n, const rg_fingerprint_pair_record *pair_records, uint32_t *groups, uint32_t *matches);

/* Test seam: how the kernels cut their work.  tile_codes = T: one workgroup of `lanes` lanes makes codes tT .. tT + T - 1 of a
 * track from T + 1 frames, two per transform.  match_lanes: lanes of the match kernel's workgroup, one per pair; lags_per_lane:
 * the most lags one of them owns.  Any pointer may be NULL. */
int rg_fingerprint_kernel_shape(uint32_t *tile_codes, uint32_t *lanes, uint32_t *lds_bytes, uint32_t *match_lanes, uint32_t *lags_per_lane);

/* Measurement hook (tools/fingerprint_rate.py): `n` tracks of `frames` frames of 2 channels of S16, filled on the device.  After
 * a warm-up of `warm_ms` milliseconds, `reps` rounds of: the fingerprint kernels over all tracks (fp_ms[r]), a read-only pass
 * over the same planes (read_ms[r]), the match kernel over all pairs at `opts` (match_ms[r]), HIP events around the launches
 * alone; when host_tracks > 0, route 2 over the first host_tracks tracks and the host match of their pairs on `threads` host
 * threads (host_fp_ms[r], host_match_ms[r]).  *mismatches: codes or pair records of those tracks that differ (must be 0). */
int rg_fingerprint_rate(void *ctx, size_t n, uint64_t frames, const rg_fingerprint_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                        double warm_ms, double *fp_ms, double *read_ms, double *match_ms, double *host_fp_ms, double *host_match_ms,
                        size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
