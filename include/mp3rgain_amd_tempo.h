/* mp3rgain_amd_tempo.h -- how fast is a track?  Tempo (BPM) and a constant-tempo beat grid, in two stages on the GPU: an onset
 * curve per track (one integer per 512 samples, from the planes the file route has put into the analysis arena), and a windowed
 * autocorrelation of that curve with an all-integer finish.  The BPM field of a tagger or a DJ library otherwise takes a second
 * decode of every file in another program.
 *
 * THE ESTIMATOR IS A CONVENTION OF THIS PROJECT, TRIED ON SYNTHETIC MATERIAL ONLY (click tracks and a drum pattern; see THE
 * MEASUREMENTS below).  NOBODY HAS COMPARED IT WITH ANOTHER BPM TOOL OR RUN IT ON REAL MUSIC.  The octave of the answer (80 or
 * 160?) is a stated convention, not a finding: the reading lies in [min_bpm, 2 min_bpm).
 *
 * STAGE 1: THE ONSET CURVE (the contract).  A track has N frames of PCM per channel, N < 2^32, at sample rate fs.
 *
 * Signal, frames   Exactly the fingerprint's (mp3rgain_amd_fingerprint.h): one channel as it is, otherwise (ch0 + ch1) * 0.5f in
 *               f32; L = 4096, hop H = 512, the periodic Hann table of the spectral scan; F = 0 when N < L, otherwise
 *               (N - L) / 512 + 1 frames, and K = max(F - 1, 0) onsets.  A frame of a float track in which some x is a NaN or
 *               Inf has all band energies 0 and is counted in nonfinite_frames.
 * Bands         32 bands (RG_TEMPO_BANDS), logarithmic from 60 to 8000 Hz: e[m] = floor(60 * (8000/60)^(m/32) * L / fs + 0.5),
 *               m = 0 .. 32, in double on the host, then forced to increase: e[0] = max(e[0], 1), e[m] = max(e[m], e[m-1] + 1)
 *               (rg_tempo_bands).  A rate is supported when e[32] <= 2048: every rate from 15997 Hz up (44100, 48000, 96000 and
 *               192000 among them).  A track at an unsupported rate gets RG_TEMPO_RATE, no onsets, no tempo, and no error.
 *               E[n][m] is the f32 sum of |X|^2 over bins e[m] .. e[m+1] - 1 of frame n's 4096-point DFT, in bin order.
 * Compression   Without a logarithm: q(E) is the IEEE-754 bit pattern of (E > 2^-16f ? E : 2^-16f), shifted right by 18; one
 *               step of q is 1/32 of an octave of power.  S[n] = sum over m of max(0, q(E[n][m]) - q(E[n-1][m])), n = 1 .. F-1,
 *               and the onset o[n-1] = min(1023, S[n] >> 2), a uint16.  FROM HERE ON NOTHING IS A FLOAT.
 * Routes        Route 0 is these definitions with the transform and the band sums in double, each E rounded to f32 before q.
 *               The kernels (route 1) and their arithmetic on the host (route 2) work in f32, two frames per complex transform,
 *               a tile of 7 onsets per workgroup (the fingerprint's tile walk): routes 1 and 2 give byte-equal onsets and band
 *               energies; route 0 differs from them in a small share of onsets, each by one step where an energy lies next to a
 *               step of q (tests/golden/tempo_measured.json).
 *
 * STAGE 2: DEFINITIONS (all integer).  rg_tempo_opts {window W, hop, min_bpm}; NULL or a zero field means the default
 * {1024, 256, 80} (a zero hop under a smaller window: the window); 32 <= W <= 1024, 1 <= hop <= W, 30 <= min_bpm <= 300.
 *
 * Windows       Window w starts at s_w = w * hop and exists while s_w + 2W <= K.  No window: RG_TEMPO_SHORT.
 * Sums          For d = 0 .. W-1:  R_w[d] = sum over i < W of o[s_w+i] * o[s_w+i+d] (fits u32),  A_w = sum of o[s_w+i],
 *               B_w[d] = sum of o[s_w+i+d],  c_w[d] = R_w[d] - floor(A_w * B_w[d] / W) (fits i32),  C[d] = sum over w of
 *               c_w[d] in i64.
 * Candidates    Periods in sixteenths of an onset: P16 in [pmax/2 + 1, pmax], pmax = floor(15 fs / (8 min_bpm)), so that
 *               BPM = 1.875 fs / P16 lies in [min_bpm, 2 min_bpm).  Kh = min(8, floor(16 (W - 2) / pmax)) harmonics; Kh = 0:
 *               RG_TEMPO_RANGE and no tempo.
 * Score         score(c, P16) = sum over k = 1 .. Kh of c[i] * (16 - f) + c[i+1] * f,  i = (k P16) >> 4, f = (k P16) & 15, i64.
 * Period        The P16 with the largest score(C, .), a tie to the smaller P16.  C[0] <= 0 (silence, a constant curve):
 *               RG_TEMPO_NONE and no tempo.  bpm_milli = round(1875 fs / P16).
 * Confidence    confidence_permille = clamp(floor(1000 score / (16 Kh C[0])), 0, 1000).
 * Stability     Every window picks P16_w from its own c_w in the same way; stable_permille = floor(1000 * (windows with
 *               |P16_w - P16| * 32 <= P16) / windows).
 * Beat grid     Constant tempo; meaningful when stable_permille is high.  For phi = 0 .. P16-1, sum(phi) is the sum of
 *               o[(phi + j P16 + 8) >> 4] over j = 0, 1, .. while the index is below K, count(phi) their number.  The best phi
 *               has the largest sum / count, by 64-bit cross-multiplication, a tie to the smaller phi.
 *               first_beat = phi * 32 + RG_TEMPO_BEAT_BIAS samples.  A 93 ms analysis window makes this COARSE: the grid is
 *               good to a few hundredths of a second, not to the sample.
 *
 * All of stage 2 is integer arithmetic: the serial host twin (route 0 of rg_tempo_from_onsets) and the kernels (route 1) agree
 * byte for byte, whatever order the windows' 64-bit atomic additions into C take.
 *
 * THE MEASUREMENTS (tools/tempo_refcheck.py, tests/golden/tempo_measured.json): click tracks and a kick / snare / hat pattern,
 * 40 s each, at 44100 and 48000 Hz and nine tempi from 80 to 159 BPM, with the float64 restatement of these definitions at the
 * defaults.  The file holds the largest relative tempo error, the confidence and stability ranges, the confidence of white
 * noise, the share of onsets in which f32 and float64 differ, and the offsets between the curve's best phase and the clicks'
 * true positions whose median RG_TEMPO_BEAT_BIAS is.
 *
 * RATES.  tools/tempo_rate.py on an MI355X (profiles/tempo_rate.json), 1000 tracks of 3 min of 16-bit stereo, HIP events around
 * the launches alone after a warm-up, medians of 5: the onset kernels 266 ms (68 times route 2 on 16 host threads; a read-only
 * pass over the same planes is 2 % of it; the fingerprint stage takes 160 ms on the same workload), the window kernel over all
 * 53000 windows 3.7 ms = 1.5e13 multiply-adds per second, the finish 0.26 ms (the two 238 times the host's stage 2 on 16
 * threads), with no onset and no record different from the host's.
 *
 * Not here: tempo that drifts or changes (only flagged, through stable_permille); downbeats and time signatures; musical key;
 * the node and multi-GPU calls; rates below 16 kHz; agreement with any other BPM tool.
 */
#ifndef MP3RGAIN_AMD_TEMPO_H
#define MP3RGAIN_AMD_TEMPO_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_TEMPO_SHORT      1u /* no window: K < 2W */
#define RG_TEMPO_RATE       2u /* the rate is not supported: no onsets */
#define RG_TEMPO_NONFINITE  4u /* some frame held a NaN or Inf */
#define RG_TEMPO_COMPLETE   8u /* dropped_frames == 0 */
#define RG_TEMPO_RANGE     16u /* Kh = 0: the window is too short for the slowest candidate */
#define RG_TEMPO_NONE      32u /* C[0] <= 0: silence or a constant curve */

#define RG_TEMPO_MAX_CHANNELS 8u
#define RG_TEMPO_FRAME 4096u
#define RG_TEMPO_HOP    512u
#define RG_TEMPO_BANDS   32u
#define RG_TEMPO_WINDOW 1024u /* the defaults of rg_tempo_opts */
#define RG_TEMPO_WINDOW_HOP 256u
#define RG_TEMPO_MIN_BPM 80u
#define RG_TEMPO_MIN_WINDOW 32u
#define RG_TEMPO_MAX_WINDOW 1024u
#define RG_TEMPO_MAX_HARMONICS 8u
#define RG_TEMPO_ONSET_MAX 1023u
#define RG_TEMPO_BEAT_BIAS 4120u /* samples; the median measured by tools/tempo_refcheck.py */

typedef struct rg_tempo_opts {
    uint32_t window, hop, min_bpm; /* 0 = the default */
} rg_tempo_opts;

typedef struct rg_tempo_result {
    int32_t status;            /* RG_OK, or why there is no reading (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;           /* N: PCM frames per channel                                          */
    uint32_t sample_rate;
    uint32_t channels;
    uint32_t format;           /* rg_sample_format of the planes                                     */
    uint32_t dropped_frames;   /* frames the decode route dropped, as the stats record counts them   */
    uint32_t onsets;           /* K (0 at an unsupported rate)                                       */
    uint32_t windows;
    uint32_t period16;         /* P16; 0: no tempo (SHORT, RATE, RANGE or NONE)                      */
    uint32_t harmonics;        /* Kh                                                                 */
    uint32_t bpm_milli;        /* round(1875 fs / P16)                                               */
    uint32_t confidence_permille;
    uint32_t stable_permille;
    uint32_t first_beat;       /* samples from the start of the track                                */
    uint32_t nonfinite_frames;
    uint32_t band_frames;      /* F: the rows of band energies the seam gives for this track         */
    uint64_t onsets_at;        /* where the track's onsets start in onsets_out, in onsets            */
} rg_tempo_result;             /* 80 bytes */

/* The band edges of a rate: edges[0 .. 32].  RG_ERR_UNSUPPORTED_RATE (edges still filled) when e[32] > 2048, RG_ERR_INVALID_ARG
 * for a NULL pointer or rate 0.  Plain host arithmetic in double. */
int rg_tempo_bands(uint32_t sample_rate, uint32_t *edges);

/* The files (RIFF/WAVE, native FLAC, MPEG Layer III) are decoded by the very route the analysis uses -- the same loaders, the
 * same groups, the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0) -- and both stages run where the
 * PCM lies.  out[i]: the file's record.  onsets_out may be NULL; otherwise it holds onsets_cap onsets and receives file i's curve
 * at out[i].onsets_at, as many files as fit whole in the order the groups ran (a file that did not fit, and every file when
 * onsets_out is NULL, has onsets_at = UINT64_MAX).  A failing file fails alone (RG_ERR_IO, RG_ERR_FORMAT; its record zero apart
 * from `status`).  RG_OK whenever the call itself worked.  The records are byte for byte the same for tuning key 14 = 1 and 0. */
int rg_tempo(rg_ctx *ctx, const char *const *paths, size_t n, const rg_tempo_opts *opts, rg_tempo_result *out, uint16_t *onsets_out,
             size_t onsets_cap);

/* Test seam, both stages: the `n` tracks that descs[i] describe in the host arena `arena` (1 .. 8 channels and fewer than 2^32
 * frames: anything else is RG_ERR_FORMAT).  out[i].dropped_frames is 0 and RG_TEMPO_COMPLETE set.  The tracks' onsets are packed
 * in track order: onsets_out (may be NULL) holds the sum of K onsets, bands_out (may be NULL) the sum of F = band_frames rows of
 * 32 floats, in track order.
 *   route 0  the serial host twin, the transform in double; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' arithmetic on the host, and the host's stage 2; `ctx` may be NULL.
 *            Routes 1 and 2 give byte-equal records, onsets and bands.
 * RG_ERR_INVALID_ARG for a track whose planes are not wholly inside the arena or not sample-aligned, or an option out of range. */
int rg_tempo_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_tempo_opts *opts,
                   rg_tempo_result *out, uint16_t *onsets_out, float *bands_out);

/* Test seam, stage 2, on constructed curves: track t has counts[t] onsets (each at most 1023, fewer than 2^32 / 512 of them) at
 * rate rates[t], packed in track order in `onsets`.  out[t]: the stage-2 fields, with frames, channels and format 0.  acf_out
 * (may be NULL) receives W values per track: C[d] of track t at acf_out[t * W + d] (zeros for a track without windows or with
 * Kh = 0).  Route 0 is the host (`ctx` may be NULL), route 1 the kernels. */
int rg_tempo_from_onsets(void *ctx, int route, size_t n, const uint32_t *counts, const uint32_t *rates, const uint16_t *onsets,
                         const rg_tempo_opts *opts, rg_tempo_result *out, int64_t *acf_out);

/* Test seam: how the kernels cut their work.  tile_onsets = T: one workgroup of `lanes` lanes makes onsets tT .. tT + T - 1 of a
 * track from T + 1 frames, two per transform, in lds_bytes of LDS.  acf_lanes: lanes of the window kernel's workgroup;
 * lags_per_lane: the consecutive lags one of them owns.  Any pointer may be NULL. */
int rg_tempo_kernel_shape(uint32_t *tile_onsets, uint32_t *lanes, uint32_t *lds_bytes, uint32_t *acf_lanes, uint32_t *lags_per_lane);

/* Measurement hook (tools/tempo_rate.py): `n` tracks of `frames` frames of 2 channels of S16 at 44100 Hz, filled on the device.
 * After a warm-up of `warm_ms` milliseconds, `reps` rounds of: the onset kernels over all tracks (onset_ms[r]), a read-only pass
 * over the same planes (read_ms[r]), the window kernel (acf_ms[r]) and the finish kernel (finish_ms[r]) at `opts`, HIP events
 * around the launches alone; when host_tracks > 0, route 2 over the first host_tracks tracks and the host's stage 2 on `threads`
 * host threads (host_onset_ms[r], host_finish_ms[r]).  *mismatches: onsets or records of those tracks that differ (must be 0). */
int rg_tempo_rate(void *ctx, size_t n, uint64_t frames, const rg_tempo_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                  double *onset_ms, double *read_ms, double *acf_ms, double *finish_ms, double *host_onset_ms, double *host_finish_ms,
                  size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
