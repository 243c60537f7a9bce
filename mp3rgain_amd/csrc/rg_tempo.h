// rg_tempo.h -- internal: the tempo scan (include/mp3rgain_amd_tempo.h) as rg_tempo.hip (the onset kernel, the window and finish
// kernels, their launchers and seams), rg_tempo_host.cpp (the serial twins and the kernels' f32 arithmetic on the host) and
// rg_file_verify.hip (rg_tempo) share it.  Stage 1 is the fingerprint's tile walk with other bands (rg_fprint.h: the track
// record RgFpTrack with `codes_at` counting onsets, the plan, rg_fp_band; rg_fprint_tile.h on the device), and what is written
// once here for both sides is how an onset comes from two rows of band energies and how a period is scored.  Stage 2 is integer
// arithmetic throughout.  Both translation units are compiled without contraction.
#pragma once

#include <vector>

#include "../../include/mp3rgain_amd_tempo.h"
#include "rg_fprint.h"

#define RG_TP_TILE_ONSETS RG_FP_TILE_CODES
#define RG_TP_ACF_LANES 256u
#define RG_TP_LAGS_PER_LANE 4u  // consecutive lags of one lane of the window kernel: 256 x 4 = RG_TEMPO_MAX_WINDOW

// One track of a stage-2 launch
struct RgTpTrack {
    uint64_t onsets_at;  // where its onsets lie, in onsets
    uint64_t first_win;  // of this track among the launch's windows
    uint32_t k;          // K
    uint32_t windows;    // (none of them is launched when kh == 0)
    uint32_t pmax, kh;
    uint32_t rate_ok, reserved;
};  // 40 bytes

// What the finish makes of a track; period16 == 0: no tempo
struct RgTpFinish {
    uint32_t period16, confidence_permille, stable_permille, first_beat;
};

// (q(E), rg_tp_q, lies in rg_fprint.h: the key scan compresses its band energies with it too)
// the onset of frame n from E[n - 1] (`prev`) and E[n] (`cur`), 32 floats each
RG_SPEC_HD uint16_t rg_tp_onset(const float *prev, const float *cur) {
    uint32_t s = 0;
    for (uint32_t m = 0; m < RG_TEMPO_BANDS; ++m) {
        const uint32_t a = rg_tp_q(cur[m]), b = rg_tp_q(prev[m]);
        s += a > b ? a - b : 0u;
    }
    s >>= 2;
    return (uint16_t)(s < RG_TEMPO_ONSET_MAX ? s : RG_TEMPO_ONSET_MAX);
}

// score(c, P16) over kh harmonics; c holds at least (kh * p16 >> 4) + 2 values
template <class T>
RG_SPEC_HD int64_t rg_tp_score(const T *c, uint32_t p16, uint32_t kh) {
    int64_t s = 0;
    for (uint32_t k = 1; k <= kh; ++k) {
        const uint32_t x = k * p16, i = x >> 4, f = x & 15u;
        s += (int64_t)c[i] * (int64_t)(16u - f) + (int64_t)c[i + 1] * (int64_t)f;
    }
    return s;
}
// a candidate period and its score; p16 == 0: none
struct RgTpBest {
    int64_t score;
    uint32_t p16, reserved;
};
// is x better than y: the larger score, then the smaller period
RG_SPEC_HD bool rg_tp_better(const RgTpBest &x, const RgTpBest &y) {
    if (!x.p16) return false;
    if (!y.p16) return true;
    if (x.score != y.score) return x.score > y.score;
    return x.p16 < y.p16;
}
// a phase of the beat grid, its sum and count; count == 0: none
struct RgTpPhase {
    uint64_t sum;
    uint32_t count, phi;
};
// is x better than y: the larger sum / count by cross-multiplication, then the smaller phase
RG_SPEC_HD bool rg_tp_phase_better(const RgTpPhase &x, const RgTpPhase &y) {
    if (!x.count) return false;
    if (!y.count) return true;
    const uint64_t l = x.sum * y.count, r = y.sum * x.count;  // sum < 2^33, count < 2^23
    if (l != r) return l > r;
    return x.phi < y.phi;
}
// phase phi of period p16 over k onsets at o
RG_SPEC_HD RgTpPhase rg_tp_phase(const uint16_t *o, uint32_t k, uint32_t p16, uint32_t phi) {
    RgTpPhase ph{0u, 0u, phi};
    for (uint64_t x = (uint64_t)phi + 8u; (x >> 4) < k; x += p16) {
        ph.sum += o[x >> 4];
        ph.count += 1u;
    }
    return ph;
}
// clamp(floor(1000 score / den), 0, 1000) for den > 0 without leaving 64 bits: three decimal digits by long division
RG_SPEC_HD uint32_t rg_tp_permille(int64_t score, int64_t den) {
    if (score <= 0) return 0u;
    if (score >= den) return 1000u;
    uint64_t r = (uint64_t)score, d = (uint64_t)den;  // r < d < 2^60: 10 r fits
    uint32_t out = 0;
    for (int digit = 0; digit < 3; ++digit) {
        r *= 10u;
        out = out * 10u + (uint32_t)(r / d);
        r %= d;
    }
    return out;
}
RG_SPEC_HD bool rg_tp_window_stable(uint32_t p16_w, uint32_t p16) {
    const uint32_t diff = p16_w > p16 ? p16_w - p16 : p16 - p16_w;
    return (uint64_t)diff * 32u <= p16;
}
// the finish of a track from its best period: everything of RgTpFinish but stable_permille's count and the phase, which the
// callers find their own way
RG_SPEC_HD void rg_tp_close(const RgTpBest &best, int64_t c0, uint32_t kh, uint32_t stable_windows, uint32_t windows, const RgTpPhase &phase,
                            RgTpFinish *out) {
    out->period16 = best.p16;
    out->confidence_permille = rg_tp_permille(best.score, 16 * (int64_t)kh * c0);
    out->stable_permille = (uint32_t)((uint64_t)stable_windows * 1000u / windows);
    out->first_beat = phase.phi * 32u + RG_TEMPO_BEAT_BIAS;
}

// ---- host side (rg_tempo_host.cpp) -------------------------------------------------------------------------------------------
// the options, checked: NULL or a zero field = the default
int rg_tp_options(const rg_tempo_opts *opts, rg_tempo_opts *out, char *err, size_t err_len);
// track i's stage-1 record of a launch, checked against the arena; everything but first_tile, codes_at and frames_at (rg_fp_plan)
int rg_tp_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgFpTrack *out, char *err, size_t err_len);
// route 0 and route 2 of one track's stage 1: onsets[0 .. K), bands[0 .. 32 F) (either may be NULL), -> non-finite frames
uint32_t rg_tp_serial_host(const unsigned char *arena, const RgFpTrack &t, uint16_t *onsets, float *bands);
uint32_t rg_tp_folded_host(const unsigned char *arena, const RgFpTrack &t, uint16_t *onsets, float *bands);
// a track's stage-2 record from its rate and K: windows, pmax, kh (onsets_at and first_win are the caller's)
void rg_tp_stage2_track(uint32_t rate, uint32_t k, const rg_tempo_opts &o, RgTpTrack *out);
// first_win of tracks[0 .. n); -> windows
uint64_t rg_tp_stage2_plan(RgTpTrack *tracks, size_t n);
// stage 2 of one track on the host, serially: acf[0 .. W) <- C unless NULL
void rg_tp_stage2_host(const uint16_t *onsets, const RgTpTrack &t, const rg_tempo_opts &o, RgTpFinish *out, int64_t *acf);
// the record: d may be NULL (rg_tempo_from_onsets: `rate` alone), f NULL for a track stage 2 never saw
void rg_tp_fill(const rg_track_desc *d, uint32_t rate, uint32_t band_frames, const RgTpTrack &t, const RgTpFinish &f, uint32_t dropped_frames,
                uint32_t nonfinite_frames, uint64_t onsets_at, rg_tempo_result *out);
int rg_tp_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_tempo_opts &o, rg_tempo_result *out,
                     uint16_t *onsets_out, float *bands_out, char *err, size_t err_len);
// the checks of rg_tempo_from_onsets's arrays, and its route 0
int rg_tp_from_onsets_check(size_t n, const uint32_t *counts, const uint16_t *onsets, char *err, size_t err_len);
int rg_tp_from_onsets_host(size_t n, const uint32_t *counts, const uint32_t *rates, const uint16_t *onsets, const rg_tempo_opts &o, rg_tempo_result *out,
                           int64_t *acf_out);

#if defined(__HIPCC__)
struct rg_ctx;
// stage 1: `n` planned tracks in the device arena at `d_arena`: the onset kernels on `s`; onsets to d_onsets[codes_at ..], band
// energies to d_bands[frames_at * 32 ..] unless NULL, nonfinite[i] <- track i's count; `s` has been synchronised on return
int rg_tempo_onsets_device(rg_ctx *c, const unsigned char *d_arena, RgFpTrack *tracks, size_t n, uint16_t *d_onsets, float *d_bands, uint32_t *nonfinite,
                           hipStream_t s);
// stage 2: the window and finish kernels over the device onsets at d_onsets; finish[i] <- track i, acf (host, n * W values) <- C
// unless NULL; `s` has been synchronised on return
int rg_tempo_stage2_device(rg_ctx *c, const uint16_t *d_onsets, RgTpTrack *tracks, size_t n, const rg_tempo_opts &o, RgTpFinish *finish, int64_t *acf,
                           hipStream_t s);
#endif
