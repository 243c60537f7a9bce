// rg_key.h -- internal: the key scan (include/mp3rgain_amd_key.h) as rg_key.hip (the decimation, tiles and finish kernels, their
// launchers and seams), rg_key_host.cpp (the serial twins and the kernels' f32 arithmetic on the host) and rg_file_verify.hip
// (rg_key) share it.  Stage 1a is this scan's own (a FIR sum per output in ascending tap order); stage 1b is the fingerprint's
// tile walk on the decimated signal as a mono f32 track, with 60 bands whose edges come through a pointer (rg_fprint.h,
// rg_fprint_tile.h); what is written once here for both sides is how a chroma row comes from a row of band energies and how a
// key is picked from twelve sums.  Stage 2 is integer arithmetic throughout.  Both translation units are compiled without
// contraction.
#pragma once

#include <vector>

#include "../../include/mp3rgain_amd_key.h"
#include "rg_fprint.h"

#define RG_KEY_DECIM_LANES 256u
#define RG_KEY_DECIM_OUTPUTS 256u  // consecutive y of one workgroup, one per lane
// the staged run of a workgroup, polyphase-transposed: D rows (k mod D) of RG_KEY_DECIM_COLS floats (k / D <= 255 + 16)
#define RG_KEY_DECIM_COLS (RG_KEY_DECIM_OUTPUTS + RG_KEY_TAPS_PER_DECIM + 1u)
#define RG_KEY_TILE_ROWS RG_FP_TILE_CODES
#define RG_KEY_FINISH_LANES 256u
#define RG_KEY_TILE_LDS_BYTES (16u * 306u * 8u + RG_FP_STAGE * 4u + RG_FP_TILE_FRAMES * RG_KEY_BANDS * 4u + (RG_KEY_BANDS + 1u) * 4u)

// One track of a launch
struct RgKeyTrack {
    uint64_t off0, off1;  // planes of the first two channels from the arena's base, in bytes
    uint64_t y_at;        // where its y lies in the decimated buffer, in floats (a multiple of 4)
    uint64_t rows_at;     // where its chroma rows (and band energies) go, in rows
    uint64_t first_wg;    // of this track among the launch's decimation workgroups (the workgroups of one format are contiguous)
    uint32_t n, m, rows;  // N, M, F
    uint32_t decim;       // D; 0: the rate is not supported (M = F = 0)
    uint32_t format, channels;  // channels: 1 or 2, the planes that count
    uint32_t taps_at;     // where the filter of D starts in the launch's tables, in floats (D >= 2)
    uint32_t n_wg;        // ceil(M / 256)
    uint32_t recip;       // floor(2^32 / D) + 1: i / D = (i * recip) >> 32 while i D < 2^32
    uint32_t reserved;
    uint32_t e[RG_KEY_BANDS + 1];
};  // 324 -> 328 bytes

// What the finish makes of a track
struct RgKeyFinish {
    uint32_t silent_rows, flags;  // flags: RG_KEY_NONE or 0
    uint32_t key, correlation_permille, margin_permille, segments, stable_permille, reserved;
};

// a key picked from twelve sums; none: no key (all zero, flat, or no positive score)
struct RgKeyPick {
    uint32_t key, correlation_permille, margin_permille, none;
};

RG_SPEC_HD int32_t rg_key_profile(uint32_t mode, uint32_t i) {
    const int32_t major[12] = {656, -286, -1, -263, 205, 139, -220, 390, -250, 41, -273, -138};
    const int32_t minor[12] = {654, -257, -47, 418, -277, -45, -292, 260, 68, -255, -92, -135};
    return mode ? minor[i] : major[i];
}

// the chroma row of a frame from its 60 band energies
RG_SPEC_HD void rg_key_row(const float *E, uint16_t *row) {
    const uint32_t floor_q = rg_tp_q(0.0f);
    uint32_t qmax = 0;
    for (uint32_t s = 0; s < RG_KEY_BANDS; ++s) {
        const uint32_t q = rg_tp_q(E[s]);
        qmax = q > qmax ? q : qmax;
    }
    for (uint32_t p = 0; p < RG_KEY_CHROMA; ++p) {
        uint32_t c = 0;
        if (qmax != floor_q)
            for (uint32_t o = 0; o < RG_KEY_BANDS / RG_KEY_CHROMA; ++o) {
                const uint32_t q = rg_tp_q(E[RG_KEY_CHROMA * o + p]);  // qmax >= q(2^-16) = 3552 > R
                c += q + RG_KEY_RANGE > qmax ? q + RG_KEY_RANGE - qmax : 0u;
            }
        row[p] = (uint16_t)c;
    }
}
RG_SPEC_HD bool rg_key_row_silent(const uint16_t *row) {
    uint32_t any = 0;
    for (uint32_t p = 0; p < RG_KEY_CHROMA; ++p) any |= row[p];
    return !any;
}

// floor(sqrt(x))
RG_SPEC_HD uint64_t rg_key_isqrt(uint64_t x) {
    uint64_t r = 0;
    for (uint64_t bit = (uint64_t)1 << 62; bit; bit >>= 2) {
        if (x >= r + bit) {
            x -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return r;
}

// score(mode, tonic) of the scaled sums h, key = 12 mode + tonic
RG_SPEC_HD int64_t rg_key_score(const uint32_t *h, uint32_t key) {
    const uint32_t mode = key / 12u, tonic = key % 12u;
    int64_t s = 0;
    for (uint32_t p = 0; p < 12; ++p) s += (int64_t)h[p] * rg_key_profile(mode, (p + 12u - tonic) % 12u);
    return s;
}

// h <- H >> sh, sh the smallest shift that brings every sum below 65536
RG_SPEC_HD void rg_key_scale(const uint64_t *H, uint32_t *h) {
    uint64_t top = 0;
    for (uint32_t p = 0; p < 12; ++p) top = H[p] > top ? H[p] : top;
    uint32_t sh = 0;
    while ((top >> sh) >= 65536u) ++sh;
    for (uint32_t p = 0; p < 12; ++p) h[p] = (uint32_t)(H[p] >> sh);
}

// the pick from the 24 scores of h
RG_SPEC_HD void rg_key_close(const uint32_t *h, const int64_t *score, RgKeyPick *out) {
    *out = RgKeyPick{0u, 0u, 0u, 1u};
    uint64_t sum = 0, squares = 0;
    for (uint32_t p = 0; p < 12; ++p) {
        sum += h[p];
        squares += (uint64_t)h[p] * h[p];
    }
    const uint64_t vh = 12u * squares - sum * sum, den = rg_key_isqrt(1000000u * vh / 12u);
    uint32_t best = 0;
    for (uint32_t k = 1; k < 24; ++k)
        if (score[k] > score[best]) best = k;
    if (!den || score[best] <= 0) return;
    uint32_t second = best ? 0u : 1u;
    for (uint32_t k = 0; k < 24; ++k)
        if (k != best && score[k] > score[second]) second = k;
    const int64_t corr = 1000 * score[best] / (int64_t)den, margin = 1000 * (score[best] - score[second]) / score[best];
    out->key = best;
    out->correlation_permille = (uint32_t)(corr > 1000 ? 1000 : corr);
    out->margin_permille = (uint32_t)(margin > 1000 ? 1000 : margin);
    out->none = 0u;
}

// the pick from twelve sums, serially
RG_SPEC_HD void rg_key_pick(const uint64_t *H, RgKeyPick *out) {
    uint32_t h[12];
    int64_t score[24];
    rg_key_scale(H, h);
    for (uint32_t k = 0; k < 24; ++k) score[k] = rg_key_score(h, k);
    rg_key_close(h, score, out);
}

// segment g of S rows at `rows`: its sums; -> whether some row of it is not zero
RG_SPEC_HD bool rg_key_segment_sums(const uint16_t *rows, uint32_t g, uint32_t S, uint64_t *H) {
    for (uint32_t p = 0; p < 12; ++p) H[p] = 0;
    const uint16_t *r = rows + (uint64_t)g * S * RG_KEY_CHROMA;
    for (uint32_t n = 0; n < S; ++n)
        for (uint32_t p = 0; p < 12; ++p) H[p] += r[n * RG_KEY_CHROMA + p];
    uint64_t any = 0;
    for (uint32_t p = 0; p < 12; ++p) any |= H[p];
    return any != 0;
}

// the finish record of a track from its pick and its counts
RG_SPEC_HD void rg_key_finish(const RgKeyPick &pick, uint32_t silent_rows, uint32_t segments, uint32_t nonzero, uint32_t agreeing, RgKeyFinish *out) {
    out->silent_rows = silent_rows;
    out->flags = pick.none ? RG_KEY_NONE : 0u;
    out->key = pick.key;
    out->correlation_permille = pick.correlation_permille;
    out->margin_permille = pick.margin_permille;
    out->segments = segments;
    out->stable_permille = pick.none || !nonzero ? 0u : (uint32_t)((uint64_t)agreeing * 1000u / nonzero);
    out->reserved = 0;
}

// ---- host side (rg_key_host.cpp) ---------------------------------------------------------------------------------------------
// the options, checked: NULL or 0 = the default
int rg_key_options(const rg_key_opts *opts, rg_key_opts *out, char *err, size_t err_len);
// track i's record of a launch, checked against the arena; everything but y_at, rows_at, first_wg and taps_at
int rg_key_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgKeyTrack *out, char *err, size_t err_len);
// y_at (16-byte aligned runs) and rows_at in track order, first_wg with the workgroups of one format contiguous
// (fmt_wg[f] .. fmt_wg[f + 1]); taps <- the filters of the Ds that occur, taps_at set; -> the floats of y
uint64_t rg_key_plan(RgKeyTrack *tracks, size_t n, uint64_t fmt_wg[4], std::vector<float> *taps, uint64_t *rows);
// the filter of D >= 2 (cached per D)
const std::vector<float> &rg_key_taps(uint32_t decim);
// the tile walk's record of a track whose y lies at byte `off` of an f32 arena
void rg_key_fp_track(const RgKeyTrack &t, uint64_t off, RgFpTrack *out);
// route 0 and route 2 of one track's stage 1: y[0 .. M), bands[0 .. 60 F), rows[0 .. 12 F) (bands may be NULL), -> non-finite frames
uint32_t rg_key_serial_host(const unsigned char *arena, const RgKeyTrack &t, float *y, float *bands, uint16_t *rows);
uint32_t rg_key_folded_host(const unsigned char *arena, const RgKeyTrack &t, float *y, float *bands, uint16_t *rows);
// stage 2 of one track of F rows on the host, serially
void rg_key_stage2_host(const uint16_t *rows, uint32_t F, const rg_key_opts &o, RgKeyFinish *out);
// the record: d may be NULL (rg_key_from_chroma), t NULL likewise
void rg_key_fill(const rg_track_desc *d, const RgKeyTrack *t, uint32_t F, const RgKeyFinish &f, uint32_t dropped_frames, uint32_t nonfinite_frames,
                 uint64_t chroma_at, rg_key_result *out);
int rg_key_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_key_opts &o, rg_key_result *out,
                      float *decim_out, float *bands_out, uint16_t *chroma_out, char *err, size_t err_len);
int rg_key_from_chroma_check(size_t n, const uint32_t *counts, const uint16_t *chroma, char *err, size_t err_len);
int rg_key_from_chroma_host(size_t n, const uint32_t *counts, const uint16_t *chroma, const rg_key_opts &o, rg_key_result *out);

#if defined(__HIPCC__)
struct rg_ctx;
// both stages: `n` tracks (rg_key_track) in the device arena at `d_arena`, planned here; y goes to c->d_key_decim, the rows to
// c->d_key_rows (track i's at tracks[i].y_at / rows_at), band energies to d_bands[rows_at * 60 ..] unless NULL; finish[i] and
// nonfinite[i] <- track i; `s` has been synchronised on return
int rg_key_device(rg_ctx *c, const unsigned char *d_arena, RgKeyTrack *tracks, size_t n, const rg_key_opts &o, bool want_bands, RgKeyFinish *finish,
                  uint32_t *nonfinite, hipStream_t s);
// Stage 1a alone, for the rational resampler's L = 1 tracks (rg_resample.hip): `tracks` hold off0, off1, n, m, decim, format,
// channels, n_wg and recip; they are planned here (first_wg, taps_at), with y_at[i] where track i's y goes.  prepare: the job,
// uploaded to c->d_key, `s` synchronised (*job stays NULL when no track has an output); launch: the decimation kernel enqueued
// on `s`, y to d_y; free: the job.
struct RgKeyDecimJob;
int rg_key_decimate_prepare(rg_ctx *c, RgKeyTrack *tracks, const uint64_t *y_at, size_t n, hipStream_t s, RgKeyDecimJob **job);
int rg_key_decimate_launch(rg_ctx *c, const unsigned char *d_arena, const RgKeyDecimJob *job, float *d_y, hipStream_t s);
void rg_key_decimate_free(RgKeyDecimJob *job);
#endif
