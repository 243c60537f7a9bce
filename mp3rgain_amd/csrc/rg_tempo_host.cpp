// rg_tempo_host.cpp -- the host side of the tempo scan (include/mp3rgain_amd_tempo.h, rg_tempo.h): the band edges, the options,
// the track records and their checks, the serial host twin of the onset curve (route 0: the transform and the band sums in
// double), the kernels' arithmetic walked by the host (route 2: the fingerprint's tile walk, rg_fprint.h, with these bands), and
// stage 2 as a serial twin of the window and finish kernels.  Plain C++: no device and no context, so a sanitizer build needs
// nothing else but rg_spectrum_host.cpp for the tables.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rg_tempo.h"

extern "C" int rg_tempo_bands(uint32_t sample_rate, uint32_t *edges) {
    if (!edges || !sample_rate) return RG_ERR_INVALID_ARG;
    for (uint32_t m = 0; m <= RG_TEMPO_BANDS; ++m) {
        const double e = std::floor(60.0 * std::pow(8000.0 / 60.0, (double)m / RG_TEMPO_BANDS) * RG_TEMPO_FRAME / (double)sample_rate + 0.5);
        edges[m] = e > 1.0e9 ? 1000000000u : (uint32_t)e;
        edges[m] = m ? std::max(edges[m], edges[m - 1] + 1u) : std::max(edges[m], 1u);
    }
    return edges[RG_TEMPO_BANDS] <= RG_TEMPO_FRAME / 2 ? RG_OK : RG_ERR_UNSUPPORTED_RATE;
}

int rg_tp_options(const rg_tempo_opts *opts, rg_tempo_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_tempo_opts{0, 0, 0};
    if (!out->window) out->window = RG_TEMPO_WINDOW;
    if (!out->hop) out->hop = std::min(RG_TEMPO_WINDOW_HOP, out->window);
    if (!out->min_bpm) out->min_bpm = RG_TEMPO_MIN_BPM;
    if (out->window >= RG_TEMPO_MIN_WINDOW && out->window <= RG_TEMPO_MAX_WINDOW && out->hop <= out->window && out->min_bpm >= 30 && out->min_bpm <= 300)
        return RG_OK;
    snprintf(err, err_len, "tempo: window %u (%u to %u), hop %u (1 to the window), min_bpm %u (30 to 300)", out->window, RG_TEMPO_MIN_WINDOW,
             RG_TEMPO_MAX_WINDOW, out->hop, out->min_bpm);
    return RG_ERR_INVALID_ARG;
}

int rg_tp_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgFpTrack *out, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_TEMPO_MAX_CHANNELS, "the tempo scan takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    memset(out, 0, sizeof *out);
    out->off0 = rg_pcm_plane_off(t, 0);
    out->off1 = t.channels >= 2 ? rg_pcm_plane_off(t, 1) : out->off0;
    out->n = (uint32_t)t.frames;
    out->format = t.format;
    out->channels = t.channels >= 2 ? 2u : 1u;
    out->rate_ok = t.sample_rate && rg_tempo_bands(t.sample_rate, out->e) == RG_OK ? 1u : 0u;
    out->frames = out->rate_ok ? rg_fp_frames(t.frames) : 0u;
    out->n_tiles = !out->frames ? 0u : std::max(1u, (out->frames - 1u + RG_TP_TILE_ONSETS - 1u) / RG_TP_TILE_ONSETS);
    return RG_OK;
}

// ---- stage 1, route 0: the definitions ------------------------------------------------------------------------------------
uint32_t rg_tp_serial_host(const unsigned char *arena, const RgFpTrack &t, uint16_t *onsets, float *bands) {
    const RgSpecTables &tb = rg_spec_tables();
    std::vector<double> re(RG_FP_FRAME), im(RG_FP_FRAME);
    float prev[RG_TEMPO_BANDS] = {0}, cur[RG_TEMPO_BANDS];
    uint32_t nonfinite = 0;
    for (uint32_t n = 0; n < t.frames; ++n) {
        bool bad = false;
        for (uint32_t k = 0; k < RG_FP_FRAME; ++k) {
            const float x = rg_fp_signal_at(arena, t, (uint64_t)n * RG_FP_HOP + k);
            bad |= rg_fp_nonfinite(x);
            re[k] = (double)x * (double)tb.window[k];
            im[k] = 0.0;
        }
        if (bad) {
            ++nonfinite;
            for (uint32_t m = 0; m < RG_TEMPO_BANDS; ++m) cur[m] = 0.0f;
        } else {
            rg_fp_fft_double(re.data(), im.data());
            for (uint32_t m = 0; m < RG_TEMPO_BANDS; ++m) {
                double s = 0.0;
                for (uint32_t b = t.e[m]; b < t.e[m + 1]; ++b) s += re[b] * re[b] + im[b] * im[b];
                cur[m] = (float)s;
            }
        }
        if (bands) memcpy(bands + (size_t)n * RG_TEMPO_BANDS, cur, sizeof cur);
        if (n && onsets) onsets[n - 1] = rg_tp_onset(prev, cur);
        memcpy(prev, cur, sizeof prev);
    }
    return nonfinite;
}

// ---- stage 1, route 2: the kernels' arithmetic -----------------------------------------------------------------------------
uint32_t rg_tp_folded_host(const unsigned char *arena, const RgFpTrack &t, uint16_t *onsets, float *bands) {
    uint32_t nonfinite = 0;
    float E[RG_FP_TILE_FRAMES * RG_TEMPO_BANDS];
    for (uint32_t tile = 0; tile < t.n_tiles; ++tile) {
        uint32_t nf = 0;
        const uint32_t f0 = tile * RG_TP_TILE_ONSETS;
        nonfinite += rg_fp_tile_bands_host<RG_TEMPO_BANDS>(arena, t, tile, E, &nf);
        for (uint32_t i = 0; i + 1 < nf; ++i)
            if (onsets) onsets[f0 + i] = rg_tp_onset(&E[i * RG_TEMPO_BANDS], &E[(i + 1) * RG_TEMPO_BANDS]);
        if (bands)
            for (uint32_t i = tile ? 1u : 0u; i < nf; ++i)
                memcpy(bands + (size_t)(f0 + i) * RG_TEMPO_BANDS, &E[i * RG_TEMPO_BANDS], RG_TEMPO_BANDS * sizeof(float));
    }
    return nonfinite;
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------------------
void rg_tp_stage2_track(uint32_t rate, uint32_t k, const rg_tempo_opts &o, RgTpTrack *out) {
    uint32_t e[RG_TEMPO_BANDS + 1];
    memset(out, 0, sizeof *out);
    out->k = k;
    out->rate_ok = rate && rg_tempo_bands(rate, e) == RG_OK ? 1u : 0u;
    if (!out->rate_ok) return;
    out->pmax = (uint32_t)(15ull * rate / (8ull * o.min_bpm));
    out->kh = std::min<uint32_t>(RG_TEMPO_MAX_HARMONICS, 16u * (o.window - 2u) / out->pmax);
    out->windows = k >= 2u * o.window ? (k - 2u * o.window) / o.hop + 1u : 0u;
}

uint64_t rg_tp_stage2_plan(RgTpTrack *tracks, size_t n) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        tracks[i].first_win = at;
        if (tracks[i].kh) at += tracks[i].windows;
    }
    return at;
}

// window w of a track: c[0 .. W) <- c_w, -> P16_w
static uint32_t window_host(const uint16_t *o, const RgTpTrack &t, const rg_tempo_opts &opts, uint32_t w, int32_t *c) {
    const uint32_t W = opts.window;
    const uint16_t *x = o + (size_t)w * opts.hop;
    uint64_t A = 0;
    for (uint32_t i = 0; i < W; ++i) A += x[i];
    for (uint32_t d = 0; d < W; ++d) {
        uint32_t R = 0;
        uint64_t B = 0;
        for (uint32_t i = 0; i < W; ++i) {
            R += (uint32_t)x[i] * (uint32_t)x[i + d];
            B += x[i + d];
        }
        c[d] = (int32_t)((int64_t)R - (int64_t)(A * B / W));
    }
    RgTpBest best{0, 0u, 0u};
    for (uint32_t p = t.pmax / 2u + 1u; p <= t.pmax; ++p) {
        const RgTpBest cand{rg_tp_score(c, p, t.kh), p, 0u};
        if (rg_tp_better(cand, best)) best = cand;
    }
    return best.p16;
}

void rg_tp_stage2_host(const uint16_t *onsets, const RgTpTrack &t, const rg_tempo_opts &o, RgTpFinish *out, int64_t *acf) {
    const uint32_t W = o.window;
    *out = RgTpFinish{0u, 0u, 0u, 0u};
    if (acf)
        for (uint32_t d = 0; d < W; ++d) acf[d] = 0;
    if (!t.windows || !t.kh) return;
    const uint16_t *x = onsets + t.onsets_at;
    std::vector<int64_t> C(W, 0);
    std::vector<int32_t> c(W);
    std::vector<uint32_t> pw(t.windows);
    for (uint32_t w = 0; w < t.windows; ++w) {
        pw[w] = window_host(x, t, o, w, c.data());
        for (uint32_t d = 0; d < W; ++d) C[d] += c[d];
    }
    if (acf) memcpy(acf, C.data(), W * sizeof(int64_t));
    if (C[0] <= 0) return;
    RgTpBest best{0, 0u, 0u};
    for (uint32_t p = t.pmax / 2u + 1u; p <= t.pmax; ++p) {
        const RgTpBest cand{rg_tp_score(C.data(), p, t.kh), p, 0u};
        if (rg_tp_better(cand, best)) best = cand;
    }
    uint32_t stable = 0;
    for (uint32_t w = 0; w < t.windows; ++w) stable += rg_tp_window_stable(pw[w], best.p16) ? 1u : 0u;
    RgTpPhase phase{0u, 0u, 0u};
    for (uint32_t phi = 0; phi < best.p16; ++phi) {
        const RgTpPhase cand = rg_tp_phase(x, t.k, best.p16, phi);
        if (rg_tp_phase_better(cand, phase)) phase = cand;
    }
    rg_tp_close(best, C[0], t.kh, stable, t.windows, phase, out);
}

void rg_tp_fill(const rg_track_desc *d, uint32_t rate, uint32_t band_frames, const RgTpTrack &t, const RgTpFinish &f, uint32_t dropped_frames,
                uint32_t nonfinite_frames, uint64_t onsets_at, rg_tempo_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = d ? d->frames : 0u;
    out->sample_rate = rate;
    out->channels = d ? d->channels : 0u;
    out->format = d ? d->format : 0u;
    out->dropped_frames = dropped_frames;
    out->onsets = t.k;
    out->windows = t.windows;
    out->harmonics = t.kh;
    out->nonfinite_frames = nonfinite_frames;
    out->band_frames = band_frames;
    out->onsets_at = onsets_at;
    out->flags = (dropped_frames == 0 ? RG_TEMPO_COMPLETE : 0u) | (nonfinite_frames ? RG_TEMPO_NONFINITE : 0u);
    if (!t.rate_ok) {
        out->flags |= RG_TEMPO_RATE | RG_TEMPO_SHORT;
        return;
    }
    if (!t.windows) out->flags |= RG_TEMPO_SHORT;
    if (!t.kh) out->flags |= RG_TEMPO_RANGE;
    if (!t.windows || !t.kh) return;
    if (!f.period16) {
        out->flags |= RG_TEMPO_NONE;
        return;
    }
    out->period16 = f.period16;
    out->bpm_milli = (uint32_t)((2ull * 1875ull * rate + f.period16) / (2ull * f.period16));
    out->confidence_permille = f.confidence_permille;
    out->stable_permille = f.stable_permille;
    out->first_beat = f.first_beat;
}

int rg_tp_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_tempo_opts &o, rg_tempo_result *out,
                     uint16_t *onsets_out, float *bands_out, char *err, size_t err_len) {
    int rc = rg_pcm_check_host_route("rg_tempo_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgFpTrack> tracks(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_tp_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    uint64_t fmt_tile[4];
    (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    std::vector<uint16_t> curve;
    for (size_t i = 0; i < n; ++i) {
        const RgFpTrack &t = tracks[i];
        const uint32_t k = t.frames ? t.frames - 1u : 0u;
        curve.assign((size_t)k + 1, 0);
        float *bands = bands_out ? bands_out + t.frames_at * RG_TEMPO_BANDS : nullptr;
        const uint32_t nonfinite = route == 0 ? rg_tp_serial_host(base, t, curve.data(), bands) : rg_tp_folded_host(base, t, curve.data(), bands);
        if (onsets_out && k) memcpy(onsets_out + t.codes_at, curve.data(), (size_t)k * sizeof(uint16_t));
        RgTpTrack s2;
        RgTpFinish f;
        rg_tp_stage2_track(descs[i].sample_rate, k, o, &s2);
        rg_tp_stage2_host(curve.data(), s2, o, &f, nullptr);
        rg_tp_fill(&descs[i], descs[i].sample_rate, t.frames, s2, f, 0, nonfinite, t.codes_at, &out[i]);
    }
    return RG_OK;
}

int rg_tp_from_onsets_check(size_t n, const uint32_t *counts, const uint16_t *onsets, char *err, size_t err_len) {
    uint64_t total = 0;
    for (size_t t = 0; t < n; ++t) {
        if (counts[t] >= (1u << 23)) {
            snprintf(err, err_len, "rg_tempo_from_onsets: track %zu has %u onsets, at most 2^23 - 1", t, counts[t]);
            return RG_ERR_INVALID_ARG;
        }
        total += counts[t];
    }
    for (uint64_t k = 0; k < total; ++k)
        if (onsets[k] > RG_TEMPO_ONSET_MAX) {
            snprintf(err, err_len, "rg_tempo_from_onsets: onset %llu is %u, at most %u", (unsigned long long)k, (unsigned)onsets[k], RG_TEMPO_ONSET_MAX);
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

int rg_tp_from_onsets_host(size_t n, const uint32_t *counts, const uint32_t *rates, const uint16_t *onsets, const rg_tempo_opts &o, rg_tempo_result *out,
                           int64_t *acf_out) {
    uint64_t at = 0;
    for (size_t t = 0; t < n; ++t) {
        RgTpTrack s2;
        RgTpFinish f;
        rg_tp_stage2_track(rates[t], counts[t], o, &s2);
        s2.onsets_at = at;
        rg_tp_stage2_host(onsets, s2, o, &f, acf_out ? acf_out + t * o.window : nullptr);
        rg_tp_fill(nullptr, rates[t], 0, s2, f, 0, 0, at, &out[t]);
        at += counts[t];
    }
    return RG_OK;
}

extern "C" int rg_tempo_kernel_shape(uint32_t *tile_onsets, uint32_t *lanes, uint32_t *lds_bytes, uint32_t *acf_lanes, uint32_t *lags_per_lane) {
    if (tile_onsets) *tile_onsets = RG_TP_TILE_ONSETS;
    if (lanes) *lanes = RG_FP_LANES;
    if (lds_bytes) *lds_bytes = (uint32_t)(16u * 306u * sizeof(RgSpecC) + RG_FP_STAGE * sizeof(float) + (RG_FP_TILE_FRAMES * RG_TEMPO_BANDS + RG_TEMPO_BANDS + 1u) * 4u);
    if (acf_lanes) *acf_lanes = RG_TP_ACF_LANES;
    if (lags_per_lane) *lags_per_lane = RG_TP_LAGS_PER_LANE;
    return RG_OK;
}
