// rg_key_host.cpp -- the host side of the key scan (include/mp3rgain_amd_key.h, rg_key.h): the decimation factor, the band
// edges and the filter tables, the options, the track records and their checks, the plan of a launch, the serial host twin of
// stage 1 (route 0: the FIR sum, the transform and the band sums in double), the kernels' arithmetic walked by the host (route
// 2: the FIR sum in f32 in tap order, then the fingerprint's tile walk, rg_fprint.h, on the decimated signal), and stage 2 as a
// serial twin of the finish kernel.  Plain C++: no device and no context, so a sanitizer build needs nothing else but
// rg_spectrum_host.cpp for the tables.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "rg_key.h"

static uint32_t key_decim(uint32_t sample_rate) { return sample_rate / RG_KEY_TARGET_RATE; }

extern "C" int rg_key_bands(uint32_t sample_rate, uint32_t *decim, uint32_t *edges) {
    if (!edges || !decim || !sample_rate) return RG_ERR_INVALID_ARG;
    const uint32_t D = key_decim(sample_rate);
    *decim = D;
    if (!D || D > RG_KEY_MAX_DECIM) return RG_ERR_UNSUPPORTED_RATE;
    const double fd = (double)sample_rate / (double)D;
    for (uint32_t s = 0; s <= RG_KEY_BANDS; ++s) {
        const double e = std::floor(440.0 * std::pow(2.0, ((double)s - 33.5) / 12.0) * RG_KEY_FRAME / fd + 0.5);
        edges[s] = (uint32_t)e;
        edges[s] = s ? std::max(edges[s], edges[s - 1] + 1u) : std::max(edges[s], 1u);
    }
    return edges[RG_KEY_BANDS] <= RG_KEY_FRAME / 2 ? RG_OK : RG_ERR_UNSUPPORTED_RATE;
}

extern "C" int rg_key_filter(uint32_t decim, float *taps) {
    if (!taps || decim < 2 || decim > RG_KEY_MAX_DECIM) return RG_ERR_INVALID_ARG;
    const double pi = 3.14159265358979323846;
    const int32_t half = (int32_t)(RG_KEY_TAPS_PER_DECIM / 2u * decim), count = 2 * half + 1;
    const double fc = 0.45 / (double)decim;
    std::vector<double> h((size_t)count);
    double sum = 0.0;
    for (int32_t k = 0; k < count; ++k) {
        const double n = (double)(k - half), t = 2.0 * fc * n;
        const double sinc = k == half ? 1.0 : std::sin(pi * t) / (pi * t);
        h[(size_t)k] = 2.0 * fc * sinc * (0.42 + 0.5 * std::cos(pi * n / half) + 0.08 * std::cos(2.0 * pi * n / half));
        sum += h[(size_t)k];
    }
    for (int32_t k = 0; k < count; ++k) taps[k] = (float)(h[(size_t)k] / sum);
    return RG_OK;
}

const std::vector<float> &rg_key_taps(uint32_t decim) {
    static std::vector<float> table[RG_KEY_MAX_DECIM + 1];
    static std::once_flag once[RG_KEY_MAX_DECIM + 1];
    std::call_once(once[decim], [decim] {
        table[decim].assign((size_t)RG_KEY_TAPS_PER_DECIM * decim + 1u, 0.0f);
        (void)rg_key_filter(decim, table[decim].data());
    });
    return table[decim];
}

int rg_key_options(const rg_key_opts *opts, rg_key_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_key_opts{0};
    if (!out->segment) out->segment = RG_KEY_SEGMENT;
    if (out->segment >= RG_KEY_MIN_SEGMENT && out->segment <= RG_KEY_MAX_SEGMENT) return RG_OK;
    snprintf(err, err_len, "key: segment %u (%u to %u rows)", out->segment, RG_KEY_MIN_SEGMENT, RG_KEY_MAX_SEGMENT);
    return RG_ERR_INVALID_ARG;
}

int rg_key_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgKeyTrack *out, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_KEY_MAX_CHANNELS, "the key scan takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    memset(out, 0, sizeof *out);
    out->off0 = rg_pcm_plane_off(t, 0);
    out->off1 = t.channels >= 2 ? rg_pcm_plane_off(t, 1) : out->off0;
    out->n = (uint32_t)t.frames;
    out->format = t.format;
    out->channels = t.channels >= 2 ? 2u : 1u;
    uint32_t D = 0;
    if (!t.sample_rate || rg_key_bands(t.sample_rate, &D, out->e) != RG_OK) return RG_OK;  // decim = 0: RG_KEY_RATE
    out->decim = D;
    out->recip = (uint32_t)(0xFFFFFFFFu / D) + 1u;  // (D = 1 never divides)
    const uint64_t taps = (uint64_t)RG_KEY_TAPS_PER_DECIM * D + 1u;
    out->m = D == 1 ? out->n : t.frames < taps ? 0u : (uint32_t)((t.frames - taps) / D + 1u);
    out->rows = rg_fp_frames(out->m);
    out->n_wg = (out->m + RG_KEY_DECIM_OUTPUTS - 1u) / RG_KEY_DECIM_OUTPUTS;
    return RG_OK;
}

uint64_t rg_key_plan(RgKeyTrack *tracks, size_t n, uint64_t fmt_wg[4], std::vector<float> *taps, uint64_t *rows) {
    uint64_t wg = 0, y = 0, r = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_wg[f] = wg;
        for (size_t i = 0; i < n; ++i) {
            if (tracks[i].format != f) continue;
            tracks[i].first_wg = wg;
            wg += tracks[i].n_wg;
        }
    }
    fmt_wg[3] = wg;
    uint32_t at[RG_KEY_MAX_DECIM + 1];
    for (uint32_t d = 0; d <= RG_KEY_MAX_DECIM; ++d) at[d] = UINT32_MAX;
    taps->clear();
    for (size_t i = 0; i < n; ++i) {
        RgKeyTrack &t = tracks[i];
        t.y_at = y;
        t.rows_at = r;
        y += ((uint64_t)t.m + 3u) & ~(uint64_t)3;
        r += t.rows;
        if (t.decim < 2) continue;
        if (at[t.decim] == UINT32_MAX) {
            const std::vector<float> &h = rg_key_taps(t.decim);
            at[t.decim] = (uint32_t)taps->size();
            taps->insert(taps->end(), h.begin(), h.end());
        }
        t.taps_at = at[t.decim];
    }
    *rows = r;
    return y;
}

void rg_key_fp_track(const RgKeyTrack &t, uint64_t off, RgFpTrack *out) {
    memset(out, 0, sizeof *out);
    out->off0 = out->off1 = off;
    out->n = t.m;
    out->frames = t.rows;
    out->n_tiles = !t.rows ? 0u : std::max(1u, (t.rows - 1u + RG_KEY_TILE_ROWS - 1u) / RG_KEY_TILE_ROWS);
    out->format = RG_FMT_F32_PLANAR;
    out->channels = 1;
    out->rate_ok = t.decim ? 1u : 0u;
}

// the down-mixed signal of a track as the kernels see it
static RgFpTrack key_signal(const RgKeyTrack &t) {
    RgFpTrack s;
    memset(&s, 0, sizeof s);
    s.off0 = t.off0;
    s.off1 = t.off1;
    s.format = t.format;
    s.channels = t.channels;
    return s;
}

// ---- stage 1, route 0: the definitions ------------------------------------------------------------------------------------
uint32_t rg_key_serial_host(const unsigned char *arena, const RgKeyTrack &t, float *y, float *bands, uint16_t *rows) {
    const RgFpTrack sig = key_signal(t);
    if (t.decim == 1) {
        for (uint32_t j = 0; j < t.m; ++j) y[j] = rg_fp_signal_at(arena, sig, j);
    } else if (t.m) {
        const std::vector<float> &h = rg_key_taps(t.decim);
        std::vector<float> x(t.n);
        for (uint32_t k = 0; k < t.n; ++k) x[k] = rg_fp_signal_at(arena, sig, k);
        for (uint32_t j = 0; j < t.m; ++j) {
            double s = 0.0;
            const float *xj = &x[(size_t)j * t.decim];
            for (size_t k = 0; k < h.size(); ++k) s += (double)h[k] * (double)xj[k];
            y[j] = (float)s;
        }
    }
    const RgSpecTables &tb = rg_spec_tables();
    std::vector<double> re(RG_FP_FRAME), im(RG_FP_FRAME);
    float cur[RG_KEY_BANDS];
    uint32_t nonfinite = 0;
    for (uint32_t n = 0; n < t.rows; ++n) {
        bool bad = false;
        for (uint32_t k = 0; k < RG_FP_FRAME; ++k) {
            const float v = y[(size_t)n * RG_FP_HOP + k];
            bad |= rg_fp_nonfinite(v);
            re[k] = (double)v * (double)tb.window[k];
            im[k] = 0.0;
        }
        if (bad) {
            ++nonfinite;
            for (uint32_t s = 0; s < RG_KEY_BANDS; ++s) cur[s] = 0.0f;
        } else {
            rg_fp_fft_double(re.data(), im.data());
            for (uint32_t s = 0; s < RG_KEY_BANDS; ++s) {
                double sum = 0.0;
                for (uint32_t b = t.e[s]; b < t.e[s + 1]; ++b) sum += re[b] * re[b] + im[b] * im[b];
                cur[s] = (float)sum;
            }
        }
        if (bands) memcpy(bands + (size_t)n * RG_KEY_BANDS, cur, sizeof cur);
        rg_key_row(cur, rows + (size_t)n * RG_KEY_CHROMA);
    }
    return nonfinite;
}

// ---- stage 1, route 2: the kernels' arithmetic -----------------------------------------------------------------------------
uint32_t rg_key_folded_host(const unsigned char *arena, const RgKeyTrack &t, float *y, float *bands, uint16_t *rows) {
    const RgFpTrack sig = key_signal(t);
    if (t.decim == 1) {
        for (uint32_t j = 0; j < t.m; ++j) y[j] = rg_fp_signal_at(arena, sig, j);
    } else if (t.m) {
        const std::vector<float> &h = rg_key_taps(t.decim);
        std::vector<float> x(t.n);
        for (uint32_t k = 0; k < t.n; ++k) x[k] = rg_fp_signal_at(arena, sig, k);
        for (uint32_t j = 0; j < t.m; ++j) {
            float s = 0.0f;
            const float *xj = &x[(size_t)j * t.decim];
            for (size_t k = 0; k < h.size(); ++k) {
                const float prod = h[k] * xj[k];
                s += prod;
            }
            y[j] = s;
        }
    }
    RgFpTrack ft;
    rg_key_fp_track(t, 0, &ft);
    uint32_t nonfinite = 0;
    float E[RG_FP_TILE_FRAMES * RG_KEY_BANDS];
    for (uint32_t tile = 0; tile < ft.n_tiles; ++tile) {
        uint32_t nf = 0;
        const uint32_t f0 = tile * RG_KEY_TILE_ROWS;
        nonfinite += rg_fp_tile_bands_host<RG_KEY_BANDS>(reinterpret_cast<const unsigned char *>(y), ft, tile, E, &nf, t.e);
        for (uint32_t i = tile ? 1u : 0u; i < nf; ++i) {
            if (bands) memcpy(bands + (size_t)(f0 + i) * RG_KEY_BANDS, &E[i * RG_KEY_BANDS], RG_KEY_BANDS * sizeof(float));
            rg_key_row(&E[i * RG_KEY_BANDS], rows + (size_t)(f0 + i) * RG_KEY_CHROMA);
        }
    }
    return nonfinite;
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------------------
void rg_key_stage2_host(const uint16_t *rows, uint32_t F, const rg_key_opts &o, RgKeyFinish *out) {
    uint64_t H[12] = {0};
    uint32_t silent = 0;
    for (uint32_t n = 0; n < F; ++n) {
        const uint16_t *r = rows + (size_t)n * RG_KEY_CHROMA;
        for (uint32_t p = 0; p < 12; ++p) H[p] += r[p];
        silent += rg_key_row_silent(r) ? 1u : 0u;
    }
    RgKeyPick pick;
    rg_key_pick(H, &pick);
    const uint32_t G = F / o.segment;
    uint32_t nonzero = 0, agreeing = 0;
    for (uint32_t g = 0; g < G; ++g) {
        uint64_t Hg[12];
        if (!rg_key_segment_sums(rows, g, o.segment, Hg)) continue;
        RgKeyPick sp;
        rg_key_pick(Hg, &sp);
        ++nonzero;
        agreeing += !sp.none && sp.key == pick.key ? 1u : 0u;
    }
    rg_key_finish(pick, silent, G, nonzero, agreeing, out);
}

void rg_key_fill(const rg_track_desc *d, const RgKeyTrack *t, uint32_t F, const RgKeyFinish &f, uint32_t dropped_frames, uint32_t nonfinite_frames,
                 uint64_t chroma_at, rg_key_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = d ? d->frames : 0u;
    out->sample_rate = d ? d->sample_rate : 0u;
    out->channels = d ? d->channels : 0u;
    out->format = d ? d->format : 0u;
    out->dropped_frames = dropped_frames;
    out->decim = t ? t->decim : 0u;
    out->decimated = t ? t->m : 0u;
    out->rows = F;
    out->nonfinite_frames = nonfinite_frames;
    out->chroma_at = chroma_at;
    out->flags = (dropped_frames == 0 ? RG_KEY_COMPLETE : 0u) | (nonfinite_frames ? RG_KEY_NONFINITE : 0u);
    if (t && !t->decim) out->flags |= RG_KEY_RATE;
    if (!F) {
        out->flags |= RG_KEY_SHORT;
        return;
    }
    out->silent_rows = f.silent_rows;
    out->segments = f.segments;
    if (f.flags & RG_KEY_NONE) {
        out->flags |= RG_KEY_NONE;
        return;
    }
    out->key = f.key;
    out->tonic = f.key % 12u;
    out->mode = f.key / 12u;
    out->correlation_permille = f.correlation_permille;
    out->margin_permille = f.margin_permille;
    out->stable_permille = f.stable_permille;
}

int rg_key_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, const rg_key_opts &o, rg_key_result *out,
                      float *decim_out, float *bands_out, uint16_t *chroma_out, char *err, size_t err_len) {
    int rc = rg_pcm_check_host_route("rg_key_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgKeyTrack> tracks(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_key_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    std::vector<float> y;
    std::vector<uint16_t> rows;
    uint64_t y_at = 0, rows_at = 0;
    for (size_t i = 0; i < n; ++i) {
        const RgKeyTrack &t = tracks[i];
        y.assign((size_t)t.m + 1, 0.0f);
        rows.assign((size_t)t.rows * RG_KEY_CHROMA + 1, 0);
        float *bands = bands_out ? bands_out + rows_at * RG_KEY_BANDS : nullptr;
        const uint32_t nonfinite = route == 0 ? rg_key_serial_host(base, t, y.data(), bands, rows.data()) : rg_key_folded_host(base, t, y.data(), bands, rows.data());
        if (decim_out && t.m) memcpy(decim_out + y_at, y.data(), (size_t)t.m * sizeof(float));
        if (chroma_out && t.rows) memcpy(chroma_out + rows_at * RG_KEY_CHROMA, rows.data(), (size_t)t.rows * RG_KEY_CHROMA * sizeof(uint16_t));
        RgKeyFinish f;
        rg_key_stage2_host(rows.data(), t.rows, o, &f);
        rg_key_fill(&descs[i], &t, t.rows, f, 0, nonfinite, rows_at, &out[i]);
        y_at += t.m;
        rows_at += t.rows;
    }
    return RG_OK;
}

int rg_key_from_chroma_check(size_t n, const uint32_t *counts, const uint16_t *chroma, char *err, size_t err_len) {
    uint64_t total = 0;
    for (size_t t = 0; t < n; ++t) {
        if (counts[t] >= (1u << 23)) {
            snprintf(err, err_len, "rg_key_from_chroma: track %zu has %u rows, at most 2^23 - 1", t, counts[t]);
            return RG_ERR_INVALID_ARG;
        }
        total += counts[t];
    }
    for (uint64_t k = 0; k < total * RG_KEY_CHROMA; ++k)
        if (chroma[k] > RG_KEY_ROW_MAX) {
            snprintf(err, err_len, "rg_key_from_chroma: entry %llu is %u, at most %u", (unsigned long long)k, (unsigned)chroma[k], RG_KEY_ROW_MAX);
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

int rg_key_from_chroma_host(size_t n, const uint32_t *counts, const uint16_t *chroma, const rg_key_opts &o, rg_key_result *out) {
    uint64_t at = 0;
    for (size_t t = 0; t < n; ++t) {
        RgKeyFinish f;
        rg_key_stage2_host(chroma + at * RG_KEY_CHROMA, counts[t], o, &f);
        rg_key_fill(nullptr, nullptr, counts[t], f, 0, 0, at, &out[t]);
        at += counts[t];
    }
    return RG_OK;
}

extern "C" int rg_key_kernel_shape(uint32_t *decim_outputs, uint32_t *decim_lanes, uint32_t *tile_rows, uint32_t *tile_lanes, uint32_t *tile_lds_bytes) {
    if (decim_outputs) *decim_outputs = RG_KEY_DECIM_OUTPUTS;
    if (decim_lanes) *decim_lanes = RG_KEY_DECIM_LANES;
    if (tile_rows) *tile_rows = RG_KEY_TILE_ROWS;
    if (tile_lanes) *tile_lanes = RG_FP_LANES;
    if (tile_lds_bytes) *tile_lds_bytes = RG_KEY_TILE_LDS_BYTES;
    return RG_OK;
}
