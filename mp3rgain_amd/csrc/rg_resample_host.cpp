// rg_resample_host.cpp -- the host side of the rational resampler and of the cross-rate fingerprint
// (include/mp3rgain_amd_resample.h, rg_resample.h): the ratio, the window of an output and the tap tables, the track records and
// their checks, the plan of a launch (with every workgroup's start, formed in 64 bits), route 0 (the sum in double) and the
// kernel's arithmetic walked by the host (route 2: the sum in f32 in tap order), and both followed by the fingerprint's host
// routes on y (rg_fprint.h).  Plain C++: no device and no context, so a sanitizer build needs nothing else but
// rg_fprint_host.cpp and rg_spectrum_host.cpp.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "rg_resample.h"

// L, M of a rate; -> supported
static bool rs_ratio(uint32_t rate, uint32_t *up, uint32_t *down) {
    const uint32_t g = rg_rs_gcd(rate, RG_RS_RATE_OUT);
    *up = RG_RS_RATE_OUT / g;
    *down = rate / g;
    return rate >= RG_RS_MIN_RATE && *up <= RG_RS_MAX_PHASES && (uint64_t)*down <= (uint64_t)RG_RS_MAX_RATIO * *up;
}
static uint32_t rs_half(uint32_t up, uint32_t down) { return RG_RS_HALF_PER_W * std::max(up, down); }
static uint32_t rs_taps(uint32_t up, uint32_t down) { return up == 1 && down == 1 ? 1u : 2u * rs_half(up, down) / up + 1u; }

extern "C" int rg_resample_plan(uint32_t sample_rate, uint32_t *up, uint32_t *down, uint32_t *taps) {
    if (!up || !down || !taps || !sample_rate) return RG_ERR_INVALID_ARG;
    const bool ok = rs_ratio(sample_rate, up, down);
    *taps = ok ? rs_taps(*up, *down) : 0u;
    return ok ? RG_OK : RG_ERR_UNSUPPORTED_RATE;
}

extern "C" int rg_resample_window(uint32_t sample_rate, uint64_t j, uint64_t *first, uint32_t *phase) {
    uint32_t up, down;
    if (!first || !phase || !sample_rate || j >= ((uint64_t)1 << 32)) return RG_ERR_INVALID_ARG;
    if (!rs_ratio(sample_rate, &up, &down)) return RG_ERR_UNSUPPORTED_RATE;
    rg_rs_window(j, up, down, first, phase);
    return RG_OK;
}

extern "C" int rg_resample_filter(uint32_t up, uint32_t down, float *taps) {
    if (!taps || !up || !down || up > RG_RS_MAX_PHASES || (uint64_t)down > (uint64_t)RG_RS_MAX_RATIO * up || rg_rs_gcd(up, down) != 1) return RG_ERR_INVALID_ARG;
    if (up == 1 && down == 1) {
        taps[0] = 1.0f;
        return RG_OK;
    }
    // (written as rg_key_filter writes its prototype: at L = 1 the two tables are the same bytes)
    const double pi = 3.14159265358979323846;
    const int32_t half = (int32_t)rs_half(up, down), P = (int32_t)rs_taps(up, down);
    const double fc = 0.45 / (double)std::max(up, down);
    std::vector<double> h((size_t)P);
    for (int32_t p = 0; p < (int32_t)up; ++p) {
        double sum = 0.0;
        for (int32_t k = 0; k < P; ++k) {
            const int32_t at = p + k * (int32_t)up - half;
            double g = 0.0;
            if (at <= half) {  // (at >= -half always)
                const double n = (double)at, t = 2.0 * fc * n;
                const double sinc = at == 0 ? 1.0 : std::sin(pi * t) / (pi * t);
                g = 2.0 * fc * sinc * (0.42 + 0.5 * std::cos(pi * n / half) + 0.08 * std::cos(2.0 * pi * n / half));
            }
            h[(size_t)k] = g;
            sum += g;
        }
        for (int32_t k = 0; k < P; ++k) taps[(size_t)p * P + k] = (float)(h[(size_t)k] / sum);
    }
    return RG_OK;
}

std::shared_ptr<const RgRsFilter> rg_rs_filter(uint32_t up, uint32_t down) {
    static std::mutex mu;
    static std::map<uint64_t, std::shared_ptr<const RgRsFilter>> cache;
    const uint64_t key = ((uint64_t)up << 32) | down;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    auto f = std::make_shared<RgRsFilter>();
    f->up = up;
    f->down = down;
    f->taps = rs_taps(up, down);
    f->h.assign((size_t)up * f->taps, 0.0f);
    (void)rg_resample_filter(up, down, f->h.data());
    f->hq.assign((size_t)up * f->taps, 0.0f);
    for (uint32_t r = 0; r < up; ++r) {  // output j of residue r has phase (-r M) mod L
        uint64_t b;
        uint32_t p;
        rg_rs_window(r, up, down, &b, &p);
        for (uint32_t k = 0; k < f->taps; ++k) f->hq[(size_t)k * up + r] = f->h[(size_t)p * f->taps + k];
    }
    cache[key] = f;
    return f;
}

int rg_xr_options(const rg_fingerprint_opts *opts, rg_fingerprint_opts *out, char *err, size_t err_len) {
    rg_fingerprint_opts o = opts ? *opts : rg_fingerprint_opts{0, 0, 0, 0};
    if (!o.block) o.block = RG_XR_BLOCK;
    if (!o.probes) o.probes = RG_XR_PROBES;
    if (!o.radius) o.radius = RG_XR_RADIUS;
    if (!o.max_ber_permille) o.max_ber_permille = RG_XR_MAX_BER_PERMILLE;
    return rg_fp_options(&o, out, err, err_len);
}

int rg_rs_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgRsTrack *out, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_RS_MAX_CHANNELS, "the resampler takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    memset(out, 0, sizeof *out);
    out->off0 = rg_pcm_plane_off(t, 0);
    out->off1 = t.channels >= 2 ? rg_pcm_plane_off(t, 1) : out->off0;
    out->n = (uint32_t)t.frames;
    out->format = t.format;
    out->channels = t.channels >= 2 ? 2u : 1u;
    uint32_t up = 0, down = 0;
    if (!t.sample_rate || !rs_ratio(t.sample_rate, &up, &down)) {  // up = 0: RG_RS_RATE (the record tells L and M from the rate)
        return RG_OK;
    }
    out->up = up;
    out->down = down;
    out->taps = rs_taps(up, down);
    const uint64_t m = rg_rs_count(t.frames, up, down, out->taps);
    if (m >= ((uint64_t)1 << 32)) {
        snprintf(err, err_len, "track %zu: %llu frames at %u Hz make 2^32 resampled samples or more", i, (unsigned long long)t.frames, t.sample_rate);
        return RG_ERR_FORMAT;
    }
    out->m = (uint32_t)m;
    out->recip = (uint32_t)(0xFFFFFFFFu / up) + 1u;  // (L = 1 never divides)
    out->n_wg = up == 1 ? 0u : (out->m + RG_RS_OUTPUTS - 1u) / RG_RS_OUTPUTS;
    out->span = (uint32_t)(((uint64_t)(RG_RS_OUTPUTS - 1u) * down + up - 1u) / up) + out->taps;
    return RG_OK;
}

uint64_t rg_rs_plan(RgRsTrack *tracks, size_t n, uint64_t fmt_wg[4], std::vector<float> *tables, std::vector<RgRsStart> *starts) {
    uint64_t wg = 0, y = 0;
    starts->clear();
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_wg[f] = wg;
        for (size_t i = 0; i < n; ++i) {
            RgRsTrack &t = tracks[i];
            if (t.format != f) continue;
            t.first_wg = wg;
            wg += t.n_wg;
            for (uint32_t w = 0; w < t.n_wg; ++w) {
                const uint64_t j0 = (uint64_t)w * RG_RS_OUTPUTS;
                uint64_t b;
                uint32_t p;
                rg_rs_window(j0, t.up, t.down, &b, &p);  // b + P <= N < 2^32
                starts->push_back(RgRsStart{(uint32_t)b, p | (uint32_t)(j0 % t.up) << 16});
            }
        }
    }
    fmt_wg[3] = wg;
    std::map<uint64_t, uint32_t> at;
    tables->clear();
    for (size_t i = 0; i < n; ++i) {
        RgRsTrack &t = tracks[i];
        t.y_at = y;
        y += ((uint64_t)t.m + 3u) & ~(uint64_t)3;
        if (t.up < 2 || !t.n_wg) continue;
        const uint64_t key = ((uint64_t)t.up << 32) | t.down;
        auto it = at.find(key);
        if (it == at.end()) {
            const std::shared_ptr<const RgRsFilter> f = rg_rs_filter(t.up, t.down);
            it = at.emplace(key, (uint32_t)tables->size()).first;
            tables->insert(tables->end(), f->hq.begin(), f->hq.end());
        }
        t.hq_at = it->second;
    }
    return y;
}

// the down-mixed signal of a track as the kernels see it
static RgFpTrack rs_signal(const RgRsTrack &t) {
    RgFpTrack s;
    memset(&s, 0, sizeof s);
    s.off0 = t.off0;
    s.off1 = t.off1;
    s.format = t.format;
    s.channels = t.channels;
    return s;
}

template <class Acc>
static void rs_host(const unsigned char *arena, const RgRsTrack &t, float *y) {
    if (!t.m) return;
    const RgFpTrack sig = rs_signal(t);
    if (t.up == 1 && t.down == 1) {
        for (uint32_t j = 0; j < t.m; ++j) y[j] = rg_fp_signal_at(arena, sig, j);
        return;
    }
    const std::shared_ptr<const RgRsFilter> f = rg_rs_filter(t.up, t.down);
    std::vector<float> x(t.n);
    for (uint32_t k = 0; k < t.n; ++k) x[k] = rg_fp_signal_at(arena, sig, k);
    for (uint32_t j = 0; j < t.m; ++j) {
        uint64_t b;
        uint32_t p;
        rg_rs_window(j, t.up, t.down, &b, &p);
        const float *h = &f->h[(size_t)p * t.taps], *xj = &x[(size_t)b];
        Acc s = 0;
        for (uint32_t k = 0; k < t.taps; ++k) {
            const Acc prod = (Acc)h[k] * (Acc)xj[k];
            s += prod;
        }
        y[j] = (float)s;
    }
}
void rg_rs_serial_host(const unsigned char *arena, const RgRsTrack &t, float *y) { rs_host<double>(arena, t, y); }
void rg_rs_folded_host(const unsigned char *arena, const RgRsTrack &t, float *y) { rs_host<float>(arena, t, y); }

void rg_xr_fp_track(const RgRsTrack &t, uint64_t off, RgFpTrack *out) {
    memset(out, 0, sizeof *out);
    out->off0 = out->off1 = off;
    out->n = t.m;
    out->format = RG_FMT_F32_PLANAR;
    out->channels = 1;
    out->rate_ok = t.up && rg_fingerprint_edges(RG_RS_RATE_OUT, out->e) == RG_OK ? 1u : 0u;
    out->frames = out->rate_ok ? rg_fp_frames(t.m) : 0u;
    out->n_tiles = !out->frames ? 0u : std::max(1u, (out->frames - 1u + RG_FP_TILE_CODES - 1u) / RG_FP_TILE_CODES);
}

void rg_rs_fill(const rg_track_desc &d, const RgRsTrack &t, uint64_t y_at, rg_resample_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = d.frames;
    out->sample_rate = d.sample_rate;
    out->channels = d.channels;
    out->format = d.format;
    if (d.sample_rate) (void)rs_ratio(d.sample_rate, &out->up, &out->down);
    out->taps = t.taps;
    out->resampled = t.m;
    out->y_at = y_at;
    out->flags = (!t.up ? RG_RS_RATE : 0u) | (!t.m ? RG_RS_SHORT : 0u);
}

void rg_xr_fill(const rg_track_desc &d, const RgRsTrack &t, const RgFpTrack &f, uint32_t dropped_frames, uint32_t nonfinite_frames, uint32_t index,
                uint64_t y_at, rg_xrate_result *out) {
    rg_fingerprint_result r;
    rg_fp_fill(d, f, dropped_frames, nonfinite_frames, index, &r);
    memset(out, 0, sizeof *out);
    static_assert(sizeof(rg_fingerprint_result) == 72 && sizeof(rg_xrate_result) == 96, "the cross-rate record starts with the fingerprint's");
    memcpy(out, &r, sizeof r);
    if (d.sample_rate) (void)rs_ratio(d.sample_rate, &out->up, &out->down);
    out->resampled = t.m;
    out->y_at = y_at;
}

int rg_rs_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_resample_result *out, float *y_out, char *err,
                     size_t err_len) {
    int rc = rg_pcm_check_host_route("rg_resample_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgRsTrack> tracks(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_rs_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    std::vector<float> y;
    uint64_t y_at = 0;
    for (size_t i = 0; i < n; ++i) {
        const RgRsTrack &t = tracks[i];
        y.assign((size_t)t.m + 1, 0.0f);
        if (route == 0) rg_rs_serial_host(base, t, y.data()); else rg_rs_folded_host(base, t, y.data());
        if (y_out && t.m) memcpy(y_out + y_at, y.data(), (size_t)t.m * sizeof(float));
        rg_rs_fill(descs[i], t, y_at, &out[i]);
        y_at += t.m;
    }
    return RG_OK;
}

int rg_xr_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_xrate_result *out, uint32_t *codes_out,
                     float *bands_out, float *y_out, char *err, size_t err_len) {
    int rc = rg_pcm_check_host_route("rg_xrate_fingerprint_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgRsTrack> tracks(n + 1);
    std::vector<RgFpTrack> fp(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_rs_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
        rg_xr_fp_track(tracks[i], 0, &fp[i]);  // every track's y is an arena of its own here
    }
    uint64_t fmt_tile[4];
    (void)rg_fp_plan(fp.data(), n, fmt_tile, 0, 0);
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    std::vector<float> y;
    uint64_t y_at = 0;
    for (size_t i = 0; i < n; ++i) {
        const RgRsTrack &t = tracks[i];
        const RgFpTrack &f = fp[i];
        y.assign((size_t)t.m + 1, 0.0f);
        if (route == 0) rg_rs_serial_host(base, t, y.data()); else rg_rs_folded_host(base, t, y.data());
        if (y_out && t.m) memcpy(y_out + y_at, y.data(), (size_t)t.m * sizeof(float));
        uint32_t *codes = codes_out ? codes_out + f.codes_at : nullptr;
        float *bands = bands_out ? bands_out + f.frames_at * RG_FP_BANDS : nullptr;
        const unsigned char *ya = reinterpret_cast<const unsigned char *>(y.data());
        const uint32_t nonfinite = route == 0 ? rg_fp_serial_host(ya, f, codes, bands) : rg_fp_folded_host(ya, f, codes, bands);
        rg_xr_fill(descs[i], t, f, 0, nonfinite, (uint32_t)i, y_at, &out[i]);
        y_at += t.m;
    }
    return RG_OK;
}

extern "C" int rg_resample_kernel_shape(uint32_t *outputs, uint32_t *lanes, uint32_t *max_span) {
    if (outputs) *outputs = RG_RS_OUTPUTS;
    if (lanes) *lanes = RG_RS_LANES;
    if (max_span) *max_span = RG_RS_MAX_SPAN;
    return RG_OK;
}
