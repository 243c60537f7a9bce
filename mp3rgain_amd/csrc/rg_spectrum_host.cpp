// rg_spectrum_host.cpp -- the host side of the spectral scan (include/mp3rgain_amd_spectrum.h, rg_spectrum.h): the tables, the
// plane records and their checks, the serial host twin (route 0: the definitions in double, a plain radix-2 transform per
// frame), the kernels' arithmetic walked by the host (route 2: the same pass, band and fold functions as rg_spectrum.hip runs,
// lane by lane), and the verdict.  Plain C++: no device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rg_spectrum.h"

static const double kPi = 3.14159265358979323846;

const RgSpecTables &rg_spec_tables() {
    static const RgSpecTables *tables = [] {
        RgSpecTables *t = new RgSpecTables;
        for (uint32_t n = 0; n < RG_SPEC_FRAME; ++n) t->window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * n / RG_SPEC_FRAME));
        for (uint32_t k0 = 0; k0 < 16; ++k0)
            for (uint32_t l = 0; l < 256; ++l) {
                const double a = -2.0 * kPi * (double)(l * k0) / RG_SPEC_FRAME;
                t->tw1[k0 * 256 + l] = RgSpecC{(float)std::cos(a), (float)std::sin(a)};
            }
        for (uint32_t k1 = 0; k1 < 16; ++k1)
            for (uint32_t n0 = 0; n0 < 16; ++n0) {
                const double a = -2.0 * kPi * (double)(n0 * k1) / 256.0;
                t->tw2[k1 * 16 + n0] = RgSpecC{(float)std::cos(a), (float)std::sin(a)};
            }
        return t;
    }();
    return *tables;
}

int rg_spec_options(const rg_spectrum_opts *opts, rg_spectrum_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_spectrum_opts{RG_SPEC_EDGE_DB, RG_SPEC_MIN_CUTOFF_HZ};
    if (out->edge_db > 0.0 && out->min_cutoff_hz > 0.0 && std::isfinite(out->edge_db) && std::isfinite(out->min_cutoff_hz)) return RG_OK;
    snprintf(err, err_len, "spectrum: edge_db %g and min_cutoff_hz %g must both be greater than 0", out->edge_db, out->min_cutoff_hz);
    return RG_ERR_INVALID_ARG;
}

int rg_spec_track_planes(size_t i, const rg_track_desc &t, size_t arena_bytes, RgSpecPlane *planes, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_SPEC_MAX_CHANNELS, "the spectrum takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    for (uint32_t c = 0; c < t.channels; ++c) {
        RgSpecPlane &p = planes[c];
        memset(&p, 0, sizeof p);
        p.off = rg_pcm_plane_off(t, c);
        p.n = (uint32_t)t.frames;
        p.frames = rg_spec_frames(t.frames);
        p.format = t.format;
    }
    return RG_OK;
}

uint64_t rg_spec_plan(RgSpecPlane *planes, size_t n, uint64_t fmt_tile[4]) {
    uint64_t tiles = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_tile[f] = tiles;
        for (size_t i = 0; i < n; ++i) {
            RgSpecPlane &p = planes[i];
            if (p.format != f) continue;
            p.first_tile = tiles;
            p.n_tiles = (p.frames + RG_SPEC_TILE_FRAMES - 1) / RG_SPEC_TILE_FRAMES;
            tiles += p.n_tiles;
        }
    }
    fmt_tile[3] = tiles;
    return tiles;
}

static inline float value_at(const unsigned char *plane, uint32_t format, uint64_t k, bool *nonfinite) {
    const uint32_t raw = rg_pcm_raw_at(plane, format, k);
    switch (format) {
        case RG_FMT_F32_PLANAR: *nonfinite = rg_spec_nonfinite<RG_FMT_F32_PLANAR>(raw); return rg_spec_value<RG_FMT_F32_PLANAR>(raw);
        case RG_FMT_S16_PLANAR: *nonfinite = false; return rg_spec_value<RG_FMT_S16_PLANAR>(raw);
        default: *nonfinite = false; return rg_spec_value<RG_FMT_S32_PLANAR>(raw);
    }
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
// re, im <- their L-point DFT: decimation in time, radix 2, in double
static void fft_double(double *re, double *im) {
    const uint32_t L = RG_SPEC_FRAME;
    static const std::vector<double> *roots = [] {
        std::vector<double> *r = new std::vector<double>(RG_SPEC_FRAME);  // cos, -sin of 2 pi k / L, k < L / 2
        for (uint32_t k = 0; k < RG_SPEC_FRAME / 2; ++k) {
            (*r)[2 * k] = std::cos(2.0 * kPi * k / RG_SPEC_FRAME);
            (*r)[2 * k + 1] = -std::sin(2.0 * kPi * k / RG_SPEC_FRAME);
        }
        return r;
    }();
    for (uint32_t i = 1, j = 0; i < L; ++i) {  // bit reversal
        uint32_t bit = L >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (uint32_t len = 2; len <= L; len <<= 1) {
        const uint32_t step = L / len;
        for (uint32_t i = 0; i < L; i += len)
            for (uint32_t k = 0; k < len / 2; ++k) {
                const double wr = (*roots)[2 * k * step], wi = (*roots)[2 * k * step + 1];
                const uint32_t a = i + k, b = i + k + len / 2;
                const double xr = re[b] * wr - im[b] * wi, xi = re[b] * wi + im[b] * wr;
                re[b] = re[a] - xr;
                im[b] = im[a] - xi;
                re[a] += xr;
                im[a] += xi;
            }
    }
}

void rg_spec_serial_host(const unsigned char *arena, const RgSpecPlane &p, RgSpecPlaneOut *out) {
    const unsigned char *plane = arena + p.off;
    const RgSpecTables &tb = rg_spec_tables();
    memset(out, 0, sizeof *out);
    std::vector<double> re(RG_SPEC_FRAME), im(RG_SPEC_FRAME);
    for (uint32_t k = 0; k < p.frames; ++k) {
        bool skip = false;
        for (uint32_t n = 0; n < RG_SPEC_FRAME; ++n) {
            bool bad;
            const float x = value_at(plane, p.format, (uint64_t)k * RG_SPEC_HOP + n, &bad);
            skip |= bad;
            re[n] = (double)x * (double)tb.window[n];
            im[n] = 0.0;
        }
        if (skip) {
            ++out->skipped;
            continue;
        }
        ++out->analysed;
        fft_double(re.data(), im.data());
        for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j)
            for (uint32_t b = 8 * j + 1; b <= 8 * j + 8; ++b) out->E[j] += re[b] * re[b] + im[b] * im[b];
    }
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
// one block of the tile kernel: frames f0 .. f0 + nf - 1 of the plane, two at a time
template <int FMT>
static void tile_host(const unsigned char *plane, uint32_t f0, uint32_t nf, double *rec, uint32_t *skipped) {
    const RgSpecTables &tb = rg_spec_tables();
    std::vector<RgSpecC> x(RG_SPEC_FRAME), z(RG_SPEC_FRAME);
    for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j) rec[j] = 0.0;
    *skipped = 0;
    for (uint32_t pr = 0; pr < nf; pr += 2) {
        const bool has_b = pr + 1 < nf;
        const uint64_t base = (uint64_t)(f0 + pr) * RG_SPEC_HOP;
        bool bad_a = false, bad_b = false;
        for (uint32_t n = 0; n < RG_SPEC_FRAME; ++n) {
            bad_a |= rg_spec_nonfinite<FMT>(rg_pcm_raw_at(plane, FMT, base + n));
            if (has_b) bad_b |= rg_spec_nonfinite<FMT>(rg_pcm_raw_at(plane, FMT, base + RG_SPEC_HOP + n));
        }
        const bool use_a = !bad_a, use_b = has_b && !bad_b;
        RgSpecC v[16];
        for (uint32_t t = 0; t < RG_SPEC_BLOCK; ++t) {  // pass 1: lane t = 16 n1 + n0
            for (uint32_t n2 = 0; n2 < 16; ++n2) {
                const uint32_t n = 256 * n2 + t;
                const float w = tb.window[n];
                v[n2].x = use_a ? rg_spec_value<FMT>(rg_pcm_raw_at(plane, FMT, base + n)) * w : 0.0f;
                v[n2].y = use_b ? rg_spec_value<FMT>(rg_pcm_raw_at(plane, FMT, base + RG_SPEC_HOP + n)) * w : 0.0f;
            }
            rg_spec_pass1(v, t, tb.tw1);
            for (uint32_t k0 = 0; k0 < 16; ++k0) x[k0 * 256 + t] = v[k0];
        }
        for (uint32_t t = 0; t < RG_SPEC_BLOCK; ++t) {  // pass 2: lane t = 16 k0 + n0, in place
            const uint32_t k0 = t >> 4, n0 = t & 15u;
            for (uint32_t n1 = 0; n1 < 16; ++n1) v[n1] = x[k0 * 256 + n1 * 16 + n0];
            rg_spec_pass2(v, n0, tb.tw2);
            for (uint32_t k1 = 0; k1 < 16; ++k1) x[k0 * 256 + k1 * 16 + n0] = v[k1];
        }
        for (uint32_t t = 0; t < RG_SPEC_BLOCK; ++t) {  // pass 3: lane t = 16 k1 + k0
            const uint32_t k1 = t >> 4, k0 = t & 15u;
            for (uint32_t n0 = 0; n0 < 16; ++n0) v[n0] = x[k0 * 256 + k1 * 16 + n0];
            rg_spec_dft16(v);
            for (uint32_t k2 = 0; k2 < 16; ++k2) z[t + 256 * k2] = v[k2];
        }
        for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j) {  // lane j: band j of both frames, in frame order
            float sa, sb;
            rg_spec_band([&](uint32_t k) { return z[k]; }, j, &sa, &sb);
            if (use_a) rec[j] += (double)sa;
            if (use_b) rec[j] += (double)sb;
        }
        *skipped += (bad_a ? 1u : 0u) + (has_b && bad_b ? 1u : 0u);
    }
}

void rg_spec_folded_host(const unsigned char *arena, const RgSpecPlane &p, RgSpecPlaneOut *out) {
    const unsigned char *plane = arena + p.off;
    memset(out, 0, sizeof *out);
    double rec[RG_SPEC_BANDS];
    for (uint32_t t = 0; t < p.n_tiles; ++t) {  // the tile kernel, one block each; then the fold kernel's sum in tile order
        const uint32_t f0 = t * RG_SPEC_TILE_FRAMES, nf = p.frames - f0 < RG_SPEC_TILE_FRAMES ? p.frames - f0 : RG_SPEC_TILE_FRAMES;
        uint32_t skipped;
        switch (p.format) {
            case RG_FMT_F32_PLANAR: tile_host<RG_FMT_F32_PLANAR>(plane, f0, nf, rec, &skipped); break;
            case RG_FMT_S16_PLANAR: tile_host<RG_FMT_S16_PLANAR>(plane, f0, nf, rec, &skipped); break;
            default: tile_host<RG_FMT_S32_PLANAR>(plane, f0, nf, rec, &skipped); break;
        }
        for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j) out->E[j] += rec[j];
        out->skipped += skipped;
    }
    out->analysed = p.frames - out->skipped;
}

// ---- the verdict -------------------------------------------------------------------------------------------------------------
static void verdict(const double *p, uint32_t analysed, uint32_t sample_rate, const rg_spectrum_opts &o, rg_spectrum_channel *out) {
    const int w = 8, B = (int)RG_SPEC_BANDS;
    memset(out, 0, sizeof *out);
    out->analysed_frames = analysed;
    double top = 0.0;
    for (int j = 0; j < B; ++j) top = p[j] > top ? p[j] : top;
    if (!analysed || !(top > 0.0)) return;
    const double fs = (double)sample_rate, floor_p = top * 1e-12, ratio = std::pow(10.0, -o.edge_db / 10.0);
    // tail[j] = max(p[j .. 255])
    double tail[RG_SPEC_BANDS + 1];
    tail[B] = 0.0;
    for (int j = B - 1; j >= 0; --j) tail[j] = p[j] > tail[j + 1] ? p[j] : tail[j + 1];
    int best = -1;
    double best_d = 0.0;
    for (int j = w - 1; j <= B - 1 - w; ++j) {
        const double f_hi = (8.0 * j + 8.5) * fs / RG_SPEC_FRAME;
        if (!(f_hi >= o.min_cutoff_hz)) continue;
        double below = 0.0, above = 0.0;
        for (int i = j - w + 1; i <= j; ++i) below += p[i];
        for (int i = j + 1; i <= j + w; ++i) above += p[i];
        below /= w;
        above /= w;
        above = above > floor_p ? above : floor_p;
        const double d = 10.0 * std::log10(below / above);
        const double back = tail[j + 1] > floor_p ? tail[j + 1] : floor_p;
        if (!(d >= o.edge_db) || !(back <= below * ratio)) continue;
        if (best < 0 || d > best_d) {
            best = j;
            best_d = d;
        }
    }
    if (best < 0) {
        out->cutoff_hz = fs / 2.0;
        return;
    }
    out->cutoff_hz = (8.0 * best + 8.5) * fs / RG_SPEC_FRAME;
    out->edge_db = best_d;
    out->flags = RG_SPEC_BANDLIMITED;
    if (sample_rate >= RG_SPEC_UPSAMPLED_MIN_RATE && out->cutoff_hz <= RG_SPEC_UPSAMPLED_MAX_CUTOFF_HZ) out->flags |= RG_SPEC_UPSAMPLED;
}

static thread_local char g_spec_err[256];

extern "C" int rg_spectrum_verdict(const double *p, uint32_t analysed_frames, uint32_t sample_rate, const rg_spectrum_opts *opts,
                                   rg_spectrum_channel *out) {
    rg_spectrum_opts o;
    if (!p || !out || !sample_rate) return RG_ERR_INVALID_ARG;
    if (rg_spec_options(opts, &o, g_spec_err, sizeof g_spec_err) != RG_OK) return RG_ERR_INVALID_ARG;
    verdict(p, analysed_frames, sample_rate, o, out);
    return RG_OK;
}

void rg_spec_fill(const rg_track_desc &t, uint32_t dropped_frames, const RgSpecPlaneOut *planes, const rg_spectrum_opts &o, rg_spectrum_result *out,
                  double *bands) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->dropped_frames = dropped_frames;
    uint32_t flags = dropped_frames == 0 ? RG_SPEC_COMPLETE : 0u;
    if (rg_spec_frames(t.frames) == 0) flags |= RG_SPEC_SHORT;
    if (bands) memset(bands, 0, sizeof(double) * RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS);
    for (uint32_t c = 0; c < t.channels; ++c) {
        const RgSpecPlaneOut &po = planes[c];
        double p[RG_SPEC_BANDS];
        for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j) p[j] = po.analysed ? po.E[j] / (8.0 * po.analysed) : 0.0;
        if (t.sample_rate) verdict(p, po.analysed, t.sample_rate, o, &out->ch[c]);
        out->ch[c].analysed_frames = po.analysed;
        out->ch[c].skipped_frames = po.skipped;
        flags |= out->ch[c].flags;
        if (po.skipped) flags |= RG_SPEC_NONFINITE;
        if (out->ch[c].cutoff_hz > out->cutoff_hz) out->cutoff_hz = out->ch[c].cutoff_hz;
        if (bands) memcpy(bands + (size_t)c * RG_SPEC_BANDS, po.E, sizeof po.E);
    }
    out->flags = flags;
}

int rg_spec_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_spectrum_opts *opts, const void *arena, size_t arena_bytes,
                       rg_spectrum_result *out, double *bands_out, char *err, size_t err_len) {
    rg_spectrum_opts o;
    int rc = rg_pcm_check_host_route("rg_spectrum_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_spec_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgSpecPlane> planes(n * RG_SPEC_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    for (size_t i = 0; i < n; ++i) {
        rc = rg_spec_track_planes(i, descs[i], arena_bytes, &planes[n_planes], err, err_len);
        if (rc != RG_OK) return rc;
        n_planes += descs[i].channels;
    }
    uint64_t fmt_tile[4];
    (void)rg_spec_plan(planes.data(), n_planes, fmt_tile);
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    std::vector<RgSpecPlaneOut> po(RG_SPEC_MAX_CHANNELS);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        for (uint32_t c = 0; c < descs[i].channels; ++c) {
            if (route == 0)
                rg_spec_serial_host(base, planes[at + c], &po[c]);
            else
                rg_spec_folded_host(base, planes[at + c], &po[c]);
        }
        rg_spec_fill(descs[i], 0, po.data(), o, &out[i], bands_out ? bands_out + i * RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS : nullptr);
        at += descs[i].channels;
    }
    return RG_OK;
}

extern "C" int rg_spectrum_kernel_shape(uint32_t *frame, uint32_t *hop, uint32_t *bands, uint32_t *frames_per_tile) {
    if (frame) *frame = RG_SPEC_FRAME;
    if (hop) *hop = RG_SPEC_HOP;
    if (bands) *bands = RG_SPEC_BANDS;
    if (frames_per_tile) *frames_per_tile = RG_SPEC_TILE_FRAMES;
    return RG_OK;
}
