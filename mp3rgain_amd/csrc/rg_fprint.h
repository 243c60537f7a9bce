// rg_fprint.h -- internal: the duplicate finder (include/mp3rgain_amd_fingerprint.h) as rg_fprint.hip (the fingerprint kernels,
// their launcher and seam), rg_fprint_match.hip (the match kernel and its seam), rg_fprint_host.cpp (the serial twins, the
// kernels' f32 arithmetic on the host, the groups) and rg_file_verify.hip (rg_same_recording) share it.  The transform is the
// spectral scan's (rg_spectrum.h: tables, passes, rg_spec_dft16); what is written once here for both sides is how a band of
// the two frames of a pair is summed and how a code comes from two rows of band energies.  Both translation units are compiled
// without contraction, so the two give the same bits.  The tempo scan (rg_tempo.h) is a second user of the track record, the
// plan, the tile walk (rg_fprint_tile.h on the device, rg_fp_tile_bands_host here) and the double transform of route 0.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mp3rgain_amd_fingerprint.h"
#include "rg_spectrum.h"

#define RG_FP_LANES 256u
#define RG_FP_TILE_CODES 7u    // T: codes of one workgroup
#define RG_FP_TILE_FRAMES 8u   // T + 1 frames, four pairs; the first is the last frame of the tile before
#define RG_FP_STAGE (RG_FP_TILE_CODES * RG_FP_HOP + RG_FP_FRAME)  // down-mixed samples of a tile: 7680 floats, 30 KB
#define RG_FP_MATCH_LANES 256u
#define RG_FP_LAGS_PER_LANE 16u  // ceil((2 * RG_FP_MAX_RADIUS + 1) / 256)

// One track of a launch
struct RgFpTrack {
    uint64_t off0, off1;  // planes of the first two channels from the arena's base, in bytes (off1 unused for one channel)
    uint64_t first_tile;  // of this track among the launch's tiles (the tiles of one format are contiguous)
    uint64_t codes_at;    // where its codes go, in codes
    uint64_t frames_at;   // where its band energies go, in frames
    uint32_t n;           // N
    uint32_t frames;      // F (0 at an unsupported rate)
    uint32_t n_tiles;     // F == 0 ? 0 : max(1, ceil((F - 1) / T))
    uint32_t format;      // rg_sample_format
    uint32_t channels;    // 1 or 2: the planes that count
    uint32_t rate_ok;
    uint32_t e[RG_FP_BANDS + 1];
};  // 200 bytes

// One compared pair of a match launch
struct RgFpPair {
    uint64_t a_at, b_at;  // the probe side's and the other side's codes, in codes
    uint32_t ka, kb;
    uint32_t rec;         // its record
    uint32_t flags;       // RG_FP_PAIR_COMPARED, with RG_FP_PAIR_PROBE_J
};  // 32 bytes

RG_SPEC_HD uint32_t rg_fp_frames(uint64_t n) { return n < RG_FP_FRAME ? 0u : (uint32_t)((n - RG_FP_FRAME) / RG_FP_HOP + 1u); }

// bins b0 .. b1 - 1 of frame `which` (0: the real part, 1: the imaginary part) of the pair whose transform z(k) = Z[k] is,
// 1 <= k <= 4095: the powers summed in f32 in bin order
template <class Z>
RG_SPEC_HD float rg_fp_band(Z z, uint32_t b0, uint32_t b1, uint32_t which) {
    float s = 0.0f;
    for (uint32_t bin = b0; bin < b1; ++bin) {
        const RgSpecC u = z(bin), w = z(RG_SPEC_FRAME - bin);
        const float re = which ? u.y + w.y : u.x + w.x, im = which ? w.x - u.x : u.y - w.y;
        s += (re * re + im * im) * 0.25f;
    }
    return s;
}

// the code of frame n from E[n - 1] (`prev`) and E[n] (`cur`), 33 floats each
RG_SPEC_HD uint32_t rg_fp_code(const float *prev, const float *cur) {
    uint32_t code = 0;
    for (uint32_t m = 0; m < 32; ++m) {
        const float d = (cur[m] - cur[m + 1]) - (prev[m] - prev[m + 1]);
        if (d > 0.0f) code |= 1u << m;
    }
    return code;
}

// is x = (a + b) * 0.5f, or a float sample, a NaN or Inf
RG_SPEC_HD bool rg_fp_nonfinite(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u & 0x7F800000u) == 0x7F800000u;
}

// q(E) of the tempo and key scans (rg_tempo.h, rg_key.h): the bit pattern of max(E, 2^-16), shifted right by 18 (a NaN takes
// the floor); one step is 1/32 of an octave of power
RG_SPEC_HD uint32_t rg_tp_q(float e) {
    const float x = e > 1.52587890625e-5f ? e : 1.52587890625e-5f;
    uint32_t u;
    memcpy(&u, &x, 4);
    return u >> 18;
}

// the best lag so far of a pair; bits == 0: none
struct RgFpBest {
    uint32_t errors, bits;
    int32_t lag;
};
// is x better than y: the smaller errors / bits, then the smaller |d|, then the negative d
RG_SPEC_HD bool rg_fp_better(const RgFpBest &x, const RgFpBest &y) {
    if (!x.bits) return false;
    if (!y.bits) return true;
    const uint64_t l = (uint64_t)x.errors * y.bits, r = (uint64_t)y.errors * x.bits;
    if (l != r) return l < r;
    const int32_t ax = x.lag < 0 ? -x.lag : x.lag, ay = y.lag < 0 ? -y.lag : y.lag;
    if (ax != ay) return ax < ay;
    return x.lag < y.lag;
}
RG_SPEC_HD void rg_fp_close(const RgFpBest &b, uint32_t pair_flags, uint32_t max_ber_permille, rg_fingerprint_pair_record *out) {
    if (!b.bits) {
        *out = rg_fingerprint_pair_record{0u, 0u, 0, RG_FP_PAIR_SKIPPED};
        return;
    }
    const bool match = (uint64_t)b.errors * 1000u <= (uint64_t)b.bits * max_ber_permille;
    *out = rg_fingerprint_pair_record{b.errors, b.bits, b.lag, pair_flags | (match ? RG_FP_PAIR_MATCH : 0u)};
}
// where probe p of `probes` starts in a probe side of ka codes
RG_SPEC_HD uint32_t rg_fp_probe_start(uint32_t p, uint32_t ka, uint32_t block, uint32_t probes) {
    return (uint32_t)((uint64_t)(2u * p + 1u) * (ka - block) / (2u * probes));
}

// ---- what the host twins of the fingerprint and of the tempo scan (rg_tempo.h) walk alike -------------------------------------
// sample k of the track's signal: the channel, or the mean of the first two, in f32
inline float rg_fp_signal_at(const unsigned char *arena, const RgFpTrack &t, uint64_t k) {
    const auto value = [&](uint64_t off) {
        const uint32_t raw = rg_pcm_raw_at(arena + off, t.format, k);
        switch (t.format) {
            case RG_FMT_F32_PLANAR: return rg_spec_value<RG_FMT_F32_PLANAR>(raw);
            case RG_FMT_S16_PLANAR: return rg_spec_value<RG_FMT_S16_PLANAR>(raw);
            default: return rg_spec_value<RG_FMT_S32_PLANAR>(raw);
        }
    };
    const float a = value(t.off0);
    return t.channels >= 2 ? (a + value(t.off1)) * 0.5f : a;
}

// re, im <- their L-point DFT: decimation in time, radix 2, in double (route 0)
inline void rg_fp_fft_double(double *re, double *im) {
    const uint32_t L = RG_FP_FRAME;
    static const std::vector<double> *roots = [] {
        std::vector<double> *r = new std::vector<double>(RG_FP_FRAME);  // cos, -sin of 2 pi k / L, k < L / 2
        for (uint32_t k = 0; k < RG_FP_FRAME / 2; ++k) {
            (*r)[2 * k] = std::cos(2.0 * 3.14159265358979323846 * k / RG_FP_FRAME);
            (*r)[2 * k + 1] = -std::sin(2.0 * 3.14159265358979323846 * k / RG_FP_FRAME);
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

// route 2, one workgroup of a tile kernel (rg_fprint_tile.h): the band energies of the tile's *nf frames, BANDS floats each, to
// E[RG_FP_TILE_FRAMES * BANDS], with t.e[0 .. BANDS] (or `edges`, when given) the edges; -> the non-finite frames among those the tile owns.  The unit
// that instantiates it is compiled without contraction.
template <uint32_t BANDS>
inline uint32_t rg_fp_tile_bands_host(const unsigned char *arena, const RgFpTrack &t, uint32_t tile, float *E, uint32_t *nf_out,
                                      const uint32_t *edges = nullptr) {
    const RgSpecTables &tb = rg_spec_tables();
    const uint32_t *e = edges ? edges : t.e;  // the key scan's 61 edges do not fit the record
    const uint32_t f0 = tile * RG_FP_TILE_CODES, left = t.frames - f0, nf = left < RG_FP_TILE_FRAMES ? left : RG_FP_TILE_FRAMES;
    const uint32_t count = (nf - 1u) * RG_FP_HOP + RG_FP_FRAME;
    std::vector<float> pcm(count);
    for (uint32_t k = 0; k < count; ++k) pcm[k] = rg_fp_signal_at(arena, t, (uint64_t)f0 * RG_FP_HOP + k);
    std::vector<RgSpecC> x(RG_SPEC_FRAME), z(RG_SPEC_FRAME);
    uint32_t nonfinite = 0;
    for (uint32_t pr = 0; pr < nf; pr += 2) {
        const bool has_b = pr + 1 < nf;
        const float *fa = &pcm[pr * RG_FP_HOP], *fb = has_b ? fa + RG_FP_HOP : fa;
        bool bad_a = false, bad_b = false;
        if (t.format == RG_FMT_F32_PLANAR)
            for (uint32_t n = 0; n < RG_FP_FRAME; ++n) {
                bad_a |= rg_fp_nonfinite(fa[n]);
                if (has_b) bad_b |= rg_fp_nonfinite(fb[n]);
            }
        const bool use_a = !bad_a, use_b = has_b && !bad_b;
        RgSpecC v[16];
        for (uint32_t l = 0; l < RG_FP_LANES; ++l) {  // pass 1: lane l = 16 n1 + n0
            for (uint32_t n2 = 0; n2 < 16; ++n2) {
                const uint32_t n = 256 * n2 + l;
                const float w = tb.window[n];
                v[n2].x = use_a ? fa[n] * w : 0.0f;
                v[n2].y = use_b ? fb[n] * w : 0.0f;
            }
            rg_spec_pass1(v, l, tb.tw1);
            for (uint32_t k0 = 0; k0 < 16; ++k0) x[k0 * 256 + l] = v[k0];
        }
        for (uint32_t l = 0; l < RG_FP_LANES; ++l) {  // pass 2: lane l = 16 k0 + n0, in place
            const uint32_t k0 = l >> 4, n0 = l & 15u;
            for (uint32_t n1 = 0; n1 < 16; ++n1) v[n1] = x[k0 * 256 + n1 * 16 + n0];
            rg_spec_pass2(v, n0, tb.tw2);
            for (uint32_t k1 = 0; k1 < 16; ++k1) x[k0 * 256 + k1 * 16 + n0] = v[k1];
        }
        for (uint32_t l = 0; l < RG_FP_LANES; ++l) {  // pass 3: lane l = 16 k1 + k0
            const uint32_t k1 = l >> 4, k0 = l & 15u;
            for (uint32_t n0 = 0; n0 < 16; ++n0) v[n0] = x[k0 * 256 + k1 * 16 + n0];
            rg_spec_dft16(v);
            for (uint32_t k2 = 0; k2 < 16; ++k2) z[l + 256 * k2] = v[k2];
        }
        const auto zat = [&](uint32_t k) { return z[k]; };
        for (uint32_t m = 0; m < BANDS; ++m) {
            E[pr * BANDS + m] = use_a ? rg_fp_band(zat, e[m], e[m + 1], 0) : 0.0f;
            if (has_b) E[(pr + 1) * BANDS + m] = use_b ? rg_fp_band(zat, e[m], e[m + 1], 1) : 0.0f;
        }
        // a tile owns every frame but its first, which is the last of the tile before; tile 0 owns that too
        if (bad_a && (pr || !tile)) ++nonfinite;
        if (has_b && bad_b) ++nonfinite;
    }
    *nf_out = nf;
    return nonfinite;
}

// ---- host side (rg_fprint_host.cpp) ------------------------------------------------------------------------------------------
// the options, checked: NULL or a zero field = the default
int rg_fp_options(const rg_fingerprint_opts *opts, rg_fingerprint_opts *out, char *err, size_t err_len);
// track i's record of a launch, checked against the arena; everything but first_tile, codes_at and frames_at
int rg_fp_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgFpTrack *out, char *err, size_t err_len);
// first_tile of tracks[0 .. n), the tiles of one format contiguous: fmt_tile[f] .. fmt_tile[f + 1]; codes_at and frames_at
// packed in track order from codes_base / frames_base; -> tiles
// (inline: the tempo scan plans its tiles with it too)
inline uint64_t rg_fp_plan(RgFpTrack *tracks, size_t n, uint64_t fmt_tile[4], uint64_t codes_base, uint64_t frames_base) {
    uint64_t tiles = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_tile[f] = tiles;
        for (size_t i = 0; i < n; ++i) {
            if (tracks[i].format != f) continue;
            tracks[i].first_tile = tiles;
            tiles += tracks[i].n_tiles;
        }
    }
    fmt_tile[3] = tiles;
    for (size_t i = 0; i < n; ++i) {
        tracks[i].codes_at = codes_base;
        tracks[i].frames_at = frames_base;
        codes_base += tracks[i].frames ? tracks[i].frames - 1u : 0u;
        frames_base += tracks[i].frames;
    }
    return tiles;
}
// route 0 and route 2 of one track: codes[0 .. K), bands[0 .. 33 F) (either may be NULL), -> non-finite frames
uint32_t rg_fp_serial_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands);
uint32_t rg_fp_folded_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands);
void rg_fp_fill(const rg_track_desc &d, const RgFpTrack &t, uint32_t dropped_frames, uint32_t nonfinite_frames, uint32_t index, rg_fingerprint_result *out);
int rg_fp_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_fingerprint_result *out,
                     uint32_t *codes_out, float *bands_out, char *err, size_t err_len);
// the compared pairs of n tracks (counts, rates, where each track's codes start) at `o`; every record that is not compared is
// filled here (RG_FP_PAIR_SKIPPED)
void rg_fp_pairs(size_t n, const uint32_t *counts, const uint32_t *rates, const uint64_t *at, const rg_fingerprint_opts &o, std::vector<RgFpPair> *pairs,
                 rg_fingerprint_pair_record *records);
// one compared pair on the host
void rg_fp_match_host(const uint32_t *codes, const RgFpPair &p, const rg_fingerprint_opts &o, rg_fingerprint_pair_record *out);
// route 0 of rg_fingerprint_match_codes: the pair list and every compared pair, serially
int rg_fp_match_codes_host(size_t n, const uint32_t *counts, const uint32_t *rates, const uint32_t *codes, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` tracks in the device arena at `d_arena`: the kernels on `s`; codes to d_codes[codes_at ..], band energies to
// d_bands[frames_at * 33 ..] unless NULL, nonfinite[i] <- track i's count; `s` has been synchronised on return
int rg_fprint_device(rg_ctx *c, const unsigned char *d_arena, RgFpTrack *tracks, size_t n, uint32_t *d_codes, float *d_bands, uint32_t *nonfinite,
                     hipStream_t s);
// the compared pairs over the device codes at d_codes: records[p.rec] <- pair p; `s` has been synchronised on return
int rg_fprint_match_device(rg_ctx *c, const uint32_t *d_codes, const std::vector<RgFpPair> &pairs, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records, hipStream_t s);
// the match kernel over `count` pairs at d_pairs, enqueued on `s` (rg_fingerprint_rate times it)
int rg_fprint_match_launch(rg_ctx *c, const uint32_t *d_codes, const RgFpPair *d_pairs, size_t count, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *d_records, hipStream_t s);
#endif
