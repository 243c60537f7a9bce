// rg_fprint_host.cpp -- the host side of the duplicate finder (include/mp3rgain_amd_fingerprint.h, rg_fprint.h): the band edges,
// the track records and their checks, the serial host twin of the fingerprint (route 0: the definitions in double, a plain
// radix-2 transform per frame), the kernels' arithmetic walked by the host (route 2: the same passes, pairs and tiles as
// rg_fprint.hip runs, lane by lane), the pair list, the serial match of one pair, and the groups.  Plain C++: no device and no
// context, so a sanitizer build needs nothing else but rg_spectrum_host.cpp for the tables.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rg_fprint.h"

extern "C" int rg_fingerprint_edges(uint32_t sample_rate, uint32_t *edges) {
    if (!edges || !sample_rate) return RG_ERR_INVALID_ARG;
    bool ok = true;
    for (uint32_t m = 0; m <= RG_FP_BANDS; ++m) {
        const double e = std::floor(300.0 * std::pow(2000.0 / 300.0, (double)m / RG_FP_BANDS) * RG_FP_FRAME / (double)sample_rate + 0.5);
        edges[m] = e > 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)e;
        if (m && edges[m] <= edges[m - 1]) ok = false;
    }
    if (edges[0] < 1 || edges[RG_FP_BANDS] > RG_FP_FRAME / 2) ok = false;
    return ok ? RG_OK : RG_ERR_UNSUPPORTED_RATE;
}

int rg_fp_options(const rg_fingerprint_opts *opts, rg_fingerprint_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_fingerprint_opts{0, 0, 0, 0};
    if (!out->block) out->block = RG_FP_BLOCK;
    if (!out->probes) out->probes = RG_FP_PROBES;
    if (!out->radius) out->radius = RG_FP_RADIUS;
    if (!out->max_ber_permille) out->max_ber_permille = RG_FP_MAX_BER_PERMILLE;
    if (out->block <= RG_FP_MAX_BLOCK && out->probes <= RG_FP_MAX_PROBES && out->radius <= RG_FP_MAX_RADIUS && out->max_ber_permille <= 1000) return RG_OK;
    snprintf(err, err_len, "fingerprint: block %u (at most %u), probes %u (at most %u), radius %u (at most %u), max_ber_permille %u (at most 1000)", out->block,
             RG_FP_MAX_BLOCK, out->probes, RG_FP_MAX_PROBES, out->radius, RG_FP_MAX_RADIUS, out->max_ber_permille);
    return RG_ERR_INVALID_ARG;
}

int rg_fp_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgFpTrack *out, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_FP_MAX_CHANNELS, "the fingerprint takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    memset(out, 0, sizeof *out);
    out->off0 = rg_pcm_plane_off(t, 0);
    out->off1 = t.channels >= 2 ? rg_pcm_plane_off(t, 1) : out->off0;
    out->n = (uint32_t)t.frames;
    out->format = t.format;
    out->channels = t.channels >= 2 ? 2u : 1u;
    out->rate_ok = t.sample_rate && rg_fingerprint_edges(t.sample_rate, out->e) == RG_OK ? 1u : 0u;
    out->frames = out->rate_ok ? rg_fp_frames(t.frames) : 0u;
    out->n_tiles = !out->frames ? 0u : std::max(1u, (out->frames - 1u + RG_FP_TILE_CODES - 1u) / RG_FP_TILE_CODES);
    return RG_OK;
}

// ---- route 0: the definitions (the signal and the double transform are rg_fprint.h's, shared with the tempo scan) ---------------
uint32_t rg_fp_serial_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands) {
    const RgSpecTables &tb = rg_spec_tables();
    std::vector<double> re(RG_FP_FRAME), im(RG_FP_FRAME);
    double prev[RG_FP_BANDS] = {0}, cur[RG_FP_BANDS];
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
            for (uint32_t m = 0; m < RG_FP_BANDS; ++m) cur[m] = 0.0;
        } else {
            rg_fp_fft_double(re.data(), im.data());
            for (uint32_t m = 0; m < RG_FP_BANDS; ++m) {
                double s = 0.0;
                for (uint32_t b = t.e[m]; b < t.e[m + 1]; ++b) s += re[b] * re[b] + im[b] * im[b];
                cur[m] = s;
            }
        }
        if (bands)
            for (uint32_t m = 0; m < RG_FP_BANDS; ++m) bands[(size_t)n * RG_FP_BANDS + m] = (float)cur[m];
        if (n && codes) {
            uint32_t code = 0;
            for (uint32_t m = 0; m < 32; ++m)
                if ((cur[m] - cur[m + 1]) - (prev[m] - prev[m + 1]) > 0.0) code |= 1u << m;
            codes[n - 1] = code;
        }
        memcpy(prev, cur, sizeof prev);
    }
    return nonfinite;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
// one workgroup of the tile kernel: tile `tile` of the track; -> the non-finite frames among those the tile owns
static uint32_t tile_host(const unsigned char *arena, const RgFpTrack &t, uint32_t tile, uint32_t *codes, float *bands) {
    float E[RG_FP_TILE_FRAMES * RG_FP_BANDS];
    uint32_t nf = 0;
    const uint32_t f0 = tile * RG_FP_TILE_CODES, nonfinite = rg_fp_tile_bands_host<RG_FP_BANDS>(arena, t, tile, E, &nf);
    for (uint32_t i = 0; i + 1 < nf; ++i)
        if (codes) codes[f0 + i] = rg_fp_code(&E[i * RG_FP_BANDS], &E[(i + 1) * RG_FP_BANDS]);
    if (bands)
        for (uint32_t i = tile ? 1u : 0u; i < nf; ++i) memcpy(bands + (size_t)(f0 + i) * RG_FP_BANDS, &E[i * RG_FP_BANDS], RG_FP_BANDS * sizeof(float));
    return nonfinite;
}

uint32_t rg_fp_folded_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands) {
    uint32_t nonfinite = 0;
    for (uint32_t tile = 0; tile < t.n_tiles; ++tile) nonfinite += tile_host(arena, t, tile, codes, bands);
    return nonfinite;
}

void rg_fp_fill(const rg_track_desc &d, const RgFpTrack &t, uint32_t dropped_frames, uint32_t nonfinite_frames, uint32_t index, rg_fingerprint_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = d.frames;
    out->sample_rate = d.sample_rate;
    out->channels = d.channels;
    out->format = d.format;
    out->dropped_frames = dropped_frames;
    out->fp_frames = t.frames;
    out->codes = t.frames ? t.frames - 1u : 0u;
    out->nonfinite_frames = nonfinite_frames;
    out->group = index;
    out->codes_at = t.codes_at;
    out->frames_at = t.frames_at;
    out->flags = (dropped_frames == 0 ? RG_FP_COMPLETE : 0u) | (!t.rate_ok ? RG_FP_RATE : 0u) | (out->codes == 0 ? RG_FP_SHORT : 0u) |
                 (nonfinite_frames ? RG_FP_NONFINITE : 0u);
}

int rg_fp_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_fingerprint_result *out,
                     uint32_t *codes_out, float *bands_out, char *err, size_t err_len) {
    int rc = rg_pcm_check_host_route("rg_fingerprint_arena", "the kernels' arithmetic", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgFpTrack> tracks(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_fp_track(i, descs[i], arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    uint64_t fmt_tile[4];
    (void)rg_fp_plan(tracks.data(), n, fmt_tile, 0, 0);
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    for (size_t i = 0; i < n; ++i) {
        const RgFpTrack &t = tracks[i];
        uint32_t *codes = codes_out ? codes_out + t.codes_at : nullptr;
        float *bands = bands_out ? bands_out + t.frames_at * RG_FP_BANDS : nullptr;
        const uint32_t nonfinite = route == 0 ? rg_fp_serial_host(base, t, codes, bands) : rg_fp_folded_host(base, t, codes, bands);
        rg_fp_fill(descs[i], t, 0, nonfinite, (uint32_t)i, &out[i]);
    }
    return RG_OK;
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------------
void rg_fp_pairs(size_t n, const uint32_t *counts, const uint32_t *rates, const uint64_t *at, const rg_fingerprint_opts &o, std::vector<RgFpPair> *pairs,
                 rg_fingerprint_pair_record *records) {
    std::vector<unsigned char> ok(n ? n : 1);
    for (size_t i = 0; i < n; ++i) {
        uint32_t e[RG_FP_BANDS + 1];
        ok[i] = counts[i] >= o.block && rates[i] && rg_fingerprint_edges(rates[i], e) == RG_OK;
    }
    pairs->clear();
    size_t rec = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j, ++rec) {
            if (!ok[i] || !ok[j] || rates[i] != rates[j]) {
                records[rec] = rg_fingerprint_pair_record{0u, 0u, 0, RG_FP_PAIR_SKIPPED};
                continue;
            }
            const bool probe_j = counts[j] < counts[i];
            const size_t a = probe_j ? j : i, b = probe_j ? i : j;
            pairs->push_back(RgFpPair{at[a], at[b], counts[a], counts[b], (uint32_t)rec, RG_FP_PAIR_COMPARED | (probe_j ? RG_FP_PAIR_PROBE_J : 0u)});
        }
}

void rg_fp_match_host(const uint32_t *codes, const RgFpPair &p, const rg_fingerprint_opts &o, rg_fingerprint_pair_record *out) {
    const uint32_t *A = codes + p.a_at, *B = codes + p.b_at;
    const uint32_t need = (o.probes + 1u) / 2u;
    RgFpBest best{0u, 0u, 0};
    for (int64_t d = -(int64_t)o.radius; d <= (int64_t)o.radius; ++d) {
        uint32_t errors = 0, counting = 0;
        for (uint32_t pr = 0; pr < o.probes; ++pr) {
            const int64_t s = rg_fp_probe_start(pr, p.ka, o.block, o.probes), start = s + d;
            if (start < 0 || start + o.block > p.kb) continue;
            for (uint32_t i = 0; i < o.block; ++i) errors += (uint32_t)__builtin_popcount(A[s + i] ^ B[start + i]);
            ++counting;
        }
        if (counting < need) continue;
        const RgFpBest cand{errors, counting * o.block * 32u, (int32_t)d};
        if (rg_fp_better(cand, best)) best = cand;
    }
    rg_fp_close(best, p.flags, o.max_ber_permille, out);
}

extern "C" size_t rg_fingerprint_groups(size_t n, const rg_fingerprint_pair_record *pair_records, uint32_t *groups, uint32_t *matches) {
    std::vector<uint32_t> parent(n ? n : 1);
    for (size_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
    const auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    if (matches)
        for (size_t i = 0; i < n; ++i) matches[i] = 0;
    size_t rec = 0, found = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j, ++rec) {
            if (!pair_records || !(pair_records[rec].flags & RG_FP_PAIR_MATCH)) continue;
            ++found;
            if (matches) {
                ++matches[i];
                ++matches[j];
            }
            const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);  // the root of a component is its smallest index
        }
    if (groups)
        for (size_t i = 0; i < n; ++i) groups[i] = find((uint32_t)i);
    return found;
}

// route 0 of rg_fingerprint_match_codes; rg_fprint_match.hip calls it
int rg_fp_match_codes_host(size_t n, const uint32_t *counts, const uint32_t *rates, const uint32_t *codes, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records) {
    std::vector<uint64_t> at(n + 1, 0);
    for (size_t i = 0; i < n; ++i) at[i + 1] = at[i] + counts[i];
    std::vector<RgFpPair> pairs;
    rg_fp_pairs(n, counts, rates, at.data(), o, &pairs, records);
    for (const RgFpPair &p : pairs) rg_fp_match_host(codes, p, o, &records[p.rec]);
    return RG_OK;
}

extern "C" int rg_fingerprint_kernel_shape(uint32_t *tile_codes, uint32_t *lanes, uint32_t *lds_bytes, uint32_t *match_lanes, uint32_t *lags_per_lane) {
    if (tile_codes) *tile_codes = RG_FP_TILE_CODES;
    if (lanes) *lanes = RG_FP_LANES;
    if (lds_bytes) *lds_bytes = (uint32_t)(16u * 306u * sizeof(RgSpecC) + RG_FP_STAGE * sizeof(float) + (RG_FP_TILE_FRAMES * RG_FP_BANDS + RG_FP_BANDS + 1u) * 4u);
    if (match_lanes) *match_lanes = RG_FP_MATCH_LANES;
    if (lags_per_lane) *lags_per_lane = RG_FP_LAGS_PER_LANE;
    return RG_OK;
}
