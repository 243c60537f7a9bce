// rg_stats_host.cpp -- the host side of the PCM defect scan (include/mp3rgain_amd_stats.h, rg_stats.h): the plane records and
// their checks, the serial host twin (route 0: the definitions, written plainly and without the part records), and the kernels'
// chunking and fold arithmetic walked by the host (route 2: the same chunk, combine and finish functions as rg_stats.hip runs,
// lane by lane).  Plain C++: no device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "rg_stats.h"

int rg_stats_options(const rg_pcm_stats_opts *opts, rg_pcm_stats_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_pcm_stats_opts{RG_STATS_MIN_CLIP_RUN, RG_STATS_MIN_ZERO_RUN};
    if (out->min_clip_run && out->min_zero_run) return RG_OK;
    snprintf(err, err_len, "pcm stats: min_clip_run %u and min_zero_run %u must both be at least 1", out->min_clip_run, out->min_zero_run);
    return RG_ERR_INVALID_ARG;
}

int rg_stats_track_planes(size_t i, const rg_track_desc &t, uint32_t bits, size_t arena_bytes, RgStatsPlane *planes, uint32_t *bits_out, char *err,
                          size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_STATS_MAX_CHANNELS, "pcm stats take", err, err_len);
    if (rc != RG_OK) return rc;
    const uint32_t w = rg_pcm_width(t.format);
    const bool is_float = t.format == RG_FMT_F32_PLANAR;
    if (!is_float && (bits < 1 || bits > w)) {
        snprintf(err, err_len, "track %zu: %u bits in a %u-bit container", i, bits, w);
        return RG_ERR_INVALID_ARG;
    }
    rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    for (uint32_t c = 0; c < t.channels; ++c) {
        RgStatsPlane &p = planes[c];
        memset(&p, 0, sizeof p);
        p.off = rg_pcm_plane_off(t, c);
        p.n = (uint32_t)t.frames;
        p.run = 1;
        p.format = t.format;
        p.bits = is_float ? w : bits;
        p.P = is_float ? 0 : rg_stats_full_scale(t.format, bits);
        p.M = is_float ? 0 : rg_stats_minus_full_scale(t.format);
    }
    *bits_out = is_float ? 0u : bits;
    return RG_OK;
}

uint64_t rg_stats_plan(RgStatsPlane *planes, size_t n, uint64_t fmt_tile[4]) {
    uint64_t tiles = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_tile[f] = tiles;
        for (size_t i = 0; i < n; ++i) {
            RgStatsPlane &p = planes[i];
            if (p.format != f) continue;
            p.first_tile = tiles;
            p.n_tiles = (uint32_t)(((uint64_t)p.n + RG_STATS_TILE - 1) / RG_STATS_TILE);
            p.run = p.n_tiles ? (p.n_tiles + RG_STATS_FOLD_LANES - 1) / RG_STATS_FOLD_LANES : 1;
            tiles += p.n_tiles;
        }
    }
    fmt_tile[3] = tiles;
    return tiles;
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
rg_pcm_stats_channel rg_stats_serial_host(const unsigned char *arena, const RgStatsPlane &p, const rg_pcm_stats_opts &o) {
    const unsigned char *plane = arena + p.off;
    const uint64_t N = p.n;
    const bool is_float = p.format == RG_FMT_F32_PLANAR;
    rg_pcm_stats_channel c;
    memset(&c, 0, sizeof c);
    c.first_clip_run = (uint32_t)N;
    bool took = false;
    double mn = 0.0, mx = 0.0;
    int clip_cls = 0;              // the clip stretch sample k - 1 is in, and the zero stretch
    uint64_t clip_len = 0, zero_len = 0;
    const auto clip_ends = [&](uint64_t end) {  // a clip stretch [end - clip_len, end)
        if (!clip_cls) return;
        if (clip_len >= o.min_clip_run) {
            if (c.clip_runs == 0) c.first_clip_run = (uint32_t)(end - clip_len);
            ++c.clip_runs;
        }
        if (clip_len > c.longest_clip_run) c.longest_clip_run = (uint32_t)clip_len;
    };
    const auto zero_ends = [&](uint64_t end) {  // a zero stretch [end - zero_len, end)
        if (!zero_len) return;
        const bool at_start = end == zero_len, at_end = end == N;
        if (at_start) c.lead_zeros = (uint32_t)zero_len;
        if (at_end) c.trail_zeros = (uint32_t)zero_len;
        if (at_start || at_end) return;
        if (zero_len >= o.min_zero_run) ++c.zero_runs;
        if (zero_len > c.longest_zero_run) c.longest_zero_run = (uint32_t)zero_len;
    };
    for (uint64_t k = 0; k < N; ++k) {
        const uint32_t raw = rg_pcm_raw_at(plane, p.format, k);
        int cls = 0;
        bool zero = false;
        if (is_float) {
            float x;
            memcpy(&x, &raw, 4);
            if (!std::isfinite(x)) {
                ++c.nonfinite;
            } else {
                cls = x >= 1.0f ? 1 : (x <= -1.0f ? -1 : 0);
                zero = x == 0.0f;
                const double xd = x, cl = xd < -256.0 ? -256.0 : (xd > 256.0 ? 256.0 : xd);
                c.sum += llrint(cl * 8388608.0);
                if (!took || xd < mn) mn = xd;
                if (!took || xd > mx) mx = xd;
                took = true;
            }
        } else {
            const int32_t v = (int32_t)raw;
            cls = v >= p.P ? 1 : (v <= p.M ? -1 : 0);
            zero = v == 0;
            c.sum += v;
            c.or_mask |= p.format == RG_FMT_S16_PLANAR ? raw & 0xFFFFu : raw;
            if (!took || v < mn) mn = v;
            if (!took || v > mx) mx = v;
            took = true;
        }
        if (cls != clip_cls) {
            clip_ends(k);
            clip_cls = cls;
            clip_len = 0;
        }
        if (cls) {
            ++clip_len;
            ++c.clipped;
        }
        if (zero) {
            ++zero_len;
            ++c.zeros;
        } else {
            zero_ends(k);
            zero_len = 0;
        }
    }
    clip_ends(N);
    zero_ends(N);
    c.min = mn + 0.0;  // (-0.0 + 0.0 is +0.0)
    c.max = mx + 0.0;
    if (c.or_mask) {
        uint32_t low = 0;
        while (!((c.or_mask >> low) & 1u)) ++low;
        c.effective_bits = rg_pcm_width(p.format) - low;
    }
    return c;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
// v[0] <- the fold of v[0 .. 2^levels) in order: the tree both kernels run over LDS
static void tree(RgStatsPart *v, uint32_t levels, const rg_pcm_stats_opts &o) {
    for (uint32_t j = 0; j < levels; ++j) {
        const uint32_t s = 1u << j;
        for (uint32_t at = 0; at < (1u << levels); at += 2 * s) rg_stats_combine(&v[at], v[at + s], o.min_clip_run, o.min_zero_run);
    }
}

template <int FMT, bool ANY>
static void tile_parts(const unsigned char *plane, const RgStatsPlane &p, const rg_pcm_stats_opts &o, uint32_t wstart, uint32_t wlen, RgStatsPart *v) {
    for (uint32_t lane = 0; lane < RG_STATS_BLOCK; ++lane) {
        uint32_t a;
        const uint32_t n = rg_stats_lane_chunk(wlen, lane, &a);
        const uint64_t k0 = (uint64_t)wstart + a;
        rg_stats_chunk<FMT, ANY>([&](uint32_t j) { return rg_pcm_raw_at(plane, FMT, k0 + j); }, n, p.P, p.M, o.min_clip_run, o.min_zero_run, &v[lane]);
    }
}

rg_pcm_stats_channel rg_stats_folded_host(const unsigned char *arena, const RgStatsPlane &p, const rg_pcm_stats_opts &o, bool any_test) {
    const unsigned char *plane = arena + p.off;
    std::vector<RgStatsPart> tiles(p.n_tiles ? p.n_tiles : 1), v(RG_STATS_BLOCK);
    for (uint32_t t = 0; t < p.n_tiles; ++t) {  // the tile kernel: one block each
        uint32_t wstart;
        const uint32_t wlen = rg_stats_tile_window(p.n, t, &wstart);
        switch (p.format * 2 + (any_test ? 1 : 0)) {
            case RG_FMT_F32_PLANAR * 2: tile_parts<RG_FMT_F32_PLANAR, false>(plane, p, o, wstart, wlen, v.data()); break;
            case RG_FMT_F32_PLANAR * 2 + 1: tile_parts<RG_FMT_F32_PLANAR, true>(plane, p, o, wstart, wlen, v.data()); break;
            case RG_FMT_S16_PLANAR * 2: tile_parts<RG_FMT_S16_PLANAR, false>(plane, p, o, wstart, wlen, v.data()); break;
            case RG_FMT_S16_PLANAR * 2 + 1: tile_parts<RG_FMT_S16_PLANAR, true>(plane, p, o, wstart, wlen, v.data()); break;
            case RG_FMT_S32_PLANAR * 2: tile_parts<RG_FMT_S32_PLANAR, false>(plane, p, o, wstart, wlen, v.data()); break;
            default: tile_parts<RG_FMT_S32_PLANAR, true>(plane, p, o, wstart, wlen, v.data()); break;
        }
        tree(v.data(), RG_STATS_LEVELS, o);
        tiles[t] = v[0];
    }
    // the fold kernel: one block per plane
    for (uint32_t lane = 0; lane < RG_STATS_FOLD_LANES; ++lane) {
        uint32_t lo;
        const uint32_t hi = rg_stats_lane_run(p.n_tiles, p.run, lane, &lo);
        RgStatsPart acc = rg_stats_empty();
        for (uint32_t t = lo; t < hi; ++t) rg_stats_combine(&acc, tiles[t], o.min_clip_run, o.min_zero_run);
        v[lane] = acc;
    }
    tree(v.data(), RG_STATS_FOLD_LEVELS, o);
    return rg_stats_finish(v[0], p.format, o.min_clip_run);
}

void rg_stats_fill(const rg_track_desc &t, uint32_t bits_reported, uint32_t dropped_frames, const rg_pcm_stats_channel *ch, rg_pcm_stats_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->bits = bits_reported;
    out->dropped_frames = dropped_frames;
    uint32_t lead = (uint32_t)t.frames, trail = (uint32_t)t.frames, eff = 0, any_mask = 0;
    uint64_t zeros = 0;
    uint32_t flags = dropped_frames == 0 ? RG_STATS_COMPLETE : 0u;
    for (uint32_t c = 0; c < t.channels; ++c) {
        out->ch[c] = ch[c];
        lead = ch[c].lead_zeros < lead ? ch[c].lead_zeros : lead;
        trail = ch[c].trail_zeros < trail ? ch[c].trail_zeros : trail;
        eff = ch[c].effective_bits > eff ? ch[c].effective_bits : eff;
        any_mask |= ch[c].or_mask;
        zeros += ch[c].zeros;
        if (ch[c].clip_runs) flags |= RG_STATS_CLIPPED;
        if (ch[c].zero_runs) flags |= RG_STATS_DROPOUT;
        if (ch[c].nonfinite) flags |= RG_STATS_NONFINITE;
    }
    if (t.format != RG_FMT_F32_PLANAR && any_mask && eff < bits_reported) flags |= RG_STATS_PADDED;
    if (zeros == t.frames * t.channels) flags |= RG_STATS_SILENT;
    out->lead_silence_frames = lead;
    out->trail_silence_frames = trail;
    out->flags = flags;
}

int rg_stats_arena_host(int route, size_t n, const rg_track_desc *descs, const uint32_t *bits, const rg_pcm_stats_opts *opts, const void *arena,
                        size_t arena_bytes, rg_pcm_stats_result *out, char *err, size_t err_len) {
    rg_pcm_stats_opts o;
    int rc = rg_pcm_check_host_route("rg_pcm_stats_arena", "folded", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_stats_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgStatsPlane> planes(n * RG_STATS_MAX_CHANNELS + 1);
    std::vector<uint32_t> reported(n ? n : 1);
    size_t n_planes = 0;
    for (size_t i = 0; i < n; ++i) {
        rc = rg_stats_track_planes(i, descs[i], bits ? bits[i] : rg_pcm_width(descs[i].format), arena_bytes, &planes[n_planes], &reported[i], err, err_len);
        if (rc != RG_OK) return rc;
        n_planes += descs[i].channels;
    }
    uint64_t fmt_tile[4];
    if (route == 2) (void)rg_stats_plan(planes.data(), n_planes, fmt_tile);
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        rg_pcm_stats_channel ch[RG_STATS_MAX_CHANNELS];
        for (uint32_t c = 0; c < descs[i].channels; ++c)
            ch[c] = route == 0 ? rg_stats_serial_host(base, planes[at + c], o) : rg_stats_folded_host(base, planes[at + c], o, RG_STATS_ANY_TEST != 0);
        rg_stats_fill(descs[i], reported[i], 0, ch, &out[i]);
        at += descs[i].channels;
    }
    return RG_OK;
}

extern "C" int rg_pcm_stats_kernel_shape(uint32_t *chunk_samples, uint32_t *tile_samples, uint32_t *fold_lanes) {
    if (chunk_samples) *chunk_samples = RG_STATS_CHUNK;
    if (tile_samples) *tile_samples = RG_STATS_TILE;
    if (fold_lanes) *fold_lanes = RG_STATS_FOLD_LANES;
    return RG_OK;
}
