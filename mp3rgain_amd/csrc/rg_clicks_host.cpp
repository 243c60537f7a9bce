// rg_clicks_host.cpp -- the host side of the click scan (include/mp3rgain_amd_clicks.h, rg_clicks.h): the options, the plane
// records and their checks, the serial host twin (route 0: the definitions, written plainly, a plane at a time), the kernels'
// tile and fold code walked by one host lane (route 2), and the finish every route shares (the channel records, the flags, the
// merge of the planes' event lists).  Plain C++: no device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "rg_clicks.h"

int rg_ck_options(const rg_clicks_opts *opts, rg_clicks_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts
                : rg_clicks_opts{RG_CK_DEFAULT_BLOCK,     RG_CK_DEFAULT_ORDER,     RG_CK_DEFAULT_RATIO_PERMILLE, RG_CK_DEFAULT_FLOOR, RG_CK_DEFAULT_GAP,
                                 RG_CK_DEFAULT_MAX_WIDTH, RG_CK_DEFAULT_MAX_EVENTS};
    if (!rg_fe_block_ok(out->block_samples)) {
        snprintf(err, err_len, "clicks: block_samples %u is not 256, 512, 1024, 2048 or 4096", out->block_samples);
        return RG_ERR_INVALID_ARG;
    }
    if (out->order < 2 || out->order > RG_CK_MAX_ORDER || (out->order & 1u)) {
        snprintf(err, err_len, "clicks: order %u is not an even number in 2 .. %u", out->order, RG_CK_MAX_ORDER);
        return RG_ERR_INVALID_ARG;
    }
    const struct {
        const char *name;
        uint32_t v, lo, hi;
    } r[5] = {{"ratio_permille", out->ratio_permille, 1000u, 1000000u},
              {"floor", out->floor, 1u, 32767u},
              {"gap", out->gap, 1u, 255u},
              {"max_width", out->max_width, 1u, 4095u},
              {"max_events", out->max_events, 0u, RG_CK_MAX_EVENTS}};
    for (const auto &t : r)
        if (t.v < t.lo || t.v > t.hi) {
            snprintf(err, err_len, "clicks: %s %u is not in %u .. %u", t.name, t.v, t.lo, t.hi);
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

int rg_ck_track_planes(size_t i, const rg_track_desc &t, const rg_clicks_opts &o, size_t arena_bytes, RgCkPlane *out, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_CK_MAX_CHANNELS, "the click scan takes", err, err_len);
    if (rc != RG_OK) return rc;
    rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    const uint32_t tb = rg_ck_tile_blocks(o.block_samples);
    for (uint32_t c = 0; c < t.channels; ++c) {
        RgCkPlane &p = out[c];
        memset(&p, 0, sizeof p);
        p.off = rg_pcm_plane_off(t, c);
        p.n = (uint32_t)t.frames;
        p.n_blocks = (uint32_t)((t.frames + o.block_samples - 1) / o.block_samples);
        p.n_tiles = (p.n_blocks + tb - 1) / tb;
        p.format = t.format;
    }
    return RG_OK;
}

uint64_t rg_ck_plan(RgCkPlane *planes, size_t n) {
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        planes[i].first_tile = tiles;
        tiles += planes[i].n_tiles;
    }
    return tiles;
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
RgCkTile rg_ck_serial_host(const unsigned char *arena, const RgCkPlane &pl, const rg_clicks_opts &o, RgCkEv *ev) {
    RgCkTile out = rg_ck_empty_tile();
    for (uint32_t k = 0; k < o.max_events; ++k) ev[k] = RgCkEv{0u, 0u, 0u, 0u};
    const uint64_t N = pl.n, B = o.block_samples;
    const uint32_t P = o.order;
    if (!N) return out;
    // q, with RG_CK_HIST zeros in front so that every sample has somewhere to look back to
    std::vector<int16_t> qbuf(RG_CK_HIST + N, 0);
    int16_t *q = qbuf.data() + RG_CK_HIST;
    for (uint64_t n = 0; n < N; ++n) {
        bool finite;
        q[n] = (int16_t)rg_ck_q_at(arena + pl.off, pl.format, n, &finite);
        out.nonfinite += finite ? 0u : 1u;
        out.nonzero |= q[n] ? 1u : 0u;
    }
    // the model of every block, the residuals under it, their median
    const uint64_t nb = (N + B - 1) / B;
    std::vector<uint32_t> e(N), med(nb), sorted;
    std::vector<int64_t> xw;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t at = b * B, n = std::min(B, N - at);
        int64_t acf[RG_CK_MAX_ORDER + 1] = {0};
        if (n >= 4u * P) {
            xw.assign(n, 0);
            for (uint64_t i = 0; i < n; ++i) xw[i] = rg_ck_windowed(q[at + i], (uint32_t)i, (uint32_t)n);
            for (uint32_t l = 0; l <= P; ++l)
                for (uint64_t i = l; i < n; ++i) acf[l] += xw[i] * xw[i - l];
        }
        RgCkModel m;
        out.fallback += rg_ck_model(acf, (uint32_t)n, P, &m) ? 1u : 0u;
        for (uint64_t i = at; i < at + n; ++i) e[i] = i < m.order ? 0u : rg_ck_abs_res(q + i, m);
        sorted.assign(e.begin() + at, e.begin() + at + n);
        std::sort(sorted.begin(), sorted.end());
        med[b] = sorted[(n - 1) / 2];
        out.median_max = std::max(out.median_max, med[b]);
    }
    // flagged samples, events
    std::vector<RgCkEv> events;
    for (uint64_t n = 0; n < N; ++n) {
        const uint64_t b = n / B;
        uint32_t S = std::max(med[b], o.floor), s;
        if (b > 0) S = std::max(S, med[b - 1]);
        if (b + 1 < nb) S = std::max(S, med[b + 1]);
        if (!rg_ck_flagged(e[n], S, o.ratio_permille, &s)) continue;
        out.sum.flagged += 1u;
        if (!events.empty() && n - events.back().last <= o.gap) {
            RgCkEv &c = events.back();
            c.last = (uint32_t)n;
            if (s > c.strength) {
                c.strength = s;
                c.peak_at = (uint32_t)n;
            }
        } else {
            events.push_back(RgCkEv{(uint32_t)n, (uint32_t)n, s, (uint32_t)n});
        }
    }
    for (size_t k = 0; k < events.size(); ++k) {
        rg_ck_inner_add(&out.sum.in, events[k], o.max_width);  // (sum.n stays 0: every event is counted)
        if (k < o.max_events) ev[k] = events[k];
    }
    return out;
}

// ---- route 2: the kernels' code on one lane ----------------------------------------------------------------------------------
RgCkTile rg_ck_folded_host(const unsigned char *arena, const RgCkPlane &pl, const rg_clicks_opts &o, RgCkEv *ev) {
    for (uint32_t k = 0; k < o.max_events; ++k) ev[k] = RgCkEv{0u, 0u, 0u, 0u};
    RgCkTile out = rg_ck_empty_tile();
    if (!pl.n_tiles) return out;
    std::unique_ptr<RgCkWork> w(new RgCkWork);
    std::unique_ptr<RgCkFoldWork> fw(new RgCkFoldWork);
    RgCkSerial x;
    std::vector<RgCkTile> recs(pl.n_tiles);
    std::vector<uint32_t> tile_first(pl.n_tiles), listed;
    for (uint32_t t = 0; t < pl.n_tiles; ++t) rg_ck_tile(x, *w, arena + pl.off, pl, o, t, &recs[t], nullptr, 0u, nullptr);
    auto emit = [&](uint32_t t) { listed.push_back(t); };
    rg_ck_fold(x, *fw, pl, o, recs.data(), tile_first.data(), &out, emit);
    RgCkEv none{0u, 0u, 0u, 0u};
    for (uint32_t t : listed) rg_ck_tile(x, *w, arena + pl.off, pl, o, t, nullptr, recs.data(), tile_first[t], o.max_events ? ev : &none);
    return out;
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
void rg_ck_fill(const rg_track_desc &t, const rg_clicks_opts &o, uint32_t dropped_frames, const RgCkTile *po, const RgCkEv *ev, rg_clicks_result *out,
                rg_clicks_event *events) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->dropped_frames = dropped_frames;
    out->block_samples = o.block_samples;
    out->order = o.order;
    out->ratio_permille = o.ratio_permille;
    out->floor = o.floor;
    out->gap = o.gap;
    out->max_width = o.max_width;
    out->max_events = o.max_events;
    const uint32_t N = (uint32_t)t.frames, K = o.max_events;
    uint32_t flags = dropped_frames == 0 ? RG_CK_COMPLETE : 0u, nonzero = 0;
    std::vector<rg_clicks_event> all;
    for (uint32_t c = 0; c < t.channels; ++c) {
        const RgCkInner in = rg_ck_close(po[c].sum, o.max_width);
        rg_clicks_channel &ch = out->ch[c];
        ch.flagged = po[c].sum.flagged;
        ch.clicks = in.clicks;
        ch.bursts = in.bursts;
        ch.widest = in.widest;
        ch.first_click = in.first_click == RG_CK_NONE ? N : in.first_click;
        ch.strongest_at = in.strongest_at == RG_CK_NONE ? N : in.strongest_at;
        ch.strongest_permille = in.strongest;
        ch.fallback_blocks = po[c].fallback;
        ch.median_max = po[c].median_max;
        out->nonfinite += po[c].nonfinite;
        out->events += (uint64_t)in.clicks + in.bursts;
        nonzero |= po[c].nonzero;
        if (in.clicks) flags |= RG_CK_CLICKS;
        if (in.bursts) flags |= RG_CK_BURSTS;
        const uint64_t have = std::min<uint64_t>((uint64_t)in.clicks + in.bursts, K);
        for (uint64_t k = 0; k < have; ++k) {
            const RgCkEv &e = ev[(size_t)c * K + k];
            const uint32_t width = e.last - e.start + 1u;
            all.push_back(rg_clicks_event{e.start, width, e.peak_at, e.strength, (uint16_t)c, (uint16_t)(width <= o.max_width ? RG_CK_KIND_CLICK : RG_CK_KIND_BURST)});
        }
    }
    if (!nonzero) flags |= RG_CK_SILENT;
    if (out->nonfinite) flags |= RG_CK_NONFINITE;
    if (out->events > K) flags |= RG_CK_TRUNCATED;
    out->listed = (uint32_t)std::min<uint64_t>(out->events, K);
    out->flags = flags;
    if (!events) return;
    // the file's first K events are among its planes' first K each
    std::sort(all.begin(), all.end(), [](const rg_clicks_event &a, const rg_clicks_event &b) { return a.start != b.start ? a.start < b.start : a.channel < b.channel; });
    if (K) memset(events, 0, K * sizeof *events);
    for (uint32_t k = 0; k < out->listed; ++k) events[k] = all[k];
}

int rg_ck_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_clicks_opts *opts, const void *arena, size_t arena_bytes, rg_clicks_result *out,
                     rg_clicks_event *events, char *err, size_t err_len) {
    rg_clicks_opts o;
    int rc = rg_pcm_check_host_route("rg_clicks_arena", "the kernels' code", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_ck_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgCkPlane> planes(n * RG_CK_MAX_CHANNELS + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_ck_track_planes(i, descs[i], o, arena_bytes, &planes[i * RG_CK_MAX_CHANNELS], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    const uint32_t K = o.max_events;
    std::vector<RgCkEv> ev((size_t)RG_CK_MAX_CHANNELS * K + 1);
    for (size_t i = 0; i < n; ++i) {
        RgCkTile po[RG_CK_MAX_CHANNELS];
        for (uint32_t c = 0; c < descs[i].channels; ++c) {
            const RgCkPlane &pl = planes[i * RG_CK_MAX_CHANNELS + c];
            po[c] = route == 0 ? rg_ck_serial_host(base, pl, o, &ev[(size_t)c * K]) : rg_ck_folded_host(base, pl, o, &ev[(size_t)c * K]);
        }
        rg_ck_fill(descs[i], o, 0, po, ev.data(), &out[i], events ? events + i * K : nullptr);
    }
    return RG_OK;
}

extern "C" int rg_clicks_kernel_shape(uint32_t block_samples, uint32_t *tile_samples, uint32_t *tile_blocks, uint32_t *fold_lanes, uint32_t *lds_bytes) {
    if (!rg_fe_block_ok(block_samples)) return RG_ERR_INVALID_ARG;
    if (tile_samples) *tile_samples = rg_ck_tile_blocks(block_samples) * block_samples;
    if (tile_blocks) *tile_blocks = rg_ck_tile_blocks(block_samples);
    if (fold_lanes) *fold_lanes = RG_CK_FOLD_LANES;
    if (lds_bytes) *lds_bytes = RG_CK_LDS_BYTES;
    return RG_OK;
}
