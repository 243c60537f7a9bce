// rg_ancestry_host.cpp -- the host side of the lossy ancestry scan (include/mp3rgain_amd_ancestry.h, rg_ancestry.h): the
// tables, the options, the views and their checks, how a plane is cut into segments and tiles, the serial host twin (route 0:
// the definitions, alignment by alignment), the kernels' cutting walked by the host (route 2: phases and tiles, the same
// functions as rg_ancestry.hip runs), and the finish every route shares.  Plain C++: no device and no context, so a sanitizer
// build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "rg_ancestry.h"
#include "rg_mp3_tables.h"

static RgAncTables make_tables() {
    RgAncTables t;
    const double pi = 3.14159265358979323846;
    double d[512] = {0.0};
    for (int i = 0; i <= 256; ++i) d[i] = (double)kMp3SynthWindowQ16[i] / 65536.0;
    for (int i = 1; i < 256; ++i) d[512 - i] = (i & 63) ? -d[i] : d[i];
    for (int i = 0; i < 512; ++i) t.c[i] = (float)(d[i] / 32.0);
    for (int k = 0; k < 32; ++k)
        for (int j = 0; j < 64; ++j) t.mt[j][k] = (float)cos((double)((2 * k + 1) * (j - 16)) * pi / 64.0);
    for (int l = 0; l < 18; ++l)
        for (int i = 0; i < 36; ++i)
            t.wt[i][l] = (float)(cos(pi / 72.0 * (double)((2 * i + 19) * (2 * l + 1))) * sin(pi / 36.0 * ((double)i + 0.5)) / 9.0);
    static const double ci[8] = {-0.6, -0.535, -0.33, -0.185, -0.095, -0.041, -0.0142, -0.0037};
    for (int i = 0; i < 8; ++i) {
        t.cs[i] = (float)(1.0 / sqrt(1.0 + ci[i] * ci[i]));
        t.ca[i] = (float)(ci[i] / sqrt(1.0 + ci[i] * ci[i]));
    }
    return t;
}
const RgAncTables &rg_anc_tables() {
    static const RgAncTables t = make_tables();
    return t;
}

int rg_anc_options(const rg_ancestry_opts *opts, rg_ancestry_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_ancestry_opts{RG_ANC_SEGMENTS, RG_ANC_GRANULES, 0.0, 0.0, 0.0f, 0u};
    if (out->segments && !out->granules) {
        snprintf(err, err_len, "ancestry: granules is 0 with %u segment(s)", out->segments);
        return RG_ERR_INVALID_ARG;
    }
    if (out->reserved) {
        snprintf(err, err_len, "ancestry: the reserved option is %u, not 0", out->reserved);
        return RG_ERR_INVALID_ARG;
    }
    if (!(out->z_min >= 0.0) || !std::isfinite(out->z_min) || !(out->iso_min >= 0.0) || !std::isfinite(out->iso_min) || !(out->active_floor >= 0.0f) ||
        !std::isfinite(out->active_floor)) {
        snprintf(err, err_len, "ancestry: z_min %g, iso_min %g and active_floor %g must be finite and not negative", out->z_min, out->iso_min,
                 (double)out->active_floor);
        return RG_ERR_INVALID_ARG;
    }
    if (out->z_min == 0.0) out->z_min = RG_ANC_Z_MIN;
    if (out->iso_min == 0.0) out->iso_min = RG_ANC_ISO_MIN;
    if (out->active_floor == 0.0f) out->active_floor = RG_ANC_ACTIVE_FLOOR;
    return RG_OK;
}

int rg_anc_track_views(size_t i, const rg_track_desc &t, size_t arena_bytes, RgAncView *views, uint32_t *n_views, char *err, size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_ANC_MAX_CHANNELS, "the ancestry scan takes", err, err_len);
    if (rc == RG_OK) rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    uint32_t n = 0;
    for (uint32_t c = 0; c < t.channels; ++c) {
        RgAncView &v = views[n++];
        memset(&v, 0, sizeof v);
        v.off_a = v.off_b = rg_pcm_plane_off(t, c);
        v.n = (uint32_t)t.frames;
        v.format = t.format;
    }
    if (t.channels == 2)
        for (uint32_t m = 1; m <= 2; ++m) {
            RgAncView &v = views[n++];
            v = views[0];
            v.off_b = views[1].off_a;
            v.mix = m;
        }
    *n_views = n;
    return RG_OK;
}

void rg_anc_jobs(uint64_t N, const rg_ancestry_opts &o, uint32_t view, std::vector<RgAncJob> *jobs, uint32_t *S, uint32_t *G) {
    rg_anc_cut(N, o.segments, o.granules, S, G);
    if (!jobs) return;
    for (uint32_t j = 0; j < *S; ++j) {
        const uint64_t a = rg_anc_start(N, *S, *G, j);
        for (uint32_t g0 = 1; g0 <= *G; g0 += RG_ANC_TILE) {
            const uint32_t left = *G - g0 + 1u;
            jobs->push_back(RgAncJob{a, view, g0, left < RG_ANC_TILE ? left : RG_ANC_TILE, 0u});
        }
    }
}

uint64_t rg_anc_count_nonfinite(const unsigned char *arena, const RgAncView &v) {
    if (v.format != RG_FMT_F32_PLANAR || v.mix) return 0;
    uint64_t cnt = 0;
    for (uint32_t k = 0; k < v.n; ++k) cnt += rg_anc_nonfinite(rg_pcm_raw_at(arena + v.off_a, v.format, k)) ? 1u : 0u;
    return cnt;
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
void rg_anc_serial_host(const unsigned char *arena, const RgAncView &v, const rg_ancestry_opts &o, uint64_t *small_, uint64_t *active_, uint64_t *nonfinite) {
    const RgAncTables &t = rg_anc_tables();
    memset(small_, 0, RG_ANC_ALIGNMENTS * sizeof(uint64_t));
    memset(active_, 0, RG_ANC_ALIGNMENTS * sizeof(uint64_t));
    *nonfinite = rg_anc_count_nonfinite(arena, v);
    uint32_t S, G;
    rg_anc_cut(v.n, o.segments, o.granules, &S, &G);
    std::vector<float> sub((size_t)18 * (G + 1) * 32);  // [granule 0 .. G][slot][subband]
    std::vector<float> ys((size_t)576 * (G + 2) + 480);  // y[a - 480 ..): what any alignment of the segment reads
    for (uint32_t j = 0; j < S; ++j) {
        const int64_t a = (int64_t)rg_anc_start(v.n, S, G, j);
        for (size_t n = 0; n < ys.size(); ++n) ys[n] = rg_anc_sample(arena, v, a - 480 + (int64_t)n);
        for (uint32_t r = 0; r < RG_ANC_ALIGNMENTS; ++r) {
            for (uint32_t u = 0; u < 18u * (G + 1u); ++u) {  // slot t of granule g is u = 18 g + t
                const float *newest = &ys[480u + r + 32u * u + 31u];
                float y[64];
                for (uint32_t jj = 0; jj < 64; ++jj) y[jj] = rg_anc_window(t, [&](uint32_t i) { return *(newest - i); }, jj);
                rg_anc_matrix32(t, y, &sub[(size_t)u * 32]);
            }
            for (uint32_t g = 1; g <= G; ++g) {
                float x[576];
                for (uint32_t k = 0; k < 32; ++k)
                    rg_anc_mdct(t, [&](uint32_t i) { return rg_anc_invert(sub[((size_t)18 * (g - 1) + i) * 32 + k], k, i); }, &x[18 * k]);
                uint32_t s, ac;
                rg_anc_granule_counts(t, x, o.active_floor, &s, &ac);
                small_[r] += s;
                active_[r] += ac;
            }
        }
    }
}

// ---- route 2: the kernels' cutting -------------------------------------------------------------------------------------------
void rg_anc_tile_host(const unsigned char *arena, const RgAncView &v, const RgAncJob &job, uint32_t phase, float floor_, uint64_t *small_, uint64_t *active_) {
    const RgAncTables &t = rg_anc_tables();
    const uint32_t nslots = 18u * job.ng + 35u;
    const int64_t x0 = (int64_t)job.a + phase + 32ll * 18 * ((int64_t)job.g0 - 1) - 480;  // the tile's first sample
    std::vector<float> xs((size_t)32 * nslots + 480), sub((size_t)nslots * 32);
    for (size_t n = 0; n < xs.size(); ++n) xs[n] = rg_anc_sample(arena, v, x0 + (int64_t)n);
    for (uint32_t s = 0; s < nslots; ++s) {
        const uint32_t e = 480u + 32u * s + 31u;
        float y[64];
        for (uint32_t j = 0; j < 64; ++j) y[j] = rg_anc_window(t, [&](uint32_t i) { return xs[e - i]; }, j);
        rg_anc_matrix32(t, y, &sub[(size_t)s * 32]);
    }
    for (uint32_t pair = 0; pair < 18u * job.ng; ++pair) {
        const uint32_t q = pair % 18u, gi = pair / 18u, u0 = q + 18u * gi;
        float x[576];
        for (uint32_t k = 0; k < 32; ++k) rg_anc_mdct(t, [&](uint32_t i) { return rg_anc_invert(sub[(size_t)(u0 + i) * 32 + k], k, i); }, &x[18 * k]);
        uint32_t s, ac;
        rg_anc_granule_counts(t, x, floor_, &s, &ac);
        small_[32u * q + phase] += s;
        active_[32u * q + phase] += ac;
    }
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
// a / b > c / d for b, d >= 1
static bool ratio_above(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return (unsigned __int128)a * d > (unsigned __int128)c * b; }

static void finish_view(const uint64_t *sm, const uint64_t *ac, const rg_ancestry_opts &o, rg_ancestry_view *w) {
    int best = -1, second = -1;
    uint64_t ssum = 0, asum = 0;
    for (int r = 0; r < (int)RG_ANC_ALIGNMENTS; ++r) {
        ssum += sm[r];
        asum += ac[r];
        if (ac[r] && (best < 0 || ratio_above(sm[r], ac[r], sm[best], ac[best]))) best = r;
    }
    w->active_total = asum;
    if (best < 0) return;
    for (int r = 0; r < (int)RG_ANC_ALIGNMENTS; ++r)
        if (r != best && ac[r] && (second < 0 || ratio_above(sm[r], ac[r], sm[second], ac[second]))) second = r;
    w->offset = (uint32_t)best;
    w->small = sm[best];
    w->active = ac[best];
    w->ratio = (double)sm[best] / (double)ac[best];
    w->second = second < 0 ? 0.0 : (double)sm[second] / (double)ac[second];
    const uint64_t rest_a = asum - ac[best];
    w->p0 = rest_a ? (double)(ssum - sm[best]) / (double)rest_a : 0.0;
    const double var = w->p0 * (1.0 - w->p0) * (double)ac[best];
    w->z = var > 0.0 ? ((double)sm[best] - w->p0 * (double)ac[best]) / sqrt(var) : 0.0;
    w->iso = w->second > 0.0 ? w->ratio / w->second : (w->ratio > 0.0 ? INFINITY : 0.0);
    w->flagged = w->z >= o.z_min && w->iso >= o.iso_min ? 1u : 0u;
}

void rg_anc_fill(const rg_track_desc &t, const rg_ancestry_opts &o, uint32_t S, uint32_t G, uint32_t dropped_frames, uint32_t n_views, const RgAncView *views,
                 const uint64_t *counts, const uint64_t *nonfinite, rg_ancestry_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->dropped_frames = dropped_frames;
    out->views = n_views;
    out->segments = S;
    out->granules = G;
    out->best_view = RG_ANC_NO_VIEW;
    uint32_t flags = dropped_frames == 0 ? RG_ANC_COMPLETE : 0u;
    bool sounding = false;
    for (uint32_t v = 0; v < n_views; ++v) {
        rg_ancestry_view &w = out->view[v];
        w.kind = views[v].mix == 0 ? v : (views[v].mix == 1 ? RG_ANC_VIEW_MID : RG_ANC_VIEW_SIDE);
        w.nonfinite = (uint32_t)(nonfinite[v] > 0xFFFFFFFFull ? 0xFFFFFFFFull : nonfinite[v]);
        if (w.nonfinite) flags |= RG_ANC_NONFINITE;
        finish_view(counts + (size_t)v * 2 * RG_ANC_ALIGNMENTS, counts + ((size_t)v * 2 + 1) * RG_ANC_ALIGNMENTS, o, &w);
        sounding = sounding || w.active_total > 0;
        if (w.flagged && (out->best_view == RG_ANC_NO_VIEW || w.z > out->z)) {
            out->best_view = v;
            out->z = w.z;
            out->iso = w.iso;
            out->grid_offset = w.offset;
        }
    }
    if (out->best_view != RG_ANC_NO_VIEW) {
        flags |= RG_ANC_MP3_GRID;
        if (views[out->best_view].mix) flags |= RG_ANC_MIDSIDE;
    }
    if (S == 0) flags |= RG_ANC_SHORT;
    if (!sounding) flags |= RG_ANC_SILENT;
    out->flags = flags;
}

int rg_anc_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_ancestry_opts *opts, const void *arena, size_t arena_bytes,
                      rg_ancestry_result *out, uint64_t *counts, char *err, size_t err_len) {
    rg_ancestry_opts o;
    int rc = rg_pcm_check_host_route("rg_ancestry_arena", "the kernels' cutting", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_anc_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgAncView> views(n * RG_ANC_MAX_VIEWS + 1);
    std::vector<uint32_t> nv(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_anc_track_views(i, descs[i], arena_bytes, &views[i * RG_ANC_MAX_VIEWS], &nv[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    const size_t per_view = 2 * RG_ANC_ALIGNMENTS;
    std::vector<uint64_t> cnt(RG_ANC_MAX_VIEWS * per_view);
    for (size_t i = 0; i < n; ++i) {
        std::fill(cnt.begin(), cnt.end(), 0);
        uint64_t nonfinite[RG_ANC_MAX_VIEWS] = {0};
        uint32_t S = 0, G = 0;
        for (uint32_t v = 0; v < nv[i]; ++v) {
            const RgAncView &vw = views[i * RG_ANC_MAX_VIEWS + v];
            uint64_t *sm = &cnt[v * per_view], *ac = sm + RG_ANC_ALIGNMENTS;
            if (route == 0) {
                rg_anc_cut(vw.n, o.segments, o.granules, &S, &G);
                rg_anc_serial_host(base, vw, o, sm, ac, &nonfinite[v]);
            } else {
                std::vector<RgAncJob> jobs;
                rg_anc_jobs(vw.n, o, v, &jobs, &S, &G);
                for (const RgAncJob &job : jobs)
                    for (uint32_t p = 0; p < RG_ANC_PHASES; ++p) rg_anc_tile_host(base, vw, job, p, o.active_floor, sm, ac);
                nonfinite[v] = rg_anc_count_nonfinite(base, vw);
            }
        }
        rg_anc_fill(descs[i], o, S, G, 0, nv[i], &views[i * RG_ANC_MAX_VIEWS], cnt.data(), nonfinite, &out[i]);
        if (counts) memcpy(counts + i * cnt.size(), cnt.data(), cnt.size() * sizeof(uint64_t));
    }
    return RG_OK;
}

// the fused multiply-adds of one workgroup (a phase of a whole tile) over the samples of a view that tile stands for:
// (18 T + 35) slots of 512 + 2048, and 18 T (alignment, granule) pairs of 32 * 648 + 2 * 248 + 576
double rg_anc_fma_per_sample(uint32_t G) {
    double fma = 0.0;
    for (uint32_t g0 = 1; g0 <= G; g0 += RG_ANC_TILE) {
        const uint32_t ng = G - g0 + 1u < RG_ANC_TILE ? G - g0 + 1u : RG_ANC_TILE;
        fma += 32.0 * ((18.0 * ng + 35.0) * 2560.0 + 18.0 * ng * (32.0 * 648.0 + 496.0 + 576.0));
    }
    return G ? fma / (576.0 * G) : 0.0;
}

extern "C" int rg_ancestry_kernel_shape(uint32_t *phases, uint32_t *tile_granules, uint32_t *lanes, uint32_t *lds_bytes) {
    if (phases) *phases = RG_ANC_PHASES;
    if (tile_granules) *tile_granules = RG_ANC_TILE;
    if (lanes) *lanes = RG_ANC_LANES;
    if (lds_bytes) *lds_bytes = (uint32_t)(sizeof(float) * (RG_ANC_TILE_SAMPLES + 32u * RG_ANC_TILE_SLOTS + 4u * 2u * 64u) + 36u * sizeof(uint32_t));
    return RG_OK;
}
