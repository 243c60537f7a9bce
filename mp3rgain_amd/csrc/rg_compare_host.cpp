// rg_compare_host.cpp -- the host side of the null test (include/mp3rgain_amd_compare.h, rg_compare.h): the options, the pair
// records and their checks, the serial host twin (route 0: the definitions, written plainly, one loop per sum), the kernels'
// cutting and fold arithmetic walked by the host (route 2: the same take, combine and block functions as rg_compare.hip runs,
// tiles of strips and lag groups summed in double), and what every route shares: the pick from the lag rows and the finish (the
// square roots and logarithms).  Plain C++: no device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "rg_compare.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

int rg_cmp_options(const rg_compare_opts *opts, rg_compare_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts
                : rg_compare_opts{RG_CMP_ALIGN_FINGERPRINT, RG_CMP_DEFAULT_COARSE_RADIUS, RG_CMP_DEFAULT_RADIUS, RG_CMP_DEFAULT_SEGMENTS,
                                  RG_CMP_DEFAULT_SEGMENT_FRAMES, 0u, RG_CMP_DEFAULT_DRIFT_FRAMES, RG_CMP_DEFAULT_LOCK_PERMILLE, RG_CMP_DEFAULT_REQUANT_MILLILSB2};
    const struct {
        const char *name;
        uint32_t v, lo, hi;
    } range[7] = {{"align", out->align, 0u, RG_CMP_ALIGN_HINT},
                  {"coarse_radius", out->coarse_radius, 1u, RG_CMP_MAX_COARSE_RADIUS},
                  {"radius", out->radius, 0u, RG_CMP_MAX_RADIUS},
                  {"segments", out->segments, 1u, RG_CMP_MAX_SEGMENTS},
                  {"block_frames", out->block_frames, 0u, RG_CMP_MAX_BLOCK_FRAMES},
                  {"lock_permille", out->lock_permille, 1u, 1000u},
                  {"requant_millilsb2", out->requant_millilsb2, 1u, 0x80000000u}};
    for (const auto &r : range)
        if (r.v < r.lo || r.v > r.hi) {
            snprintf(err, err_len, "compare: %s %u is not in %u .. %u", r.name, r.v, r.lo, r.hi);
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

int rg_cmp_plan_pair(size_t i, const rg_track_desc *descs, size_t n, const rg_compare_pair &pair, const rg_compare_opts &o, bool rate_is_format,
                     size_t arena_bytes, RgCmpPair *out, char *err, size_t err_len) {
    memset(out, 0, sizeof *out);
    if (pair.a >= n || pair.b >= n) {
        snprintf(err, err_len, "pair %zu: (%u, %u) is not a pair of the %zu tracks", i, pair.a, pair.b, n);
        return RG_ERR_INVALID_ARG;
    }
    if (pair.a == pair.b) {
        snprintf(err, err_len, "pair %zu: track %u against itself", i, pair.a);
        return RG_ERR_INVALID_ARG;
    }
    if (pair.hint > RG_CMP_MAX_HINT || pair.hint < -RG_CMP_MAX_HINT) {
        snprintf(err, err_len, "pair %zu: a hint of %lld frames is beyond 2^32", i, (long long)pair.hint);
        return RG_ERR_INVALID_ARG;
    }
    const rg_track_desc &ta = descs[pair.a], &tb = descs[pair.b];
    for (const uint32_t k : {pair.a, pair.b}) {
        int rc = rg_pcm_check_format(k, descs[k], RG_CMP_MAX_CHANNELS, "the null test takes", err, err_len);
        if (rc == RG_OK) rc = rg_pcm_check_place(k, descs[k], arena_bytes, err, err_len);
        if (rc != RG_OK) return rc;
    }
    out->off_a = ta.offset_bytes;
    out->off_b = tb.offset_bytes;
    out->h = pair.hint;
    out->na = (uint32_t)ta.frames;
    out->nb = (uint32_t)tb.frames;
    out->fmt_a = ta.format;
    out->fmt_b = tb.format;
    out->sigma = 1;
    if (ta.channels != tb.channels) out->flags |= RG_CMP_CHANNELS_DIFFER;
    if (ta.sample_rate != tb.sample_rate) {
        out->flags |= RG_CMP_RATE;
        return RG_OK;
    }
    const uint64_t block = o.block_frames ? o.block_frames : (uint64_t)ta.sample_rate;
    if (block < 1 || block > RG_CMP_MAX_BLOCK_FRAMES) {
        snprintf(err, err_len, "pair %zu: a block of %llu frames (sample rate %u) is not in 1 .. %u", i, (unsigned long long)block, ta.sample_rate,
                 RG_CMP_MAX_BLOCK_FRAMES);
        return rate_is_format && !o.block_frames ? RG_ERR_FORMAT : RG_ERR_INVALID_ARG;
    }
    out->block = (uint32_t)block;
    const uint32_t cc = ta.channels < tb.channels ? ta.channels : tb.channels;
    const uint64_t shorter = ta.frames < tb.frames ? ta.frames : tb.frames;
    if (cc * shorter >= ((uint64_t)1 << 32)) {
        snprintf(err, err_len, "pair %zu: %u channels of %llu frames, the null test takes fewer than 2^32 samples", i, cc, (unsigned long long)shorter);
        return RG_ERR_FORMAT;
    }
    const int64_t h = pair.hint, n0 = h < 0 ? -h : 0, n1 = (int64_t)tb.frames - h < (int64_t)ta.frames ? (int64_t)tb.frames - h : (int64_t)ta.frames;
    if (n1 <= n0) {
        out->flags |= RG_CMP_NO_OVERLAP;
        return RG_OK;
    }
    out->cc = cc;
    out->n0 = (uint32_t)n0;
    out->v = (uint32_t)(n1 - n0);
    const bool whole = o.segment_frames == 0 || (uint64_t)out->v <= (uint64_t)o.segments * o.segment_frames;
    out->n_seg = whole ? 1u : o.segments;
    out->seg_len = whole ? out->v : o.segment_frames;
    return RG_OK;
}

uint64_t rg_cmp_plan_lags(RgCmpPair *pairs, size_t n, uint64_t *n_rows) {
    uint64_t tiles = 0, rows = 0;
    for (size_t i = 0; i < n; ++i) {
        pairs[i].first_tile = tiles;
        pairs[i].first_row = rows;
        if (!pairs[i].cc) continue;
        tiles += rg_cmp_pair_tiles(pairs[i]);
        rows += rg_cmp_pair_rows(pairs[i]);
    }
    *n_rows = rows;
    return tiles;
}

uint64_t rg_cmp_plan_moments(RgCmpPair *pairs, size_t n, uint64_t kind_piece[5], uint64_t *n_blocks) {
    uint64_t pieces = 0, blocks = 0;
    for (uint32_t kind = 0; kind < 4; ++kind) {
        kind_piece[kind] = pieces;
        for (size_t i = 0; i < n; ++i) {
            RgCmpPair &p = pairs[i];
            if (rg_cmp_kind(p.fmt_a, p.fmt_b) != kind) continue;
            p.first_piece = pieces;
            p.first_block = blocks;
            if (!p.cc) continue;
            pieces += rg_cmp_pair_pieces(p);
            blocks += p.n_blocks;
        }
    }
    kind_piece[4] = pieces;
    *n_blocks = blocks;
    return pieces;
}

// ---- the pick ------------------------------------------------------------------------------------------------------------------
// d*, the sign and the lock of `n_rows` rows taken together
static void pick_rows(const int64_t *rows, uint32_t n_rows, uint32_t radius, int32_t *d_out, int32_t *sigma, double *lock) {
    const uint32_t RL = rg_cmp_row_len(radius);
    int32_t best_d = 0;
    i128 best_t = 0;
    u128 best_abs = 0;
    for (int32_t d = -(int32_t)radius; d <= (int32_t)radius; ++d) {
        i128 t = 0;
        for (uint32_t r = 0; r < n_rows; ++r) t += rows[(size_t)r * RL + (uint32_t)(d + (int32_t)radius)];
        const u128 mag = t < 0 ? (u128)(-t) : (u128)t;
        const int32_t ad = d < 0 ? -d : d, ab = best_d < 0 ? -best_d : best_d;
        const bool first = d == -(int32_t)radius;
        if (first || mag > best_abs || (mag == best_abs && (ad < ab || (ad == ab && d < best_d)))) {
            best_d = d;
            best_t = t;
            best_abs = mag;
        }
    }
    u128 ea = 0, eb = 0;
    for (uint32_t r = 0; r < n_rows; ++r) {
        ea += (u128)(uint64_t)rows[(size_t)r * RL + 2u * radius + 1u];
        eb += (u128)(uint64_t)rows[(size_t)r * RL + 2u * radius + 2u];
    }
    *d_out = best_d;
    *sigma = best_t < 0 ? -1 : 1;
    *lock = (ea && eb) ? (double)best_abs / sqrt((double)ea * (double)eb) : 0.0;
}

RgCmpPicked rg_cmp_pick(const RgCmpPair &p, const rg_compare_opts &o, const int64_t *rows) {
    RgCmpPicked k;
    memset(&k, 0, sizeof k);
    const double need = (double)o.lock_permille / 1000.0;
    pick_rows(rows, p.n_seg * p.cc, o.radius, &k.d, &k.sigma, &k.lock);
    if (k.lock >= need) k.flags |= RG_CMP_LOCKED;
    if (o.radius > 0 && (uint32_t)(k.d < 0 ? -k.d : k.d) == o.radius) k.flags |= RG_CMP_AT_EDGE;
    for (uint32_t s = 0; s < p.n_seg; ++s) {
        int32_t d, sigma;
        double lock;
        pick_rows(rows + (size_t)s * p.cc * rg_cmp_row_len(o.radius), p.cc, o.radius, &d, &sigma, &lock);
        if (!(lock >= need)) continue;
        const int64_t lag = p.h + d;
        if (!k.locked_segments || lag < k.seg_lag_min) k.seg_lag_min = lag;
        if (!k.locked_segments || lag > k.seg_lag_max) k.seg_lag_max = lag;
        k.locked_segments += 1;
    }
    if (k.locked_segments > 1 && k.seg_lag_max - k.seg_lag_min > (int64_t)o.drift_frames) k.flags |= RG_CMP_DRIFT;
    return k;
}

void rg_cmp_set_lag(RgCmpPair *p, const RgCmpPicked &k) {
    p->lag = p->h + k.d;
    p->sigma = k.sigma;
    const int64_t m0 = p->lag < 0 ? -p->lag : 0, m1 = (int64_t)p->nb - p->lag < (int64_t)p->na ? (int64_t)p->nb - p->lag : (int64_t)p->na;
    p->m0 = (uint32_t)m0;
    p->w = m1 > m0 ? (uint32_t)(m1 - m0) : 0u;
    p->n_blocks = (uint32_t)(((uint64_t)p->w + p->block - 1) / p->block);
    p->pieces_per_block = rg_cmp_pieces_of(p->block, rg_cmp_piece_frames(p->fmt_a, p->fmt_b));
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
static int64_t q_of(uint32_t format, uint32_t raw, uint64_t *nonfinite) {
    if (format == RG_FMT_S16_PLANAR) return (int32_t)raw;
    if (format == RG_FMT_S32_PLANAR) return (int32_t)raw >> 16;
    float x;
    memcpy(&x, &raw, 4);
    if (!std::isfinite(x)) {
        ++*nonfinite;
        return 0;
    }
    const double xd = x;
    const long long q = llrint((xd < -1.0 ? -1.0 : (xd > 1.0 ? 1.0 : xd)) * 32768.0);  // exact in float, so exact in double
    return q > 32767 ? 32767 : q;
}
static std::vector<int16_t> q_plane(const unsigned char *plane, uint32_t format, uint64_t n) {
    std::vector<int16_t> q(n);
    uint64_t nf = 0;
    for (uint64_t j = 0; j < n; ++j) q[j] = (int16_t)q_of(format, rg_pcm_raw_at(plane, format, j), &nf);
    return q;
}

void rg_cmp_lags_serial(const unsigned char *arena, const RgCmpPair &p, uint32_t radius, int64_t *rows) {
    const uint32_t RL = rg_cmp_row_len(radius);
    for (uint32_t c = 0; c < p.cc; ++c) {
        const std::vector<int16_t> qa = q_plane(arena + rg_cmp_plane_a(p, c), p.fmt_a, p.na), qb = q_plane(arena + rg_cmp_plane_b(p, c), p.fmt_b, p.nb);
        for (uint32_t s = 0; s < p.n_seg; ++s) {
            int64_t *row = rows + ((size_t)s * p.cc + c) * RL;
            const int64_t start = (int64_t)rg_cmp_seg_start(p, s), end = start + p.seg_len;
            for (int64_t d = -(int64_t)radius; d <= (int64_t)radius; ++d) {
                int64_t sum = 0;
                for (int64_t n = start; n < end; ++n) {
                    const int64_t m = n + p.h + d;
                    if (m >= 0 && m < (int64_t)p.nb) sum += (int64_t)qa[n] * qb[m];
                }
                row[d + radius] = sum;
            }
            int64_t ea = 0, eb = 0;
            for (int64_t n = start; n < end; ++n) {
                ea += (int64_t)qa[n] * qa[n];
                const int64_t m = n + p.h;
                if (m >= 0 && m < (int64_t)p.nb) eb += (int64_t)qb[m] * qb[m];
            }
            row[2 * radius + 1] = ea;
            row[2 * radius + 2] = eb;
        }
    }
}

RgCmpTotals rg_cmp_moments_serial(const unsigned char *arena, const RgCmpPair &p, rg_compare_block *blocks) {
    RgCmpTotals t;
    memset(&t, 0, sizeof t);
    t.first_diff = RG_CMP_NONE;
    const bool raw = p.fmt_a == p.fmt_b && p.sigma > 0;
    for (uint64_t at = 0; at < p.w; at += p.block) {
        const uint64_t len = p.block < p.w - at ? p.block : p.w - at;
        int64_t aa = 0, bb = 0, ab = 0;
        uint64_t equal = 0, first = RG_CMP_NONE, nonfinite = 0;
        uint32_t max_diff = 0;
        for (uint32_t c = 0; c < p.cc; ++c) {
            const unsigned char *pa = arena + rg_cmp_plane_a(p, c), *pb = arena + rg_cmp_plane_b(p, c);
            for (uint64_t j = at; j < at + len; ++j) {
                const uint64_t fa = p.m0 + j, fb = (uint64_t)((int64_t)fa + p.lag);
                const uint32_t ra = rg_pcm_raw_at(pa, p.fmt_a, fa), rb = rg_pcm_raw_at(pb, p.fmt_b, fb);
                const int64_t qa = q_of(p.fmt_a, ra, &nonfinite), qb = q_of(p.fmt_b, rb, &nonfinite);
                aa += qa * qa;
                bb += qb * qb;
                ab += qa * qb;
                bool eq;
                if (!raw) {
                    eq = qa == p.sigma * qb;
                } else if (p.fmt_a == RG_FMT_F32_PLANAR) {
                    float xa, xb;
                    memcpy(&xa, &ra, 4);
                    memcpy(&xb, &rb, 4);
                    eq = xa == xb;
                } else {
                    eq = (int32_t)ra == (int32_t)rb;
                }
                equal += eq;
                if (!eq && fa < first) first = fa;
                const int64_t diff = qa - p.sigma * qb;
                if ((uint64_t)(diff < 0 ? -diff : diff) > max_diff) max_diff = (uint32_t)(diff < 0 ? -diff : diff);
            }
        }
        blocks[t.blocks] = rg_compare_block{aa, bb, ab, first, (uint32_t)equal, max_diff, (uint32_t)len, 0u};
        t.aa += (uint64_t)aa;
        t.bb += (uint64_t)bb;
        t.ab += ab;
        t.equal += equal;
        t.nonfinite += nonfinite;
        if (first < t.first_diff) t.first_diff = first;
        if (max_diff > t.max_diff) t.max_diff = max_diff;
        t.differing += equal < len * p.cc;
        t.blocks += 1;
    }
    return t;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
static int16_t q16_of(uint32_t format, const unsigned char *plane, uint64_t j) {
    bool finite;
    return (int16_t)rg_cmp_q(format, rg_pcm_raw_at(plane, format, j), &finite);
}

void rg_cmp_lags_folded(const unsigned char *arena, const RgCmpPair &p, uint32_t radius, int64_t *rows) {
    const uint32_t RL = rg_cmp_row_len(radius), W = 2 * radius + 1, groups = rg_cmp_groups(radius);
    for (uint64_t r = 0; r < rg_cmp_pair_rows(p) * RL; ++r) rows[r] = 0;
    std::vector<int16_t> sa(RG_CMP_TILE), sb(RG_CMP_B_LDS);
    for (uint64_t rel = 0; rel < rg_cmp_pair_tiles(p); ++rel) {  // the lag kernel, one workgroup per tile
        uint32_t s, c;
        uint64_t tstart;
        const uint32_t len = rg_cmp_tile_window(p, rel, &s, &c, &tstart);
        const uint32_t strips = (len + RG_CMP_STRIP - 1) / RG_CMP_STRIP;
        const unsigned char *pa = arena + rg_cmp_plane_a(p, c), *pb = arena + rg_cmp_plane_b(p, c);
        int64_t *row = rows + ((size_t)s * p.cc + c) * RL;
        for (uint32_t i = 0; i < strips * RG_CMP_STRIP; ++i) sa[i] = i < len ? q16_of(p.fmt_a, pa, tstart + i) : (int16_t)0;
        for (uint32_t k = 0; k < RG_CMP_STRIP * (strips + groups); ++k) {
            const int64_t m = (int64_t)tstart + p.h + (int64_t)k - (int64_t)radius;
            sb[k] = m >= 0 && m < (int64_t)p.nb ? q16_of(p.fmt_b, pb, (uint64_t)m) : (int16_t)0;
        }
        for (uint32_t lane = 0; lane < RG_CMP_LANES; ++lane) {
            uint32_t first, g;
            const uint32_t end = rg_cmp_lane_strips(lane, groups, strips, &g, &first);
            double acc[RG_CMP_LAG_GROUP] = {0.0};
            for (uint32_t st = first; st < end; ++st)
                for (uint32_t i = 0; i < RG_CMP_STRIP; ++i)
                    for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j) acc[j] += (double)sa[RG_CMP_STRIP * st + i] * (double)sb[RG_CMP_STRIP * (st + g) + i + j];
            for (uint32_t j = 0; j < RG_CMP_LAG_GROUP; ++j)
                if (RG_CMP_LAG_GROUP * g + j < W) row[RG_CMP_LAG_GROUP * g + j] += (int64_t)acc[j];
            uint64_t ea = 0, eb = 0;  // the lanes' share of EA and EB: frames lane, lane + 256, ...
            for (uint32_t i = lane; i < len; i += RG_CMP_LANES) {
                ea += (uint64_t)((int32_t)sa[i] * (int32_t)sa[i]);
                eb += (uint64_t)((int32_t)sb[i + radius] * (int32_t)sb[i + radius]);
            }
            row[W] += (int64_t)ea;
            row[W + 1] += (int64_t)eb;
        }
    }
}

RgCmpTotals rg_cmp_moments_folded(const unsigned char *arena, const RgCmpPair &p, rg_compare_block *blocks) {
    RgCmpTotals t;
    memset(&t, 0, sizeof t);
    t.first_diff = RG_CMP_NONE;
    const uint64_t per = rg_cmp_channel_pieces(p);
    std::vector<RgCmpPiece> pieces(per * p.cc);
    for (uint64_t rel = 0; rel < pieces.size(); ++rel) {  // the moments kernels, one workgroup per piece
        uint32_t c, b, start;
        const uint32_t len = rg_cmp_piece_window(p, rel, &c, &b, &start);
        const unsigned char *pa = arena + rg_cmp_plane_a(p, c), *pb = arena + rg_cmp_plane_b(p, c);
        RgCmpPiece acc = rg_cmp_empty();
        for (uint32_t j = 0; j < len; ++j) {
            const uint64_t fa = (uint64_t)p.m0 + start + j, fb = (uint64_t)((int64_t)fa + p.lag);
            const uint32_t ra = rg_pcm_raw_at(pa, p.fmt_a, fa), rb = rg_pcm_raw_at(pb, p.fmt_b, fb);
            if (p.fmt_a != p.fmt_b)
                rg_cmp_take_mixed(p.fmt_a, ra, p.fmt_b, rb, p.sigma, fa, &acc);
            else if (p.fmt_a == RG_FMT_F32_PLANAR)
                rg_cmp_take<RG_FMT_F32_PLANAR>(ra, rb, p.sigma, fa, &acc);
            else if (p.fmt_a == RG_FMT_S16_PLANAR)
                rg_cmp_take<RG_FMT_S16_PLANAR>(ra, rb, p.sigma, fa, &acc);
            else
                rg_cmp_take<RG_FMT_S32_PLANAR>(ra, rb, p.sigma, fa, &acc);
        }
        pieces[rel] = acc;
    }
    for (uint32_t b = 0; b < p.n_blocks; ++b) {  // the fold
        uint32_t start;
        const uint32_t len = rg_cmp_block_window(p, b, &start);
        const uint32_t cnt = rg_cmp_pieces_of(len, rg_cmp_piece_frames(p.fmt_a, p.fmt_b));
        RgCmpPiece blk = rg_cmp_empty();
        for (uint32_t c = 0; c < p.cc; ++c)
            for (uint32_t k = 0; k < cnt; ++k) rg_cmp_combine(&blk, pieces[c * per + (uint64_t)b * p.pieces_per_block + k]);
        blocks[b] = rg_cmp_block_row(blk, len);
        rg_cmp_block_into(&t, blk, len, p.cc);
    }
    return t;
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
static void fill_head(const rg_track_desc *descs, const rg_compare_pair &pair, const rg_compare_opts &o, const RgCmpPair &p, uint32_t dropped_a,
                      uint32_t dropped_b, rg_compare_result *out) {
    memset(out, 0, sizeof *out);
    const rg_track_desc &ta = descs[pair.a], &tb = descs[pair.b];
    out->status = RG_OK;
    out->a = pair.a;
    out->b = pair.b;
    out->frames_a = ta.frames;
    out->frames_b = tb.frames;
    out->sample_rate = ta.sample_rate;
    out->channels = ta.channels < tb.channels ? ta.channels : tb.channels;
    out->format_a = ta.format;
    out->format_b = tb.format;
    out->dropped_a = dropped_a;
    out->dropped_b = dropped_b;
    out->block_frames = p.block;
    out->radius = o.radius;
    out->hint = pair.hint;
    out->first_diff = RG_CMP_NONE;
    out->flags = p.flags | ((dropped_a | dropped_b) == 0 ? RG_CMP_COMPLETE : 0u);
}

void rg_cmp_fill_skipped(const rg_track_desc *descs, const rg_compare_pair &pair, const rg_compare_opts &o, const RgCmpPair &p, uint32_t dropped_a,
                         uint32_t dropped_b, rg_compare_result *out) {
    fill_head(descs, pair, o, p, dropped_a, dropped_b, out);
}

void rg_cmp_fill(const rg_track_desc *descs, const rg_compare_pair &pair, const rg_compare_opts &o, const RgCmpPair &p, const RgCmpPicked &k,
                 const RgCmpTotals &tot, const rg_compare_block *blocks, uint32_t dropped_a, uint32_t dropped_b, uint32_t more_flags,
                 rg_compare_result *out) {
    fill_head(descs, pair, o, p, dropped_a, dropped_b, out);
    uint32_t flags = out->flags | more_flags | k.flags;
    out->segments = p.n_seg;
    out->locked_segments = k.locked_segments;
    out->polarity = k.sigma;
    out->max_diff = tot.max_diff;
    out->lag = p.lag;
    out->seg_lag_min = k.seg_lag_min;
    out->seg_lag_max = k.seg_lag_max;
    out->overlap = p.w;
    out->a_head = p.m0;
    out->a_tail = (uint64_t)p.na - p.m0 - p.w;
    out->b_head = (uint64_t)((int64_t)p.m0 + p.lag);
    out->b_tail = (uint64_t)((int64_t)p.nb - (int64_t)p.m0 - (int64_t)p.w - p.lag);
    out->blocks = tot.blocks;
    out->differing_blocks = tot.differing;
    out->equal = tot.equal;
    out->first_diff = tot.first_diff;
    out->nonfinite = tot.nonfinite;
    out->aa = (int64_t)tot.aa;
    out->bb = (int64_t)tot.bb;
    out->ab = tot.ab;
    out->lock = k.lock;
    const i128 AA = (i128)tot.aa, BB = (i128)tot.bb, AB = (i128)tot.ab;
    const double aa = (double)tot.aa, bb = (double)tot.bb, ab = (double)tot.ab, samples = (double)((uint64_t)p.w * p.cc);
    const double gamma = tot.bb ? ab / bb : 0.0;
    out->gain_db = (tot.ab != 0 && tot.bb != 0) ? 20.0 * log10(fabs(gamma)) : 0.0;
    const u128 unity = (u128)(AA - 2 * (i128)k.sigma * AB + BB);  // a sum of squares: never negative
    out->null_unity_db = !tot.aa ? 0.0 : (unity ? 10.0 * log10((double)unity / aa) : -INFINITY);
    const u128 det = (u128)(AA * BB - AB * AB);  // Cauchy-Schwarz: never negative
    out->null_db = (!tot.aa || !tot.bb) ? 0.0 : (det ? 10.0 * log10((double)det / (double)(u128)(AA * BB)) : -INFINITY);
    const double g2 = gamma * gamma;
    out->residual_lsb2 = !p.w ? 0.0 : (tot.bb ? (double)det / bb / samples / (g2 > 1.0 ? g2 : 1.0) : aa / samples);
    bool any_worst = false, any_gain = false;
    const double two_g = 2.0 * gamma;
    for (uint32_t b = 0; b < tot.blocks; ++b) {
        const rg_compare_block &r = blocks[b];
        if (r.aa > 0) {
            const double t1 = two_g * (double)r.ab, t2 = g2 * (double)r.bb;
            const double res = ((double)r.aa - t1) + t2;
            const double db = res > 0.0 ? 10.0 * log10(res / (double)r.aa) : -INFINITY;
            if (!any_worst || db > out->worst_block_db) {
                out->worst_block = b;
                out->worst_block_db = db;
            }
            any_worst = true;
        }
        if ((u128)100 * (u128)r.aa * tot.blocks >= (u128)tot.aa && r.ab != 0 && r.bb != 0) {
            const double g = 20.0 * log10(fabs((double)r.ab / (double)r.bb));
            if (!any_gain || g < out->gain_min_db) out->gain_min_db = g;
            if (!any_gain || g > out->gain_max_db) out->gain_max_db = g;
            any_gain = true;
        }
    }
    const bool identical = p.w > 0 && k.sigma > 0 && tot.equal == (uint64_t)p.w * p.cc, locked = (k.flags & RG_CMP_LOCKED) != 0;
    if (identical) flags |= RG_CMP_IDENTICAL;
    if (p.lag != 0) flags |= RG_CMP_SHIFTED;
    if (out->a_head | out->a_tail | out->b_head | out->b_tail) flags |= RG_CMP_LENGTHS;
    if (k.sigma < 0) flags |= RG_CMP_INVERTED;
    if (tot.nonfinite) flags |= RG_CMP_NONFINITE;
    if (p.fmt_a == p.fmt_b && k.sigma > 0) flags |= RG_CMP_RAW;
    if (!locked)
        flags |= RG_CMP_UNRELATED;
    else if (!identical)
        flags |= out->residual_lsb2 <= (double)o.requant_millilsb2 / 1000.0 ? RG_CMP_SAME_MASTER : RG_CMP_DIFFERS;
    out->flags = flags;
}

void rg_cmp_rows_out(const RgCmpPair &p, const rg_compare_opts &o, const int64_t *rows, int64_t *slab) {
    const uint32_t RL = rg_cmp_row_len(o.radius);
    for (uint32_t s = 0; s < p.n_seg; ++s)
        for (uint32_t c = 0; c < p.cc; ++c) memcpy(slab + ((size_t)s * RG_CMP_MAX_CHANNELS + c) * RL, rows + ((size_t)s * p.cc + c) * RL, RL * sizeof(int64_t));
}

void rg_cmp_blocks_out(const RgCmpPair &p, const rg_compare_block *blocks, rg_compare_block *out, size_t blocks_per_pair) {
    const size_t cnt = p.n_blocks < blocks_per_pair ? p.n_blocks : blocks_per_pair;
    if (cnt) memcpy(out, blocks, cnt * sizeof *out);
}

int rg_cmp_arena_host(int route, size_t n, const rg_track_desc *descs, size_t n_pairs, const rg_compare_pair *pairs, const rg_compare_opts *opts,
                      const void *arena, size_t arena_bytes, rg_compare_result *out, rg_compare_block *blocks_out, size_t blocks_per_pair,
                      int64_t *lag_sums, char *err, size_t err_len) {
    rg_compare_opts o;
    int rc = rg_pcm_check_host_route("rg_compare_arena", "folded", route, n_pairs, pairs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_cmp_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    const size_t slab = (size_t)o.segments * RG_CMP_MAX_CHANNELS * rg_cmp_row_len(o.radius);
    if (lag_sums && n_pairs) memset(lag_sums, 0, n_pairs * slab * sizeof(int64_t));
    if (blocks_out && n_pairs && blocks_per_pair) memset(blocks_out, 0, n_pairs * blocks_per_pair * sizeof *blocks_out);
    std::vector<RgCmpPair> plan(n_pairs + 1);
    for (size_t i = 0; i < n_pairs; ++i) {
        rc = rg_cmp_plan_pair(i, descs, n, pairs[i], o, false, arena_bytes, &plan[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    for (size_t i = 0; i < n_pairs; ++i) {
        RgCmpPair &p = plan[i];
        if (!p.cc) {
            rg_cmp_fill_skipped(descs, pairs[i], o, p, 0, 0, &out[i]);
            continue;
        }
        std::vector<int64_t> rows(rg_cmp_pair_rows(p) * rg_cmp_row_len(o.radius));
        if (route == 0)
            rg_cmp_lags_serial(base, p, o.radius, rows.data());
        else
            rg_cmp_lags_folded(base, p, o.radius, rows.data());
        const RgCmpPicked k = rg_cmp_pick(p, o, rows.data());
        rg_cmp_set_lag(&p, k);
        std::vector<rg_compare_block> blocks(p.n_blocks + 1);
        const RgCmpTotals tot = route == 0 ? rg_cmp_moments_serial(base, p, blocks.data()) : rg_cmp_moments_folded(base, p, blocks.data());
        rg_cmp_fill(descs, pairs[i], o, p, k, tot, blocks.data(), 0, 0, 0, &out[i]);
        if (lag_sums) rg_cmp_rows_out(p, o, rows.data(), lag_sums + i * slab);
        if (blocks_out) rg_cmp_blocks_out(p, blocks.data(), blocks_out + i * blocks_per_pair, blocks_per_pair);
    }
    return RG_OK;
}

extern "C" int rg_compare_kernel_shape(uint32_t format_a, uint32_t format_b, uint32_t *piece_frames, uint32_t *tile_frames, uint32_t *strip_frames,
                                       uint32_t *lag_group, uint32_t *lds_bytes) {
    if (!rg_pcm_is_planar(format_a) || !rg_pcm_is_planar(format_b)) return RG_ERR_FORMAT;
    if (piece_frames) *piece_frames = rg_cmp_piece_frames(format_a, format_b);
    if (tile_frames) *tile_frames = RG_CMP_TILE;
    if (strip_frames) *strip_frames = RG_CMP_STRIP;
    if (lag_group) *lag_group = RG_CMP_LAG_GROUP;
    if (lds_bytes) *lds_bytes = RG_CMP_LDS_BYTES;
    return RG_OK;
}
