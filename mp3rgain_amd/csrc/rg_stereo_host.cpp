// rg_stereo_host.cpp -- the host side of the stereo image scan (include/mp3rgain_amd_stereo.h, rg_stereo.h): the options, the
// track records and their checks, the serial host twin (route 0: the definitions, written plainly, one loop per sum), the
// kernels' cutting and fold arithmetic walked by the host (route 2: the same take, combine, block and choice functions as
// rg_stereo.hip runs, tiles of strips and lag groups summed in double), and the finish every route shares (the square roots
// and logarithms).  Plain C++: no device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "rg_stereo.h"

int rg_st_options(const rg_stereo_opts *opts, rg_stereo_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts
                : rg_stereo_opts{0u, RG_ST_DEFAULT_RADIUS, RG_ST_DEFAULT_PHASE_PERMILLE, RG_ST_DEFAULT_DELAY_PERMILLE, RG_ST_DEFAULT_MONO_DB, RG_ST_DEFAULT_BALANCE_DB};
    if (out->radius > RG_ST_MAX_RADIUS) {
        snprintf(err, err_len, "stereo: radius %u is more than %u", out->radius, RG_ST_MAX_RADIUS);
        return RG_ERR_INVALID_ARG;
    }
    if (out->block_frames > RG_ST_MAX_BLOCK_FRAMES) {
        snprintf(err, err_len, "stereo: block_frames %u is more than %u", out->block_frames, RG_ST_MAX_BLOCK_FRAMES);
        return RG_ERR_INVALID_ARG;
    }
    const struct {
        const char *name;
        uint32_t v;
    } th[4] = {{"phase_permille", out->phase_permille}, {"delay_permille", out->delay_permille}, {"mono_db", out->mono_db}, {"balance_db_limit", out->balance_db_limit}};
    for (const auto &t : th)
        if (t.v < 1 || t.v > 1000) {
            snprintf(err, err_len, "stereo: %s %u is not in 1 .. 1000", t.name, t.v);
            return RG_ERR_INVALID_ARG;
        }
    return RG_OK;
}

int rg_st_track(size_t i, const rg_track_desc &t, const rg_stereo_opts &o, bool rate_is_format, size_t arena_bytes, RgStTrack *out, char *err,
                size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_ST_MAX_CHANNELS, "the stereo scan takes", err, err_len);
    if (rc != RG_OK) return rc;
    const uint64_t block = o.block_frames ? o.block_frames : (uint64_t)t.sample_rate;
    if (block < 1 || block > RG_ST_MAX_BLOCK_FRAMES) {
        snprintf(err, err_len, "track %zu: a block of %llu frames (sample rate %u) is not in 1 .. %u", i, (unsigned long long)block, t.sample_rate,
                 RG_ST_MAX_BLOCK_FRAMES);
        return rate_is_format && !o.block_frames ? RG_ERR_FORMAT : RG_ERR_INVALID_ARG;
    }
    rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    memset(out, 0, sizeof *out);
    out->block = (uint32_t)block;
    out->format = t.format;
    out->pieces_per_block = rg_st_pieces_of(out->block, t.format);
    if (t.channels < 2) return RG_OK;  // not measured: no frames, no blocks, no tiles
    out->off_l = rg_pcm_plane_off(t, 0);
    out->off_r = rg_pcm_plane_off(t, 1);
    out->n = (uint32_t)t.frames;
    out->n_blocks = (uint32_t)((t.frames + block - 1) / block);
    out->n_tiles = (uint32_t)((t.frames + RG_ST_TILE - 1) / RG_ST_TILE);
    return RG_OK;
}

uint64_t rg_st_plan(RgStTrack *tracks, size_t n, uint64_t fmt_piece[4], uint64_t *n_tiles) {
    uint64_t pieces = 0, tiles = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_piece[f] = pieces;
        for (size_t i = 0; i < n; ++i) {
            RgStTrack &t = tracks[i];
            if (t.format != f) continue;
            t.first_piece = pieces;
            t.first_tile = tiles;
            pieces += rg_st_track_pieces(t);
            tiles += t.n_tiles;
        }
    }
    fmt_piece[3] = pieces;
    *n_tiles = tiles;
    return pieces;
}

// the choice of the two lags from the 2 * radius + 1 sums, in ascending d
static void choose(const int64_t *sums, uint32_t radius, RgStTotals *t) {
    t->lag = t->anti_lag = -(int32_t)radius;
    t->lag_sum = t->anti_sum = sums[0];
    for (int32_t d = -(int32_t)radius + 1; d <= (int32_t)radius; ++d) {
        const int64_t c = sums[d + (int32_t)radius];
        if (rg_st_better(c, d, t->lag_sum, t->lag)) {
            t->lag_sum = c;
            t->lag = d;
        }
        if (rg_st_lower(c, d, t->anti_sum, t->anti_lag)) {
            t->anti_sum = c;
            t->anti_lag = d;
        }
    }
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

RgStTotals rg_st_serial_host(const unsigned char *arena, const RgStTrack &t, uint32_t radius, int64_t *sums) {
    RgStTotals o;
    memset(&o, 0, sizeof o);
    const uint64_t N = t.n, B = t.block;
    const uint32_t W = 2 * radius + 1;
    for (uint32_t k = 0; k < W; ++k) sums[k] = 0;
    if (!N) return o;
    const unsigned char *pl = arena + t.off_l, *pr = arena + t.off_r;
    std::vector<int16_t> ql(N), qr(N);
    for (uint64_t j = 0; j < N; ++j) {
        ql[j] = (int16_t)q_of(t.format, rg_pcm_raw_at(pl, t.format, j), &o.nonfinite);
        qr[j] = (int16_t)q_of(t.format, rg_pcm_raw_at(pr, t.format, j), &o.nonfinite);
    }
    for (uint64_t at = 0; at < N; at += B) {
        const uint64_t n = B < N - at ? B : N - at;
        int64_t ell = 0, err = 0, elr = 0;
        uint64_t equal = 0;
        for (uint64_t j = at; j < at + n; ++j) {
            ell += (int64_t)ql[j] * ql[j];
            err += (int64_t)qr[j] * qr[j];
            elr += (int64_t)ql[j] * qr[j];
            const uint32_t rl = rg_pcm_raw_at(pl, t.format, j), rr = rg_pcm_raw_at(pr, t.format, j);
            bool eq, opp, zero;
            if (t.format == RG_FMT_F32_PLANAR) {
                float xl, xr;
                memcpy(&xl, &rl, 4);
                memcpy(&xr, &rr, 4);
                eq = xl == xr;
                opp = xl == -xr && xl != 0.0f;
                zero = xl == 0.0f && xr == 0.0f;
            } else {
                const int64_t vl = (int32_t)rl, vr = (int32_t)rr;
                eq = vl == vr;
                opp = vl + vr == 0 && vl != 0;
                zero = vl == 0 && vr == 0;
            }
            equal += eq;
            o.opposite += opp;
            o.zero += zero;
        }
        o.ell += (uint64_t)ell;
        o.err += (uint64_t)err;
        o.elr += elr;
        o.equal += equal;
        o.blocks += 1;
        o.active += ell + err > 0;
        o.neg += elr < 0;
        o.mono += ell + err > 0 && equal == n;
    }
    for (int64_t d = -(int64_t)radius; d <= (int64_t)radius; ++d) {
        int64_t c = 0;
        for (int64_t n = 0; n < (int64_t)N; ++n)
            if (n + d >= 0 && n + d < (int64_t)N) c += (int64_t)ql[n] * qr[n + d];
        sums[d + radius] = c;
    }
    choose(sums, radius, &o);
    return o;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
template <int FMT>
static RgStPiece piece_sums(const unsigned char *pl, const unsigned char *pr, uint64_t first, uint32_t n) {
    RgStPiece acc = rg_st_empty();
    for (uint32_t j = 0; j < n; ++j) rg_st_take<FMT>(rg_pcm_raw_at(pl, FMT, first + j), rg_pcm_raw_at(pr, FMT, first + j), &acc);
    return acc;
}
template <int FMT>
static int16_t q16(const unsigned char *plane, uint64_t j) {
    bool finite;
    return (int16_t)rg_st_q<FMT>(rg_pcm_raw_at(plane, FMT, j), &finite);
}
static int16_t q16_of(uint32_t format, const unsigned char *plane, uint64_t j) {
    return format == RG_FMT_F32_PLANAR ? q16<RG_FMT_F32_PLANAR>(plane, j) : format == RG_FMT_S16_PLANAR ? q16<RG_FMT_S16_PLANAR>(plane, j) : q16<RG_FMT_S32_PLANAR>(plane, j);
}

RgStTotals rg_st_folded_host(const unsigned char *arena, const RgStTrack &t, uint32_t radius, int64_t *sums) {
    const unsigned char *pl = arena + t.off_l, *pr = arena + t.off_r;
    RgStTotals o;
    memset(&o, 0, sizeof o);
    const uint32_t W = 2 * radius + 1, groups = rg_st_groups(radius);
    for (uint32_t k = 0; k < W; ++k) sums[k] = 0;
    for (uint32_t b = 0; b < t.n_blocks; ++b) {  // the moments kernel, one workgroup per piece, and the fold
        uint64_t bstart;
        const uint32_t len = rg_st_block_window(t, b, &bstart);
        RgStPiece acc = rg_st_empty();
        for (uint32_t k = 0; k < rg_st_pieces_of(len, t.format); ++k) {
            uint32_t pstart;
            const uint32_t plen = rg_st_piece_window(len, k, t.format, &pstart);
            const uint64_t first = bstart + pstart;
            rg_st_combine(&acc, t.format == RG_FMT_F32_PLANAR   ? piece_sums<RG_FMT_F32_PLANAR>(pl, pr, first, plen)
                                : t.format == RG_FMT_S16_PLANAR ? piece_sums<RG_FMT_S16_PLANAR>(pl, pr, first, plen)
                                                                : piece_sums<RG_FMT_S32_PLANAR>(pl, pr, first, plen));
        }
        rg_st_block_into(&o, acc, len);
    }
    // the lag kernel: a tile's two planes as its LDS holds them, every lane's strips and lag group in double
    std::vector<int16_t> left(RG_ST_TILE), right(RG_ST_RIGHT_LDS);
    for (uint32_t k = 0; k < t.n_tiles; ++k) {
        uint64_t tstart;
        const uint32_t len = rg_st_tile_window(t, k, &tstart);
        const uint32_t strips = (len + RG_ST_STRIP - 1) / RG_ST_STRIP;
        for (uint32_t i = 0; i < strips * RG_ST_STRIP; ++i) left[i] = i < len ? q16_of(t.format, pl, tstart + i) : (int16_t)0;
        for (uint32_t p = 0; p < RG_ST_STRIP * (strips + groups); ++p) {
            const int64_t m = (int64_t)tstart + p - radius;
            right[p] = m >= 0 && m < (int64_t)t.n ? q16_of(t.format, pr, (uint64_t)m) : (int16_t)0;
        }
        for (uint32_t lane = 0; lane < RG_ST_LANES; ++lane) {
            uint32_t first;
            const uint32_t end = rg_st_lane_strips(lane, groups, strips, &first), g = lane % groups;
            double acc[RG_ST_LAG_GROUP] = {0.0};
            for (uint32_t c = first; c < end; ++c)
                for (uint32_t i = 0; i < RG_ST_STRIP; ++i)
                    for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j) acc[j] += (double)left[RG_ST_STRIP * c + i] * (double)right[RG_ST_STRIP * (c + g) + i + j];
            for (uint32_t j = 0; j < RG_ST_LAG_GROUP; ++j)
                if (RG_ST_LAG_GROUP * g + j < W) sums[RG_ST_LAG_GROUP * g + j] += (int64_t)acc[j];
        }
    }
    // the choice, by the fold kernel's tree: the lanes' candidates, then halves
    struct Pick {
        int64_t c;
        int32_t d;
    };
    std::vector<Pick> hi(RG_ST_LANES), lo(RG_ST_LANES);
    for (uint32_t l = 0; l < RG_ST_LANES; ++l) {
        const uint32_t a = l < W ? l : 0u;  // (a lane without a candidate repeats the first)
        hi[l] = lo[l] = Pick{sums[a], (int32_t)a - (int32_t)radius};
        const uint32_t b = l + RG_ST_LANES;
        if (b < W) {
            const Pick p{sums[b], (int32_t)b - (int32_t)radius};
            if (rg_st_better(p.c, p.d, hi[l].c, hi[l].d)) hi[l] = p;
            if (rg_st_lower(p.c, p.d, lo[l].c, lo[l].d)) lo[l] = p;
        }
    }
    for (uint32_t half = RG_ST_LANES / 2; half >= 1; half >>= 1)
        for (uint32_t l = 0; l < half; ++l) {
            if (rg_st_better(hi[l + half].c, hi[l + half].d, hi[l].c, hi[l].d)) hi[l] = hi[l + half];
            if (rg_st_lower(lo[l + half].c, lo[l + half].d, lo[l].c, lo[l].d)) lo[l] = lo[l + half];
        }
    o.lag = hi[0].d;
    o.lag_sum = hi[0].c;
    o.anti_lag = lo[0].d;
    o.anti_sum = lo[0].c;
    return o;
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
// 10 log10(a / b) of two non-negative numbers, and what it is when one of them is 0
static double ratio_db(double a, double b) {
    if (a > 0.0 && b > 0.0) return 10.0 * log10(a / b);
    return a > 0.0 ? INFINITY : (b > 0.0 ? -INFINITY : 0.0);
}

void rg_st_fill(const rg_track_desc &t, const rg_stereo_opts &o, uint32_t block, uint32_t dropped_frames, const RgStTotals &tot, rg_stereo_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->dropped_frames = dropped_frames;
    out->block_frames = block;
    out->radius = o.radius;
    uint32_t flags = dropped_frames == 0 ? RG_ST_COMPLETE : 0u;
    if (t.channels < 2) {
        out->flags = flags | RG_ST_MONO;
        return;
    }
    if (t.channels > 2) flags |= RG_ST_MORE_CHANNELS;
    out->blocks = tot.blocks;
    out->active_blocks = tot.active;
    out->neg_blocks = tot.neg;
    out->mono_blocks = tot.mono;
    out->lag = tot.lag;
    out->anti_lag = tot.anti_lag;
    out->equal_frames = tot.equal;
    out->opposite_frames = tot.opposite;
    out->zero_frames = tot.zero;
    out->nonfinite = tot.nonfinite;
    out->ell = (int64_t)tot.ell;
    out->err = (int64_t)tot.err;
    out->elr = tot.elr;
    out->lag_sum = tot.lag_sum;
    out->anti_sum = tot.anti_sum;
    const double ell = (double)tot.ell, err = (double)tot.err;
    const double norm = sqrt(ell) * sqrt(err);
    const bool both = tot.ell > 0 && tot.err > 0;
    out->correlation = both ? (double)tot.elr / norm : 0.0;
    out->lag_correlation = both ? (double)tot.lag_sum / norm : 0.0;
    out->anti_correlation = both ? (double)tot.anti_sum / norm : 0.0;
    out->balance_db = ratio_db(ell, err);
    const __int128 sum = (__int128)tot.ell + (__int128)tot.err, twice = 2 * (__int128)tot.elr;
    const unsigned __int128 emm = (unsigned __int128)(sum + twice), ess = (unsigned __int128)(sum - twice);  // sums of squares: never negative
    out->side_db = ratio_db((double)ess, (double)emm);
    const uint64_t N = t.frames;
    const bool dual = N > 0 && tot.equal == N;
    if (tot.ell + tot.err == 0) flags |= RG_ST_SILENT;
    if (tot.nonfinite) flags |= RG_ST_NONFINITE;
    if (dual) flags |= RG_ST_DUAL_MONO;
    if (tot.opposite > 0 && tot.opposite + tot.zero == N) flags |= RG_ST_INVERTED_COPY;
    if (out->correlation <= -(double)o.phase_permille / 1000.0) flags |= RG_ST_OUT_OF_PHASE;
    if (!dual && out->side_db <= -(double)o.mono_db) flags |= RG_ST_NEAR_MONO;
    if (fabs(out->balance_db) >= (double)o.balance_db_limit || (tot.ell == 0) != (tot.err == 0)) flags |= RG_ST_ONE_SIDED;
    if (tot.lag != 0 && tot.lag_sum > tot.elr && out->lag_correlation >= (double)o.delay_permille / 1000.0) flags |= RG_ST_DELAYED;
    out->flags = flags;
}

int rg_st_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_stereo_opts *opts, const void *arena, size_t arena_bytes,
                     rg_stereo_result *out, int64_t *lag_sums, char *err, size_t err_len) {
    rg_stereo_opts o;
    int rc = rg_pcm_check_host_route("rg_stereo_arena", "folded", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_st_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgStTrack> tracks(n + 1);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_st_track(i, descs[i], o, false, arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    const uint32_t W = 2 * o.radius + 1;
    std::vector<int64_t> row(W);
    for (size_t i = 0; i < n; ++i) {
        int64_t *sums = lag_sums ? lag_sums + i * W : row.data();
        const RgStTotals tot = route == 0 ? rg_st_serial_host(base, tracks[i], o.radius, sums) : rg_st_folded_host(base, tracks[i], o.radius, sums);
        rg_st_fill(descs[i], o, tracks[i].block, 0, tot, &out[i]);
    }
    return RG_OK;
}

extern "C" int rg_stereo_kernel_shape(uint32_t format, uint32_t *piece_samples, uint32_t *tile_frames, uint32_t *strip_frames, uint32_t *lag_group,
                                      uint32_t *lds_bytes) {
    if (format != RG_FMT_F32_PLANAR && format != RG_FMT_S16_PLANAR && format != RG_FMT_S32_PLANAR) return RG_ERR_FORMAT;
    if (piece_samples) *piece_samples = rg_st_piece_samples(format);
    if (tile_frames) *tile_frames = RG_ST_TILE;
    if (strip_frames) *strip_frames = RG_ST_STRIP;
    if (lag_group) *lag_group = RG_ST_LAG_GROUP;
    if (lds_bytes) *lds_bytes = RG_ST_LDS_BYTES;
    return RG_OK;
}
