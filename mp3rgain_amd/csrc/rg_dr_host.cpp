// rg_dr_host.cpp -- the host side of the dynamic range scan (include/mp3rgain_amd_dr.h, rg_dr.h): the options, the plane
// records and their checks, the serial host twin (route 0: the definitions, written plainly, with a 128-bit sum and a sort),
// the kernels' cutting and fold arithmetic walked by the host (route 2: the same take, combine, block, pick and plane
// functions as rg_dr.hip runs), and the finish every route shares (the logarithms).  Plain C++: no device and no context, so
// a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#include "rg_dr.h"

int rg_dr_options(const rg_dr_opts *opts, rg_dr_opts *out, char *err, size_t err_len) {
    *out = opts ? *opts : rg_dr_opts{0u, RG_DR_TOP_PERMILLE};
    if (out->top_permille < 1 || out->top_permille > 1000) {
        snprintf(err, err_len, "dynamic range: top_permille %u is not in 1 .. 1000", out->top_permille);
        return RG_ERR_INVALID_ARG;
    }
    if (out->block_frames > RG_DR_MAX_BLOCK_FRAMES) {
        snprintf(err, err_len, "dynamic range: block_frames %u is more than %u", out->block_frames, RG_DR_MAX_BLOCK_FRAMES);
        return RG_ERR_INVALID_ARG;
    }
    return RG_OK;
}

int rg_dr_track_planes(size_t i, const rg_track_desc &t, const rg_dr_opts &o, bool rate_is_format, size_t arena_bytes, RgDrPlane *planes, char *err,
                       size_t err_len) {
    int rc = rg_pcm_check_format(i, t, RG_DR_MAX_CHANNELS, "the dynamic range takes", err, err_len);
    if (rc != RG_OK) return rc;
    const uint64_t block = o.block_frames ? o.block_frames : (uint64_t)3 * t.sample_rate;
    if (block < 1 || block > RG_DR_MAX_BLOCK_FRAMES) {
        snprintf(err, err_len, "track %zu: a block of %llu frames (sample rate %u) is not in 1 .. %u", i, (unsigned long long)block, t.sample_rate,
                 RG_DR_MAX_BLOCK_FRAMES);
        return rate_is_format && !o.block_frames ? RG_ERR_FORMAT : RG_ERR_INVALID_ARG;
    }
    rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    for (uint32_t c = 0; c < t.channels; ++c) {
        RgDrPlane &p = planes[c];
        memset(&p, 0, sizeof p);
        p.off = rg_pcm_plane_off(t, c);
        p.n = (uint32_t)t.frames;
        p.block = (uint32_t)block;
        p.n_blocks = (uint32_t)((t.frames + block - 1) / block);
        p.pieces_per_block = rg_dr_pieces_of(p.block, t.format);
        const uint64_t k = (uint64_t)p.n_blocks * o.top_permille / 1000;
        p.k = p.n_blocks ? (uint32_t)(k > 1 ? k : 1) : 0u;
        p.format = t.format;
    }
    return RG_OK;
}

uint64_t rg_dr_plan(RgDrPlane *planes, size_t n, uint64_t fmt_piece[4], uint64_t *n_blocks) {
    uint64_t pieces = 0, blocks = 0;
    for (uint32_t f = 0; f < 3; ++f) {
        fmt_piece[f] = pieces;
        for (size_t i = 0; i < n; ++i) {
            RgDrPlane &p = planes[i];
            if (p.format != f) continue;
            p.first_piece = pieces;
            p.first_block = blocks;
            pieces += rg_dr_plane_pieces(p);
            blocks += p.n_blocks;
        }
    }
    fmt_piece[3] = pieces;
    *n_blocks = blocks;
    return pieces;
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
RgDrPlaneOut rg_dr_serial_host(const unsigned char *arena, const RgDrPlane &p) {
    const unsigned char *plane = arena + p.off;
    const uint64_t N = p.n, B = p.block;
    const double s2 = rg_dr_scale2(p.format);
    RgDrPlaneOut o;
    memset(&o, 0, sizeof o);
    if (!N) return o;
    std::vector<double> ms, e;
    std::vector<uint32_t> peaks;
    for (uint64_t at = 0; at < N; at += B) {
        const uint64_t n = std::min(B, N - at);
        unsigned __int128 E = 0;
        uint64_t peak = 0;
        for (uint64_t j = at; j < at + n; ++j) {
            const uint32_t raw = rg_pcm_raw_at(plane, p.format, j);
            int64_t q;
            if (p.format == RG_FMT_F32_PLANAR) {
                float x;
                memcpy(&x, &raw, 4);
                if (!std::isfinite(x)) {
                    ++o.nonfinite;
                    q = 0;
                } else {
                    const double xd = x;
                    q = llrint((xd < -256.0 ? -256.0 : (xd > 256.0 ? 256.0 : xd)) * 8388608.0);
                }
            } else {
                q = (int32_t)raw;
            }
            const uint64_t a = (uint64_t)(q < 0 ? -q : q);
            E += (unsigned __int128)a * a;
            peak = std::max(peak, a);
        }
        const double ei = (double)(uint64_t)(E >> 32) * 4294967296.0 + (double)(uint64_t)(E & 0xFFFFFFFFu);
        e.push_back(ei);
        ms.push_back(2.0 * ei / ((double)n * s2));
        peaks.push_back((uint32_t)peak);
    }
    const size_t blocks = ms.size();
    const size_t k = p.k;  // max(1, floor(blocks * top_permille / 1000)): rg_dr_track_planes
    std::vector<double> sorted(ms);
    std::sort(sorted.begin(), sorted.end(), std::greater<double>());
    const double t = sorted[k - 1];
    size_t g = 0;
    double S = 0.0, esum = 0.0;
    for (size_t b = 0; b < blocks; ++b) {
        if (ms[b] > t) {
            S += ms[b];
            ++g;
        }
        esum += e[b];
    }
    for (size_t j = g; j < k; ++j) S += t;
    std::vector<uint32_t> ps(peaks);
    std::sort(ps.begin(), ps.end(), std::greater<uint32_t>());
    o.top_ms = S / (double)k;
    o.mean_square = 2.0 * esum / ((double)N * s2);
    o.peak = ps[0];
    o.peak2 = ps.size() > 1 ? ps[1] : ps[0];
    o.blocks = (uint32_t)blocks;
    o.top_blocks = (uint32_t)k;
    return o;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
template <int FMT>
static RgDrPiece piece_sums(const unsigned char *plane, uint64_t first, uint32_t n) {
    RgDrPiece acc = rg_dr_empty();
    for (uint32_t j = 0; j < n; ++j) rg_dr_take<FMT>(rg_pcm_raw_at(plane, FMT, first + j), &acc);
    return acc;
}

RgDrPlaneOut rg_dr_folded_host(const unsigned char *arena, const RgDrPlane &p) {
    const unsigned char *plane = arena + p.off;
    std::vector<RgDrBlock> blocks(p.n_blocks);
    uint32_t nonfinite = 0;
    for (uint32_t b = 0; b < p.n_blocks; ++b) {  // the reading kernel, one workgroup per piece, and the fold's first step
        uint64_t bstart;
        const uint32_t len = rg_dr_block_window(p, b, &bstart);
        RgDrPiece acc = rg_dr_empty();
        for (uint32_t k = 0; k < rg_dr_pieces_of(len, p.format); ++k) {
            uint32_t pstart;
            const uint32_t plen = rg_dr_piece_window(len, k, p.format, &pstart);
            const uint64_t first = bstart + pstart;
            rg_dr_combine(&acc, p.format == RG_FMT_F32_PLANAR   ? piece_sums<RG_FMT_F32_PLANAR>(plane, first, plen)
                                : p.format == RG_FMT_S16_PLANAR ? piece_sums<RG_FMT_S16_PLANAR>(plane, first, plen)
                                                                : piece_sums<RG_FMT_S32_PLANAR>(plane, first, plen));
        }
        blocks[b] = rg_dr_block(acc, len, p.format);
        nonfinite += acc.nonfinite;
    }
    // the radix select: the k-th largest pattern, a digit a pass
    uint64_t prefix = 0;
    uint32_t above = 0;
    if (p.n_blocks)
        for (uint32_t pass = 0; pass < RG_DR_PASSES; ++pass) {
            uint32_t hist[RG_DR_BINS] = {0};
            for (uint32_t b = 0; b < p.n_blocks; ++b) {
                const uint64_t key = rg_dr_key(blocks[b].ms);
                if (rg_dr_in_prefix(key, prefix, pass)) ++hist[rg_dr_digit(key, pass)];
            }
            uint32_t more;
            const uint32_t d = rg_dr_pick(hist, p.k - above, &more);
            above += more;
            prefix = (prefix << RG_DR_RADIX_BITS) | d;
        }
    return rg_dr_plane([&](uint32_t b) { return blocks[b]; }, p, rg_dr_unkey(prefix), above, nonfinite);
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
static double db_or_floor(double factor, double x) { return x > 0.0 ? factor * log10(x) : -INFINITY; }

void rg_dr_fill(const rg_track_desc &t, uint32_t block, uint32_t dropped_frames, const RgDrPlaneOut *po, rg_dr_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->frames = t.frames;
    out->sample_rate = t.sample_rate;
    out->channels = t.channels;
    out->format = t.format;
    out->dropped_frames = dropped_frames;
    out->block_frames = block;
    const double s = rg_dr_scale(t.format);
    uint32_t flags = dropped_frames == 0 ? RG_DR_COMPLETE : 0u;
    bool sounding = false;
    double dr_sum = 0.0, ms_sum = 0.0, peak_db = -INFINITY;
    for (uint32_t c = 0; c < t.channels; ++c) {
        rg_dr_channel &ch = out->ch[c];
        const RgDrPlaneOut &p = po[c];
        ch.top_ms = p.top_ms;
        ch.mean_square = p.mean_square;
        ch.peak = p.peak;
        ch.peak2 = p.peak2;
        ch.blocks = p.blocks;
        ch.top_blocks = p.top_blocks;
        ch.nonfinite = p.nonfinite;
        const bool has = p.peak2 > 0 && p.top_ms > 0.0;
        ch.dr = has ? 20.0 * log10(((double)p.peak2 / s) / sqrt(p.top_ms)) : 0.0;
        ch.peak_db = db_or_floor(20.0, (double)p.peak / s);
        ch.rms_db = db_or_floor(10.0, p.mean_square);
        sounding = sounding || has;
        if (p.nonfinite) flags |= RG_DR_NONFINITE;
        dr_sum += ch.dr;
        ms_sum += p.mean_square;
        peak_db = ch.peak_db > peak_db ? ch.peak_db : peak_db;
    }
    if (!sounding || !t.frames) flags |= RG_DR_SILENT;
    if (t.frames < block) flags |= RG_DR_SHORT;
    out->dr_mean = dr_sum / (double)t.channels;
    out->dr = (int32_t)llrint(out->dr_mean);
    out->peak_db = peak_db;
    out->rms_db = db_or_floor(10.0, ms_sum / (double)t.channels);
    out->flags = flags;
}

int rg_dr_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_dr_opts *opts, const void *arena, size_t arena_bytes, rg_dr_result *out,
                     char *err, size_t err_len) {
    rg_dr_opts o;
    int rc = rg_pcm_check_host_route("rg_dr_arena", "folded", route, n, descs, out, arena, arena_bytes, err, err_len);
    if (rc == RG_OK) rc = rg_dr_options(opts, &o, err, err_len);
    if (rc != RG_OK) return rc;
    std::vector<RgDrPlane> planes(n * RG_DR_MAX_CHANNELS + 1);
    size_t n_planes = 0;
    for (size_t i = 0; i < n; ++i) {
        rc = rg_dr_track_planes(i, descs[i], o, false, arena_bytes, &planes[n_planes], err, err_len);
        if (rc != RG_OK) return rc;
        n_planes += descs[i].channels;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        RgDrPlaneOut po[RG_DR_MAX_CHANNELS];
        for (uint32_t c = 0; c < descs[i].channels; ++c) po[c] = route == 0 ? rg_dr_serial_host(base, planes[at + c]) : rg_dr_folded_host(base, planes[at + c]);
        rg_dr_fill(descs[i], planes[at].block, 0, po, &out[i]);
        at += descs[i].channels;
    }
    return RG_OK;
}

extern "C" int rg_dr_kernel_shape(uint32_t format, uint32_t *step_samples, uint32_t *piece_samples, uint32_t *fold_lanes, uint32_t *select_bins) {
    if (format != RG_FMT_F32_PLANAR && format != RG_FMT_S16_PLANAR && format != RG_FMT_S32_PLANAR) return RG_ERR_FORMAT;
    if (step_samples) *step_samples = rg_dr_step_samples(format);
    if (piece_samples) *piece_samples = rg_dr_piece_samples(format);
    if (fold_lanes) *fold_lanes = RG_DR_FOLD_LANES;
    if (select_bins) *select_bins = RG_DR_BINS;
    return RG_OK;
}
