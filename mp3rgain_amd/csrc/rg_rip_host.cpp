// rg_rip_host.cpp -- the host side of the rip checksums (include/mp3rgain_amd_rip.h, rg_rip.h): the track records and their
// checks, the serial host twin (route 0: the definitions, written plainly), and the kernels' fold arithmetic walked by the
// host (route 2: the same chunk, combine and finish functions as rg_rip_crc.hip runs, lane by lane); and of the signatures at
// every drive offset: the disc's records, the definition (route 0) and arv1's sliding recurrence (route 2).  Plain C++: no
// device and no context, so a sanitizer build needs nothing else.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rg_rip.h"

int rg_rip_track_record(size_t i, const rg_track_desc &t, uint32_t flags, size_t arena_bytes, RgRipTrack *out, char *err, size_t err_len) {
    if (t.format != RG_FMT_S16_PLANAR) {
        snprintf(err, err_len, "track %zu: format %u is not 16-bit planar PCM", i, (unsigned)t.format);
        return RG_ERR_FORMAT;
    }
    if (t.channels != 2) {
        snprintf(err, err_len, "track %zu: %u channel(s), rip checksums take 2", i, (unsigned)t.channels);
        return RG_ERR_FORMAT;
    }
    if (t.frames >= ((uint64_t)1 << 32)) {
        snprintf(err, err_len, "track %zu: %llu frames, rip checksums take fewer than 2^32", i, (unsigned long long)t.frames);
        return RG_ERR_FORMAT;
    }
    if (t.offset_bytes % 2) {
        snprintf(err, err_len, "track %zu: offset %llu is not sample-aligned", i, (unsigned long long)t.offset_bytes);
        return RG_ERR_INVALID_ARG;
    }
    if (t.offset_bytes > arena_bytes || t.frames > (arena_bytes - t.offset_bytes) / 4) {
        snprintf(err, err_len, "track %zu: its planes reach beyond the arena (%zu bytes)", i, arena_bytes);
        return RG_ERR_INVALID_ARG;
    }
    memset(out, 0, sizeof *out);
    out->off = t.offset_bytes;
    out->frames = t.frames;
    out->from = (flags & RG_RIP_FIRST_TRACK) ? RG_RIP_AR_SKIP : 0u;
    out->to = (flags & RG_RIP_LAST_TRACK) ? (int64_t)t.frames - (int64_t)RG_RIP_AR_SKIP : (int64_t)t.frames;
    out->run = 1;
    return RG_OK;
}

uint64_t rg_rip_plan(RgRipTrack *recs, size_t n) {
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        RgRipTrack &r = recs[i];
        r.first_tile = tiles;
        r.n_tiles = (uint32_t)((r.frames + RG_RIP_TILE - 1) / RG_RIP_TILE);
        r.run = r.n_tiles ? (r.n_tiles + RG_RIP_FOLD_LANES - 1) / RG_RIP_FOLD_LANES : 1;
        for (uint32_t j = 0; j < RG_RIP_FOLD_LEVELS; ++j) r.pw[j] = rg_crc32_x8n(((uint64_t)RG_RIP_TILE_BYTES * r.run) << j);
        tiles += r.n_tiles;
    }
    return tiles;
}

RgRipPowers rg_rip_powers() {
    RgRipPowers P;
    for (uint32_t j = 0; j < RG_RIP_LEVELS; ++j) P.pw[j] = rg_crc32_x8n((uint64_t)RG_RIP_CHUNK_BYTES << j);
    P.x_tile = rg_crc32_x8n(RG_RIP_TILE_BYTES);
    uint32_t sq = RG_CRC32_X8;
    for (uint32_t j = 0; j < RG_CRC32_X2_ENTRIES; ++j) {
        P.x2[j] = sq;
        sq = rg_crc32_mul(sq, sq);
    }
    return P;
}

static inline uint32_t sample_at(const unsigned char *plane, uint64_t k) {  // planes are only sample-aligned
    uint16_t s;
    memcpy(&s, plane + 2 * k, 2);
    return s;
}

// ---- route 0: the definitions ------------------------------------------------------------------------------------------------
RgRipSums rg_rip_serial_host(const unsigned char *arena, const RgRipTrack &r) {
    const unsigned char *L = arena + r.off, *R = L + 2 * r.frames;
    const uint32_t *t = kRgCrc32.t;
    uint32_t crc = 0xFFFFFFFFu, nn = 0xFFFFFFFFu, arv1 = 0, arv2 = 0;
    uint64_t zeros = 0;
    for (uint64_t k = 0; k < r.frames; ++k) {
        const uint32_t s[2] = {sample_at(L, k), sample_at(R, k)};
        for (int c = 0; c < 2; ++c) {
            crc = rg_crc32_u16(crc, s[c], t);
            if (s[c]) nn = rg_crc32_u16(nn, s[c], t);
            else ++zeros;
        }
        const uint64_t i = k + 1;
        if (i >= r.from && (int64_t)i <= r.to) {
            const uint64_t p = (uint64_t)(s[0] | (s[1] << 16)) * i;
            arv1 += (uint32_t)p;
            arv2 += (uint32_t)p + (uint32_t)(p >> 32);
        }
    }
    RgRipSums out;
    out.null_samples = zeros;
    out.crc32 = r.frames ? ~crc : 0u;
    out.crc32_nonnull = zeros < 2 * r.frames ? ~nn : 0u;
    out.arv1 = arv1;
    out.arv2 = arv2;
    return out;
}

// ---- route 2: the kernels' arithmetic ---------------------------------------------------------------------------------------
// v[0] <- the fold of v[0 .. lanes) in order, level j multiplying by pw[j]: the tree both kernels run over LDS
static void tree(RgRipPart *v, uint32_t levels, const uint32_t *pw, const uint32_t *x2) {
    for (uint32_t j = 0; j < levels; ++j) {
        const uint32_t s = 1u << j;
        for (uint32_t at = 0; at < (1u << levels); at += 2 * s) rg_rip_combine(&v[at], v[at + s], pw[j], x2);
    }
}

RgRipSums rg_rip_folded_host(const unsigned char *arena, const RgRipTrack &r, const RgRipPowers &P) {
    const unsigned char *L = arena + r.off, *R = L + 2 * r.frames;
    std::vector<RgRipPart> tiles(r.n_tiles ? r.n_tiles : 1), v(RG_RIP_BLOCK);
    for (uint32_t t = 0; t < r.n_tiles; ++t) {  // the tile kernel: one block each
        uint64_t wstart;
        const uint32_t wlen = rg_rip_tile_window(r.frames, r.n_tiles, t, &wstart);
        for (uint32_t lane = 0; lane < RG_RIP_BLOCK; ++lane) {
            uint32_t a;
            const uint32_t n = rg_rip_lane_chunk(wlen, lane, &a);
            const uint64_t k0 = wstart + a;
            rg_rip_chunk<false>([&](uint32_t p, uint32_t j) { return sample_at(p ? R : L, k0 + j); }, k0, n, r.from, r.to, kRgCrc32.t, &v[lane]);
        }
        tree(v.data(), RG_RIP_LEVELS, P.pw, P.x2);
        tiles[t] = v[0];
    }
    // the fold kernel: one block per track
    for (uint32_t lane = 0; lane < RG_RIP_FOLD_LANES; ++lane) {
        int64_t lo;
        const int64_t hi = rg_rip_lane_run(r.n_tiles, r.run, lane, &lo);
        RgRipPart acc = rg_rip_empty();
        for (int64_t t = lo; t < hi; ++t) rg_rip_combine(&acc, tiles[(size_t)t], P.x_tile, P.x2);
        v[lane] = acc;
    }
    tree(v.data(), RG_RIP_FOLD_LEVELS, r.pw, P.x2);
    return rg_rip_finish(v[0], r.frames, P.x2);
}

void rg_rip_fill(const RgRipSums &s, uint64_t frames, uint32_t sample_rate, uint32_t dropped_frames, rg_rip_result *out) {
    memset(out, 0, sizeof *out);
    out->status = RG_OK;
    out->flags = (sample_rate == 44100 ? RG_RIP_CD_RATE : 0u) | (frames % 588 == 0 ? RG_RIP_CD_FRAMES : 0u) | (dropped_frames == 0 ? RG_RIP_COMPLETE : 0u);
    out->frames = frames;
    out->null_samples = s.null_samples;
    out->sample_rate = sample_rate;
    out->dropped_frames = dropped_frames;
    out->crc32 = s.crc32;
    out->crc32_nonnull = s.crc32_nonnull;
    out->arv1 = s.arv1;
    out->arv2 = s.arv2;
}

int rg_rip_arena_host(int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, const void *arena, size_t arena_bytes,
                      rg_rip_result *out, char *err, size_t err_len) {
    if (route != 0 && route != 2) {
        snprintf(err, err_len, "rg_rip_checksums_arena: route %d is not a host route (0 = serial twin, 2 = folded)", route);
        return RG_ERR_INVALID_ARG;
    }
    if (n && (!descs || !out || (arena_bytes && !arena))) {
        snprintf(err, err_len, "rg_rip_checksums_arena: null array");
        return RG_ERR_INVALID_ARG;
    }
    std::vector<RgRipTrack> recs(n ? n : 1);
    for (size_t i = 0; i < n; ++i) {
        const int rc = rg_rip_track_record(i, descs[i], track_flags ? track_flags[i] : 0u, arena_bytes, &recs[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    const unsigned char *base = static_cast<const unsigned char *>(arena);
    RgRipPowers P{};
    if (route == 2) {
        (void)rg_rip_plan(recs.data(), n);
        P = rg_rip_powers();
    }
    for (size_t i = 0; i < n; ++i)
        rg_rip_fill(route == 0 ? rg_rip_serial_host(base, recs[i]) : rg_rip_folded_host(base, recs[i], P), descs[i].frames, descs[i].sample_rate, 0, &out[i]);
    return RG_OK;
}

// ---- the signatures at every drive offset ----------------------------------------------------------------------------------
void rg_rip_disc(const RgRipTrack *recs, size_t n, RgRipDiscTrack *out) {
    uint64_t base = 0;
    for (size_t t = 0; t <= n; ++t) {
        memset(&out[t], 0, sizeof out[t]);
        out[t].base = base;
        if (t == n) break;  // the disc's end
        out[t].off = recs[t].off;
        out[t].frames = recs[t].frames;
        out[t].from = recs[t].from;
        out[t].to = recs[t].to;
        base += recs[t].frames;
    }
}

void rg_rip_offsets_plan(const RgRipDiscTrack *tr, size_t n, std::vector<RgRipOffTile> *tiles) {
    tiles->clear();
    for (size_t t = 0; t < n; ++t) {
        const int64_t k_lo = tr[t].from > 1u ? (int64_t)tr[t].from - 1 : 0, k_hi = tr[t].to;  // frames [k_lo, k_hi) count
        for (int64_t k0 = k_lo / RG_RIP_OFF_TILE * RG_RIP_OFF_TILE; k0 < k_hi; k0 += RG_RIP_OFF_TILE)
            tiles->push_back(RgRipOffTile{(uint32_t)t, (uint32_t)k0});
    }
}

void rg_rip_disc_words(const unsigned char *arena, const RgRipDiscTrack *tr, size_t n, std::vector<uint32_t> *W) {
    W->resize((size_t)tr[n].base);
    for (size_t t = 0; t < n; ++t) {
        const unsigned char *L = arena + tr[t].off, *R = L + 2 * tr[t].frames;
        for (uint64_t k = 0; k < tr[t].frames; ++k) (*W)[(size_t)(tr[t].base + k)] = sample_at(L, k) | (sample_at(R, k) << 16);
    }
}

// ---- route 0: the definition -----------------------------------------------------------------------------------------------
void rg_rip_offsets_cell(const std::vector<uint32_t> &W, const RgRipDiscTrack &t, int32_t o, uint32_t *v1, uint32_t *v2) {
    const int64_t total = (int64_t)W.size();
    uint32_t lo = 0, hi = 0;
    for (int64_t i = t.from > 1u ? t.from : 1; i <= t.to; ++i) {  // positions are 1-based
        const int64_t j = (int64_t)t.base + i - 1 + o;
        const uint32_t w = j >= 0 && j < total ? W[(size_t)j] : 0u;
        rg_rip_off_product(w, (uint32_t)i, &lo, &hi);
    }
    *v1 = lo;
    *v2 = lo + hi;
}

// ---- route 2: arv1 by the sliding recurrence ----------------------------------------------------------------------------------
static void offsets_sliding(const std::vector<uint32_t> &W, const RgRipDiscTrack &t, int32_t radius, uint32_t *v1) {
    const int64_t total = (int64_t)W.size(), f = t.from > 1u ? t.from : 1, T = t.to, c = (int64_t)t.base - 1;
    const auto w = [&](int64_t j) -> uint32_t { return j >= 0 && j < total ? W[(size_t)j] : 0u; };
    if (T < f) {
        for (int32_t o = -radius; o <= radius; ++o) v1[o + radius] = 0;
        return;
    }
    uint32_t A = 0, S = 0;  // A(-radius) and S(-radius) = sum of W[c + i - radius] over i = f + 1 .. T + 1, both mod 2^32
    for (int64_t i = f; i <= T; ++i) A += w(c + i - radius) * (uint32_t)i;
    for (int64_t i = f + 1; i <= T + 1; ++i) S += w(c + i - radius);
    for (int32_t o = -radius;; ++o) {
        v1[o + radius] = A;
        if (o == radius) break;
        A = A - (uint32_t)f * w(c + f + o) + (uint32_t)(T + 1) * w(c + T + 1 + o) - S;
        S = S - w(c + f + 1 + o) + w(c + T + 2 + o);
    }
}

int rg_rip_offsets_check(int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, int32_t radius, const void *arena,
                         size_t arena_bytes, const uint32_t *arv2, std::vector<RgRipDiscTrack> *recs, char *err, size_t err_len) {
    if (route < 0 || route > 2) {
        snprintf(err, err_len, "rg_rip_offsets_arena: route %d (0 = the definition, 1 = kernel, 2 = arv1 by the sliding recurrence)", route);
        return RG_ERR_INVALID_ARG;
    }
    if (route == 2 && arv2) {
        snprintf(err, err_len, "rg_rip_offsets_arena: route 2 computes arv1 only");
        return RG_ERR_INVALID_ARG;
    }
    if (radius < 0 || radius > RG_RIP_OFFSET_MAX) {
        snprintf(err, err_len, "rg_rip_offsets_arena: radius %d is outside 0..%d", (int)radius, RG_RIP_OFFSET_MAX);
        return RG_ERR_INVALID_ARG;
    }
    if (n > RG_RIP_DISC_MAX_TRACKS) {
        snprintf(err, err_len, "rg_rip_offsets_arena: %zu tracks, a disc has at most %u", n, RG_RIP_DISC_MAX_TRACKS);
        return RG_ERR_INVALID_ARG;
    }
    if (n && (!descs || (arena_bytes && !arena))) {
        snprintf(err, err_len, "rg_rip_offsets_arena: null array");
        return RG_ERR_INVALID_ARG;
    }
    std::vector<RgRipTrack> tracks(n ? n : 1);
    for (size_t i = 0; i < n; ++i) {
        const int rc = rg_rip_track_record(i, descs[i], track_flags ? track_flags[i] : 0u, arena_bytes, &tracks[i], err, err_len);
        if (rc != RG_OK) return rc;
    }
    recs->resize(n + 1);
    rg_rip_disc(tracks.data(), n, recs->data());
    return RG_OK;
}

int rg_rip_offsets_host(int route, const std::vector<RgRipDiscTrack> &recs, int32_t radius, const void *arena, uint32_t *arv1, uint32_t *arv2) {
    const size_t n = recs.size() - 1, n_off = 2 * (size_t)radius + 1;
    std::vector<uint32_t> W;
    rg_rip_disc_words(static_cast<const unsigned char *>(arena), recs.data(), n, &W);
    for (size_t t = 0; t < n; ++t) {
        if (route == 2) {
            if (arv1) offsets_sliding(W, recs[t], radius, arv1 + t * n_off);
            continue;
        }
        for (int32_t o = -radius; o <= radius; ++o) {
            uint32_t v1, v2;
            rg_rip_offsets_cell(W, recs[t], o, &v1, &v2);
            if (arv1) arv1[t * n_off + (size_t)(o + radius)] = v1;
            if (arv2) arv2[t * n_off + (size_t)(o + radius)] = v2;
        }
    }
    return RG_OK;
}

extern "C" int rg_rip_offsets_kernel_shape(uint32_t *tile_frames, uint32_t *block_lanes) {
    if (tile_frames) *tile_frames = RG_RIP_OFF_TILE;
    if (block_lanes) *block_lanes = RG_RIP_OFF_BLOCK;
    return RG_OK;
}

extern "C" int rg_rip_kernel_shape(uint32_t *chunk_frames, uint32_t *tile_frames, uint32_t *fold_lanes) {
    if (chunk_frames) *chunk_frames = RG_RIP_CHUNK;
    if (tile_frames) *tile_frames = RG_RIP_TILE;
    if (fold_lanes) *fold_lanes = RG_RIP_FOLD_LANES;
    return RG_OK;
}

extern "C" int rg_rip_crc32_algebra(uint32_t a, uint32_t b, uint64_t n, uint32_t *product, uint32_t *power) {
    if (product) *product = rg_crc32_mul(a, b);
    if (power) *power = rg_crc32_x8n(n);
    return RG_OK;
}
