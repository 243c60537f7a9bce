// rg_rip.h -- internal: the rip checksums (include/mp3rgain_amd_rip.h) as rg_rip_crc.hip (kernels, launcher, seams),
// rg_rip_host.cpp (the serial host twin and the kernels' fold arithmetic on the host) and rg_file_verify.hip (rg_rip_checksums)
// share them.  What one lane hashes, how two neighbours fold and how a track is finished is host and device code, written
// once here; the kernels and the folded host route differ only in who walks the lanes.  The signatures at every drive offset
// (rg_rip_offsets.hip, rg_rip_offset_signatures) share the disc's records, the tile table and the product further down.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mp3rgain_amd_rip.h"
#include "rg_crc32.h"

// ---- how a track is cut --------------------------------------------------------------------------------------------------
#define RG_RIP_CHUNK 32u                              // C: frames one lane hashes (128 interleaved bytes)
#define RG_RIP_BLOCK 256u                             // lanes of a tile block = chunks of a tile
#define RG_RIP_LEVELS 8                               // log2(RG_RIP_BLOCK)
#define RG_RIP_TILE (RG_RIP_CHUNK * RG_RIP_BLOCK)     // T: frames of a tile
#define RG_RIP_FOLD_LANES 64u                         // F: lanes of the fold kernel (one wave per track)
#define RG_RIP_FOLD_LEVELS 6                          // log2(RG_RIP_FOLD_LANES)
#define RG_RIP_CHUNK_BYTES (4u * RG_RIP_CHUNK)        // of the plain CRC's message
#define RG_RIP_TILE_BYTES (4u * RG_RIP_TILE)

// What a stretch of a track comes to: a lane's chunk, a subtree, a tile, a run of tiles.  Both CRCs are raw registers.
struct RgRipPart {
    uint32_t crc;      // of the 4 bytes of every frame
    uint32_t nn_crc;   // of the 2 bytes of every non-null sample ...
    uint32_t lo, hi;   // sums of lo32(p), hi32(p) over the positions that count
    uint64_t nn_len;   // ... which are this many bytes
    uint64_t zeros;    // null samples
};  // 32 bytes

// One track of a launch
struct RgRipTrack {
    uint64_t off;         // of plane L from the arena's base, in bytes; plane R follows at off + 2 * frames
    uint64_t frames;      // N < 2^32
    uint64_t first_tile;  // of this track among the launch's tiles
    int64_t to;           // positions from..to count (1-based, inclusive; empty when to < from)
    uint32_t from;
    uint32_t n_tiles;
    uint32_t run;         // tile records one lane of the fold kernel folds (>= 1)
    uint32_t reserved;
    uint32_t pw[RG_RIP_FOLD_LEVELS];  // x^(8 TILE_BYTES run 2^j)
    uint32_t reserved2[2];
};  // 80 bytes
struct RgRipPowers {
    uint32_t pw[RG_RIP_LEVELS];        // x^(8 CHUNK_BYTES 2^j)
    uint32_t x_tile;                   // x^(8 TILE_BYTES)
    uint32_t x2[RG_CRC32_X2_ENTRIES];  // x^(8 2^j)
};
// what the fold kernel writes per track
struct RgRipSums {
    uint64_t null_samples;
    uint32_t crc32, crc32_nonnull, arv1, arv2;
};  // 24 bytes

// ---- one lane's chunk -----------------------------------------------------------------------------------------------------
// Frames k0 .. k0 + n - 1 of a track (k0 counted from the track's first frame), sample j of plane p of the chunk = get(p, j)
// as a uint16.  `t`: the byte table; with SLICE4 tables 1..3 of slice-by-4 lie behind it.
template <bool SLICE4, class Get>
RG_CRC32_HD void rg_rip_chunk(Get get, uint64_t k0, uint32_t n, uint32_t from, int64_t to, const uint32_t *t, RgRipPart *out) {
    uint32_t crc = 0, nn = 0, lo = 0, hi = 0, nn_len = 0, zeros = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t l = get(0u, j), r = get(1u, j);
        const uint32_t v = l | (r << 16);
        crc = SLICE4 ? rg_crc32_u32_slice4(crc, v, t) : rg_crc32_u32(crc, v, t);
        if (l) {
            nn = rg_crc32_u16(nn, l, t);
            nn_len += 2;
        } else {
            ++zeros;
        }
        if (r) {
            nn = rg_crc32_u16(nn, r, t);
            nn_len += 2;
        } else {
            ++zeros;
        }
        const uint64_t i = k0 + j + 1;  // <= N < 2^32
        if (i >= from && (int64_t)i <= to) {
            const uint64_t p = (uint64_t)v * i;
            lo += (uint32_t)p;
            hi += (uint32_t)(p >> 32);
        }
    }
    out->crc = crc;
    out->nn_crc = nn;
    out->lo = lo;
    out->hi = hi;
    out->nn_len = nn_len;
    out->zeros = zeros;
}

// ---- folding ---------------------------------------------------------------------------------------------------------------
// a <- a || b.  The plain CRC's stretches are counted from the track's end, so b is always full and `pw_b` = x^(8 len b) is
// one constant per level; the non-null message's lengths are the data's, and its power comes from the table x2.
RG_CRC32_HD void rg_rip_combine(RgRipPart *a, const RgRipPart &b, uint32_t pw_b, const uint32_t *x2) {
    a->crc = (a->crc ? rg_crc32_mul(a->crc, pw_b) : 0u) ^ b.crc;
    a->nn_crc = (a->nn_crc && b.nn_len ? rg_crc32_mul(a->nn_crc, rg_crc32_x8n_tab(b.nn_len, x2)) : a->nn_crc) ^ b.nn_crc;
    a->nn_len += b.nn_len;
    a->zeros += b.zeros;
    a->lo += b.lo;
    a->hi += b.hi;
}
RG_CRC32_HD RgRipPart rg_rip_empty() { return RgRipPart{0u, 0u, 0u, 0u, 0u, 0u}; }

// the window of tile `t` of a track of `frames` frames in `n_tiles` tiles, counted from the track's end: [*start, *start + return)
RG_CRC32_HD uint32_t rg_rip_tile_window(uint64_t frames, uint32_t n_tiles, uint64_t t, uint64_t *start) {
    const uint64_t wend = frames - (uint64_t)(n_tiles - 1 - t) * RG_RIP_TILE;
    *start = wend > RG_RIP_TILE ? wend - RG_RIP_TILE : 0;
    return (uint32_t)(wend - *start);
}
// lane `lane`'s chunk of a window of `wlen` frames: [*start, *start + return) of the window; it ends (255 - lane) chunks
// before the window's end
RG_CRC32_HD uint32_t rg_rip_lane_chunk(uint32_t wlen, uint32_t lane, uint32_t *start) {
    const int64_t e = (int64_t)wlen - (int64_t)(RG_RIP_BLOCK - 1 - lane) * RG_RIP_CHUNK;
    if (e <= 0) {
        *start = 0;
        return 0;
    }
    *start = (uint32_t)(e > (int64_t)RG_RIP_CHUNK ? e - RG_RIP_CHUNK : 0);
    return (uint32_t)e - *start;
}
// lane `lane` of the fold kernel folds tile records [*lo, return) of its track: the run that ends (F - 1 - lane) runs before
// the last tile
RG_CRC32_HD int64_t rg_rip_lane_run(uint32_t n_tiles, uint32_t run, uint32_t lane, int64_t *lo) {
    const int64_t hi = (int64_t)n_tiles - (int64_t)(RG_RIP_FOLD_LANES - 1 - lane) * run;
    *lo = hi - run < 0 ? 0 : hi - run;
    return hi;
}

// the track's numbers from the fold of all of it: the initial value and the final XOR of both CRCs are applied here, once
RG_CRC32_HD RgRipSums rg_rip_finish(const RgRipPart &all, uint64_t frames, const uint32_t *x2) {
    RgRipSums s;
    s.null_samples = all.zeros;
    s.crc32 = rg_crc32_finish(all.crc, 4 * frames, rg_crc32_x8n_tab(4 * frames, x2));
    s.crc32_nonnull = rg_crc32_finish(all.nn_crc, all.nn_len, rg_crc32_x8n_tab(all.nn_len, x2));
    s.arv1 = all.lo;
    s.arv2 = all.lo + all.hi;
    return s;
}

// ---- rg_rip_host.cpp (plain C++: no device, no context) -----------------------------------------------------------------
// The record of track i, described by `t` with the input flags `flags`, in an arena of `arena_bytes` bytes.  RG_ERR_FORMAT
// unless it is 2 channels of S16 planar of fewer than 2^32 frames, RG_ERR_INVALID_ARG unless both planes lie inside the
// arena, sample-aligned; the text goes to err[err_len].  first_tile, n_tiles, run and pw are rg_rip_plan's to set.
int rg_rip_track_record(size_t i, const rg_track_desc &t, uint32_t flags, size_t arena_bytes, RgRipTrack *out, char *err, size_t err_len);
// tiles, runs and powers of the `n` tracks of a launch; returns the number of tiles
uint64_t rg_rip_plan(RgRipTrack *recs, size_t n);
RgRipPowers rg_rip_powers();
// one track's numbers from host memory: the definitions, serially ...
RgRipSums rg_rip_serial_host(const unsigned char *arena, const RgRipTrack &r);
// ... and as the kernels compute them: chunks, trees, tile records, runs, the fix-up (`r` has been through rg_rip_plan)
RgRipSums rg_rip_folded_host(const unsigned char *arena, const RgRipTrack &r, const RgRipPowers &P);
// the result record of a track that was hashed
void rg_rip_fill(const RgRipSums &s, uint64_t frames, uint32_t sample_rate, uint32_t dropped_frames, rg_rip_result *out);
// routes 0 and 2 of rg_rip_checksums_arena
int rg_rip_arena_host(int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, const void *arena, size_t arena_bytes,
                      rg_rip_result *out, char *err, size_t err_len);

// ---- the signatures at every drive offset (rg_rip_offsets.hip, rg_rip_host.cpp) -------------------------------------------
#define RG_RIP_OFF_TILE 4096u   // T: frames of a track one block takes
#define RG_RIP_OFF_BLOCK 256u   // lanes of a block
#define RG_RIP_OFF_J 23u        // consecutive offsets one lane holds in registers: BLOCK * J = 5888 >= 2 * 2939 + 1
#define RG_RIP_OFF_SPAN (RG_RIP_OFF_BLOCK * RG_RIP_OFF_J)
#define RG_RIP_OFF_LDS (RG_RIP_OFF_TILE + RG_RIP_OFF_SPAN)  // disc words of a block: 9984 (39 936 bytes, four blocks a CU)

// One track of a disc.  A launch has n + 1 of them: entry n is the disc's end (base = the disc's length, frames = 0).
struct RgRipDiscTrack {
    uint64_t off;     // of plane L from the arena's base, in bytes; plane R follows at off + 2 * frames
    uint64_t frames;  // N < 2^32
    uint64_t base;    // B: disc position of the track's first frame
    int64_t to;       // positions from..to count (1-based, inclusive; empty when to < from)
    uint32_t from;
    uint32_t reserved;
};  // 40 bytes
// One block's work: frames k0 .. k0 + T - 1 of track `track` (those of them that count)
struct RgRipOffTile {
    uint32_t track, k0;
};

// the track that holds disc position pos (0 <= pos < tr[n].base): the last u with tr[u].base <= pos, which is never empty
RG_CRC32_HD uint32_t rg_rip_disc_find(const RgRipDiscTrack *tr, uint32_t n, uint64_t pos) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (tr[mid].base <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// one product into the two sums, of lo32(p) and of hi32(p): they cannot be one 64-bit sum (its high word would hold lo's carries)
RG_CRC32_HD void rg_rip_off_product(uint32_t w, uint32_t i, uint32_t *lo, uint32_t *hi) {
    const uint64_t p = (uint64_t)w * i;
    *lo += (uint32_t)p;
    *hi += (uint32_t)(p >> 32);
}

// rg_rip_host.cpp: the disc of `n` track records (rg_rip_track_record) in call order: out[0 .. n] (n + 1 entries)
void rg_rip_disc(const RgRipTrack *recs, size_t n, RgRipDiscTrack *out);
// the blocks of a launch: every tile of every track that holds a frame that counts
void rg_rip_offsets_plan(const RgRipDiscTrack *tr, size_t n, std::vector<RgRipOffTile> *tiles);
// W[0 .. tr[n].base) of a disc in host memory
void rg_rip_disc_words(const unsigned char *arena, const RgRipDiscTrack *tr, size_t n, std::vector<uint32_t> *W);
// the definition: one track at one offset
void rg_rip_offsets_cell(const std::vector<uint32_t> &W, const RgRipDiscTrack &t, int32_t o, uint32_t *v1, uint32_t *v2);
// routes 0 and 2 of rg_rip_offsets_arena, and every route's argument checks (recs: n + 1 entries on RG_OK)
int rg_rip_offsets_check(int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, int32_t radius, const void *arena,
                         size_t arena_bytes, const uint32_t *arv2, std::vector<RgRipDiscTrack> *recs, char *err, size_t err_len);
int rg_rip_offsets_host(int route, const std::vector<RgRipDiscTrack> &recs, int32_t radius, const void *arena, uint32_t *arv1, uint32_t *arv2);

#if defined(__HIPCC__)
struct rg_ctx;
// the disc tr[0 .. n] in the device arena at `d_arena`: the kernel on `s`, arv1 / arv2 (host, n x (2 radius + 1), either may
// be null) <- the tables; `s` has been synchronised on return
int rg_rip_offsets_device(rg_ctx *c, const unsigned char *d_arena, const RgRipDiscTrack *tr, size_t n, int32_t radius, uint32_t *arv1, uint32_t *arv2,
                          hipStream_t s);
// `n` records of planes in the device arena at `d_arena` (allocated in whole 16-byte words): the two kernels on `s`,
// sums[i] <- track i; `s` has been synchronised on return
int rg_rip_device(rg_ctx *c, const unsigned char *d_arena, RgRipTrack *recs, size_t n, RgRipSums *sums, hipStream_t s);
// rg_pcm_stats_rate's yardstick, the same two kernels without their copies: with `upload` the `n` planned records (rg_rip_plan:
// `n_tiles`) go to the device on `s` and nothing is launched; without it the two kernels are enqueued over what was uploaded
int rg_rip_kernels(rg_ctx *c, const unsigned char *d_arena, const RgRipTrack *recs, size_t n, uint64_t n_tiles, bool upload, hipStream_t s);
#endif
