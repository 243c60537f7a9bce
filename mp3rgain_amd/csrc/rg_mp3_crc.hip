// rg_mp3_crc.hip -- the checksums of MP3 verification on the device (include/mp3rgain_amd_mp3verify.h, rg_crc16.h).
//
// CRC-16/ARC with initial value 0 is linear, so a byte range is cut into chunks, every chunk hashed by its own lane and the
// chunk CRCs folded in order: crc(A || B) = x^(8 len B) crc(A) + crc(B).  Chunks of RG_CRC_CHUNK bytes are counted from the
// range's END: only the first chunk is short, and leading zeros do not change the CRC, so a missing chunk in front is a
// zero and every fold step of one level multiplies by one constant.
//
//   rg_mp3_crc_tiles_kernel   one block per tile of RG_CRC_BLOCK chunks, many ranges per launch.  The block stages the tile's
//                             bytes into LDS with aligned 16-byte loads (the staging may read bytes next to the tile, inside
//                             the buffer, which is allocated in whole 16-byte words; it never hashes them), skewed by one
//                             dword per 16 so that lanes 64 bytes apart read different banks; each lane hashes its chunk
//                             from LDS with a byte table in LDS; a fixed tree over LDS folds the 256 chunk CRCs with the
//                             host-computed powers x^(8 L 2^j).  One 16-bit CRC per tile.
//   rg_mp3_crc_fold_kernel    one block per range: each lane folds a run of `run` tile CRCs in order, then the same tree with
//                             the range's powers x^(8 TILE run 2^j).  Two bytes per range come back.
//   rg_mp3_frame_crc_kernel   one lane per protected frame, from a table of frame offsets: the frame CRC over header bytes
//                             2, 3 and the side information, compared with the stored word.
// No atomics anywhere: same input, same bits.  The launcher checks every range and frame offset against the buffer first.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_crc16.h"
#include "rg_ctx.h"
#include "rg_mp3verify.h"

struct RgCrcRangeRec {
    uint64_t off, len;
    uint64_t first_tile;   // of this range among the launch's tiles
    uint32_t n_tiles, run; // run: tile CRCs one lane of the fold kernel folds (>= 1)
    uint16_t pw[RG_CRC_LEVELS];  // x^(8 TILE run 2^j)
};
struct RgCrcPowers {
    uint16_t pw[RG_CRC_LEVELS];  // x^(8 L 2^j)
    uint16_t x_tile;             // x^(8 TILE)
};

// LDS image of a tile: dword d of the aligned window at d + (d >> 4)
#define RG_CRC_WIN_DWORDS ((RG_CRC_TILE_BYTES + 32) / 4)
#define RG_CRC_LDS_DWORDS (RG_CRC_WIN_DWORDS + RG_CRC_WIN_DWORDS / 16 + 4)
__device__ __forceinline__ uint32_t rg_crc_skew(uint32_t d) { return d + (d >> 4); }

// the fixed tree: v[0] <- the fold of v[0..255] in order, level j multiplying by pw[j]
__device__ __forceinline__ void rg_crc_tree(uint16_t *v, const uint16_t *pw, uint32_t tid) {
    for (uint32_t j = 0; j < RG_CRC_LEVELS; ++j) {
        const uint32_t s = 1u << j;
        __syncthreads();
        if ((tid & (2 * s - 1)) == 0) v[tid] = (uint16_t)(rg_crc16_mul(v[tid], pw[j]) ^ v[tid + s]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(RG_CRC_BLOCK) void rg_mp3_crc_tiles_kernel(const uint8_t *__restrict__ buf, const RgCrcRangeRec *__restrict__ recs,
                                                                        uint32_t n_ranges, RgCrcPowers P, uint16_t *__restrict__ tile_crc) {
    __shared__ uint32_t s_data[RG_CRC_LDS_DWORDS];
    __shared__ uint16_t s_tab[256];
    __shared__ uint16_t s_crc[RG_CRC_BLOCK];
    __shared__ uint32_t s_range;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    s_tab[tid] = rg_crc16_arc_entry(tid);
    if (tid == 0) {  // the last range whose first tile is not behind this one (ranges without tiles share their successor's)
        uint32_t lo = 0, hi = n_ranges - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (recs[mid].first_tile <= tile) lo = mid;
            else hi = mid - 1;
        }
        while (recs[lo].n_tiles == 0 && lo > 0) --lo;  // (only behind the last tile's range; never taken for a valid launch)
        s_range = lo;
    }
    __syncthreads();
    const RgCrcRangeRec r = recs[s_range];
    const uint64_t t = tile - r.first_tile;
    // the tile's window of the range, counted from the range's end
    const uint64_t wend = r.len - (uint64_t)(r.n_tiles - 1 - t) * RG_CRC_TILE_BYTES;
    const uint64_t wstart = wend > RG_CRC_TILE_BYTES ? wend - RG_CRC_TILE_BYTES : 0;
    const uint32_t wlen = (uint32_t)(wend - wstart);
    const uint64_t g0 = r.off + wstart, ab = g0 & ~(uint64_t)15;
    const uint32_t mis = (uint32_t)(g0 - ab);
    const uint32_t nvec = (mis + wlen + 15) / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(buf + ab);
    for (uint32_t v = tid; v < nvec; v += RG_CRC_BLOCK) {
        const uint4 q = src[v];
        const uint32_t at = rg_crc_skew(4 * v);  // (4v .. 4v + 3 share one skew)
        s_data[at] = q.x;
        s_data[at + 1] = q.y;
        s_data[at + 2] = q.z;
        s_data[at + 3] = q.w;
    }
    __syncthreads();
    // lane i hashes the chunk that ends (255 - i) chunks before the window's end
    const int64_t e = (int64_t)wlen - (int64_t)(RG_CRC_BLOCK - 1 - tid) * RG_CRC_CHUNK;
    uint32_t crc = 0;
    if (e > 0) {
        uint32_t a = mis + (uint32_t)(e > (int64_t)RG_CRC_CHUNK ? e - RG_CRC_CHUNK : 0);
        const uint32_t a1 = mis + (uint32_t)e;
        for (; (a & 3u) && a < a1; ++a) crc = rg_crc16_arc_byte(crc, (s_data[rg_crc_skew(a >> 2)] >> (8 * (a & 3u))) & 0xFFu, s_tab);
        for (; a + 4 <= a1; a += 4) {
            const uint32_t w = s_data[rg_crc_skew(a >> 2)];
            crc = rg_crc16_arc_byte(crc, w & 0xFFu, s_tab);
            crc = rg_crc16_arc_byte(crc, (w >> 8) & 0xFFu, s_tab);
            crc = rg_crc16_arc_byte(crc, (w >> 16) & 0xFFu, s_tab);
            crc = rg_crc16_arc_byte(crc, w >> 24, s_tab);
        }
        for (; a < a1; ++a) crc = rg_crc16_arc_byte(crc, (s_data[rg_crc_skew(a >> 2)] >> (8 * (a & 3u))) & 0xFFu, s_tab);
    }
    s_crc[tid] = (uint16_t)crc;
    rg_crc_tree(s_crc, P.pw, tid);
    if (tid == 0) tile_crc[tile] = s_crc[0];
}

__global__ __launch_bounds__(RG_CRC_BLOCK) void rg_mp3_crc_fold_kernel(const RgCrcRangeRec *__restrict__ recs, const uint16_t *__restrict__ tile_crc,
                                                                       RgCrcPowers P, uint16_t *__restrict__ out) {
    __shared__ uint16_t s_crc[RG_CRC_BLOCK];
    __shared__ uint16_t s_pw[RG_CRC_LEVELS];
    const uint32_t tid = threadIdx.x;
    const RgCrcRangeRec r = recs[blockIdx.x];
    if (tid < RG_CRC_LEVELS) s_pw[tid] = r.pw[tid];
    // lane i folds the run that ends (255 - i) runs before the range's last tile
    const int64_t hi = (int64_t)r.n_tiles - (int64_t)(RG_CRC_BLOCK - 1 - tid) * r.run;
    int64_t lo = hi - r.run;
    if (lo < 0) lo = 0;
    uint32_t acc = 0;
    for (int64_t t = lo; t < hi; ++t) acc = rg_crc16_mul(acc, P.x_tile) ^ tile_crc[r.first_tile + (uint64_t)t];
    s_crc[tid] = (uint16_t)acc;
    rg_crc_tree(s_crc, s_pw, tid);
    if (tid == 0) out[blockIdx.x] = s_crc[0];
}

__global__ __launch_bounds__(RG_CRC_BLOCK) void rg_mp3_frame_crc_kernel(const uint8_t *__restrict__ buf, uint64_t nbytes, const uint64_t *__restrict__ offs,
                                                                        uint32_t n, uint8_t *__restrict__ ok) {
    __shared__ uint16_t s_tab[256];
    s_tab[threadIdx.x] = rg_crc16_mpeg_entry(threadIdx.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * RG_CRC_BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = (uint8_t)rg_mp3_frame_crc_ok(buf, nbytes, offs[i], s_tab);
}

static RgCrcPowers crc_powers() {
    RgCrcPowers P;
    for (uint32_t j = 0; j < RG_CRC_LEVELS; ++j) P.pw[j] = (uint16_t)rg_crc16_x8n((uint64_t)RG_CRC_CHUNK << j);
    P.x_tile = (uint16_t)rg_crc16_x8n(RG_CRC_TILE_BYTES);
    return P;
}

// the range records of a launch; returns the number of tiles
static uint64_t crc_records(const uint64_t *off, const uint64_t *len, size_t n, RgCrcRangeRec *recs) {
    uint64_t tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        RgCrcRangeRec &r = recs[i];
        r.off = off[i];
        r.len = len[i];
        r.first_tile = tiles;
        r.n_tiles = (uint32_t)rg_crc_tiles_of(len[i]);
        r.run = r.n_tiles ? (r.n_tiles + RG_CRC_BLOCK - 1) / RG_CRC_BLOCK : 1;
        for (uint32_t j = 0; j < RG_CRC_LEVELS; ++j) r.pw[j] = (uint16_t)rg_crc16_x8n(((uint64_t)RG_CRC_TILE_BYTES * r.run) << j);
        tiles += r.n_tiles;
    }
    return tiles;
}

int rg_mp3_crc_check_job(rg_ctx *c, const RgMp3CrcJob &job) {
    for (size_t i = 0; i < job.n_ranges; ++i)
        if (job.range_off[i] > job.nbytes || job.range_len[i] > job.nbytes - job.range_off[i])
            return rg_set_err(c, RG_ERR_INVALID_ARG, "range %zu: [%llu, +%llu) is not inside the buffer (%llu bytes)", i, (unsigned long long)job.range_off[i],
                              (unsigned long long)job.range_len[i], (unsigned long long)job.nbytes);
    for (size_t i = 0; i < job.n_frames; ++i)
        if (job.frame_off[i] > job.nbytes || job.nbytes - job.frame_off[i] < 6)
            return rg_set_err(c, RG_ERR_INVALID_ARG, "frame %zu: header and CRC word at %llu are not inside the buffer (%llu bytes)", i,
                              (unsigned long long)job.frame_off[i], (unsigned long long)job.nbytes);
    if (job.nbytes >= ((uint64_t)1 << 40) || job.n_ranges > 0x7fffffffu || job.n_frames > 0x7fffffffu)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %llu bytes, %zu ranges, %zu frames", (unsigned long long)job.nbytes, job.n_ranges, job.n_frames);
    return RG_OK;
}

// Device layout, every part 16-byte aligned: [bytes | range records | frame offsets] (one H2D copy) then
// [tile CRCs] [range CRCs | frame verdicts] (one D2H copy)
struct CrcLayout {
    size_t recs, frames, up_end, tiles, res, ok, end;
};
static CrcLayout crc_layout(uint64_t nbytes, size_t n_ranges, size_t n_frames, uint64_t n_tiles) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    CrcLayout l;
    l.recs = a16((size_t)nbytes);
    l.frames = a16(l.recs + n_ranges * sizeof(RgCrcRangeRec));
    l.up_end = a16(l.frames + n_frames * sizeof(uint64_t));
    l.tiles = l.up_end;
    l.res = a16(l.tiles + (size_t)n_tiles * sizeof(uint16_t));
    l.ok = l.res + n_ranges * sizeof(uint16_t);
    l.end = a16(l.ok + n_frames);
    return l;
}

static int crc_launch(rg_ctx *c, unsigned char *d, const CrcLayout &l, uint64_t nbytes, size_t n_ranges, size_t n_frames, uint64_t n_tiles, hipStream_t s) {
    const RgCrcPowers P = crc_powers();
    const RgCrcRangeRec *d_recs = reinterpret_cast<const RgCrcRangeRec *>(d + l.recs);
    uint16_t *d_tiles = reinterpret_cast<uint16_t *>(d + l.tiles);
    if (n_tiles) {
        hipLaunchKernelGGL(rg_mp3_crc_tiles_kernel, dim3((uint32_t)n_tiles), dim3(RG_CRC_BLOCK), 0, s, d, d_recs, (uint32_t)n_ranges, P, d_tiles);
        RG_HIP(c, hipGetLastError());
    }
    if (n_ranges) {
        hipLaunchKernelGGL(rg_mp3_crc_fold_kernel, dim3((uint32_t)n_ranges), dim3(RG_CRC_BLOCK), 0, s, d_recs, d_tiles, P, reinterpret_cast<uint16_t *>(d + l.res));
        RG_HIP(c, hipGetLastError());
    }
    if (n_frames) {
        const uint32_t blocks = (uint32_t)((n_frames + RG_CRC_BLOCK - 1) / RG_CRC_BLOCK);
        hipLaunchKernelGGL(rg_mp3_frame_crc_kernel, dim3(blocks), dim3(RG_CRC_BLOCK), 0, s, d, nbytes, reinterpret_cast<const uint64_t *>(d + l.frames),
                           (uint32_t)n_frames, d + l.ok);
        RG_HIP(c, hipGetLastError());
    }
    return RG_OK;
}

int rg_mp3_crc_device(rg_ctx *c, const RgMp3CrcJob &job, hipStream_t s) {
    int rc = rg_mp3_crc_check_job(c, job);
    if (rc != RG_OK) return rc;
    if (!job.n_ranges && !job.n_frames) return RG_OK;
    std::vector<RgCrcRangeRec> recs(job.n_ranges ? job.n_ranges : 1);
    const uint64_t n_tiles = crc_records(job.range_off, job.range_len, job.n_ranges, recs.data());
    if (n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many tiles in one launch: %llu", (unsigned long long)n_tiles);
    const CrcLayout l = crc_layout(job.nbytes, job.n_ranges, job.n_frames, n_tiles);
    // the upload, put together in pinned memory (no second pageable copy of the group, no staged transfer): one copy.  The
    // parts tile the byte region up to their 16-byte padding, which is zeroed so that no launch reads bytes of an earlier one
    const size_t res_bytes = l.end - l.res;
    RG_HIP(c, c->h_mp3_crc.reserve(std::max(l.up_end, res_bytes) + 16));
    unsigned char *up = c->h_mp3_crc.p;
    for (size_t k = 0; k < job.n_parts; ++k) {
        const size_t e = (size_t)(job.part_off[k] + job.part_len[k]), pe = std::min((e + 15) & ~(size_t)15, l.recs);
        if (job.part_len[k]) memcpy(up + job.part_off[k], job.parts[k], (size_t)job.part_len[k]);
        if (pe > e) memset(up + e, 0, pe - e);
    }
    if (job.n_ranges) memcpy(up + l.recs, recs.data(), job.n_ranges * sizeof(RgCrcRangeRec));
    if (job.n_frames) memcpy(up + l.frames, job.frame_off, job.n_frames * sizeof(uint64_t));
    RG_HIP(c, c->d_mp3_crc.reserve(l.end ? l.end : 16));
    unsigned char *d = c->d_mp3_crc.p;
    RG_HIP(c, hipMemcpyAsync(d, up, l.up_end, hipMemcpyHostToDevice, s));
    rc = crc_launch(c, d, l, job.nbytes, job.n_ranges, job.n_frames, n_tiles, s);
    if (rc != RG_OK) return rc;
    unsigned char *res = up;  // the results come back into the same pinned buffer, behind the upload in stream order
    RG_HIP(c, hipMemcpyAsync(res, d + l.res, res_bytes, hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    if (job.n_ranges) memcpy(job.crc_out, res, job.n_ranges * sizeof(uint16_t));
    if (job.n_frames) memcpy(job.ok_out, res + (l.ok - l.res), job.n_frames);
    return RG_OK;
}

// ---- test seams (include/mp3rgain_amd_mp3verify.h) --------------------------------------------------------------------------
static int crc_seam(rg_ctx *c, int route, const char *who, RgMp3CrcJob &job, const void *bytes, size_t nbytes) {
    if (!c && route != 0) return RG_ERR_INVALID_ARG;
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: route %d (0 = host twin, 1 = kernels)", who, route);
    if (nbytes && !bytes) return rg_set_err(c, RG_ERR_INVALID_ARG, "%s: null buffer", who);
    const uint8_t *b = static_cast<const uint8_t *>(bytes);
    const uint64_t zero = 0, len = nbytes;
    job.parts = &b;
    job.part_off = &zero;
    job.part_len = &len;
    job.n_parts = 1;
    job.nbytes = nbytes;
    try {
        if (route == 0) {
            const int rc = rg_mp3_crc_check_job(c, job);
            if (rc != RG_OK) return rc;
            for (size_t i = 0; i < job.n_ranges; ++i) job.crc_out[i] = rg_mp3_crc_range_host(b, job.range_off[i], job.range_len[i]);
            for (size_t i = 0; i < job.n_frames; ++i) job.ok_out[i] = (uint8_t)rg_mp3_frame_crc_host(b, nbytes, job.frame_off[i]);
            return RG_OK;
        }
        int rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        return rg_mp3_crc_device(c, job, c->slots[0].stream);
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

extern "C" int rg_mp3_crc_ranges(rg_ctx *c, int route, size_t n, const uint64_t *offsets, const uint64_t *lengths, const void *bytes, size_t nbytes,
                                 uint16_t *out) {
    if (n && (!offsets || !lengths || !out)) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_mp3_crc_ranges: null array");
    RgMp3CrcJob job;
    job.range_off = offsets;
    job.range_len = lengths;
    job.n_ranges = n;
    job.crc_out = out;
    return crc_seam(c, route, "rg_mp3_crc_ranges", job, bytes, nbytes);
}

extern "C" int rg_mp3_frame_crc_check(rg_ctx *c, int route, size_t n_frames, const uint64_t *frame_offsets, const void *bytes, size_t nbytes,
                                      uint8_t *out_ok) {
    if (n_frames && (!frame_offsets || !out_ok)) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_mp3_frame_crc_check: null array");
    RgMp3CrcJob job;
    job.frame_off = frame_offsets;
    job.n_frames = n_frames;
    job.ok_out = out_ok;
    return crc_seam(c, route, "rg_mp3_frame_crc_check", job, bytes, nbytes);
}

// ---- measurement hook (tools/mp3_crc_rate.py) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_mp3_crc_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}

extern "C" int rg_mp3_crc_rate(rg_ctx *c, size_t n, uint64_t stream_bytes, size_t host_streams, uint32_t threads, uint32_t reps, size_t n_frames,
                               double *dev_ms, double *host_ms, double *frame_dev_ms, double *frame_host_ms, size_t *mismatches) {
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !stream_bytes || !reps || !dev_ms || !host_ms || !frame_dev_ms || !frame_host_ms || !mismatches || !threads || !host_streams ||
        host_streams > n)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_mp3_crc_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        const uint64_t stride = (stream_bytes + 15) & ~(uint64_t)15, total = n * stride;
        // the frames: 38-byte MPEG-1 stereo protected frames laid over the first stream bytes, their CRC words made right on the host
        const size_t frame_span = 40;
        if (n_frames * frame_span > total) n_frames = (size_t)(total / frame_span);
        std::vector<uint64_t> off(n), len(n, stream_bytes), foff(n_frames);
        for (size_t i = 0; i < n; ++i) off[i] = i * stride;
        for (size_t i = 0; i < n_frames; ++i) foff[i] = i * frame_span;
        std::vector<RgCrcRangeRec> recs(n);
        const uint64_t n_tiles = crc_records(off.data(), len.data(), n, recs.data());
        if (n_tiles > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_mp3_crc_rate: too many tiles");
        const CrcLayout l = crc_layout(total, n, n_frames, n_tiles);
        RG_HIP(c, c->d_mp3_crc.reserve(l.end));
        unsigned char *d = c->d_mp3_crc.p;
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_mp3_crc_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d), (uint64_t)(l.recs / 4));
        RG_HIP(c, hipGetLastError());
        const size_t host_bytes = (size_t)std::max<uint64_t>(host_streams * stride, n_frames * frame_span);
        std::vector<unsigned char> h(host_bytes);
        RG_HIP(c, hipMemcpyAsync(h.data(), d, host_bytes, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < n_frames; ++i) {  // a valid protected header; the side information stays random
            unsigned char *f = h.data() + foff[i];
            f[0] = 0xFF; f[1] = 0xFA; f[2] = 0x90; f[3] = 0x00;
            uint32_t crc = 0xFFFFu;
            crc = rg_crc16_mpeg_byte(crc, f[2], kRgCrc16.mpeg);
            crc = rg_crc16_mpeg_byte(crc, f[3], kRgCrc16.mpeg);
            for (int k = 0; k < 32; ++k) crc = rg_crc16_mpeg_byte(crc, f[6 + k], kRgCrc16.mpeg);
            f[4] = (unsigned char)(crc >> 8);
            f[5] = (unsigned char)crc;
        }
        if (n_frames) RG_HIP(c, hipMemcpyAsync(d, h.data(), n_frames * frame_span, hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemcpyAsync(d + l.recs, recs.data(), n * sizeof(RgCrcRangeRec), hipMemcpyHostToDevice, s));
        if (n_frames) RG_HIP(c, hipMemcpyAsync(d + l.frames, foff.data(), n_frames * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        std::vector<uint16_t> host_crc(host_streams), dev_crc(n);
        std::vector<uint8_t> host_ok(n_frames ? n_frames : 1), dev_ok(n_frames ? n_frames : 1);
        auto pool_run = [&](size_t items, auto &&fn) {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < items; i = next.fetch_add(1)) fn(i);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        for (uint32_t r = 0; r < reps + 1; ++r) {  // round 0 warms both sides up and is not reported
            float ms = 0.0f;
            RG_HIP(c, hipEventRecord(e0, s));
            int lr = crc_launch(c, d, l, total, n, 0, n_tiles, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            if (r) dev_ms[r - 1] = ms;
            auto t0 = std::chrono::steady_clock::now();
            pool_run(host_streams, [&](size_t i) { host_crc[i] = rg_mp3_crc_range_host(h.data(), off[i], stream_bytes); });
            if (r) host_ms[r - 1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            RG_HIP(c, hipEventRecord(e0, s));
            lr = crc_launch(c, d, l, total, 0, n_frames, 0, s);
            if (lr != RG_OK) return lr;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            if (r) frame_dev_ms[r - 1] = ms;
            t0 = std::chrono::steady_clock::now();
            const size_t slices = threads * 8;
            pool_run(slices, [&](size_t k) {
                for (size_t i = k * n_frames / slices; i < (k + 1) * n_frames / slices; ++i) host_ok[i] = (uint8_t)rg_mp3_frame_crc_host(h.data(), host_bytes, foff[i]);
            });
            if (r) frame_host_ms[r - 1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        RG_HIP(c, hipMemcpy(dev_crc.data(), d + l.res, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        if (n_frames) RG_HIP(c, hipMemcpy(dev_ok.data(), d + l.ok, n_frames, hipMemcpyDeviceToHost));
        *mismatches = 0;
        for (size_t i = 0; i < host_streams; ++i) *mismatches += dev_crc[i] != host_crc[i];
        for (size_t i = 0; i < n_frames; ++i) *mismatches += (dev_ok[i] != host_ok[i]) || !host_ok[i];
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_mp3_crc_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}
