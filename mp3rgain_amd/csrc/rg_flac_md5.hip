// rg_flac_md5.hip -- MD5 of decoded FLAC audio where it lies, in the analysis arena (include/mp3rgain_amd_flac.h: "What is
// hashed").  MD5 of one stream is a serial chain, so the parallelism is across streams: one lane hashes one stream, one
// launch hashes every FLAC stream of a group, and only the digests come back.  The kernel and its host twin run the same
// code (rg_md5.h).
//
// The kernel uses no atomics, no LDS and no scratch; a lane reads the elements of its own stream's planes, each with a load
// of the element's size at its own address (planes are only sample-aligned), and writes its 16 digest bytes.  The launcher
// checks every record against the arena before the launch: nothing outside the arena can be read.
#include <string.h>

#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_flac.h"
#include "rg_flac_md5.h"
#include "rg_md5.h"

__global__ __launch_bounds__(RG_FLAC_MD5_BLOCK) void rg_flac_md5_kernel(const RgFlacMd5Rec *__restrict__ recs, uint32_t n,
                                                                        uint4 *__restrict__ digests) {
    const uint32_t i = blockIdx.x * RG_FLAC_MD5_BLOCK + threadIdx.x;
    if (i >= n) return;
    const RgFlacMd5Rec r = recs[i];
    uint32_t d[4];
    rg_md5_stream(RgMd5ArenaSource(r.plane0, r.frames, r.channels, r.elem_bytes, r.shift), r.frames, r.channels, r.bps, d);
    digests[i] = make_uint4(d[0], d[1], d[2], d[3]);
}

void rg_flac_md5_host(const RgFlacMd5Rec &r, uint8_t out[16]) {
    uint32_t d[4];
    rg_md5_stream(RgMd5ArenaSource(r.plane0, r.frames, r.channels, r.elem_bytes, r.shift), r.frames, r.channels, r.bps, d);
    for (int k = 0; k < 16; ++k) out[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
}

int rg_flac_md5_record(rg_ctx *c, size_t i, const rg_track_desc &t, uint32_t bps, const unsigned char *base, size_t arena_bytes,
                       RgFlacMd5Rec *out) {
    if (t.format != RG_FMT_S16_PLANAR && t.format != RG_FMT_S32_PLANAR)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: format %u is neither S16 nor S32 planar", i, (unsigned)t.format);
    const uint32_t elem = t.format == RG_FMT_S16_PLANAR ? 2u : 4u;
    if (bps < 4 || bps > 24 || bps > 8 * elem) return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: %u bits per sample in %u-byte elements", i, bps, elem);
    if (t.channels < 1 || t.channels > 8) return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: %u channels", i, (unsigned)t.channels);
    if (t.offset_bytes % elem) return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: offset %llu is not sample-aligned", i, (unsigned long long)t.offset_bytes);
    const uint64_t per_frame = (uint64_t)t.channels * elem;
    if (t.offset_bytes > arena_bytes || t.frames > (arena_bytes - t.offset_bytes) / per_frame)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "stream %zu: its planes reach beyond the arena (%zu bytes)", i, arena_bytes);
    out->plane0 = base + t.offset_bytes;
    out->frames = t.frames;
    out->channels = t.channels;
    out->bps = bps;
    out->elem_bytes = elem;
    out->shift = 8 * elem - bps;
    return RG_OK;
}

int rg_flac_md5_device(rg_ctx *c, const RgFlacMd5Rec *recs, size_t n, uint8_t *digests, hipStream_t s) {
    if (!n) return RG_OK;
    if (n > 0x7fffffffu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many streams in one launch: %zu", n);
    // [records | digests], both 16-byte aligned
    const size_t rec_bytes = n * sizeof(RgFlacMd5Rec), dig_bytes = n * 16;
    RG_HIP(c, c->d_flac_md5.reserve(rec_bytes + dig_bytes));
    RG_HIP(c, hipMemcpyAsync(c->d_flac_md5.p, recs, rec_bytes, hipMemcpyHostToDevice, s));
    uint4 *d_dig = reinterpret_cast<uint4 *>(c->d_flac_md5.p + rec_bytes);
    const uint32_t blocks = (uint32_t)((n + RG_FLAC_MD5_BLOCK - 1) / RG_FLAC_MD5_BLOCK);
    hipLaunchKernelGGL(rg_flac_md5_kernel, dim3(blocks), dim3(RG_FLAC_MD5_BLOCK), 0, s, reinterpret_cast<const RgFlacMd5Rec *>(c->d_flac_md5.p),
                       (uint32_t)n, d_dig);
    RG_HIP(c, hipGetLastError());
    RG_HIP(c, hipMemcpyAsync(digests, d_dig, dig_bytes, hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- host helpers of include/mp3rgain_amd_flac.h ---------------------------------------------------------------------------
extern "C" int rg_flac_stream_md5(const void *data, size_t len, uint8_t out[16]) {
    if (!data || !out) return RG_FLAC_ERR_ARG;
    rg_flac_info si;
    const int rc = rg_flac_scan(data, len, &si);
    if (rc != RG_FLAC_OK) return rc;
    // "fLaC", the block header, then STREAMINFO: the signature is its last 16 bytes (rg_flac_scan saw all 34)
    const uint8_t *sig = static_cast<const uint8_t *>(data) + si.id3v2_bytes + 4 + 4 + 18;
    memcpy(out, sig, 16);
    for (int k = 0; k < 16; ++k)
        if (sig[k]) return 1;
    return 0;
}

extern "C" int rg_flac_md5_s32(const int32_t *const *planes, uint32_t channels, uint64_t frames, uint32_t bps, uint8_t out[16]) {
    if (!out || channels < 1 || channels > 8 || bps < 4 || bps > 24 || (frames && !planes)) return RG_FLAC_ERR_ARG;
    for (uint32_t ch = 0; ch < channels && frames; ++ch)
        if (!planes[ch]) return RG_FLAC_ERR_ARG;
    uint32_t d[4];
    rg_md5_stream(RgMd5PlanesSource(planes, channels), frames, channels, bps, d);
    for (int k = 0; k < 16; ++k) out[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
    return RG_FLAC_OK;
}

extern "C" int rg_flac_md5_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena,
                                 size_t arena_bytes, uint8_t *digests) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c && route != 0) return RG_ERR_INVALID_ARG;  // the host twin needs no context (its error text: rg_last_error(NULL))
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_md5_arena: route %d (0 = host twin, 1 = kernel)", route);
    if (n && (!descs || !bps || !digests || (arena_bytes && !arena))) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_md5_arena: null array");
    try {
        std::vector<RgFlacMd5Rec> recs(n);
        if (route == 0) {
            for (size_t i = 0; i < n; ++i) {
                const int rc = rg_flac_md5_record(c, i, descs[i], bps[i], static_cast<const unsigned char *>(arena), arena_bytes, &recs[i]);
                if (rc != RG_OK) return rc;
                rg_flac_md5_host(recs[i], digests + 16 * i);
            }
            return RG_OK;
        }
        int rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        RG_HIP(c, c->d_arena.reserve(arena_bytes ? arena_bytes : 16));
        for (size_t i = 0; i < n; ++i) {
            rc = rg_flac_md5_record(c, i, descs[i], bps[i], c->d_arena.p, arena_bytes, &recs[i]);
            if (rc != RG_OK) return rc;
        }
        hipStream_t s = c->slots[0].stream;
        if (arena_bytes) RG_HIP(c, hipMemcpyAsync(c->d_arena.p, arena, arena_bytes, hipMemcpyHostToDevice, s));
        return rg_flac_md5_device(c, recs.data(), n, digests, s);
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

// ---- measurement hook (tools/flac_md5_rate.py) ---------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per 32-bit word: word w <- a mix of its index
__global__ __launch_bounds__(256) void rg_flac_md5_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        dst[w] = (uint32_t)(x >> 24);
    }
}

// `n` streams of `frames` frames of `channels` channels of 16-bit PCM, each at its own 16-byte-aligned offset of a device
// arena of its own, filled on the device.  After one warm-up of each side, `reps` rounds of: the kernel over all n streams
// (dev_ms[r], HIP events around the launch), then the host twin over a host copy of the first `host_streams` streams on
// `threads` threads (host_ms[r], host clock).  *mismatches: host digests that differ from the device's.
extern "C" int rg_flac_md5_rate(void *ctx, size_t n, uint64_t frames, uint32_t channels, size_t host_streams, uint32_t threads,
                                uint32_t reps, double *dev_ms, double *host_ms, size_t *mismatches) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || channels < 1 || channels > 8 || !reps || !dev_ms || (host_streams && (!host_ms || !threads || !mismatches)) || host_streams > n)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_md5_rate: bad arguments");
    int rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t stream_bytes = (size_t)frames * channels * 2, stride = (stream_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<unsigned char> h_arena;
    std::vector<RgFlacMd5Rec> recs(n), h_recs(host_streams);
    std::vector<uint8_t> dev_dig(n * 16), host_dig(host_streams * 16);
    hipStream_t s = c->slots[0].stream;
    auto run = [&]() -> int {
        RG_HIP(c, hipMalloc((void **)&d_arena, total));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_flac_md5_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        for (size_t i = 0; i < n; ++i) recs[i] = RgFlacMd5Rec{d_arena + i * stride, frames, channels, 16u, 2u, 0u};
        if (host_streams) {
            h_arena.resize(host_streams * stride);
            RG_HIP(c, hipMemcpyAsync(h_arena.data(), d_arena, h_arena.size(), hipMemcpyDeviceToHost, s));
            for (size_t i = 0; i < host_streams; ++i) h_recs[i] = RgFlacMd5Rec{h_arena.data() + i * stride, frames, channels, 16u, 2u, 0u};
        }
        RG_HIP(c, hipStreamSynchronize(s));
        RG_HIP(c, c->d_flac_md5.reserve(n * (sizeof(RgFlacMd5Rec) + 16)));
        RG_HIP(c, hipMemcpyAsync(c->d_flac_md5.p, recs.data(), n * sizeof(RgFlacMd5Rec), hipMemcpyHostToDevice, s));
        uint4 *d_dig = reinterpret_cast<uint4 *>(c->d_flac_md5.p + n * sizeof(RgFlacMd5Rec));
        const uint32_t blocks = (uint32_t)((n + RG_FLAC_MD5_BLOCK - 1) / RG_FLAC_MD5_BLOCK);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < host_streams; i = next.fetch_add(1)) rg_flac_md5_host(h_recs[i], &host_dig[16 * i]);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        for (uint32_t r = 0; r < reps + 1; ++r) {  // round 0 warms both sides up and is not reported
            RG_HIP(c, hipEventRecord(e0, s));
            hipLaunchKernelGGL(rg_flac_md5_kernel, dim3(blocks), dim3(RG_FLAC_MD5_BLOCK), 0, s, reinterpret_cast<const RgFlacMd5Rec *>(c->d_flac_md5.p),
                               (uint32_t)n, d_dig);
            RG_HIP(c, hipGetLastError());
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            float ms = 0.0f;
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            if (r) dev_ms[r - 1] = ms;
            if (host_streams) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                if (r) host_ms[r - 1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        RG_HIP(c, hipMemcpy(dev_dig.data(), d_dig, n * 16, hipMemcpyDeviceToHost));
        if (host_streams) {
            *mismatches = 0;
            for (size_t i = 0; i < host_streams; ++i) *mismatches += memcmp(&dev_dig[16 * i], &host_dig[16 * i], 16) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_flac_md5_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
