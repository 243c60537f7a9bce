// rg_flacdev.hip -- the device half of the FLAC decoder: the staged compressed streams and their frame index in, planar
// integer PCM out, written straight into the analysis arena.
//
// Three kernels on one stream, after one H2D copy of [stream bytes | frame table | stream table]:
//   rg_flac_check_kernel  one lane per frame: CRC-16 of the frame (table in LDS) -> good / dropped
//   rg_flac_layout_kernel one block per stream: prefix sum of the good frames' block sizes -> each frame's first output
//                         sample, the stream's decoded length (the plane stride) and its decoded frame count
//   rg_flac_decode_kernel one lane per frame, channels in order (rg_flac_frame.h: a subframe's start is known only once
//                         the one before it is parsed); consecutive lanes take consecutive frames of one stream, so a
//                         wave's predictor orders and Rice parameters are mostly alike.  Orders <= 12 keep predictor
//                         history and coefficients in registers (order-templated), orders 13-32 an LDS column per lane.
// A frame whose CRC-16 holds but that does not parse marks itself dropped and counts itself; the host then runs the
// layout and decode once more (the verdict of a frame does not depend on where its samples go), so the arena never
// holds a gap.  Nothing here uses scratch (tests/test_flac_isa.py) and every store is a plain C++ vector store.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/mp3rgain_amd.h"
#include "rg_ctx.h"
#include "rg_flac.h"
#include "rg_flac_frame.h"

namespace {

constexpr int kDecodeBlock = 128;  // lanes per block of the decode kernel: 64 LDS words per lane for the high-order ring
constexpr size_t kPad = 64;        // zero bytes behind the staged streams: the bit reader loads whole words a little ahead

struct FlacDevFrame {
    uint64_t off;      // in the blob
    uint32_t len;
    uint32_t bs;
    uint32_t stream;
    uint8_t assign, hlen;
    uint16_t pad;
};
static_assert(sizeof(FlacDevFrame) == 24, "frame record layout");

struct FlacDevStreamD {
    uint64_t dst;      // device address of plane 0
    uint32_t first_frame, n_frames;
    uint32_t channels, bps, elem, shift;
};
static_assert(sizeof(FlacDevStreamD) == 32, "stream record layout");

// per stream, written by the layout kernel
struct FlacDevResult {
    uint64_t samples;
    uint32_t good;
    uint32_t pad;
};

__global__ void __launch_bounds__(256)
rg_flac_check_kernel(const uint8_t *__restrict__ blob, const FlacDevFrame *__restrict__ frames, uint32_t n_frames,
                     const uint8_t *__restrict__ dropped, uint8_t *__restrict__ good) {
    __shared__ uint16_t tab[256];
    tab[threadIdx.x] = rg_flac_crc16_entry(threadIdx.x);
    __syncthreads();
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    const FlacDevFrame fr = frames[f];
    if (dropped[f] || fr.len < (uint32_t)fr.hlen + 2) {
        good[f] = 0;
        return;
    }
    const uint8_t *p = blob + fr.off;
    const uint32_t n = fr.len - 2;
    uint32_t c = 0;
    uint32_t k = 0;
    for (; k < n && (((uintptr_t)(p + k)) & 3); ++k) c = ((c << 8) ^ tab[((c >> 8) ^ p[k]) & 0xFF]) & 0xFFFF;
    for (; k + 4 <= n; k += 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(p + k);
        c = ((c << 8) ^ tab[((c >> 8) ^ w) & 0xFF]) & 0xFFFF;
        c = ((c << 8) ^ tab[((c >> 8) ^ (w >> 8)) & 0xFF]) & 0xFFFF;
        c = ((c << 8) ^ tab[((c >> 8) ^ (w >> 16)) & 0xFF]) & 0xFFFF;
        c = ((c << 8) ^ tab[((c >> 8) ^ (w >> 24)) & 0xFF]) & 0xFFFF;
    }
    for (; k < n; ++k) c = ((c << 8) ^ tab[((c >> 8) ^ p[k]) & 0xFF]) & 0xFFFF;
    good[f] = c == (((uint32_t)p[n] << 8) | p[n + 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
rg_flac_layout_kernel(const FlacDevFrame *__restrict__ frames, const FlacDevStreamD *__restrict__ streams, const uint8_t *__restrict__ good,
                      uint64_t *__restrict__ out_off, FlacDevResult *__restrict__ results) {
    __shared__ uint64_t part[256];
    const FlacDevStreamD st = streams[blockIdx.x];
    uint64_t base = 0;
    uint32_t n_good = 0;
    for (uint32_t at = 0; at < st.n_frames; at += 256) {
        const uint32_t f = st.first_frame + at + threadIdx.x;
        const bool in = at + threadIdx.x < st.n_frames;
        const uint32_t g = in ? good[f] : 0;
        const uint64_t mine = g ? frames[f].bs : 0;
        part[threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele scan
            const uint64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (in) out_off[f] = base + part[threadIdx.x] - mine;
        base += part[255];
        __syncthreads();
        n_good += (uint32_t)__syncthreads_count(g != 0);
    }
    if (threadIdx.x == 0) {
        FlacDevResult r;
        r.samples = base;
        r.good = n_good;
        r.pad = 0;
        results[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(kDecodeBlock)
rg_flac_decode_kernel(const uint8_t *__restrict__ blob, uint64_t blob_len, const FlacDevFrame *__restrict__ frames, uint32_t n_frames,
                      const FlacDevStreamD *__restrict__ streams, const uint8_t *__restrict__ good, const uint64_t *__restrict__ out_off,
                      const FlacDevResult *__restrict__ results, uint8_t *__restrict__ dropped, uint32_t *__restrict__ failures) {
    __shared__ int32_t ring[64 * kDecodeBlock];  // per lane: 32 history words, then 32 coefficients, kDecodeBlock apart
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames || !good[f]) return;
    const FlacDevFrame fr = frames[f];
    const FlacDevStreamD st = streams[fr.stream];
    RgFlacArenaOut out{reinterpret_cast<unsigned char *>(st.dst), results[fr.stream].samples, out_off[f], st.elem, st.shift};
    if (!rg_flac_decode_frame(blob, blob_len, fr.off, fr.len, fr.hlen, fr.bs, fr.assign, st.channels, st.bps, ring + threadIdx.x,
                              kDecodeBlock, out)) {
        dropped[f] = 1;
        atomicAdd(failures, 1u);
    }
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

int rg_flacdev_decode(rg_ctx *c, RgFlacDevStream *streams, size_t n, hipStream_t s) {
    if (n == 0) return RG_OK;
    size_t bytes = 0, n_frames = 0;
    for (size_t i = 0; i < n; ++i) {
        bytes = align16(bytes + streams[i].len);
        n_frames += streams[i].n_frames;
    }
    if (n_frames > 0xFFFFFFFFu) return rg_set_err(c, RG_ERR_INVALID_ARG, "too many FLAC frames in one call");
    const size_t frames_off = align16(bytes + kPad);
    const size_t streams_off = align16(frames_off + n_frames * sizeof(FlacDevFrame));
    const size_t blob_total = streams_off + n * sizeof(FlacDevStreamD);
    // work: dropped[F] | good[F] | out_off[F] (u64) | results[n] | failures
    const size_t drop_off = 0, good_off = align16(n_frames), offs_off = align16(good_off + n_frames);
    const size_t res_off = align16(offs_off + n_frames * sizeof(uint64_t)), fail_off = align16(res_off + n * sizeof(FlacDevResult));
    const size_t work_total = fail_off + 16;
    RG_HIP(c, c->h_flac_stage.reserve(std::max(blob_total, work_total)));
    RG_HIP(c, c->d_flac_blob.reserve(blob_total));
    RG_HIP(c, c->d_flac_work.reserve(work_total));
    // the staging buffer may still be the source of an earlier call's copy
    RG_HIP(c, hipStreamSynchronize(s));
    unsigned char *h = c->h_flac_stage.p;
    FlacDevFrame *hf = reinterpret_cast<FlacDevFrame *>(h + frames_off);
    FlacDevStreamD *hs = reinterpret_cast<FlacDevStreamD *>(h + streams_off);
    size_t at = 0, fi = 0;
    for (size_t i = 0; i < n; ++i) {
        const RgFlacDevStream &in = streams[i];
        memcpy(h + at, in.bytes, in.len);
        memset(h + at + in.len, 0, align16(at + in.len) - (at + in.len));
        FlacDevStreamD &d = hs[i];
        d.dst = (uint64_t)(uintptr_t)in.dst;
        d.first_frame = (uint32_t)fi;
        d.n_frames = in.n_frames;
        d.channels = in.channels;
        d.bps = in.bps;
        d.elem = in.elem_bytes;
        d.shift = in.shift;
        for (uint32_t k = 0; k < in.n_frames; ++k, ++fi) {
            const rg_flac_frame &g = in.frames[k];
            FlacDevFrame &r = hf[fi];
            r.off = at + g.offset;
            r.len = g.length;
            r.bs = g.block_size;
            r.stream = (uint32_t)i;
            r.assign = g.channel_assignment;
            r.hlen = g.header_length;
            r.pad = 0;
        }
        at = align16(at + in.len);
    }
    memset(h + bytes, 0, frames_off - bytes);
    unsigned char *db = c->d_flac_blob.p, *dw = c->d_flac_work.p;
    RG_HIP(c, hipMemcpyAsync(db, h, blob_total, hipMemcpyHostToDevice, s));
    RG_HIP(c, hipMemsetAsync(dw, 0, work_total, s));
    const uint32_t F = (uint32_t)n_frames;
    const FlacDevFrame *d_frames = reinterpret_cast<const FlacDevFrame *>(db + frames_off);
    const FlacDevStreamD *d_streams = reinterpret_cast<const FlacDevStreamD *>(db + streams_off);
    uint8_t *d_drop = dw + drop_off, *d_good = dw + good_off;
    uint64_t *d_offs = reinterpret_cast<uint64_t *>(dw + offs_off);
    FlacDevResult *d_res = reinterpret_cast<FlacDevResult *>(dw + res_off);
    uint32_t *d_fail = reinterpret_cast<uint32_t *>(dw + fail_off);
    // at most two rounds: the second only when a frame with a good CRC-16 failed to parse in the first
    for (int round = 0; round < 2; ++round) {
        if (F) {
            hipLaunchKernelGGL(rg_flac_check_kernel, dim3((F + 255) / 256), dim3(256), 0, s, db, d_frames, F, d_drop, d_good);
            RG_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(rg_flac_layout_kernel, dim3((uint32_t)n), dim3(256), 0, s, d_frames, d_streams, d_good, d_offs, d_res);
        RG_HIP(c, hipGetLastError());
        if (F) {
            RG_HIP(c, hipMemsetAsync(d_fail, 0, sizeof(uint32_t), s));
            hipLaunchKernelGGL(rg_flac_decode_kernel, dim3((F + kDecodeBlock - 1) / kDecodeBlock), dim3(kDecodeBlock), 0, s, db,
                               (uint64_t)blob_total, d_frames, F, d_streams, d_good, d_offs, d_res, d_drop, d_fail);
            RG_HIP(c, hipGetLastError());
        }
        RG_HIP(c, hipMemcpyAsync(h + res_off, dw + res_off, fail_off + sizeof(uint32_t) - res_off, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        uint32_t failures = 0;
        memcpy(&failures, h + fail_off, sizeof failures);
        if (failures == 0) break;
    }
    const FlacDevResult *hr = reinterpret_cast<const FlacDevResult *>(h + res_off);
    for (size_t i = 0; i < n; ++i) {
        streams[i].samples = hr[i].samples;
        streams[i].decoded_frames = hr[i].good;
        streams[i].dropped_frames = streams[i].n_frames - hr[i].good;
    }
    return RG_OK;
}
