// rg_wav.hip -- RIFF/WAVE input of the file layer: the container parser (rg_wav_parse), the device kernels that turn the
// interleaved samples (integer PCM 8/16/24/32 bit, IEEE float 32 bit) into the planar arena, and the batch of WAV streams
// in memory (rg_analyze_wav_batch's staging).
#include "rg_files.h"

// =================================================================================================
// WAV container (host)
namespace {

uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

enum WavKind { WAV_U8 = 0, WAV_S16 = 1, WAV_S24 = 2, WAV_S32 = 3, WAV_F32 = 4 };

// the sample format of the planar arena a WAV kind is converted to: 8/16-bit -> S16, 24/32-bit -> S32
// (same normalised amplitude: x/2^15 resp. x/2^31, src/replaygain.rs:984-1018), float -> F32
uint16_t planar_format(int kind) { return kind == WAV_F32 ? RG_FMT_F32_PLANAR : (kind <= WAV_S16 ? RG_FMT_S16_PLANAR : RG_FMT_S32_PLANAR); }

}  // namespace

int rgf::wav_kind(const rg_wav_info &w) {
    if (w.sample_format == 3) return w.bits_per_sample == 32 ? WAV_F32 : -1;
    if (w.sample_format != 1) return -1;
    switch (w.bits_per_sample) {
        case 8: return WAV_U8;
        case 16: return WAV_S16;
        case 24: return WAV_S24;
        case 32: return WAV_S32;
        default: return -1;
    }
}

extern "C" int rg_wav_parse(const void *data, size_t len, rg_wav_info *out) {
    if (!data || !out) return RG_ERR_INVALID_ARG;
    const uint8_t *d = (const uint8_t *)data;
    memset(out, 0, sizeof *out);
    if (len < 12 || memcmp(d, "RIFF", 4) != 0 || memcmp(d + 8, "WAVE", 4) != 0) return RG_ERR_INVALID_ARG;
    bool have_fmt = false;
    size_t pos = 12;
    while (pos + 8 <= len) {
        const uint32_t size = le32(d + pos + 4);
        const size_t body = pos + 8;
        if (memcmp(d + pos, "fmt ", 4) == 0) {
            if (size < 16 || body + 16 > len) return RG_ERR_INVALID_ARG;
            uint16_t tag = le16(d + body);
            out->channels = le16(d + body + 2);
            out->sample_rate = le32(d + body + 4);
            out->block_align = le16(d + body + 12);
            out->bits_per_sample = le16(d + body + 14);
            if (tag == 0xFFFE && size >= 40 && body + 40 <= len) tag = le16(d + body + 24);  // SubFormat GUID, first field
            out->sample_format = tag;
            have_fmt = true;
        } else if (memcmp(d + pos, "data", 4) == 0) {
            if (!have_fmt) return RG_ERR_INVALID_ARG;
            const uint32_t bytes_per_frame = (uint32_t)out->channels * (out->bits_per_sample / 8u);
            if (out->channels == 0 || bytes_per_frame == 0 || out->block_align != bytes_per_frame) return RG_ERR_INVALID_ARG;
            // a streamed WAV (decoder pipe) cannot know its length: 0 or 0xFFFFFFFF mean "to the end"
            uint64_t avail = len - body;
            uint64_t n = (size == 0 || size == 0xFFFFFFFFu || size > avail) ? avail : size;
            out->data_offset = body;
            out->frames = n / bytes_per_frame;
            return RG_OK;
        }
        const uint64_t next = (uint64_t)body + size + (size & 1u);  // chunks are word aligned
        if (next > len) break;
        pos = (size_t)next;
    }
    return RG_ERR_INVALID_ARG;
}

uint32_t rgf::wav_channel_mask(const void *data, size_t len) {
    const uint8_t *d = (const uint8_t *)data;
    if (!d || len < 12 || memcmp(d, "RIFF", 4) != 0 || memcmp(d + 8, "WAVE", 4) != 0) return 0;
    size_t pos = 12;
    while (pos + 8 <= len) {
        const uint32_t size = le32(d + pos + 4);
        const size_t body = pos + 8;
        if (memcmp(d + pos, "fmt ", 4) == 0)
            return size >= 40 && body + 40 <= len && le16(d + body) == 0xFFFE ? le32(d + body + 20) : 0u;
        if (memcmp(d + pos, "data", 4) == 0) return 0;
        const uint64_t next = (uint64_t)body + size + (size & 1u);
        if (next > len) break;
        pos = (size_t)next;
    }
    return 0;
}

// =================================================================================================
// interleaved bytes -> planar arena (device).  One thread per frame in the general kernel; stereo f32 and
// stereo s16 (what decoders emit) move 16 bytes per lane per access when the planes are 16-byte aligned.
namespace {

template <int KIND> struct WavIn;
template <> struct WavIn<WAV_U8> { typedef int16_t out_t; static constexpr int bytes = 1;
    static __device__ out_t load(const uint8_t *p) { return (int16_t)(((int)p[0] - 128) * 256); } };
template <> struct WavIn<WAV_S16> { typedef int16_t out_t; static constexpr int bytes = 2;
    static __device__ out_t load(const uint8_t *p) { return (int16_t)(p[0] | (p[1] << 8)); } };
template <> struct WavIn<WAV_S24> { typedef int32_t out_t; static constexpr int bytes = 3;
    static __device__ out_t load(const uint8_t *p) { return (int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24)); } };
template <> struct WavIn<WAV_S32> { typedef int32_t out_t; static constexpr int bytes = 4;
    static __device__ out_t load(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); } };
template <> struct WavIn<WAV_F32> { typedef float out_t; static constexpr int bytes = 4;
    static __device__ out_t load(const uint8_t *p) {
        return __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); } };

template <int KIND>
__global__ void __launch_bounds__(256)
rg_deinterleave_kernel(const uint8_t *__restrict__ src, void *__restrict__ dst, uint64_t first, uint64_t frames, uint32_t channels) {
    typedef WavIn<KIND> W;
    typedef typename W::out_t T;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t f = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < frames; f += stride) {
        const uint8_t *p = src + f * channels * W::bytes;
        for (uint32_t c = 0; c < channels; ++c) reinterpret_cast<T *>(dst)[(uint64_t)c * frames + f] = W::load(p + c * W::bytes);
    }
}

// stereo, 4-byte samples (float and s32 share the bit copy): `quads` groups of four frames
__global__ void __launch_bounds__(256)
rg_deinterleave_stereo32_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ left, uint4 *__restrict__ right, uint64_t quads) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const uint4 a = src[2 * q], b = src[2 * q + 1];  // L0 R0 L1 R1 | L2 R2 L3 R3
        left[q] = make_uint4(a.x, a.z, b.x, b.z);
        right[q] = make_uint4(a.y, a.w, b.y, b.w);
    }
}

__global__ void __launch_bounds__(256)
rg_deinterleave_stereo16_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ left, uint4 *__restrict__ right, uint64_t octs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < octs; q += stride) {
        const uint4 a = src[2 * q], b = src[2 * q + 1];  // eight frames: each word = L (low half) | R (high half)
        auto lo = [](uint32_t x, uint32_t y) { return (x & 0xFFFFu) | (y << 16); };
        auto hi = [](uint32_t x, uint32_t y) { return (x >> 16) | (y & 0xFFFF0000u); };
        left[q] = make_uint4(lo(a.x, a.y), lo(a.z, a.w), lo(b.x, b.y), lo(b.z, b.w));
        right[q] = make_uint4(hi(a.x, a.y), hi(a.z, a.w), hi(b.x, b.y), hi(b.z, b.w));
    }
}

uint32_t grid_for(uint64_t items) {
    const uint64_t blocks = (items + 255) / 256;
    return (uint32_t)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));  // 8192 blocks = 32 per CU; grid-stride beyond
}

template <int KIND>
void launch_general(const uint8_t *src, void *dst, uint64_t first, uint64_t frames, uint32_t channels, hipStream_t s) {
    if (first >= frames) return;
    hipLaunchKernelGGL((rg_deinterleave_kernel<KIND>), dim3(grid_for(frames - first)), dim3(256), 0, s, src, dst, first, frames, channels);
}

hipError_t launch_deinterleave(int kind, const uint8_t *src, void *dst, uint64_t frames, uint32_t channels, hipStream_t s) {
    if (frames == 0) return hipSuccess;
    uint64_t done = 0;
    const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    if (channels == 2 && aligned && (kind == WAV_F32 || kind == WAV_S32) && (frames * 4) % 16 == 0) {
        const uint64_t quads = frames / 4;
        hipLaunchKernelGGL(rg_deinterleave_stereo32_kernel, dim3(grid_for(quads)), dim3(256), 0, s, (const uint4 *)src,
                           (uint4 *)dst, (uint4 *)((uint8_t *)dst + frames * 4), quads);
        done = quads * 4;
    } else if (channels == 2 && aligned && kind == WAV_S16 && (frames * 2) % 16 == 0) {
        const uint64_t octs = frames / 8;
        hipLaunchKernelGGL(rg_deinterleave_stereo16_kernel, dim3(grid_for(octs)), dim3(256), 0, s, (const uint4 *)src, (uint4 *)dst,
                           (uint4 *)((uint8_t *)dst + frames * 2), octs);
        done = octs * 8;
    }
    switch (kind) {
        case WAV_U8: launch_general<WAV_U8>(src, dst, done, frames, channels, s); break;
        case WAV_S16: launch_general<WAV_S16>(src, dst, done, frames, channels, s); break;
        case WAV_S24: launch_general<WAV_S24>(src, dst, done, frames, channels, s); break;
        case WAV_S32: launch_general<WAV_S32>(src, dst, done, frames, channels, s); break;
        default: launch_general<WAV_F32>(src, dst, done, frames, channels, s); break;
    }
    return hipGetLastError();
}

}  // namespace

namespace rgf {

int wav_layout(rg_ctx *c, size_t i, const void *bytes, size_t len, WavItem *it, rg_track_desc *d, size_t *src_total, size_t *dst_total) {
    it->bytes = (const uint8_t *)bytes;
    if (!bytes || rg_wav_parse(bytes, len, &it->info) != RG_OK) return rg_set_err(c, RG_ERR_FORMAT, "input %zu is not a RIFF/WAVE stream", i);
    it->kind = wav_kind(it->info);
    if (it->kind < 0)
        return rg_set_err(c, RG_ERR_FORMAT, "input %zu: unsupported WAV sample format (tag %u, %u bits)", i, it->info.sample_format,
                          it->info.bits_per_sample);
    it->src_off = *src_total;
    it->src_len = it->info.frames * it->info.block_align;
    *src_total = align16(*src_total + it->src_len);
    d->offset_bytes = *dst_total;
    d->frames = it->info.frames;
    d->sample_rate = it->info.sample_rate;
    d->channels = it->info.channels;
    d->format = planar_format(it->kind);
    *dst_total = align16(*dst_total + (size_t)it->info.frames * it->info.channels * rg_bytes_per_sample(d->format));
    return RG_OK;
}

int wav_copy_launch(rg_ctx *c, const WavItem &it, unsigned char *dst, hipStream_t fs) {
    if (it.src_len == 0) return RG_OK;
    RG_HIP(c, hipMemcpyAsync(c->d_wav.p + it.src_off, it.bytes + it.info.data_offset, it.src_len, hipMemcpyHostToDevice, fs));
    RG_HIP(c, launch_deinterleave(it.kind, c->d_wav.p + it.src_off, dst, it.info.frames, it.info.channels, fs));
    return RG_OK;
}

int stage_wavs(rg_ctx *c, const void *const *wav, const size_t *wav_len, size_t n, std::vector<rg_track_desc> *descs, size_t *arena_bytes) {
    std::vector<WavItem> items(n);
    size_t src_total = 0, dst_total = 0;
    descs->assign(n ? n : 1, rg_track_desc{});
    int rc = RG_OK;
    for (size_t i = 0; i < n; ++i) {
        rc = wav_layout(c, i, wav[i], wav_len[i], &items[i], &(*descs)[i], &src_total, &dst_total);
        if (rc != RG_OK) return rc;
    }
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    // the staging buffers may still be read by an earlier batch
    RG_HIP(c, rg_sync_slots(c, c->n_slots));
    RG_HIP(c, c->d_wav.reserve(src_total ? src_total : 16));
    RG_HIP(c, c->d_arena.reserve(dst_total ? dst_total : 16));
    hipStream_t fs = c->file_stream();
    for (size_t i = 0; i < n; ++i) {
        rc = wav_copy_launch(c, items[i], c->d_arena.p + (*descs)[i].offset_bytes, fs);
        if (rc != RG_OK) return rc;
    }
    // every pipeline stream must see the arena: the next enqueue waits for this point (as rg_synth_fill_device)
    if (!c->user_attached) RG_HIP(c, hipEventRecord(c->user_ev, fs));
    c->user_dirty = true;
    *arena_bytes = dst_total;
    return RG_OK;
}

}  // namespace rgf
