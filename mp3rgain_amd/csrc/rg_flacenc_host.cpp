// rg_flacenc_host.cpp -- the host half of the FLAC encoder (include/mp3rgain_amd_flacenc.h): the checks of a call, the stream
// assembly (metadata: host byte work on every route) and the serial twin, which runs the frame functions of rg_flacenc.h on
// one lane.  Plain C++: builds alone with g++, no device and no context.
#include <stdio.h>

#include <memory>
#include <new>
#include <vector>

#include "rg_flacenc.h"
#include "rg_md5.h"
#include "rg_pcm_plane.h"

int rg_fe_options(const rg_flac_encode_options *o, uint32_t *block, uint32_t *max_lpc, uint32_t *flags, char *err, size_t err_len) {
    *block = RG_FLAC_ENC_DEFAULT_BLOCK;
    *max_lpc = RG_FLAC_ENC_DEFAULT_LPC;
    *flags = RG_FLAC_ENC_VERIFY;
    if (!o) return RG_OK;
    if (o->struct_size != sizeof(rg_flac_encode_options)) {
        snprintf(err, err_len, "rg_flac_encode_options: struct_size %u, this library's is %zu", o->struct_size, sizeof(rg_flac_encode_options));
        return RG_ERR_INVALID_ARG;
    }
    if (o->block_size) *block = o->block_size;
    if (!rg_fe_block_ok(*block)) {
        snprintf(err, err_len, "rg_flac_encode_options: block size %u (256, 512, 1024, 2048 or 4096)", *block);
        return RG_ERR_INVALID_ARG;
    }
    if (o->max_lpc_order > RG_FLAC_ENC_MAX_LPC) {
        snprintf(err, err_len, "rg_flac_encode_options: max_lpc_order %u (0 to %u)", o->max_lpc_order, RG_FLAC_ENC_MAX_LPC);
        return RG_ERR_INVALID_ARG;
    }
    *max_lpc = o->max_lpc_order & ~1u;
    *flags = o->flags;
    if (o->flags & ~RG_FLAC_ENC_VERIFY) {
        snprintf(err, err_len, "rg_flac_encode_options: flags %#x (RG_FLAC_ENC_VERIFY is all there is)", o->flags);
        return RG_ERR_INVALID_ARG;
    }
    return RG_OK;
}

int rg_fe_stream(size_t i, const rg_track_desc &t, uint32_t bps, const unsigned char *base, size_t arena_bytes, uint32_t block, uint32_t max_lpc,
                 RgFeStream *out, char *err, size_t err_len) {
    if (t.format != RG_FMT_S16_PLANAR && t.format != RG_FMT_S32_PLANAR) {
        snprintf(err, err_len, "track %zu: format %u is not integer PCM (the encoder takes S16 and S32 planar)", i, (unsigned)t.format);
        return RG_ERR_FORMAT;
    }
    int rc = rg_pcm_check_format(i, t, 8, "the encoder takes", err, err_len);
    if (rc != RG_OK) return rc;
    const uint32_t elem = rg_pcm_bps(t.format);
    if (bps < 4 || bps > 24 || bps > 8 * elem) {
        snprintf(err, err_len, "track %zu: %u bits per sample in %u-byte elements (4 to 24)", i, bps, elem);
        return RG_ERR_FORMAT;
    }
    if (t.sample_rate < 1 || t.sample_rate >= (1u << 20)) {
        snprintf(err, err_len, "track %zu: sample rate %u (1 to 1048575)", i, (unsigned)t.sample_rate);
        return RG_ERR_FORMAT;
    }
    rc = rg_pcm_check_place(i, t, arena_bytes, err, err_len);
    if (rc != RG_OK) return rc;
    out->plane0 = base ? base + t.offset_bytes : nullptr;  // no base yet: the caller sets it
    out->frames = t.frames;
    out->first_frame = 0;
    out->audio_at = 0;
    out->n_frames = rg_fe_frames_of(t.frames, block);
    out->rate = t.sample_rate;
    out->channels = t.channels;
    out->bps = bps;
    out->elem_bytes = elem;
    out->shift = 8 * elem - bps;
    out->block = block;
    out->max_lpc = max_lpc;
    out->meta_bytes = (uint32_t)rg_fe_metadata_bytes();
    out->reserved = 0;
    return RG_OK;
}

static void put_be(uint8_t *p, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) p[k] = (uint8_t)(v >> (8 * (bytes - 1 - k)));
}

void rg_fe_finish_stream(const RgFeStream &s, uint32_t min_frame, uint32_t max_frame, uint64_t audio_bytes, const uint8_t md5[16], uint8_t *dst,
                         rg_flac_encode_result *res, const uint8_t *blocks, size_t blocks_len) {
    const uint32_t vendor = sizeof(RG_FE_VENDOR) - 1;
    uint8_t *p = dst;
    memcpy(p, "fLaC", 4);
    p += 4;
    put_be(p, 34, 4);  // STREAMINFO, not the last block
    p += 4;
    put_be(p, s.block, 2);
    put_be(p + 2, s.block, 2);
    put_be(p + 4, min_frame, 3);
    put_be(p + 7, max_frame, 3);
    put_be(p + 10, ((uint64_t)s.rate << 44) | ((uint64_t)(s.channels - 1) << 41) | ((uint64_t)(s.bps - 1) << 36) | s.frames, 8);
    memcpy(p + 18, md5, 16);
    p += 34;
    if (blocks) {
        memcpy(p, blocks, blocks_len);
    } else {
        put_be(p, 0x84000000u | (8 + vendor), 4);  // VORBIS_COMMENT, the last block
        p += 4;
        for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(vendor >> (8 * k));  // little-endian lengths
        memcpy(p + 4, RG_FE_VENDOR, vendor);
        memset(p + 4 + vendor, 0, 4);  // no comments
    }

    memset(res, 0, sizeof *res);
    res->status = RG_OK;
    res->flags = RG_FLAC_ENC_COMPLETE;
    res->pcm_frames = s.frames;
    res->flac_frames = s.n_frames;
    res->sample_rate = s.rate;
    res->channels = s.channels;
    res->bits_per_sample = s.bps;
    res->block_size = s.block;
    res->min_frame_bytes = min_frame;
    res->max_frame_bytes = max_frame;
    res->pcm_bytes = s.frames * s.channels * ((s.bps + 7) / 8);
    res->metadata_bytes = s.meta_bytes;
    res->stream_bytes = res->metadata_bytes + audio_bytes;
    memcpy(res->md5_pcm, md5, 16);
}

bool rg_fe_source_blocks(const uint8_t *file, size_t len, std::vector<uint8_t> *blocks) {
    blocks->clear();
    size_t at = 0;
    if (len >= 10 && memcmp(file, "ID3", 3) == 0) {  // an ID3v2 tag in front, as rg_flac_scan skips it
        at = 10 + (((size_t)file[6] & 0x7F) << 21 | ((size_t)file[7] & 0x7F) << 14 | ((size_t)file[8] & 0x7F) << 7 | ((size_t)file[9] & 0x7F));
        if (file[5] & 0x10) at += 10;
    }
    if (at + 4 > len || memcmp(file + at, "fLaC", 4) != 0) return false;
    at += 4;
    const uint32_t vendor = sizeof(RG_FE_VENDOR) - 1;
    std::vector<uint8_t> kept;
    std::vector<size_t> starts;  // of the kept blocks, in `kept`
    bool comment = false;
    for (bool last = false; !last;) {
        if (at + 4 > len) return false;
        last = (file[at] & 0x80) != 0;
        const uint32_t type = file[at] & 0x7F;
        const size_t body = ((size_t)file[at + 1] << 16) | ((size_t)file[at + 2] << 8) | file[at + 3];
        if (at + 4 + body > len) return false;
        if (type != 0 && type != 1 && type != 3) {  // not STREAMINFO, PADDING, SEEKTABLE
            starts.push_back(kept.size());
            kept.insert(kept.end(), file + at, file + at + 4 + body);
            comment = comment || type == 4;
        }
        at += 4 + body;
    }
    if (!comment) {
        uint8_t vc[8] = {4, 0, 0, (uint8_t)(8 + vendor), (uint8_t)vendor, 0, 0, 0};
        blocks->insert(blocks->end(), vc, vc + 8);
        const char *text = RG_FE_VENDOR;
        blocks->insert(blocks->end(), text, text + vendor);
        blocks->insert(blocks->end(), 4, 0);
        for (size_t &s : starts) s += blocks->size();
        if (starts.empty()) starts.push_back(0);
        else starts.insert(starts.begin(), 0);
    }
    blocks->insert(blocks->end(), kept.begin(), kept.end());
    for (size_t k = 0; k < starts.size(); ++k) (*blocks)[starts[k]] = (uint8_t)(((*blocks)[starts[k]] & 0x7F) | (k + 1 == starts.size() ? 0x80 : 0));
    return true;
}

int rg_fe_arena_host(size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena, size_t arena_bytes,
                     const rg_flac_encode_options *options, void *out, size_t out_capacity, uint64_t *offsets, rg_flac_encode_result *results,
                     char *err, size_t err_len) {
    if (!offsets || (n && (!descs || !bps || !results || (arena_bytes && !arena))) || (out_capacity && !out)) {
        snprintf(err, err_len, "rg_flac_encode_arena: null array");
        return RG_ERR_INVALID_ARG;
    }
    uint32_t block, max_lpc, flags;
    int rc = rg_fe_options(options, &block, &max_lpc, &flags, err, err_len);
    if (rc != RG_OK) return rc;
    try {
        std::vector<RgFeStream> st(n);
        uint64_t total_frames = 0;
        for (size_t i = 0; i < n; ++i) {
            rc = rg_fe_stream(i, descs[i], bps[i], static_cast<const unsigned char *>(arena), arena_bytes, block, max_lpc, &st[i], err, err_len);
            if (rc != RG_OK) return rc;
            st[i].first_frame = total_frames;
            total_frames += st[i].n_frames;
        }
        std::vector<RgFeFrame> recs(total_frames);
        std::unique_ptr<RgFeWork> w(new RgFeWork);
        RgFeSerial x;
        for (size_t i = 0; i < n; ++i)
            for (uint32_t f = 0; f < st[i].n_frames; ++f) rg_fe_analyse_frame(x, *w, st[i], f, &recs[st[i].first_frame + f]);
        // the layout: a running sum of the frame lengths
        std::vector<uint64_t> audio(n), fmin(n), fmax(n);
        offsets[0] = 0;
        for (size_t i = 0; i < n; ++i) {
            uint64_t sum = 0;
            uint32_t lo = 0, hi = 0;
            for (uint32_t f = 0; f < st[i].n_frames; ++f) {
                const uint32_t b = recs[st[i].first_frame + f].bytes;
                sum += b;
                lo = f ? (b < lo ? b : lo) : b;
                hi = b > hi ? b : hi;
            }
            audio[i] = sum;
            fmin[i] = lo;
            fmax[i] = hi;
            st[i].audio_at = offsets[i] + st[i].meta_bytes;
            offsets[i + 1] = st[i].audio_at + sum;
        }
        if (offsets[n] > out_capacity) {
            snprintf(err, err_len, "rg_flac_encode_arena: the streams take %llu bytes, out has %zu", (unsigned long long)offsets[n], out_capacity);
            return RG_ERR_INVALID_ARG;
        }
        uint8_t *o = static_cast<uint8_t *>(out);
        std::unique_ptr<RgFeWriteWork> ww(new RgFeWriteWork);
        RgFeSerialWrite xw;
        rg_fe_write_init(xw, *ww);
        for (size_t i = 0; i < n; ++i) {
            uint64_t at = st[i].audio_at;
            for (uint32_t f = 0; f < st[i].n_frames; ++f) {
                const RgFeFrame &r = recs[st[i].first_frame + f];
                rg_fe_write_frame(xw, *ww, st[i], f, r, o + at);
                at += r.bytes;
            }
            uint32_t d[4];
            uint8_t md5[16];
            rg_md5_stream(RgMd5ArenaSource(st[i].plane0, st[i].frames, st[i].channels, st[i].elem_bytes, st[i].shift), st[i].frames, st[i].channels,
                          st[i].bps, d);
            for (int k = 0; k < 16; ++k) md5[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
            rg_fe_finish_stream(st[i], (uint32_t)fmin[i], (uint32_t)fmax[i], audio[i], md5, o + offsets[i], &results[i]);
        }
        if (ww->fail) {
            snprintf(err, err_len, "rg_flac_encode_arena: a frame's bits did not end where its record says (internal error)");
            return RG_ERR_STATE;
        }
        return RG_OK;
    } catch (const std::bad_alloc &) {
        snprintf(err, err_len, "out of memory");
        return RG_ERR_NOMEM;
    }
}

extern "C" int rg_flac_encode_source_blocks(const void *file, size_t len, void *out, size_t capacity, size_t *need) {
    if (!file || !need) return RG_ERR_INVALID_ARG;
    try {
        std::vector<uint8_t> blocks;
        if (!rg_fe_source_blocks(static_cast<const uint8_t *>(file), len, &blocks)) return RG_ERR_FORMAT;
        *need = blocks.size();
        if (capacity < blocks.size() || !out) return RG_ERR_INVALID_ARG;
        memcpy(out, blocks.data(), blocks.size());
        return RG_OK;
    } catch (const std::bad_alloc &) {
        return RG_ERR_NOMEM;
    }
}
