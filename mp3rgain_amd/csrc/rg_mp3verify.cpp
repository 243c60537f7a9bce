// rg_mp3verify.cpp -- the host side of MP3 verification (include/mp3rgain_amd_mp3verify.h): the info-tag parser, the frame
// walk's findings, the host twin of both CRCs (rg_crc16.h, the code the kernels run) and the result record.  Host code only.
#include "rg_mp3verify.h"

#include <string.h>

#include <new>

#include "../../include/mp3rgain_amd_flac.h"
#include "../../include/mp3rgain_amd_mp3.h"
#include "rg_crc16.h"
#include "rg_mp3_frame.h"

namespace {

uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }

// the tag frame at `f` (`avail` bytes of the file from there on; the whole frame lies inside, rg_mp3_scan has seen to that)
void parse_tag_frame(const uint8_t *f, size_t avail, rg_mp3_tag_info *t) {
    RgMp3FrameHdr h;
    if (avail < 4 || !rg_mp3_frame_header(f, &h) || h.frame_bytes > avail) return;
    t->tag_frame_bytes = h.frame_bytes;
    const uint32_t fb = h.frame_bytes, off = 4u + h.side_bytes;
    uint32_t marker = 0;
    auto is_marker = [&](uint32_t at) { return at + 4 <= fb && (memcmp(f + at, "Xing", 4) == 0 || memcmp(f + at, "Info", 4) == 0); };
    if (is_marker(off)) marker = off;
    else if (h.crc && is_marker(off + 2)) marker = off + 2;
    t->info_frame = 1;  // the scan's verdict; no fields unless this function finds the marker itself
    if (!marker) {
        if (36 + 4 <= fb && memcmp(f + 36, "VBRI", 4) == 0) t->info_frame = 2;  // VBRI: no checksums
        return;
    }
    uint32_t p = marker + 4;
    if (p + 4 > fb) return;
    t->xing_flags = be32(f + p);
    p += 4;
    if (t->xing_flags & 1u) {
        if (p + 4 > fb) return;
        t->has_frames = 1;
        t->xing_frames = be32(f + p);
        p += 4;
    }
    if (t->xing_flags & 2u) {
        if (p + 4 > fb) return;
        t->xing_bytes = be32(f + p);
        p += 4;
    }
    if (t->xing_flags & 4u) p += 100;
    if (t->xing_flags & 8u) p += 4;
    if (p + 36 > fb) return;
    if (memcmp(f + p, "LAME", 4) != 0 && memcmp(f + p, "Lavc", 4) != 0 && memcmp(f + p, "Lavf", 4) != 0) return;
    t->has_lame_ext = 1;
    t->ext_offset = p;
    memcpy(t->encoder, f + p, 9);
    t->music_length = be32(f + p + 28);
    t->music_crc = (uint16_t)be16(f + p + 32);
    t->tag_crc = (uint16_t)be16(f + p + 34);
}

}  // namespace

uint16_t rg_mp3_crc_range_host(const uint8_t *bytes, uint64_t off, uint64_t len) {
    return (uint16_t)rg_crc16_arc_chunk(0, bytes + off, (size_t)len, kRgCrc16.arc);
}

// The arithmetic of the kernels (rg_mp3_crc.hip) on the host, step for step: chunks counted from the end, a tree over the 256
// chunk CRCs of a tile with x^(8 L 2^j), runs of tile CRCs folded with x^(8 TILE), a tree over the 256 runs with
// x^(8 TILE run 2^j).  tests/test_mp3_verify_cpu.py holds it to a bit-by-bit CRC, so the combine is proven without a GPU.
static uint32_t tree256(uint32_t *v, uint64_t unit_bytes) {
    for (uint32_t j = 0; j < RG_CRC_LEVELS; ++j) {
        const uint32_t s = 1u << j, pw = rg_crc16_x8n(unit_bytes << j);
        for (uint32_t i = 0; i < RG_CRC_BLOCK; i += 2 * s) v[i] = rg_crc16_mul(v[i], pw) ^ v[i + s];
    }
    return v[0];
}
extern "C" uint16_t rg_mp3_crc_folded_host(const void *data, size_t len) {
    const uint8_t *d = static_cast<const uint8_t *>(data);
    const uint64_t n_tiles = rg_crc_tiles_of(len);
    std::vector<uint16_t> tiles((size_t)n_tiles);
    uint32_t v[RG_CRC_BLOCK];
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const uint64_t wend = len - (n_tiles - 1 - t) * RG_CRC_TILE_BYTES, wstart = wend > RG_CRC_TILE_BYTES ? wend - RG_CRC_TILE_BYTES : 0;
        for (uint32_t i = 0; i < RG_CRC_BLOCK; ++i) {
            const int64_t e = (int64_t)(wend - wstart) - (int64_t)(RG_CRC_BLOCK - 1 - i) * RG_CRC_CHUNK;
            const int64_t b = e > (int64_t)RG_CRC_CHUNK ? e - RG_CRC_CHUNK : 0;
            v[i] = e > 0 ? rg_crc16_arc_chunk(0, d + wstart + b, (size_t)(e - b), kRgCrc16.arc) : 0;
        }
        tiles[(size_t)t] = (uint16_t)tree256(v, RG_CRC_CHUNK);
    }
    const uint64_t run = n_tiles ? (n_tiles + RG_CRC_BLOCK - 1) / RG_CRC_BLOCK : 1;
    const uint32_t x_tile = rg_crc16_x8n(RG_CRC_TILE_BYTES);
    for (uint32_t i = 0; i < RG_CRC_BLOCK; ++i) {
        const int64_t hi = (int64_t)n_tiles - (int64_t)(RG_CRC_BLOCK - 1 - i) * (int64_t)run;
        uint32_t acc = 0;
        for (int64_t t = hi - (int64_t)run < 0 ? 0 : hi - (int64_t)run; t < hi; ++t) acc = rg_crc16_mul(acc, x_tile) ^ tiles[(size_t)t];
        v[i] = acc;
    }
    return (uint16_t)tree256(v, (uint64_t)RG_CRC_TILE_BYTES * run);
}

uint32_t rg_mp3_frame_crc_host(const uint8_t *bytes, uint64_t nbytes, uint64_t off) { return rg_mp3_frame_crc_ok(bytes, nbytes, off, kRgCrc16.mpeg); }

extern "C" int rg_mp3_info_tag(const void *data, size_t len, rg_mp3_tag_info *out) {
    if (!data || !out) return RG_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    rg_mp3_stream_info si;
    if (rg_mp3_scan(data, len, &si) != RG_MP3DEC_OK) return RG_ERR_FORMAT;
    out->tag_frame_offset = si.first_frame_offset;
    if (si.info_frame) parse_tag_frame(static_cast<const uint8_t *>(data) + si.first_frame_offset, len - (size_t)si.first_frame_offset, out);
    return RG_OK;
}

int rg_mp3_verify_plan(const uint8_t *d, size_t len, RgMp3VerifyPlan *plan) {
    *plan = RgMp3VerifyPlan();
    size_t n = 0;
    if (rg_mp3_walk_offsets(d, len, nullptr, 0, &n, &plan->last_end, &plan->si) != RG_MP3DEC_OK || n == 0) return RG_ERR_FORMAT;
    std::vector<uint64_t> offs(n);
    (void)rg_mp3_walk_offsets(d, len, offs.data(), n, &n, &plan->last_end, &plan->si);
    for (uint64_t o : offs)
        if ((d[o + 1] & 1u) == 0) plan->prot.push_back(o);
    rg_mp3_tag_info &t = plan->tag;
    t.tag_frame_offset = plan->si.first_frame_offset;
    if (plan->si.info_frame) parse_tag_frame(d + t.tag_frame_offset, len - (size_t)t.tag_frame_offset, &t);
    if (t.has_lame_ext) {
        const uint64_t from = t.tag_frame_offset + t.tag_frame_bytes;
        uint64_t to = t.tag_frame_offset + (uint64_t)t.music_length;
        if (to > len) to = len;
        plan->music_off = from;
        plan->music_len = to > from ? to - from : 0;
    }
    char buf[8];
    plan->gain_tag = rg_ape_get_data(d, len, "MP3GAIN_UNDO", buf, sizeof buf) >= 0;
    return RG_OK;
}

void rg_mp3_verify_fill(const uint8_t *d, size_t len, const RgMp3VerifyPlan &plan, uint32_t dropped, uint16_t music_crc, uint32_t crc_failed,
                        rg_mp3_verify_result *r) {
    memset(r, 0, sizeof *r);
    const rg_mp3_tag_info &t = plan.tag;
    r->status = RG_OK;
    r->audio_frames = plan.si.audio_frames;
    r->dropped_frames = dropped;
    r->protected_frames = (uint32_t)plan.prot.size();
    r->frame_crc_failed = crc_failed;
    r->junk_bytes = plan.si.junk_bytes;
    r->info_frame = t.info_frame;
    r->xing_frames = t.xing_frames;
    r->xing_flags = (uint8_t)t.xing_flags;
    if (t.info_frame) r->flags |= RG_MP3_VERIFY_HAS_INFO_TAG;
    if (t.has_frames && t.xing_frames == plan.si.audio_frames) r->flags |= RG_MP3_VERIFY_FRAME_COUNT_MATCH;
    if (dropped == 0) r->flags |= RG_MP3_VERIFY_COMPLETE;
    if (crc_failed == 0) r->flags |= RG_MP3_VERIFY_FRAME_CRCS_OK;
    if (plan.gain_tag) r->flags |= RG_MP3_VERIFY_GAIN_TAG;
    if (!t.has_lame_ext) return;
    r->flags |= RG_MP3_VERIFY_HAS_LAME_EXT;
    memcpy(r->encoder, t.encoder, 9);
    r->music_length = t.music_length;
    r->audio_bytes = plan.music_len;
    r->music_crc_stored = t.music_crc;
    r->music_crc_computed = music_crc;
    if (music_crc == t.music_crc) r->flags |= RG_MP3_VERIFY_MUSIC_CRC_MATCH;
    const uint64_t music_end = t.tag_frame_offset + (uint64_t)t.music_length;
    if (music_end <= len && music_end == plan.last_end) r->flags |= RG_MP3_VERIFY_LENGTH_MATCH;
    // the tag's own CRC: LAME's rule, then libavformat's
    const uint8_t *f = d + t.tag_frame_offset;
    const uint32_t field = t.ext_offset + 34;
    const uint16_t lame = (uint16_t)rg_crc16_arc_chunk(0, f, field, kRgCrc16.arc);
    uint32_t span = 190;
    if (span > t.tag_frame_bytes) span = t.tag_frame_bytes;
    uint32_t lavf = 0;
    for (uint32_t k = 0; k < span; ++k) lavf = rg_crc16_arc_byte(lavf, (k == field || k == field + 1) ? 0u : f[k], kRgCrc16.arc);
    r->tag_crc_stored = t.tag_crc;
    r->tag_crc_computed = lame;
    if (lame == t.tag_crc) r->flags |= RG_MP3_VERIFY_TAG_CRC_MATCH;
    else if ((uint16_t)lavf == t.tag_crc) {
        r->tag_crc_computed = (uint16_t)lavf;
        r->flags |= RG_MP3_VERIFY_TAG_CRC_MATCH;
    }
}

extern "C" int rg_mp3_verify_data(const void *data, size_t len, rg_mp3_verify_result *out) {
    if (!out) return RG_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    const uint8_t *d = static_cast<const uint8_t *>(data);
    auto fail = [&](int code) {
        out->status = code;
        return code;
    };
    if (!d) return fail(RG_ERR_INVALID_ARG);
    // what the file layer's loaders take for something else (rg_file_load.hip: RIFF/WAVE, FLAC, ISO base media)
    if ((len >= 12 && memcmp(d, "RIFF", 4) == 0 && memcmp(d + 8, "WAVE", 4) == 0) || rg_flac_is_flac(d, len) || (len >= 8 && memcmp(d + 4, "ftyp", 4) == 0))
        return fail(RG_ERR_FORMAT);
    try {
        RgMp3VerifyPlan plan;
        if (rg_mp3_verify_plan(d, len, &plan) != RG_OK) return fail(RG_ERR_FORMAT);
        std::vector<float> pcm((size_t)plan.si.frames * plan.si.channels + 1);
        rg_mp3_stream_info di;
        if (rg_mp3_decode_f32(d, len, pcm.data(), plan.si.channels == 2 ? pcm.data() + plan.si.frames : nullptr, plan.si.frames, &di) != RG_MP3DEC_OK)
            return fail(RG_ERR_FORMAT);
        uint32_t failed = 0;
        for (uint64_t o : plan.prot) failed += rg_mp3_frame_crc_host(d, len, o) ? 0u : 1u;
        rg_mp3_verify_fill(d, len, plan, di.skipped_frames, rg_mp3_crc_range_host(d, plan.music_off, plan.music_len), failed, out);
    } catch (const std::bad_alloc &) {
        return fail(RG_ERR_NOMEM);
    }
    return RG_OK;
}
