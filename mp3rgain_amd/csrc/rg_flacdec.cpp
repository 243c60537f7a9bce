// rg_flacdec.cpp -- the host half of the FLAC decoder (include/mp3rgain_amd_flac.h): STREAMINFO, the frame walk the device
// route uses as its index, and the whole-stream reference decoder.  Frame decoding itself is rg_flac_frame.h, shared with
// the device kernel.
#include <string.h>
#include <stdio.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/mp3rgain_amd_flac.h"
#include "rg_flac.h"
#include "rg_flac_frame.h"

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

struct Tables {
    uint8_t crc8[256];
    uint16_t crc16[256];
    Tables() {
        for (uint32_t b = 0; b < 256; ++b) {
            crc8[b] = rg_flac_crc8_entry(b);
            crc16[b] = rg_flac_crc16_entry(b);
        }
    }
};
const Tables &tables() {
    static const Tables t;
    return t;
}

size_t id3v2_size(const uint8_t *d, size_t len) {
    if (len < 10 || memcmp(d, "ID3", 3) != 0 || d[3] == 0xFF || d[4] == 0xFF) return 0;
    if ((d[6] | d[7] | d[8] | d[9]) & 0x80) return 0;
    size_t n = ((size_t)d[6] << 21) | ((size_t)d[7] << 14) | ((size_t)d[8] << 7) | d[9];
    n += 10 + ((d[5] & 0x10) ? 10 : 0);  // footer
    return n <= len ? n : len;
}

int scan_impl(const uint8_t *d, size_t len, rg_flac_info *out) {
    memset(out, 0, sizeof *out);
    const size_t tag = id3v2_size(d, len);
    out->id3v2_bytes = (uint32_t)tag;
    if (len < tag + 4 || memcmp(d + tag, "fLaC", 4) != 0) return fail(RG_FLAC_ERR_NOT_FLAC, "no fLaC marker");
    size_t pos = tag + 4;
    bool first = true, last = false;
    while (!last) {
        if (pos + 4 > len) return fail(RG_FLAC_ERR_NOT_FLAC, "metadata block header past the end");
        last = (d[pos] & 0x80) != 0;
        const uint32_t type = d[pos] & 0x7F;
        const size_t blen = ((size_t)d[pos + 1] << 16) | ((size_t)d[pos + 2] << 8) | d[pos + 3];
        pos += 4;
        if (pos + blen > len) return fail(RG_FLAC_ERR_NOT_FLAC, "metadata block past the end");
        if (first) {
            if (type != 0 || blen < 34) return fail(RG_FLAC_ERR_NOT_FLAC, "the first metadata block is not STREAMINFO");
            const uint8_t *s = d + pos;
            out->min_block_size = ((uint32_t)s[0] << 8) | s[1];
            out->max_block_size = ((uint32_t)s[2] << 8) | s[3];
            out->sample_rate = ((uint32_t)s[10] << 12) | ((uint32_t)s[11] << 4) | (s[12] >> 4);
            out->channels = ((s[12] >> 1) & 7u) + 1;
            out->bits_per_sample = (((uint32_t)(s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            out->total_samples = ((uint64_t)(s[13] & 15) << 32) | ((uint64_t)s[14] << 24) | ((uint64_t)s[15] << 16) | ((uint64_t)s[16] << 8) | s[17];
            if (out->sample_rate == 0) return fail(RG_FLAC_ERR_NOT_FLAC, "STREAMINFO sample rate 0");
            first = false;
        }
        pos += blen;
    }
    out->metadata_bytes = pos;
    return RG_FLAC_OK;
}

// the frame header at d[0..avail): fields into `f`, number into *num, fixed/variable into *variable.  false if invalid.
bool parse_header(const uint8_t *d, size_t avail, const rg_flac_info &si, rg_flac_frame *f, uint64_t *num, bool *variable) {
    if (avail < 6 || d[0] != 0xFF || (d[1] & 0xFE) != 0xF8) return false;
    *variable = (d[1] & 1) != 0;
    const uint32_t bs_code = d[2] >> 4, sr_code = d[2] & 15, ch = d[3] >> 4, ss_code = (d[3] >> 1) & 7;
    if (bs_code == 0 || sr_code == 15 || ch > 10 || ss_code == 3 || (d[3] & 1)) return false;
    // coded number (UTF-8 style): up to 6 bytes for a frame number, 7 for a sample number
    size_t p = 4;
    uint32_t b0 = d[p++];
    uint64_t v;
    int extra;
    if (b0 < 0x80) { v = b0; extra = 0; }
    else if ((b0 & 0xE0) == 0xC0) { v = b0 & 0x1F; extra = 1; }
    else if ((b0 & 0xF0) == 0xE0) { v = b0 & 0x0F; extra = 2; }
    else if ((b0 & 0xF8) == 0xF0) { v = b0 & 0x07; extra = 3; }
    else if ((b0 & 0xFC) == 0xF8) { v = b0 & 0x03; extra = 4; }
    else if ((b0 & 0xFE) == 0xFC) { v = b0 & 0x01; extra = 5; }
    else if (b0 == 0xFE) { v = 0; extra = 6; }
    else return false;
    if (extra == 6 && !*variable) return false;
    if (p + (size_t)extra > avail) return false;
    for (int k = 0; k < extra; ++k) {
        const uint32_t c = d[p++];
        if ((c & 0xC0) != 0x80) return false;
        v = (v << 6) | (c & 0x3F);
    }
    *num = v;
    uint32_t bs;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576u << (bs_code - 2);
    else if (bs_code == 6) { if (p + 1 > avail) return false; bs = (uint32_t)d[p] + 1; p += 1; }
    else if (bs_code == 7) { if (p + 2 > avail) return false; bs = (((uint32_t)d[p] << 8) | d[p + 1]) + 1; p += 2; }
    else bs = 256u << (bs_code - 8);
    static const uint32_t rates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    uint32_t rate;
    if (sr_code < 12) rate = rates[sr_code];
    else if (sr_code == 12) { if (p + 1 > avail) return false; rate = (uint32_t)d[p] * 1000; p += 1; }
    else if (sr_code == 13) { if (p + 2 > avail) return false; rate = ((uint32_t)d[p] << 8) | d[p + 1]; p += 2; }
    else { if (p + 2 > avail) return false; rate = ((((uint32_t)d[p] << 8) | d[p + 1])) * 10; p += 2; }
    if (p + 1 > avail) return false;
    const uint8_t *t = tables().crc8;
    uint8_t crc = 0;
    for (size_t k = 0; k < p; ++k) crc = t[crc ^ d[k]];
    if (crc != d[p]) return false;
    // consistency with STREAMINFO
    static const uint32_t sizes[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    if (sr_code != 0 && rate != si.sample_rate) return false;
    if (ss_code != 0 && sizes[ss_code] != si.bits_per_sample) return false;
    const uint32_t nch = ch < 8 ? ch + 1 : 2;
    if (nch != si.channels) return false;
    f->block_size = bs;
    f->channel_assignment = (uint8_t)ch;
    f->header_length = (uint8_t)(p + 1);
    return true;
}

// is there a header with exactly number `want` within the next few frames' bytes after `from`?
// `budget`: bytes all such look-aheads of one walk may still scan (hostile input full of gapped candidates stays linear)
bool continued(const uint8_t *d, size_t len, size_t from, const rg_flac_info &si, bool variable, uint64_t want, size_t *budget) {
    const size_t reach = std::min(std::min(len, from + ((size_t)4 << 20)), from + *budget);
    *budget -= reach > from ? reach - from : 0;
    for (size_t pos = from; pos + 2 <= reach;) {
        const uint8_t *hit = (const uint8_t *)memchr(d + pos, 0xFF, reach - pos - 1);
        if (!hit) return false;
        pos = (size_t)(hit - d);
        rg_flac_frame f{};
        uint64_t num = 0;
        bool var = false;
        if (parse_header(d + pos, len - pos, si, &f, &num, &var) && var == variable && num == want) return true;
        ++pos;
    }
    return false;
}

uint16_t crc16(const uint8_t *d, size_t n) {
    const uint16_t *t = tables().crc16;
    uint16_t c = 0;
    for (size_t k = 0; k < n; ++k) c = (uint16_t)((c << 8) ^ t[(c >> 8) ^ d[k]]);
    return c;
}

struct HostOut {
    int32_t *const *planes;
    uint64_t at;
    void put(uint32_t ch, uint32_t i, int32_t v) { planes[ch][at + i] = v; }
    int32_t get(uint32_t ch, uint32_t i) const { return planes[ch][at + i]; }
};

// a frame's output goes to a per-frame buffer first: a frame that fails part way must leave no samples behind
bool decode_one(const uint8_t *d, size_t len, const rg_flac_frame &f, const rg_flac_info &si, std::vector<int32_t> *buf, int32_t *ring) {
    if (f.length < (uint32_t)f.header_length + 2) return false;
    const uint64_t body = f.offset + f.length - 2;
    if (crc16(d + f.offset, (size_t)(f.length - 2)) != (uint16_t)((d[body] << 8) | d[body + 1])) return false;
    buf->resize((size_t)f.block_size * si.channels);
    int32_t *pl[8];
    for (uint32_t c = 0; c < si.channels; ++c) pl[c] = buf->data() + (size_t)c * f.block_size;
    HostOut out{pl, 0};
    return rg_flac_decode_frame(d, len, f.offset, f.length, f.header_length, f.block_size, f.channel_assignment, si.channels,
                                si.bits_per_sample, ring, 1, out);
}

}  // namespace

int rg_flac_index_vec(const uint8_t *d, size_t len, std::vector<rg_flac_frame> *frames, rg_flac_info *out) {
    frames->clear();
    int rc = scan_impl(d, len, out);
    if (rc != RG_FLAC_OK) return rc;
    if (out->bits_per_sample > 24 || out->bits_per_sample < 4)
        return fail(RG_FLAC_ERR_UNSUPPORTED, "FLAC stream of more than 24 (or fewer than 4) bits per sample");
    size_t pos = (size_t)out->metadata_bytes;
    bool have = false, variable = false;
    uint64_t prev_num = 0;
    uint32_t prev_bs = 0;
    uint64_t total = 0;
    const uint64_t unit = out->max_block_size ? out->max_block_size : 4096;
    size_t budget = len + ((size_t)4 << 20);
    while (pos + 2 <= len) {
        const uint8_t *hit = (const uint8_t *)memchr(d + pos, 0xFF, len - pos - 1);
        if (!hit) break;
        pos = (size_t)(hit - d);
        rg_flac_frame f{};
        uint64_t num = 0;
        bool var = false;
        if (parse_header(d + pos, len - pos, *out, &f, &num, &var)) {
            bool ok = true;
            if (have && var == variable && num == prev_num && frames->size() >= 2 &&
                crc16(d + (*frames)[frames->size() - 2].offset, pos - (*frames)[frames->size() - 2].offset) == 0) {
                // the previous number again, and the frame before the last one holds its CRC-16 all the way up to here: the
                // last accepted header was a false sync inside that frame (with the very number expected next) -- this is
                // the real one
                frames->pop_back();
            } else if (have) {
                // continuity: strictly after the previous frame, at most 64 frames (or 64 x 65536 samples) later
                const uint64_t expect = var ? prev_num + prev_bs : prev_num + 1;
                const uint64_t window = var ? (uint64_t)64 * 65536 : 64;
                ok = var == variable && num >= expect && num - expect <= window;
                // a gap (frames lost to damage) is believed only when the header after this one continues it: a false sync
                // inside a payload that jumps ahead would otherwise shadow every real frame up to its number
                if (ok && num != expect) ok = continued(d, len, pos + f.header_length, *out, var, var ? num + f.block_size : num + 1, &budget);
            }
            if (ok) {
                if (have) frames->back().length = (uint32_t)std::min<uint64_t>(pos - frames->back().offset, 0xFFFFFFFFu);
                f.offset = pos;
                f.first_sample = var ? num : num * unit;
                frames->push_back(f);
                have = true;
                variable = var;
                prev_num = num;
                prev_bs = f.block_size;
                pos += f.header_length;  // the next header starts after this one
                continue;
            }
        }
        ++pos;
    }
    if (have) {
        // the last frame: up to the last point where its CRC-16 holds (a trailing tag or junk is not part of it); if it holds
        // nowhere, to the end of the data (and it will be dropped)
        rg_flac_frame &f = frames->back();
        const uint64_t avail = len - f.offset;
        const uint16_t *t = tables().crc16;
        uint16_t c = 0;
        uint64_t best = 0;
        const uint8_t *p = d + f.offset;
        for (uint64_t k = 0; k < avail && k < 0xFFFFFFFFu; ++k) {
            c = (uint16_t)((c << 8) ^ t[(c >> 8) ^ p[k]]);
            if (c == 0 && k + 1 >= (uint64_t)f.header_length + 2) best = k + 1;
        }
        f.length = (uint32_t)(best ? best : std::min<uint64_t>(avail, 0xFFFFFFFFu));
    }
    for (const rg_flac_frame &f : *frames) total += f.block_size;
    out->frames = total;
    out->audio_frames = (uint32_t)frames->size();
    return RG_FLAC_OK;
}

int rg_flac_decode_vec(const uint8_t *d, size_t len, const std::vector<rg_flac_frame> &frames, const rg_flac_info &si,
                       int32_t *const *planes, uint64_t capacity, rg_flac_info *out, std::vector<uint8_t> *good) {
    std::vector<int32_t> buf;
    std::vector<int32_t> ring(64);
    uint64_t at = 0;
    uint32_t dropped = 0;
    if (good) good->assign(frames.size(), 0);
    for (size_t k = 0; k < frames.size(); ++k) {
        const rg_flac_frame &f = frames[k];
        if (!decode_one(d, len, f, si, &buf, ring.data())) {
            ++dropped;
            continue;
        }
        if (good) (*good)[k] = 1;
        if (planes) {
            if (at + f.block_size > capacity) return fail(RG_FLAC_ERR_CAPACITY, "output capacity too small");
            for (uint32_t c = 0; c < si.channels; ++c) memcpy(planes[c] + at, buf.data() + (size_t)c * f.block_size, sizeof(int32_t) * f.block_size);
        }
        at += f.block_size;
    }
    *out = si;
    out->frames = at;
    out->audio_frames = (uint32_t)(frames.size() - dropped);
    out->dropped_frames = dropped;
    return RG_FLAC_OK;
}

extern "C" int rg_flac_is_flac(const void *data, size_t len) {
    if (!data) return 0;
    const uint8_t *d = (const uint8_t *)data;
    const size_t tag = id3v2_size(d, len);
    return len >= tag + 4 && memcmp(d + tag, "fLaC", 4) == 0;
}

extern "C" int rg_flac_scan(const void *data, size_t len, rg_flac_info *out) {
    if (!data || !out) return fail(RG_FLAC_ERR_ARG, "null argument");
    g_err[0] = 0;
    return scan_impl((const uint8_t *)data, len, out);
}

extern "C" int rg_flac_index_frames(const void *data, size_t len, rg_flac_frame *frames, size_t capacity, size_t *n_frames, rg_flac_info *out) {
    if (!data || !out || !n_frames || (capacity && !frames)) return fail(RG_FLAC_ERR_ARG, "null argument");
    g_err[0] = 0;
    try {
        std::vector<rg_flac_frame> v;
        const int rc = rg_flac_index_vec((const uint8_t *)data, len, &v, out);
        if (rc != RG_FLAC_OK) return rc;
        *n_frames = v.size();
        if (v.size() > capacity) return fail(RG_FLAC_ERR_CAPACITY, "frame capacity too small");
        if (!v.empty()) memcpy(frames, v.data(), v.size() * sizeof(rg_flac_frame));
        return RG_FLAC_OK;
    } catch (const std::bad_alloc &) {
        return fail(RG_FLAC_ERR_ARG, "out of memory");
    }
}

extern "C" int rg_flac_decode_s32(const void *data, size_t len, int32_t *const *planes, uint64_t capacity, rg_flac_info *out) {
    if (!data || !out) return fail(RG_FLAC_ERR_ARG, "null argument");
    g_err[0] = 0;
    try {
        std::vector<rg_flac_frame> v;
        rg_flac_info si;
        int rc = rg_flac_index_vec((const uint8_t *)data, len, &v, &si);
        if (rc != RG_FLAC_OK) {
            memset(out, 0, sizeof *out);
            return rc;
        }
        if (!planes && capacity) return fail(RG_FLAC_ERR_ARG, "null planes");
        if (planes)
            for (uint32_t c = 0; c < si.channels; ++c)
                if (!planes[c]) return fail(RG_FLAC_ERR_ARG, "null plane");
        return rg_flac_decode_vec((const uint8_t *)data, len, v, si, planes, capacity, out, nullptr);
    } catch (const std::bad_alloc &) {
        return fail(RG_FLAC_ERR_ARG, "out of memory");
    }
}

extern "C" int rg_flac_decode_arena(const void *data, size_t len, void *out, size_t capacity_bytes, uint32_t *elem_bytes, rg_flac_info *info) {
    if (!data || !info || !elem_bytes || (capacity_bytes && !out)) return fail(RG_FLAC_ERR_ARG, "null argument");
    g_err[0] = 0;
    try {
        const uint8_t *d = (const uint8_t *)data;
        std::vector<rg_flac_frame> v;
        rg_flac_info si;
        int rc = rg_flac_index_vec(d, len, &v, &si);
        if (rc != RG_FLAC_OK) {
            memset(info, 0, sizeof *info);
            return rc;
        }
        // as on the device: which frames decode first (the plane stride is the decoded length), then the good ones into place
        std::vector<uint8_t> good;
        rc = rg_flac_decode_vec(d, len, v, si, nullptr, 0, info, &good);
        if (rc != RG_FLAC_OK) return rc;
        const uint32_t eb = rgf::flac_elem_bytes(si.bits_per_sample), sh = rgf::flac_shift(si.bits_per_sample);
        *elem_bytes = eb;
        if ((uint64_t)capacity_bytes < info->frames * si.channels * eb) return fail(RG_FLAC_ERR_CAPACITY, "output capacity too small");
        std::vector<int32_t> ring(64);
        uint64_t at = 0;
        for (size_t k = 0; k < v.size(); ++k) {
            if (!good[k]) continue;
            const rg_flac_frame &f = v[k];
            RgFlacArenaOut sink{static_cast<unsigned char *>(out), info->frames, at, eb, sh};
            if (!rg_flac_decode_frame(d, len, f.offset, f.length, f.header_length, f.block_size, f.channel_assignment, si.channels,
                                      si.bits_per_sample, ring.data(), 1, sink))
                return fail(RG_FLAC_ERR_ARG, "a frame decodes into int32 planes but not through the arena sink");
            at += f.block_size;
        }
        return RG_FLAC_OK;
    } catch (const std::bad_alloc &) {
        return fail(RG_FLAC_ERR_ARG, "out of memory");
    }
}

extern "C" int rg_flac_index_selfcheck(const void *data, size_t len) {
    if (!data) return fail(RG_FLAC_ERR_ARG, "null argument");
    try {
        std::vector<rg_flac_frame> v;
        rg_flac_info si, di;
        int rc = rg_flac_index_vec((const uint8_t *)data, len, &v, &si);
        if (rc != RG_FLAC_OK) return rc;
        // the frames tile the stream: each starts where the one before it ends
        for (size_t k = 1; k < v.size(); ++k)
            if (v[k - 1].offset + v[k - 1].length != v[k].offset) return 1;
        if (!v.empty() && v.back().offset + v.back().length > len) return 1;
        std::vector<uint8_t> good;
        rc = rg_flac_decode_vec((const uint8_t *)data, len, v, si, nullptr, 0, &di, &good);
        if (rc != RG_FLAC_OK) return rc;
        uint64_t want = 0;
        uint32_t n_good = 0;
        for (size_t k = 0; k < v.size(); ++k)
            if (good[k]) { want += v[k].block_size; ++n_good; }
        if (di.audio_frames + di.dropped_frames != si.audio_frames || di.audio_frames != n_good || di.frames != want) return 1;
        // and the PCM length is what a decode into planes produces
        std::vector<std::vector<int32_t>> pl(si.channels, std::vector<int32_t>((size_t)want + 1));
        int32_t *ptr[8];
        for (uint32_t c = 0; c < si.channels; ++c) ptr[c] = pl[c].data();
        rg_flac_info ei;
        rc = rg_flac_decode_s32(data, len, ptr, want, &ei);
        if (rc != RG_FLAC_OK || ei.frames != want || ei.dropped_frames != di.dropped_frames) return 1;
        return 0;
    } catch (const std::bad_alloc &) {
        return fail(RG_FLAC_ERR_ARG, "out of memory");
    }
}

extern "C" const char *rg_flac_last_error(void) { return g_err; }
