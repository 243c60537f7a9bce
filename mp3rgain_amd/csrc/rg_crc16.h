// rg_crc16.h -- the two 16-bit CRCs of MP3 verification (include/mp3rgain_amd_mp3verify.h), compiled for host and device: the
// byte tables, the chunk function, the combine, and the check of one protected frame.  rg_mp3_crc.hip (kernels) and
// rg_mp3verify.cpp (host twin) run this one piece of integer code.
//
// CRC-16/ARC with initial value 0 is linear in the message: crc(A || B) = x^(8 len B) * crc(A) + crc(B) in GF(2)[x] / P, and
// leading zero bytes leave it unchanged.  States are kept REFLECTED as the byte-wise algorithm keeps them: bit 15 is x^0,
// bit 0 is x^15.  rg_crc16_mul multiplies two such residues; x^(8n) comes from squaring (rg_crc16_x8n).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_CRC_HD __host__ __device__ inline
#else
#define RG_CRC_HD inline
#endif

#define RG_CRC16_ARC_POLY 0xA001u   // 0x8005 reflected
#define RG_CRC16_MPEG_POLY 0x8005u  // MSB first

// entry b of the byte tables (what the tables below hold; a kernel fills its LDS copy from these)
RG_CRC_HD constexpr uint16_t rg_crc16_arc_entry(uint32_t b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ RG_CRC16_ARC_POLY : c >> 1;
    return (uint16_t)c;
}
RG_CRC_HD constexpr uint16_t rg_crc16_mpeg_entry(uint32_t b) {
    uint32_t c = b << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ RG_CRC16_MPEG_POLY) & 0xFFFFu : (c << 1) & 0xFFFFu;
    return (uint16_t)c;
}

struct RgCrc16Tables {
    uint16_t arc[256];
    uint16_t mpeg[256];
    constexpr RgCrc16Tables() : arc(), mpeg() {
        for (uint32_t b = 0; b < 256; ++b) {
            arc[b] = rg_crc16_arc_entry(b);
            mpeg[b] = rg_crc16_mpeg_entry(b);
        }
    }
};
// the host's copy
static constexpr RgCrc16Tables kRgCrc16 = RgCrc16Tables();

// one byte through either CRC, `t` the matching byte table (host memory, LDS, ...)
RG_CRC_HD uint32_t rg_crc16_arc_byte(uint32_t crc, uint32_t byte, const uint16_t *t) { return (crc >> 8) ^ t[(crc ^ byte) & 0xFFu]; }
RG_CRC_HD uint32_t rg_crc16_mpeg_byte(uint32_t crc, uint32_t byte, const uint16_t *t) { return ((crc << 8) & 0xFFFFu) ^ t[((crc >> 8) ^ byte) & 0xFFu]; }

// the chunk function: `n` bytes at `p` through CRC-16/ARC, from state `crc`
RG_CRC_HD uint32_t rg_crc16_arc_chunk(uint32_t crc, const uint8_t *p, size_t n, const uint16_t *t) {
    for (size_t k = 0; k < n; ++k) crc = rg_crc16_arc_byte(crc, p[k], t);
    return crc;
}

// a * b mod P, reflected residues
RG_CRC_HD uint32_t rg_crc16_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x8000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ RG_CRC16_ARC_POLY : b >> 1;
    }
    return p;
}

// x^(8n) mod P, by squaring: x^8 is 0x0080 reflected
RG_CRC_HD uint32_t rg_crc16_x8n(uint64_t n) {
    uint32_t r = 0x8000u, sq = 0x0080u;  // x^0, x^8
    for (; n; n >>= 1) {
        if (n & 1u) r = rg_crc16_mul(r, sq);
        sq = rg_crc16_mul(sq, sq);
    }
    return r;
}

// crc(A || B) from crc(A), crc(B) and x^(8 len B)
RG_CRC_HD uint32_t rg_crc16_combine(uint32_t crc_a, uint32_t crc_b, uint32_t x8n_b) { return rg_crc16_mul(crc_a, x8n_b) ^ crc_b; }

// ---- one protected frame --------------------------------------------------------------------------------------------------
// The frame at `off` of a buffer of `nbytes` (off + 6 <= nbytes is the caller's to ensure): 1 when its header is a valid
// Layer III header with the protection bit 0, its side information lies inside the buffer, and the CRC over header bytes 2
// and 3 and the side information equals the big-endian word behind the header; else 0.  The header rules are
// rg_mp3_frame_header's (rg_mp3_frame.h), restated here because only the side information's size is needed.
RG_CRC_HD uint32_t rg_mp3_side_bytes_of(const uint8_t *h) {  // 0: not a Layer III header this library takes
    if (h[0] != 0xFF || (h[1] & 0xE0) != 0xE0) return 0;
    const uint32_t ver = (h[1] >> 3) & 3u, layer = (h[1] >> 1) & 3u;
    if (ver == 1 || layer != 1) return 0;
    const uint32_t br = h[2] >> 4, sr = (h[2] >> 2) & 3u;
    if (br == 0 || br == 15 || sr == 3) return 0;
    const bool lsf = ver != 3, mono = (h[3] >> 6) == 3;
    return lsf ? (mono ? 9u : 17u) : (mono ? 17u : 32u);
}
RG_CRC_HD uint32_t rg_mp3_frame_crc_ok(const uint8_t *buf, uint64_t nbytes, uint64_t off, const uint16_t *mpeg_table) {
    const uint8_t *f = buf + off;
    const uint32_t side = rg_mp3_side_bytes_of(f);
    if (!side || (f[1] & 1u)) return 0;
    if (off + 6 + side > nbytes) return 0;
    uint32_t crc = 0xFFFFu;
    crc = rg_crc16_mpeg_byte(crc, f[2], mpeg_table);
    crc = rg_crc16_mpeg_byte(crc, f[3], mpeg_table);
    for (uint32_t k = 0; k < side; ++k) crc = rg_crc16_mpeg_byte(crc, f[6 + k], mpeg_table);
    return crc == (((uint32_t)f[4] << 8) | f[5]) ? 1u : 0u;
}

// ---- how a range is cut (shared by the launcher and the kernels) ------------------------------------------------------------
#define RG_CRC_CHUNK 64u        // L: bytes one lane hashes
#define RG_CRC_BLOCK 256u       // lanes of a block = chunks of a tile
#define RG_CRC_TILE_BYTES (RG_CRC_CHUNK * RG_CRC_BLOCK)
#define RG_CRC_LEVELS 8         // log2(RG_CRC_BLOCK)

// chunks are counted from the range's END, so only the first one is short and every fold step multiplies by one constant
RG_CRC_HD uint64_t rg_crc_tiles_of(uint64_t n) { return (n + RG_CRC_TILE_BYTES - 1) / RG_CRC_TILE_BYTES; }
