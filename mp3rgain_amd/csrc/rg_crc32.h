// rg_crc32.h -- CRC-32 as zlib computes it (reflected polynomial 0xEDB88320), compiled for host and device: the constexpr
// table entry, the byte step, the product of two residues and x^(8n).  rg_rip_crc.hip (kernels) and rg_rip_host.cpp (host
// twins) run this one piece of integer code; it is modelled on rg_crc16.h.
//
// States are kept REFLECTED as the byte-wise algorithm keeps them: bit 31 is x^0, bit 0 is x^31.  One property of
// CRC-16/ARC does not carry over: zlib's CRC starts from 0xFFFFFFFF, and with a non-zero initial value leading zero bytes
// do change the CRC.  So every chunk and every fold keeps the RAW register -- initial value 0, no final XOR.  The raw
// register is linear in the message, raw(A || B) = x^(8 len B) raw(A) + raw(B) in GF(2)[x] / P, and a missing chunk in
// front is a zero.  The initial value and the final XOR are applied once per message (rg_crc32_finish): a register that
// starts at I instead of 0 ends I * x^(8 len) further on.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_CRC32_HD __host__ __device__ inline
#else
#define RG_CRC32_HD inline
#endif

#define RG_CRC32_POLY 0xEDB88320u  // 0x04C11DB7 reflected
#define RG_CRC32_X0 0x80000000u    // x^0
#define RG_CRC32_X8 0x00800000u    // x^8
#define RG_CRC32_X2_ENTRIES 40     // x^(8 2^j), j < 40: every byte count below 2^40

// entry b of the byte table (a kernel fills its LDS copy from these)
RG_CRC32_HD constexpr uint32_t rg_crc32_entry(uint32_t b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ RG_CRC32_POLY : c >> 1;
    return c;
}
// entry b of table k of slice-by-4: the byte table's entry carried over k further zero bytes
RG_CRC32_HD constexpr uint32_t rg_crc32_slice_entry(uint32_t k, uint32_t b) {
    uint32_t c = rg_crc32_entry(b);
    for (uint32_t j = 0; j < k; ++j) c = (c >> 8) ^ rg_crc32_entry(c & 0xFFu);
    return c;
}

struct RgCrc32Table {
    uint32_t t[256];
    constexpr RgCrc32Table() : t() {
        for (uint32_t b = 0; b < 256; ++b) t[b] = rg_crc32_entry(b);
    }
};
// the host's copy
static constexpr RgCrc32Table kRgCrc32 = RgCrc32Table();

// one byte through the register, `t` the byte table (host memory, LDS, ...)
RG_CRC32_HD uint32_t rg_crc32_byte(uint32_t crc, uint32_t byte, const uint32_t *t) { return (crc >> 8) ^ t[(crc ^ byte) & 0xFFu]; }
// the two bytes of a 16-bit sample, low byte first
RG_CRC32_HD uint32_t rg_crc32_u16(uint32_t crc, uint32_t s, const uint32_t *t) {
    crc = rg_crc32_byte(crc, s & 0xFFu, t);
    return rg_crc32_byte(crc, s >> 8, t);
}
// the four bytes of a little-endian word: by the byte table ...
RG_CRC32_HD uint32_t rg_crc32_u32(uint32_t crc, uint32_t w, const uint32_t *t) {
    crc ^= w;
    crc = (crc >> 8) ^ t[crc & 0xFFu];
    crc = (crc >> 8) ^ t[crc & 0xFFu];
    crc = (crc >> 8) ^ t[crc & 0xFFu];
    return (crc >> 8) ^ t[crc & 0xFFu];
}
// ... or by slice-by-4, `t4` = tables 0..3 of 256 entries each: four look-ups that do not wait for one another
RG_CRC32_HD uint32_t rg_crc32_u32_slice4(uint32_t crc, uint32_t w, const uint32_t *t4) {
    crc ^= w;
    return t4[768 + (crc & 0xFFu)] ^ t4[512 + ((crc >> 8) & 0xFFu)] ^ t4[256 + ((crc >> 16) & 0xFFu)] ^ t4[crc >> 24];
}

// a * b mod P, reflected residues
RG_CRC32_HD uint32_t rg_crc32_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = RG_CRC32_X0; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (RG_CRC32_POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8n) mod P, by squaring
RG_CRC32_HD uint32_t rg_crc32_x8n(uint64_t n) {
    uint32_t r = RG_CRC32_X0, sq = RG_CRC32_X8;
    for (; n; n >>= 1) {
        if (n & 1u) r = rg_crc32_mul(r, sq);
        sq = rg_crc32_mul(sq, sq);
    }
    return r;
}
// the same from a table x2[j] = x^(8 2^j), j < RG_CRC32_X2_ENTRIES: one product per set bit of n (n < 2^40)
RG_CRC32_HD uint32_t rg_crc32_x8n_tab(uint64_t n, const uint32_t *x2) {
    uint32_t r = RG_CRC32_X0;
    for (uint32_t j = 0; n; n >>= 1, ++j)
        if (n & 1u) r = rg_crc32_mul(r, x2[j]);
    return r;
}

// raw(A || B) from raw(A), raw(B) and x^(8 len B)
RG_CRC32_HD uint32_t rg_crc32_combine(uint32_t raw_a, uint32_t raw_b, uint32_t x8n_b) { return rg_crc32_mul(raw_a, x8n_b) ^ raw_b; }

// zlib's CRC of a message of `len` bytes from its raw register and x^(8 len); a message of no bytes gives 0
RG_CRC32_HD uint32_t rg_crc32_finish(uint32_t raw, uint64_t len, uint32_t x8n_len) {
    return len ? ~(raw ^ rg_crc32_mul(0xFFFFFFFFu, x8n_len)) : 0u;
}
