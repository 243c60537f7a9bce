// rg_md5.h -- RFC 1321 MD5 of a FLAC stream's unencoded audio (include/mp3rgain_amd_flac.h: "What is hashed"), shared by
// the device kernel and its host twin (rg_flac_md5.hip) so that the two cannot drift apart: the block function, and the
// walk that turns planar samples into the message -- frames in order, channels within a frame, every sample as a signed
// little-endian integer of B = (bps + 7) / 8 bytes -- and pads it.  One caller hashes one stream; nothing here touches
// memory except through the sample source it is given, and that source is asked for each sample of the stream once.
#ifndef RG_MD5_H
#define RG_MD5_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RG_MD5_HD __host__ __device__ __forceinline__
#else
#define RG_MD5_HD inline
#endif

struct RgMd5State {
    uint32_t a, b, c, d;
};

RG_MD5_HD void rg_md5_init(RgMd5State *s) {
    s->a = 0x67452301u;
    s->b = 0xefcdab89u;
    s->c = 0x98badcfeu;
    s->d = 0x10325476u;
}

RG_MD5_HD uint32_t rg_md5_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// one step: a = b + rotl(a + f(b, c, d) + m + k, s)
#define RG_MD5_FF(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define RG_MD5_GG(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define RG_MD5_HH(x, y, z) ((x) ^ (y) ^ (z))
#define RG_MD5_II(x, y, z) ((y) ^ ((x) | ~(z)))
#define RG_MD5_STEP(f, a, b, c, d, m, k, s) (a) = (b) + rg_md5_rotl((a) + f((b), (c), (d)) + (m) + (k), (s))

// The 64 steps on one 64-byte block, its 16 little-endian words in m0..m15 (named, so that they live in registers).
RG_MD5_HD void rg_md5_block(RgMd5State *st, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t m4, uint32_t m5, uint32_t m6,
                            uint32_t m7, uint32_t m8, uint32_t m9, uint32_t m10, uint32_t m11, uint32_t m12, uint32_t m13, uint32_t m14,
                            uint32_t m15) {
    uint32_t a = st->a, b = st->b, c = st->c, d = st->d;
    RG_MD5_STEP(RG_MD5_FF, a, b, c, d, m0, 0xd76aa478u, 7);
    RG_MD5_STEP(RG_MD5_FF, d, a, b, c, m1, 0xe8c7b756u, 12);
    RG_MD5_STEP(RG_MD5_FF, c, d, a, b, m2, 0x242070dbu, 17);
    RG_MD5_STEP(RG_MD5_FF, b, c, d, a, m3, 0xc1bdceeeu, 22);
    RG_MD5_STEP(RG_MD5_FF, a, b, c, d, m4, 0xf57c0fafu, 7);
    RG_MD5_STEP(RG_MD5_FF, d, a, b, c, m5, 0x4787c62au, 12);
    RG_MD5_STEP(RG_MD5_FF, c, d, a, b, m6, 0xa8304613u, 17);
    RG_MD5_STEP(RG_MD5_FF, b, c, d, a, m7, 0xfd469501u, 22);
    RG_MD5_STEP(RG_MD5_FF, a, b, c, d, m8, 0x698098d8u, 7);
    RG_MD5_STEP(RG_MD5_FF, d, a, b, c, m9, 0x8b44f7afu, 12);
    RG_MD5_STEP(RG_MD5_FF, c, d, a, b, m10, 0xffff5bb1u, 17);
    RG_MD5_STEP(RG_MD5_FF, b, c, d, a, m11, 0x895cd7beu, 22);
    RG_MD5_STEP(RG_MD5_FF, a, b, c, d, m12, 0x6b901122u, 7);
    RG_MD5_STEP(RG_MD5_FF, d, a, b, c, m13, 0xfd987193u, 12);
    RG_MD5_STEP(RG_MD5_FF, c, d, a, b, m14, 0xa679438eu, 17);
    RG_MD5_STEP(RG_MD5_FF, b, c, d, a, m15, 0x49b40821u, 22);

    RG_MD5_STEP(RG_MD5_GG, a, b, c, d, m1, 0xf61e2562u, 5);
    RG_MD5_STEP(RG_MD5_GG, d, a, b, c, m6, 0xc040b340u, 9);
    RG_MD5_STEP(RG_MD5_GG, c, d, a, b, m11, 0x265e5a51u, 14);
    RG_MD5_STEP(RG_MD5_GG, b, c, d, a, m0, 0xe9b6c7aau, 20);
    RG_MD5_STEP(RG_MD5_GG, a, b, c, d, m5, 0xd62f105du, 5);
    RG_MD5_STEP(RG_MD5_GG, d, a, b, c, m10, 0x02441453u, 9);
    RG_MD5_STEP(RG_MD5_GG, c, d, a, b, m15, 0xd8a1e681u, 14);
    RG_MD5_STEP(RG_MD5_GG, b, c, d, a, m4, 0xe7d3fbc8u, 20);
    RG_MD5_STEP(RG_MD5_GG, a, b, c, d, m9, 0x21e1cde6u, 5);
    RG_MD5_STEP(RG_MD5_GG, d, a, b, c, m14, 0xc33707d6u, 9);
    RG_MD5_STEP(RG_MD5_GG, c, d, a, b, m3, 0xf4d50d87u, 14);
    RG_MD5_STEP(RG_MD5_GG, b, c, d, a, m8, 0x455a14edu, 20);
    RG_MD5_STEP(RG_MD5_GG, a, b, c, d, m13, 0xa9e3e905u, 5);
    RG_MD5_STEP(RG_MD5_GG, d, a, b, c, m2, 0xfcefa3f8u, 9);
    RG_MD5_STEP(RG_MD5_GG, c, d, a, b, m7, 0x676f02d9u, 14);
    RG_MD5_STEP(RG_MD5_GG, b, c, d, a, m12, 0x8d2a4c8au, 20);

    RG_MD5_STEP(RG_MD5_HH, a, b, c, d, m5, 0xfffa3942u, 4);
    RG_MD5_STEP(RG_MD5_HH, d, a, b, c, m8, 0x8771f681u, 11);
    RG_MD5_STEP(RG_MD5_HH, c, d, a, b, m11, 0x6d9d6122u, 16);
    RG_MD5_STEP(RG_MD5_HH, b, c, d, a, m14, 0xfde5380cu, 23);
    RG_MD5_STEP(RG_MD5_HH, a, b, c, d, m1, 0xa4beea44u, 4);
    RG_MD5_STEP(RG_MD5_HH, d, a, b, c, m4, 0x4bdecfa9u, 11);
    RG_MD5_STEP(RG_MD5_HH, c, d, a, b, m7, 0xf6bb4b60u, 16);
    RG_MD5_STEP(RG_MD5_HH, b, c, d, a, m10, 0xbebfbc70u, 23);
    RG_MD5_STEP(RG_MD5_HH, a, b, c, d, m13, 0x289b7ec6u, 4);
    RG_MD5_STEP(RG_MD5_HH, d, a, b, c, m0, 0xeaa127fau, 11);
    RG_MD5_STEP(RG_MD5_HH, c, d, a, b, m3, 0xd4ef3085u, 16);
    RG_MD5_STEP(RG_MD5_HH, b, c, d, a, m6, 0x04881d05u, 23);
    RG_MD5_STEP(RG_MD5_HH, a, b, c, d, m9, 0xd9d4d039u, 4);
    RG_MD5_STEP(RG_MD5_HH, d, a, b, c, m12, 0xe6db99e5u, 11);
    RG_MD5_STEP(RG_MD5_HH, c, d, a, b, m15, 0x1fa27cf8u, 16);
    RG_MD5_STEP(RG_MD5_HH, b, c, d, a, m2, 0xc4ac5665u, 23);

    RG_MD5_STEP(RG_MD5_II, a, b, c, d, m0, 0xf4292244u, 6);
    RG_MD5_STEP(RG_MD5_II, d, a, b, c, m7, 0x432aff97u, 10);
    RG_MD5_STEP(RG_MD5_II, c, d, a, b, m14, 0xab9423a7u, 15);
    RG_MD5_STEP(RG_MD5_II, b, c, d, a, m5, 0xfc93a039u, 21);
    RG_MD5_STEP(RG_MD5_II, a, b, c, d, m12, 0x655b59c3u, 6);
    RG_MD5_STEP(RG_MD5_II, d, a, b, c, m3, 0x8f0ccc92u, 10);
    RG_MD5_STEP(RG_MD5_II, c, d, a, b, m10, 0xffeff47du, 15);
    RG_MD5_STEP(RG_MD5_II, b, c, d, a, m1, 0x85845dd1u, 21);
    RG_MD5_STEP(RG_MD5_II, a, b, c, d, m8, 0x6fa87e4fu, 6);
    RG_MD5_STEP(RG_MD5_II, d, a, b, c, m15, 0xfe2ce6e0u, 10);
    RG_MD5_STEP(RG_MD5_II, c, d, a, b, m6, 0xa3014314u, 15);
    RG_MD5_STEP(RG_MD5_II, b, c, d, a, m13, 0x4e0811a1u, 21);
    RG_MD5_STEP(RG_MD5_II, a, b, c, d, m4, 0xf7537e82u, 6);
    RG_MD5_STEP(RG_MD5_II, d, a, b, c, m11, 0xbd3af235u, 10);
    RG_MD5_STEP(RG_MD5_II, c, d, a, b, m2, 0x2ad7d2bbu, 15);
    RG_MD5_STEP(RG_MD5_II, b, c, d, a, m9, 0xeb86d391u, 21);
    st->a += a;
    st->b += b;
    st->c += c;
    st->d += d;
}

// Planes of the analysis arena: elements of `elem` bytes (2 or 4), the sample left-justified in its element by `shift` bits,
// plane c at plane0 + c * frames * elem.  next() gives the samples in message order -- frame by frame, the channels of a
// frame in order -- and reads each element with a load of its own size at its own (element-aligned) address: no byte
// outside the stream's planes is ever touched.
struct RgMd5ArenaSource {
    const unsigned char *p;   // the next element
    uint64_t plane_bytes;     // frames * elem
    int64_t rewind;           // from the last channel of frame f back to channel 0 of frame f + 1: (channels - 1) * plane_bytes - elem
    uint32_t channels, ch, elem, shift;
    RG_MD5_HD RgMd5ArenaSource(const unsigned char *plane0, uint64_t frames, uint32_t channels_, uint32_t elem_, uint32_t shift_)
        : p(plane0), plane_bytes(frames * elem_), rewind((int64_t)((uint64_t)(channels_ - 1) * frames * elem_) - (int64_t)elem_), channels(channels_), ch(0),
          elem(elem_), shift(shift_) {}
    RG_MD5_HD int32_t next() {
        const int32_t v = elem == 2 ? (int32_t) * reinterpret_cast<const int16_t *>(p) : *reinterpret_cast<const int32_t *>(p);
        if (++ch == channels) {
            ch = 0;
            p -= rewind;
        } else {
            p += plane_bytes;
        }
        return v >> shift;
    }
};

// Right-justified int32 planes behind separate pointers (what rg_flac_decode_s32 returns); host only.
struct RgMd5PlanesSource {
    const int32_t *const *planes;
    uint64_t f;
    uint32_t channels, ch;
    RgMd5PlanesSource(const int32_t *const *planes_, uint32_t channels_) : planes(planes_), f(0), channels(channels_), ch(0) {}
    int32_t next() {
        const int32_t v = planes[ch][f];
        if (++ch == channels) {
            ch = 0;
            ++f;
        }
        return v;
    }
};

// The message as 32-bit words: the samples' bytes, then the padding's 0x80 and zeros (the caller puts the bit length into
// the last block's words 14 and 15).  A 64-bit window takes whole samples at its top and gives words from its bottom; with
// B = 3 a word straddles samples, and the window never holds more than 31 + 24 bits.
template <typename Source>
struct RgMd5Words {
    Source src;
    uint64_t left;  // samples not yet taken
    uint64_t acc;
    uint32_t nbits, sample_bits, mask;
    bool padded;
    RG_MD5_HD RgMd5Words(const Source &s, uint64_t samples, uint32_t bytes_per_sample)
        : src(s), left(samples), acc(0), nbits(0), sample_bits(8 * bytes_per_sample), mask((1u << (8 * bytes_per_sample)) - 1u),
          padded(false) {}
    RG_MD5_HD uint32_t next() {
        while (nbits < 32) {
            if (left) {
                --left;
                acc |= (uint64_t)((uint32_t)src.next() & mask) << nbits;
                nbits += sample_bits;
            } else if (!padded) {
                padded = true;
                acc |= (uint64_t)0x80u << nbits;
                nbits += 8;
            } else {
                nbits += 32;  // zeros
            }
        }
        const uint32_t w = (uint32_t)acc;
        acc >>= 32;
        nbits -= 32;
        return w;
    }
};

// MD5 of the stream `src` gives: `frames` frames of `channels` samples, `bps` bits each (4..24).  digest[0..3] are the
// 16 digest bytes as little-endian words.
template <typename Source>
RG_MD5_HD void rg_md5_stream(const Source &src, uint64_t frames, uint32_t channels, uint32_t bps, uint32_t digest[4]) {
    const uint32_t B = (bps + 7) / 8;
    const uint64_t samples = frames * channels, bytes = samples * B;
    const uint64_t blocks = (bytes + 8) / 64 + 1;  // the message, 0x80, zeros up to 56 (mod 64), the 64-bit bit length
    RgMd5Words<Source> words(src, samples, B);
    RgMd5State st;
    rg_md5_init(&st);
    for (uint64_t k = 0; k < blocks; ++k) {
        const uint32_t m0 = words.next(), m1 = words.next(), m2 = words.next(), m3 = words.next(), m4 = words.next(), m5 = words.next(),
                       m6 = words.next(), m7 = words.next(), m8 = words.next(), m9 = words.next(), m10 = words.next(), m11 = words.next(),
                       m12 = words.next(), m13 = words.next();
        uint32_t m14 = words.next(), m15 = words.next();
        if (k + 1 == blocks) {
            m14 = (uint32_t)(bytes << 3);
            m15 = (uint32_t)(bytes >> 29);
        }
        rg_md5_block(&st, m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15);
    }
    digest[0] = st.a;
    digest[1] = st.b;
    digest[2] = st.c;
    digest[3] = st.d;
}

#endif  // RG_MD5_H
