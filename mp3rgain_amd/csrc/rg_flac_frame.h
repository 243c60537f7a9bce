// rg_flac_frame.h -- the FLAC frame decoder both halves share: the host decoder (rg_flacdec.cpp) and the device decode
// kernel (rg_flacdev.hip) run this very code, so which frames decode and what they decode to cannot differ between them.
//
// A frame is decoded from its frame index entry (include/mp3rgain_amd_flac.h: rg_flac_frame): the header is already
// parsed, the subframes start `header_len` bytes in, and the frame's CRC-16 sits in its last two bytes.  Channels are
// decoded in order (a subframe's start is only known once the one before it is parsed); the stereo decorrelations are
// applied by reading the first channel back from the output, so no per-lane PCM buffer is needed:
//   left/side : left is written, side arrives second -> right = left - side
//   mid/side  : mid is written, side arrives second  -> left, right (both overwrite)
//   right/side: side comes first and does not fit a 16-bit plane, so it is parsed and thrown away, right is decoded and
//               written, then the side subframe is decoded again from its saved position -> left = side + right
// A frame fails (and is dropped by the caller) when it does not parse, when its subframes need bits past the CRC-16,
// or when a decoded sample does not fit its channel's width: every rule here is exact integer arithmetic.
#ifndef RG_FLAC_FRAME_H
#define RG_FLAC_FRAME_H

#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#define RG_FLAC_HD __host__ __device__ inline
#else
#define RG_FLAC_HD inline
#endif

// CRC-16 of FLAC frames: polynomial 0x8005, MSB first, initial value 0
RG_FLAC_HD uint16_t rg_flac_crc16_entry(uint32_t b) {
    uint32_t c = b << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
    return (uint16_t)(c & 0xFFFFu);
}
// CRC-8 of frame headers: polynomial 0x07, initial value 0
RG_FLAC_HD uint8_t rg_flac_crc8_entry(uint32_t b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) : (c << 1);
    return (uint8_t)(c & 0xFFu);
}

// Big-endian bit reader over [base, base + limit): 32-bit refills, zeros beyond `limit` (the host reads an exact-size
// buffer; the device's staging buffer is padded, so its words are whole loads).
struct RgFlacBits {
    const uint8_t *base;
    uint64_t limit;
    uint64_t next;  // next byte to load (a multiple of 4 after the first refill)
    uint64_t buf;   // valid bits left-aligned, the rest zero
    int n;

    RG_FLAC_HD uint32_t load_be32(uint64_t i) const {
        uint32_t w = 0;
        if (i + 4 <= limit) {
#if defined(__HIP_DEVICE_COMPILE__)
            // the staged streams start 16-byte aligned and `i` is a multiple of 4: one dword load
            const uint32_t x = *reinterpret_cast<const uint32_t *>(base + i);
#else
            uint32_t x;
            memcpy(&x, base + i, 4);
#endif
            w = (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
        } else {
            for (int k = 0; k < 4; ++k) w = (w << 8) | (i + (uint64_t)k < limit ? base[i + k] : 0u);
        }
        return w;
    }
    RG_FLAC_HD void refill() {
        while (n <= 32) {
            buf |= (uint64_t)load_be32(next) << (32 - n);
            n += 32;
            next += 4;
        }
    }
    RG_FLAC_HD void init(const uint8_t *b, uint64_t lim, uint64_t byte_off) {
        base = b;
        limit = lim;
        next = byte_off & ~(uint64_t)3;
        buf = 0;
        n = 0;
        refill();
        const int skip = (int)(byte_off & 3) * 8;
        buf <<= skip;
        n -= skip;
    }
    RG_FLAC_HD uint64_t pos() const { return next * 8 - (uint64_t)n; }
    // 0 <= k <= 32
    RG_FLAC_HD uint32_t get(int k) {
        if (k == 0) return 0;
        refill();
        const uint32_t v = (uint32_t)(buf >> (64 - k));
        buf <<= k;
        n -= k;
        return v;
    }
    // 1 <= k <= 32, two's complement
    RG_FLAC_HD int32_t get_signed(int k) {
        const uint32_t v = get(k);
        return k == 32 ? (int32_t)v : (int32_t)(v << (32 - k)) >> (32 - k);
    }
    // zeros before the next one bit (consumed with it); false once the count runs past `end_bits`
    RG_FLAC_HD bool unary(uint64_t end_bits, uint32_t *q) {
        uint32_t z = 0;
        for (;;) {
            refill();
            if (buf) {
                const int lz = __builtin_clzll(buf);
                z += (uint32_t)lz;
                buf = (buf << lz) << 1;
                n -= lz + 1;
                *q = z;
                return true;
            }
            z += (uint32_t)n;
            buf = 0;
            n = 0;
            if (pos() > end_bits || z > 0x7FFFFFFFu) return false;
        }
    }
};

enum RgFlacSinkMode { RG_FLAC_SINK_DIRECT = 0, RG_FLAC_SINK_DISCARD, RG_FLAC_SINK_LS_SIDE, RG_FLAC_SINK_MS_SIDE, RG_FLAC_SINK_RS_SIDE };

RG_FLAC_HD bool rg_flac_fits(int64_t v, uint32_t bits) {
    const int64_t h = (int64_t)1 << (bits - 1);
    return v >= -h && v < h;
}

// Where the samples of one subframe go.  Out: put(ch, i, v) / get(ch, i) with get returning exactly what put stored.
template <class Out>
struct RgFlacSink {
    Out *out;
    int mode;
    uint32_t ch;
    uint32_t bps;  // of the stream
    RG_FLAC_HD bool put(uint32_t i, int64_t v) {
        switch (mode) {
            case RG_FLAC_SINK_DIRECT: out->put(ch, i, (int32_t)v); return true;
            case RG_FLAC_SINK_DISCARD: return true;
            case RG_FLAC_SINK_LS_SIDE: {
                const int64_t r = (int64_t)out->get(0, i) - v;
                if (!rg_flac_fits(r, bps)) return false;
                out->put(1, i, (int32_t)r);
                return true;
            }
            case RG_FLAC_SINK_MS_SIDE: {
                const int64_t m = ((int64_t)out->get(0, i) * 2) | (v & 1);
                const int64_t l = (m + v) >> 1, r = (m - v) >> 1;
                if (!rg_flac_fits(l, bps) || !rg_flac_fits(r, bps)) return false;
                out->put(0, i, (int32_t)l);
                out->put(1, i, (int32_t)r);
                return true;
            }
            default: {  // RS_SIDE: right is in plane 1
                const int64_t l = v + (int64_t)out->get(1, i);
                if (!rg_flac_fits(l, bps)) return false;
                out->put(0, i, (int32_t)l);
                return true;
            }
        }
    }
};

// The Out of the analysis arena: planar elements of 2 or 4 bytes, each sample shifted left into its element (rg_flac.h:
// flac_elem_bytes, flac_shift), plane `ch` of the stream `stride` elements behind plane ch - 1, this frame's first sample at
// element `at`.  get() undoes put() exactly for every value of the stream's width -- the decorrelations read the first
// channel back through it, for a CD rip through a 16-bit plane.  The device decode kernel (rg_flacdev.hip) writes through
// it, and so does the host twin rg_flac_decode_arena (rg_flacdec.cpp).
struct RgFlacArenaOut {
    unsigned char *base;
    uint64_t stride;
    uint64_t at;
    uint32_t elem, shift;
    RG_FLAC_HD void put(uint32_t ch, uint32_t i, int32_t v) {
        const uint64_t idx = (uint64_t)ch * stride + at + i;
        if (elem == 2) reinterpret_cast<int16_t *>(base)[idx] = (int16_t)((uint32_t)v << shift);
        else reinterpret_cast<int32_t *>(base)[idx] = (int32_t)((uint32_t)v << shift);
    }
    RG_FLAC_HD int32_t get(uint32_t ch, uint32_t i) const {
        const uint64_t idx = (uint64_t)ch * stride + at + i;
        if (elem == 2) return (int32_t)reinterpret_cast<const int16_t *>(base)[idx] >> shift;
        return reinterpret_cast<const int32_t *>(base)[idx] >> shift;
    }
};

// The residual of a predicted subframe, with the prediction applied as it is decoded.  ORDER > 0: history and
// coefficients live in registers (compile-time indices only); ORDER < 0: the runtime order `order` (13..32) keeps them
// in `ring` (32 history words, then 32 coefficients, `stride` apart: an LDS column per lane on the device).
template <int ORDER>
struct RgFlacPred {
    int32_t c[ORDER > 0 ? ORDER : 1];
    int32_t h[ORDER > 0 ? ORDER : 1];  // h[0] = the newest sample (a subframe's samples fit 25 bits)
    RG_FLAC_HD int64_t predict(int shift) const {
        int64_t s = 0;
#pragma unroll
        for (int j = 0; j < ORDER; ++j) s += (int64_t)c[j] * h[j];
        return s >> shift;
    }
    RG_FLAC_HD void push(int64_t v) {
#pragma unroll
        for (int j = ORDER - 1; j > 0; --j) h[j] = h[j - 1];
        if (ORDER > 0) h[0] = (int32_t)v;
    }
};

struct RgFlacRing {
    int32_t *ring;
    int stride;
    uint32_t order;
    uint32_t pos;
    RG_FLAC_HD int32_t &hist(uint32_t k) { return ring[(size_t)(k & 31u) * stride]; }
    RG_FLAC_HD int32_t &coef(uint32_t j) { return ring[(size_t)(32 + j) * stride]; }
    RG_FLAC_HD int64_t predict(int shift) {
        int64_t s = 0;
        for (uint32_t j = 0; j < order; ++j) s += (int64_t)coef(j) * hist(pos - 1 - j);
        return s >> shift;
    }
    RG_FLAC_HD void push(int64_t v) { hist(pos++) = (int32_t)v; }
};

// residual partitions (Rice / Rice2 with escapes) of a subframe of `bs` samples whose first `order` samples were warm-up
template <class P, class Out>
RG_FLAC_HD bool rg_flac_residual(RgFlacBits &br, uint64_t end_bits, uint32_t bs, uint32_t order, uint32_t ebps, int wasted, int shift,
                                 P &pred, RgFlacSink<Out> &sink) {
    const uint32_t method = br.get(2);
    if (method > 1) return false;
    const int pbits = method == 0 ? 4 : 5;
    const uint32_t escape = method == 0 ? 15u : 31u;
    const uint32_t porder = br.get(4);
    const uint32_t psize = bs >> porder;
    if ((psize << porder) != bs || psize < order) return false;
    uint32_t i = order;
    for (uint32_t p = 0; p < (1u << porder); ++p) {
        const uint32_t k = br.get(pbits);
        const uint32_t cnt = p == 0 ? psize - order : psize;
        if (k == escape) {
            const uint32_t raw = br.get(5);
            for (uint32_t t = 0; t < cnt; ++t, ++i) {
                const int64_t r = raw ? (int64_t)br.get_signed((int)raw) : 0;
                const int64_t s = r + pred.predict(shift);
                if (!rg_flac_fits(s, ebps)) return false;
                pred.push(s);
                if (!sink.put(i, s * ((int64_t)1 << wasted))) return false;
            }
        } else {
            for (uint32_t t = 0; t < cnt; ++t, ++i) {
                uint32_t q;
                if (!br.unary(end_bits, &q)) return false;
                const uint64_t u = ((uint64_t)q << k) | br.get((int)k);
                const int64_t r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
                const int64_t s = r + pred.predict(shift);
                if (!rg_flac_fits(s, ebps)) return false;
                pred.push(s);
                if (!sink.put(i, s * ((int64_t)1 << wasted))) return false;
            }
        }
        if (br.pos() > end_bits) return false;
    }
    return true;
}

// warm-up, coefficients, residual for a register-resident order
template <int ORDER, class Out>
RG_FLAC_HD bool rg_flac_predicted(RgFlacBits &br, uint64_t end_bits, uint32_t bs, bool lpc, uint32_t fixed_order, uint32_t ebps, int wasted,
                                  RgFlacSink<Out> &sink) {
    RgFlacPred<ORDER> pred;
#pragma unroll
    for (int j = 0; j < (ORDER > 0 ? ORDER : 1); ++j) { pred.c[j] = 0; pred.h[j] = 0; }
    if ((uint32_t)ORDER > bs) return false;
    for (int j = 0; j < ORDER; ++j) {
        const int64_t s = br.get_signed((int)ebps);
        pred.push(s);
        if (!sink.put((uint32_t)j, s * ((int64_t)1 << wasted))) return false;
    }
    int shift = 0;
    if (lpc) {
        const uint32_t prec = br.get(4) + 1;
        if (prec == 16) return false;
        shift = br.get_signed(5);
        if (shift < 0) return false;
#pragma unroll
        for (int j = 0; j < ORDER; ++j) pred.c[j] = br.get_signed((int)prec);
    } else {
        // FIXED orders 1..4 as integer predictors: [1], [2,-1], [3,-3,1], [4,-6,4,-1] (binomial coefficients, alternating)
        int32_t binom = 1;
#pragma unroll
        for (int j = 0; j < ORDER; ++j) {
            binom = binom * (ORDER - j) / (j + 1);
            pred.c[j] = (j & 1) ? -binom : binom;
        }
        (void)fixed_order;
    }
    if (br.pos() > end_bits) return false;
    return rg_flac_residual(br, end_bits, bs, (uint32_t)ORDER, ebps, wasted, shift, pred, sink);
}

template <class Out>
RG_FLAC_HD bool rg_flac_predicted_ring(RgFlacBits &br, uint64_t end_bits, uint32_t bs, uint32_t order, uint32_t ebps, int wasted,
                                       int32_t *ring, int stride, RgFlacSink<Out> &sink) {
    RgFlacRing pred{ring, stride, order, 0};
    if (order > bs) return false;
    for (uint32_t j = 0; j < order; ++j) {
        const int64_t s = br.get_signed((int)ebps);
        pred.push(s);
        if (!sink.put(j, s * ((int64_t)1 << wasted))) return false;
    }
    const uint32_t prec = br.get(4) + 1;
    if (prec == 16) return false;
    const int shift = br.get_signed(5);
    if (shift < 0) return false;
    for (uint32_t j = 0; j < order; ++j) pred.coef(j) = br.get_signed((int)prec);
    if (br.pos() > end_bits) return false;
    return rg_flac_residual(br, end_bits, bs, order, ebps, wasted, shift, pred, sink);
}

// one subframe of `sbps` bits (the stream's, +1 for a side channel)
template <class Out>
RG_FLAC_HD bool rg_flac_subframe(RgFlacBits &br, uint64_t end_bits, uint32_t bs, uint32_t sbps, int32_t *ring, int stride,
                                 RgFlacSink<Out> &sink) {
    if (br.get(1) != 0) return false;
    const uint32_t type = br.get(6);
    int wasted = 0;
    if (br.get(1)) {
        uint32_t z;
        if (!br.unary(end_bits, &z)) return false;
        if (z + 1 >= sbps) return false;
        wasted = (int)z + 1;
    }
    const uint32_t ebps = sbps - (uint32_t)wasted;
    bool ok;
    if (type == 0) {  // CONSTANT
        const int64_t v = br.get_signed((int)ebps);
        ok = true;
        for (uint32_t i = 0; i < bs && ok; ++i) ok = sink.put(i, v * ((int64_t)1 << wasted));
    } else if (type == 1) {  // VERBATIM
        ok = true;
        for (uint32_t i = 0; i < bs && ok; ++i) {
            const int64_t v = br.get_signed((int)ebps);
            ok = sink.put(i, v * ((int64_t)1 << wasted));
            if ((i & 255u) == 255u && br.pos() > end_bits) return false;
        }
    } else if (type >= 8 && type <= 12) {  // FIXED
        switch (type - 8) {
            case 0: ok = rg_flac_predicted<0>(br, end_bits, bs, false, 0, ebps, wasted, sink); break;
            case 1: ok = rg_flac_predicted<1>(br, end_bits, bs, false, 1, ebps, wasted, sink); break;
            case 2: ok = rg_flac_predicted<2>(br, end_bits, bs, false, 2, ebps, wasted, sink); break;
            case 3: ok = rg_flac_predicted<3>(br, end_bits, bs, false, 3, ebps, wasted, sink); break;
            default: ok = rg_flac_predicted<4>(br, end_bits, bs, false, 4, ebps, wasted, sink); break;
        }
    } else if (type >= 32) {  // LPC
        const uint32_t order = type - 31;
        switch (order) {
            case 1: ok = rg_flac_predicted<1>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 2: ok = rg_flac_predicted<2>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 3: ok = rg_flac_predicted<3>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 4: ok = rg_flac_predicted<4>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 5: ok = rg_flac_predicted<5>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 6: ok = rg_flac_predicted<6>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 7: ok = rg_flac_predicted<7>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 8: ok = rg_flac_predicted<8>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 9: ok = rg_flac_predicted<9>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 10: ok = rg_flac_predicted<10>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 11: ok = rg_flac_predicted<11>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            case 12: ok = rg_flac_predicted<12>(br, end_bits, bs, true, 0, ebps, wasted, sink); break;
            default: ok = rg_flac_predicted_ring(br, end_bits, bs, order, ebps, wasted, ring, stride, sink); break;
        }
    } else {
        return false;  // reserved subframe types
    }
    return ok && br.pos() <= end_bits;
}

// A whole frame.  `data` / `limit`: the bytes the reader may touch; the frame is [off, off + len).  Returns true when it
// decoded (every sample of every channel written through `out`).  The CRC-16 is the caller's to check.
template <class Out>
RG_FLAC_HD bool rg_flac_decode_frame(const uint8_t *data, uint64_t limit, uint64_t off, uint32_t len, uint32_t header_len, uint32_t bs,
                                     uint32_t assign, uint32_t channels, uint32_t bps, int32_t *ring, int stride, Out &out) {
    if (len < header_len + 2) return false;
    const uint64_t end_bits = (off + len - 2) * 8;
    RgFlacBits br;
    br.init(data, limit, off + header_len);
    RgFlacSink<Out> sink{&out, RG_FLAC_SINK_DIRECT, 0, bps};
    // One call site of the subframe decoder (it is large: every order is a template), driven by a short plan per channel
    // assignment.  Right/side takes three steps: side parsed and discarded, right, side again from its saved position.
    const uint32_t steps = assign < 8 ? channels : (assign == 9 ? 3u : 2u);
    RgFlacBits side_at = br;
    for (uint32_t k = 0; k < steps; ++k) {
        uint32_t sbps = bps;
        if (assign < 8) {
            sink.mode = RG_FLAC_SINK_DIRECT;
            sink.ch = k;
        } else if (assign == 8 || assign == 10) {  // left/side, mid/side: the side channel second
            sink.mode = k == 0 ? RG_FLAC_SINK_DIRECT : (assign == 8 ? RG_FLAC_SINK_LS_SIDE : RG_FLAC_SINK_MS_SIDE);
            sink.ch = 0;
            sbps = bps + (k == 1 ? 1u : 0u);
        } else {  // right/side
            if (k == 0) side_at = br;
            if (k == 2) br = side_at;
            sink.mode = k == 0 ? RG_FLAC_SINK_DISCARD : (k == 1 ? RG_FLAC_SINK_DIRECT : RG_FLAC_SINK_RS_SIDE);
            sink.ch = 1;
            sbps = bps + (k == 1 ? 0u : 1u);
        }
        if (!rg_flac_subframe(br, end_bits, bs, sbps, ring, stride, sink)) return false;
    }
    return true;
}

#endif  // RG_FLAC_FRAME_H
