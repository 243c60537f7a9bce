// rg_flacenc.h -- internal: the FLAC encoder both halves share (include/mp3rgain_amd_flacenc.h has the definitions).  The
// kernels (rg_flacenc.hip) and the serial twin (rg_flacenc_host.cpp) run this very code: a frame is analysed and written by
// one function each, parametrised by an executor X that says how many lanes work on the frame (256 in a workgroup, 1 on the
// host), how they wait for one another and how a value is reduced or scanned across them.  Every quantity a choice depends
// on is an exact integer (the autocorrelation in 64 bits, the Rice sizes) or comes from one lane's double arithmetic in a
// fixed order with no libm call and no contraction, so the order of the lanes cannot change a byte.
//
// Plain C++ that also compiles under hipcc; no device and no context.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mp3rgain_amd.h"
#include "../../include/mp3rgain_amd_flacenc.h"
#include "rg_flac_frame.h"  // the CRC table entries

#define RG_FE_HD RG_FLAC_HD

#define RG_FE_MAX_BLOCK 4096u
#define RG_FE_PIECE 64u         // residuals per piece of the Rice sums
#define RG_FE_MAX_PIECES 64u
#define RG_FE_KS 32u            // row length of the sums: k = 0 .. 30 used
#define RG_FE_MAX_ORDER 12u
#define RG_FE_MAX_PORDER 6u
#define RG_FE_LANES 256u        // lanes of a workgroup
#define RG_FE_IMG_WORDS 3328u   // bit image of one subframe: 4096 x 25 bits, its header, the carried word, the frame header
#define RG_FE_SIG_MID 8u
#define RG_FE_SIG_SIDE 9u

enum { RG_FE_CONSTANT = 0, RG_FE_VERBATIM = 1, RG_FE_FIXED = 2, RG_FE_LPC = 3 };

// ---- records ---------------------------------------------------------------------------------------------------------------
struct RgFeSub {       // the decision for one subframe
    uint8_t type;      // RG_FE_*
    uint8_t order;     // FIXED 0-4, LPC 2-12
    uint8_t wasted;    // bits removed from every sample
    uint8_t shift;     // LPC quantisation shift
    uint8_t precision; // LPC coefficient bits
    uint8_t porder;    // partition order
    uint8_t signal;    // channel 0-7, RG_FE_SIG_MID, RG_FE_SIG_SIDE
    uint8_t sbps;      // bits of the signal before the wasted bits are removed
    uint32_t bits;     // the whole subframe
    int16_t coef[RG_FE_MAX_ORDER];
    uint8_t param[1u << RG_FE_MAX_PORDER];
};  // 100 bytes

struct RgFeFrame {     // the decision record of one frame
    uint32_t bytes;    // frame length: header, subframes padded to a byte, CRC-16
    uint32_t block;    // samples per channel
    uint8_t assignment, nsub, header_bytes, reserved;
    RgFeSub sub[8];
};  // 812 bytes

struct RgFeStream {                // one stream of a call
    const unsigned char *plane0;   // plane c at plane0 + c * frames * elem_bytes
    uint64_t frames;               // PCM frames per channel
    uint64_t first_frame;          // index of its first FLAC frame among all frames of the call
    uint64_t audio_at;             // where its first frame goes, from the output's base
    uint32_t n_frames;             // FLAC frames
    uint32_t rate, channels, bps, elem_bytes, shift;
    uint32_t block, max_lpc;
    uint32_t meta_bytes;           // bytes in front of its first frame
    uint32_t reserved;
};

// ---- small things ----------------------------------------------------------------------------------------------------------
RG_FE_HD uint32_t rg_fe_frames_of(uint64_t pcm_frames, uint32_t block) { return (uint32_t)((pcm_frames + block - 1) / block); }
RG_FE_HD bool rg_fe_block_ok(uint32_t b) { return b == 256 || b == 512 || b == 1024 || b == 2048 || b == 4096; }
// the width that decides the residual method and the coefficient precision: the signal's own after its wasted bits are
// removed, the side signal counted as its channels (one bit less), so 16-bit audio padded to 24 is coded as 16-bit audio is
RG_FE_HD uint32_t rg_fe_width(uint32_t sbps, uint32_t wasted, uint32_t signal) { return sbps - wasted - (signal == RG_FE_SIG_SIDE ? 1u : 0u); }
RG_FE_HD bool rg_fe_rice2(uint32_t width) { return width > 16; }
RG_FE_HD uint32_t rg_fe_ctz(uint32_t v) {  // v != 0
    uint32_t n = 0;
    while (!(v & 1u)) {
        v >>= 1;
        ++n;
    }
    return n;
}

RG_FE_HD int32_t rg_fe_sample(const RgFeStream &s, uint32_t ch, uint64_t i) {
    const unsigned char *p = s.plane0 + ((uint64_t)ch * s.frames + i) * s.elem_bytes;
    if (s.elem_bytes == 2) return (int32_t) * reinterpret_cast<const int16_t *>(p) >> s.shift;
    return *reinterpret_cast<const int32_t *>(p) >> s.shift;
}
// sample i of a frame's signal: a channel, mid or side
RG_FE_HD int32_t rg_fe_signal_at(const RgFeStream &s, uint32_t signal, uint64_t i) {
    if (signal < 8) return rg_fe_sample(s, signal, i);
    const int32_t l = rg_fe_sample(s, 0, i), r = rg_fe_sample(s, 1, i);
    return signal == RG_FE_SIG_MID ? (l + r) >> 1 : l - r;
}

// The integer Welch window: 15-bit weights, w(i) = floor(32767 (N^2 - d^2) / N^2) with N = n - 1, d = 2 i - N  (n >= 2)
RG_FE_HD int32_t rg_fe_window(uint32_t i, uint32_t n) {
    const int64_t N = (int64_t)n - 1, d = 2 * (int64_t)i - N;
    const uint64_t nn = (uint64_t)(N * N);
    return (int32_t)((32767ull * (nn - (uint64_t)(d * d))) / nn);
}

// the frame header into h[16] -> its length, CRC-8 included
RG_FE_HD uint32_t rg_fe_frame_header(uint8_t *h, uint32_t n, uint32_t rate, uint32_t assignment, uint32_t bps, uint64_t number) {
    uint32_t at = 0, bcode, rcode, scode = 0;
    h[at++] = 0xFF;
    h[at++] = 0xF8;
    if (n >= 256 && n <= 4096 && !(n & (n - 1))) bcode = 8 + rg_fe_ctz(n >> 8);
    else bcode = n <= 256 ? 6 : 7;
    switch (rate) {
        case 88200: rcode = 1; break;
        case 176400: rcode = 2; break;
        case 192000: rcode = 3; break;
        case 8000: rcode = 4; break;
        case 16000: rcode = 5; break;
        case 22050: rcode = 6; break;
        case 24000: rcode = 7; break;
        case 32000: rcode = 8; break;
        case 44100: rcode = 9; break;
        case 48000: rcode = 10; break;
        case 96000: rcode = 11; break;
        default:
            if (rate % 1000 == 0 && rate / 1000 < 256) rcode = 12;
            else if (rate < 65536) rcode = 13;
            else if (rate % 10 == 0 && rate / 10 < 65536) rcode = 14;
            else rcode = 0;  // from STREAMINFO
    }
    switch (bps) {
        case 8: scode = 1; break;
        case 12: scode = 2; break;
        case 16: scode = 4; break;
        case 20: scode = 5; break;
        case 24: scode = 6; break;
        default: scode = 0;  // from STREAMINFO
    }
    h[at++] = (uint8_t)((bcode << 4) | rcode);
    h[at++] = (uint8_t)((assignment << 4) | (scode << 1));
    if (number < 0x80) h[at++] = (uint8_t)number;
    else {
        uint32_t extra = 1;
        while (extra < 6 && number >= ((uint64_t)1 << (6 + 5 * extra))) ++extra;  // 11, 16, 21, 26, 31, 36 bits
        h[at++] = (uint8_t)((0xFF00u >> (extra + 1)) | (uint32_t)(number >> (6 * extra)));
        for (uint32_t k = extra; k-- > 0;) h[at++] = (uint8_t)(0x80u | ((number >> (6 * k)) & 0x3Fu));
    }
    if (bcode == 6) h[at++] = (uint8_t)(n - 1);
    if (bcode == 7) {
        h[at++] = (uint8_t)((n - 1) >> 8);
        h[at++] = (uint8_t)(n - 1);
    }
    if (rcode == 12) h[at++] = (uint8_t)(rate / 1000);
    if (rcode == 13 || rcode == 14) {
        const uint32_t v = rcode == 13 ? rate : rate / 10;
        h[at++] = (uint8_t)(v >> 8);
        h[at++] = (uint8_t)v;
    }
    uint32_t c = 0;
    for (uint32_t k = 0; k < at; ++k) c = rg_flac_crc8_entry(c ^ h[k]);
    h[at++] = (uint8_t)c;
    return at;
}

// CRC-16 (0x8005, MSB first): a * b mod P, residues as the register holds them
RG_FE_HD uint32_t rg_fe_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 15; i >= 0; --i) {
        p = (p & 0x8000u) ? ((p << 1) ^ 0x8005u) & 0xFFFFu : (p << 1);
        if ((a >> i) & 1u) p ^= b;
    }
    return p;
}
RG_FE_HD uint32_t rg_fe_crc_byte(uint32_t crc, uint32_t byte, const uint16_t *t) { return ((crc << 8) & 0xFFFFu) ^ t[((crc >> 8) ^ byte) & 0xFFu]; }

// ---- the analysis of a frame ---------------------------------------------------------------------------------------------
struct RgFeWork {
    int32_t sig[RG_FE_MAX_BLOCK];                // the signal, wasted bits removed
    uint32_t u[RG_FE_MAX_BLOCK];                 // zig-zag residuals; before them the windowed signal
    uint64_t piece[RG_FE_MAX_PIECES][RG_FE_KS];  // sum of u >> k over a piece
    uint64_t red[4];
    uint64_t pbits[(2u << RG_FE_MAX_PORDER) - 1];
    uint8_t pk[(2u << RG_FE_MAX_PORDER) - 1];
    int64_t acf[RG_FE_MAX_ORDER + 1];
    double lp[RG_FE_MAX_ORDER], tmp[RG_FE_MAX_ORDER];
    double lpc[RG_FE_MAX_ORDER / 2][RG_FE_MAX_ORDER];
    int32_t qc[RG_FE_MAX_ORDER / 2][RG_FE_MAX_ORDER];
    int32_t qshift[RG_FE_MAX_ORDER / 2];
    uint32_t lpc_orders;  // even orders 2 .. 2 * lpc_orders came out of the recursion
    uint32_t qok[RG_FE_MAX_ORDER / 2];
    RgFeSub cand, best;
    RgFeSub keep[4];  // two channels: left, right, mid, side
    uint8_t hdr[16];
};

// the serial executor: one lane
struct RgFeSerial {
    RG_FE_HD uint32_t tid() const { return 0; }
    RG_FE_HD uint32_t nt() const { return 1; }
    RG_FE_HD void sync() const {}
    RG_FE_HD uint64_t sum(uint64_t v, uint64_t *) const { return v; }
    RG_FE_HD uint64_t any(uint64_t v, uint64_t *) const { return v; }  // bitwise OR
};

RG_FE_HD uint32_t rg_fe_zigzag(int64_t r) { return (uint32_t)(((uint64_t)r << 1) ^ (uint64_t)(r >> 63)); }
RG_FE_HD bool rg_fe_res_fits(int64_t r) { return r > -2147483648ll && r <= 2147483647ll; }

// residual of sample i (i >= order) under a FIXED predictor
RG_FE_HD int64_t rg_fe_fixed_res(const int32_t *x, uint32_t i, uint32_t order) {
    switch (order) {
        case 0: return x[i];
        case 1: return (int64_t)x[i] - x[i - 1];
        case 2: return (int64_t)x[i] - 2 * (int64_t)x[i - 1] + x[i - 2];
        case 3: return (int64_t)x[i] - 3 * (int64_t)x[i - 1] + 3 * (int64_t)x[i - 2] - x[i - 3];
        default: return (int64_t)x[i] - 4 * (int64_t)x[i - 1] + 6 * (int64_t)x[i - 2] - 4 * (int64_t)x[i - 3] + x[i - 4];
    }
}
RG_FE_HD int64_t rg_fe_lpc_res(const int32_t *x, uint32_t i, uint32_t order, const int32_t *c, int shift) {
    int64_t s = 0;
    for (uint32_t j = 0; j < order; ++j) s += (int64_t)c[j] * x[i - 1 - j];
    return (int64_t)x[i] - (s >> shift);
}
RG_FE_HD int64_t rg_fe_sub_res(const int32_t *x, uint32_t i, const RgFeSub &sub, const int32_t *c) {
    return sub.type == RG_FE_FIXED ? rg_fe_fixed_res(x, i, sub.order) : rg_fe_lpc_res(x, i, sub.order, c, sub.shift);
}

// largest partition order of a block of n samples: partitions are whole pieces
RG_FE_HD uint32_t rg_fe_max_porder(uint32_t n) {
    uint32_t p = 0;
    while (p < RG_FE_MAX_PORDER && !(n & ((RG_FE_PIECE << (p + 1)) - 1))) ++p;
    return p;
}

// The exact size of the residual of w.u[order .. n) (w.u[0 .. order) and w.u[n .. pieces) are 0): the best parameter of
// every partition of every order, then the best order -> w.cand.porder, .param and the bits in w.cand.bits (added to it).
template <class X>
RG_FE_HD void rg_fe_rice(X &x, RgFeWork &w, uint32_t n, uint32_t order, bool rice2) {
    const uint32_t kmax = rice2 ? 30u : 14u, pb = rice2 ? 5u : 4u;
    const uint32_t pieces = (n + RG_FE_PIECE - 1) / RG_FE_PIECE;
    x.sync();
    for (uint32_t t = x.tid(); t < pieces * RG_FE_KS; t += x.nt()) {
        const uint32_t p = t / RG_FE_KS, k = t % RG_FE_KS;
        if (k > kmax) continue;
        uint64_t s = 0;
        for (uint32_t i = 0; i < RG_FE_PIECE; ++i) s += w.u[p * RG_FE_PIECE + i] >> k;
        w.piece[p][k] = s;
    }
    x.sync();
    const uint32_t maxp = rg_fe_max_porder(n);
    for (uint32_t node = x.tid(); node < (2u << maxp) - 1; node += x.nt()) {
        uint32_t p = 0;
        while (node >= (2u << p) - 1) ++p;
        const uint32_t j = node - ((1u << p) - 1);
        const uint32_t m = p ? (n >> p) / RG_FE_PIECE : pieces;  // pieces of this partition
        const uint64_t cnt = (p ? n >> p : n) - (j ? 0 : order);
        uint64_t best = ~(uint64_t)0;
        uint32_t bk = 0;
        for (uint32_t k = 0; k <= kmax; ++k) {
            uint64_t s = cnt * (k + 1);
            for (uint32_t q = 0; q < m; ++q) s += w.piece[j * m + q][k];
            if (s < best) {
                best = s;
                bk = k;
            }
        }
        w.pbits[node] = best;
        w.pk[node] = (uint8_t)bk;
    }
    x.sync();
    if (x.tid() == 0) {
        uint64_t best = ~(uint64_t)0;
        uint32_t bp = 0;
        for (uint32_t p = 0; p <= maxp; ++p) {
            uint64_t s = (uint64_t)pb << p;
            for (uint32_t j = 0; j < (1u << p); ++j) s += w.pbits[(1u << p) - 1 + j];
            if (s < best) {
                best = s;
                bp = p;
            }
        }
        w.cand.porder = (uint8_t)bp;
        for (uint32_t j = 0; j < (1u << bp); ++j) w.cand.param[j] = w.pk[(1u << bp) - 1 + j];
        const uint64_t total = (uint64_t)w.cand.bits + best;
        w.cand.bits = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;
        if (w.cand.bits < w.best.bits) w.best = w.cand;  // ties: the earlier candidate stays
    }
    x.sync();
}

// one predicted candidate: w.cand holds type, order, (shift, precision, coef) and the bits in front of the residual
template <class X>
RG_FE_HD void rg_fe_try(X &x, RgFeWork &w, uint32_t n, const int32_t *c, bool rice2) {
    const uint32_t order = w.cand.order, pieces = (n + RG_FE_PIECE - 1) / RG_FE_PIECE;
    uint64_t bad = 0;
    for (uint32_t i = x.tid(); i < pieces * RG_FE_PIECE; i += x.nt()) {
        uint32_t u = 0;
        if (i >= order && i < n) {
            const int64_t r = rg_fe_sub_res(w.sig, i, w.cand, c);
            if (!rg_fe_res_fits(r)) bad = 1;
            u = rg_fe_zigzag(r);
        }
        w.u[i] = u;
    }
    bad = x.any(bad, w.red);
    if (bad) return;  // the residual does not fit 32 bits: not a candidate
    rg_fe_rice(x, w, n, order, rice2);
}

// One step of the Levinson-Durbin recursion: order i -> i + 1 over lp[0 .. i] (tmp: scratch of i values); `err` is the
// prediction error before the step, the return value the one after it.  The click scan (rg_clicks.h) runs these very steps.
RG_FE_HD double rg_fe_levinson_step(const int64_t *acf, double *lp, double *tmp, uint32_t i, double err) {
    double acc = (double)acf[i + 1];
    for (uint32_t j = 0; j < i; ++j) acc = acc - lp[j] * (double)acf[i - j];
    const double k = acc / err;
    for (uint32_t j = 0; j < i; ++j) tmp[j] = lp[j] - k * lp[i - 1 - j];
    for (uint32_t j = 0; j < i; ++j) lp[j] = tmp[j];
    lp[i] = k;
    return err * (1.0 - k * k);
}

// Levinson-Durbin on one lane: w.acf[0 .. maxo] -> w.lpc[o / 2 - 1][0 .. o) for the even orders o, w.lpc_orders of them
RG_FE_HD void rg_fe_levinson(RgFeWork &w, uint32_t maxo) {
    w.lpc_orders = 0;
    if (w.acf[0] <= 0) return;
    double err = (double)w.acf[0];
    for (uint32_t i = 0; i < maxo; ++i) {
        err = rg_fe_levinson_step(w.acf, w.lp, w.tmp, i, err);
        if ((i & 1u) == 1u) {
            for (uint32_t j = 0; j <= i; ++j) w.lpc[i / 2][j] = w.lp[j];
            w.lpc_orders = i / 2 + 1;
        }
        if (!(err > 0.0)) break;
    }
}

// quantise lpc[0 .. order) to `precision` bits: the shift from the largest coefficient's exponent bits, rounding with error
// feedback -> qc[0 .. order) and *qshift; false when there is no such quantisation
RG_FE_HD bool rg_fe_quantise_to(const double *lpc, uint32_t order, uint32_t precision, int32_t *qc, int32_t *qshift) {
    uint64_t top = 0;  // the largest magnitude's bit pattern: for finite doubles the patterns order as the values do
    for (uint32_t j = 0; j < order; ++j) {
        uint64_t b;
        const double c = lpc[j];
        memcpy(&b, &c, 8);
        b &= 0x7FFFFFFFFFFFFFFFull;
        if ((b >> 52) == 0x7FFu) return false;
        if (b > top) top = b;
    }
    const int e = (int)(top >> 52) - 1022;  // |c| = m 2^e, 0.5 <= m < 1
    if ((top >> 52) == 0) return false;
    int shift = (int)precision - 1 - e;
    if (shift > 15) shift = 15;
    if (shift < 0) return false;
    const double scale = (double)(1u << shift);
    const int64_t hi = ((int64_t)1 << (precision - 1)) - 1, lo = -hi - 1;
    double err = 0.0;
    for (uint32_t j = 0; j < order; ++j) {
        err = err + lpc[j] * scale;
        int64_t q = err >= 0.0 ? (int64_t)(err + 0.5) : -(int64_t)(0.5 - err);
        if (q > hi) q = hi;
        if (q < lo) q = lo;
        err = err - (double)q;
        qc[j] = (int32_t)q;
    }
    *qshift = shift;
    return true;
}
// ... w.lpc[oi] -> w.qc[oi], w.qshift[oi], w.qok[oi]
RG_FE_HD void rg_fe_quantise(RgFeWork &w, uint32_t oi, uint32_t precision) {
    w.qok[oi] = rg_fe_quantise_to(w.lpc[oi], 2 * oi + 2, precision, w.qc[oi], &w.qshift[oi]) ? 1u : 0u;
}

// The search over one signal: w.sig[0 .. n) holds it (sbps bits) -> w.best.  Candidates in this order, the earlier one
// kept on a tie: CONSTANT, VERBATIM, FIXED 0 .. 4, LPC 2, 4, .. max_lpc.
template <class X>
RG_FE_HD void rg_fe_search(X &x, RgFeWork &w, uint32_t n, uint32_t sbps, uint32_t signal, uint32_t max_lpc) {
    x.sync();
    uint64_t acc = 0;
    const int32_t first = w.sig[0];
    for (uint32_t i = x.tid(); i < n; i += x.nt()) acc |= (uint64_t)(uint32_t)w.sig[i] | ((uint64_t)(uint32_t)(w.sig[i] ^ first) << 32);
    acc = x.any(acc, w.red);
    const uint32_t ored = (uint32_t)acc, wasted = ored ? rg_fe_ctz(ored) : 0u;
    const bool constant = (acc >> 32) == 0;
    const uint32_t ebps = sbps - wasted, head = 8 + wasted;
    const uint32_t width = rg_fe_width(sbps, wasted, signal);
    const bool rice2 = rg_fe_rice2(width);
    if (wasted) {
        for (uint32_t i = x.tid(); i < n; i += x.nt()) w.sig[i] >>= wasted;
    }
    if (x.tid() == 0) {
        memset(&w.best, 0, sizeof w.best);
        w.best.type = constant ? RG_FE_CONSTANT : RG_FE_VERBATIM;
        w.best.wasted = (uint8_t)wasted;
        w.best.signal = (uint8_t)signal;
        w.best.sbps = (uint8_t)sbps;
        w.best.bits = head + (constant ? ebps : n * ebps);
    }
    x.sync();
    if (constant) return;
    for (uint32_t order = 0; order <= 4 && order < n; ++order) {
        if (x.tid() == 0) {
            w.cand = w.best;
            w.cand.type = RG_FE_FIXED;
            w.cand.order = (uint8_t)order;
            w.cand.bits = head + order * ebps + 6;
        }
        x.sync();
        rg_fe_try(x, w, n, nullptr, rice2);
    }
    uint32_t maxo = max_lpc > RG_FE_MAX_ORDER ? RG_FE_MAX_ORDER : max_lpc;
    maxo &= ~1u;
    while (maxo && maxo >= n) maxo -= 2;
    if (!maxo) return;
    // the windowed signal, then its autocorrelation: exact, so the lanes may add in any order
    int32_t *xw = reinterpret_cast<int32_t *>(w.u);
    for (uint32_t i = x.tid(); i < n; i += x.nt()) xw[i] = (int32_t)(((int64_t)w.sig[i] * rg_fe_window(i, n)) >> 15);
    x.sync();
    int64_t r[RG_FE_MAX_ORDER + 1];
#pragma unroll
    for (uint32_t l = 0; l <= RG_FE_MAX_ORDER; ++l) r[l] = 0;
    for (uint32_t i = x.tid(); i < n; i += x.nt()) {
        const int64_t v = xw[i];
#pragma unroll
        for (uint32_t l = 0; l <= RG_FE_MAX_ORDER; ++l)
            if (l <= maxo && l <= i) r[l] += v * xw[i - l];
    }
#pragma unroll
    for (uint32_t l = 0; l <= RG_FE_MAX_ORDER; ++l) {
        const uint64_t s = x.sum((uint64_t)r[l], w.red);
        if (x.tid() == 0) w.acf[l] = (int64_t)s;
    }
    const uint32_t precision = width <= 16 ? 12u : 15u;
    if (x.tid() == 0) {
        rg_fe_levinson(w, maxo);
        for (uint32_t oi = 0; oi < w.lpc_orders; ++oi) rg_fe_quantise(w, oi, precision);
    }
    x.sync();
    const uint32_t orders = w.lpc_orders;
    for (uint32_t oi = 0; oi < orders; ++oi) {
        if (!w.qok[oi]) continue;
        const uint32_t order = 2 * oi + 2;
        if (x.tid() == 0) {
            w.cand = w.best;
            w.cand.type = RG_FE_LPC;
            w.cand.order = (uint8_t)order;
            w.cand.shift = (uint8_t)w.qshift[oi];
            w.cand.precision = (uint8_t)precision;
            for (uint32_t j = 0; j < RG_FE_MAX_ORDER; ++j) w.cand.coef[j] = j < order ? (int16_t)w.qc[oi][j] : (int16_t)0;
            w.cand.bits = head + order * ebps + 4 + 5 + order * precision + 6;
        }
        x.sync();
        rg_fe_try(x, w, n, w.qc[oi], rice2);
    }
}

template <class X>
RG_FE_HD void rg_fe_load_signal(X &x, int32_t *sig, const RgFeStream &s, uint32_t signal, uint64_t first, uint32_t n) {
    x.sync();
    for (uint32_t i = x.tid(); i < n; i += x.nt()) sig[i] = rg_fe_signal_at(s, signal, first + i);
    x.sync();
}

// Frame f of stream s -> its decision record.  Two channels: the cheapest of L/R, L/S, R/S and M/S, the earlier one on a tie.
template <class X>
RG_FE_HD void rg_fe_analyse_frame(X &x, RgFeWork &w, const RgFeStream &s, uint32_t f, RgFeFrame *out) {
    const uint64_t first = (uint64_t)f * s.block;
    const uint32_t n = (uint32_t)(s.frames - first < s.block ? s.frames - first : s.block);
    uint64_t bits = 0;
    uint32_t assignment = s.channels - 1;
    if (s.channels == 2) {
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t signal = k < 2 ? k : RG_FE_SIG_MID + (k - 2);  // left, right, mid, side
            rg_fe_load_signal(x, w.sig, s, signal, first, n);
            rg_fe_search(x, w, n, s.bps + (k == 3 ? 1u : 0u), signal, s.max_lpc);
            x.sync();
            if (x.tid() == 0) w.keep[k] = w.best;
            x.sync();
        }
        const uint64_t l = w.keep[0].bits, r = w.keep[1].bits, m = w.keep[2].bits, sd = w.keep[3].bits;
        uint32_t a = 0, b = 1;
        bits = l + r;
        if (l + sd < bits) bits = l + sd, a = 0, b = 3, assignment = 8;
        if (sd + r < bits) bits = sd + r, a = 3, b = 1, assignment = 9;
        if (m + sd < bits) bits = m + sd, a = 2, b = 3, assignment = 10;
        if (x.tid() == 0) {
            out->sub[0] = w.keep[a];
            out->sub[1] = w.keep[b];
        }
    } else {
        for (uint32_t c = 0; c < s.channels; ++c) {
            rg_fe_load_signal(x, w.sig, s, c, first, n);
            rg_fe_search(x, w, n, s.bps, c, s.max_lpc);
            x.sync();
            bits += w.best.bits;
            if (x.tid() == 0) out->sub[c] = w.best;
            x.sync();
        }
    }
    if (x.tid() == 0) {
        const uint32_t hl = rg_fe_frame_header(w.hdr, n, s.rate, assignment, s.bps, f);
        out->bytes = hl + (uint32_t)((bits + 7) / 8) + 2;
        out->block = n;
        out->assignment = (uint8_t)assignment;
        out->nsub = (uint8_t)s.channels;
        out->header_bytes = (uint8_t)hl;
        out->reserved = 0;
        for (uint32_t c = s.channels; c < 8; ++c) memset(&out->sub[c], 0, sizeof(RgFeSub));
    }
}

// ---- writing a frame -----------------------------------------------------------------------------------------------------
struct RgFeWriteWork {
    int32_t sig[RG_FE_MAX_BLOCK];
    uint32_t u[RG_FE_MAX_BLOCK];
    uint32_t img[RG_FE_IMG_WORDS];  // big-endian bit image: bit 0 is the top bit of word 0
    uint32_t scan[RG_FE_LANES];
    uint32_t chunk[RG_FE_LANES];    // CRC-16 of each lane's chunk
    uint32_t x512[8];               // x^(512 * 2^l) mod P
    uint16_t crc_table[256];
    int32_t coef[RG_FE_MAX_ORDER];
    uint32_t fail;                  // a position left the image or the frame (it must not)
    uint8_t hdr[16];
};

// the serial executor of the write: plain stores, a serial CRC
struct RgFeSerialWrite : RgFeSerial {
    RG_FE_HD void or_word(uint32_t *p, uint32_t v) const { *p |= v; }
    RG_FE_HD uint32_t exscan(uint32_t, RgFeWriteWork &) const { return 0; }
    RG_FE_HD uint32_t crc(RgFeWriteWork &w, uint32_t nbytes, uint32_t crc) const {
        for (uint32_t b = 0; b < nbytes; ++b) crc = rg_fe_crc_byte(crc, (w.img[b >> 2] >> (24 - 8 * (b & 3u))) & 0xFFu, w.crc_table);
        return crc;
    }
};

// `len` (1 .. 32) bits of v at bit `pos` of the image
template <class X>
RG_FE_HD void rg_fe_put(X &x, RgFeWriteWork &w, uint32_t pos, uint32_t v, uint32_t len) {
    const uint32_t word = pos >> 5, off = pos & 31u;
    if (len < 32) v &= (1u << len) - 1;
    if (word + 1 >= RG_FE_IMG_WORDS) {
        w.fail = 1;
        return;
    }
    if (off + len <= 32) x.or_word(&w.img[word], v << (32 - off - len));
    else {
        const uint32_t low = off + len - 32;  // bits that go to the next word
        x.or_word(&w.img[word], v >> low);
        x.or_word(&w.img[word + 1], v << (32 - low));
    }
}

template <class X>
RG_FE_HD void rg_fe_write_init(X &x, RgFeWriteWork &w) {
    for (uint32_t b = x.tid(); b < 256; b += x.nt()) w.crc_table[b] = rg_flac_crc16_entry(b);
    if (x.tid() == 0) {
        w.fail = 0;
        uint32_t r = 1;  // x^0; a zero byte multiplies the register by x^8 (the table is not complete yet: from the entries)
        for (uint32_t k = 0; k < 64; ++k) r = ((r << 8) & 0xFFFFu) ^ rg_flac_crc16_entry((r >> 8) & 0xFFu);
        for (uint32_t l = 0; l < 8; ++l) {
            w.x512[l] = r;
            r = rg_fe_crc_mul(r, r);
        }
    }
    x.sync();
}

// Frame f of stream s from its record -> rec.bytes bytes at dst.  Subframes are bit-contiguous: the image holds one
// subframe at a time, its whole words go out and the partial last word is carried into the next image.
template <class X>
RG_FE_HD void rg_fe_write_frame(X &x, RgFeWriteWork &w, const RgFeStream &s, uint32_t f, const RgFeFrame &rec, uint8_t *dst) {
    const uint64_t first = (uint64_t)f * s.block;
    const uint32_t n = rec.block;
    x.sync();
    for (uint32_t i = x.tid(); i < RG_FE_IMG_WORDS; i += x.nt()) w.img[i] = 0;
    x.sync();
    if (x.tid() == 0) {
        const uint32_t hl = rg_fe_frame_header(w.hdr, n, s.rate, rec.assignment, s.bps, f);
        for (uint32_t k = 0; k < hl; ++k) rg_fe_put(x, w, 8 * k, w.hdr[k], 8);
    }
    uint32_t P = 8u * rec.header_bytes, base = 0, crc = 0;
    for (uint32_t si = 0; si < rec.nsub; ++si) {
        const RgFeSub &sub = rec.sub[si];
        const uint32_t wasted = sub.wasted, ebps = sub.sbps - wasted, order = sub.order;
        const bool rice2 = rg_fe_rice2(rg_fe_width(sub.sbps, wasted, sub.signal));
        const uint32_t pb = rice2 ? 5u : 4u;
        x.sync();
        for (uint32_t i = x.tid(); i < n; i += x.nt()) w.sig[i] = rg_fe_signal_at(s, sub.signal, first + i) >> wasted;
        if (x.tid() < RG_FE_MAX_ORDER) w.coef[x.tid()] = sub.coef[x.tid()];
        if (x.nt() == 1)
            for (uint32_t j = 0; j < RG_FE_MAX_ORDER; ++j) w.coef[j] = sub.coef[j];
        x.sync();
        const bool predicted = sub.type == RG_FE_FIXED || sub.type == RG_FE_LPC;
        if (predicted) {
            for (uint32_t i = x.tid(); i < n; i += x.nt()) w.u[i] = i >= order ? rg_fe_zigzag(rg_fe_sub_res(w.sig, i, sub, w.coef)) : 0u;
        }
        const uint32_t hb = 8 + wasted;
        if (x.tid() == 0) {
            const uint32_t code = sub.type == RG_FE_CONSTANT ? 0u : sub.type == RG_FE_VERBATIM ? 1u : sub.type == RG_FE_FIXED ? 8u + order : 31u + order;
            rg_fe_put(x, w, P, (code << 1) | (wasted ? 1u : 0u), 8);
            if (wasted) rg_fe_put(x, w, P + 8, 1, wasted);
            if (sub.type == RG_FE_CONSTANT) rg_fe_put(x, w, P + hb, (uint32_t)w.sig[0], ebps);
        }
        uint32_t end = P + hb + ebps;  // CONSTANT
        if (sub.type == RG_FE_VERBATIM) {
            for (uint32_t i = x.tid(); i < n; i += x.nt()) rg_fe_put(x, w, P + hb + i * ebps, (uint32_t)w.sig[i], ebps);
            end = P + hb + n * ebps;
        } else if (predicted) {
            for (uint32_t i = x.tid(); i < order; i += x.nt()) rg_fe_put(x, w, P + hb + i * ebps, (uint32_t)w.sig[i], ebps);
            uint32_t q = P + hb + order * ebps;
            if (sub.type == RG_FE_LPC) {
                if (x.tid() == 0) {
                    rg_fe_put(x, w, q, sub.precision - 1u, 4);
                    rg_fe_put(x, w, q + 4, sub.shift, 5);
                    for (uint32_t j = 0; j < order; ++j) rg_fe_put(x, w, q + 9 + j * sub.precision, (uint32_t)(int32_t)sub.coef[j], sub.precision);
                }
                q += 9 + order * sub.precision;
            }
            if (x.tid() == 0) {
                rg_fe_put(x, w, q, rice2 ? 1u : 0u, 2);
                rg_fe_put(x, w, q + 2, sub.porder, 4);
            }
            q += 6;
            x.sync();
            // lanes own runs of consecutive residuals; a scan of the runs' lengths places every code
            const uint32_t per = (n + x.nt() - 1) / x.nt(), plen = n >> sub.porder;
            const uint32_t a = x.tid() * per < n ? x.tid() * per : n, b = a + per < n ? a + per : n;
            uint32_t mine = 0;
            for (uint32_t i = a < order ? order : a; i < b; ++i) {
                const uint32_t j = sub.porder ? i / plen : 0u, k = sub.param[j];
                mine += (w.u[i] >> k) + 1 + k + (i == (j ? j * plen : order) ? pb : 0u);
            }
            uint32_t pos = q + x.exscan(mine, w);
            for (uint32_t i = a < order ? order : a; i < b; ++i) {
                const uint32_t j = sub.porder ? i / plen : 0u, k = sub.param[j];
                if (i == (j ? j * plen : order)) {
                    rg_fe_put(x, w, pos, k, pb);
                    pos += pb;
                }
                const uint32_t hi = w.u[i] >> k;
                rg_fe_put(x, w, pos + hi, (1u << k) | (w.u[i] & ((1u << k) - 1)), k + 1);  // the unary run costs only its stop bit
                pos += hi + 1 + k;
            }
            end = P + sub.bits;
            if (x.tid() == x.nt() - 1 && pos != end && b == n) w.fail = 1;
        }
        x.sync();
        // whole words out (the last subframe: every byte, padded with zero bits), the CRC-16 over them, the rest carried
        const bool last = si + 1 == rec.nsub;
        uint32_t nbytes = last ? (end + 7) / 8 : (end >> 5) * 4;
        if (nbytes >= 4 * RG_FE_IMG_WORDS) {  // a record no analysis writes: nothing is read or stored beyond the image
            if (x.tid() == 0) w.fail = 1;
            nbytes = 0;
        }
        const bool inside = (uint64_t)base + nbytes + 2 <= rec.bytes;
        if (!inside && x.tid() == 0) w.fail = 1;
        if (inside)
            for (uint32_t b = x.tid(); b < nbytes; b += x.nt()) dst[base + b] = (uint8_t)(w.img[b >> 2] >> (24 - 8 * (b & 3u)));
        crc = x.crc(w, nbytes, crc);
        x.sync();
        const uint32_t carry = last ? 0u : w.img[nbytes >> 2];
        x.sync();
        for (uint32_t i = x.tid(); i < RG_FE_IMG_WORDS; i += x.nt()) w.img[i] = i ? 0u : carry;
        P = end - 8 * nbytes;
        base += nbytes;
    }
    x.sync();
    if (x.tid() == 0 && (uint64_t)base + 2 <= rec.bytes) {
        if (base + 2 != rec.bytes) w.fail = 1;
        dst[base] = (uint8_t)(crc >> 8);
        dst[base + 1] = (uint8_t)crc;
    }
}

// ---- host side (rg_flacenc_host.cpp) -----------------------------------------------------------------------------------------
#define RG_FE_VENDOR "mp3rgain_amd flacenc 1"
// bytes in front of the first frame: "fLaC", STREAMINFO, one VORBIS_COMMENT block with the vendor string and no comments
inline uint64_t rg_fe_metadata_bytes() { return 4 + 4 + 34 + 4 + 4 + (sizeof(RG_FE_VENDOR) - 1) + 4; }

// options (NULL = defaults) -> block and max_lpc; RG_ERR_INVALID_ARG with a text
int rg_fe_options(const rg_flac_encode_options *o, uint32_t *block, uint32_t *max_lpc, uint32_t *flags, char *err, size_t err_len);
// stream i of a seam call against the arena at `base` (host or device memory; only its address is used)
int rg_fe_stream(size_t i, const rg_track_desc &t, uint32_t bps, const unsigned char *base, size_t arena_bytes, uint32_t block, uint32_t max_lpc,
                 RgFeStream *out, char *err, size_t err_len);
// The metadata of stream s into dst[s.meta_bytes], and its result record.  blocks: the metadata blocks behind STREAMINFO as
// they go into the stream (s.meta_bytes = 42 + blocks_len), or NULL: the VORBIS_COMMENT block with the vendor string.
void rg_fe_finish_stream(const RgFeStream &s, uint32_t min_frame, uint32_t max_frame, uint64_t audio_bytes, const uint8_t md5[16], uint8_t *dst,
                         rg_flac_encode_result *res, const uint8_t *blocks = nullptr, size_t blocks_len = 0);
// The blocks behind STREAMINFO for a FLAC source: the source's own, unchanged and in order, without STREAMINFO, SEEKTABLE and
// PADDING; its VORBIS_COMMENT block stands for the vendor block, which is added behind STREAMINFO when the source has none.
// false: `file` is not a FLAC stream whose metadata can be walked.
bool rg_fe_source_blocks(const uint8_t *file, size_t len, std::vector<uint8_t> *blocks);
// the serial twin of rg_flac_encode_arena (route 0)
int rg_fe_arena_host(size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena, size_t arena_bytes,
                     const rg_flac_encode_options *options, void *out, size_t out_capacity, uint64_t *offsets, rg_flac_encode_result *results,
                     char *err, size_t err_len);

#ifdef __HIP__
#include <hip/hip_runtime.h>

struct rg_ctx;
// `st`: streams whose planes are device memory -> the streams' bytes, offsets[0 .. n], results.  blocks: NULL, or per stream the
// metadata blocks behind STREAMINFO (st[i].meta_bytes says how long; empty: the vendor block).  The bytes go to out[out_capacity] (RG_ERR_INVALID_ARG
// with the offsets set when it is too small) or, when `grow` is given, into *grow, sized to fit.  ms: NULL, or the kernels'
// times of this run by HIP events (analyse, layout, write, MD5).  `s` has been synchronised on return.
int rg_fe_device(rg_ctx *c, std::vector<RgFeStream> &st, const std::vector<std::vector<uint8_t>> *blocks, void *out, size_t out_capacity,
                 std::vector<uint8_t> *grow, uint64_t *offsets, rg_flac_encode_result *results, hipStream_t s, float *ms);
// The verified write's check: the streams out[offsets[i] .. offsets[i + 1]) through the device decoder (frame check, layout,
// decode kernels) into a device buffer in the arena's format, hashed there by the MD5 kernel; results[i].md5_decoded is set
// and ok[i] = the decode is complete, as long as the source and has its MD5.
int rg_fe_verify_device(rg_ctx *c, const std::vector<RgFeStream> &st, const uint8_t *out, const uint64_t *offsets, rg_flac_encode_result *results,
                        std::vector<uint8_t> *ok, hipStream_t s);
#endif
