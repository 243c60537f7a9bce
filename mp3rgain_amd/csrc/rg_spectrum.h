// rg_spectrum.h -- internal: the spectral scan (include/mp3rgain_amd_spectrum.h) as rg_spectrum.hip (kernels, launcher, seams),
// rg_spectrum_host.cpp (the serial host twin in double, the kernels' arithmetic on the host, the verdict) and
// rg_file_verify.hip (rg_spectrum) share it.  What one lane does in each of the three passes of the 4096-point transform, how
// two frames are separated and a band summed, is host and device code, written once here; the kernels and the host route 2
// differ only in who walks the lanes and in where the exchanged values lie.  Every operation is a plain f32 multiply, add or
// subtract, and both translation units are compiled without contraction, so the two give the same bits.
//
// The transform.  Two real frames a, b go in as z[n] = a[n] w[n] + i b[n] w[n], n = 256 n2 + 16 n1 + n0, and
// Z[k], k = k0 + 16 k1 + 256 k2, comes out of three radix-16 passes of 256 lanes with 16 points each (W = e^(-2 pi i / 4096)):
//   pass 1  lane (n1, n0): A[k0] = DFT16 over n2, times W^((16 n1 + n0) k0)          (rg_spec_pass1, table tw1)
//   pass 2  lane (k0, n0): B[k1] = DFT16 over n1, times W^(16 n0 k1)                 (rg_spec_pass2, table tw2)
//   pass 3  lane (k1, k0): Z[k2] = DFT16 over n0                                     (rg_spec_dft16)
// With a, b real, A[b] = (Z[b] + conj Z[L - b]) / 2 and B[b] = (Z[b] - conj Z[L - b]) / 2i (rg_spec_band).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mp3rgain_amd_spectrum.h"
#include "rg_pcm_plane.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_SPEC_HD __host__ __device__ inline
#else
#define RG_SPEC_HD inline
#endif

#define RG_SPEC_BLOCK 256u             // lanes of a tile block = points / 16 = bands
#define RG_SPEC_TILE_FRAMES 32u        // T: frames one block transforms, two at a time
#define RG_SPEC_MAX_LAUNCH_TILES 32768u  // tile records of one launch: 64 MiB (a plane is never split: at most 65536 tiles, 128 MiB)

struct RgSpecC {
    float x, y;
};

// the tables both sides read: built once on the host in double and rounded once
struct RgSpecTables {
    float window[RG_SPEC_FRAME];  // periodic Hann
    RgSpecC tw1[16 * 256];        // [k0 * 256 + t]  = W^(t k0)
    RgSpecC tw2[16 * 16];         // [k1 * 16 + n0]  = W^(16 n0 k1)
};  // 51200 bytes

// One plane of a launch
struct RgSpecPlane {
    uint64_t off;         // from the arena's base, in bytes (sample-aligned)
    uint64_t first_tile;  // of this plane among the launch's tiles (the tiles of one format are contiguous)
    uint32_t n;           // N < 2^32
    uint32_t frames;      // K
    uint32_t n_tiles;     // ceil(K / T)
    uint32_t format;      // rg_sample_format
};  // 32 bytes

// what the fold leaves per plane
struct RgSpecPlaneOut {
    double E[RG_SPEC_BANDS];
    uint32_t analysed, skipped;
    uint32_t reserved[2];
};  // 2064 bytes

RG_SPEC_HD uint32_t rg_spec_frames(uint64_t n) { return n < RG_SPEC_FRAME ? 0u : (uint32_t)((n - RG_SPEC_FRAME) / RG_SPEC_HOP + 1u); }

// `raw`: the stored pattern, an S16 sample sign-extended to 32 bits
template <int FMT>
RG_SPEC_HD float rg_spec_value(uint32_t raw) {
    if (FMT == RG_FMT_F32_PLANAR) {
        float f;
        memcpy(&f, &raw, 4);
        return f;
    }
    return (float)(int32_t)raw * (FMT == RG_FMT_S16_PLANAR ? 1.0f / 32768.0f : 1.0f / 2147483648.0f);
}
template <int FMT>
RG_SPEC_HD bool rg_spec_nonfinite(uint32_t raw) {
    return FMT == RG_FMT_F32_PLANAR && (raw & 0x7F800000u) == 0x7F800000u;
}

RG_SPEC_HD RgSpecC rg_spec_mul(RgSpecC a, RgSpecC b) { return RgSpecC{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// (a, b, c, d) <- their 4-point DFT
RG_SPEC_HD void rg_spec_dft4(RgSpecC &a, RgSpecC &b, RgSpecC &c, RgSpecC &d) {
    const RgSpecC t0{a.x + c.x, a.y + c.y}, t1{a.x - c.x, a.y - c.y}, t2{b.x + d.x, b.y + d.y}, t3{b.x - d.x, b.y - d.y};
    a = RgSpecC{t0.x + t2.x, t0.y + t2.y};
    b = RgSpecC{t1.x + t3.y, t1.y - t3.x};  // t1 - i t3
    c = RgSpecC{t0.x - t2.x, t0.y - t2.y};
    d = RgSpecC{t1.x - t3.y, t1.y + t3.x};  // t1 + i t3
}

// v[k] <- sum over n of v[n] e^(-2 pi i n k / 16): two layers of radix 4 with the 16th roots between them
RG_SPEC_HD void rg_spec_dft16(RgSpecC v[16]) {
    const float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
    for (int n0 = 0; n0 < 4; ++n0) rg_spec_dft4(v[n0], v[n0 + 4], v[n0 + 8], v[n0 + 12]);  // v[n0 + 4 k0]
    // times e^(-2 pi i n0 k0 / 16)
    v[5] = rg_spec_mul(v[5], RgSpecC{c1, -s1});          // n0 = 1, k0 = 1
    v[9] = rg_spec_mul(v[9], RgSpecC{h, -h});            //          k0 = 2
    v[13] = rg_spec_mul(v[13], RgSpecC{s1, -c1});        //          k0 = 3
    v[6] = rg_spec_mul(v[6], RgSpecC{h, -h});            // n0 = 2: exponents 2, 4, 6
    v[10] = RgSpecC{v[10].y, -v[10].x};
    v[14] = rg_spec_mul(v[14], RgSpecC{-h, -h});
    v[7] = rg_spec_mul(v[7], RgSpecC{s1, -c1});          // n0 = 3: exponents 3, 6, 9
    v[11] = rg_spec_mul(v[11], RgSpecC{-h, -h});
    v[15] = rg_spec_mul(v[15], RgSpecC{-c1, s1});
    for (int k0 = 0; k0 < 4; ++k0) rg_spec_dft4(v[4 * k0], v[4 * k0 + 1], v[4 * k0 + 2], v[4 * k0 + 3]);  // v[4 k0 + k1] = X[k0 + 4 k1]
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) {
            const RgSpecC t = v[4 * a + b];
            v[4 * a + b] = v[4 * b + a];
            v[4 * b + a] = t;
        }
}

RG_SPEC_HD void rg_spec_pass1(RgSpecC v[16], uint32_t t, const RgSpecC *tw1) {
    rg_spec_dft16(v);
    for (uint32_t k0 = 1; k0 < 16; ++k0) v[k0] = rg_spec_mul(v[k0], tw1[k0 * 256u + t]);
}
RG_SPEC_HD void rg_spec_pass2(RgSpecC v[16], uint32_t n0, const RgSpecC *tw2) {
    rg_spec_dft16(v);
    for (uint32_t k1 = 1; k1 < 16; ++k1) v[k1] = rg_spec_mul(v[k1], tw2[k1 * 16u + n0]);
}

// band j of the two frames that went in as real and imaginary part: the eight powers of each summed in f32, bin order.
// z(k) = Z[k], 1 <= k <= 4095.
template <class Z>
RG_SPEC_HD void rg_spec_band(Z z, uint32_t j, float *sum_a, float *sum_b) {
    float a = 0.0f, b = 0.0f;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t bin = 8u * j + 1u + i;
        const RgSpecC u = z(bin), w = z(RG_SPEC_FRAME - bin);
        const float ar = u.x + w.x, ai = u.y - w.y, br = u.y + w.y, bi = w.x - u.x;
        a += (ar * ar + ai * ai) * 0.25f;
        b += (br * br + bi * bi) * 0.25f;
    }
    *sum_a = a;
    *sum_b = b;
}

// ---- host side (rg_spectrum_host.cpp) ---------------------------------------------------------------------------------------
const RgSpecTables &rg_spec_tables();
// the options, checked: NULL = the defaults
int rg_spec_options(const rg_spectrum_opts *opts, rg_spectrum_opts *out, char *err, size_t err_len);
// planes[0 .. channels) <- track i's planes, checked against the arena; everything but first_tile / n_tiles
int rg_spec_track_planes(size_t i, const rg_track_desc &t, size_t arena_bytes, RgSpecPlane *planes, char *err, size_t err_len);
// first_tile and n_tiles of planes[0 .. n), the tiles of one format contiguous: fmt_tile[f] .. fmt_tile[f + 1]; -> tiles
uint64_t rg_spec_plan(RgSpecPlane *planes, size_t n, uint64_t fmt_tile[4]);
// route 0 and route 2 of one plane
void rg_spec_serial_host(const unsigned char *arena, const RgSpecPlane &p, RgSpecPlaneOut *out);
void rg_spec_folded_host(const unsigned char *arena, const RgSpecPlane &p, RgSpecPlaneOut *out);
// a track's record (and its 8 x 256 band energies when bands is not NULL) from its planes' folds
void rg_spec_fill(const rg_track_desc &t, uint32_t dropped_frames, const RgSpecPlaneOut *planes, const rg_spectrum_opts &o, rg_spectrum_result *out,
                  double *bands);
int rg_spec_arena_host(int route, size_t n, const rg_track_desc *descs, const rg_spectrum_opts *opts, const void *arena, size_t arena_bytes,
                       rg_spectrum_result *out, double *bands_out, char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` planes in the device arena at `d_arena`: the two kernels on `s`, out[i] <- plane i; `s` has been synchronised on return
int rg_spectrum_device(rg_ctx *c, const unsigned char *d_arena, RgSpecPlane *planes, size_t n, RgSpecPlaneOut *out, hipStream_t s);
#endif
