// rg_r128_design.cpp -- host design of the EBU R 128 path: the K-weighting biquads of ITU-R BS.1770 at any sample rate, and
// the true-peak interpolator's taps.  Host only, no GPU needed.
//
// BS.1770 prints its two filters as coefficients at 48 kHz.  They are bilinear transforms of analogue prototypes (a
// high-shelf and a second-order high-pass), and the prototypes' parameters below reproduce the printed table to all 14
// digits; other rates use the same prototypes.
#include <math.h>

#include "rg_r128.h"

bool rg_r128_design(uint32_t rate, RgR128Design *o) {
    if (rate < RG_R128_MIN_RATE || rate > RG_R128_MAX_RATE) return false;
    const long double pi = 3.14159265358979323846264338327950288L;
    {   // stage 1: high shelf
        const long double f0 = 1681.974450955533L, G = 3.999843853973347L, Q = 0.7071752369554196L;
        const long double K = tanl(pi * f0 / (long double)rate);
        const long double Vh = powl(10.0L, G / 20.0L), Vb = powl(Vh, 0.4996667741545416L);
        const long double a0 = 1.0L + K / Q + K * K;
        o->b1[0] = (double)((Vh + Vb * K / Q + K * K) / a0);
        o->b1[1] = (double)(2.0L * (K * K - Vh) / a0);
        o->b1[2] = (double)((Vh - Vb * K / Q + K * K) / a0);
        o->a1[0] = 1.0;
        o->a1[1] = (double)(2.0L * (K * K - 1.0L) / a0);
        o->a1[2] = (double)((1.0L - K / Q + K * K) / a0);
    }
    {   // stage 2: the "revised low-frequency B" high-pass
        const long double f0 = 38.13547087602444L, Q = 0.5003270373238773L;
        const long double K = tanl(pi * f0 / (long double)rate);
        const long double a0 = 1.0L + K / Q + K * K;
        o->b2[0] = 1.0;
        o->b2[1] = -2.0;
        o->b2[2] = 1.0;
        o->a2[0] = 1.0;
        o->a2[1] = (double)(2.0L * (K * K - 1.0L) / a0);
        o->a2[2] = (double)((1.0L - K / Q + K * K) / a0);
    }
    o->hop = (rate + 5u) / 10u;
    o->tp_factor = rate < 96000u ? 4u : rate < 192000u ? 2u : 1u;
    return true;
}

void rg_r128_tp_table(uint32_t F, float *taps) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < RG_R128_TP_TAPS; ++j) {
        const double x = (double)(j - 24) / (double)F;
        const double s = x == 0.0 ? 1.0 : sin(pi * x) / (pi * x);
        const double w = 0.5 * (1.0 - cos(2.0 * pi * (double)j / 48.0));
        taps[j] = (float)(s * w);
    }
}

extern "C" int rg_r128_supported_rate(uint32_t rate) { return rate >= RG_R128_MIN_RATE && rate <= RG_R128_MAX_RATE ? 1 : 0; }

extern "C" int rg_r128_design_info(uint32_t rate, double *b1, double *a1, double *b2, double *a2, uint32_t *hop, uint32_t *tp_factor) {
    RgR128Design d;
    if (!rg_r128_design(rate, &d)) return RG_ERR_UNSUPPORTED_RATE;
    for (int i = 0; i < 3; ++i) {
        if (b1) b1[i] = d.b1[i];
        if (a1) a1[i] = d.a1[i];
        if (b2) b2[i] = d.b2[i];
        if (a2) a2[i] = d.a2[i];
    }
    if (hop) *hop = d.hop;
    if (tp_factor) *tp_factor = d.tp_factor;
    return RG_OK;
}

extern "C" uint64_t rg_r128_block_count(uint32_t rate, uint64_t frames) {
    if (!rg_r128_supported_rate(rate)) return 0;
    const uint64_t H = frames / ((rate + 5u) / 10u);
    return H > 3 ? H - 3 : 0;
}

extern "C" uint64_t rg_r128_short_term_count(uint32_t rate, uint64_t frames) {
    if (!rg_r128_supported_rate(rate)) return 0;
    const uint64_t H = frames / ((rate + 5u) / 10u);
    return H > 29 ? H - 29 : 0;
}
