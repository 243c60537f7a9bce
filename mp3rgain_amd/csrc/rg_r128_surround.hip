// rg_r128_surround.hip -- BS.1770 channel weights for the EBU R 128 path: the layout rule (host), and the fold kernel that
// turns the per-channel hop energies the main kernel wrote for a weighted track into the one row everything behind it reads.
// DESIGN.md section 14.3.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "rg_r128.h"

// =================================================================================================
// Fold kernel: e[h] = sum over the channels with w_c != 0 of w_c * e_c[h].
//
// One thread owns one (track, hop) and writes it with a plain store; a workgroup covers RG_R128_FOLD_BLOCK consecutive hops
// of one track, so every channel row is read in 2 KiB runs along h.  The sum runs in ascending channel order and starts
// from the first channel that counts; contraction is switched off in the kernel's body, so every product and every sum is
// a rounding of its own (no fused multiply-add): a weight of 1.0 leaves a channel's energy as it is and a power of two
// scales the row exactly.  Memory-bound, and small: 8 bytes per channel-hop against the hop's PCM.
__global__ void __launch_bounds__(RG_R128_FOLD_BLOCK)
rg_r128_fold_kernel(const RgR128FoldItem *__restrict__ items, const uint32_t n_items) {
#pragma clang fp contract(off)
    uint32_t lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (items[mid].block_base <= (uint64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const RgR128FoldItem &T = items[lo];
    const uint64_t h = ((uint64_t)blockIdx.x - T.block_base) * RG_R128_FOLD_BLOCK + threadIdx.x;
    if (h >= T.H) return;
    const double *__restrict__ src = T.src + h;
    const uint32_t nch = T.nch < 8u ? T.nch : 8u;
    double acc = 0.0;
    bool any = false;
    for (uint32_t c = 0; c < nch; ++c) {
        const double w = T.w[c];
        if (w == 0.0) continue;
        const double p = w * src[(size_t)c * T.H];
        acc = any ? acc + p : p;
        any = true;
    }
    T.dst[h] = acc;
}

int rg_r128_fold_launch(const RgR128FoldItem *d_items, uint32_t n_items, uint64_t blocks, void *stream) {
    if (!n_items || !blocks) return (int)hipSuccess;
    hipLaunchKernelGGL(rg_r128_fold_kernel, dim3((uint32_t)blocks), dim3(RG_R128_FOLD_BLOCK), 0, (hipStream_t)stream, d_items, n_items);
    return (int)hipGetLastError();
}

// =================================================================================================
// The layout rule (BS.1770-4 table 4 over the WAVE channel mask)
extern "C" int rg_r128_layout_weights(uint32_t channels, uint32_t channel_mask, rg_r128_channel_weights *out) {
    static const uint32_t kDefault[9] = {0, 0x4, 0x3, 0x7, 0x33, 0x37, 0x3F, 0x70F, 0x63F};  // the FLAC channel order
    if (!out || channels < 1 || channels > 8) return RG_ERR_INVALID_ARG;
    uint32_t mask = channel_mask;
    if (mask == 0 || (uint32_t)__builtin_popcount(mask) != channels) mask = kDefault[channels];
    const bool sides = (mask & 0x600u) != 0;
    memset(out, 0, sizeof *out);
    uint32_t i = 0;
    for (uint32_t bit = 0; bit < 32 && i < channels; ++bit) {
        const uint32_t pos = 1u << bit;
        if (!(mask & pos)) continue;
        double w = 1.0;
        if (pos == 0x8u) w = 0.0;                                          // LFE
        else if (pos == 0x200u || pos == 0x400u) w = 1.41;                 // SL, SR
        else if ((pos == 0x10u || pos == 0x20u) && !sides) w = 1.41;       // BL, BR standing in for the surrounds
        out->w[i++] = w;
    }
    return RG_OK;
}
