// rg_fprint_match.hip -- stage 2 of the duplicate finder on the device (include/mp3rgain_amd_fingerprint.h, rg_fprint.h): every
// compared pair of a call at every lag within the radius, by Hamming distance over probe blocks.
//
//   rg_fp_match_kernel  one workgroup of 256 lanes per compared pair.  For each probe the probe side's block (`block` words)
//                       and the other side's window (`block + 2 radius` words, zeros where it leaves the track) are staged in
//                       LDS.  Lanes own lags: lane l has lags l, l + 256, .. (at most 16, RG_FP_MAX_RADIUS = 2047), so in step
//                       i consecutive lanes read consecutive words of the window (no bank conflict) and all of them the same
//                       word of the block (a broadcast); one XOR, one popcount and one add per word and lag, in a loop without
//                       a branch (match_words, one instance per number of lag slots in use).  The per-lag
//                       totals stay in registers across the probes (fully unrolled: no scratch); each lane then keeps the best
//                       of its lags, and a tree over the 256 lanes in LDS with the same total order (rg_fp_better) closes the
//                       pair.  No atomics.  Everything is integer: the record is the host twin's byte for byte.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "rg_ctx.h"
#include "rg_fprint.h"

// the words of one probe at the first R lag slots of a lane: e[r] += the distance at lag slot r.  Every lane computes every one
// of its slots, whether the probe counts there or not (the caller keeps only those that do): a lag that is out of the other
// side reads the window's zeros, and a slot past the last lag reads the last lag's words, so no read leaves the window.
template <uint32_t R>
__device__ __forceinline__ void match_words(const uint32_t *s_a, const uint32_t *s_b, uint32_t block, uint32_t tid, uint32_t nl,
                                            uint32_t (&e)[RG_FP_LAGS_PER_LANE]) {
    const uint32_t *w[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t l = tid + RG_FP_MATCH_LANES * r;
        w[r] = s_b + (l < nl ? l : nl - 1u);  // l + i <= 2 radius + block - 1
    }
    for (uint32_t i = 0; i < block; ++i) {
        const uint32_t a = s_a[i];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) e[r] += (uint32_t)__popc(a ^ w[r][i]);
    }
}

__global__ __launch_bounds__(RG_FP_MATCH_LANES) void rg_fp_match_kernel(const uint32_t *__restrict__ codes, const RgFpPair *__restrict__ pairs,
                                                                        uint32_t block, uint32_t probes, uint32_t radius, uint32_t max_ber_permille,
                                                                        rg_fingerprint_pair_record *__restrict__ records) {
    extern __shared__ uint32_t s_w[];  // [block | block + 2 radius]
    __shared__ RgFpBest s_best[RG_FP_MATCH_LANES];
    uint32_t *s_a = s_w, *s_b = s_w + block;
    const uint32_t tid = threadIdx.x;
    const RgFpPair p = pairs[blockIdx.x];
    const uint32_t *A = codes + p.a_at, *B = codes + p.b_at;
    const uint32_t nl = 2u * radius + 1u, window = block + 2u * radius, slots = (nl + RG_FP_MATCH_LANES - 1u) / RG_FP_MATCH_LANES;
    uint32_t err[RG_FP_LAGS_PER_LANE], cnt[RG_FP_LAGS_PER_LANE];
#pragma unroll
    for (uint32_t r = 0; r < RG_FP_LAGS_PER_LANE; ++r) err[r] = cnt[r] = 0u;
    for (uint32_t pr = 0; pr < probes; ++pr) {
        const uint32_t sp = rg_fp_probe_start(pr, p.ka, block, probes);
        __syncthreads();  // the probe before has been read
        for (uint32_t i = tid; i < block; i += RG_FP_MATCH_LANES) s_a[i] = A[sp + i];  // sp + block <= ka
        for (uint32_t w = tid; w < window; w += RG_FP_MATCH_LANES) {
            const int64_t pos = (int64_t)sp - (int64_t)radius + (int64_t)w;
            s_b[w] = pos >= 0 && pos < (int64_t)p.kb ? B[pos] : 0u;
        }
        __syncthreads();
        uint32_t valid = 0;
#pragma unroll
        for (uint32_t r = 0; r < RG_FP_LAGS_PER_LANE; ++r) {
            const uint32_t l = tid + RG_FP_MATCH_LANES * r;
            const int64_t start = (int64_t)sp + (int64_t)l - (int64_t)radius;
            if (l < nl && start >= 0 && start + (int64_t)block <= (int64_t)p.kb) valid |= 1u << r;
        }
        uint32_t e[RG_FP_LAGS_PER_LANE];
#pragma unroll
        for (uint32_t r = 0; r < RG_FP_LAGS_PER_LANE; ++r) e[r] = 0u;
        switch (slots) {  // uniform: the word loop itself has no branch
            case 1: match_words<1>(s_a, s_b, block, tid, nl, e); break;
            case 2: match_words<2>(s_a, s_b, block, tid, nl, e); break;
            case 3: match_words<3>(s_a, s_b, block, tid, nl, e); break;
            case 4: match_words<4>(s_a, s_b, block, tid, nl, e); break;
            case 5: match_words<5>(s_a, s_b, block, tid, nl, e); break;
            case 6: match_words<6>(s_a, s_b, block, tid, nl, e); break;
            case 7: match_words<7>(s_a, s_b, block, tid, nl, e); break;
            case 8: match_words<8>(s_a, s_b, block, tid, nl, e); break;
            default: match_words<RG_FP_LAGS_PER_LANE>(s_a, s_b, block, tid, nl, e); break;
        }
#pragma unroll
        for (uint32_t r = 0; r < RG_FP_LAGS_PER_LANE; ++r)
            if (valid & (1u << r)) {
                err[r] += e[r];
                cnt[r] += 1u;
            }
    }
    const uint32_t need = (probes + 1u) / 2u;
    RgFpBest best{0u, 0u, 0};
#pragma unroll
    for (uint32_t r = 0; r < RG_FP_LAGS_PER_LANE; ++r) {
        if (cnt[r] < need || !cnt[r]) continue;
        const RgFpBest cand{err[r], cnt[r] * block * 32u, (int32_t)(tid + RG_FP_MATCH_LANES * r) - (int32_t)radius};
        if (rg_fp_better(cand, best)) best = cand;
    }
    s_best[tid] = best;
    __syncthreads();
    for (uint32_t w = RG_FP_MATCH_LANES / 2; w; w >>= 1) {
        if (tid < w) {
            const RgFpBest other = s_best[tid + w];
            if (rg_fp_better(other, s_best[tid])) s_best[tid] = other;
        }
        __syncthreads();
    }
    if (tid == 0) rg_fp_close(s_best[0], p.flags, max_ber_permille, &records[p.rec]);
}

static size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

// the pair list goes up in pieces of at most this many pairs: 32 MB of the work buffer, whatever the call's size
static const size_t kMatchPiece = (size_t)1 << 20;

int rg_fprint_match_launch(rg_ctx *c, const uint32_t *d_codes, const RgFpPair *d_pairs, size_t count, const rg_fingerprint_opts &o,
                        rg_fingerprint_pair_record *d_records, hipStream_t s) {
    const size_t lds = ((size_t)2 * o.block + (size_t)2 * o.radius) * sizeof(uint32_t);  // at most 49 KB
    hipLaunchKernelGGL(rg_fp_match_kernel, dim3((uint32_t)count), dim3(RG_FP_MATCH_LANES), lds, s, d_codes, d_pairs, o.block, o.probes, o.radius,
                       o.max_ber_permille, d_records);
    RG_HIP(c, hipGetLastError());
    return RG_OK;
}

int rg_fprint_match_device(rg_ctx *c, const uint32_t *d_codes, const std::vector<RgFpPair> &pairs, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records, hipStream_t s) {
    if (pairs.empty()) return RG_OK;
    const size_t piece = std::min(pairs.size(), kMatchPiece), rec_at = a16(piece * sizeof(RgFpPair));
    RG_HIP(c, c->d_fprint.reserve(rec_at + piece * sizeof(rg_fingerprint_pair_record)));
    RgFpPair *d_pairs = reinterpret_cast<RgFpPair *>(c->d_fprint.p);
    rg_fingerprint_pair_record *d_rec = reinterpret_cast<rg_fingerprint_pair_record *>(c->d_fprint.p + rec_at);
    std::vector<RgFpPair> up(piece);
    std::vector<rg_fingerprint_pair_record> down(piece);
    for (size_t first = 0; first < pairs.size(); first += piece) {
        const size_t count = std::min(piece, pairs.size() - first);
        for (size_t k = 0; k < count; ++k) {  // a piece's records are its own 0 .. count - 1
            up[k] = pairs[first + k];
            up[k].rec = (uint32_t)k;
        }
        RG_HIP(c, hipMemcpyAsync(d_pairs, up.data(), count * sizeof(RgFpPair), hipMemcpyHostToDevice, s));
        const int rc = rg_fprint_match_launch(c, d_codes, d_pairs, count, o, d_rec, s);
        if (rc != RG_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        RG_HIP(c, hipMemcpyAsync(down.data(), d_rec, count * sizeof(rg_fingerprint_pair_record), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t k = 0; k < count; ++k) records[pairs[first + k].rec] = down[k];
    }
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_fingerprint.h) --------------------------------------------------------------------------
extern "C" int rg_fingerprint_match_codes(void *ctx, int route, size_t n, const uint32_t *counts, const uint32_t *rates, const uint32_t *codes,
                                          const rg_fingerprint_opts *opts, rg_fingerprint_pair_record *pair_records) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    char err[256] = "";
    if (!c && route == 1) return RG_ERR_INVALID_ARG;
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_match_codes: route %d (0 = serial host twin, 1 = kernel)", route);
    if (n && (!counts || !rates || (n > 1 && !pair_records))) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_match_codes: null array");
    if (n > 65535) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_match_codes: %zu tracks, at most 65535 in one call", n);
    rg_fingerprint_opts o;
    int rc = rg_fp_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    try {
        std::vector<uint64_t> at(n + 1, 0);
        for (size_t i = 0; i < n; ++i) at[i + 1] = at[i] + counts[i];
        if (at[n] && !codes) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_fingerprint_match_codes: null array");
        if (route == 0) return rg_fp_match_codes_host(n, counts, rates, codes, o, pair_records);
        std::vector<RgFpPair> pairs;
        rg_fp_pairs(n, counts, rates, at.data(), o, &pairs, pair_records);
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        RG_HIP(c, c->d_fp_codes.reserve((size_t)at[n] + 4));
        if (at[n]) RG_HIP(c, hipMemcpyAsync(c->d_fp_codes.p, codes, (size_t)at[n] * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        rc = rg_fprint_match_device(c, c->d_fp_codes.p, pairs, o, pair_records, s);
        RG_HIP(c, hipStreamSynchronize(s));
        return rc;
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}
