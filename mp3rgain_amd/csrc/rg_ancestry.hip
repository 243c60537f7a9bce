// rg_ancestry.hip -- the lossy ancestry scan on the device (include/mp3rgain_amd_ancestry.h, rg_ancestry.h): per view and
// alignment the counts of active and of small spectral lines of the encoder's hybrid filterbank.
//
//   rg_anc_tile_kernel   one workgroup of 256 lanes per (tile, phase): grid = 32 * tiles.  The tile's 32 (18 ng + 35) + 480
//                        samples of its phase go to LDS as floats (mid and side are mixed here); the four waves take the slots
//                        two at a time -- 64 lanes window Y[64] of each slot into LDS, then 2 x 32 lanes matrix one subband
//                        each, taps and matrix column in registers -- and leave 18 ng + 35 slots x 32 subbands in LDS.  Then
//                        a half-wave takes one (alignment q, granule) pair, lane = subband: its 36 slots from LDS into
//                        registers, 18 lines as 18 chains over 36 coefficients that are the same for every lane (the compiler
//                        pairs the lines into v_pk_fma_f32), the butterflies and the groups of 12 across neighbouring lanes by
//                        shuffles, the counts reduced over the half-wave into 36 integer counters in LDS, and those added to
//                        the view's table at the end (integer atomics: any order gives the same sums).  30.8 KB of LDS with
//                        tiles of 4 granules, no scratch.
//   rg_anc_nonfinite_kernel  NaN / Inf samples of the float planes, counted over the whole plane.
// Every read of the arena is guarded by 0 <= index < N of a plane the callers have checked to lie inside the arena.
#include <string.h>

#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include "rg_ctx.h"
#include "rg_ancestry.h"
#include "rg_pcm_seam.h"

__global__ __launch_bounds__(RG_ANC_LANES) void rg_anc_tile_kernel(const unsigned char *__restrict__ arena, const RgAncTables *__restrict__ tables,
                                                                   const RgAncView *__restrict__ views, const RgAncJob *__restrict__ jobs, float floor_,
                                                                   unsigned long long *__restrict__ counts) {
    __shared__ float s_x[RG_ANC_TILE_SAMPLES];
    __shared__ float s_sub[RG_ANC_TILE_SLOTS * 32u];
    __shared__ float s_y[4][2][64];
    __shared__ uint32_t s_cnt[36];
    const RgAncTables &t = *tables;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const RgAncJob job = jobs[blockIdx.x / RG_ANC_PHASES];
    const uint32_t phase = blockIdx.x % RG_ANC_PHASES;
    const RgAncView v = views[job.view];
    const uint32_t nslots = 18u * job.ng + 35u, nsamp = 32u * nslots + 480u;
    const int64_t x0 = (int64_t)job.a + phase + 32ll * 18 * ((int64_t)job.g0 - 1) - 480;
    if (tid < 36) s_cnt[tid] = 0;
    for (uint32_t n = tid; n < nsamp; n += RG_ANC_LANES) s_x[n] = rg_anc_sample(arena, v, x0 + (int64_t)n);
    __syncthreads();
    // the subband samples: every wave two slots per step (the loop is uniform over the workgroup).  A lane's window taps and its
    // column of the matrix stay in registers over the whole loop; the chains are rg_anc_window's and rg_anc_matrix's, term by term
    float cw[8], mk[64];
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) cw[m] = t.c[lane + 64u * m];
#pragma unroll
    for (uint32_t j = 0; j < 64; ++j) mk[j] = t.mt[j][lane & 31u];
    const uint32_t npairs = (nslots + 1u) / 2u;
    for (uint32_t it = 0; it < (npairs + 3u) / 4u; ++it) {
        const uint32_t s0 = 2u * (4u * it + wave);
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t s = s0 + h;
            if (s < nslots) {
                const float *newest = &s_x[480u + 32u * s + 31u - lane];
                float acc = 0.0f;
#pragma unroll
                for (uint32_t m = 0; m < 8; ++m) acc = rg_anc_fma(cw[m], *(newest - 64u * m), acc);
                s_y[wave][h][lane] = acc;
            }
        }
        __syncthreads();
        {
            const uint32_t h = lane >> 5, k = lane & 31u, s = s0 + h;
            if (s < nslots) {
                const float *y = s_y[wave][h];
                float acc = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < 64; ++j) acc = rg_anc_fma(mk[j], y[j], acc);
                s_sub[s * 32u + k] = acc;
            }
        }
        __syncthreads();
    }
    // the MDCT, the butterflies and the statistic: a half-wave per (q, granule) pair, lane = subband
    const uint32_t sb = tid & 31u, total = 18u * job.ng;
    for (uint32_t it = 0; it < (total + 7u) / 8u; ++it) {
        const uint32_t want = 8u * it + (tid >> 5);
        const bool valid = want < total;
        const uint32_t pair = valid ? want : total - 1u;  // (the shuffles below are run by every lane)
        const uint32_t q = pair % 18u, u0 = q + 18u * (pair / 18u);
        float x[18];
        // the 648 coefficients are taken inside the loop: hoisted out of it as scalars they do not fit the scalar registers,
        // and every multiply-add then pays for nine moves out of spill lanes (measured: a tenth of the vector peak)
        const RgAncTables *tp = tables;
        asm volatile("" : "+s"(tp));
        rg_anc_mdct(*tp, [&](uint32_t i) { return rg_anc_invert(s_sub[(u0 + i) * 32u + sb], sb, i); }, x);
        // butterflies: lines 0 .. 7 with the subband below, lines 17 .. 10 with the one above
        float below[8], above[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            below[i] = __shfl_up(x[17 - i], 1, 32);  // a of my lines 0 .. 7
            above[i] = __shfl_down(x[i], 1, 32);     // b of my lines 17 .. 10
        }
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const float up = x[i], lo = x[17 - i];
            if (sb >= 1) x[i] = rg_anc_bfly_up(below[i], up, t.cs[i], t.ca[i]);
            if (sb <= 30) x[17 - i] = rg_anc_bfly_lo(lo, above[i], t.cs[i], t.ca[i]);
        }
        // groups of 12: an even subband has lines 0 .. 11 and begins a group with 12 .. 17; the odd one above ends it with
        // its lines 0 .. 5 and has 6 .. 17
        const bool odd = sb & 1u;
        float qa = 0.0f, qb = 0.0f;  // even: group of lines 0 .. 11, the part 12 .. 17; odd: (part +) 0 .. 5, lines 6 .. 17
        if (!odd) {
#pragma unroll
            for (uint32_t i = 0; i < 12; ++i) qa = rg_anc_ssq(qa, x[i]);
#pragma unroll
            for (uint32_t i = 12; i < 18; ++i) qb = rg_anc_ssq(qb, x[i]);
        }
        const float part = __shfl_up(qb, 1, 32);
        if (odd) {
            qa = part;
#pragma unroll
            for (uint32_t i = 0; i < 6; ++i) qa = rg_anc_ssq(qa, x[i]);
            qb = 0.0f;
#pragma unroll
            for (uint32_t i = 6; i < 18; ++i) qb = rg_anc_ssq(qb, x[i]);
        }
        const float shared_ms = __shfl_down(rg_anc_ms(qa), 1, 32);  // to the even lane: the group its lines 12 .. 17 are in
        const float ms_a = rg_anc_ms(qa), ms_b = odd ? rg_anc_ms(qb) : shared_ms;
        const bool act_a = ms_a >= floor_, act_b = ms_b >= floor_;
        const uint32_t split = odd ? 6u : 12u;  // lines below `split` are in group a, the others in group b
        uint32_t small_ = 0;
#pragma unroll
        for (uint32_t i = 0; i < 18; ++i) {
            const bool in_a = i < split;
            if ((in_a ? act_a : act_b) && rg_anc_is_small(x[i], in_a ? ms_a : ms_b)) ++small_;
        }
        // a group's 12 lines are counted once: group a by its lane, the shared group by the odd lane (its group a), group b of
        // an odd lane by that lane
        uint32_t active_ = (act_a ? RG_ANC_GROUP : 0u) + (odd && act_b ? RG_ANC_GROUP : 0u);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            small_ += __shfl_xor(small_, d, 32);
            active_ += __shfl_xor(active_, d, 32);
        }
        if (valid && sb == 0) {
            atomicAdd(&s_cnt[q], small_);
            atomicAdd(&s_cnt[18u + q], active_);
        }
    }
    __syncthreads();
    if (tid < 36) {
        const uint32_t q = tid % 18u, which = tid / 18u;
        if (s_cnt[tid]) atomicAdd(&counts[((size_t)job.view * 2u + which) * RG_ANC_ALIGNMENTS + 32u * q + phase], (unsigned long long)s_cnt[tid]);
    }
}

__global__ __launch_bounds__(256) void rg_anc_nonfinite_kernel(const unsigned char *__restrict__ arena, const RgAncView *__restrict__ views,
                                                               unsigned long long *__restrict__ nonfinite) {
    const RgAncView v = views[blockIdx.y];
    if (v.format != RG_FMT_F32_PLANAR || v.mix) return;
    uint32_t cnt = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < v.n; k += (uint64_t)gridDim.x * 256u)
        cnt += rg_anc_nonfinite(*reinterpret_cast<const uint32_t *>(arena + v.off_a + 4ull * k)) ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&nonfinite[blockIdx.y], (unsigned long long)cnt);
}

// Device layout of one launch's bookkeeping, every part 16-byte aligned: [tables | views | jobs | counts | nonfinite]
struct AncLayout {
    size_t views, jobs, counts, nonfinite, end;
};
static AncLayout anc_layout(size_t n_views, size_t n_jobs) {
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    AncLayout l;
    l.views = a16(sizeof(RgAncTables));
    l.jobs = a16(l.views + n_views * sizeof(RgAncView));
    l.counts = a16(l.jobs + n_jobs * sizeof(RgAncJob));
    l.nonfinite = a16(l.counts + n_views * 2 * RG_ANC_ALIGNMENTS * sizeof(uint64_t));
    l.end = a16(l.nonfinite + n_views * sizeof(uint64_t));
    return l;
}
static void anc_head(const RgAncView *views, size_t n_views, const std::vector<RgAncJob> &jobs, const AncLayout &l, std::vector<unsigned char> *head) {
    head->assign(l.counts, 0);
    memcpy(head->data(), &rg_anc_tables(), sizeof(RgAncTables));
    if (n_views) memcpy(head->data() + l.views, views, n_views * sizeof(RgAncView));
    if (!jobs.empty()) memcpy(head->data() + l.jobs, jobs.data(), jobs.size() * sizeof(RgAncJob));
}
static int anc_launch(rg_ctx *c, const unsigned char *d_arena, unsigned char *d, const AncLayout &l, size_t n_views, size_t n_jobs, bool any_float, float floor_,
                      hipStream_t s) {
    RG_HIP(c, hipMemsetAsync(d + l.counts, 0, l.end - l.counts, s));
    const RgAncView *d_views = reinterpret_cast<const RgAncView *>(d + l.views);
    if (n_jobs) {
        hipLaunchKernelGGL(rg_anc_tile_kernel, dim3((uint32_t)(n_jobs * RG_ANC_PHASES)), dim3(RG_ANC_LANES), 0, s, d_arena, reinterpret_cast<const RgAncTables *>(d),
                           d_views, reinterpret_cast<const RgAncJob *>(d + l.jobs), floor_, reinterpret_cast<unsigned long long *>(d + l.counts));
        RG_HIP(c, hipGetLastError());
    }
    if (any_float) {
        hipLaunchKernelGGL(rg_anc_nonfinite_kernel, dim3(64, (uint32_t)n_views), dim3(256), 0, s, d_arena, d_views,
                           reinterpret_cast<unsigned long long *>(d + l.nonfinite));
        RG_HIP(c, hipGetLastError());
    }
    return RG_OK;
}
static bool anc_any_float(const RgAncView *views, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (views[i].format == RG_FMT_F32_PLANAR) return true;
    return false;
}

int rg_anc_device(rg_ctx *c, const unsigned char *d_arena, const RgAncView *views, size_t n_views, const std::vector<RgAncJob> &jobs, float floor_,
                  uint64_t *counts, uint64_t *nonfinite, hipStream_t s) {
    if (!n_views) return RG_OK;
    if (n_views > 65535u || jobs.size() > 0x7fffffffu / RG_ANC_PHASES)
        return rg_set_err(c, RG_ERR_INVALID_ARG, "too much for one launch: %zu views, %zu tiles", n_views, jobs.size());
    const AncLayout l = anc_layout(n_views, jobs.size());
    std::vector<unsigned char> head;
    anc_head(views, n_views, jobs, l, &head);
    RG_HIP(c, c->d_ancestry.reserve(l.end));
    unsigned char *d = c->d_ancestry.p;
    RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
    const int rc = anc_launch(c, d_arena, d, l, n_views, jobs.size(), anc_any_float(views, n_views), floor_, s);
    if (rc != RG_OK) {
        (void)hipStreamSynchronize(s);  // (`head` is on its way)
        return rc;
    }
    RG_HIP(c, hipMemcpyAsync(counts, d + l.counts, n_views * 2 * RG_ANC_ALIGNMENTS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipMemcpyAsync(nonfinite, d + l.nonfinite, n_views * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RG_HIP(c, hipStreamSynchronize(s));
    return RG_OK;
}

// ---- test seam (include/mp3rgain_amd_ancestry.h) -----------------------------------------------------------------------------
extern "C" int rg_ancestry_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const rg_ancestry_opts *opts, const void *arena,
                                 size_t arena_bytes, rg_ancestry_result *out, uint64_t *counts) {
    rg_ancestry_opts o;
    std::vector<RgAncView> views;
    std::vector<RgAncJob> jobs;
    struct Track {
        uint32_t first, nv, S, G;  // its first view and how many, its cut
    };
    std::vector<Track> tracks;
    size_t n_views = 0;
    const auto host = [&](char *err, size_t err_len) { return rg_anc_arena_host(route, n, descs, opts, arena, arena_bytes, out, counts, err, err_len); };
    const auto plan = [&](char *err, size_t err_len) -> int {
        int rc = rg_anc_options(opts, &o, err, err_len);
        if (rc != RG_OK) return rc;
        views = std::vector<RgAncView>(n * RG_ANC_MAX_VIEWS + 1);
        tracks = std::vector<Track>(n + 1);
        for (size_t i = 0; i < n; ++i) {
            Track &t = tracks[i];
            rc = rg_anc_track_views(i, descs[i], arena_bytes, &views[n_views], &t.nv, err, err_len);
            if (rc != RG_OK) return rc;
            t.first = (uint32_t)n_views;
            for (uint32_t v = 0; v < t.nv; ++v) rg_anc_jobs(descs[i].frames, o, (uint32_t)n_views + v, &jobs, &t.S, &t.G);
            n_views += t.nv;
        }
        return RG_OK;
    };
    const auto device = [&](rg_ctx *c, hipStream_t s) -> int {
        const size_t per_view = 2 * RG_ANC_ALIGNMENTS;
        std::vector<uint64_t> cnt((n_views ? n_views : 1) * per_view), nonfinite(n_views ? n_views : 1);
        const int rc = rg_anc_device(c, c->d_arena.p, views.data(), n_views, jobs, o.active_floor, cnt.data(), nonfinite.data(), s);
        if (rc != RG_OK) return rc;
        for (size_t i = 0; i < n; ++i) {
            const Track &t = tracks[i];
            rg_anc_fill(descs[i], o, t.S, t.G, 0, t.nv, &views[t.first], &cnt[t.first * per_view], &nonfinite[t.first], &out[i]);
            if (counts) {
                memset(counts + i * RG_ANC_MAX_VIEWS * per_view, 0, RG_ANC_MAX_VIEWS * per_view * sizeof(uint64_t));
                memcpy(counts + i * RG_ANC_MAX_VIEWS * per_view, &cnt[t.first * per_view], t.nv * per_view * sizeof(uint64_t));
            }
        }
        return RG_OK;
    };
    return rg_pcm_arena_seam(ctx, route, "rg_ancestry_arena", "the kernels' cutting", n, descs, out, arena, arena_bytes, host, plan, device);
}

// ---- measurement hook (tools/ancestry_rate.py) -------------------------------------------------------------------------------
// pseudo-random 16-bit samples, two per word: word w <- a mix of its index, scaled down to a quarter of full scale
__global__ __launch_bounds__(256) void rg_anc_fill_kernel(uint32_t *__restrict__ dst, uint64_t words) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        const uint32_t u = (uint32_t)(x >> 24);
        const int32_t lo = (int32_t)(int16_t)u >> 2, hi = (int32_t)u >> 18;
        dst[w] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
    }
}

extern "C" int rg_ancestry_rate(void *ctx, size_t n, uint64_t frames, const rg_ancestry_opts *opts, size_t host_tracks, uint32_t threads, uint32_t reps,
                                double warm_ms, double *kernel_ms, double *host_ms, size_t *mismatches, double *fma_per_sample) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !frames || frames >= ((uint64_t)1 << 32) || !reps || !kernel_ms || (host_tracks && (!host_ms || !threads || !mismatches)) || host_tracks > n ||
        !(warm_ms >= 0.0))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_ancestry_rate: bad arguments");
    char err[256] = "";
    rg_ancestry_opts o;
    int rc = rg_anc_options(opts, &o, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    rc = rg_bind_device(c);
    if (rc != RG_OK) return rc;
    const size_t track_bytes = (size_t)frames * 2 * 2, stride = (track_bytes + 15) & ~(size_t)15, total = n * stride;
    unsigned char *d_arena = nullptr, *d = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        hipStream_t s = c->slots[0].stream;
        std::vector<RgAncView> views(4 * n);
        std::vector<RgAncJob> jobs;
        uint32_t S = 0, G = 0;
        for (size_t i = 0; i < n; ++i) {
            rg_track_desc t{};
            t.offset_bytes = i * stride;
            t.frames = frames;
            t.sample_rate = 44100;
            t.channels = 2;
            t.format = RG_FMT_S16_PLANAR;
            uint32_t nv;
            if (rg_anc_track_views(i, t, total, &views[4 * i], &nv, err, sizeof err) != RG_OK) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_ancestry_rate: %s", err);
            for (uint32_t v = 0; v < 4; ++v) rg_anc_jobs(frames, o, (uint32_t)(4 * i + v), &jobs, &S, &G);
        }
        if (fma_per_sample) *fma_per_sample = rg_anc_fma_per_sample(G) * (double)S * 576.0 * G / (double)frames;
        if (jobs.size() > 0x7fffffffu / RG_ANC_PHASES) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_ancestry_rate: too many tiles");
        const AncLayout l = anc_layout(views.size(), jobs.size());
        std::vector<unsigned char> head;
        anc_head(views.data(), views.size(), jobs, l, &head);
        RG_HIP(c, hipMalloc((void **)&d_arena, total + 16));
        RG_HIP(c, hipMalloc((void **)&d, l.end));
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        hipLaunchKernelGGL(rg_anc_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_arena), (uint64_t)(total / 4));
        RG_HIP(c, hipGetLastError());
        std::vector<unsigned char> h(host_tracks * stride);
        if (host_tracks) RG_HIP(c, hipMemcpyAsync(h.data(), d_arena, h.size(), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(d, head.data(), head.size(), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipStreamSynchronize(s));
        const size_t per_view = 2 * RG_ANC_ALIGNMENTS;
        std::vector<uint64_t> host_cnt((host_tracks ? 4 * host_tracks : 1) * per_view), dev_cnt((host_tracks ? 4 * host_tracks : 1) * per_view);
        auto host_pass = [&]() {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                uint64_t nf;
                for (size_t i = next.fetch_add(1); i < 4 * host_tracks; i = next.fetch_add(1))
                    rg_anc_serial_host(h.data(), views[i], o, &host_cnt[i * per_view], &host_cnt[i * per_view + RG_ANC_ALIGNMENTS], &nf);
            };
            std::vector<std::thread> pool;
            for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
        };
        const auto timed = [&](double *ms_out) -> int {
            float ms = 0.0f;
            RG_HIP(c, hipEventRecord(e0, s));
            const int r = anc_launch(c, d_arena, d, l, views.size(), jobs.size(), false, o.active_floor, s);
            if (r != RG_OK) return r;
            RG_HIP(c, hipEventRecord(e1, s));
            RG_HIP(c, hipStreamSynchronize(s));
            RG_HIP(c, hipEventElapsedTime(&ms, e0, e1));
            *ms_out = ms;
            return RG_OK;
        };
        int lr;
        const auto w0 = std::chrono::steady_clock::now();
        do {
            double ms;
            if ((lr = timed(&ms)) != RG_OK) return lr;
        } while (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count() < warm_ms);
        for (uint32_t r = 0; r < reps; ++r) {
            if ((lr = timed(&kernel_ms[r])) != RG_OK) return lr;
            if (host_tracks) {
                const auto t0 = std::chrono::steady_clock::now();
                host_pass();
                host_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
        }
        if (host_tracks) {
            RG_HIP(c, hipMemcpy(dev_cnt.data(), d + l.counts, dev_cnt.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            *mismatches = 0;
            for (size_t i = 0; i < 4 * host_tracks; ++i) *mismatches += memcmp(&dev_cnt[i * per_view], &host_cnt[i * per_view], per_view * sizeof(uint64_t)) != 0;
        }
        return RG_OK;
    };
    try {
        rc = run();
    } catch (const std::bad_alloc &) {
        rc = rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    } catch (const std::exception &ex) {
        rc = rg_set_err(c, RG_ERR_DEVICE, "rg_ancestry_rate: %s", ex.what());
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_arena) (void)hipFree(d_arena);
    return rc;
}
