// rg_flacenc.hip -- the FLAC encoder on the device (include/mp3rgain_amd_flacenc.h, rg_flacenc.h): three kernels and the seam.
//
//   analyse: one workgroup per frame.  A signal of the block (a channel, mid or side) is loaded from the arena planes into
//            LDS once and every candidate is sized exactly there (rg_flacenc.h: rg_fe_search); the frame's decision record
//            and its length in bytes go out.
//   layout : one workgroup per stream: the prefix sum of the frame lengths -> every frame's offset in its stream, the
//            stream's audio bytes, the smallest and largest frame.
//   write  : one workgroup per frame.  Subframe by subframe the residuals are recomputed from the record, lanes own runs of
//            consecutive residuals, a workgroup scan of the runs' bit lengths places every code, the bit image is built in
//            zeroed LDS with LDS atomics (a unary run costs only its stop bit), its whole words go out and the partial
//            last word is carried into the next subframe's image; the CRC-16 is folded over the bytes as they leave.
//
// The kernels run the frame functions of rg_flacenc.h with a 256-lane executor; the serial twin runs them with one lane.
// No global atomics apart from the one error flag, no scratch.  The launcher checks every stream against the arena before
// a launch, and the write kernel stores only inside the bytes its frame's record claims.
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "rg_ctx.h"
#include "rg_flac.h"
#include "rg_flac_md5.h"
#include "rg_flacenc.h"

// ---- the executors -----------------------------------------------------------------------------------------------------------
struct RgFeDev {
    __device__ uint32_t tid() const { return threadIdx.x; }
    __device__ uint32_t nt() const { return RG_FE_LANES; }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint64_t sum(uint64_t v, uint64_t *red) const {
        for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
        if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const uint64_t r = red[0] + red[1] + red[2] + red[3];
        __syncthreads();
        return r;
    }
    __device__ uint64_t any(uint64_t v, uint64_t *red) const {
        for (int o = 32; o; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o);
        if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const uint64_t r = red[0] | red[1] | red[2] | red[3];
        __syncthreads();
        return r;
    }
};

struct RgFeDevWrite : RgFeDev {
    __device__ void or_word(uint32_t *p, uint32_t v) const { atomicOr(p, v); }
    // exclusive scan over the lanes
    __device__ uint32_t exscan(uint32_t v, RgFeWriteWork &w) const {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t inc = v;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) w.scan[wave] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t k = 0; k < wave; ++k) base += w.scan[k];
        __syncthreads();
        return base + inc - v;
    }
    // The CRC-16 register after the image's first nbytes bytes, from `crc`.  Chunks of 64 bytes are counted from the END, so
    // only the first one is short and every fold step multiplies by one constant; the first chunk starts from `crc`.
    __device__ uint32_t crc(RgFeWriteWork &w, uint32_t nbytes, uint32_t crc) const {
        if (!nbytes) return crc;
        const int start = (int)nbytes - 64 * (int)(RG_FE_LANES - threadIdx.x);
        uint32_t c = 0;
        if (start + 64 > 0) {
            const uint32_t lo = start < 0 ? 0u : (uint32_t)start;
            if (lo == 0) c = crc;
            for (uint32_t b = lo; b < (uint32_t)(start + 64); ++b) c = rg_fe_crc_byte(c, (w.img[b >> 2] >> (24 - 8 * (b & 3u))) & 0xFFu, w.crc_table);
        }
        w.chunk[threadIdx.x] = c;
        for (uint32_t l = 0; l < 8; ++l) {
            const uint32_t s = 1u << l;
            __syncthreads();
            if ((threadIdx.x & (2 * s - 1)) == 0) w.chunk[threadIdx.x] = rg_fe_crc_mul(w.chunk[threadIdx.x], w.x512[l]) ^ w.chunk[threadIdx.x + s];
        }
        __syncthreads();
        const uint32_t r = w.chunk[0];
        __syncthreads();
        return r;
    }
};

// the stream that holds frame g of the call: the last one whose first_frame <= g (streams without frames share a first_frame
// with their successor and are passed over)
__device__ inline uint32_t rg_fe_stream_of(const RgFeStream *st, uint32_t n, uint64_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (st[mid].first_frame <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(RG_FE_LANES) void rg_flacenc_analyse_kernel(const RgFeStream *__restrict__ st, uint32_t n, RgFeFrame *__restrict__ recs) {
    __shared__ RgFeWork w;
    const uint64_t g = blockIdx.x;
    const RgFeStream s = st[rg_fe_stream_of(st, n, g)];
    RgFeDev x;
    rg_fe_analyse_frame(x, w, s, (uint32_t)(g - s.first_frame), &recs[g]);
}

struct RgFeLayout {
    uint64_t audio_bytes;
    uint32_t min_frame, max_frame;
};

__global__ __launch_bounds__(RG_FE_LANES) void rg_flacenc_layout_kernel(const RgFeStream *__restrict__ st, const RgFeFrame *__restrict__ recs,
                                                                        uint64_t *__restrict__ frame_at, RgFeLayout *__restrict__ lay) {
    __shared__ uint64_t sums[RG_FE_LANES];
    __shared__ uint32_t los[RG_FE_LANES], his[RG_FE_LANES];
    const RgFeStream s = st[blockIdx.x];
    const uint32_t nf = s.n_frames, per = (nf + RG_FE_LANES - 1) / RG_FE_LANES;
    const uint32_t a = min(threadIdx.x * per, nf), b = min(a + per, nf);
    uint64_t sum = 0;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t f = a; f < b; ++f) {
        const uint32_t v = recs[s.first_frame + f].bytes;
        sum += v;
        lo = min(lo, v);
        hi = max(hi, v);
    }
    sums[threadIdx.x] = sum;
    los[threadIdx.x] = lo;
    his[threadIdx.x] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (uint32_t k = 0; k < RG_FE_LANES; ++k) {
            const uint64_t v = sums[k];
            sums[k] = run;
            run += v;
            lo = min(lo, los[k]);
            hi = max(hi, his[k]);
        }
        lay[blockIdx.x].audio_bytes = run;
        lay[blockIdx.x].min_frame = nf ? lo : 0u;
        lay[blockIdx.x].max_frame = hi;
    }
    __syncthreads();
    uint64_t at = sums[threadIdx.x];
    for (uint32_t f = a; f < b; ++f) {
        frame_at[s.first_frame + f] = at;
        at += recs[s.first_frame + f].bytes;
    }
}

__global__ __launch_bounds__(RG_FE_LANES) void rg_flacenc_write_kernel(const RgFeStream *__restrict__ st, uint32_t n, const RgFeFrame *__restrict__ recs,
                                                                       const uint64_t *__restrict__ frame_at, uint8_t *__restrict__ out,
                                                                       uint32_t *__restrict__ fail) {
    __shared__ RgFeWriteWork w;
    const uint64_t g = blockIdx.x;
    const RgFeStream s = st[rg_fe_stream_of(st, n, g)];
    RgFeDevWrite x;
    rg_fe_write_init(x, w);
    rg_fe_write_frame(x, w, s, (uint32_t)(g - s.first_frame), recs[g], out + s.audio_at + frame_at[g]);
    __syncthreads();
    if (threadIdx.x == 0 && w.fail) atomicOr(fail, 1u);
}

// ---- the launcher --------------------------------------------------------------------------------------------------------------
static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

int rg_fe_device(rg_ctx *c, std::vector<RgFeStream> &st, const std::vector<std::vector<uint8_t>> *blocks, void *out, size_t out_capacity,
                 std::vector<uint8_t> *grow, uint64_t *offsets, rg_flac_encode_result *results, hipStream_t s, float *ms) {
    const size_t n = st.size();
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        st[i].first_frame = total;
        total += st[i].n_frames;
    }
    offsets[0] = 0;
    if (!n) return RG_OK;
    if (total > 0x7FFFFFFFull || n > 0x7FFFFFFFull) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_encode: %llu frames in one call", (unsigned long long)total);
    const size_t st_bytes = up16(n * sizeof(RgFeStream)), rec_bytes = up16((size_t)total * sizeof(RgFeFrame)), at_bytes = up16((size_t)total * 8),
                 lay_bytes = up16(n * sizeof(RgFeLayout));
    RG_HIP(c, c->d_flacenc.reserve(st_bytes + rec_bytes + at_bytes + lay_bytes + 16));
    unsigned char *d = c->d_flacenc.p;
    RgFeStream *d_st = reinterpret_cast<RgFeStream *>(d);
    RgFeFrame *d_recs = reinterpret_cast<RgFeFrame *>(d + st_bytes);
    uint64_t *d_at = reinterpret_cast<uint64_t *>(d + st_bytes + rec_bytes);
    RgFeLayout *d_lay = reinterpret_cast<RgFeLayout *>(d + st_bytes + rec_bytes + at_bytes);
    uint32_t *d_fail = reinterpret_cast<uint32_t *>(d + st_bytes + rec_bytes + at_bytes + lay_bytes);
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<RgFeLayout> lay(n);
    std::vector<uint8_t> md5(n * 16);
    uint32_t fail = 0;
    auto run = [&]() -> int {
        if (ms)
            for (auto &e : ev) RG_HIP(c, hipEventCreate(&e));
        RG_HIP(c, hipMemcpyAsync(d_st, st.data(), n * sizeof(RgFeStream), hipMemcpyHostToDevice, s));
        RG_HIP(c, hipMemsetAsync(d_fail, 0, 16, s));
        if (ms) RG_HIP(c, hipEventRecord(ev[0], s));
        if (total) {
            hipLaunchKernelGGL(rg_flacenc_analyse_kernel, dim3((uint32_t)total), dim3(RG_FE_LANES), 0, s, d_st, (uint32_t)n, d_recs);
            RG_HIP(c, hipGetLastError());
        }
        if (ms) RG_HIP(c, hipEventRecord(ev[1], s));
        hipLaunchKernelGGL(rg_flacenc_layout_kernel, dim3((uint32_t)n), dim3(RG_FE_LANES), 0, s, d_st, d_recs, d_at, d_lay);
        RG_HIP(c, hipGetLastError());
        if (ms) RG_HIP(c, hipEventRecord(ev[2], s));
        RG_HIP(c, hipMemcpyAsync(lay.data(), d_lay, n * sizeof(RgFeLayout), hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) {
            st[i].audio_at = offsets[i] + st[i].meta_bytes;
            offsets[i + 1] = st[i].audio_at + lay[i].audio_bytes;
        }
        if (grow) {
            grow->resize((size_t)offsets[n]);
            out = grow->data();
            out_capacity = grow->size();
        }
        if (offsets[n] > out_capacity)
            return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_encode_arena: the streams take %llu bytes, out has %zu", (unsigned long long)offsets[n], out_capacity);
        RG_HIP(c, c->d_flacenc_out.reserve((size_t)offsets[n] + 16));
        RG_HIP(c, hipMemcpyAsync(d_st, st.data(), n * sizeof(RgFeStream), hipMemcpyHostToDevice, s));
        if (ms) RG_HIP(c, hipEventRecord(ev[3], s));
        if (total) {
            hipLaunchKernelGGL(rg_flacenc_write_kernel, dim3((uint32_t)total), dim3(RG_FE_LANES), 0, s, d_st, (uint32_t)n, d_recs, d_at, c->d_flacenc_out.p, d_fail);
            RG_HIP(c, hipGetLastError());
        }
        if (ms) RG_HIP(c, hipEventRecord(ev[4], s));
        std::vector<RgFlacMd5Rec> mrecs(n);
        for (size_t i = 0; i < n; ++i) mrecs[i] = RgFlacMd5Rec{st[i].plane0, st[i].frames, st[i].channels, st[i].bps, st[i].elem_bytes, st[i].shift};
        const int rc = rg_flac_md5_device(c, mrecs.data(), n, md5.data(), s);
        if (rc != RG_OK) return rc;
        if (ms) RG_HIP(c, hipEventRecord(ev[5], s));
        RG_HIP(c, hipMemcpyAsync(out, c->d_flacenc_out.p, (size_t)offsets[n], hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipMemcpyAsync(&fail, d_fail, 4, hipMemcpyDeviceToHost, s));
        RG_HIP(c, hipStreamSynchronize(s));
        if (ms) {
            RG_HIP(c, hipEventElapsedTime(&ms[0], ev[0], ev[1]));
            RG_HIP(c, hipEventElapsedTime(&ms[1], ev[1], ev[2]));
            RG_HIP(c, hipEventElapsedTime(&ms[2], ev[3], ev[4]));
            RG_HIP(c, hipEventElapsedTime(&ms[3], ev[4], ev[5]));
        }
        return RG_OK;
    };
    const int rc = run();
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != RG_OK) return rc;
    if (fail) return rg_set_err(c, RG_ERR_STATE, "rg_flac_encode_arena: a frame's bits did not end where its record says (internal error)");
    for (size_t i = 0; i < n; ++i)
        rg_fe_finish_stream(st[i], lay[i].min_frame, lay[i].max_frame, lay[i].audio_bytes, &md5[16 * i], static_cast<uint8_t *>(out) + offsets[i], &results[i],
                            blocks && !(*blocks)[i].empty() ? (*blocks)[i].data() : nullptr, blocks ? (*blocks)[i].size() : 0);
    return RG_OK;
}

int rg_fe_verify_device(rg_ctx *c, const std::vector<RgFeStream> &st, const uint8_t *out, const uint64_t *offsets, rg_flac_encode_result *results,
                        std::vector<uint8_t> *ok, hipStream_t s) {
    const size_t n = st.size();
    ok->assign(n, 0);
    if (!n) return RG_OK;
    std::vector<std::vector<rg_flac_frame>> index(n);
    std::vector<RgFlacDevStream> ds(n);
    std::vector<size_t> at(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        rg_flac_info si;
        const uint8_t *bytes = out + offsets[i];
        const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
        if (rg_flac_index_vec(bytes, len, &index[i], &si) != RG_FLAC_OK) return rg_set_err(c, RG_ERR_STATE, "stream %zu does not index: %s", i, rg_flac_last_error());
        ds[i] = RgFlacDevStream{bytes, len, index[i].data(), (uint32_t)index[i].size(), si.channels, si.bits_per_sample, rgf::flac_elem_bytes(si.bits_per_sample),
                                rgf::flac_shift(si.bits_per_sample), nullptr, 0, 0, 0};
        at[i + 1] = at[i] + up16((size_t)si.frames * si.channels * ds[i].elem_bytes);
    }
    RG_HIP(c, c->d_flacenc_verify.reserve(at[n] + 16));
    for (size_t i = 0; i < n; ++i) ds[i].dst = c->d_flacenc_verify.p + at[i];
    int rc = rg_flacdev_decode(c, ds.data(), n, s);
    if (rc != RG_OK) return rc;
    std::vector<RgFlacMd5Rec> mrecs(n);
    for (size_t i = 0; i < n; ++i) mrecs[i] = RgFlacMd5Rec{ds[i].dst, ds[i].samples, ds[i].channels, ds[i].bps, ds[i].elem_bytes, ds[i].shift};
    std::vector<uint8_t> md5(n * 16);
    rc = rg_flac_md5_device(c, mrecs.data(), n, md5.data(), s);
    if (rc != RG_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
        memcpy(results[i].md5_decoded, &md5[16 * i], 16);
        (*ok)[i] = ds[i].dropped_frames == 0 && ds[i].samples == st[i].frames && ds[i].channels == st[i].channels && ds[i].bps == st[i].bps &&
                   memcmp(results[i].md5_decoded, results[i].md5_pcm, 16) == 0;
    }
    return RG_OK;
}

// the checks of a seam call and its streams against the arena at `base`
static int rg_fe_plan(rg_ctx *c, size_t n, const rg_track_desc *descs, const uint32_t *bps, const unsigned char *base, size_t arena_bytes,
                      const rg_flac_encode_options *options, std::vector<RgFeStream> *st) {
    char err[256] = "";
    uint32_t block, max_lpc, flags;
    int rc = rg_fe_options(options, &block, &max_lpc, &flags, err, sizeof err);
    if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    st->resize(n);
    for (size_t i = 0; i < n; ++i) {
        rc = rg_fe_stream(i, descs[i], bps[i], base, arena_bytes, block, max_lpc, &(*st)[i], err, sizeof err);
        if (rc != RG_OK) return rg_set_err(c, rc, "%s", err);
    }
    return RG_OK;
}

extern "C" int rg_flac_encode_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena, size_t arena_bytes,
                                    const rg_flac_encode_options *options, void *out, size_t out_capacity, uint64_t *offsets,
                                    rg_flac_encode_result *results) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c && route != 0) return RG_ERR_INVALID_ARG;  // the twin needs no context (its error text: rg_last_error(NULL))
    if (route != 0 && route != 1) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_encode_arena: route %d (0 = serial host twin, 1 = kernels)", route);
    if (route == 0) {
        char err[256] = "";
        const int rc = rg_fe_arena_host(n, descs, bps, arena, arena_bytes, options, out, out_capacity, offsets, results, err, sizeof err);
        return rc == RG_OK ? RG_OK : rg_set_err(c, rc, "%s", err);
    }
    if (!offsets || (n && (!descs || !bps || !results || (arena_bytes && !arena))) || (out_capacity && !out))
        return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_encode_arena: null array");
    try {
        std::vector<RgFeStream> st;
        int rc = rg_fe_plan(c, n, descs, bps, nullptr, arena_bytes, options, &st);  // the checks first, with no device yet
        if (rc != RG_OK) return rc;
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        RG_HIP(c, c->d_arena.reserve(((arena_bytes + 15) & ~(size_t)15) + 16));
        hipStream_t s = c->slots[0].stream;
        if (arena_bytes) RG_HIP(c, hipMemcpyAsync(c->d_arena.p, arena, arena_bytes, hipMemcpyHostToDevice, s));
        for (size_t i = 0; i < n; ++i) st[i].plane0 = c->d_arena.p + descs[i].offset_bytes;
        return rg_fe_device(c, st, nullptr, out, out_capacity, nullptr, offsets, results, s, nullptr);
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}

// ---- measurement hook (tools/flacenc_rate.py) ----------------------------------------------------------------------------------
// the read-only pass the kernels are set beside: every 16-byte word of the arena once, folded so that nothing is elided
__global__ __launch_bounds__(256) void rg_flacenc_read_kernel(const uint4 *__restrict__ src, uint64_t words, uint32_t *__restrict__ sink) {
    uint32_t acc = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        const uint4 v = src[w];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;  // (practically never: the loads stay)
}

extern "C" int rg_flac_encode_rate(void *ctx, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena, size_t arena_bytes,
                                   const rg_flac_encode_options *options, uint32_t reps, double *ms, uint64_t *stream_bytes) {
    rg_ctx *c = static_cast<rg_ctx *>(ctx);
    if (!c) return RG_ERR_INVALID_ARG;
    if (!n || !descs || !bps || !arena || !reps || !ms) return rg_set_err(c, RG_ERR_INVALID_ARG, "rg_flac_encode_rate: bad arguments");
    try {
        std::vector<RgFeStream> st;
        int rc = rg_fe_plan(c, n, descs, bps, nullptr, arena_bytes, options, &st);
        if (rc != RG_OK) return rc;
        rc = rg_bind_device(c);
        if (rc != RG_OK) return rc;
        RG_HIP(c, rg_sync_slots(c, c->n_slots));
        RG_HIP(c, c->d_arena.reserve(((arena_bytes + 15) & ~(size_t)15) + 16));
        hipStream_t s = c->slots[0].stream;
        RG_HIP(c, hipMemcpyAsync(c->d_arena.p, arena, arena_bytes, hipMemcpyHostToDevice, s));
        for (size_t i = 0; i < n; ++i) st[i].plane0 = c->d_arena.p + descs[i].offset_bytes;
        std::vector<uint64_t> offsets(n + 1);
        std::vector<rg_flac_encode_result> results(n);
        std::vector<uint8_t> out;
        std::vector<float> rounds[4];
        for (uint32_t r = 0; r < reps + 2; ++r) {  // round 0 finds the size, round 1 warms up; neither is reported
            float t[4] = {0, 0, 0, 0};
            rc = rg_fe_device(c, st, nullptr, out.data(), out.size(), nullptr, offsets.data(), results.data(), s, t);
            if (r == 0 && rc == RG_ERR_INVALID_ARG && offsets[n] > out.size()) {
                out.resize((size_t)offsets[n]);
                continue;
            }
            if (rc != RG_OK) return rc;
            if (r >= 2)
                for (int k = 0; k < 4; ++k) rounds[k].push_back(t[k]);
        }
        for (int k = 0; k < 4; ++k) {
            std::sort(rounds[k].begin(), rounds[k].end());
            ms[k] = rounds[k][rounds[k].size() / 2];
        }
        // the read-only pass over the same planes (the arena's whole 16-byte words), after a warm-up of its own
        hipEvent_t e0 = nullptr, e1 = nullptr;
        RG_HIP(c, hipEventCreate(&e0));
        RG_HIP(c, hipEventCreate(&e1));
        std::vector<float> reads;
        int rrc = RG_OK;
        for (uint32_t r = 0; r < reps + 1 && rrc == RG_OK; ++r) {
            float t = 0.0f;
            hipError_t e = hipEventRecord(e0, s);
            hipLaunchKernelGGL(rg_flacenc_read_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<const uint4 *>(c->d_arena.p), (uint64_t)(arena_bytes / 16),
                               reinterpret_cast<uint32_t *>(c->d_flacenc.p));
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipEventRecord(e1, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
            if (e != hipSuccess) rrc = rg_set_err(c, RG_ERR_DEVICE, "rg_flac_encode_rate: %s", hipGetErrorString(e));
            if (r) reads.push_back(t);
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (rrc != RG_OK) return rrc;
        std::sort(reads.begin(), reads.end());
        ms[4] = reads[reads.size() / 2];
        if (stream_bytes) *stream_bytes = offsets[n];
        return RG_OK;
    } catch (const std::bad_alloc &) {
        return rg_set_err(c, RG_ERR_NOMEM, "out of memory");
    }
}
