// rg_fprint.h -- internal: the duplicate finder (include/mp3rgain_amd_fingerprint.h) as rg_fprint.hip (the fingerprint kernels,
// their launcher and seam), rg_fprint_match.hip (the match kernel and its seam), rg_fprint_host.cpp (the serial twins, the
// kernels' f32 arithmetic on the host, the groups) and rg_file_verify.hip (rg_same_recording) share it.  The transform is the
// spectral scan's (rg_spectrum.h: tables, passes, rg_spec_dft16); what is written once here for both sides is how a band of
// the two frames of a pair is summed and how a code comes from two rows of band energies.  Both translation units are compiled
// without contraction, so the two give the same bits.
#pragma once

#include <vector>

#include "../../include/mp3rgain_amd_fingerprint.h"
#include "rg_spectrum.h"

#define RG_FP_LANES 256u
#define RG_FP_TILE_CODES 7u    // T: codes of one workgroup
#define RG_FP_TILE_FRAMES 8u   // T + 1 frames, four pairs; the first is the last frame of the tile before
#define RG_FP_STAGE (RG_FP_TILE_CODES * RG_FP_HOP + RG_FP_FRAME)  // down-mixed samples of a tile: 7680 floats, 30 KB
#define RG_FP_MATCH_LANES 256u
#define RG_FP_LAGS_PER_LANE 16u  // ceil((2 * RG_FP_MAX_RADIUS + 1) / 256)

// One track of a launch
struct RgFpTrack {
    uint64_t off0, off1;  // planes of the first two channels from the arena's base, in bytes (off1 unused for one channel)
    uint64_t first_tile;  // of this track among the launch's tiles (the tiles of one format are contiguous)
    uint64_t codes_at;    // where its codes go, in codes
    uint64_t frames_at;   // where its band energies go, in frames
    uint32_t n;           // N
    uint32_t frames;      // F (0 at an unsupported rate)
    uint32_t n_tiles;     // F == 0 ? 0 : max(1, ceil((F - 1) / T))
    uint32_t format;      // rg_sample_format
    uint32_t channels;    // 1 or 2: the planes that count
    uint32_t rate_ok;
    uint32_t e[RG_FP_BANDS + 1];
};  // 200 bytes

// One compared pair of a match launch
struct RgFpPair {
    uint64_t a_at, b_at;  // the probe side's and the other side's codes, in codes
    uint32_t ka, kb;
    uint32_t rec;         // its record
    uint32_t flags;       // RG_FP_PAIR_COMPARED, with RG_FP_PAIR_PROBE_J
};  // 32 bytes

RG_SPEC_HD uint32_t rg_fp_frames(uint64_t n) { return n < RG_FP_FRAME ? 0u : (uint32_t)((n - RG_FP_FRAME) / RG_FP_HOP + 1u); }

// bins b0 .. b1 - 1 of frame `which` (0: the real part, 1: the imaginary part) of the pair whose transform z(k) = Z[k] is,
// 1 <= k <= 4095: the powers summed in f32 in bin order
template <class Z>
RG_SPEC_HD float rg_fp_band(Z z, uint32_t b0, uint32_t b1, uint32_t which) {
    float s = 0.0f;
    for (uint32_t bin = b0; bin < b1; ++bin) {
        const RgSpecC u = z(bin), w = z(RG_SPEC_FRAME - bin);
        const float re = which ? u.y + w.y : u.x + w.x, im = which ? w.x - u.x : u.y - w.y;
        s += (re * re + im * im) * 0.25f;
    }
    return s;
}

// the code of frame n from E[n - 1] (`prev`) and E[n] (`cur`), 33 floats each
RG_SPEC_HD uint32_t rg_fp_code(const float *prev, const float *cur) {
    uint32_t code = 0;
    for (uint32_t m = 0; m < 32; ++m) {
        const float d = (cur[m] - cur[m + 1]) - (prev[m] - prev[m + 1]);
        if (d > 0.0f) code |= 1u << m;
    }
    return code;
}

// is x = (a + b) * 0.5f, or a float sample, a NaN or Inf
RG_SPEC_HD bool rg_fp_nonfinite(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u & 0x7F800000u) == 0x7F800000u;
}

// the best lag so far of a pair; bits == 0: none
struct RgFpBest {
    uint32_t errors, bits;
    int32_t lag;
};
// is x better than y: the smaller errors / bits, then the smaller |d|, then the negative d
RG_SPEC_HD bool rg_fp_better(const RgFpBest &x, const RgFpBest &y) {
    if (!x.bits) return false;
    if (!y.bits) return true;
    const uint64_t l = (uint64_t)x.errors * y.bits, r = (uint64_t)y.errors * x.bits;
    if (l != r) return l < r;
    const int32_t ax = x.lag < 0 ? -x.lag : x.lag, ay = y.lag < 0 ? -y.lag : y.lag;
    if (ax != ay) return ax < ay;
    return x.lag < y.lag;
}
RG_SPEC_HD void rg_fp_close(const RgFpBest &b, uint32_t pair_flags, uint32_t max_ber_permille, rg_fingerprint_pair_record *out) {
    if (!b.bits) {
        *out = rg_fingerprint_pair_record{0u, 0u, 0, RG_FP_PAIR_SKIPPED};
        return;
    }
    const bool match = (uint64_t)b.errors * 1000u <= (uint64_t)b.bits * max_ber_permille;
    *out = rg_fingerprint_pair_record{b.errors, b.bits, b.lag, pair_flags | (match ? RG_FP_PAIR_MATCH : 0u)};
}
// where probe p of `probes` starts in a probe side of ka codes
RG_SPEC_HD uint32_t rg_fp_probe_start(uint32_t p, uint32_t ka, uint32_t block, uint32_t probes) {
    return (uint32_t)((uint64_t)(2u * p + 1u) * (ka - block) / (2u * probes));
}

// ---- host side (rg_fprint_host.cpp) ------------------------------------------------------------------------------------------
// the options, checked: NULL or a zero field = the default
int rg_fp_options(const rg_fingerprint_opts *opts, rg_fingerprint_opts *out, char *err, size_t err_len);
// track i's record of a launch, checked against the arena; everything but first_tile, codes_at and frames_at
int rg_fp_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgFpTrack *out, char *err, size_t err_len);
// first_tile of tracks[0 .. n), the tiles of one format contiguous: fmt_tile[f] .. fmt_tile[f + 1]; codes_at and frames_at
// packed in track order from codes_base / frames_base; -> tiles
uint64_t rg_fp_plan(RgFpTrack *tracks, size_t n, uint64_t fmt_tile[4], uint64_t codes_base, uint64_t frames_base);
// route 0 and route 2 of one track: codes[0 .. K), bands[0 .. 33 F) (either may be NULL), -> non-finite frames
uint32_t rg_fp_serial_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands);
uint32_t rg_fp_folded_host(const unsigned char *arena, const RgFpTrack &t, uint32_t *codes, float *bands);
void rg_fp_fill(const rg_track_desc &d, const RgFpTrack &t, uint32_t dropped_frames, uint32_t nonfinite_frames, uint32_t index, rg_fingerprint_result *out);
int rg_fp_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_fingerprint_result *out,
                     uint32_t *codes_out, float *bands_out, char *err, size_t err_len);
// the compared pairs of n tracks (counts, rates, where each track's codes start) at `o`; every record that is not compared is
// filled here (RG_FP_PAIR_SKIPPED)
void rg_fp_pairs(size_t n, const uint32_t *counts, const uint32_t *rates, const uint64_t *at, const rg_fingerprint_opts &o, std::vector<RgFpPair> *pairs,
                 rg_fingerprint_pair_record *records);
// one compared pair on the host
void rg_fp_match_host(const uint32_t *codes, const RgFpPair &p, const rg_fingerprint_opts &o, rg_fingerprint_pair_record *out);
// route 0 of rg_fingerprint_match_codes: the pair list and every compared pair, serially
int rg_fp_match_codes_host(size_t n, const uint32_t *counts, const uint32_t *rates, const uint32_t *codes, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` tracks in the device arena at `d_arena`: the kernels on `s`; codes to d_codes[codes_at ..], band energies to
// d_bands[frames_at * 33 ..] unless NULL, nonfinite[i] <- track i's count; `s` has been synchronised on return
int rg_fprint_device(rg_ctx *c, const unsigned char *d_arena, RgFpTrack *tracks, size_t n, uint32_t *d_codes, float *d_bands, uint32_t *nonfinite,
                     hipStream_t s);
// the compared pairs over the device codes at d_codes: records[p.rec] <- pair p; `s` has been synchronised on return
int rg_fprint_match_device(rg_ctx *c, const uint32_t *d_codes, const std::vector<RgFpPair> &pairs, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *records, hipStream_t s);
// the match kernel over `count` pairs at d_pairs, enqueued on `s` (rg_fingerprint_rate times it)
int rg_fprint_match_launch(rg_ctx *c, const uint32_t *d_codes, const RgFpPair *d_pairs, size_t count, const rg_fingerprint_opts &o,
                           rg_fingerprint_pair_record *d_records, hipStream_t s);
#endif
