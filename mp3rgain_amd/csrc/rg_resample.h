// rg_resample.h -- internal: the rational resampler and the cross-rate fingerprint (include/mp3rgain_amd_resample.h) as
// rg_resample.hip (the kernel, its launcher and the seams), rg_resample_host.cpp (the plan, the tap tables, route 0 and the
// kernel's f32 arithmetic on the host) and rg_file_verify.hip (rg_same_recording_xrate) share it.  Everything behind y is the
// fingerprint's (rg_fprint.h): the tile walk over y as an arena of mono f32 tracks, the pair list, the match, the groups.  The
// L = 1 tracks of a launch are the key scan's decimation (rg_key.h: rg_key_decimate_device).  Both translation units are
// compiled without contraction.
#pragma once

#include <memory>
#include <vector>

#include "../../include/mp3rgain_amd_resample.h"
#include "rg_fprint.h"

#define RG_RS_LANES 256u
#define RG_RS_OUTPUTS 256u  // consecutive y of one workgroup, one per lane
// the staged samples of a workgroup at most: b_{j0 + 255} - b_{j0} <= ceil(255 M / L) <= 8160, and P <= 16 * 32 + 1
#define RG_RS_MAX_SPAN (255u * RG_RS_MAX_RATIO + 16u * RG_RS_MAX_RATIO + 1u)

// One track of a launch
struct RgRsTrack {
    uint64_t off0, off1;  // planes of the first two channels from the arena's base, in bytes
    uint64_t y_at;        // where its y lies in the resampled buffer, in floats (a multiple of 4)
    uint64_t first_wg;    // of this track among the launch's workgroups (the workgroups of one format are contiguous)
    uint32_t n, m;        // N, M_out
    uint32_t up, down;    // L, M; up = 0: the rate is not supported (M_out = 0)
    uint32_t taps;        // P
    uint32_t format, channels;  // channels: 1 or 2, the planes that count
    uint32_t hq_at;       // where the table of (L, M) starts in the launch's tables, in floats (L >= 2)
    uint32_t n_wg;        // ceil(M_out / 256); 0 for L = 1: those tracks are the key scan's decimation kernel's
    uint32_t recip;       // floor(2^32 / L) + 1: u / L = (u * recip) >> 32 while u L < 2^32
    uint32_t span;        // ceil(255 M / L) + P: the most samples one of its workgroups stages
    uint32_t reserved;
};  // 80 bytes

// Where a workgroup's first output starts: the host forms j0 M in 64 bits, the kernel goes on from here in 32
struct RgRsStart {
    uint32_t first;        // b_{j0}
    uint32_t phase_resid;  // p_{j0} | (j0 mod L) << 16
};

// The tap table of one (L, M)
struct RgRsFilter {
    uint32_t up, down, taps;
    std::vector<float> h;   // phase-major: h[p * P + k]
    std::vector<float> hq;  // tap-major, by output residue: hq[k * L + j mod L] = h[p_j][k]
};

RG_SPEC_HD uint32_t rg_rs_gcd(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}
// b_j and p_j: j M in 64 bits (j < 2^32, M <= 14112)
RG_SPEC_HD void rg_rs_window(uint64_t j, uint32_t up, uint32_t down, uint64_t *first, uint32_t *phase) {
    const uint64_t jm = j * down, b = (jm + up - 1u) / up;
    *first = b;
    *phase = (uint32_t)(b * up - jm);
}
// M_out of N frames
RG_SPEC_HD uint64_t rg_rs_count(uint64_t n, uint32_t up, uint32_t down, uint32_t taps) {
    return n < taps ? 0u : (n - taps) * up / down + 1u;
}

// ---- host side (rg_resample_host.cpp) -----------------------------------------------------------------------------------------
// the table of coprime (L, M), cached; L = M = 1 is the one tap 1
std::shared_ptr<const RgRsFilter> rg_rs_filter(uint32_t up, uint32_t down);
// the options of the cross-rate call, checked: NULL or a zero field = its default
int rg_xr_options(const rg_fingerprint_opts *opts, rg_fingerprint_opts *out, char *err, size_t err_len);
// track i's record of a launch, checked against the arena; everything but y_at, first_wg and hq_at
int rg_rs_track(size_t i, const rg_track_desc &t, size_t arena_bytes, RgRsTrack *out, char *err, size_t err_len);
// y_at (16-byte aligned runs) in track order, first_wg with the workgroups of one format contiguous (fmt_wg[f] .. fmt_wg[f + 1]);
// tables <- the hq of the (L, M) that occur, hq_at set; starts <- one record per workgroup; -> the floats of y
uint64_t rg_rs_plan(RgRsTrack *tracks, size_t n, uint64_t fmt_wg[4], std::vector<float> *tables, std::vector<RgRsStart> *starts);
// route 0 and route 2 of one track: y[0 .. M_out)
void rg_rs_serial_host(const unsigned char *arena, const RgRsTrack &t, float *y);
void rg_rs_folded_host(const unsigned char *arena, const RgRsTrack &t, float *y);
// the tile walk's record of a track whose y (M_out floats) lies at byte `off` of an f32 arena, at 11025 Hz
void rg_xr_fp_track(const RgRsTrack &t, uint64_t off, RgFpTrack *out);
void rg_rs_fill(const rg_track_desc &d, const RgRsTrack &t, uint64_t y_at, rg_resample_result *out);
void rg_xr_fill(const rg_track_desc &d, const RgRsTrack &t, const RgFpTrack &f, uint32_t dropped_frames, uint32_t nonfinite_frames, uint32_t index,
                uint64_t y_at, rg_xrate_result *out);
int rg_rs_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_resample_result *out, float *y_out, char *err,
                     size_t err_len);
int rg_xr_arena_host(int route, size_t n, const rg_track_desc *descs, const void *arena, size_t arena_bytes, rg_xrate_result *out, uint32_t *codes_out,
                     float *bands_out, float *y_out, char *err, size_t err_len);

#if defined(__HIPCC__)
struct rg_ctx;
// `n` tracks (rg_rs_track) in the device arena at `d_arena`, planned here; y goes to c->d_rs_y (track i's at tracks[i].y_at);
// `s` has been synchronised on return
int rg_resample_device(rg_ctx *c, const unsigned char *d_arena, RgRsTrack *tracks, size_t n, hipStream_t s);
// the resampler, then the fingerprint's tile walk over c->d_rs_y: fp[i] <- track i's tile record (codes_at and frames_at packed
// from codes_base and 0), codes to d_codes[codes_at ..], band energies to d_bands unless NULL, nonfinite[i] <- track i's count
int rg_xrate_device(rg_ctx *c, const unsigned char *d_arena, RgRsTrack *tracks, RgFpTrack *fp, size_t n, uint64_t codes_base, uint32_t *d_codes, float *d_bands,
                    uint32_t *nonfinite, hipStream_t s);
#endif
