// rg_r128.h -- what the EBU R 128 path's translation units share: the host design (rg_r128_design.cpp), the device
// descriptors and the host driver (rg_r128.hip), the file-level entry points (rg_files.hip).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mp3rgain_amd_r128.h"

#define RG_R128_TP_TAPS 49
#define RG_R128_WARM_HOPS 3   // a lane starts this many hops early from the zero state
#define RG_R128_MAX_S 4096

struct RgR128Design {
    double b1[3], a1[3], b2[3], a2[3];
    uint32_t hop, tp_factor;
};
// long double derivation from the analogue prototypes; false outside 8000..384000 Hz
bool rg_r128_design(uint32_t rate, RgR128Design *out);
// the interpolator's taps, generated here and nowhere else: f64, rounded once to f32
void rg_r128_tp_table(uint32_t factor, float *taps /* RG_R128_TP_TAPS */);

// One track of a launch.  Lanes [lane_base, lane_base + nch * runs) belong to it, channel-major: lane = c * runs + r owns hops
// [r S, min((r + 1) S, H)) of channel c.
struct RgR128TrackDev {
    const unsigned char *ch[8];  // the planes of channels 0 .. nch-1, nullptr from there on
    double *e;                   // hop energies [nch][H]; behind the weighted fold (rg_r128_surround.hip): nch = 1, the folded row
    uint64_t frames;
    uint64_t lane_base;
    uint64_t z_base;             // first block of the track in block_z_out
    uint64_t tile_base;          // true peak: first block (a chunk of tiles) of the track in its launch
    uint32_t hop, H, runs, nch, S, index, tp_factor, sample_rate, format, pad;
    double b[3];                 // stage 1 numerator times the format's full-scale factor (a power of two: exact)
    double a1[2], a2[2];         // denominators of stage 1 and stage 2 (a[1], a[2])
};

struct rg_ctx;
// Loudness (and true peak) of n tracks whose PCM is on the device.  keep_for_album: the tracks' hop energies stay on the
// device until rg_r128_album_end runs the album stage over them (rg_r128_albums_stage with one album; call
// rg_r128_album_reset first).  dyn_out (without keep_for_album) and dyn_out / album_dyn_out of rg_r128_album_end (every
// kept track, in input order): nullptr, or loudness range and maxima are computed too (rg_r128_range.hip) after the
// launches of the plain call, which do not change; st_z_out goes with them.
// tr_out: nullptr, or the tracks' device descriptors go there (rg_r128_albums_stage reads them); their hop energies are in
// the context's own buffer until the next call, or, with e_out, in a buffer of their own that the caller frees (hipFree).
// weights: nullptr (every track by the context's channel mode: a pair, or rg_r128_layout_weights(channels, 0)), or one entry
// per track.  A weighted track of at most two channels whose used weights are all 1.0 is a plain track; any other runs all
// its channels through the main kernel into a scratch area and is folded to one row (rg_r128_surround.hip), which is what
// everything behind sees (nch = 1 in tr_out, in the kept descriptors and in the gate kernel's).
int rg_r128_run(rg_ctx *c, const rg_track_desc *tracks, size_t n, const void *d_base, size_t pcm_bytes, int want_true_peak,
                int keep_for_album, rg_r128_track_result *out, double *block_z_out, rg_r128_dynamics *dyn_out = nullptr,
                double *st_z_out = nullptr, RgR128TrackDev *tr_out = nullptr, double **e_out = nullptr,
                const rg_r128_channel_weights *weights = nullptr);
int rg_r128_channel_mode(rg_ctx *c);  // RG_R128_CHANNELS_*
// arguments of a weighted track: 1 to 8 channels, every used weight finite and >= 0; else RG_ERR_INVALID_ARG naming track t
int rg_r128_check_weights(rg_ctx *c, size_t t, uint32_t channels, const rg_r128_channel_weights *w);

// rg_r128_surround.hip: e[h] = sum over the channels with w != 0 of w_c * e_c[h], ascending c, every product and every sum
// rounded on its own; all weights zero: 0.  One launch over n_items tracks on the HIP stream `stream`, not waited for; the
// return value is the launch's hipError_t.
struct RgR128FoldItem {
    const double *src;    // [nch][H]
    double *dst;          // [H]
    uint64_t block_base;  // first workgroup of the track in the launch
    uint32_t H, nch;
    double w[8];
};
#define RG_R128_FOLD_BLOCK 256
int rg_r128_fold_launch(const RgR128FoldItem *d_items, uint32_t n_items, uint64_t blocks, void *stream);

void rg_r128_album_reset(rg_ctx *c);
int rg_r128_album_end(rg_ctx *c, int want_true_peak, rg_r128_album_result *album_out, rg_r128_dynamics *dyn_out = nullptr,
                      rg_r128_dynamics *album_dyn_out = nullptr, double *st_z_out = nullptr);

// the absolute gate of both measures, -70 LUFS as a mean square (rg_r128.hip)
double rg_r128_abs_gate();

// rg_r128_range.hip: loudness range and momentary / short-term maxima of n tracks whose hop energies (tr[i].e) are on the
// device, waited for; res[i].flags marks the tracks that are not finite.  *slot holds the stage's device buffers between
// calls (rg_r128_range_free).  Albums are rg_r128_albums_stage's.
int rg_r128_dynamics_run(rg_ctx *c, void **slot, const RgR128TrackDev *tr, const rg_r128_track_result *res, size_t n,
                         rg_r128_dynamics *out, double *st_z_out);
void rg_r128_dynamics_none(rg_r128_dynamics *d);  // the values of a track or an album without blocks
void rg_r128_range_free(void *slot);
void rg_r128_dynamics_nan(rg_r128_dynamics *d);   // the values of a track or an album that is not finite

// Stage 1 and the per-track selection over n tracks, launched on the context's stream and not waited for: what they leave
// on the device (in *slot's buffers, until the next call) and where every track's short-term blocks lie.
struct RgR128RangeDev {
    const double *st = nullptr;                  // every track's short-term blocks, track after track
    const unsigned long long *max_bits = nullptr;  // [n][2]: momentary, short-term
    const rg_r128_dynamics *dyn = nullptr;       // [n]
    uint64_t total = 0;
    std::vector<uint64_t> st_base;               // [n + 1]
};
int rg_r128_range_tracks(rg_ctx *c, void **slot, const RgR128TrackDev *tr, size_t n, RgR128RangeDev *dev);

// rg_r128_albums.hip: the album stage of one album or of many at once.  tr / res: n tracks whose hop energies are on the device;
// album a is tracks [first[a], first[a + 1]), first[n_albums] <= n (tracks past it belong to no album and get their own
// dynamics only).  albums_dyn_out: nullptr, or loudness range and maxima of every track (dyn_out, may be nullptr) and every
// album are computed too.  Empty albums get the record of rg_r128_analyze_album for n = 0.
#define RG_R128A_ROUND 64  // wide albums whose selection state is on the device at once
int rg_r128_albums_stage(rg_ctx *c, const RgR128TrackDev *tr, const rg_r128_track_result *res, size_t n, const size_t *first,
                         size_t n_albums, int want_true_peak, rg_r128_album_result *albums_out, rg_r128_dynamics *dyn_out,
                         rg_r128_dynamics *albums_dyn_out, double *st_z_out);
// the context's album selection mode and the slot of its range buffers (rg_r128.hip owns both)
int rg_r128_album_select(rg_ctx *c);
void **rg_r128_range_slot(rg_ctx *c);
void **rg_r128_albums_slot(rg_ctx *c);  // the stage's device buffers between calls
void rg_r128_albums_free(void *slot);
