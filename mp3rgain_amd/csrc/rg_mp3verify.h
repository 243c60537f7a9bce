// rg_mp3verify.h -- internal: what rg_mp3verify.cpp (host: info-tag parser, frame walk, host twin of both CRCs, the result
// record), rg_mp3_crc.hip (the kernels and their launcher) and rg_file_verify.hip (rg_mp3_verify) share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "../../include/mp3rgain_amd_dec.h"
#include "../../include/mp3rgain_amd_mp3verify.h"

// rg_mp3dec.cpp: rg_mp3_scan's walk with the places it visits
extern "C" int rg_mp3_walk_offsets(const void *data, size_t len, uint64_t *offsets, size_t cap, size_t *n_frames, uint64_t *last_end,
                                   rg_mp3_stream_info *out);

// What the host finds in one stream before any checksum is computed
struct RgMp3VerifyPlan {
    rg_mp3_tag_info tag{};
    rg_mp3_stream_info si{};
    uint64_t last_end = 0;            // where the walk's last audio frame ends
    std::vector<uint64_t> prot;       // offsets of the audio frames whose protection bit is 0
    uint64_t music_off = 0, music_len = 0;  // the music CRC's range (empty without the extension)
    bool gain_tag = false;
};
// RG_OK, or RG_ERR_FORMAT: no MPEG Layer III stream
int rg_mp3_verify_plan(const uint8_t *d, size_t len, RgMp3VerifyPlan *plan);
// the record of one stream from its plan, the decode route's dropped frames and the computed checksums
void rg_mp3_verify_fill(const uint8_t *d, size_t len, const RgMp3VerifyPlan &plan, uint32_t dropped, uint16_t music_crc, uint32_t crc_failed,
                        rg_mp3_verify_result *r);
// host twins
uint16_t rg_mp3_crc_range_host(const uint8_t *bytes, uint64_t off, uint64_t len);
uint32_t rg_mp3_frame_crc_host(const uint8_t *bytes, uint64_t nbytes, uint64_t off);

// rg_mp3_crc.hip: one launch of the kernels.  `bytes` (host) goes to the device together with the range and frame tables in
// one copy; crc_out[n_ranges] and ok_out[n_frames] come back.  Ranges and frames are checked against nbytes first.
struct RgMp3CrcJob {
    const uint8_t *const *parts = nullptr;  // the buffer is the concatenation of these host blocks, each at part_off[k]
    const uint64_t *part_off = nullptr;
    const uint64_t *part_len = nullptr;
    size_t n_parts = 0;
    uint64_t nbytes = 0;
    const uint64_t *range_off = nullptr, *range_len = nullptr;
    size_t n_ranges = 0;
    const uint64_t *frame_off = nullptr;
    size_t n_frames = 0;
    uint16_t *crc_out = nullptr;
    uint8_t *ok_out = nullptr;
};
struct rg_ctx;
int rg_mp3_crc_check_job(rg_ctx *c, const RgMp3CrcJob &job);
#if defined(__HIPCC__)
int rg_mp3_crc_device(rg_ctx *c, const RgMp3CrcJob &job, hipStream_t s);
#endif
