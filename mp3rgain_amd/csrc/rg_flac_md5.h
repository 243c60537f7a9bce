// rg_flac_md5.h -- internal: the MD5 of decoded FLAC audio in the analysis arena (rg_flac_md5.hip), as the file layer's
// verify call (rg_file_verify.hip: rg_flac_verify) uses it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mp3rgain_amd.h"

struct rg_ctx;

#define RG_FLAC_MD5_BLOCK 64  // one wave per block: the streams of a call spread over as many CUs as there are waves

// One stream of a launch: where its planes lie and how a sample sits in its element.  The lane that takes record i writes
// digest i.
struct RgFlacMd5Rec {
    const unsigned char *plane0;  // plane c at plane0 + c * frames * elem_bytes
    uint64_t frames;              // PCM frames per channel
    uint32_t channels, bps;
    uint32_t elem_bytes;          // 2: S16 planar, 4: S32 planar
    uint32_t shift;               // the sample is the element >> shift (arithmetic)
};                                // 32 bytes

// The record of stream i, described by `t` (format S16 or S32 planar, left-justified) in an arena of `arena_bytes` bytes at
// `base` (host or device).  RG_ERR_INVALID_ARG, with a text, unless every plane lies inside the arena, sample-aligned.
int rg_flac_md5_record(rg_ctx *c, size_t i, const rg_track_desc &t, uint32_t bps, const unsigned char *base, size_t arena_bytes,
                       RgFlacMd5Rec *out);
// the host twin: the record's planes are host memory
void rg_flac_md5_host(const RgFlacMd5Rec &r, uint8_t out[16]);
// `n` records of device planes: one launch on `s`, digests[16 * i ..] <- stream i; `s` has been synchronised on return
int rg_flac_md5_device(rg_ctx *c, const RgFlacMd5Rec *recs, size_t n, uint8_t *digests, hipStream_t s);
