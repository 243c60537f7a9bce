// rg_pcm_plane.h -- internal, header-only: what the scans that read planar PCM where it lies in an arena (rg_stats.h,
// rg_spectrum.h, rg_dr.h, rg_stereo.h, rg_ancestry.h) share on the host: what a sample format is, how a stored sample is read, the checks of
// a track descriptor against the scan's limits and against the arena, and the argument checks of a test seam's host routes.
// Plain C++ that also compiles under hipcc; no device and no context, so a sanitizer build of one *_host.cpp needs nothing else.
//
// The checks are two functions because a scan may have one of its own between them (stats: bits, DR: the block length), and a
// descriptor that is wrong in two ways reports the first: format, the scan's own, place.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mp3rgain_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_PCM_HD __host__ __device__ inline
#else
#define RG_PCM_HD inline
#endif

// ---- sample formats ----------------------------------------------------------------------------------------------------------
RG_PCM_HD bool rg_pcm_is_planar(uint32_t format) { return format == RG_FMT_F32_PLANAR || format == RG_FMT_S16_PLANAR || format == RG_FMT_S32_PLANAR; }
RG_PCM_HD uint32_t rg_pcm_width(uint32_t format) { return format == RG_FMT_S16_PLANAR ? 16u : 32u; }  // W: bits of the container
RG_PCM_HD uint32_t rg_pcm_bps(uint32_t format) { return format == RG_FMT_S16_PLANAR ? 2u : 4u; }      // bytes per sample

// sample k of a plane as the stored pattern, S16 sign-extended (planes are only sample-aligned)
inline uint32_t rg_pcm_raw_at(const unsigned char *plane, uint32_t format, uint64_t k) {
    if (format == RG_FMT_S16_PLANAR) {
        int16_t s;
        memcpy(&s, plane + 2 * k, 2);
        return (uint32_t)(int32_t)s;
    }
    uint32_t u;
    memcpy(&u, plane + 4 * k, 4);
    return u;
}

// ---- a track descriptor against a scan and an arena --------------------------------------------------------------------------
// RG_ERR_FORMAT unless track i is 1 .. max_channels planes of one of the three formats and fewer than 2^32 frames.  `takes`: the
// scan as the text names it ("pcm stats take", "the spectrum takes"); the text goes to err[err_len].
inline int rg_pcm_check_format(size_t i, const rg_track_desc &t, uint32_t max_channels, const char *takes, char *err, size_t err_len) {
    if (!rg_pcm_is_planar(t.format)) {
        snprintf(err, err_len, "track %zu: format %u is not a planar PCM format", i, (unsigned)t.format);
        return RG_ERR_FORMAT;
    }
    if (t.channels < 1 || t.channels > max_channels) {
        snprintf(err, err_len, "track %zu: %u channel(s), %s 1 to %u", i, (unsigned)t.channels, takes, max_channels);
        return RG_ERR_FORMAT;
    }
    if (t.frames >= ((uint64_t)1 << 32)) {
        snprintf(err, err_len, "track %zu: %llu frames, %s fewer than 2^32", i, (unsigned long long)t.frames, takes);
        return RG_ERR_FORMAT;
    }
    return RG_OK;
}
// RG_ERR_INVALID_ARG unless the planes of track i (which has passed rg_pcm_check_format) start sample-aligned and lie inside an
// arena of `arena_bytes` bytes
inline int rg_pcm_check_place(size_t i, const rg_track_desc &t, size_t arena_bytes, char *err, size_t err_len) {
    const uint32_t bps = rg_pcm_bps(t.format);
    if (t.offset_bytes % bps) {
        snprintf(err, err_len, "track %zu: offset %llu is not sample-aligned", i, (unsigned long long)t.offset_bytes);
        return RG_ERR_INVALID_ARG;
    }
    if (t.offset_bytes > arena_bytes || t.frames > (arena_bytes - t.offset_bytes) / ((size_t)bps * t.channels)) {
        snprintf(err, err_len, "track %zu: its planes reach beyond the arena (%zu bytes)", i, arena_bytes);
        return RG_ERR_INVALID_ARG;
    }
    return RG_OK;
}
// where the plane of channel c starts, from the arena's base, in bytes
inline uint64_t rg_pcm_plane_off(const rg_track_desc &t, uint32_t c) { return t.offset_bytes + (uint64_t)c * t.frames * rg_pcm_bps(t.format); }

// ---- the host routes of a test seam ------------------------------------------------------------------------------------------
// the arrays of a seam called `name` over n tracks: RG_ERR_INVALID_ARG with the text for one that is missing
inline int rg_pcm_check_arrays(const char *name, size_t n, const void *descs, const void *out, const void *arena, size_t arena_bytes, char *err,
                               size_t err_len) {
    if (!n || (descs && out && (arena || !arena_bytes))) return RG_OK;
    snprintf(err, err_len, "%s: null array", name);
    return RG_ERR_INVALID_ARG;
}
// ... and its route, which has to be one the host walks.  `route2`: what the seam calls route 2 ("folded")
inline int rg_pcm_check_host_route(const char *name, const char *route2, int route, size_t n, const void *descs, const void *out, const void *arena,
                                   size_t arena_bytes, char *err, size_t err_len) {
    if (route != 0 && route != 2) {
        snprintf(err, err_len, "%s: route %d is not a host route (0 = serial twin, 2 = %s)", name, route, route2);
        return RG_ERR_INVALID_ARG;
    }
    return rg_pcm_check_arrays(name, n, descs, out, arena, arena_bytes, err, err_len);
}
