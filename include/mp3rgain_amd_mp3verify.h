/* mp3rgain_amd_mp3verify.h -- C ABI of MP3 verification: what a bare MPEG Layer III stream says about its own integrity,
 * collected by one call.  Nothing here changes which frames any decoder drops.
 *
 * The two checksums
 *   CRC-16/ARC     polynomial 0x8005 reflected (0xA001), initial value 0, no final xor; "123456789" -> 0xBB3D.
 *                  The LAME extension's music CRC and tag CRC.
 *   frame CRC      polynomial 0x8005, MSB first, initial value 0xFFFF (ISO/IEC 11172-3): over header bytes 2 and 3 and the
 *                  side information of a frame whose protection bit is 0, compared with the 16-bit big-endian word behind
 *                  the header.
 *
 * The info tag
 *   The first frame behind an ID3v2 tag (rg_mp3_scan: first_frame_offset) is the TAG FRAME when "Xing" or "Info" lies behind
 *   its side information (two bytes later in a protected frame), or "VBRI" at byte 36.  A flags word follows the marker and says
 *   which of frames (4 bytes, bit 0), bytes (4, bit 1), TOC (100, bit 2) and quality (4, bit 3) follow it.  The 36-byte
 *   extension follows the present fields (flags 15: offset 0x78 from the marker) and counts as present only when its 9-byte
 *   version string starts with "LAME", "Lavc" or "Lavf" and all 36 bytes lie inside the frame.  Music length: big-endian at
 *   extension + 28; music CRC: + 32; tag CRC: + 34.  A VBRI header has no checksums: info_frame = 2 and nothing more.
 *
 * What is compared
 *   music CRC      CRC-16/ARC of [end of the tag frame, min(tag_frame_offset + music_length, file length)).
 *   tag CRC        matches when either rule gives the stored value: LAME's (the frame's bytes from its first up to the CRC
 *                  field) or libavformat's (the frame's first 190 bytes with the field's two bytes taken as zero; bytes
 *                  beyond the file count as absent).  tag_crc_computed is the matching rule's value, else LAME's rule's.
 *   LENGTH_MATCH   tag_frame_offset + music_length <= file length, and it is exactly where the frame walk's last frame ends.
 *   FRAME_COUNT_MATCH  the Xing `frames` field is present and equals the audio frames walked (the tag frame is not one).
 *   COMPLETE       no walked frame was dropped by the decode route.
 *   FRAME_CRCS_OK  no protected audio frame fails its CRC (also set when there is none).
 *   GAIN_TAG       an APEv2 MP3GAIN_UNDO item is present: gain was applied by rewriting global_gain bytes, which the music
 *                  CRC cannot follow; a music-CRC mismatch in such a file proves nothing.
 */
#ifndef MP3RGAIN_AMD_MP3VERIFY_H
#define MP3RGAIN_AMD_MP3VERIFY_H

#include <stddef.h>
#include <stdint.h>

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_MP3_VERIFY_HAS_INFO_TAG 1u
#define RG_MP3_VERIFY_HAS_LAME_EXT 2u
#define RG_MP3_VERIFY_TAG_CRC_MATCH 4u
#define RG_MP3_VERIFY_MUSIC_CRC_MATCH 8u
#define RG_MP3_VERIFY_LENGTH_MATCH 16u
#define RG_MP3_VERIFY_FRAME_COUNT_MATCH 32u
#define RG_MP3_VERIFY_COMPLETE 64u
#define RG_MP3_VERIFY_FRAME_CRCS_OK 128u
#define RG_MP3_VERIFY_GAIN_TAG 256u

/* rg_mp3_tag_info: what the tag frame holds */
typedef struct rg_mp3_tag_info {
    uint32_t info_frame;        /* 0 none, 1 Xing / Info, 2 VBRI                                              */
    uint32_t has_lame_ext;
    uint64_t tag_frame_offset;  /* rg_mp3_scan's first_frame_offset                                           */
    uint32_t tag_frame_bytes;   /* the tag frame's length from its header                                     */
    uint32_t xing_flags;
    uint32_t has_frames;        /* the flags word announces the frames field                                  */
    uint32_t xing_frames;
    uint32_t xing_bytes;
    uint32_t ext_offset;        /* of the extension, from the frame's first byte                              */
    uint32_t music_length;
    uint16_t music_crc;
    uint16_t tag_crc;
    char encoder[9];            /* the version string, as stored                                              */
    uint8_t reserved[7];
} rg_mp3_tag_info;

/* Host parser.  RG_OK (out->info_frame says whether there is a tag frame), RG_ERR_FORMAT: no MPEG Layer III stream. */
int rg_mp3_info_tag(const void *data, size_t len, rg_mp3_tag_info *out);

typedef struct rg_mp3_verify_result {
    int32_t status;             /* RG_OK, or why there is no verdict (every other field is then zero)         */
    uint32_t flags;             /* RG_MP3_VERIFY_*                                                            */
    uint32_t audio_frames;      /* audio frames the frame walk found                                          */
    uint32_t dropped_frames;    /* of those, frames the decode route dropped                                  */
    uint32_t protected_frames;  /* audio frames with the protection bit 0                                     */
    uint32_t frame_crc_failed;  /* of those, frames whose CRC word does not match                             */
    uint32_t junk_bytes;        /* bytes the walk skipped while resynchronising                               */
    uint32_t xing_frames;       /* the Xing `frames` field (0 when absent)                                    */
    uint32_t music_length;      /* LAME extension                                                             */
    uint32_t info_frame;        /* 0 none, 1 Xing / Info, 2 VBRI                                              */
    uint64_t audio_bytes;       /* bytes the music CRC was computed over                                      */
    uint16_t music_crc_stored;
    uint16_t music_crc_computed;
    uint16_t tag_crc_stored;
    uint16_t tag_crc_computed;
    char encoder[9];
    uint8_t xing_flags;         /* low byte of the Xing flags word: bit 0 frames, 1 bytes, 2 TOC, 3 quality   */
    uint8_t reserved[6];
} rg_mp3_verify_result;         /* 72 bytes */

/* Every file decoded by the route the analysis uses (no decoder command is run), its dropped frames counted, and its
 * checksums computed on the device the context is bound to (with tuning key 6 = 0, the host decoder, by the host twin).
 * A failing file fails alone: RG_ERR_IO when it cannot be opened, RG_ERR_FORMAT for anything that is not a bare MPEG
 * Layer III stream (WAV, FLAC and MPEG audio inside MP4 included); its text: rg_tracks_error(ctx, i). */
int rg_mp3_verify(rg_ctx *ctx, const char *const *paths, size_t n, rg_mp3_verify_result *out);

/* The host twin of rg_mp3_verify for one stream in memory: the host decoder (rg_mp3_decode_f32) says which frames are
 * dropped and the host twin of both CRCs computes the checksums.  No GPU, no context.  Returns out->status. */
int rg_mp3_verify_data(const void *data, size_t len, rg_mp3_verify_result *out);

/* ---- test seams --------------------------------------------------------------------------------------------------------
 * route 0: the host twin (ctx may be NULL); route 1: `bytes` copied to the device, then the kernels of the file call.
 * rg_mp3_crc_ranges: out[i] <- CRC-16/ARC of bytes[offsets[i], offsets[i] + lengths[i]).  A range not wholly inside the
 * buffer is refused with RG_ERR_INVALID_ARG and nothing is launched.
 * rg_mp3_frame_crc_check: out_ok[i] <- 1 when the frame at frame_offsets[i] has a valid Layer III header with the
 * protection bit 0, its side information lies inside the buffer and its CRC word matches; else 0.  An offset whose header
 * and CRC word (6 bytes) do not lie inside the buffer is refused with RG_ERR_INVALID_ARG. */
int rg_mp3_crc_ranges(rg_ctx *ctx, int route, size_t n, const uint64_t *offsets, const uint64_t *lengths, const void *bytes,
                      size_t nbytes, uint16_t *out);
int rg_mp3_frame_crc_check(rg_ctx *ctx, int route, size_t n_frames, const uint64_t *frame_offsets, const void *bytes,
                           size_t nbytes, uint8_t *out_ok);

/* CRC-16/ARC of `data` by the kernels' arithmetic -- chunks counted from the end, the trees, the powers of x -- run on the host:
 * the combine without a GPU. */
uint16_t rg_mp3_crc_folded_host(const void *data, size_t len);

/* Measurement hook (tools/mp3_crc_rate.py): `n` streams of `stream_bytes` pseudo-random bytes filled on the device, then
 * `reps` alternating rounds after one warm-up: the chunk and fold kernels over all streams (dev_ms[r], HIP events) and the
 * host twin over the first `host_streams` streams on `threads` threads (host_ms[r]); the same for the frame-CRC kernel over
 * `n_frames` synthetic protected frames (frame_dev_ms / frame_host_ms).  *mismatches: host results that differ from the
 * device's. */
int rg_mp3_crc_rate(rg_ctx *ctx, size_t n, uint64_t stream_bytes, size_t host_streams, uint32_t threads, uint32_t reps,
                    size_t n_frames, double *dev_ms, double *host_ms, double *frame_dev_ms, double *frame_host_ms,
                    size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* MP3RGAIN_AMD_MP3VERIFY_H */
