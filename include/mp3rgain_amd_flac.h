/* mp3rgain_amd_flac.h -- C ABI of the FLAC decode row: a native FLAC stream (optionally behind an ID3v2 tag) -> planar
 * integer PCM, on the host (rg_flac_decode_s32) and on the device (rg_flac_decode_device, and the file-level entry points
 * of mp3rgain_amd.h, tuning key 14).
 *
 * Scope: every subframe type (CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32 with up to 15-bit coefficients), wasted bits,
 * Rice / Rice2 partitions of order 0-15 with escape codes, independent (1-8 channels), left/side, right/side and mid/side
 * channel assignments, every block-size and sample-rate header code, 4-24 bits per sample.  A stream of 25-32 bits per
 * sample is reported as RG_FLAC_ERR_UNSUPPORTED (the file route hands it to the decoder command).
 *
 * Frames.  The stream is walked by a byte-aligned forward scan (rg_flac_index_frames): a frame header is accepted when its
 * sync code, reserved bits, fields, CRC-8 and frame / sample number all hold (the number continues the previous accepted
 * frame's: strictly after it, at most 64 frames -- or 64 x 65536 samples -- later).  A frame reaches to the next accepted
 * header or to the end of the data (the last frame ends at the last point its CRC-16 holds, so a trailing tag is not part
 * of it).  A frame whose CRC-16 does not match, that does not parse, or whose samples do not fit their width is dropped and
 * contributes no samples: the rule the MPEG decoder follows (DecodeError -> continue, src/replaygain.rs:896-899).  The
 * reference decodes FLAC with symphonia, whose source is not in the reference tree; its handling of damaged FLAC could not
 * be compared, and this rule is the project's own.
 *
 * What is hashed (rg_flac_verify, rg_flac_md5_s32, rg_flac_md5_arena).  STREAMINFO carries the MD5 signature of the
 * unencoded audio: RFC 1321 MD5, with its padding and 64-bit bit length, over the frames in order and within a frame the
 * channels in order, each sample a signed two's-complement integer of B = (bps + 7) / 8 bytes, little-endian, sign-extended
 * from bps bits (B is 1, 2 or 3 for the 4-24 bits this decoder takes).  A stream of `frames` frames hashes
 * frames * channels * B bytes; zero frames give the MD5 of the empty message; a STREAMINFO field of sixteen zero bytes means
 * "no signature".  In the analysis arena a FLAC sample lies left-justified in its element (16-bit planes for bps <= 16,
 * << 16 - bps; 32-bit planes above, << 32 - bps; rg_flac_stage_device_batch); the sample value is the element shifted back
 * arithmetically.
 *
 * Host code (apart from rg_flac_decode_device, rg_flac_stage_device_batch, route 1 of rg_flac_md5_arena and rg_flac_verify),
 * plain C types, no exceptions or aborts across the ABI.
 */
#ifndef MP3RGAIN_AMD_FLAC_H
#define MP3RGAIN_AMD_FLAC_H

#include <stddef.h>
#include <stdint.h>

#include "mp3rgain_amd.h" /* rg_track_desc (rg_flac_stage_device_batch) */

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rg_flac_status {
    RG_FLAC_OK = 0,
    RG_FLAC_ERR_ARG = -1,
    RG_FLAC_ERR_NOT_FLAC = -2,    /* no "fLaC" marker or no valid STREAMINFO                                   */
    RG_FLAC_ERR_CAPACITY = -3,    /* output too small (what is needed is in the info)                          */
    RG_FLAC_ERR_UNSUPPORTED = -4  /* a FLAC stream this decoder does not take (25-32 bits per sample)          */
} rg_flac_status;

typedef struct rg_flac_info {
    uint32_t sample_rate;      /* STREAMINFO                                                                   */
    uint32_t channels;
    uint32_t bits_per_sample;
    uint32_t min_block_size;
    uint32_t max_block_size;
    uint32_t id3v2_bytes;      /* tag skipped in front of "fLaC"                                               */
    uint64_t total_samples;    /* STREAMINFO, per channel; 0 = unknown                                         */
    uint64_t metadata_bytes;   /* offset of the first byte after the metadata blocks (ID3v2 tag included)      */
    uint64_t frames;           /* PCM frames per channel: index = if every frame decodes, decode = produced     */
    uint32_t audio_frames;     /* FLAC frames: indexed / decoded                                               */
    uint32_t dropped_frames;   /* indexed frames that did not decode (CRC-16, parse, range)                    */
} rg_flac_info;

typedef struct rg_flac_frame {
    uint64_t offset;           /* byte offset of the frame header in the data                                 */
    uint64_t first_sample;     /* from the header: frame number x max block size, or the sample number         */
    uint32_t length;           /* bytes, CRC-16 included                                                       */
    uint32_t block_size;
    uint8_t channel_assignment;/* 0-7: channels - 1 independent; 8 left/side, 9 right/side, 10 mid/side        */
    uint8_t header_length;     /* bytes of the frame header, CRC-8 included                                    */
    uint16_t reserved;
    uint32_t reserved2;
} rg_flac_frame;               /* 32 bytes */

/* 1 if `data` is a native FLAC stream (after an optional ID3v2 tag). */
int rg_flac_is_flac(const void *data, size_t len);

/* Metadata only: STREAMINFO, the ID3v2 and metadata sizes (frames / audio_frames / dropped_frames are 0). */
int rg_flac_scan(const void *data, size_t len, rg_flac_info *out);

/* The frame walk.  Writes up to `capacity` entries; *n_frames = frames found (RG_FLAC_ERR_CAPACITY if more than
 * `capacity`).  out->frames = the sum of their block sizes. */
int rg_flac_index_frames(const void *data, size_t len, rg_flac_frame *frames, size_t capacity, size_t *n_frames, rg_flac_info *out);

/* Decode a whole stream into `channels` planes of `capacity` int32 samples each, right-justified.  On RG_FLAC_OK
 * out->frames is the number of samples written per channel and out->dropped_frames the frames dropped. */
int rg_flac_decode_s32(const void *data, size_t len, int32_t *const *planes, uint64_t capacity, rg_flac_info *out);

/* The index and the decoder agree on the frame count and the PCM length: 0 = yes, 1 = no, < 0 = not decodable. */
int rg_flac_index_selfcheck(const void *data, size_t len);

/* Text of the calling thread's last error ("" if none). */
const char *rg_flac_last_error(void);

/* Test seam of the device decoder: the stream through the file route's device kernels (frame check, layout, decode),
 * PCM back to `planes` as rg_flac_decode_s32 returns it (bit for bit, tests/test_gpu_flac.py).  `ctx` is an rg_ctx. */
int rg_flac_decode_device(void *ctx, const void *data, size_t len, int32_t *const *planes, uint64_t capacity, rg_flac_info *out);

/* Test seam of the file route's FLAC staging: `n` streams in memory are loaded (the frame walk; with tuning key 14 = 0 the
 * host decoder and its repacking) and staged by the very code a file call runs -- one launch of the device decoder for
 * all of them, each stream at its own 16-byte-aligned arena offset, <= 16 bits per sample in 16-bit planes (<< 16 - bps),
 * 17-24 bits in 32-bit planes (<< 32 - bps), plane c of stream i at offset_bytes + c * frames * element size -- and the
 * first *arena_bytes bytes of the analysis arena are copied to `arena_out` (tests/test_gpu_flac_batch.py).
 * descs[i]: what the analysis kernels would be given for stream i (offset, decoded PCM frames, rate, channels, format).
 * infos[i]: STREAMINFO, and frames = decoded PCM frames per channel, audio_frames = FLAC frames decoded, dropped_frames
 * = FLAC frames dropped (walked = audio_frames + dropped_frames).  RG_ERR_INVALID_ARG with *arena_bytes set when
 * `arena_capacity` is too small.  `ctx` is an rg_ctx. */
int rg_flac_stage_device_batch(void *ctx, size_t n, const void *const *data, const size_t *len, rg_track_desc *descs,
                               rg_flac_info *infos, void *arena_out, size_t arena_capacity, size_t *arena_bytes);

/* Test seam, host code: the CPU twin of the device decoder's output stage.  Decodes the stream as rg_flac_decode_s32
 * does, but writes -- and, for the stereo decorrelations, reads back -- every sample through the arena sink of the device
 * kernel (rg_flac_frame.h: RgFlacArenaOut) into `out`, in the arena's format: planes of *elem_bytes-byte elements (2 for
 * <= 16 bits per sample, else 4), plane c at out + c * info->frames * *elem_bytes.  RG_FLAC_ERR_CAPACITY (info->frames
 * set) when capacity_bytes < channels * frames * elem_bytes; RG_FLAC_ERR_ARG if a frame's verdict through this sink
 * differs from the host decoder's (it must not). */
int rg_flac_decode_arena(const void *data, size_t len, void *out, size_t capacity_bytes, uint32_t *elem_bytes, rg_flac_info *info);

/* STREAMINFO's MD5 signature into out[16] (behind an ID3v2 tag as rg_flac_scan skips it): 1 = a signature is set, 0 = the
 * field is all zero (no signature), < 0 = an rg_flac_status (not a FLAC stream). */
int rg_flac_stream_md5(const void *data, size_t len, uint8_t out[16]);

/* The signature of right-justified planes as rg_flac_decode_s32 returns them ("What is hashed" above): RG_FLAC_OK, or
 * RG_FLAC_ERR_ARG (1-8 channels, 4-24 bits per sample). */
int rg_flac_md5_s32(const int32_t *const *planes, uint32_t channels, uint64_t frames, uint32_t bps, uint8_t out[16]);

/* Test seam of the hash: the `n` streams that descs[i] (format S16 or S32 planar, the arena's left-justified form: the
 * sample is the element >> (8 * element size - bps[i])) describe in the host arena `arena`, each hashed into
 * digests[16 * i ..].  route 0: the host twin reads that form where it lies (`ctx` may be NULL); route 1: the arena is
 * copied to the device and the kernel of the file route hashes it, one lane per stream (`ctx` is an rg_ctx).  A stream
 * needs only sample alignment; RG_ERR_INVALID_ARG for one whose planes are not wholly inside the arena. */
int rg_flac_md5_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena,
                      size_t arena_bytes, uint8_t *digests /* [n][16] */);

/* Measurement hook (tools/flac_md5_rate.py): `n` streams of `frames` frames of `channels` channels of 16-bit PCM, filled on
 * the device, each at its own offset of one device arena.  After a warm-up, `reps` rounds of: the kernel over all n streams
 * (dev_ms[r], HIP events around the launch), then the host twin over a host copy of the first `host_streams` (<= n) streams
 * on `threads` host threads (host_ms[r]).  *mismatches: host digests that differ from the kernel's (it must be 0).  `ctx` is
 * an rg_ctx. */
int rg_flac_md5_rate(void *ctx, size_t n, uint64_t frames, uint32_t channels, size_t host_streams, uint32_t threads, uint32_t reps,
                     double *dev_ms, double *host_ms, size_t *mismatches);

/* rg_flac_verify: what `flac -t` gives.  The files are decoded by the very route the analysis uses -- the same loaders, the
 * same groups (tuning key 13) for lists larger than the device, the device decoder (tuning key 14 = 1) or the host decoder
 * (key 14 = 0) -- and the decoded PCM is hashed where it lies: in the analysis arena by a device kernel, one lane per
 * stream, only the digests coming back (key 14 = 1), or on the host (key 14 = 0).  Both give the same bytes in `out`. */
#define RG_FLAC_VERIFY_HAS_SIGNATURE 1u  /* STREAMINFO's MD5 is not all zero                          */
#define RG_FLAC_VERIFY_MD5_MATCH     2u  /* set only with HAS_SIGNATURE: md5_decoded == md5_stream    */
#define RG_FLAC_VERIFY_LENGTH_MATCH  4u  /* total_samples == 0 (unknown) or == frames                 */
#define RG_FLAC_VERIFY_COMPLETE      8u  /* dropped_frames == 0                                       */
typedef struct rg_flac_verify_result {
    int32_t status;          /* RG_OK, or why there is no decode (text: rg_tracks_error(ctx, i))      */
    uint32_t flags;
    uint64_t frames;         /* PCM frames per channel that were decoded and hashed                   */
    uint64_t total_samples;  /* STREAMINFO                                                            */
    uint32_t audio_frames, dropped_frames;
    uint8_t md5_stream[16], md5_decoded[16];
} rg_flac_verify_result;     /* 64 bytes */
/* A failing file fails alone: RG_ERR_IO (it cannot be opened), RG_ERR_FORMAT (not a native FLAC stream, or one of 25-32
 * bits per sample; no decoder command is run), its record otherwise zero.  RG_OK whenever the call itself worked. */
int rg_flac_verify(rg_ctx *ctx, const char *const *paths, size_t n, rg_flac_verify_result *out);

#ifdef __cplusplus
}
#endif
#endif /* MP3RGAIN_AMD_FLAC_H */
