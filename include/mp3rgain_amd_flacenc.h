/* mp3rgain_amd_flacenc.h -- C ABI of the FLAC encoder: planar integer PCM where the loaders leave it in the analysis arena
 * -> native FLAC streams, analysed and written by device kernels (mp3rgain_amd/csrc/rg_flacenc.hip) or by their serial twin
 * on the host (rg_flacenc_host.cpp).  Both run one header (rg_flacenc.h) and give the same bytes.
 *
 * Streams.  Native FLAC, fixed blocking strategy.  The block size comes from the options: 256, 512, 1024, 2048 or 4096
 * (default 4096); the last block is whatever remains, down to one sample.  1 to 8 channels, 4 to 24 bits per sample.  The
 * frame header codes the rate from its table, else in kHz, Hz or tens of Hz, else "from STREAMINFO"; the sample size from its
 * table (8, 12, 16, 20, 24), else "from STREAMINFO".  A track of zero frames gives a valid stream with no audio frames.  The
 * metadata is STREAMINFO (block sizes, frame sizes, rate, channels, bits, total samples, MD5 of the audio as
 * mp3rgain_amd_flac.h defines "What is hashed") and one VORBIS_COMMENT block with the vendor string and no comments.  No
 * SEEKTABLE and no PADDING is written.
 *
 * Signals per frame.  The channels; for two-channel frames also mid = (L + R) >> 1 and side = L - R (bps + 1 bits).  Wasted
 * bits (zero low bits common to every sample of the signal in the block) are detected per signal and removed.
 *
 * Candidates per signal, in this order: CONSTANT (only when every sample is equal), VERBATIM, FIXED orders 0 to 4, LPC at
 * every even order from 2 to max_lpc_order (default 8, at most 12, 0 = none).  Orders not below the block length are left
 * out.  The candidate with the fewest bits wins, the earlier one on a tie.  A predictor whose residual does not fit 32 bits
 * (|r| < 2^31) is not a candidate.  VERBATIM always is, so a frame is never larger than its plain coding.  For two channels
 * the cheapest of L/R, L/S, R/S and M/S is taken, in this order on a tie.
 *
 * LPC.  The block is weighted with an integer Welch window, w(i) = floor(32767 (N^2 - d^2) / N^2) with N = n - 1 and
 * d = 2 i - N, the product shifted right by 15.  The autocorrelation at lags 0 to max_lpc_order is exact in 64-bit integers
 * (4096 values of 25 bits fit).  Levinson-Durbin runs in double on one lane in a fixed order of operations; both sides are
 * built with -ffp-contract=off and call no libm function.  Coefficients have 12 bits for widths <= 16 and 15 bits above
 * (the width of a signal: its bits after the wasted bits are removed, the side signal counted as its channels are); the
 * shift (0 to 15; a negative one drops the order) comes from the exponent bits of the largest coefficient; rounding carries
 * the error forward.  If the recursion's error stops being positive the higher orders are left out.
 *
 * Residual coding, sized exactly.  u is the zig-zag value of a residual.  A partition of n residuals costs
 * n (k + 1) + sum(u >> k) bits under parameter k.  These sums are taken for every k per piece of 64 samples and added up to
 * the partitions of orders 0 to 6: an order p is considered when the partition length n >> p is a whole number of pieces
 * (order 0 always is considered), so a short last block of a length that is no multiple of 64 has one partition.  The
 * parameter is minimised per partition (the smallest k on a tie), then the order (the smallest on a tie), with the 4 or 5
 * parameter bits of every partition counted.  The Rice method with k <= 14 codes signals of width <= 16, Rice2 with k <= 30
 * the others, so 16-bit audio padded to 24 bits costs what the 16-bit audio costs plus its wasted-bits fields.  No escape
 * partitions.
 *
 * Files (rg_flac_encode_files).  The sources are loaded and staged by the route the analysis uses (the same loaders, the
 * same groups, tuning key 13, for lists larger than the device) and encoded where their PCM lies.  Sources are WAV with 8,
 * 16 or 24-bit integer samples and FLAC; float or 32-bit WAV and MPEG sources fail alone with RG_ERR_FORMAT: a lossless
 * container round lossy or float audio is not what this call is for.  A FLAC source keeps its own VORBIS_COMMENT block in
 * place of the vendor block, and every other metadata block of it is copied through unchanged and in order, except
 * STREAMINFO, SEEKTABLE and PADDING.  A source with dropped frames is encoded from what decoded; its record says how many
 * frames were dropped and lacks RG_FLAC_ENC_COMPLETE.  An output path that exists, or that names its input, fails alone
 * with RG_ERR_IO and nothing is written.  An output is written to "<path>.part" beside it and linked to its name when
 * complete, so an existing file is never replaced.
 *
 * Verified write (RG_FLAC_ENC_VERIFY, on by default).  Before a file is written its encoded bytes go through the device
 * decoder of the tree (frame check, layout and decode kernels) into a device buffer of the arena's format, the MD5 kernel
 * hashes that decode there, and the digest and the length must equal those of the source planes.  A mismatch fails the file
 * with RG_ERR_STATE, writes nothing and sets RG_FLAC_ENC_VERIFY_FAILED: it must never happen.
 *
 * Host code apart from route 1 of rg_flac_encode_arena and rg_flac_encode_files; plain C types, no exceptions or aborts
 * across the ABI.
 */
#ifndef MP3RGAIN_AMD_FLACENC_H
#define MP3RGAIN_AMD_FLACENC_H

#include <stddef.h>
#include <stdint.h>

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_FLAC_ENC_DEFAULT_BLOCK 4096u
#define RG_FLAC_ENC_DEFAULT_LPC 8u
#define RG_FLAC_ENC_MAX_LPC 12u

typedef struct rg_flac_encode_options {
    uint32_t struct_size;    /* sizeof(rg_flac_encode_options)                                              */
    uint32_t block_size;     /* 0 = RG_FLAC_ENC_DEFAULT_BLOCK; else 256, 512, 1024, 2048 or 4096            */
    uint32_t max_lpc_order;  /* 0 .. RG_FLAC_ENC_MAX_LPC; odd values count as the even one below             */
    uint32_t flags;          /* RG_FLAC_ENC_VERIFY (the seam ignores it) or 0                               */
} rg_flac_encode_options;    /* NULL = block 4096, max_lpc_order 8, RG_FLAC_ENC_VERIFY                      */
#define RG_FLAC_ENC_VERIFY 1u

#define RG_FLAC_ENC_COMPLETE 1u       /* the stream holds every frame of its source: none was dropped by the decode */
#define RG_FLAC_ENC_VERIFIED 2u       /* the stream was decoded on the device and its MD5 and length matched         */
#define RG_FLAC_ENC_WRITTEN 4u        /* the output file exists under its name                                       */
#define RG_FLAC_ENC_VERIFY_FAILED 8u  /* the decode of the stream differed from its source (it must not)             */
typedef struct rg_flac_encode_result {
    int32_t status;          /* RG_OK                                                                       */
    uint32_t flags;
    uint64_t pcm_frames;     /* per channel                                                                 */
    uint32_t flac_frames;
    uint32_t dropped_frames; /* FLAC frames of the source that did not decode (the seam has none: 0)        */
    uint32_t sample_rate, channels, bits_per_sample, block_size;
    uint32_t min_frame_bytes, max_frame_bytes; /* 0 when there is no frame                                  */
    uint64_t pcm_bytes;      /* pcm_frames * channels * ((bps + 7) / 8): what the MD5 covers                */
    uint64_t stream_bytes;   /* metadata and frames                                                         */
    uint64_t metadata_bytes;
    uint8_t md5_pcm[16];     /* of the source planes; STREAMINFO carries it                                 */
    uint8_t md5_decoded[16]; /* of the verified write's decode; zero without one (the seam has none)        */
} rg_flac_encode_result;     /* 104 bytes */

/* The encoder's seam: the `n` tracks that descs[i] (format S16 or S32 planar, the arena's left-justified form: the sample is
 * the element >> (8 * element size - bps[i]); 1-8 channels; sample-aligned, wholly inside the arena) describe in the host
 * arena `arena` are encoded, stream i into out[offsets[i] .. offsets[i + 1]).  route 0: the serial twin (`ctx` may be NULL);
 * route 1: the arena is copied to the device and the kernels analyse, lay out and write every frame of every stream in one
 * launch each (`ctx` is an rg_ctx), the MD5 kernel of the file route hashes the planes.  There is no route 2: the kernels
 * order nothing differently from the twin.  offsets[0 .. n] is always set; when out_capacity < offsets[n] nothing is written
 * and the call returns RG_ERR_INVALID_ARG (the text names the size needed).  Text: rg_last_error(ctx). */
int rg_flac_encode_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena,
                         size_t arena_bytes, const rg_flac_encode_options *options, void *out, size_t out_capacity,
                         uint64_t *offsets /* n + 1 */, rg_flac_encode_result *results);

/* `n` files: in_paths[i] encoded into out_paths[i].  A failing file fails alone (status and rg_tracks_error(ctx, i)), its
 * record otherwise zero apart from the flags; RG_OK whenever the call itself worked.  `ctx` is an rg_ctx. */
int rg_flac_encode_files(rg_ctx *ctx, const char *const *in_paths, const char *const *out_paths, size_t n, const rg_flac_encode_options *options,
                         rg_flac_encode_result *results);

/* Host helper (what rg_flac_encode_files does with a FLAC source's metadata): the metadata blocks that follow STREAMINFO in
 * the output for the FLAC stream `file`, as they go into it -- the source's own blocks, unchanged and in order, without
 * STREAMINFO, SEEKTABLE and PADDING; when it has no VORBIS_COMMENT block, the vendor block first; the last-block flag set on
 * the final one.  *need = their length; they are copied to out[capacity] when they fit.  RG_OK, RG_ERR_INVALID_ARG (null,
 * capacity < *need) or RG_ERR_FORMAT (not a FLAC stream whose metadata can be walked). */
int rg_flac_encode_source_blocks(const void *file, size_t len, void *out, size_t capacity, size_t *need);

/* Measurement hook (tools/flacenc_rate.py): route 1 of the seam, timed per kernel with HIP events after a warm-up: ms[0]
 * analyse, ms[1] layout, ms[2] write, ms[3] MD5, ms[4] a read-only pass over the arena's bytes, each the median of `reps`
 * rounds.  *stream_bytes: what the streams take. */
int rg_flac_encode_rate(void *ctx, size_t n, const rg_track_desc *descs, const uint32_t *bps, const void *arena, size_t arena_bytes,
                        const rg_flac_encode_options *options, uint32_t reps, double *ms /* 5 */, uint64_t *stream_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MP3RGAIN_AMD_FLACENC_H */
