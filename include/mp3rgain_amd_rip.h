/* mp3rgain_amd_rip.h -- rip checksums on the GPU: per track the CRC-32 of the PCM (EAC's "Copy CRC"), the same CRC with
 * null samples left out, and the AccurateRip v1 / v2 signatures, computed from the 16-bit planes the file route has put into
 * the analysis arena -- one decode, on the device, and only a 48-byte record per track comes back.
 *
 * rg_flac_verify and rg_mp3_verify answer "does this file still decode to what its encoder saw".  These numbers answer "is
 * this the audio the ripper read from the disc": a ripper's log (EAC, XLD, whipper, CUETools) holds them per track.
 *
 * DEFINITIONS (the contract).  They are, as far as the authors know, the definitions the rippers use; THIS WAS NOT CHECKED
 * AGAINST A RIPPER, an AccurateRip database or a real rip log.  The tests hold the code to an independent restatement of
 * the text below (zlib's crc32 and plain sums).
 *
 * A track takes part when it has exactly 2 channels of exactly 16-bit samples and fewer than 2^32 frames: a 16-bit
 * RIFF/WAVE file, or a FLAC stream with bits_per_sample == 16.  Both lie in the arena as RG_FMT_S16_PLANAR, unshifted.
 * Everything else fails alone with RG_ERR_FORMAT and a text saying why: mono, other widths, float WAV, MPEG streams, more
 * than 2 channels.  The sample rate is reported and not required.
 *
 * Let the track have N frames (L_k, R_k), k = 0..N-1, int16.
 *   crc32          CRC-32 as zlib computes it (reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF) over
 *                  the 4N bytes L_k low, L_k high, R_k low, R_k high, in frame order.  N = 0 gives 0.
 *   crc32_nonnull  the same CRC over the bytes of the 16-bit samples that are not 0, in the same order.  Each sample is
 *                  taken or skipped on its own, so L_k may be skipped while R_k is kept.  A track with no non-zero sample
 *                  gives 0.
 *   null_samples   the number of 16-bit samples that are 0.  The message of crc32_nonnull is 2 * (2N - null_samples) bytes.
 *   AccurateRip    v_k = (uint16)L_k | (uint16)R_k << 16, and i = k + 1.  Position i counts when from <= i <= to.  `from`
 *                  is 2940 when the track is flagged first of its disc, otherwise 0.  `to` is N - 2940 when the track is
 *                  flagged last of its disc, otherwise N; it is computed signed: the range may be empty, and then both sums
 *                  are 0.  With p = (uint64)v_k * i:
 *                      arv1 = sum of lo32(p)            mod 2^32
 *                      arv2 = sum of lo32(p) + hi32(p)  mod 2^32
 *                  So a first track leaves out its first 2939 frames, and a last track leaves out its last 2940.
 *
 * DRIVE OFFSETS (rg_rip_offset_signatures).  A different pressing, or a drive whose read offset was not corrected, shifts the
 * audio of a rip by a few samples; then every AccurateRip signature differs although the audio is the same.  So the signatures
 * are also computed at every sample offset of a window.  The `n` tracks of a call are one disc, in call order.  Track t has
 * N_t frames, and B_t = sum of N_u over u < t.  Disc positions are 64-bit.  W[j] = (uint16)L | (uint16)R << 16 of disc frame
 * j for 0 <= j < sum N, and 0 for every other j.  from_t and to_t are exactly those above, from the track's flags.  For every
 * offset o with -radius <= o <= radius, where 0 <= radius <= 2939 (RG_RIP_OFFSET_MAX), let
 * p = (uint64)W[B_t + i - 1 + o] * i.  Then
 *                      arv1_t(o) = sum over the i that count of lo32(p)            mod 2^32
 *                      arv2_t(o) = sum over the i that count of lo32(p) + hi32(p)  mod 2^32
 * A positive o takes the samples that lie later on the disc.  At o = 0 both are arv1 / arv2 above, bit for bit.  A first and
 * a last track that are flagged never read outside the disc -- that is what the 2940 is for; unflagged tracks at the disc's
 * edges read zeros outside it.  THE SIGN CONVENTION AND THE +-2939 WINDOW WERE NOT CHECKED AGAINST A RIPPER either.
 *
 * Not here: disc IDs and database lookups, CUETools DB parity, other widths or channel counts,
 * checksums of MPEG-decoded audio, cue sheets.  Nothing is written to files.
 */
#ifndef MP3RGAIN_AMD_RIP_H
#define MP3RGAIN_AMD_RIP_H

#include "mp3rgain_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RG_RIP_FIRST_TRACK 1u /* input flag, per file: the first track of its disc */
#define RG_RIP_LAST_TRACK  2u /* input flag, per file: the last track of its disc  */
#define RG_RIP_CD_RATE     1u /* result flag: 44100 Hz            */
#define RG_RIP_CD_FRAMES   2u /* result flag: frames % 588 == 0   */
#define RG_RIP_COMPLETE    4u /* result flag: dropped_frames == 0 */
#define RG_RIP_AR_SKIP 2940u  /* 5 CD sectors of 588 frames */
#define RG_RIP_OFFSET_MAX 2939        /* the largest radius of the offset window */
#define RG_RIP_DISC_MAX_TRACKS 1024u  /* tracks of one disc: bounds the device's signature tables at about 48 MB */

typedef struct rg_rip_result {
    int32_t status;          /* RG_OK, or why there are no checksums (text: rg_tracks_error(ctx, i)) */
    uint32_t flags;
    uint64_t frames;         /* N: PCM frames per channel that were hashed                            */
    uint64_t null_samples;
    uint32_t sample_rate;
    uint32_t dropped_frames; /* FLAC frames the decode route dropped (0 for a WAV file)               */
    uint32_t crc32, crc32_nonnull, arv1, arv2;
} rg_rip_result;             /* 48 bytes */

/* The files are decoded by the very route the analysis uses -- the same loaders, the same groups (tuning key 13) for lists
 * larger than the device, the device FLAC decoder (tuning key 14 = 1) or the host decoder (key 14 = 0); no decoder command
 * is run -- and the checksums are computed where the PCM lies, in the analysis arena, by two kernels on the stream the
 * decode ran on.  track_flags[i]: RG_RIP_FIRST_TRACK / RG_RIP_LAST_TRACK of file i; NULL = all 0.  A failing file fails
 * alone: RG_ERR_IO (it cannot be opened), RG_ERR_FORMAT (not 2 channels of 16-bit PCM in a WAV or native FLAC stream), its
 * record zero apart from `status`.  A FLAC file with dropped frames gets the checksums of what the route decoded, with
 * dropped_frames set and RG_RIP_COMPLETE clear.  RG_OK whenever the call itself worked.  `out` is byte for byte the same
 * for tuning key 14 = 1 and 14 = 0. */
int rg_rip_checksums(rg_ctx *ctx, const char *const *paths, size_t n, const uint32_t *track_flags, rg_rip_result *out);

/* Test seam: the `n` tracks that descs[i] (RG_FMT_S16_PLANAR, 2 channels, fewer than 2^32 frames: anything else is
 * RG_ERR_FORMAT) describe in the host arena `arena`.  out[i].dropped_frames is 0 and RG_RIP_COMPLETE set.
 *   route 0  the serial host twin: the definitions above, written as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the file route's kernels (`ctx` is an rg_ctx)
 *   route 2  the kernels' fold arithmetic run on the host -- chunks, trees, powers, the final fix-up; `ctx` may be NULL
 * A track needs only sample alignment; RG_ERR_INVALID_ARG for one whose planes are not wholly inside the arena.  With a
 * NULL ctx the error text is rg_last_error(NULL)'s. */
int rg_rip_checksums_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, const void *arena,
                           size_t arena_bytes, rg_rip_result *out);

/* Test seam: how the kernels cut a track.  chunk_frames: frames one lane hashes; tile_frames: frames of one block of the
 * tile kernel (chunks and tiles are counted from the track's END, so only the first of each is short); fold_lanes: lanes of
 * the fold kernel, each folding a run of ceil(tiles / fold_lanes) tile records.  Any pointer may be NULL. */
int rg_rip_kernel_shape(uint32_t *chunk_frames, uint32_t *tile_frames, uint32_t *fold_lanes);

/* Test seam of rg_crc32.h: *product = a * b mod P on reflected residues, *power = x^(8 n) mod P.  Either may be NULL. */
int rg_rip_crc32_algebra(uint32_t a, uint32_t b, uint64_t n, uint32_t *product, uint32_t *power);

/* Measurement hook (tools/rip_crc_rate.py): `n` tracks of `frames` frames of 16-bit stereo PCM, filled on the device, each
 * at its own offset of one device arena.  After a warm-up of `warm_ms` milliseconds of launches, `reps` rounds of: the two
 * kernels over all n tracks (dev_ms[r], HIP events around the two launches) with the plain CRC's look-ups taken from
 * `table_layout` (0 = one byte table, 1 = slice-by-4), then the serial host twin over a host copy of the first
 * `host_tracks` (<= n) tracks on `threads` host threads (host_ms[r]).  *mismatches: host records that differ from the
 * kernels' (it must be 0).  `ctx` is an rg_ctx. */
int rg_rip_rate(void *ctx, size_t n, uint64_t frames, int table_layout, size_t host_tracks, uint32_t threads, uint32_t reps, double warm_ms,
                double *dev_ms, double *host_ms, size_t *mismatches);

/* The AccurateRip signatures of a disc at every offset of -radius .. radius (DRIVE OFFSETS above).  The route is
 * rg_rip_checksums': same loaders, both FLAC decoders (tuning key 14), WAV, no decoder command; out[i] is byte for byte what
 * rg_rip_checksums gives for the same files and flags.  arv1 / arv2: n x (2 radius + 1) values, row-major, [t][o + radius];
 * either may be NULL.  The tables are computed only when every file took part (status == RG_OK for all of them): a hole in
 * the disc would silently shift every later track.  Otherwise the call returns RG_ERR_REFUSED, the text (rg_last_error) names
 * the first file that failed, out[] is still filled and the tables are zero.  A FLAC file with dropped frames takes part with
 * what was decoded; out[i] says so.  A disc must lie in the arena at once: a list the route would cut into groups (tuning key
 * 13, or the device's size) is RG_ERR_REFUSED before anything is loaded, out[] and the tables zero.  RG_ERR_INVALID_ARG for a
 * radius outside 0 .. RG_RIP_OFFSET_MAX or n > RG_RIP_DISC_MAX_TRACKS.  The tables are byte for byte the same for tuning key
 * 14 = 1 and 14 = 0. */
int rg_rip_offset_signatures(rg_ctx *ctx, const char *const *paths, size_t n, const uint32_t *track_flags, int32_t radius, rg_rip_result *out,
                             uint32_t *arv1, uint32_t *arv2);

/* Test seam: the disc that descs[0 .. n) describe in the host arena `arena`, as rg_rip_checksums_arena takes them (the same
 * argument errors; in addition RG_ERR_INVALID_ARG for a radius outside 0 .. RG_RIP_OFFSET_MAX and n > RG_RIP_DISC_MAX_TRACKS;
 * n = 0 is RG_OK).  Tracks lie anywhere in the arena, in any order, and may alias.  Tables as above; either may be NULL.
 *   route 0  the definition, serially and as plainly as possible; `ctx` may be NULL
 *   route 1  the arena copied to the device, and the kernel of rg_rip_offsets.hip (`ctx` is an rg_ctx)
 *   route 2  arv1 only (arv2 must be NULL, else RG_ERR_INVALID_ARG), by the sliding recurrence on the host; `ctx` may be
 *            NULL.  With f = max(from, 1), T = to, c = B - 1:  A(o + 1) = A(o) - f W[c + f + o] + (T + 1) W[c + T + 1 + o] - S(o),
 *            where S(o) = sum of W[c + i + o] over i = f + 1 .. T + 1 slides as well.  An independent check on signs and edges. */
int rg_rip_offsets_arena(void *ctx, int route, size_t n, const rg_track_desc *descs, const uint32_t *track_flags, int32_t radius,
                         const void *arena, size_t arena_bytes, uint32_t *arv1, uint32_t *arv2);

/* Test seam: how the offsets kernel cuts a disc.  tile_frames: frames of a track one block takes (tiles are counted from
 * the track's first frame); block_lanes: its lanes.  Either may be NULL. */
int rg_rip_offsets_kernel_shape(uint32_t *tile_frames, uint32_t *block_lanes);

/* Measurement hook (tools/rip_offsets_rate.py): a disc of `n` tracks of `frames` frames of 16-bit stereo PCM, filled on the
 * device, the first track flagged first and the last last.  After a warm-up of `warm_ms` milliseconds of launches, `reps`
 * rounds of the tables' zeroing and the kernel at `radius` (dev_ms[r], HIP events around them), a lane holding `lane_offsets`
 * consecutive offsets in registers: 23, the product's kernel, or 1, the plain form it is measured against.  Then the
 * definition (route 0's arithmetic) for all n tracks at `host_offsets` offsets spread evenly over the window, -radius and
 * +radius among them, on `threads` host threads over a host copy of the disc: *host_ms, the wall time of that;
 * *host_products, the products it took (the disc's are *disc_products, which may be NULL).  *mismatches: (track, offset)
 * pairs whose host values differ from the kernel's (it must be 0).  host_offsets = 0 runs no host pass.  `ctx` is an rg_ctx. */
int rg_rip_offsets_rate(void *ctx, size_t n, uint64_t frames, int32_t radius, uint32_t lane_offsets, uint32_t host_offsets, uint32_t threads, uint32_t reps,
                        double warm_ms, double *dev_ms, double *host_ms, uint64_t *host_products, uint64_t *disc_products, size_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif
