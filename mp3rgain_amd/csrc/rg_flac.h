// rg_flac.h -- the library-internal side of the FLAC decoder: the frame index as a vector (rg_flacdec.cpp) and the
// device decode chain (rg_flacdev.hip) the file route calls.
#ifndef RG_FLAC_H
#define RG_FLAC_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mp3rgain_amd_flac.h"

// rg_flac_index_frames into a vector
int rg_flac_index_vec(const uint8_t *d, size_t len, std::vector<rg_flac_frame> *frames, rg_flac_info *out);
// decode along an index; planes may be null (count only); good[k] = 1 for frames that decoded
int rg_flac_decode_vec(const uint8_t *d, size_t len, const std::vector<rg_flac_frame> &frames, const rg_flac_info &si,
                       int32_t *const *planes, uint64_t capacity, rg_flac_info *out, std::vector<uint8_t> *good);

namespace rgf {
// The arena format of FLAC PCM, the WAV route's convention: up to 16 bits S16 planar (<< 16 - bps), 17-24 bits S32 planar
// (<< 32 - bps).  Both are exact powers of two, so the analysis sees the same normalised samples either way.
inline uint32_t flac_elem_bytes(uint32_t bps) { return bps <= 16 ? 2u : 4u; }
inline uint32_t flac_shift(uint32_t bps) { return bps <= 16 ? 16u - bps : 32u - bps; }
}  // namespace rgf

#ifdef __HIP__
#include <hip/hip_runtime.h>

struct rg_ctx;

// One stream of a device decode: its bytes in the staging buffer and where its PCM goes.
struct RgFlacDevStream {
    const uint8_t *bytes;                   // host: the stream (offsets in its frames are relative to it)
    size_t len;
    const rg_flac_frame *frames;            // host: its index
    uint32_t n_frames;
    uint32_t channels, bps;
    uint32_t elem_bytes;                    // 2: S16 planar, 4: S32 planar
    uint32_t shift;                         // left shift into the element (16 - bps, 32 - bps, or 0 for right-justified)
    unsigned char *dst;                     // device: plane 0; plane c at dst + c * (samples decoded) * elem_bytes
    // results
    uint64_t samples;                       // per channel, decoded
    uint32_t decoded_frames, dropped_frames;
};

// Copy the streams to the device, check, lay out and decode them on `s`; on return the results are filled in and the
// PCM is in place (the stream has been synchronised).
int rg_flacdev_decode(rg_ctx *c, RgFlacDevStream *streams, size_t n, hipStream_t s);
#endif

#endif  // RG_FLAC_H
