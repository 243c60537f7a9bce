// Stand-alone driver of tests/test_flacenc_sanitizers.py: the FLAC encoder's serial twin (rg_flacenc_host.cpp with rg_flacenc.h,
// the header the kernels share) and the host decoder (rg_flacdec.cpp) on tracks read from files, each in an exact-size heap
// arena at an offset that is only sample-aligned and encoded into an exact-size heap buffer, so a read past a plane, a store
// past the stream, a signed overflow or a misaligned access aborts the driver.  A file is [u64 frames][u32 channels][u32
// format][u32 sample rate][u32 bits per sample][u32 block][u32 max_lpc_order][planes], little-endian; a line per file goes
// to stdout: the stream's length, whether the decoder returned the planes' samples, and the stream in hexadecimal.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/mp3rgain_amd_flac.h"
#include "../../mp3rgain_amd/csrc/rg_flacenc.h"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t head[6];
        if (fread(&frames, 8, 1, f) != 1 || fread(head, 4, 6, f) != 6) return 2;
        const uint32_t channels = head[0], format = head[1], elem = format == RG_FMT_S16_PLANAR ? 2 : 4, bps = head[3];
        const size_t off = elem * (size_t)(a % 5), pcm = (size_t)frames * channels * elem, bytes = off + pcm;
        std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: the planes end at the block's end
        if (pcm && fread(arena->data() + off, 1, pcm, f) != pcm) return 2;
        fclose(f);
        rg_track_desc d{};
        d.offset_bytes = off;
        d.frames = frames;
        d.sample_rate = head[2];
        d.channels = (uint16_t)channels;
        d.format = (uint16_t)format;
        const rg_flac_encode_options o{(uint32_t)sizeof(rg_flac_encode_options), head[4], head[5], 0};
        uint64_t offsets[2] = {0, 0};
        rg_flac_encode_result res;
        char err[256] = "";
        // the first call, into nothing, says how much the stream takes
        if (rg_fe_arena_host(1, &d, &bps, bytes ? arena->data() : nullptr, bytes, &o, nullptr, 0, offsets, &res, err, sizeof err) != RG_ERR_INVALID_ARG) return 3;
        std::vector<uint8_t> *out = new std::vector<uint8_t>((size_t)offsets[1]);  // exact size as well
        const int rc = rg_fe_arena_host(1, &d, &bps, bytes ? arena->data() : nullptr, bytes, &o, out->data(), out->size(), offsets, &res, err, sizeof err);
        if (rc != RG_OK) {
            fprintf(stderr, "%s: %d %s\n", argv[a], rc, err);
            return 3;
        }
        // decode: the planes must come back
        std::vector<std::vector<int32_t>> planes(channels, std::vector<int32_t>(frames ? (size_t)frames : 1));  // (the decoder refuses a null plane)
        std::vector<int32_t *> ptrs(channels);
        for (uint32_t c = 0; c < channels; ++c) ptrs[c] = planes[c].data();
        rg_flac_info info;
        if (rg_flac_decode_s32(out->data(), out->size(), ptrs.data(), frames, &info) != RG_FLAC_OK) return 4;
        int same = info.frames == frames && info.dropped_frames == 0;
        for (uint32_t c = 0; c < channels && same; ++c)
            for (uint64_t i = 0; i < frames && same; ++i) {
                int32_t v;
                if (elem == 2) {
                    int16_t s;
                    memcpy(&s, arena->data() + off + ((size_t)c * frames + i) * 2, 2);
                    v = s >> (16 - bps);
                } else {
                    memcpy(&v, arena->data() + off + ((size_t)c * frames + i) * 4, 4);
                    v >>= 32 - bps;
                }
                same = v == planes[c][i];
            }
        printf("%s %zu %d ", argv[a], out->size(), same);
        for (uint8_t b : *out) printf("%02x", b);
        printf("\n");
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_fe_arena_host(1, &d, &bps, arena->data(), bytes, &o, out->data(), out->size(), offsets, &res, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete out;
        delete arena;
    }
    return 0;
}
