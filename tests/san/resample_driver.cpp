// Stand-alone driver of tests/test_resample_sanitizers.py: the host side of the rational resampler and of the cross-rate
// fingerprint (rg_resample_host.cpp: route 0, the sum in double, and route 2, the kernel's f32 arithmetic, each followed by the
// fingerprint's host route on y) on tracks read from files, each in an exact-size heap arena at an offset that is only
// sample-aligned, with exact-size y, code and band arrays, so a read past a plane, a write past the last output, a signed overflow
// or a misaligned access aborts the driver.  A file is [u64 frames][u32 channels][u32 format][u32 sample rate][planes],
// little-endian; a line per file and route goes to stdout: the rg_xrate_result's bytes, y, the codes and the band energies in
// hexadecimal.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_resample.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t head[3];
        if (fread(&frames, 8, 1, f) != 1 || fread(head, 4, 3, f) != 3) return 2;
        const uint32_t channels = head[0], format = head[1], bps = format == RG_FMT_S16_PLANAR ? 2 : 4;
        const size_t off = bps * (size_t)(a % 5), pcm = (size_t)frames * channels * bps, bytes = off + pcm;
        std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: the planes end at the block's end
        if (pcm && fread(arena->data() + off, 1, pcm, f) != pcm) return 2;
        fclose(f);
        rg_track_desc d{};
        d.offset_bytes = off;
        d.frames = frames;
        d.sample_rate = head[2];
        d.channels = (uint16_t)channels;
        d.format = (uint16_t)format;
        uint32_t up = 0, down = 0, taps = 0;
        const uint64_t M = rg_resample_plan(d.sample_rate, &up, &down, &taps) == RG_OK ? rg_rs_count(frames, up, down, taps) : 0u;
        const uint32_t F = rg_fp_frames(M), K = F ? F - 1u : 0u;
        rg_xrate_result *r = new rg_xrate_result[1];
        rg_resample_result *rr = new rg_resample_result[1];
        float *y = new float[M], *y2 = new float[M];  // exact sizes
        uint32_t *codes = new uint32_t[K];
        float *bands = new float[(size_t)F * RG_FP_BANDS];
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            int rc = rg_xr_arena_host(route, 1, &d, bytes ? arena->data() : nullptr, bytes, r, codes, bands, y, err, sizeof err);
            if (rc == RG_OK) rc = rg_rs_arena_host(route, 1, &d, bytes ? arena->data() : nullptr, bytes, rr, y2, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            if (r->codes != K || r->fp_frames != F || r->resampled != M || rr->resampled != M || memcmp(y, y2, M * sizeof(float)) != 0) return 4;
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" x");
            hex(y, (size_t)M * 4);
            printf(" x");
            hex(codes, (size_t)K * 4);
            printf(" x");
            hex(bands, (size_t)F * RG_FP_BANDS * 4);
            printf("\n");
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_rs_arena_host(2, 1, &d, arena->data(), bytes, rr, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete[] bands;
        delete[] codes;
        delete[] y2;
        delete[] y;
        delete[] rr;
        delete[] r;
        delete arena;
    }
    return 0;
}
