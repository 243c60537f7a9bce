// Stand-alone driver of tests/test_rip_sanitizers.py: the host routes of the rip checksums (rg_rip_host.cpp: route 0, the
// serial twin, and route 2, the kernels' fold arithmetic) on tracks read from files, each in an exact-size heap arena at an
// offset that is only sample-aligned, so a read past a plane, a signed overflow or a misaligned access aborts the driver.
// A file is [u64 frames][u32 flags][L plane][R plane], little-endian; a line per file and route goes to stdout.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_rip.h"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t flags = 0;
        if (fread(&frames, 8, 1, f) != 1 || fread(&flags, 4, 1, f) != 1) return 2;
        const size_t off = 2 * (size_t)(a % 5), bytes = off + (size_t)frames * 4;
        std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: the planes end at the block's end
        if (frames && fread(arena->data() + off, 4, (size_t)frames, f) != frames) return 2;
        fclose(f);
        rg_track_desc d{};
        d.offset_bytes = off;
        d.frames = frames;
        d.sample_rate = 44100;
        d.channels = 2;
        d.format = RG_FMT_S16_PLANAR;
        rg_rip_result r[2];
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            rg_rip_result *out = &r[route / 2];
            const int rc = rg_rip_arena_host(route, 1, &d, &flags, bytes ? arena->data() : nullptr, bytes, out, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            printf("%s %d %08x %08x %llu %08x %08x\n", argv[a], route, out->crc32, out->crc32_nonnull, (unsigned long long)out->null_samples, out->arv1, out->arv2);
        }
        if (memcmp(&r[0], &r[1], sizeof r[0]) != 0) {
            fprintf(stderr, "%s: routes 0 and 2 differ\n", argv[a]);
            return 4;
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_rip_arena_host(0, 1, &d, &flags, arena->data(), bytes, &r[0], err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete arena;
    }
    return 0;
}
