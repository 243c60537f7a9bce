// Stand-alone driver of tests/test_ancestry_sanitizers.py: the host routes of the lossy ancestry scan (rg_ancestry_host.cpp: route
// 0, the serial twin, and route 2, the kernels' cutting into phases and tiles) on tracks read from files, each in an exact-size
// heap arena at an offset that is only sample-aligned, so a read past a plane, before frame 0 or past the last granule, a signed
// overflow or a misaligned access aborts the driver.  A file is [u64 frames][u32 channels][u32 format][u32 sample rate]
// [u32 segments][u32 granules][planes], little-endian; a line per file and route goes to stdout: the rg_ancestry_result's bytes
// and then the counts of its views in hexadecimal.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_ancestry.h"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t head[5];
        if (fread(&frames, 8, 1, f) != 1 || fread(head, 4, 5, f) != 5) return 2;
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
        const rg_ancestry_opts o{head[3], head[4], 0.0, 0.0, 0.0f, 0u};
        rg_ancestry_result *r = new rg_ancestry_result[1];
        std::vector<uint64_t> *counts = new std::vector<uint64_t>((size_t)RG_ANC_MAX_VIEWS * 2 * RG_ANC_ALIGNMENTS);
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_anc_arena_host(route, 1, &d, &o, bytes ? arena->data() : nullptr, bytes, r, counts->data(), err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            printf("%s %d ", argv[a], route);
            const unsigned char *b = reinterpret_cast<const unsigned char *>(r);
            for (size_t j = 0; j < sizeof *r; ++j) printf("%02x", b[j]);
            printf(" ");
            b = reinterpret_cast<const unsigned char *>(counts->data());
            for (size_t j = 0; j < (size_t)r->views * 2 * RG_ANC_ALIGNMENTS * sizeof(uint64_t); ++j) printf("%02x", b[j]);
            printf("\n");
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_anc_arena_host(0, 1, &d, &o, arena->data(), bytes, r, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete counts;
        delete[] r;
        delete arena;
    }
    return 0;
}
