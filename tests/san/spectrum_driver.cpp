// Stand-alone driver of tests/test_spectrum_sanitizers.py: the host routes of the spectral scan (rg_spectrum_host.cpp: route 0,
// the serial twin in double, and route 2, the kernels' f32 arithmetic) on tracks read from files, each in an exact-size heap
// arena at an offset that is only sample-aligned, so a read past a plane, a signed overflow or a misaligned access aborts the
// driver.  A file is [u64 frames][u32 channels][u32 format][u32 sample rate][planes], little-endian; a line per file, route and
// channel goes to stdout: the record's fields and the 256 band energies as hexadecimal floats.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_spectrum.h"

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
        rg_spectrum_result *r = new rg_spectrum_result[1];
        std::vector<double> *e = new std::vector<double>(RG_SPEC_MAX_CHANNELS * RG_SPEC_BANDS);
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_spec_arena_host(route, 1, &d, nullptr, bytes ? arena->data() : nullptr, bytes, r, e->data(), err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            for (uint32_t c = 0; c < r->channels; ++c) {
                const rg_spectrum_channel &s = r->ch[c];
                printf("%s %d %u %u %u %u %u %a %a", argv[a], route, c, r->flags, s.flags, s.analysed_frames, s.skipped_frames, s.cutoff_hz, s.edge_db);
                for (uint32_t j = 0; j < RG_SPEC_BANDS; ++j) printf(" %a", (*e)[c * RG_SPEC_BANDS + j]);
                printf("\n");
            }
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_spec_arena_host(0, 1, &d, nullptr, arena->data(), bytes, r, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete e;
        delete[] r;
        delete arena;
    }
    return 0;
}
