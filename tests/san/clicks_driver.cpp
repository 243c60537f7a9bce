// Stand-alone driver of tests/test_clicks_cpu.py: the host routes of the click scan (rg_clicks_host.cpp: route 0, the serial twin,
// and route 2, the kernels' tile and fold code on one lane) on tracks read from files, each in an exact-size heap arena at an
// offset that is only sample-aligned, so a read past a plane, a signed overflow or a misaligned access aborts the driver.  A file
// is [u64 frames][u32 channels][u32 format][u32 sample rate][7 x u32 options][planes], little-endian; a line per file and route
// goes to stdout: the rg_clicks_result's bytes in hexadecimal, then the event row's.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_clicks.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t head[10];
        if (fread(&frames, 8, 1, f) != 1 || fread(head, 4, 10, f) != 10) return 2;
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
        const rg_clicks_opts o{head[3], head[4], head[5], head[6], head[7], head[8], head[9]};
        rg_clicks_result *r = new rg_clicks_result[1];
        std::vector<rg_clicks_event> *row = new std::vector<rg_clicks_event>(o.max_events);  // exact size as well
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_ck_arena_host(route, 1, &d, &o, bytes ? arena->data() : nullptr, bytes, r, row->data(), err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" ");
            hex(row->data(), row->size() * sizeof(rg_clicks_event));
            printf("\n");
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_ck_arena_host(0, 1, &d, &o, arena->data(), bytes, r, row->data(), err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete row;
        delete[] r;
        delete arena;
    }
    return 0;
}
