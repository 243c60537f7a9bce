// Stand-alone driver of tests/test_key_sanitizers.py: the host side of the key scan (rg_key_host.cpp: route 0, the serial twin,
// route 2, the kernels' FIR sums and tiles, and the serial stage 2) on tracks read from files, each in an exact-size heap arena
// at an offset that is only sample-aligned, with exact-size arrays for the decimated signal, the band energies and the rows, so
// a read past a plane, a write past the last row, a signed overflow or a misaligned access aborts the driver.  A file is
// [u64 frames][u32 channels][u32 format][u32 sample rate][planes], little-endian; a line per file and route goes to stdout: the
// rg_key_result's bytes (at segment 8), its decimated signal, band energies and rows in hexadecimal.  Then stage 2 runs over
// every file's route 2 rows, packed end to end in an exact-size block: a last line with the records.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_key.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    std::vector<uint16_t> all_rows;
    std::vector<uint32_t> counts;
    rg_key_opts o;
    char err[256] = "";
    const rg_key_opts small{8};
    if (rg_key_options(&small, &o, err, sizeof err) != RG_OK) return 1;
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
        RgKeyTrack t;
        if (rg_key_track(0, d, bytes, &t, err, sizeof err) != RG_OK) return 3;
        const uint32_t M = t.m, F = t.rows;
        rg_key_result *r = new rg_key_result[1];
        float *y = new float[M];  // exact sizes
        float *bands = new float[(size_t)F * RG_KEY_BANDS];
        uint16_t *rows = new uint16_t[(size_t)F * RG_KEY_CHROMA];
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_key_arena_host(route, 1, &d, bytes ? arena->data() : nullptr, bytes, o, r, y, bands, rows, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            if (r->decimated != M || r->rows != F) return 4;
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" x");
            hex(y, (size_t)M * 4);
            printf(" x");
            hex(bands, (size_t)F * RG_KEY_BANDS * 4);
            printf(" x");
            hex(rows, (size_t)F * RG_KEY_CHROMA * 2);
            printf("\n");
        }
        all_rows.insert(all_rows.end(), rows, rows + (size_t)F * RG_KEY_CHROMA);
        counts.push_back(F);
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_key_arena_host(0, 1, &d, arena->data(), bytes, o, r, nullptr, nullptr, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete[] rows;
        delete[] bands;
        delete[] y;
        delete[] r;
        delete arena;
    }
    const size_t n = counts.size();
    uint16_t *packed = new uint16_t[all_rows.size()];
    if (!all_rows.empty()) memcpy(packed, all_rows.data(), all_rows.size() * 2);
    rg_key_result *rec = new rg_key_result[n];
    if (rg_key_from_chroma_check(n, counts.data(), packed, err, sizeof err) != RG_OK) return 6;
    if (rg_key_from_chroma_host(n, counts.data(), packed, o, rec) != RG_OK) return 6;
    printf("stage2 x");
    hex(rec, n * sizeof *rec);
    printf("\n");
    delete[] rec;
    delete[] packed;
    return 0;
}
