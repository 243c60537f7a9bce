// Stand-alone driver of tests/test_tempo_sanitizers.py: the host side of the tempo scan (rg_tempo_host.cpp: route 0, the serial
// twin, route 2, the kernels' pairs of frames and tiles, and the serial stage 2) on tracks read from files, each in an exact-size
// heap arena at an offset that is only sample-aligned, with exact-size onset and band arrays, so a read past a plane, a write
// past the last onset, a signed overflow or a misaligned access aborts the driver.  A file is [u64 frames][u32 channels]
// [u32 format][u32 sample rate][planes], little-endian; a line per file and route goes to stdout: the rg_tempo_result's bytes
// (at the small options {32, 8, 300}), its onsets and its band energies in hexadecimal.  Then stage 2 runs over every file's
// route 2 onsets, packed end to end in an exact-size block, with an exact-size block for the sums C: a last line with the
// records and the sums.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_tempo.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    std::vector<uint16_t> all_onsets;
    std::vector<uint32_t> counts, rates;
    rg_tempo_opts o;
    char err[256] = "";
    const rg_tempo_opts small{32, 8, 300};
    if (rg_tp_options(&small, &o, err, sizeof err) != RG_OK) return 1;
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
        uint32_t e[RG_TEMPO_BANDS + 1];
        const uint32_t F = rg_tempo_bands(d.sample_rate, e) == RG_OK ? rg_fp_frames(frames) : 0u, K = F ? F - 1u : 0u;
        rg_tempo_result *r = new rg_tempo_result[1];
        uint16_t *onsets = new uint16_t[K];  // exact sizes
        float *bands = new float[(size_t)F * RG_TEMPO_BANDS];
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_tp_arena_host(route, 1, &d, bytes ? arena->data() : nullptr, bytes, o, r, onsets, bands, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            if (r->onsets != K || r->band_frames != F) return 4;
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" x");
            hex(onsets, (size_t)K * 2);
            printf(" x");
            hex(bands, (size_t)F * RG_TEMPO_BANDS * 4);
            printf("\n");
        }
        all_onsets.insert(all_onsets.end(), onsets, onsets + K);
        counts.push_back(K);
        rates.push_back(d.sample_rate);
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_tp_arena_host(0, 1, &d, arena->data(), bytes, o, r, nullptr, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete[] bands;
        delete[] onsets;
        delete[] r;
        delete arena;
    }
    const size_t n = counts.size();
    uint16_t *packed = new uint16_t[all_onsets.size()];
    if (!all_onsets.empty()) memcpy(packed, all_onsets.data(), all_onsets.size() * 2);
    rg_tempo_result *rec = new rg_tempo_result[n];
    int64_t *acf = new int64_t[n * o.window];
    if (rg_tp_from_onsets_check(n, counts.data(), packed, err, sizeof err) != RG_OK) return 6;
    if (rg_tp_from_onsets_host(n, counts.data(), rates.data(), packed, o, rec, acf) != RG_OK) return 6;
    printf("stage2 x");
    hex(rec, n * sizeof *rec);
    printf(" x");
    hex(acf, n * o.window * sizeof *acf);
    printf("\n");
    delete[] acf;
    delete[] rec;
    delete[] packed;
    return 0;
}
