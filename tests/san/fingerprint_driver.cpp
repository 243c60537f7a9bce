// Stand-alone driver of tests/test_fingerprint_sanitizers.py: the host side of the duplicate finder (rg_fprint_host.cpp: route 0,
// the serial twin, route 2, the kernels' pairs of frames and tiles, and the serial match) on tracks read from files, each in an
// exact-size heap arena at an offset that is only sample-aligned, with exact-size code and band arrays, so a read past a plane,
// a write past the last code, a signed overflow or a misaligned access aborts the driver.  A file is [u64 frames][u32 channels]
// [u32 format][u32 sample rate][planes], little-endian; a line per file and route goes to stdout: the rg_fingerprint_result's
// bytes, its codes and its band energies in hexadecimal.  Then every pair of the files' route 2 codes is matched at the small
// options {32, 3, 8, 100}, the code arrays packed end to end in an exact-size block: a last line with the pair records.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_fprint.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    std::vector<uint32_t> all_codes, counts, rates;
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
        uint32_t e[RG_FP_BANDS + 1];
        const uint32_t F = rg_fingerprint_edges(d.sample_rate, e) == RG_OK ? rg_fp_frames(frames) : 0u, K = F ? F - 1u : 0u;
        rg_fingerprint_result *r = new rg_fingerprint_result[1];
        uint32_t *codes = new uint32_t[K];  // exact sizes
        float *bands = new float[(size_t)F * RG_FP_BANDS];
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_fp_arena_host(route, 1, &d, bytes ? arena->data() : nullptr, bytes, r, codes, bands, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            if (r->codes != K || r->fp_frames != F) return 4;
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" x");
            hex(codes, (size_t)K * 4);
            printf(" x");
            hex(bands, (size_t)F * RG_FP_BANDS * 4);
            printf("\n");
        }
        all_codes.insert(all_codes.end(), codes, codes + K);
        counts.push_back(K);
        rates.push_back(d.sample_rate);
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_fp_arena_host(0, 1, &d, arena->data(), bytes, r, nullptr, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete[] bands;
        delete[] codes;
        delete[] r;
        delete arena;
    }
    const size_t n = counts.size(), n_rec = n * (n - 1) / 2;
    uint32_t *packed = new uint32_t[all_codes.size()];
    if (!all_codes.empty()) memcpy(packed, all_codes.data(), all_codes.size() * 4);
    rg_fingerprint_pair_record *rec = new rg_fingerprint_pair_record[n_rec];
    const rg_fingerprint_opts o{32, 3, 8, 100};
    if (rg_fp_match_codes_host(n, counts.data(), rates.data(), packed, o, rec) != RG_OK) return 6;
    uint32_t *groups = new uint32_t[n], *matches = new uint32_t[n];
    const size_t found = rg_fingerprint_groups(n, rec, groups, matches);
    printf("pairs %zu x", found);
    hex(rec, n_rec * sizeof *rec);
    printf(" x");
    hex(groups, n * 4);
    printf("\n");
    delete[] matches;
    delete[] groups;
    delete[] rec;
    delete[] packed;
    return 0;
}
