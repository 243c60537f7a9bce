// Stand-alone driver of tests/test_rip_offsets_sanitizers.py: the host routes of the AccurateRip signatures at every drive
// offset (rg_rip_host.cpp: route 0, the definition, and route 2, arv1 by the sliding recurrence) on a disc read from a file,
// its tracks stored back to front in an exact-size heap arena at offsets that are only sample-aligned, so a read past a
// plane or before the disc's first word, a signed overflow or a misaligned access aborts the driver.
// The file is [u32 tracks][u32 radius] and per track [u64 frames][u32 flags][L plane][R plane], little-endian.  The tables go
// to the output file as uint32: arv1 and arv2 of route 0, then arv1 of route 2.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_rip.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n = 0, radius = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&radius, 4, 1, f) != 1) return 2;
    std::vector<std::vector<unsigned char>> pcm(n);
    std::vector<rg_track_desc> descs(n);
    std::vector<uint32_t> flags(n);
    size_t bytes = 0;
    for (uint32_t t = 0; t < n; ++t) {
        uint64_t frames = 0;
        if (fread(&frames, 8, 1, f) != 1 || fread(&flags[t], 4, 1, f) != 1) return 2;
        pcm[t].resize((size_t)frames * 4);
        if (frames && fread(pcm[t].data(), 4, (size_t)frames, f) != frames) return 2;
        memset(&descs[t], 0, sizeof descs[t]);
        descs[t].frames = frames;
        descs[t].sample_rate = 44100;
        descs[t].channels = 2;
        descs[t].format = RG_FMT_S16_PLANAR;
        bytes += pcm[t].size() + 2;
    }
    fclose(f);
    std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: the first track's planes end at the block's end
    size_t at = 0;
    for (uint32_t t = n; t-- > 0;) {  // back to front, two bytes in front of each
        at += 2;
        descs[t].offset_bytes = at;
        if (!pcm[t].empty()) memcpy(arena->data() + at, pcm[t].data(), pcm[t].size());
        at += pcm[t].size();
    }
    const size_t cells = (size_t)n * (2 * (size_t)radius + 1);
    std::vector<uint32_t> *v1 = new std::vector<uint32_t>(cells), *v2 = new std::vector<uint32_t>(cells), *s1 = new std::vector<uint32_t>(cells);
    char err[256] = "";
    std::vector<RgRipDiscTrack> recs;
    for (int route = 0; route <= 2; route += 2) {
        int rc = rg_rip_offsets_check(route, n, descs.data(), flags.data(), (int32_t)radius, arena->data(), bytes, nullptr, &recs, err, sizeof err);
        if (rc == RG_OK && n) rc = rg_rip_offsets_host(route, recs, (int32_t)radius, arena->data(), route ? s1->data() : v1->data(), route ? nullptr : v2->data());
        if (rc != RG_OK) {
            fprintf(stderr, "route %d: %d %s\n", route, rc, err);
            return 3;
        }
    }
    // a track that reaches one frame beyond the arena is refused, not read; so is a radius beyond the window
    if (n) {
        descs[0].frames += 1;
        if (rg_rip_offsets_check(0, n, descs.data(), flags.data(), (int32_t)radius, arena->data(), bytes, nullptr, &recs, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        descs[0].frames -= 1;
    }
    if (rg_rip_offsets_check(0, n, descs.data(), flags.data(), RG_RIP_OFFSET_MAX + 1, arena->data(), bytes, nullptr, &recs, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (const std::vector<uint32_t> *v : {v1, v2, s1})
        if (cells && fwrite(v->data(), 4, cells, o) != cells) return 2;
    fclose(o);
    delete arena;
    delete v1;
    delete v2;
    delete s1;
    return 0;
}
