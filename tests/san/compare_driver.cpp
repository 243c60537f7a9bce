// Stand-alone driver of tests/test_compare_sanitizers.py: the host routes of the null test (rg_compare_host.cpp: route 0, the serial
// twin, and route 2, the kernels' cutting and fold arithmetic) on pairs of tracks read from files, each pair in an exact-size heap
// arena at offsets that are only sample-aligned, so a read past a plane, a signed overflow or a misaligned access aborts the
// driver.  A file is [u64 frames a][u64 frames b][i64 hint][u32 channels a, b][u32 format a, b][u32 sample rate a, b][u32 radius]
// [u32 segments][u32 segment_frames][u32 block_frames][planes of a][planes of b], little-endian; a line per file and route goes to
// stdout: the rg_compare_result's bytes in hexadecimal, then the lag rows', then the block rows'.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_compare.h"

static void hex(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t j = 0; j < n; ++j) printf("%02x", b[j]);
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames[2] = {0, 0};
        int64_t hint = 0;
        uint32_t head[10];
        if (fread(frames, 8, 2, f) != 2 || fread(&hint, 8, 1, f) != 1 || fread(head, 4, 10, f) != 10) return 2;
        const uint32_t bps_a = head[2] == RG_FMT_S16_PLANAR ? 2 : 4, bps_b = head[3] == RG_FMT_S16_PLANAR ? 2 : 4;
        const size_t pcm_a = (size_t)frames[0] * head[0] * bps_a, pcm_b = (size_t)frames[1] * head[1] * bps_b;
        const size_t off_a = bps_a * (size_t)(a % 5), off_b = (off_a + pcm_a + bps_b - 1) / bps_b * bps_b, bytes = off_b + pcm_b;
        std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: b's planes end at the block's end
        if ((pcm_a && fread(arena->data() + off_a, 1, pcm_a, f) != pcm_a) || (pcm_b && fread(arena->data() + off_b, 1, pcm_b, f) != pcm_b)) return 2;
        fclose(f);
        rg_track_desc d[2] = {};
        for (int k = 0; k < 2; ++k) {
            d[k].offset_bytes = k ? off_b : off_a;
            d[k].frames = frames[k];
            d[k].sample_rate = head[4 + k];
            d[k].channels = (uint16_t)head[k];
            d[k].format = (uint16_t)head[2 + k];
        }
        const rg_compare_opts o{RG_CMP_ALIGN_HINT,         RG_CMP_DEFAULT_COARSE_RADIUS, head[6], head[7], head[8], head[9],
                                RG_CMP_DEFAULT_DRIFT_FRAMES, RG_CMP_DEFAULT_LOCK_PERMILLE, RG_CMP_DEFAULT_REQUANT_MILLILSB2};
        const rg_compare_pair pair{0u, 1u, hint};
        const size_t slab = (size_t)head[7] * RG_CMP_MAX_CHANNELS * (2 * (size_t)head[6] + 3), n_blocks = 1200;
        rg_compare_result *r = new rg_compare_result[1];
        std::vector<int64_t> *rows = new std::vector<int64_t>(slab);  // exact size as well
        std::vector<rg_compare_block> *blocks = new std::vector<rg_compare_block>(n_blocks);
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            const int rc = rg_cmp_arena_host(route, 2, d, 1, &pair, &o, bytes ? arena->data() : nullptr, bytes, r, blocks->data(), n_blocks, rows->data(), err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            printf("%s %d ", argv[a], route);
            hex(r, sizeof *r);
            printf(" ");
            hex(rows->data(), rows->size() * sizeof(int64_t));
            printf(" ");
            hex(blocks->data(), (r->blocks < n_blocks ? r->blocks : n_blocks) * sizeof(rg_compare_block));
            printf("\n");
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d[1].frames = frames[1] + 1;
        if (rg_cmp_arena_host(0, 2, d, 1, &pair, &o, arena->data(), bytes, r, nullptr, 0, nullptr, err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete blocks;
        delete rows;
        delete[] r;
        delete arena;
    }
    return 0;
}
