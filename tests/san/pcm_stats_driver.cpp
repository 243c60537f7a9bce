// Stand-alone driver of tests/test_pcm_stats_sanitizers.py: the host routes of the PCM defect scan (rg_stats_host.cpp: route 0,
// the serial twin, and route 2, the kernels' chunking and fold arithmetic) on tracks read from files, each in an exact-size heap
// arena at an offset that is only sample-aligned, so a read past a plane, a signed overflow or a misaligned access aborts the
// driver.  A file is [u64 frames][u32 channels][u32 format][u32 bits][u32 min_clip_run][u32 min_zero_run][planes], little-endian;
// a line per file, route and channel goes to stdout.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../mp3rgain_amd/csrc/rg_stats.h"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        uint64_t frames = 0;
        uint32_t head[5];
        if (fread(&frames, 8, 1, f) != 1 || fread(head, 4, 5, f) != 5) return 2;
        const uint32_t channels = head[0], format = head[1], bits = head[2], bps = format == RG_FMT_S16_PLANAR ? 2 : 4;
        const rg_pcm_stats_opts opts{head[3], head[4]};
        const size_t off = bps * (size_t)(a % 5), pcm = (size_t)frames * channels * bps, bytes = off + pcm;
        std::vector<unsigned char> *arena = new std::vector<unsigned char>(bytes);  // exact size: the planes end at the block's end
        if (pcm && fread(arena->data() + off, 1, pcm, f) != pcm) return 2;
        fclose(f);
        rg_track_desc d{};
        d.offset_bytes = off;
        d.frames = frames;
        d.sample_rate = 44100;
        d.channels = (uint16_t)channels;
        d.format = (uint16_t)format;
        rg_pcm_stats_result *r = new rg_pcm_stats_result[2];
        char err[256] = "";
        for (int route = 0; route <= 2; route += 2) {
            rg_pcm_stats_result *out = &r[route / 2];
            const int rc = rg_stats_arena_host(route, 1, &d, &bits, &opts, bytes ? arena->data() : nullptr, bytes, out, err, sizeof err);
            if (rc != RG_OK) {
                fprintf(stderr, "%s: route %d: %d %s\n", argv[a], route, rc, err);
                return 3;
            }
            for (uint32_t c = 0; c < out->channels; ++c) {
                const rg_pcm_stats_channel &s = out->ch[c];
                printf("%s %d %u %u %a %a %lld %u %u %u %u %u %u %u %u %u %u %u %u\n", argv[a], route, c, out->flags, s.min, s.max, (long long)s.sum, s.or_mask,
                       s.effective_bits, s.clipped, s.clip_runs, s.longest_clip_run, s.first_clip_run, s.zeros, s.lead_zeros, s.trail_zeros, s.zero_runs,
                       s.longest_zero_run, s.nonfinite);
            }
        }
        if (memcmp(&r[0], &r[1], sizeof r[0]) != 0) {
            fprintf(stderr, "%s: routes 0 and 2 differ\n", argv[a]);
            return 4;
        }
        // a record that reaches one frame beyond the arena is refused, not read
        d.frames = frames + 1;
        if (rg_stats_arena_host(0, 1, &d, &bits, &opts, arena->data(), bytes, &r[0], err, sizeof err) != RG_ERR_INVALID_ARG) return 5;
        delete[] r;
        delete arena;
    }
    return 0;
}
