// Sanitizer driver (tests/test_flac_sanitizers.py): every file on the command line, as an exact-size heap copy, through the
// host FLAC decoder's scan, frame index, whole-stream decoder and self-check (include/mp3rgain_amd_flac.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mp3rgain_amd_flac.h"

int main(int argc, char **argv) {
    unsigned long long samples = 0, files = 0, dropped = 0;
    for (int a = 1; a < argc; ++a) {
        std::vector<unsigned char> v;
        FILE *f = fopen(argv[a], "rb");
        if (!f) continue;
        unsigned char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        fclose(f);
        unsigned char *p = static_cast<unsigned char *>(malloc(v.size() ? v.size() : 1));
        if (!v.empty()) memcpy(p, v.data(), v.size());
        rg_flac_info si;
        (void)rg_flac_is_flac(p, v.size());
        (void)rg_flac_scan(p, v.size(), &si);
        size_t nf = 0;
        if (rg_flac_index_frames(p, v.size(), nullptr, 0, &nf, &si) == RG_FLAC_ERR_CAPACITY || nf == 0) {
            std::vector<rg_flac_frame> fr(nf + 1);
            (void)rg_flac_index_frames(p, v.size(), fr.data(), nf, &nf, &si);
        }
        if (si.channels >= 1 && si.channels <= 8 && si.frames < (1u << 22)) {
            std::vector<std::vector<int32_t>> pl(si.channels, std::vector<int32_t>(si.frames + 1));
            int32_t *ptr[8];
            for (uint32_t c = 0; c < si.channels; ++c) ptr[c] = pl[c].data();
            rg_flac_info di;
            if (rg_flac_decode_s32(p, v.size(), ptr, si.frames, &di) == RG_FLAC_OK) {
                samples += di.frames;
                dropped += di.dropped_frames;
            }
            if (rg_flac_index_selfcheck(p, v.size()) == 1) {
                fprintf(stderr, "%s: the index and the decoder disagree\n", argv[a]);
                return 1;
            }
        }
        free(p);
        ++files;
    }
    printf("%llu files, %llu samples, %llu frames dropped\n", files, samples, dropped);
    return 0;
}
