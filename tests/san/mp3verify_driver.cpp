// Sanitizer driver (tests/test_mp3_verify_sanitizers.py): every file on the command line, as an exact-size heap copy, through
// the host side of MP3 verification (include/mp3rgain_amd_mp3verify.h): the info-tag parser, the host twin that fills the result
// record, and the kernels' fold arithmetic run on the host, which must agree with the record's serial music CRC.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mp3rgain_amd_mp3verify.h"

int main(int argc, char **argv) {
    unsigned long long files = 0, verdicts = 0, tags = 0;
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
        rg_mp3_tag_info t;
        rg_mp3_verify_result r;
        const int trc = rg_mp3_info_tag(p, v.size(), &t);
        if (rg_mp3_verify_data(p, v.size(), &r) == RG_OK) {
            ++verdicts;
            if (r.flags & RG_MP3_VERIFY_HAS_LAME_EXT) {
                ++tags;
                const size_t from = (size_t)t.tag_frame_offset + t.tag_frame_bytes;
                if (trc != RG_OK || from + r.audio_bytes > v.size() || rg_mp3_crc_folded_host(p + from, (size_t)r.audio_bytes) != r.music_crc_computed) {
                    fprintf(stderr, "%s: the folded CRC and the record disagree\n", argv[a]);
                    return 1;
                }
            }
        }
        free(p);
        ++files;
    }
    printf("%llu files, %llu verdicts, %llu with the extension\n", files, verdicts, tags);
    return 0;
}
