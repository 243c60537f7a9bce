// Driver of tests/test_pipe_plan_cpu.py: the loader pipeline's two sizing rules (mp3rgain_amd/csrc/rg_pipe_plan.h), one
// question per line of stdin, one answer per line of stdout.
//   cap <open_index> <chunk_units> <starved> <files_placed> <units_placed> <n_files>  ->  "<unit cap> <tapering>"
//   part <used_bytes> <units> <min_bytes_per_unit> <starved>                          ->  "<0 | 1>"
#include <stdio.h>
#include <string.h>

#include "rg_pipe_plan.h"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a, b, c, d, e, f;
        double at;
        if (sscanf(line, "cap %llu %llu %llu %llu %llu %llu", &a, &b, &c, &d, &e, &f) == 6) {
            bool tapering = false;
            const uint64_t cap = rg_pipe_unit_cap((size_t)a, b, c != 0, (size_t)d, e, (size_t)f, &tapering);
            printf("%llu %d\n", (unsigned long long)cap, tapering ? 1 : 0);
        } else if (sscanf(line, "part %llu %llu %lf %llu", &a, &b, &at, &c) == 4) {
            printf("%d\n", rg_pipe_chunk_is_part((size_t)a, b, at, c != 0) ? 1 : 0);
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
