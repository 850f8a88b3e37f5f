// replay::group_is_full and replay::group_cover_line (sigfish_amd/csrc/cli/replay.hpp) on hand-written records;
// tests/test_realtime_group_cap_cpu.py compares its lines with realtime.group_is_full and realtime.group_cover_line.
// stdin: one record per line, <name> <columns> <capped> <depth_sum>; stdout: <0|1 full> and the summary line with tabs written
// as \t (the line's own newline dropped).
#include <stdio.h>

#include <string>

#include "cli/replay.hpp"

int main() {
    char name[64];
    long long columns, capped;
    unsigned long long sum;
    while (scanf("%63s %lld %lld %llu", name, &columns, &capped, &sum) == 4) {
        std::string out;
        for (const char c : cli::replay::group_cover_line(name, columns, capped, sum)) {
            if (c == '\n') continue;
            out += c == '\t' ? std::string("\\t") : std::string(1, c);
        }
        printf("%d %s\n", cli::replay::group_is_full(columns, capped) ? 1 : 0, out.c_str());
    }
    return 0;
}
