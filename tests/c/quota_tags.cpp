// replay::quota_tags (sigfish_amd/csrc/cli/replay.hpp) on hand-written records; tests/test_session_quota_cpu.py compares its lines
// with realtime.quota_tags.  stdin: <n names> <names>, then one on_group per line; stdout: the tag with tabs written as \t.
#include <stdio.h>

#include <string>
#include <vector>

#include "cli/replay.hpp"

int main() {
    int n;
    if (scanf("%d", &n) != 1 || n < 0 || n > 1023) return 2;
    std::vector<std::string> names(n);
    for (std::string &s : names) {
        char buf[64];
        if (scanf("%63s", buf) != 1) return 2;
        s = buf;
    }
    int on_group;
    while (scanf("%d", &on_group) == 1) {
        std::string out;
        for (const char c : cli::replay::quota_tags(on_group, names)) out += c == '\t' ? std::string("\\t") : std::string(1, c);
        printf("%s\n", out.c_str());
    }
    return 0;
}
