// replay::group_tags (sigfish_amd/csrc/cli/replay.hpp), the two tags `sigfish-amd realtime --by-name` adds to a line, as a
// stand-alone host program; tests/test_session_groups_cpu.py compares its strings with realtime.group_tags of the same records.
//   <n names> <names ...> then lines of: <best> <second> <best_score> <second_score> <n_events>   ->  the tags, tabs as "\t"
#include <stdio.h>

#include <string>
#include <vector>

#include "cli/replay.hpp"

int main() {
    int n;
    if (scanf("%d", &n) != 1 || n < 0 || n > 1023) return 2;
    std::vector<std::string> names;
    for (int k = 0; k < n; ++k) {
        char name[128];
        if (scanf("%127s", name) != 1) return 2;
        names.push_back(name);
    }
    int best, second, n_events;
    float bs, ss;
    while (scanf("%d %d %f %f %d", &best, &second, &bs, &ss, &n_events) == 5) {
        const std::string t = cli::replay::group_tags(best, second, bs, ss, n_events, names);
        for (const char c : t) c == '\t' ? (void)fputs("\\t", stdout) : (void)putchar(c);
        putchar('\n');
    }
    return 0;
}
