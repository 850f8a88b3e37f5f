// The window rule of raw-session recalibration (sigfish_amd/csrc/recal_rule.hpp) as a stand-alone host program: prints the
// window for every q_avail in 0..80, both values of `ended` and four configurations over (norm 25, query 70), then the
// expansion of "double" for the shapes named on the command line (norm:query ...), then what recal_list_error says about the
// lists the command line must refuse.  tests/test_recal_cpu.py compares every line with the Python twin.
#include <cstdio>
#include <cstdlib>

#include "recal_rule.hpp"

int main(int argc, char **argv) {
    const int32_t norm = 25, query = 70;
    const int32_t at[3] = {30, 40, 70};
    struct Config {
        const char *name;
        int32_t n_at;
        uint32_t flags;
    };
    const Config configs[4] = {{"none", 0, 0}, {"at", 3, 0}, {"at_end", 0, sfa::kRecalAtEnd}, {"both", 3, sfa::kRecalAtEnd}};
    for (const Config &c : configs) {
        if (sfa::recal_list_error(at, c.n_at, norm, query)) return 2;
        for (int ended = 0; ended < 2; ++ended) {
            printf("window %s ended=%d:", c.name, ended);
            for (int32_t q = 0; q <= 80; ++q) printf(" %d", sfa::recal_window(sfa::recal_q_avail(q + 3, 3, query), ended != 0, norm, query, at, c.n_at, c.flags));
            printf("\n");
        }
    }
    for (int i = 1; i < argc; ++i) {
        int n = 0, q = 0;
        if (sscanf(argv[i], "%d:%d", &n, &q) != 2) return 2;
        int32_t pts[sfa::kRecalMaxPoints];
        const int32_t m = sfa::recal_double(n, q, pts);
        printf("double %d:%d:", n, q);
        for (int32_t k = 0; k < m; ++k) printf(" %d", pts[k]);
        printf("\n");
        if (sfa::recal_list_error(pts, m, n, q)) return 3;
    }
    const int32_t not_ascending[3] = {40, 30, 70}, twice[2] = {40, 40}, at_norm[2] = {25, 40}, above[2] = {40, 71};
    int32_t many[33];
    for (int k = 0; k < 33; ++k) many[k] = 26 + k;
    printf("refused not_ascending=%d twice=%d at_norm=%d above=%d many=%d empty=%d full=%d\n", sfa::recal_list_error(not_ascending, 3, norm, query) != nullptr,
           sfa::recal_list_error(twice, 2, norm, query) != nullptr, sfa::recal_list_error(at_norm, 2, norm, query) != nullptr,
           sfa::recal_list_error(above, 2, norm, query) != nullptr, sfa::recal_list_error(many, 33, norm, 100) != nullptr,
           sfa::recal_list_error(nullptr, 0, norm, query) != nullptr, sfa::recal_list_error(many, 32, norm, 100) != nullptr);
    return 0;
}
