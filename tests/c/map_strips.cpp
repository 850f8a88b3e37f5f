// map_strips.cpp -- event maps of rows beyond 2048 events in row strips, the parts that need no GPU (tests/test_map_strips_cpu.py).
//   1. plan_map_slices_strips (sfa_plan.hpp): byte counts of long rows, the budget, slices, input order, and that it is
//      plan_map_slices where no row is long.
//   2. The hand-over rule of sdtw_path_strip_kernel, as a plain C++ model: the band recurrence strip by strip, every strip below
//      the first taking the bottom row of the one above as its boundary (up = top[j], diagonal = top[j - 1], +inf in front of the
//      band), 2-bit moves per strip, one walk through the strips with the pair rules of sdtw_path_walk_kernel.  Its path and
//      pairs must be band_traceback's and path_to_pairs' over the whole query.
// Prints "bytes qlen m strips move_bytes row_bytes" and "model ..." lines for the test to read, "FAIL ..." and exit status 1
// where a check does not hold.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "host/sam.hpp"
#include "sfa_plan.hpp"

static int n_fail = 0;
#define CHECK(cond, ...)            \
    do {                            \
        if (!(cond)) {              \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);    \
            printf("\n");           \
            ++n_fail;               \
        }                           \
    } while (0)

static bool same(const sfa::MapSlices &a, const sfa::MapSlices &b) {
    return a.slice_begin == b.slice_begin && a.order == b.order && a.host_rows == b.host_rows && a.mv_off == b.mv_off;
}

static void planner() {
    for (int qlen : {2049, 4096, 4097})
        for (int32_t m : {1, 5000})
            printf("bytes %d %d %d %lld %lld\n", qlen, m, sfa::map_strip_count(qlen), (long long)sfa::map_long_move_bytes(qlen, m), (long long)sfa::map_long_row_bytes(qlen, m));
    CHECK(sfa::map_strip_count(2048) == 1 && sfa::map_strip_count(2049) == 2 && sfa::map_strip_count(4096) == 2 && sfa::map_strip_count(4097) == 3, "strip counts");
    CHECK(sfa::map_row_bytes_strips(2048, 700) == sfa::map_row_bytes(2048, 700) && sfa::map_row_bytes_strips(25, 30) == sfa::map_row_bytes(25, 30), "short rows keep their bytes");
    {   // a long row alone over the budget goes to the host, the others stay, order kept
        const int32_t q[] = {250, 4097, 3000, 64}, m[] = {300, 5000, 2500, 70};
        const int64_t big = sfa::map_long_row_bytes(4097, 5000);
        sfa::MapSlices s = sfa::plan_map_slices_strips(q, m, 4, big - 1);
        CHECK(s.host_rows == std::vector<int32_t>{1}, "the row over the budget is the host's");
        CHECK((s.order == std::vector<int32_t>{0, 2, 3}), "input order");
        CHECK(s.slice_begin.size() == 2, "one slice");
        CHECK(s.mv_off[1] == sfa::map_row_bytes(250, 300) && s.mv_off[2] == s.mv_off[1] + sfa::map_long_row_bytes(3000, 2500), "offsets count moves and hand-over rows");
        s = sfa::plan_map_slices_strips(q, m, 4, big);
        CHECK(s.host_rows.empty(), "a row that fits exactly is the device's");
        // the hand-over rows count: a budget of the moves alone is too small
        s = sfa::plan_map_slices_strips(q + 1, m + 1, 1, sfa::map_long_move_bytes(4097, 5000));
        CHECK(s.host_rows.size() == 1 && s.order.empty(), "moves alone are not the row's bytes");
    }
    {   // two long rows that do not fit together: two slices
        const int32_t q[] = {3000, 25, 3000, 2100}, m[] = {2500, 30, 2500, 100};
        const int64_t one = sfa::map_long_row_bytes(3000, 2500);
        const sfa::MapSlices s = sfa::plan_map_slices_strips(q, m, 4, 2 * one - 1);
        CHECK((s.slice_begin == std::vector<int32_t>{0, 2, 4}), "two slices");
        CHECK((s.order == std::vector<int32_t>{0, 1, 2, 3}) && s.host_rows.empty(), "all four on the device in input order");
        CHECK((s.mv_off == std::vector<int64_t>{0, one, 0, one}), "offsets restart with the slice");
    }
    {   // no long rows: plan_map_slices
        std::mt19937 rng(5);
        const int lens[] = {7, 25, 64, 65, 250, 300, 513, 1025, 2048, 0};
        for (int it = 0; it < 50; ++it) {
            std::vector<int32_t> q, m;
            for (int k = 0; k < 40; ++k) {
                q.push_back(lens[rng() % 10]);
                m.push_back(static_cast<int32_t>(rng() % 3000) - 10);
            }
            const int64_t budget = static_cast<int64_t>(rng() % 2000000);
            CHECK(same(sfa::plan_map_slices(q.data(), m.data(), 40, budget), sfa::plan_map_slices_strips(q.data(), m.data(), 40, budget)), "short rows, case %d", it);
        }
        // and with long rows the old planner still leaves them to the host
        const int32_t q[] = {250, 2049, 2048}, m[] = {300, 10, 2500};
        const sfa::MapSlices a = sfa::plan_map_slices(q, m, 3, 1 << 30), b = sfa::plan_map_slices_strips(q, m, 3, 1 << 30);
        CHECK(a.host_rows == std::vector<int32_t>{1} && b.host_rows.empty() && (b.order == std::vector<int32_t>{0, 1, 2}), "long row: host without strips, device with them");
    }
}

// ---- the model ----
constexpr int kStrip = 2048;

struct Model {
    std::vector<int32_t> px, py;     // the walk's cells, start -> end (columns of the array)
    std::vector<int32_t> pairs;      // [2 * m], INT32_MIN where the walk wrote nothing
    int32_t first_col = 0;
};

static Model strips_model(const float *x, int32_t n, const float *y, int32_t col_st, int32_t col_end, bool std_dtw) {
    const int32_t m = col_end - col_st + 1;
    const float inf = std::numeric_limits<float>::infinity();
    const int n_strips = (n + kStrip - 1) / kStrip;
    std::vector<std::vector<uint8_t>> moves(n_strips);  // per strip [row in strip][column]
    std::vector<float> hand[2] = {std::vector<float>(m), std::vector<float>(m)};
    std::vector<float> prev(m), cur(m);
    float prefix = 0.0f;
    if (std_dtw && col_st > 0) {
        float acc = std::fabs(x[0] - y[0]);
        for (int32_t j = 1; j < col_st; ++j) acc = std::fabs(x[0] - y[j]) + acc;
        prefix = acc;
    }
    for (int s = 0; s < n_strips; ++s) {
        const int32_t i0 = s * kStrip, rows = std::min(kStrip, n - i0);
        moves[s].assign(static_cast<size_t>(rows) * m, 3);
        const std::vector<float> &top = hand[(s + 1) & 1];  // written by strip s - 1
        for (int32_t r = 0; r < rows; ++r) {
            const float xi = x[i0 + r];
            for (int32_t j = 0; j < m; ++j) {
                float up, diag;
                if (r > 0) {
                    up = prev[j];
                    diag = j > 0 ? prev[j - 1] : inf;
                } else if (s > 0) {
                    up = top[j];
                    diag = j > 0 ? top[j - 1] : inf;
                } else {  // the constant boundary above query row 0
                    up = std_dtw ? inf : 0.0f;
                    diag = j > 0 ? up : inf;
                }
                const float left = j > 0 ? cur[j - 1] : inf;
                float mn = std::fmin(std::fmin(up, diag), left);
                if (std_dtw && s == 0 && r == 0 && j == 0) mn = prefix;
                cur[j] = std::fabs(xi - y[col_st + j]) + mn;
                moves[s][static_cast<size_t>(r) * m + j] = diag == mn ? 0 : (left == mn ? 1 : 2);
            }
            prev.swap(cur);
        }
        if (s + 1 < n_strips) hand[s & 1] = prev;  // bottom row of a full strip
    }
    Model o;
    o.pairs.assign(2 * static_cast<size_t>(m), INT32_MIN);
    int32_t i = n - 1, j = m - 1, last = i;
    std::vector<int32_t> bx{i}, by{j};
    while (i > 0) {
        uint32_t move = 2;
        if (j > 0) move = moves[i / kStrip][static_cast<size_t>(i % kStrip) * m + j];
        if (move == 2) {
            i--;
        } else if (move == 0) {
            o.pairs[2 * j] = i;
            o.pairs[2 * j + 1] = last;
            i--;
            j--;
            last = i;
        } else {
            o.pairs[2 * j] = i == last ? -1 : i + 1;
            o.pairs[2 * j + 1] = i == last ? -1 : last;
            j--;
            last = i;
        }
        bx.push_back(i);
        by.push_back(j);
    }
    o.pairs[2 * j] = 0;
    o.pairs[2 * j + 1] = last;
    o.first_col = j;
    o.px.assign(bx.rbegin(), bx.rend());
    for (size_t k = by.size(); k-- > 0;) o.py.push_back(by[k] + col_st);
    return o;
}

static void hand_over() {
    std::mt19937 rng(11);
    const int32_t rlen = 3000;
    auto level = [&] { return static_cast<float>(static_cast<int>(rng() % 13) - 6) / 4.0f; };  // few values: ties everywhere
    std::vector<float> y(rlen);
    for (float &v : y) v = level();
    const int32_t bands[][2] = {{0, 499}, {2500, rlen - 1}, {1000, 1036}, {0, rlen - 1}};
    for (int32_t n : {2049, 2080, 4096, 4097}) {
        std::vector<float> x(n);
        for (float &v : x) v = level();
        for (int std_dtw = 0; std_dtw < 2; ++std_dtw)
            for (const auto &b : bands) {
                const sfa::WarpPath want = sfa::band_traceback(x.data(), n, y.data(), rlen, b[0], b[1], std_dtw != 0);
                const Model got = strips_model(x.data(), n, y.data(), b[0], b[1], std_dtw != 0);
                const bool path_ok = got.px == want.px && got.py == want.py;
                CHECK(path_ok, "path: n %d std %d band %d..%d", n, std_dtw, b[0], b[1]);
                const std::vector<int32_t> p = sfa::path_to_pairs(want);
                const int32_t f = want.py.front() - b[0], m = b[1] - b[0] + 1;
                bool pairs_ok = got.first_col == f && static_cast<int32_t>(p.size()) == 2 * (m - f);
                for (int32_t k = 0; pairs_ok && k < 2 * m; ++k) pairs_ok = got.pairs[k] == (k < 2 * f ? INT32_MIN : p[k - 2 * f]);
                CHECK(pairs_ok, "pairs: n %d std %d band %d..%d", n, std_dtw, b[0], b[1]);
                // how much of the walk lies below the first strip, and whether it crossed a strip edge diagonally
                int below = 0, diag_cross = 0;
                for (size_t k = 1; k < want.px.size(); ++k) {
                    below += want.px[k] >= kStrip;
                    diag_cross += want.px[k] % kStrip == 0 && want.px[k - 1] == want.px[k] - 1 && want.py[k - 1] == want.py[k] - 1;
                }
                printf("model n %d std %d band %d..%d cells %zu below %d diag_cross %d first_col %d %s\n", n, std_dtw, b[0], b[1], want.px.size(), below, diag_cross, f,
                       path_ok && pairs_ok ? "ok" : "bad");
            }
    }
}

int main() {
    planner();
    hand_over();
    printf("done %d\n", n_fail);
    return n_fail ? 1 : 0;
}
