// sdtw_path.hpp -- the warp paths of a batch's result rows on the device: aln_t.r2qevent_map (path_to_map, src/sigfish.c:530-571)
// for every requested row, behind sfa_event_maps.  Device twin of band_traceback + path_to_pairs (host/sam.cpp); the host keeps
// both for rows the device leaves to it (queries beyond SFA_MAX_QUERY, a move matrix beyond the scratch budget).
//
// Two launches per rows-per-lane class of a slice of rows:
//   sdtw_path_fill_kernel   re-fills the band [col_st, col_end] x qlen of every row with the recurrence of the fill, in the fill's
//                           lane layout (R query rows per lane, L lanes per row, 64 / L rows per wave, anti-diagonal steps, the
//                           lane above handing its bottom cost down through Exchange), and stores the predecessor of every cell
//                           as a 2-bit move: 0 diagonal, 1 left, 2 up -- the order path() tries them in (src/cdtw.c:134-146).
//                           One record per (step, lane): the lane's R moves of that step's column in one 32-bit word (R <= 16,
//                           row r in bits 2r, 2r+1) or two (R = 32).  Records are laid out BY STEP, [step][lane][word], so the 64
//                           lanes of a wave store one contiguous piece per step; cell (i, j) is found at step j + i / R, lane i / R.
//   sdtw_path_walk_kernel   one lane per row walks back from (qlen - 1, col_end) to query row 0 through the moves and writes the
//                           (start, stop) pair of every column as it leaves it.
// Costs are bit-identical to the host's (same operands, |x - y| + min3, no contraction): only then do ties break identically.
// Columns outside the band read +inf as reference level, which makes their cells +inf: the first band column then continues
// from above only, as on the host.
#pragma once
#include "sdtw_kernels.hpp"
#include "sfa_plan.hpp"  // kStripRows

namespace sfa {

struct PathRow {
    int64_t mv_off;   // 32-bit word offset of the row's move records in the slice's scratch
    int64_t out_off;  // offset of its map in the slice's output, in pairs
    int32_t read;     // read of the last call whose query this row aligns
    int32_t job;      // (contig, strand) array
    int32_t col_st;   // first band column, in columns of that array
    int32_t m;        // band columns
    int32_t qlen;
    int32_t pad;
};

struct PathArgs {
    const float *queries;    // the last call's, still resident
    const int64_t *q_off;    // [n_reads + 1]
    const float *ref;        // padded reference event arrays
    const int64_t *job_off;  // [n_jobs]
    const PathRow *rows;     // rows of this launch (one class)
    uint32_t *moves;         // scratch of the slice
    int32_t *pairs;          // maps of the slice, 2 ints per column
    int32_t *first_col;      // [n_rows] band column in which the walk reached query row 0 (0 for a row whose map is complete)
    int32_t n_rows;
    int32_t rev_query;       // 1: query rows are the events reversed (RNA without --invert)
    int32_t strip;           // the strip kernels: the strip level of this launch (query rows strip * 2048 ...)
};

// One anti-diagonal step of the band fill for the R rows of this lane at reference level yv: dp_step's recurrence, with the
// predecessor choice of its TRACK branch kept as a move instead of a start column.
//   first   std_dtw, the lane holding query row 0, in the first band column: row 0 continues the running sum `prefix` of the
//           columns in front of the band (src/cdtw.c:85-86) instead of its left neighbour
//   TOP     the rows of this wave are a strip below query row 0: the lane holding the strip's first row (top_lane) takes the cost
//           above it from `top`, the row the strip before handed over, instead of the boundary word
template <int R, bool STD, bool TOP = false>
__device__ __forceinline__ void path_step(float (&c)[R], float &dprev, const float (&x)[R], const float yv, const bool first,
                                          const float prefix, Exchange &xc, uint32_t (&mv)[R > 16 ? 2 : 1], const bool top_lane = false,
                                          const float top = 0.0f) {
    float up = xc.shift(c[R - 1]);
    if (TOP) up = top_lane ? top : up;
    float diag = dprev;
    dprev = up;
    mv[0] = 0;
    if (R > 16) mv[R > 16 ? 1 : 0] = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float left = c[r];
        float m = fminf(fminf(up, diag), left);
        if (STD && r == 0) m = first ? prefix : m;
        const float cn = fabsf(x[r] - yv) + m;
        // traceback order of path(): diagonal first, then left, then up
        const uint32_t move = (diag == m) ? 0u : ((left == m) ? 1u : 2u);
        mv[r >> 4] |= move << (2 * (r & 15));
        diag = left;
        up = cn;
        c[r] = cn;
    }
}

template <int R, int L, bool STD>
__global__ void __launch_bounds__(256) sdtw_path_fill_kernel(const PathArgs a) {
    constexpr int S = 64 / L;           // rows per wave
    constexpr int W = R > 16 ? 2 : 1;   // words per record
    __shared__ float lds_f[4 * kXchWordsPerWave];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int slot = lane / L, g = lane % L;
    const int k = (blockIdx.x * 4 + wib) * S + slot;
    const bool live = k < a.n_rows;
    PathRow pr{};
    if (live) pr = a.rows[k];
    const int m = live ? pr.m : 0;
    const bool lane0 = g == 0;
    Exchange xc;
    xc.init(lds_f, reinterpret_cast<int *>(lds_f), wib, slot, g, L);
    // boundary above query row 0: 0 = free start of subsequence(); std_dtw(): row 0 only continues along itself
    xc.set_boundary<false>(lane0, STD ? INFINITY : 0.0f);
    float x[R], c[R];
    {
        const float *q = a.queries + a.q_off[live ? pr.read : 0];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = g * R + r;
            const int src = a.rev_query ? (pr.qlen - 1 - i) : i;
            x[r] = (live && i < pr.qlen) ? q[src] : 0.0f;
            c[r] = INFINITY;
        }
    }
    const float *ybase = a.ref + (live ? a.job_off[pr.job] : 0);
    const float *yp = ybase + pr.col_st;
    float prefix = 0.0f;
    if (STD && live && lane0 && pr.col_st > 0) {  // sequential fp32 running sum of row 0 from column 0 of the array
        float acc = fabsf(x[0] - ybase[0]);
        for (int j = 1; j < pr.col_st; ++j) acc = fabsf(x[0] - ybase[j]) + acc;
        prefix = acc;
    }
    // steps of the wave: its widest band + the lanes' skew
    int mmax = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) mmax = max(mmax, __shfl(m, s * L));
    const int n_steps = __builtin_amdgcn_readfirstlane(mmax > 0 ? mmax + L - 1 : 0);
    const int mlast = m > 0 ? m - 1 : 0;
    auto load4 = [&](const int t0, float(&y)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = t0 + u - g;
            const float v = yp[min(max(j, 0), mlast)];  // (always inside the band, or word 0 of the arrays for an idle slot)
            y[u] = (j >= 0 && j < m) ? v : INFINITY;
        }
    };
    uint32_t *rec = a.moves + pr.mv_off + static_cast<int64_t>(g) * W;
    float dprev = INFINITY;
    float ycur[4], ynext[4];
    load4(0, ycur);
    for (int t0 = 0; t0 < n_steps; t0 += 4) {
        load4(t0 + 4, ynext);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u, j = t - g;
            uint32_t mv[W];
            path_step<R, STD>(c, dprev, x, ycur[u], STD && lane0 && j == 0, prefix, xc, mv);
            if (j >= 0 && j < m) {  // record t of this row: t <= m - 1 + g < m + L - 1
                uint32_t *p = rec + static_cast<int64_t>(t) * (L * W);
                if (W == 2)
                    *reinterpret_cast<uint2 *>(p) = make_uint2(mv[0], mv[W - 1]);
                else
                    *p = mv[0];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) ycur[u] = ynext[u];
    }
}

// ---- rows of more than 2048 events: the band fill in strips of 2048 query rows (the "map_strips" option) ----
// One launch per strip level s covers every long row of the slice that has a strip s; launches follow each other on one stream and
// that order is the only dependency.  A strip is the 32 x 64 shape, one row per wave: query rows s * 2048 + 32 g + r.  Its moves are
// the row's records s * (m + 63) ... in the layout above.  Behind the moves of all strips lie two hand-over rows of m floats:
// lane 63 of a full strip stores the cost of its bottom row (query row s * 2048 + 2047) at every band column into row s & 1, lane 0
// of the strip below reads row (s - 1) & 1 four columns ahead: `up` of band column j is top[j], the diagonal top[j - 1] (the `up`
// of the step before, +inf at j = 0: the column in front of the band is +inf on the host too).  std_dtw's prefix rule is strip 0's.
__device__ __forceinline__ int64_t path_strip_words(const int m) { return (static_cast<int64_t>(m) + 63) * 128; }

template <bool STD, bool TOP>
__global__ void __launch_bounds__(256) sdtw_path_strip_kernel(const PathArgs a) {
    constexpr int R = 32, L = 64, W = 2;
    __shared__ float lds_f[4 * kXchWordsPerWave];
    const int g = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wib;
    if (k >= a.n_rows) return;  // (whole waves; the kernel has no block-wide barrier)
    const PathRow pr = a.rows[k];
    const int n_strips = (pr.qlen + kStripRows - 1) / kStripRows;
    const int s = TOP ? a.strip : 0;
    if (s >= n_strips) return;
    const int m = pr.m;
    const bool lane0 = g == 0;
    Exchange xc;
    xc.init(lds_f, reinterpret_cast<int *>(lds_f), wib, 0, g, L);
    xc.set_boundary<false>(lane0, STD ? INFINITY : 0.0f);  // (strip 0; below it lane 0 never uses the word)
    float x[R], c[R];
    {
        const float *q = a.queries + a.q_off[pr.read];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = s * kStripRows + g * R + r;
            const int src = a.rev_query ? (pr.qlen - 1 - i) : i;
            x[r] = i < pr.qlen ? q[src] : 0.0f;
            c[r] = INFINITY;
        }
    }
    const float *ybase = a.ref + a.job_off[pr.job];
    const float *yp = ybase + pr.col_st;
    float prefix = 0.0f;
    if (STD && !TOP && lane0 && pr.col_st > 0) {
        float acc = fabsf(x[0] - ybase[0]);
        for (int j = 1; j < pr.col_st; ++j) acc = fabsf(x[0] - ybase[j]) + acc;
        prefix = acc;
    }
    uint32_t *row_mv = a.moves + pr.mv_off;
    float *hand = reinterpret_cast<float *>(row_mv + n_strips * path_strip_words(m));
    const float *top_in = hand + ((s + 1) & 1) * static_cast<int64_t>(m);  // row (s - 1) & 1
    float *top_out = hand + (s & 1) * static_cast<int64_t>(m);
    const bool hands_over = s + 1 < n_strips && g == L - 1;  // a strip with a strip below it is full: its bottom row is lane 63's c[31]
    const int n_steps = m + L - 1;
    const int mlast = m - 1;
    auto load4 = [&](const int t0, float(&y)[4], float(&tp)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = t0 + u - g;
            const int jc = min(max(j, 0), mlast);
            const float v = yp[jc];
            y[u] = (j >= 0 && j < m) ? v : INFINITY;
            if (TOP) {
                const float tv = lane0 ? top_in[jc] : 0.0f;
                tp[u] = j < m ? tv : INFINITY;
            }
        }
    };
    uint32_t *rec = row_mv + s * path_strip_words(m) + static_cast<int64_t>(g) * W;
    float dprev = INFINITY;
    float ycur[4], ynext[4], tcur[4] = {0.0f, 0.0f, 0.0f, 0.0f}, tnext[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4(0, ycur, tcur);
    for (int t0 = 0; t0 < n_steps; t0 += 4) {
        load4(t0 + 4, ynext, tnext);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u, j = t - g;
            uint32_t mv[W];
            path_step<R, STD, TOP>(c, dprev, x, ycur[u], STD && !TOP && lane0 && j == 0, prefix, xc, mv, lane0, tcur[u]);
            if (j >= 0 && j < m) {
                *reinterpret_cast<uint2 *>(rec + static_cast<int64_t>(t) * (L * W)) = make_uint2(mv[0], mv[1]);
                if (hands_over) top_out[j] = c[R - 1];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) ycur[u] = ynext[u], tcur[u] = tnext[u];
    }
}

#define SFA_PATH_SHAPES(X, ...) X(32, 64, __VA_ARGS__) X(32, 32, __VA_ARGS__) X(32, 16, __VA_ARGS__) X(16, 16, __VA_ARGS__) X(8, 16, __VA_ARGS__) X(4, 16, __VA_ARGS__)

#ifdef SFA_DEFINE_PATH_WALK_KERNEL  // plain (non-template) kernel: defined in exactly one translation unit
// path() (src/cdtw.c:98-167) from (qlen - 1, col_end) until query row 0, and path_to_map's rules (src/sigfish.c:530-571) applied
// as every column is left: first and last query row of the column; a column entered without advancing in the query loses that
// first point (and is -1 / -1 when it has no other).  rshift, L: the class's rows per lane (log2) and lanes per row.
// STRIPS: a row of more than 2048 events, filled by sdtw_path_strip_kernel: query row i lies in strip i >> 11, whose records are
// found as above from i & 2047; a move out of a strip's first row simply continues in the strip above.
template <bool STRIPS>
__device__ __forceinline__ void path_walk(const PathArgs &a, const int rshift, const int L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_rows) return;
    const PathRow pr = a.rows[k];
    const int W = rshift > 4 ? 2 : 1;
    const uint32_t *mv = a.moves + pr.mv_off;
    const int64_t strip_words = STRIPS ? path_strip_words(pr.m) : 0;
    int32_t *out = a.pairs + 2 * pr.out_off;
    int i = pr.qlen - 1, j = pr.m - 1;
    int last = i;  // last query row of the column the walk is in
    while (i > 0) {
        uint32_t move = 2;  // first band column: up, as on the host
        if (j > 0) {
            const int il = STRIPS ? (i & (kStripRows - 1)) : i;
            const int g = il >> rshift, r = il & ((1 << rshift) - 1);
            const uint32_t w = mv[(STRIPS ? (i / kStripRows) * strip_words : 0) + (static_cast<int64_t>(j + g) * L + g) * W + (r >> 4)];
            move = (w >> (2 * (r & 15))) & 3u;
        }
        if (move == 2) {
            i--;
        } else if (move == 0) {
            out[2 * j] = i;
            out[2 * j + 1] = last;
            i--;
            j--;
            last = i;
        } else {
            out[2 * j] = i == last ? -1 : i + 1;
            out[2 * j + 1] = i == last ? -1 : last;
            j--;
            last = i;
        }
    }
    out[2 * j] = 0;  // the path's first column is never blanked
    out[2 * j + 1] = last;
    a.first_col[k] = j;
}

__global__ void __launch_bounds__(256) sdtw_path_walk_kernel(const PathArgs a, const int rshift, const int L) { path_walk<false>(a, rshift, L); }
__global__ void __launch_bounds__(256) sdtw_path_walk_strips_kernel(const PathArgs a) { path_walk<true>(a, 5, 64); }
#endif

}  // namespace sfa
