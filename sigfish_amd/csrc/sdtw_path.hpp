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
};

// One anti-diagonal step of the band fill for the R rows of this lane at reference level yv: dp_step's recurrence, with the
// predecessor choice of its TRACK branch kept as a move instead of a start column.
//   first   std_dtw, the lane holding query row 0, in the first band column: row 0 continues the running sum `prefix` of the
//           columns in front of the band (src/cdtw.c:85-86) instead of its left neighbour
template <int R, bool STD>
__device__ __forceinline__ void path_step(float (&c)[R], float &dprev, const float (&x)[R], const float yv, const bool first,
                                          const float prefix, Exchange &xc, uint32_t (&mv)[R > 16 ? 2 : 1]) {
    float up = xc.shift(c[R - 1]);
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

#define SFA_PATH_SHAPES(X, ...) X(32, 64, __VA_ARGS__) X(32, 32, __VA_ARGS__) X(32, 16, __VA_ARGS__) X(16, 16, __VA_ARGS__) X(8, 16, __VA_ARGS__) X(4, 16, __VA_ARGS__)

#ifdef SFA_DEFINE_PATH_WALK_KERNEL  // plain (non-template) kernel: defined in exactly one translation unit
// path() (src/cdtw.c:98-167) from (qlen - 1, col_end) until query row 0, and path_to_map's rules (src/sigfish.c:530-571) applied
// as every column is left: first and last query row of the column; a column entered without advancing in the query loses that
// first point (and is -1 / -1 when it has no other).  rshift, L: the class's rows per lane (log2) and lanes per row.
__global__ void __launch_bounds__(256) sdtw_path_walk_kernel(const PathArgs a, const int rshift, const int L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_rows) return;
    const PathRow pr = a.rows[k];
    const int W = rshift > 4 ? 2 : 1;
    const uint32_t *mv = a.moves + pr.mv_off;
    int32_t *out = a.pairs + 2 * pr.out_off;
    int i = pr.qlen - 1, j = pr.m - 1;
    int last = i;  // last query row of the column the walk is in
    while (i > 0) {
        uint32_t move = 2;  // first band column: up, as on the host
        if (j > 0) {
            const int g = i >> rshift, r = i & ((1 << rshift) - 1);
            const uint32_t w = mv[(static_cast<int64_t>(j + g) * L + g) * W + (r >> 4)];
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
#endif

}  // namespace sfa
