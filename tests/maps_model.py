"""A plain numpy model of one row's event map (aln_t.r2qevent_map), independent of the library: the band DP of a result row, the
walk back through it and path_to_map, written from the reference's rules as SURVEY.md, DESIGN.md ("Event maps") and the comments
of sigfish_amd/csrc/sdtw_path.hpp state them -- not from host/sam.cpp, which the tests hold against this file.

Everything is float32 and every cell is the two roundings the kernels make, t = |x - y| and t + min(up, diag, left), so costs are
bit-identical and ties break as they do on the device.

  band cost  C over query rows 0 .. qlen-1 x band columns col_st .. col_end of the strand's array y
             row 0            subsequence: |x0 - y[j]| (free start);  --dtw-std: the sequential running sum of |x0 - y[j]| from
                              column 0 OF THE ARRAY, so it carries the columns in front of the band (src/cdtw.c:85-86)
             first column     a cell continues from above only (the column in front of the band does not exist)
             elsewhere        |x_i - y_j| + min(C[i-1][j], C[i-1][j-1], C[i][j-1])                      (src/cdtw.c:184-187)
  walk       from (qlen-1, col_end); at a cell with i > 0: first band column -> up; otherwise diagonal if C[i-1][j-1] is the minimum
             of the three, else left if C[i][j-1] is, else up (src/cdtw.c:134-146); it ends at the first row-0 cell it meets
             (subsequence_path drops the row-0 run in front of it, src/cdtw.c:204-221)
  map        path_to_map (src/sigfish.c:530-571) over the path in forward order: a column's start is the first query row seen in
             it, its stop the last; a point whose query row equals the point's before it blanks its column (a later point of the
             same column starts it again); the first point has no point before it
  no map     the walk reached row 0 behind the first band column: the path has fewer columns than the row claims -> None
"""
import numpy as np

F = np.float32
INF = F(np.inf)


def band_costs(x, y, col_st, col_end, std):
    """The band's cost matrix, filled by anti-diagonals, in a skewed store: S[i + j, i] = C[i][j] (j counted from col_st).
    Cells of a diagonal that lie outside the matrix stay +inf and are never read by cost()."""
    x = np.asarray(x, F)
    y = np.asarray(y, F)
    n, m = len(x), col_end - col_st + 1
    assert n >= 1 and m >= 1 and 0 <= col_st and col_end < len(y)
    yb = y[col_st:col_end + 1]
    S = np.full((n + m - 1, n), INF, F)
    if std:
        row0 = np.cumsum(np.abs(x[0] - y[:col_end + 1]), dtype=F)[col_st:]  # (add.accumulate: sequential, in float32)
    else:
        row0 = np.abs(x[0] - yb)
    S[np.arange(m), 0] = row0
    for d in range(1, n + m - 1):
        lo, hi = max(1, d - m + 1), min(n - 1, d)  # query rows i >= 1 of this diagonal, j = d - i
        if lo > hi:
            continue
        i = np.arange(lo, hi + 1)
        dist = np.abs(x[lo:hi + 1] - yb[d - i])
        up = S[d - 1, lo - 1:hi]
        if hi == d:  # its last cell lies in the first band column: from above only
            best = up.copy()
            if hi > lo:
                best[:-1] = np.minimum(np.minimum(up[:-1], S[d - 2, lo - 1:hi - 1]), S[d - 1, lo:hi])
        else:
            best = np.minimum(np.minimum(up, S[d - 2, lo - 1:hi]), S[d - 1, lo:hi + 1])
        S[d, lo:hi + 1] = dist + best
    return S


def walk(S, n, m):
    """[(query row, band column)] in forward order, from the first row-0 cell the walk back meets to (n - 1, m - 1)"""
    i, j = n - 1, m - 1
    pts = [(i, j)]
    while i > 0:
        if j == 0:
            i -= 1
        else:
            up, diag, left = S[i + j - 1, i - 1], S[i + j - 2, i - 1], S[i + j - 1, i]
            mn = min(up, diag, left)
            if diag == mn:
                i, j = i - 1, j - 1
            elif left == mn:
                j -= 1
            else:
                i -= 1
        pts.append((i, j))
    return pts[::-1]


def path_to_map(pts, m):
    """path_to_map over points whose columns count from the path's first; m pairs"""
    out = np.full((m, 2), -1, np.int32)
    j0 = pts[0][1]
    prev = -1
    for i, j in pts:
        c = j - j0
        if out[c, 0] == -1:
            out[c, 0] = i
        out[c, 1] = i
        if prev == i:
            out[c] = -1
        prev = i
    return out


def band_map(x, y, col_st, col_end, std):
    """The map of the band [col_st, col_end] of array y for the query x (in DP order): int32 [m, 2], or None without a complete map"""
    n, m = len(x), col_end - col_st + 1
    pts = walk(band_costs(x, y, col_st, col_end, std), n, m)
    if pts[0][1] != 0:
        return None
    return path_to_map(pts, m)


def row_columns(pos_st, pos_end, plus, rlen, st_offset):
    """(col_st, col_end) of a result row in columns of its strand's array: the row reports '+' columns shifted by the contig's
    st_offset, and '-' columns flipped about rlen (not rlen - 1) first (src/sigfish.c:971-975)"""
    if plus:
        return pos_st - st_offset, pos_end - st_offset
    return rlen - (pos_end - st_offset), rlen - (pos_st - st_offset)


def row_positions(col_st, col_end, plus, rlen, st_offset):
    """the inverse: (pos_st, pos_end) a row reports for a band"""
    if plus:
        return col_st + st_offset, col_end + st_offset
    return rlen - col_end + st_offset, rlen - col_st + st_offset


def dp_query(events, rna, inv):
    """the query in DP order: direct RNA without --invert is aligned with its events reversed (src/sigfish.c:860-866)"""
    x = np.asarray(events, F)
    return x[::-1].copy() if (rna and not inv) else x


def row_map(row, events, forward, reverse, st_offset, rna, inv, std):
    """The map of a RESULT_DTYPE-like row (fields rid, pos_st, pos_end, strand) of a read whose events are `events`"""
    j, plus = int(row["rid"]), int(row["strand"]) == ord("+")
    y = forward[j] if plus else reverse[j]
    st, en = row_columns(int(row["pos_st"]), int(row["pos_end"]), plus, len(y), int(st_offset[j]))
    return band_map(dp_query(events, rna, inv), y, st, en, std)
