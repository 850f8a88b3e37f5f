// sfa_maps.hip -- sfa_event_maps: the reference-column -> query-event maps (aln_t.r2qevent_map) of rows of the last align call,
// a whole batch at a time on the device (sdtw_path.hpp); and the core it shares with sfa_session_event_maps (sfa_session.hip),
// which takes a device query base, per-row query offsets and lengths, the rows' bands and the scratch of its caller.  Host work: band of every row in columns of its strand's array (the
// flip and offset of src/sigfish.c:971-975 undone, as path_of_row does for the per-read host routine), slices of rows whose move
// matrices fit the scratch budget (sfa_plan.hpp, plan_map_slices), one fill + one walk launch per rows-per-lane class of a
// slice, maps back through page-locked memory.  With the option "map_strips" rows of more than SFA_MAX_QUERY events run in strips
// of 2048 query rows (plan_map_slices_strips; one launch per strip level of a slice, then one walk through the strips).  Rows the
// device does not take -- a move matrix beyond the budget, and without that option queries beyond SFA_MAX_QUERY -- are computed by
// the host routine (band_traceback) inside the same call, from the same resident data.
#include "sfa_ctx.hpp"
#define SFA_DEFINE_PATH_WALK_KERNEL
#include "sdtw_path.hpp"
#include "host/sam.hpp"

#include <map>

using sfa::PathArgs;
using sfa::PathRow;

namespace sfa {
#define SFA_PATH_DECL(RR, LL, SD) extern template __global__ void sdtw_path_fill_kernel<RR, LL, SD>(const PathArgs);
SFA_PATH_SHAPES(SFA_PATH_DECL, false)
SFA_PATH_SHAPES(SFA_PATH_DECL, true)
#undef SFA_PATH_DECL
extern template __global__ void sdtw_path_strip_kernel<false, false>(const PathArgs);
extern template __global__ void sdtw_path_strip_kernel<false, true>(const PathArgs);
extern template __global__ void sdtw_path_strip_kernel<true, false>(const PathArgs);
extern template __global__ void sdtw_path_strip_kernel<true, true>(const PathArgs);
}  // namespace sfa

namespace {

template <bool STD>
void launch_path_fill(int ci, const PathArgs &pa, hipStream_t st) {
    const sfa::ClassShape s = sfa::kClassShapes[ci];
    const int per_block = 4 * (64 / s.lanes);
    const dim3 grid((pa.n_rows + per_block - 1) / per_block), block(256);
    switch (ci) {
#define SFA_PATH_CASE(I, RR, LL)                                                          \
    case I:                                                                               \
        hipLaunchKernelGGL((sfa::sdtw_path_fill_kernel<RR, LL, STD>), grid, block, 0, st, pa); \
        break;
        SFA_PATH_CASE(0, 32, 64) SFA_PATH_CASE(1, 32, 32) SFA_PATH_CASE(2, 32, 16)
        SFA_PATH_CASE(3, 16, 16) SFA_PATH_CASE(4, 8, 16) SFA_PATH_CASE(5, 4, 16)
#undef SFA_PATH_CASE
    }
}

// strip level pa.strip of the long rows of a slice, one row per wave; level 0 starts from the boundary, every other one from the
// row the level before handed over
template <bool STD>
void launch_path_strip(const PathArgs &pa, hipStream_t st) {
    const dim3 grid((pa.n_rows + 3) / 4), block(256);
    if (pa.strip == 0)
        hipLaunchKernelGGL((sfa::sdtw_path_strip_kernel<STD, false>), grid, block, 0, st, pa);
    else
        hipLaunchKernelGGL((sfa::sdtw_path_strip_kernel<STD, true>), grid, block, 0, st, pa);
}

}  // namespace

namespace sfa {

int map_row_band(const sfa_ctx *c, const sfa_result_t &r, int32_t k, int64_t ql, int64_t gap, const char *who, const char *what, MapRow *b) {
    const int strands = (c->flag & SFA_RNA) ? 1 : 2;
    if (r.rid >= c->model.num_ref || (r.strand != '+' && r.strand != '-') || (strands == 1 && r.strand != '+'))
        return fail(SFA_EINVAL, "%s: row %d (contig %d, strand %d) is not a row of this reference", who, k, r.rid, (int)r.strand);
    b->k = k;
    b->job = r.rid * strands + (r.strand == '+' ? 0 : 1);
    const int32_t rlen = c->model.h_job_len[b->job], off = c->model.h_ref_off[r.rid];
    const bool plus = r.strand == '+';
    const int64_t st = plus ? static_cast<int64_t>(r.pos_st) - off : static_cast<int64_t>(rlen) - (static_cast<int64_t>(r.pos_end) - off);
    const int64_t en = plus ? static_cast<int64_t>(r.pos_end) - off : static_cast<int64_t>(rlen) - (static_cast<int64_t>(r.pos_st) - off);
    if (st < 0 || en < st || en >= rlen || ql <= 0)
        return fail(SFA_EINVAL, "%s: row %d (columns %d..%d of contig %d, %lld events) is not a row of %s", who, k, r.pos_st, r.pos_end, r.rid, (long long)ql, what);
    const int64_t need = en - st + 1;
    if (gap < need) return fail(SFA_ERANGE, "%s: row %d needs %lld pairs, map_off leaves %lld", who, k, (long long)need, (long long)gap);
    b->col_st = static_cast<int32_t>(st);
    b->m = static_cast<int32_t>(need);
    b->qlen = static_cast<int32_t>(std::min<int64_t>(ql, INT32_MAX));
    return SFA_OK;
}

int event_maps_core(sfa_ctx *c, ctx::MapScratch &sc, const float *d_queries, const int64_t *q_off, size_t n_q_off, bool reversed, const MapRow *band, int32_t n_idx,
                    const int64_t *map_off, int32_t *pairs, int32_t *n_on_host) {
    const bool std_dtw = (c->flag & SFA_DTW) != 0;
    std::vector<int32_t> qlen(n_idx), m(n_idx);
    for (int32_t t = 0; t < n_idx; ++t) qlen[t] = band[t].qlen, m[t] = band[t].m;
    const sfa::MapSlices ms = c->opt_map_strips ? sfa::plan_map_slices_strips(qlen.data(), m.data(), n_idx, c->opt_map_scratch)
                                                : sfa::plan_map_slices(qlen.data(), m.data(), n_idx, c->opt_map_scratch);
    hipStream_t st = c->stream;
    // the query offsets of the call live in the staging area of its launches only; the walks need them again
    std::vector<PathRow> prow;
    std::vector<int32_t> t_of;  // position in prow -> t
    for (size_t s = 0; s + 1 < ms.slice_begin.size(); ++s) {
        const int32_t lo = ms.slice_begin[s], hi = ms.slice_begin[s + 1];
        // rows of the slice by class (long first, as the fill runs them), input order inside a class; in front of the six classes
        // the rows beyond kMaxQuery events ("map_strips"; class_for gives -1), which run in row strips
        prow.clear();
        t_of.clear();
        int32_t cls_store[8], *const cls_begin = cls_store + 1;
        int64_t out_pairs = 0, mv_bytes = 0;
        int32_t strip_levels = 0;
        for (int ci = -1; ci < 6; ++ci) {
            cls_begin[ci] = static_cast<int32_t>(prow.size());
            for (int32_t o = lo; o < hi; ++o) {
                const int32_t t = ms.order[o];
                const MapRow &b = band[t];
                if (sfa::class_for(b.qlen) != ci) continue;
                PathRow p{};
                p.mv_off = ms.mv_off[o] / 4;
                p.out_off = out_pairs;
                p.read = b.query;
                p.job = b.job;
                p.col_st = b.col_st;
                p.m = b.m;
                p.qlen = b.qlen;
                out_pairs += b.m;
                mv_bytes = std::max(mv_bytes, ms.mv_off[o] + sfa::map_row_bytes_strips(b.qlen, b.m));
                if (ci < 0) strip_levels = std::max(strip_levels, sfa::map_strip_count(b.qlen));
                prow.push_back(p);
                t_of.push_back(t);
            }
        }
        cls_begin[6] = static_cast<int32_t>(prow.size());
        const int32_t n = cls_begin[6];
        int rc;
        const size_t qoff_bytes = sizeof(int64_t) * n_q_off;
        if ((rc = sc.reserve(static_cast<size_t>(mv_bytes), sizeof(PathRow) * n + qoff_bytes + 8, static_cast<size_t>(n), static_cast<size_t>(out_pairs)))) return rc;
        static_assert(sizeof(PathRow) % 8 == 0, "the query offsets follow the rows in one buffer");
        int64_t *d_qoff = reinterpret_cast<int64_t *>(sc.d_prow.as<char>() + sizeof(PathRow) * n);
        HIP_TRY(hipMemcpyAsync(sc.d_prow.p, prow.data(), sizeof(PathRow) * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_qoff, q_off, qoff_bytes, hipMemcpyHostToDevice, st));
        for (int ci = -1; ci < 6; ++ci) {
            const int32_t nc = cls_begin[ci + 1] - cls_begin[ci];
            if (nc == 0) continue;
            PathArgs pa{};
            pa.queries = d_queries;
            pa.q_off = d_qoff;
            pa.ref = c->model.d_ref.as<float>();
            pa.job_off = c->model.d_job_off.as<int64_t>();
            pa.rows = sc.d_prow.as<PathRow>() + cls_begin[ci];
            pa.moves = sc.d_mv.as<uint32_t>();
            pa.pairs = sc.d_pairs.as<int32_t>();
            pa.first_col = sc.d_pfirst.as<int32_t>() + cls_begin[ci];
            pa.n_rows = nc;
            pa.rev_query = reversed ? 1 : 0;
            if (ci < 0) {  // one launch per strip level; a level reads what the one before handed over, in stream order
                for (pa.strip = 0; pa.strip < strip_levels; ++pa.strip) {
                    if (std_dtw)
                        launch_path_strip<true>(pa, st);
                    else
                        launch_path_strip<false>(pa, st);
                    KERNEL_TRY();
                }
                hipLaunchKernelGGL(sfa::sdtw_path_walk_strips_kernel, dim3((nc + 255) / 256), dim3(256), 0, st, pa);
                KERNEL_TRY();
                continue;
            }
            if (std_dtw)
                launch_path_fill<true>(ci, pa, st);
            else
                launch_path_fill<false>(ci, pa, st);
            KERNEL_TRY();
            const sfa::ClassShape sh = sfa::kClassShapes[ci];
            const int rshift = sh.R == 32 ? 5 : (sh.R == 16 ? 4 : (sh.R == 8 ? 3 : 2));
            hipLaunchKernelGGL(sfa::sdtw_path_walk_kernel, dim3((nc + 255) / 256), dim3(256), 0, st, pa, rshift, sh.lanes);
            KERNEL_TRY();
        }
        int32_t *h_pairs = sc.h_pairs.as<int32_t>();
        int32_t *h_first = h_pairs + 2 * out_pairs;
        HIP_TRY(hipMemcpyAsync(h_pairs, sc.d_pairs.p, 8 * static_cast<size_t>(out_pairs), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_first, sc.d_pfirst.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int32_t i = 0; i < n; ++i) {
            // a walk that met query row 0 behind the row's first column has no complete map; like sfa_r2qevent_map, nothing is written
            if (h_first[i] != 0) continue;
            memcpy(pairs + 2 * map_off[band[t_of[i]].k], h_pairs + 2 * prow[i].out_off, 8 * static_cast<size_t>(prow[i].m));
        }
    }
    // rows left to the host routine: query and (contig,strand) array come back from the device
    std::map<int32_t, std::vector<float>> ref_of_job;
    std::vector<float> q, qdp;
    for (const int32_t t : ms.host_rows) {
        const MapRow &b = band[t];
        const int64_t ql = b.qlen;
        q.resize(static_cast<size_t>(ql));
        qdp.resize(static_cast<size_t>(ql));
        HIP_TRY(hipMemcpy(q.data(), d_queries + q_off[b.query], sizeof(float) * static_cast<size_t>(ql), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < ql; ++j) qdp[reversed ? ql - 1 - j : j] = q[j];
        std::vector<float> &y = ref_of_job[b.job];
        const int32_t rlen = c->model.h_job_len[b.job];
        if (y.empty()) {
            y.resize(static_cast<size_t>(rlen));
            HIP_TRY(hipMemcpy(y.data(), c->model.d_ref.as<float>() + c->model.h_job_off[b.job], sizeof(float) * static_cast<size_t>(rlen), hipMemcpyDeviceToHost));
        }
        const sfa::WarpPath path = sfa::band_traceback(qdp.data(), static_cast<int32_t>(ql), y.data(), rlen, b.col_st, b.col_st + b.m - 1, std_dtw);
        if (path.px.empty()) continue;
        const std::vector<int32_t> p = sfa::path_to_pairs(path);
        if (static_cast<int32_t>(p.size() / 2) != b.m) continue;  // (sfa_r2qevent_map: SFA_EINVAL, nothing written)
        memcpy(pairs + 2 * map_off[b.k], p.data(), sizeof(int32_t) * p.size());
    }
    if (n_on_host) *n_on_host = static_cast<int32_t>(ms.host_rows.size());
    return SFA_OK;
}

}  // namespace sfa

namespace {

// sfa_event_maps on one device: what is about the context's last batch -- where its queries lie, the host copy of their offsets,
// which read a row names -- in front of the core.  Rows idx[0..n_idx) (caller's numbering; nullptr: 0..n_idx-1); reads are
// numbered from read_base
int event_maps_one(sfa_ctx *c, const sfa_result_t *rows, const int32_t *read_of_row, const int32_t *idx, int32_t n_idx, int32_t read_base,
                   const int64_t *map_off, int32_t *pairs, int32_t *n_on_host) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = sfa::resolve_profile(c)) return rc;
    if (c->maps.map_n < 0) return fail(SFA_EINVAL, "sfa_event_maps: no align call has completed on this context");
    if (c->maps.map_n > 0 && c->maps.map_queries != c->io.d_queries.as<float>())
        return fail(SFA_EINVAL, "sfa_event_maps: the last call was sfa_align_batch_device, whose queries are the caller's; the context kept none");
    const bool reversed = (c->flag & SFA_RNA) && !(c->flag & SFA_INV);  // src/sigfish.c:860-866
    std::vector<sfa::MapRow> band(n_idx);
    for (int32_t t = 0; t < n_idx; ++t) {
        const int32_t k = idx ? idx[t] : t;
        band[t].k = k;
        const sfa_result_t &r = rows[k];
        if (!r.valid || r.rid < 0) continue;  // unaligned: nothing is written
        const int64_t read = static_cast<int64_t>(read_of_row ? read_of_row[k] : k) - read_base;
        if (read < 0 || read >= c->maps.map_n) return fail(SFA_EINVAL, "sfa_event_maps: row %d names read %lld, the last call had %d", k, (long long)(read + read_base), c->maps.map_n);
        if (int rc = sfa::map_row_band(c, r, k, c->maps.map_q_off[read + 1] - c->maps.map_q_off[read], map_off[k + 1] - map_off[k], "sfa_event_maps", "the last call", &band[t])) return rc;
        band[t].query = static_cast<int32_t>(read);
    }
    return sfa::event_maps_core(c, c->maps, c->maps.map_queries, c->maps.map_q_off.data(), static_cast<size_t>(c->maps.map_n) + 1, reversed, band.data(), n_idx, map_off, pairs,
                                n_on_host);
}

}  // namespace

extern "C" int sfa_event_maps(sfa_ctx_t *c, const sfa_result_t *rows, const int32_t *read_of_row, int32_t n_rows, const int64_t *map_off,
                              int32_t *pairs, int32_t *n_on_host) {
    if (!c || n_rows < 0 || (n_rows > 0 && (!rows || !map_off || !pairs))) return fail(SFA_EINVAL, "sfa_event_maps: bad argument");
    if (n_on_host) *n_on_host = 0;
    for (int32_t k = 0; k < n_rows; ++k)
        if (map_off[k + 1] < map_off[k] || map_off[k] < 0) return fail(SFA_EINVAL, "sfa_event_maps: map_off not monotone at row %d", k);
    if (c->shards.empty()) {
        if (!read_of_row && c->maps.map_n >= 0 && n_rows != c->maps.map_n)
            return fail(SFA_EINVAL, "sfa_event_maps: the last call aligned %d reads, %d rows given without read_of_row", c->maps.map_n, n_rows);
        return event_maps_one(c, rows, read_of_row, nullptr, n_rows, 0, map_off, pairs, n_on_host);
    }
    const int32_t n_reads = c->maps.map_n;
    if (n_reads < 0) return fail(SFA_EINVAL, "sfa_event_maps: no align call has completed on this context");
    if (!read_of_row && n_rows != n_reads)
        return fail(SFA_EINVAL, "sfa_event_maps: the last call aligned %d reads, %d rows given without read_of_row", n_reads, n_rows);
    // every entry point splits a call the same way (shard_ranges): shard r holds the queries of reads [lo_r, hi_r)
    const size_t G = c->shards.size();
    std::vector<int32_t> lo;
    sfa::shard_ranges(n_reads, G, &lo);
    std::vector<std::vector<int32_t>> idx(G);
    for (int32_t k = 0; k < n_rows; ++k) {
        const int32_t read = read_of_row ? read_of_row[k] : k;
        if (!rows[k].valid || rows[k].rid < 0) continue;
        if (read < 0 || read >= n_reads) return fail(SFA_EINVAL, "sfa_event_maps: row %d names read %d, the last call had %d", k, read, n_reads);
        const size_t r = std::upper_bound(lo.begin(), lo.end(), read) - lo.begin() - 1;
        idx[r].push_back(k);
    }
    std::vector<int32_t> on_host(G, 0);
    const int rc = sfa::for_each_shard_range(c, n_reads, [&](size_t r, int32_t a, int32_t) {
        if (idx[r].empty()) return static_cast<int>(SFA_OK);
        return event_maps_one(c->shards[r], rows, read_of_row, idx[r].data(), static_cast<int32_t>(idx[r].size()), a, map_off, pairs, &on_host[r]);
    });
    if (!rc && n_on_host)
        for (int32_t v : on_host) *n_on_host += v;
    return rc;
}
