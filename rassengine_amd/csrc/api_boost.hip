// api_boost.hip — the C ABI of include/rass_engine.h: the boosted search rass_index_search_boosted(_device) (exact top-k of
// boost * T(cos) + a per-row bonus column) and the builders of its columns: rass_index_bonus_scatter(_device),
// rass_index_bonus_from_attr_clauses, rass_index_bonus_mask.  Host-side C++ only: the kernels are scan_boost.hip and bonus.hip;
// the merge and the store of a pass are the allow-list search's (merge_topk.hip, allow.hip).  The pass driver
// (boost_device_group), the argument checks and the host and device group loops (boost_search_host / boost_search_device) also
// serve the function-score search (api_fscore.hip, scan_fscore.hip).  The objects and the threading rules: api_internal.h.

#include <cmath>
#include <tuple>

#include "api_internal.h"

namespace rass {
namespace host {

// One launch group of a boosted or a function-score search: api_internal.h.
int boost_device_group(rass_index* idx, const BoostRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    // the scan reports slab rows (the continuation bound names rows): the store translates them
    const IndexView iv = index_view(idx, r.q_filter != nullptr, 0, /*continued=*/true);
    const int64_t stride = idx->stride;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (scratch_layout(nullptr, RASS_MAX_QBATCH, RASS_MAX_K).total > eng->scratch_bytes)
        return fail(RASS_ERR_INVALID, "scan workspace too small");
    if (r.combine >= 0 && r.bonus_rows != iv.rows)
        return fail(RASS_ERR_INVALID, "the function column covers " + std::to_string(r.bonus_rows) + " rows, the index holds " +
                                          std::to_string(iv.rows) + ": fn_rows must equal the index's rows");
    if (iv.rows == 0) {   // nothing to scan: the empty answer
        HIP_TRY(rass::launch_fill_i32(reinterpret_cast<int32_t*>(r.out_scores), (int64_t)nq * k, (int32_t)0xff800000u, st));
        HIP_TRY(hipMemsetAsync(r.out_ids, 0xff, (size_t)nq * k * sizeof(int64_t), st));
        return RASS_OK;
    }
    const int64_t bonus_bytes = ((r.q_stride > 0 ? (int64_t)(nq - 1) * r.q_stride : 0) + r.bonus_rows) * 4;
    if (bonus_bytes > rass::kBoostMaxBonusBytes)
        return fail(RASS_ERR_INVALID, "a launch group's bonus columns exceed 2 GiB: use fewer rows per column or a shared column");
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, RASS_MAX_QBATCH));
    for (int kdone = 0; kdone < k;) {
        const int kk = std::min(RASS_MAX_K, k - kdone);
        const int grid = scan_grid((iv.rows + 31) / 32, kk, eng->n_cus);
        rass::BoostArgs a;
        a.scan.corpus = iv.corpus;
        a.scan.row_tag = iv.row_tag;
        a.scan.q_padded = L.q_padded;
        a.scan.q_filter = r.q_filter;
        a.scan.q_filter_mask = r.q_filter_mask;
        a.scan.q_after_score = kdone > 0 ? eng->d_after_s : nullptr;
        a.scan.q_after_id = kdone > 0 ? eng->d_after_i : nullptr;
        a.scan.part_scores = L.part_scores;
        a.scan.part_ids = L.part_ids;
        a.scan.row_stride = stride;
        a.scan.id_base = 0;
        a.scan.n_rows = (int)iv.rows;
        a.scan.nq = nq;
        a.scan.k = kk;
        a.bonus = r.bonus;
        a.bonus_q_stride = r.q_stride;
        a.bonus_rows = r.bonus_rows;
        a.bonus_bytes = (unsigned)bonus_bytes;
        a.transform = r.transform;
        a.boost = r.boost;
        int rc;
        if (r.combine >= 0) {
            rass::FscoreArgs f;
            f.scan = a.scan;
            f.fn = r.bonus, f.fn_q_stride = r.q_stride, f.fn_rows = r.bonus_rows, f.fn_bytes = (unsigned)bonus_bytes;
            f.transform = r.transform, f.mode = r.combine, f.boost = r.boost, f.min_score = r.min_score;
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_fscore_f32(f, grid, st)); });
        } else {
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_boost_f32(a, grid, st)); });
        }
        if (rc != RASS_OK) return rc;
        HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, kk, L.cand_scores, L.cand_ids, st));
        HIP_TRY(rass::launch_allow_store(L.cand_scores, L.cand_ids, nq, kk, k, kdone, iv.id_map ? 0 : r.id_base, iv.id_map, r.out_scores,
                                         r.out_ids, eng->d_after_s, eng->d_after_i, st));
        kdone += kk;
    }
    return RASS_OK;
}

namespace {

// Launch group [done, done + r.nq) of the call `c` (device pointers): its slice of every per-query array, its column(s).
BoostRequest group_of(const BoostRequest& c, int done, int dim, int n_cols, int64_t col_stride) {
    const bool shared = n_cols == 1;
    BoostRequest r = c;
    r.queries = c.queries + (int64_t)done * dim, r.nq = std::min(RASS_MAX_QBATCH, c.nq - done);
    r.boost = c.boost ? c.boost + done : nullptr, r.min_score = c.min_score ? c.min_score + done : nullptr;
    r.bonus = c.bonus + (shared ? 0 : (int64_t)done * col_stride), r.q_stride = shared ? 0 : col_stride;
    r.q_filter = c.q_filter ? c.q_filter + done : nullptr, r.q_filter_mask = c.q_filter_mask ? c.q_filter_mask + done : nullptr;
    r.out_scores = c.out_scores + (int64_t)done * c.k, r.out_ids = c.out_ids + (int64_t)done * c.k;
    return r;
}

// The argument checks the entry points share (everything that does not need the row count: fn_rows == the index's rows is
// checked by boost_device_group under the engine's lock, before a group's first launch).
int check_boosted(const rass_index* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored) {
    const char *col = scored ? "fn" : "bonus", *who = scored ? "function-score" : "boosted";   // the words of the messages
    if (!idx || !c.out_scores || !c.out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (c.nq > 0 && !c.queries) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (c.nq < 0 || c.nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [0, RASS_MAX_DEVICE_BATCH]");
    if (c.k < 1 || c.k > RASS_MAX_K_MULTIPASS) return fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K_MULTIPASS]");
    if (c.transform != RASS_BOOST_RAW && c.transform != RASS_BOOST_OPENSEARCH)
        return fail(RASS_ERR_INVALID, "transform must be RASS_BOOST_RAW or RASS_BOOST_OPENSEARCH");
    if (scored && (c.combine < RASS_COMBINE_SUM || c.combine > RASS_COMBINE_REPLACE))
        return fail(RASS_ERR_INVALID, "combine must be one of RASS_COMBINE_*");
    if (c.nq > 0 && !c.bonus) return fail(RASS_ERR_INVALID, "NULL argument");
    if (c.nq > 0 && n_cols != 1 && n_cols != c.nq)
        return fail(RASS_ERR_INVALID, std::string("n_") + col + " must be 1 (shared) or nq (one column per query)");
    if (c.bonus_rows < 0 || col_stride < c.bonus_rows)
        return fail(RASS_ERR_INVALID, std::string(col) + "_rows must be in [0, " + col + "_stride]");
    if (c.q_filter_mask && !c.q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, std::string(who) + " search needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, std::string(who) + " search needs dim <= 1024 (no wide-row form)");
    return RASS_OK;
}

// One attempt of the host search (host_groups): the group's queries and filters through a pinned slot as
// rass_index_search_ex, its boosts, its gates (the function-score search's) and its [b][k] answer through the engine's own
// staging block (eng->d_allow_io).
int search_boosted_once(rass_index_t* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored) {
    rass_engine* eng = idx->eng;
    const int k = c.k;
    return host_groups(
        idx, c.queries, c.nq, c.q_filter, c.q_filter_mask, /*io_bytes=*/0, no_fill,
        [&](HostSlot*, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const size_t cells = (size_t)b * k;
            float *d_boost = nullptr, *d_gate = nullptr, *d_s = nullptr;
            int64_t* d_i = nullptr;
            auto carve = [&](unsigned char* base) {
                Carver d{base};
                d_boost = d.take<float>(RASS_MAX_QBATCH * sizeof(float));
                if (scored) d_gate = d.take<float>(RASS_MAX_QBATCH * sizeof(float));
                d_s = d.take<float>((size_t)RASS_MAX_QBATCH * k * sizeof(float));
                d_i = d.take<int64_t>((size_t)RASS_MAX_QBATCH * k * sizeof(int64_t));
                return d.off;
            };
            if (int rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, carve(nullptr), st)) return rc;
            carve(eng->d_allow_io);
            // (pageable sources: a copy has read the caller's array when it returns)
            if (c.boost) HIP_TRY(hipMemcpyAsync(d_boost, c.boost + done, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            if (c.min_score) HIP_TRY(hipMemcpyAsync(d_gate, c.min_score + done, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            BoostRequest r = group_of(c, done, idx->dim, n_cols, col_stride);
            r.queries = eng->d_qraw, r.nq = b, r.boost = c.boost ? d_boost : nullptr, r.min_score = c.min_score ? d_gate : nullptr;
            r.q_filter = c.q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = c.q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = d_s, r.out_ids = d_i;
            if (int rc = boost_device_group(idx, r)) return rc;
            HIP_TRY(hipMemcpyAsync(c.out_scores + (int64_t)done * k, d_s, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(c.out_ids + (int64_t)done * k, d_i, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [](HostSlot*, int, int) -> int { return RASS_OK; });   // the answer was copied straight to the caller's arrays
}

}  // namespace

// The host and the device form of both searches: api_internal.h.
int boost_search_host(rass_index* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored) {
    if (int rc = check_boosted(idx, c, n_cols, col_stride, scored)) return rc;
    for (int q = 0; q < c.nq; ++q) {
        if (c.boost && !std::isfinite(c.boost[q])) return fail(RASS_ERR_INVALID, "boost[" + std::to_string(q) + "] is not finite");
        if (c.min_score && std::isnan(c.min_score[q])) return fail(RASS_ERR_INVALID, "min_score[" + std::to_string(q) + "] is NaN");
    }
    if (c.nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); },
                      [&] { return search_boosted_once(idx, c, n_cols, col_stride, scored); });
}

int boost_search_device(rass_index* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored) {
    if (int rc = check_boosted(idx, c, n_cols, col_stride, scored)) return rc;
    if (c.nq == 0) return RASS_OK;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    for (int done = 0; done < c.nq; done += RASS_MAX_QBATCH) {
        rc = boost_device_group(idx, group_of(c, done, idx->dim, n_cols, col_stride));
        if (rc != RASS_OK) return rc;
    }
    return RASS_OK;
}

namespace {

// What the column builders check of their target: the block [n_bonus][stride] must hold a value for every row of the index.
int check_bonus_target(const rass_index* idx, const float* d_bonus, int n_bonus, int64_t stride) {
    if (!idx || !d_bonus) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_bonus < 1 || n_bonus > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "n_bonus must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (stride < 0 || stride % 32 != 0) return fail(RASS_ERR_INVALID, "the bonus stride must be a non-negative multiple of 32");
    return RASS_OK;
}
int check_bonus_rows(int64_t n_rows, int64_t stride) {
    if (stride < n_rows)
        return fail(RASS_ERR_INVALID, "the bonus stride (" + std::to_string(stride) + ") is smaller than the index's rows (" +
                                          std::to_string(n_rows) + ")");
    return RASS_OK;
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_boosted(rass_index_t* idx, const float* queries, int nq, int k, const float* boost, int transform,
                              const float* d_bonus, int n_bonus, int64_t bonus_rows, int64_t bonus_stride, const int32_t* q_filter,
                              const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    BoostRequest c;
    c.queries = queries, c.nq = nq, c.k = k, c.boost = boost, c.transform = transform, c.bonus = d_bonus, c.bonus_rows = bonus_rows;
    c.q_filter = q_filter, c.q_filter_mask = q_filter_mask, c.out_scores = out_scores, c.out_ids = out_ids;
    return boost_search_host(idx, c, n_bonus, bonus_stride, /*scored=*/false);
}

int rass_index_search_boosted_device(rass_index_t* idx, const float* d_queries, int nq, int k, const float* d_boost, int transform,
                                     const float* d_bonus, int n_bonus, int64_t bonus_rows, int64_t bonus_stride,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base, float* d_out_scores,
                                     int64_t* d_out_ids) {
    BoostRequest c;
    c.queries = d_queries, c.nq = nq, c.k = k, c.boost = d_boost, c.transform = transform, c.bonus = d_bonus, c.bonus_rows = bonus_rows;
    c.q_filter = d_q_filter, c.q_filter_mask = d_q_filter_mask, c.id_base = id_base, c.out_scores = d_out_scores, c.out_ids = d_out_ids;
    return boost_search_device(idx, c, n_bonus, bonus_stride, /*scored=*/false);
}

int rass_index_bonus_scatter(rass_index_t* idx, const int32_t* q_of, const int64_t* rows, const float* values, int64_t n, float* d_bonus,
                             int n_bonus, int64_t stride) {
    if (int rc = check_bonus_target(idx, d_bonus, n_bonus, stride)) return rc;
    if (n < 0 || (n > 0 && (!q_of || !rows || !values))) return fail(RASS_ERR_INVALID, "bad q_of / rows / values / n");
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if (int rc = check_bonus_rows(n_rows, stride)) return rc;
    std::vector<std::pair<int32_t, int64_t>> cells((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (q_of[i] < 0 || q_of[i] >= n_bonus) return fail(RASS_ERR_INVALID, "a scatter entry names a column outside [0, n_bonus)");
        if (rows[i] < 0 || rows[i] >= n_rows) return fail(RASS_ERR_INVALID, "a scatter entry names a row outside [0, rows)");
        cells[(size_t)i] = {q_of[i], rows[i]};
    }
    std::sort(cells.begin(), cells.end());
    if (std::adjacent_find(cells.begin(), cells.end()) != cells.end())
        return fail(RASS_ERR_INVALID, "a (column, row) pair occurs twice in one scatter: sum duplicates before the call");
    if (n == 0) return RASS_OK;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    Carver c{nullptr};
    c.take<int64_t>((size_t)n * sizeof(int64_t));
    c.take<int32_t>((size_t)n * sizeof(int32_t));
    c.take<float>((size_t)n * sizeof(float));
    if ((rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, c.off, st)) != RASS_OK) return rc;
    Carver d{eng->d_allow_io};
    int64_t* d_rows = d.take<int64_t>((size_t)n * sizeof(int64_t));
    int32_t* d_q = d.take<int32_t>((size_t)n * sizeof(int32_t));
    float* d_v = d.take<float>((size_t)n * sizeof(float));
    HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_q, q_of, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_v, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(rass::launch_bonus_scatter(d_q, d_rows, d_v, n, d_bonus, stride, st));
    HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays have been read
    return RASS_OK;
}

int rass_index_bonus_scatter_device(rass_index_t* idx, const int32_t* d_q_of, const int64_t* d_rows, const float* d_values, int64_t n,
                                    float* d_bonus, int n_bonus, int64_t stride) {
    if (int rc = check_bonus_target(idx, d_bonus, n_bonus, stride)) return rc;
    if (n < 0 || (n > 0 && (!d_q_of || !d_rows || !d_values))) return fail(RASS_ERR_INVALID, "bad q_of / rows / values / n");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    if ((rc = check_bonus_rows(idx->rows.load(std::memory_order_acquire), stride)) != RASS_OK) return rc;
    HIP_TRY(rass::launch_bonus_scatter(d_q_of, d_rows, d_values, n, d_bonus, stride, eng->stream));
    return RASS_OK;
}

int rass_index_bonus_from_attr_clauses(rass_index_t* idx, const int32_t* clauses, const float* weights, int64_t n_clauses, int nq,
                                       int n_bonus, float* d_bonus, int64_t stride, int op) {
    if (int rc = check_bonus_target(idx, d_bonus, n_bonus, stride)) return rc;
    if (n_clauses < 0 || (n_clauses > 0 && (!clauses || !weights))) return fail(RASS_ERR_INVALID, "bad clauses / weights / n_clauses");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (n_bonus != 1 && n_bonus != nq) return fail(RASS_ERR_INVALID, "n_bonus must be 1 (shared) or nq (one column per query)");
    if (op != RASS_BONUS_REPLACE && op != RASS_BONUS_ADD) return fail(RASS_ERR_INVALID, "op must be RASS_BONUS_REPLACE or RASS_BONUS_ADD");
    // query by query, each query's clauses in the caller's order (a stable sort): the order the adds are made in
    struct Clause {
        int32_t q, col, lo, hi, neg;
        float w;
    };
    std::vector<Clause> sorted((size_t)n_clauses);
    std::vector<int32_t> per_query((size_t)n_bonus, 0);
    for (int64_t i = 0; i < n_clauses; ++i) {
        const int32_t* c = clauses + i * 5;
        if (c[0] < 0 || c[0] >= n_bonus)
            return fail(RASS_ERR_INVALID, n_bonus == 1 && nq > 1 ? "a clause of a shared column must name query 0"
                                                                   : "a clause names a query outside [0, nq)");
        if (c[1] < 0 || c[1] >= RASS_MAX_ATTRS) return fail(RASS_ERR_INVALID, "a clause names a column outside [0, RASS_MAX_ATTRS)");
        if (++per_query[(size_t)c[0]] > RASS_MAX_ATTR_CLAUSES)
            return fail(RASS_ERR_INVALID, "more than RASS_MAX_ATTR_CLAUSES clauses for query " + std::to_string(c[0]));
        sorted[(size_t)i] = {c[0], c[1], c[2], c[3], c[4] != 0 ? 1 : 0, weights[i]};
    }
    std::stable_sort(sorted.begin(), sorted.end(), [](const Clause& x, const Clause& y) { return x.q < y.q; });
    // one upload for all launch groups: [n_bonus + groups] offsets (every group's own, rebased, nq_g + 1 of them), the clauses, the weights
    const GroupOffsets off = group_offsets(n_bonus, sorted.size(), [&](size_t i) { return sorted[i].q; });
    const int groups = (int)off.group_off.size();
    std::vector<int32_t> packed((size_t)n_clauses * 4);
    std::vector<float> w((size_t)n_clauses);
    for (size_t i = 0; i < sorted.size(); ++i) {
        packed[4 * i] = sorted[i].col, packed[4 * i + 1] = sorted[i].lo, packed[4 * i + 2] = sorted[i].hi, packed[4 * i + 3] = sorted[i].neg;
        w[i] = sorted[i].w;
    }

    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_bonus_rows(n_rows, stride)) != RASS_OK) return rc;
    Carver c{nullptr};
    c.take<int32_t>(packed.size() * sizeof(int32_t) + 16);
    c.take<float>(w.size() * sizeof(float) + 4);
    c.take<int32_t>(off.q_off.size() * sizeof(int32_t));
    if ((rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, c.off, st)) != RASS_OK) return rc;
    Carver d{eng->d_allow_io};
    int4* d_clauses = reinterpret_cast<int4*>(d.take<int32_t>(packed.size() * sizeof(int32_t) + 16));
    float* d_w = d.take<float>(w.size() * sizeof(float) + 4);
    int32_t* d_off = d.take<int32_t>(off.q_off.size() * sizeof(int32_t));
    if (n_clauses > 0) {
        HIP_TRY(hipMemcpyAsync(d_clauses, packed.data(), packed.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_off, off.q_off.data(), off.q_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    rc = RASS_OK;
    for (int g = 0; g < groups && rc == RASS_OK; ++g) {
        rass::BonusClauseArgs a;
        for (int col = 0; col < RASS_MAX_ATTRS; ++col) a.col[col] = idx->d_attr[col];
        a.clauses = d_clauses + off.group_at[(size_t)g];
        a.weights = d_w + off.group_at[(size_t)g];
        a.q_off = d_off + off.group_off[(size_t)g];
        a.n_rows = n_rows;
        a.bonus = d_bonus + (int64_t)g * RASS_MAX_QBATCH * stride;
        a.stride = stride;
        a.nq = std::min(RASS_MAX_QBATCH, n_bonus - g * RASS_MAX_QBATCH);
        a.add = op == RASS_BONUS_ADD ? 1 : 0;
        rc = HIP_RC(rass::launch_bonus_clauses(a, st));
    }
    const hipError_t e = hipStreamSynchronize(st);   // the host vectors have been read, whatever became of the launches
    if (rc == RASS_OK) rc = HIP_RC(e);
    return rc;
}

int rass_index_bonus_mask(rass_index_t* idx, float* d_bonus, int n_bonus, int64_t stride, const uint32_t* d_allow, int n_bitmaps,
                          int64_t words) {
    if (int rc = check_bonus_target(idx, d_bonus, n_bonus, stride)) return rc;
    if (!d_allow) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_bitmaps != 1 && n_bitmaps != n_bonus) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or n_bonus (one per column)");
    if (words < 0) return fail(RASS_ERR_INVALID, "words is negative");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_bonus_rows(n_rows, stride)) != RASS_OK) return rc;
    if ((rc = check_words(n_rows, words)) != RASS_OK) return rc;
    for (int done = 0; done < n_bonus; done += 32768) {   // the launch's second grid dimension
        const int nb = std::min(32768, n_bonus - done);
        HIP_TRY(rass::launch_bonus_mask(d_bonus + (int64_t)done * stride, nb, stride, n_rows,
                                        d_allow + (n_bitmaps == 1 ? 0 : (int64_t)done * words), n_bitmaps == 1 ? 0 : words, eng->stream));
    }
    return RASS_OK;
}

}  // extern "C"
