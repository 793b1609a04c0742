// api_fscore.hip — the C ABI of include/rass_engine.h: the function-score search rass_index_search_scored(_device) (exact
// top-k of combine(boost * T(cos), a function column), gated by the transformed similarity) and the builder of its columns,
// rass_index_fn_from_attr.  Host-side C++ only: the kernels are scan_fscore.hip and score_fn.hip; the search itself —
// checks, group loops, pass driver, merge and store — is the boosted search's (boost_search_host / boost_search_device in
// api_boost.hip).  The objects and the threading rules: api_internal.h.

#include <cmath>

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// One record, checked and turned into the device's form (the constants derived in double).
int convert_fn(const rass_score_fn_t& f, int64_t i, int n_fn, int n_filters, rass::ScoreFnRec* out) {
    const std::string at = "function " + std::to_string(i) + ": ";
    if (f.query < 0 || f.query >= n_fn)
        return fail(RASS_ERR_INVALID, at + "names a query outside [0, n_fn) (a shared column's functions name query 0)");
    if (f.kind < RASS_FN_GAUSS || f.kind > RASS_FN_WEIGHT) return fail(RASS_ERR_INVALID, at + "unknown kind");
    if (f.kind != RASS_FN_WEIGHT && (f.col < 0 || f.col >= RASS_MAX_ATTRS))
        return fail(RASS_ERR_INVALID, at + "names a column outside [0, RASS_MAX_ATTRS)");
    if (f.filter < -1 || f.filter >= n_filters) return fail(RASS_ERR_INVALID, at + "names a filter outside [-1, n_filters)");
    if (!std::isfinite(f.weight)) return fail(RASS_ERR_INVALID, at + "the weight is not finite");
    rass::ScoreFnRec r{};
    r.kind = f.kind, r.col = f.kind == RASS_FN_WEIGHT ? 0 : f.col, r.filter = f.filter, r.modifier = 0, r.weight = f.weight;
    r.p0 = r.p1 = r.c = 0.0, r.missing = 0.0;
    if (f.kind <= RASS_FN_LINEAR) {
        if (!std::isfinite(f.origin)) return fail(RASS_ERR_INVALID, at + "origin is not finite");
        if (!(f.scale > 0.0) || !std::isfinite(f.scale)) return fail(RASS_ERR_INVALID, at + "scale must be > 0");
        if (!(f.offset >= 0.0) || !std::isfinite(f.offset)) return fail(RASS_ERR_INVALID, at + "offset must be >= 0");
        if (!(f.decay > 0.0 && f.decay < 1.0)) return fail(RASS_ERR_INVALID, at + "decay must be in (0, 1)");
        r.p0 = f.origin, r.p1 = f.offset;
        if (f.kind == RASS_FN_GAUSS) r.c = std::log(f.decay) / (f.scale * f.scale);
        if (f.kind == RASS_FN_EXP) r.c = std::log(f.decay) / f.scale;
        if (f.kind == RASS_FN_LINEAR) r.c = f.scale / (1.0 - f.decay);
    } else if (f.kind == RASS_FN_FIELD_VALUE) {
        if (f.modifier < RASS_FN_MOD_NONE || f.modifier > RASS_FN_MOD_RECIPROCAL) return fail(RASS_ERR_INVALID, at + "unknown modifier");
        if (!std::isfinite(f.factor)) return fail(RASS_ERR_INVALID, at + "factor is not finite");
        if (std::isinf(f.missing)) return fail(RASS_ERR_INVALID, at + "missing must be finite, or NaN for none");
        r.modifier = f.modifier, r.p0 = f.factor, r.missing = f.missing;
    }
    *out = r;
    return RASS_OK;
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_scored(rass_index_t* idx, const float* queries, int nq, int k, const float* boost, int transform, int combine,
                             const float* min_score, const float* d_fn, int n_fn, int64_t fn_rows, int64_t fn_stride,
                             const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    BoostRequest c;
    c.queries = queries, c.nq = nq, c.k = k, c.boost = boost, c.transform = transform, c.combine = combine, c.min_score = min_score;
    c.bonus = d_fn, c.bonus_rows = fn_rows, c.q_filter = q_filter, c.q_filter_mask = q_filter_mask;
    c.out_scores = out_scores, c.out_ids = out_ids;
    return boost_search_host(idx, c, n_fn, fn_stride, /*scored=*/true);
}

int rass_index_search_scored_device(rass_index_t* idx, const float* d_queries, int nq, int k, const float* d_boost, int transform,
                                    int combine, const float* d_min_score, const float* d_fn, int n_fn, int64_t fn_rows,
                                    int64_t fn_stride, const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base,
                                    float* d_out_scores, int64_t* d_out_ids) {
    BoostRequest c;
    c.queries = d_queries, c.nq = nq, c.k = k, c.boost = d_boost, c.transform = transform, c.combine = combine, c.min_score = d_min_score;
    c.bonus = d_fn, c.bonus_rows = fn_rows, c.q_filter = d_q_filter, c.q_filter_mask = d_q_filter_mask, c.id_base = id_base;
    c.out_scores = d_out_scores, c.out_ids = d_out_ids;
    return boost_search_device(idx, c, n_fn, fn_stride, /*scored=*/true);
}

int rass_index_fn_from_attr(rass_index_t* idx, const rass_score_fn_t* fns, int64_t n_fns, int n_fn, int score_mode, double max_boost,
                            const uint32_t* d_filters, int n_filters, int64_t words, float* d_fn, int64_t stride) {
    if (!idx || !d_fn) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_fn < 1 || n_fn > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "n_fn must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (stride < 0 || stride % 32 != 0) return fail(RASS_ERR_INVALID, "the column stride must be a non-negative multiple of 32");
    if (n_fns < 0 || (n_fns > 0 && !fns)) return fail(RASS_ERR_INVALID, "bad fns / n_fns");
    if (score_mode < RASS_FN_SCORE_MULTIPLY || score_mode > RASS_FN_SCORE_MIN)
        return fail(RASS_ERR_INVALID, "score_mode must be one of RASS_FN_SCORE_*");
    if (std::isnan(max_boost)) return fail(RASS_ERR_INVALID, "max_boost is NaN (+inf: no cap)");
    if (n_filters < 0 || words < 0 || (n_filters > 0 && !d_filters)) return fail(RASS_ERR_INVALID, "bad d_filters / n_filters / words");
    // query by query, each query's functions in the caller's order (a stable sort): the order they are folded in
    std::vector<std::pair<int32_t, rass::ScoreFnRec>> sorted((size_t)n_fns);
    std::vector<int32_t> per_query((size_t)n_fn, 0);
    bool filtered = false;
    for (int64_t i = 0; i < n_fns; ++i) {
        if (int rc = convert_fn(fns[i], i, n_fn, n_filters, &sorted[(size_t)i].second)) return rc;
        sorted[(size_t)i].first = fns[i].query;
        filtered = filtered || fns[i].filter >= 0;
        if (++per_query[(size_t)fns[i].query] > RASS_MAX_SCORE_FNS)
            return fail(RASS_ERR_INVALID, "more than RASS_MAX_SCORE_FNS functions for query " + std::to_string(fns[i].query));
    }
    std::stable_sort(sorted.begin(), sorted.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    // one upload for all launch groups: every group's own offsets (rebased, nq_g + 1 of them), then the records
    const GroupOffsets off = group_offsets(n_fn, sorted.size(), [&](size_t i) { return sorted[i].first; });
    const int groups = (int)off.group_off.size();
    std::vector<rass::ScoreFnRec> recs((size_t)n_fns);
    for (size_t i = 0; i < sorted.size(); ++i) recs[i] = sorted[i].second;

    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if (stride < n_rows)
        return fail(RASS_ERR_INVALID, "the column stride (" + std::to_string(stride) + ") is smaller than the index's rows (" +
                                          std::to_string(n_rows) + ")");
    if (filtered && (rc = check_words(n_rows, words)) != RASS_OK) return rc;
    Carver c{nullptr};
    c.take<rass::ScoreFnRec>((recs.size() + 1) * sizeof(rass::ScoreFnRec));
    c.take<int32_t>(off.q_off.size() * sizeof(int32_t));
    if ((rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, c.off, st)) != RASS_OK) return rc;
    Carver d{eng->d_allow_io};
    rass::ScoreFnRec* d_recs = d.take<rass::ScoreFnRec>((recs.size() + 1) * sizeof(rass::ScoreFnRec));
    int32_t* d_off = d.take<int32_t>(off.q_off.size() * sizeof(int32_t));
    if (n_fns > 0) HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), recs.size() * sizeof(rass::ScoreFnRec), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, off.q_off.data(), off.q_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    rc = RASS_OK;
    for (int g = 0; g < groups && rc == RASS_OK; ++g) {
        rass::ScoreFnArgs a;
        for (int col = 0; col < RASS_MAX_ATTRS; ++col) a.col[col] = idx->d_attr[col];
        a.recs = d_recs + off.group_at[(size_t)g];
        a.q_off = d_off + off.group_off[(size_t)g];
        a.filters = d_filters;
        a.words = words;
        a.n_rows = n_rows;
        a.out = d_fn + (int64_t)g * RASS_MAX_QBATCH * stride;
        a.stride = stride;
        a.nq = std::min(RASS_MAX_QBATCH, n_fn - g * RASS_MAX_QBATCH);
        a.score_mode = score_mode;
        a.max_boost = max_boost;
        rc = HIP_RC(rass::launch_score_fn(a, st));
    }
    const hipError_t e = hipStreamSynchronize(st);   // the host vectors have been read, whatever became of the launches
    if (rc == RASS_OK) rc = HIP_RC(e);
    return rc;
}

}  // extern "C"
