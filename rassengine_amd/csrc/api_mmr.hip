// api_mmr.hip — the C ABI of include/rass_engine.h: the diversified (MMR) search rass_index_search_mmr(_device) — a greedy
// maximal-marginal-relevance re-rank of the exact top fetch_k — and its building block rass_index_rows_gram(_device), the
// Gram matrices of short row lists.  Host-side C++ only: the candidates come from the exact fp32 scan (scan_launch, in passes
// of 32 chained on the device by the continuation bound), the kernels are mmr.hip.  The objects and the threading rules:
// api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// The engine's MMR block (eng->d_mmr) of one launch group: a pass's merged lists, the candidates, their Gram matrices, and
// the host entry points' staging (lambda in, answer out).  rass_index_rows_gram stages its lists in cand_rows / gram.
struct MmrView {
    float* pass_s;        // [32][32] one pass of the candidate search (scores, slab rows)
    int64_t* pass_rows;
    float* cand_s;        // [32][kMmrMaxFetch]; a call uses [nq][fetch_k]
    int64_t* cand_rows;
    float* gram;          // [32][kMmrMaxFetch][kMmrMaxFetch]; a call uses [nq][fetch_k][fetch_k]
    float* lambda;        // [32]
    float* out_s;         // [32][kMmrMaxFetch]; a call uses [nq][k]
    int64_t* out_i;
    int32_t* out_rank;
    size_t total;
};
MmrView mmr_layout(unsigned char* base) {
    Carver c{base};
    MmrView L;
    const size_t cells = (size_t)RASS_MAX_QBATCH * rass::kMmrMaxFetch;
    L.pass_s = c.take<float>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(float));
    L.pass_rows = c.take<int64_t>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(int64_t));
    L.cand_s = c.take<float>(cells * sizeof(float));
    L.cand_rows = c.take<int64_t>(cells * sizeof(int64_t));
    L.gram = c.take<float>(cells * rass::kMmrMaxFetch * sizeof(float));
    L.lambda = c.take<float>(RASS_MAX_QBATCH * sizeof(float));
    L.out_s = c.take<float>(cells * sizeof(float));
    L.out_i = c.take<int64_t>(cells * sizeof(int64_t));
    L.out_rank = c.take<int32_t>(cells * sizeof(int32_t));
    L.total = c.off;
    return L;
}

// One launch group (<= 32 queries) of an MMR search: per pass of <= 32 candidates the exact fp32 scan (whatever the index's
// prefilter mode) reporting slab rows, its store into the candidate list (which also leaves the next pass's continuation
// bound); then the Gram matrices of the candidate rows and the selection, which translates rows to ids.  Everything is a
// device pointer; the caller holds eng->mu, has set the device and has checked the arguments.
struct MmrRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    int k = 0;
    int fetch_k = 0;
    const float* lambda = nullptr;      // [nq]
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    float* out_scores = nullptr;        // [nq][k]
    int64_t* out_ids = nullptr;
    int32_t* out_rank = nullptr;        // or nullptr
};

int mmr_device_group(rass_index* idx, const MmrRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    // the scan reports slab rows (the continuation bound names rows, the Gram kernel gathers them): the selection translates
    const IndexView iv = index_view(idx, r.q_filter != nullptr, 0, /*continued=*/true);
    if (iv.id_map && r.fetch_k > RASS_MAX_K)   // the limit rass_index_search_ex has: its list is the definition of the candidates
        return fail(RASS_ERR_UNSUPPORTED, "fetch_k > RASS_MAX_K on an index with caller-assigned row ids");
    int rc = grow_block(&eng->d_mmr, &eng->mmr_bytes, mmr_layout(nullptr).total, st);
    if (rc != RASS_OK) return rc;
    const MmrView W = mmr_layout(eng->d_mmr);
    for (int kdone = 0; kdone < r.fetch_k;) {
        const int kk = std::min(RASS_MAX_K, r.fetch_k - kdone);
        ScanRequest s = scan_request(eng);
        s.corpus = iv.corpus, s.n_rows = iv.rows, s.stride = idx->stride, s.row_tag = iv.row_tag;
        s.queries = r.queries, s.q_dim = idx->dim, s.q_stride = idx->dim, s.nq = r.nq, s.q_filter = r.q_filter;
        s.k = kk, s.id_base = 0, s.id_map = nullptr, s.out_scores = W.pass_s, s.out_ids = W.pass_rows;
        s.timing = eng;
        s.ext.d_q_mask = r.q_filter_mask;
        if (kdone > 0) s.ext.d_after_s = eng->d_after_s, s.ext.d_after_i = eng->d_after_i;
        if ((rc = scan_launch(s)) != RASS_OK) return rc;
        HIP_TRY(rass::launch_allow_store(W.pass_s, W.pass_rows, r.nq, kk, r.fetch_k, kdone, 0, nullptr, W.cand_s, W.cand_rows,
                                         eng->d_after_s, eng->d_after_i, st));
        kdone += kk;
    }
    HIP_TRY(rass::launch_rows_gram(idx->d_rows, idx->stride, idx->d_tags, iv.rows, W.cand_rows, r.nq, r.fetch_k, W.gram, st));
    HIP_TRY(rass::launch_mmr_select(W.cand_s, W.cand_rows, W.gram, r.lambda, r.nq, r.fetch_k, r.k, iv.id_map ? 0 : r.id_base,
                                    iv.id_map, r.out_scores, r.out_ids, r.out_rank, st));
    return RASS_OK;
}

// The argument checks the two search entry points share.
int check_mmr(const rass_index* idx, int k, int fetch_k, const int32_t* q_filter, const int32_t* q_filter_mask) {
    if (fetch_k < 1 || fetch_k > RASS_MAX_MMR_FETCH) return fail(RASS_ERR_INVALID, "fetch_k must be in [1, RASS_MAX_MMR_FETCH]");
    if (k < 1 || k > fetch_k) return fail(RASS_ERR_INVALID, "k must be in [1, fetch_k]");
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "the MMR search needs an fp32 index");
    return RASS_OK;
}

int check_gram(const rass_index* idx, const int64_t* rows, int n_lists, int list_len, const float* out) {
    if (!idx || !rows || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_lists < 1) return fail(RASS_ERR_INVALID, "n_lists must be >= 1");
    if (list_len < 1 || list_len > RASS_MAX_MMR_FETCH) return fail(RASS_ERR_INVALID, "list_len must be in [1, RASS_MAX_MMR_FETCH]");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "rows_gram needs an fp32 index");
    return RASS_OK;
}

// One attempt of the host MMR search (host_groups): the group's queries and filters through a pinned slot as
// rass_index_search_ex, its lambdas and its [b][k] answer through the engine's MMR block.
int search_mmr_once(rass_index_t* idx, const float* queries, int nq, int k, int fetch_k, const float* lambda, const int32_t* q_filter,
                    const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids, int32_t* out_rank) {
    rass_engine* eng = idx->eng;
    return host_groups(
        idx, queries, nq, q_filter, q_filter_mask, /*io_bytes=*/0, no_fill,
        [&](HostSlot*, int done, int b) -> int {
            hipStream_t st = eng->stream;
            if (int rc = grow_block(&eng->d_mmr, &eng->mmr_bytes, mmr_layout(nullptr).total, st)) return rc;
            const MmrView W = mmr_layout(eng->d_mmr);
            HIP_TRY(hipMemcpyAsync(W.lambda, lambda + done, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
            MmrRequest r;
            r.queries = eng->d_qraw, r.nq = b, r.k = k, r.fetch_k = fetch_k, r.lambda = W.lambda;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = W.out_s, r.out_ids = W.out_i, r.out_rank = out_rank ? W.out_rank : nullptr;
            if (int rc = mmr_device_group(idx, r)) return rc;
            const size_t cells = (size_t)b * k;
            HIP_TRY(hipMemcpyAsync(out_scores + (int64_t)done * k, W.out_s, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_ids + (int64_t)done * k, W.out_i, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (out_rank)
                HIP_TRY(hipMemcpyAsync(out_rank + (int64_t)done * k, W.out_rank, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [](HostSlot*, int, int) -> int { return RASS_OK; });   // the answer was copied straight to the caller's arrays
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_rows_gram_device(rass_index_t* idx, const int64_t* d_rows, int n_lists, int list_len, float* d_out) {
    if (int rc = check_gram(idx, d_rows, n_lists, list_len, d_out)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    HIP_TRY(rass::launch_rows_gram(idx->d_rows, idx->stride, idx->d_tags, n_rows, d_rows, n_lists, list_len, d_out, eng->stream));
    return RASS_OK;
}

int rass_index_rows_gram(rass_index_t* idx, const int64_t* rows, int n_lists, int list_len, float* out) {
    if (int rc = check_gram(idx, rows, n_lists, list_len, out)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    if ((rc = grow_block(&eng->d_mmr, &eng->mmr_bytes, mmr_layout(nullptr).total, st)) != RASS_OK) return rc;
    const MmrView W = mmr_layout(eng->d_mmr);
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    // groups of as many lists as the block's candidate area holds (32 lists of 128): staged in, computed, staged out
    const int per_group = RASS_MAX_QBATCH * RASS_MAX_MMR_FETCH / list_len;
    for (int done = 0; done < n_lists; done += per_group) {
        const int b = std::min(per_group, n_lists - done);
        const size_t cells = (size_t)b * list_len;
        HIP_TRY(hipMemcpyAsync(W.cand_rows, rows + (int64_t)done * list_len, cells * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(rass::launch_rows_gram(idx->d_rows, idx->stride, idx->d_tags, n_rows, W.cand_rows, b, list_len, W.gram, st));
        HIP_TRY(hipMemcpyAsync(out + (int64_t)done * list_len * list_len, W.gram, cells * list_len * sizeof(float),
                               hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays have been read and written
    return RASS_OK;
}

int rass_index_search_mmr(rass_index_t* idx, const float* queries, int nq, int k, int fetch_k, const float* lambda,
                          const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                          int32_t* out_rank) {
    if (!idx || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && (!queries || !lambda))) return fail(RASS_ERR_INVALID, "bad queries / lambda / nq");
    if (int rc = check_mmr(idx, k, fetch_k, q_filter, q_filter_mask)) return rc;
    for (int q = 0; q < nq; ++q)
        if (!(lambda[q] >= 0.0f && lambda[q] <= 1.0f)) return fail(RASS_ERR_INVALID, "lambda must be in [0, 1] (and not NaN)");
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_mmr_once(idx, queries, nq, k, fetch_k, lambda, q_filter, q_filter_mask, out_scores, out_ids, out_rank);
    });
}

int rass_index_search_mmr_device(rass_index_t* idx, const float* d_queries, int nq, int k, int fetch_k, const float* d_lambda,
                                 const int32_t* d_q_filter, const int32_t* d_q_filter_mask, int64_t id_base, float* d_out_scores,
                                 int64_t* d_out_ids, int32_t* d_out_rank) {
    if (!idx || !d_queries || !d_lambda || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_mmr(idx, k, fetch_k, d_q_filter, d_q_filter_mask)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    MmrRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.fetch_k = fetch_k, r.lambda = d_lambda;
    r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask, r.id_base = id_base;
    r.out_scores = d_out_scores, r.out_ids = d_out_ids, r.out_rank = d_out_rank;
    return mmr_device_group(idx, r);
}

}  // extern "C"
