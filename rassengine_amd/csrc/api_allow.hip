// api_allow.hip — the C ABI of include/rass_engine.h: the allow-list search rass_index_search_allowed(_device) (exact
// top-k within a per-query row bitmap), the bitmap builders rass_index_allow_from_rows / _from_tag_values, the plan hook
// rass_index_allow_plan and a bitmap's popcount rass_index_allow_count.  Host-side C++ only: the kernels are scan_topk.hip (ScanMode kAllow) and allow.hip.  The objects
// and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {

// The work list of one launch group and the plan's workspace (eng->d_allow), sized by the index's tiles (AllowView: api_internal.h).
AllowView allow_layout(unsigned char* base, int64_t rows) {
    Carver c{base};
    AllowView L;
    const size_t tiles = (size_t)std::max<int64_t>((rows + 31) / 32, 1);
    L.work_tile = c.take<int32_t>(tiles * sizeof(int32_t));
    L.work_rows = c.take<int32_t>(tiles * sizeof(int32_t));
    L.work_mask = c.take<uint32_t>(tiles * sizeof(uint32_t));
    L.n_work = c.take<int32_t>(sizeof(int32_t));
    L.plan_ws = c.take<unsigned char>(rass::allow_plan_workspace_bytes(rows));
    L.total = c.off;
    return L;
}

int check_words(int64_t rows, int64_t words) {
    if (words < (rows + 31) / 32)
        return fail(RASS_ERR_INVALID, "words_per_bitmap (" + std::to_string(words) + ") is smaller than ceil(rows / 32) = " +
                                          std::to_string((rows + 31) / 32));
    return RASS_OK;
}

namespace {

// One launch group (<= 32 queries) of an allowed search: normalise -> plan -> per pass of <= 32 hits: the allow scan over the
// work list, merge, store (which also leaves the next pass's continuation bound).  Always the exact fp32 scan: the prefilter
// mode of the index is not looked at.  Everything is a device pointer; the caller holds eng->mu, has set the device and has
// checked the arguments that do not depend on the row count.
struct AllowRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    int k = 0;
    const uint32_t* allow = nullptr;    // query q's words at allow + q * q_stride
    int64_t q_stride = 0;               // 0: one bitmap shared by every query
    int64_t words = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    float* out_scores = nullptr;        // [nq][k]
    int64_t* out_ids = nullptr;
};

int allow_device_group(rass_index* idx, const AllowRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    // the scan reports slab rows (the continuation bound names rows): the store translates them
    const IndexView iv = index_view(idx, r.q_filter != nullptr, 0, /*continued=*/true);
    const int64_t stride = idx->stride;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (int rc = check_words(iv.rows, r.words)) return rc;
    if (scratch_layout(nullptr, RASS_MAX_QBATCH, RASS_MAX_K).total > eng->scratch_bytes)
        return fail(RASS_ERR_INVALID, "scan workspace too small");
    if (iv.rows == 0) {   // nothing to plan or scan: the empty answer
        HIP_TRY(rass::launch_fill_i32(reinterpret_cast<int32_t*>(r.out_scores), (int64_t)nq * k, (int32_t)0xff800000u, st));
        HIP_TRY(hipMemsetAsync(r.out_ids, 0xff, (size_t)nq * k * sizeof(int64_t), st));
        return RASS_OK;
    }
    int rc = grow_block(&eng->d_allow, &eng->allow_bytes, allow_layout(nullptr, iv.rows).total, st);
    if (rc != RASS_OK) return rc;
    const AllowView W = allow_layout(eng->d_allow, iv.rows);
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    // 32 query rows whatever nq is: the allow scan has one variant per stride (two MFMA N tiles)
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, RASS_MAX_QBATCH));
    HIP_TRY(rass::launch_allow_plan(r.allow, r.q_stride, nq, iv.rows, W.work_tile, W.work_rows, W.work_mask, W.n_work, W.plan_ws, st));
    for (int kdone = 0; kdone < k;) {
        const int kk = std::min(RASS_MAX_K, k - kdone);
        // the item count is only known on the device: the grid is sized by the slab, a workgroup without items writes empty lists
        const int grid = scan_grid((iv.rows + 31) / 32, kk, eng->n_cus);
        rass::ScanArgs a;
        a.corpus = iv.corpus;
        a.row_tag = iv.row_tag;
        a.q_padded = L.q_padded;
        a.q_filter = r.q_filter;
        a.q_filter_mask = r.q_filter_mask;
        a.q_after_score = kdone > 0 ? eng->d_after_s : nullptr;
        a.q_after_id = kdone > 0 ? eng->d_after_i : nullptr;
        a.part_scores = L.part_scores;
        a.part_ids = L.part_ids;
        a.row_stride = stride;
        a.id_base = 0;
        a.n_rows = (int)iv.rows;
        a.nq = nq;
        a.k = kk;
        a.xcd_skew = scan_xcd_skew(RASS_MAX_QBATCH, grid, eng->n_cus);
        set_plan(a, IvfPlan{W.work_tile, W.work_rows, W.work_mask, W.n_work, (iv.rows + 31) / 32});
        a.allow = r.allow;
        a.allow_q_stride = r.q_stride;
        rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
        if (rc != RASS_OK) return rc;
        HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, kk, L.cand_scores, L.cand_ids, st));
        HIP_TRY(rass::launch_allow_store(L.cand_scores, L.cand_ids, nq, kk, k, kdone, iv.id_map ? 0 : r.id_base, iv.id_map, r.out_scores,
                                         r.out_ids, eng->d_after_s, eng->d_after_i, st));
        kdone += kk;
    }
    return RASS_OK;
}

// The argument checks the entry points share (everything that does not need the row count).
int check_allowed(const rass_index* idx, int nq, int k, const uint32_t* allow, int n_bitmaps, int64_t words, const int32_t* q_filter,
                  const int32_t* q_filter_mask) {
    if (nq < 0 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [0, RASS_MAX_DEVICE_BATCH]");
    if (k < 1 || k > RASS_MAX_K_MULTIPASS) return fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K_MULTIPASS]");
    if (nq > 0 && !allow) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && n_bitmaps != 1 && n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
    if (words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "allowed search needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "allowed search needs dim <= 1024 (no wide-row form)");
    return RASS_OK;
}

int check_bitmap_target(const rass_index* idx, const uint32_t* d_allow, int64_t words) {
    if (!idx || !d_allow) return fail(RASS_ERR_INVALID, "NULL argument");
    if (words < 0) return fail(RASS_ERR_INVALID, "words is negative");
    return RASS_OK;
}

// One attempt of the host allowed search (host_groups): the group's queries and filters through a pinned slot as
// rass_index_search_ex, its bitmaps and its [b][k] answer through the engine's own staging block (eng->d_allow_io).
int search_allowed_once(rass_index_t* idx, const float* queries, int nq, int k, const uint32_t* allow, int n_bitmaps, int64_t words,
                        const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    rass_engine* eng = idx->eng;
    const bool shared = n_bitmaps == 1;
    return host_groups(
        // io_bytes 0: h_io / d_io are not used.  The staging is sized by the bitmaps, not by a fixed layout, and pageable on
        // the host side (the caller's own arrays): it stays in eng->d_allow_io, grown below.
        idx, queries, nq, q_filter, q_filter_mask, /*io_bytes=*/0, no_fill,
        [&](HostSlot*, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const size_t cells = (size_t)b * k;
            Carver c{nullptr};
            const size_t bits_bytes = (size_t)(shared ? 1 : b) * words * sizeof(uint32_t);
            c.take<uint32_t>(bits_bytes);
            c.take<float>((size_t)RASS_MAX_QBATCH * k * sizeof(float));
            c.take<int64_t>((size_t)RASS_MAX_QBATCH * k * sizeof(int64_t));
            if (int rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, c.off, st)) return rc;
            Carver d{eng->d_allow_io};
            uint32_t* d_bits = d.take<uint32_t>(bits_bytes);
            float* d_s = d.take<float>((size_t)RASS_MAX_QBATCH * k * sizeof(float));
            int64_t* d_i = d.take<int64_t>((size_t)RASS_MAX_QBATCH * k * sizeof(int64_t));
            if (bits_bytes)
                HIP_TRY(hipMemcpyAsync(d_bits, allow + (shared ? 0 : (int64_t)done * words), bits_bytes, hipMemcpyHostToDevice, st));
            AllowRequest r;
            r.queries = eng->d_qraw, r.nq = b, r.k = k, r.allow = d_bits, r.q_stride = shared ? 0 : words, r.words = words;
            r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = d_s, r.out_ids = d_i;
            if (int rc = allow_device_group(idx, r)) return rc;
            HIP_TRY(hipMemcpyAsync(out_scores + (int64_t)done * k, d_s, cells * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_ids + (int64_t)done * k, d_i, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            return RASS_OK;
        },
        [](HostSlot*, int, int) -> int { return RASS_OK; });   // the answer was copied straight to the caller's arrays
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_allowed(rass_index_t* idx, const float* queries, int nq, int k, const uint32_t* allow, int n_bitmaps,
                              int64_t words_per_bitmap, const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores,
                              int64_t* out_ids) {
    if (!idx || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && !queries) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_allowed(idx, nq, k, allow, n_bitmaps, words_per_bitmap, q_filter, q_filter_mask)) return rc;
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_allowed_once(idx, queries, nq, k, allow, n_bitmaps, words_per_bitmap, q_filter, q_filter_mask, out_scores, out_ids);
    });
}

int rass_index_search_allowed_device(rass_index_t* idx, const float* d_queries, int nq, int k, const uint32_t* d_allow, int n_bitmaps,
                                     int64_t words_per_bitmap, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, float* d_out_scores, int64_t* d_out_ids) {
    if (!idx || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq > 0 && !d_queries) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_allowed(idx, nq, k, d_allow, n_bitmaps, words_per_bitmap, d_q_filter, d_q_filter_mask)) return rc;
    if (nq == 0) return RASS_OK;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const bool shared = n_bitmaps == 1;
    for (int done = 0; done < nq; done += RASS_MAX_QBATCH) {
        AllowRequest r;
        r.queries = d_queries + (int64_t)done * idx->dim, r.nq = std::min(RASS_MAX_QBATCH, nq - done), r.k = k;
        r.allow = d_allow + (shared ? 0 : (int64_t)done * words_per_bitmap), r.q_stride = shared ? 0 : words_per_bitmap;
        r.words = words_per_bitmap;
        r.q_filter = d_q_filter ? d_q_filter + done : nullptr, r.q_filter_mask = d_q_filter_mask ? d_q_filter_mask + done : nullptr;
        r.id_base = id_base;
        r.out_scores = d_out_scores + (int64_t)done * k, r.out_ids = d_out_ids + (int64_t)done * k;
        rc = allow_device_group(idx, r);
        if (rc != RASS_OK) return rc;
    }
    return RASS_OK;
}

int rass_index_allow_from_rows(rass_index_t* idx, const int64_t* rows, int64_t n, uint32_t* d_allow, int64_t words) {
    if (int rc = check_bitmap_target(idx, d_allow, words)) return rc;
    if (n < 0 || (n > 0 && !rows)) return fail(RASS_ERR_INVALID, "bad rows / n");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_words(n_rows, words)) != RASS_OK) return rc;
    if (words) HIP_TRY(hipMemsetAsync(d_allow, 0, (size_t)words * sizeof(uint32_t), st));
    if (n == 0 || n_rows == 0) return RASS_OK;
    rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, (size_t)n * sizeof(int64_t), st);
    if (rc != RASS_OK) return rc;
    int64_t* d_rows = reinterpret_cast<int64_t*>(eng->d_allow_io);
    HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(rass::launch_allow_from_rows(d_rows, n, n_rows, d_allow, st));
    HIP_TRY(hipStreamSynchronize(st));   // the caller's array has been read
    return RASS_OK;
}

int rass_index_allow_from_tag_values(rass_index_t* idx, const int32_t* values, int64_t n_values, int32_t mask, uint32_t* d_allow,
                                     int64_t words) {
    if (int rc = check_bitmap_target(idx, d_allow, words)) return rc;
    if (n_values < 0 || n_values > 0x7fffffff || (n_values > 0 && !values)) return fail(RASS_ERR_INVALID, "bad values / n_values");
    std::vector<int32_t> sorted(values, values + n_values);   // the kernel searches an ascending set
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_words(n_rows, words)) != RASS_OK) return rc;
    if (words) HIP_TRY(hipMemsetAsync(d_allow, 0, (size_t)words * sizeof(uint32_t), st));
    if (sorted.empty() || n_rows == 0) return RASS_OK;
    rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, sorted.size() * sizeof(int32_t), st);
    if (rc != RASS_OK) return rc;
    int32_t* d_values = reinterpret_cast<int32_t*>(eng->d_allow_io);
    HIP_TRY(hipMemcpyAsync(d_values, sorted.data(), sorted.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(rass::launch_allow_from_tag_values(idx->d_tags, n_rows, d_values, (int)sorted.size(), mask, d_allow, st));
    HIP_TRY(hipStreamSynchronize(st));   // `sorted` has been read
    return RASS_OK;
}

int rass_index_allow_plan(rass_index_t* idx, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap, int nq, int32_t* out_tile,
                          int32_t* out_rows, uint32_t* out_mask, int64_t capacity, int64_t* out_n) {
    if (!idx || !d_allow || !out_n) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (n_bitmaps != 1 && n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
    if (capacity < 0 || (capacity > 0 && (!out_tile || !out_rows || !out_mask))) return fail(RASS_ERR_INVALID, "bad capacity / outputs");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if (n_rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if ((rc = check_words(n_rows, words_per_bitmap)) != RASS_OK) return rc;
    *out_n = 0;
    if (n_rows == 0) return RASS_OK;
    rc = grow_block(&eng->d_allow, &eng->allow_bytes, allow_layout(nullptr, n_rows).total, st);
    if (rc != RASS_OK) return rc;
    const AllowView W = allow_layout(eng->d_allow, n_rows);
    HIP_TRY(rass::launch_allow_plan(d_allow, n_bitmaps == 1 ? 0 : words_per_bitmap, nq, n_rows, W.work_tile, W.work_rows, W.work_mask,
                                    W.n_work, W.plan_ws, st));
    int32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, W.n_work, sizeof(n), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_n = n;
    const size_t take = (size_t)std::min<int64_t>(n, capacity);
    if (take) {
        HIP_TRY(hipMemcpyAsync(out_tile, W.work_tile, take * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_rows, W.work_rows, take * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_mask, W.work_mask, take * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RASS_OK;
}

int rass_index_allow_count(rass_index_t* idx, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap, int64_t* out_counts) {
    if (!idx || !d_allow || !out_counts) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_bitmaps < 1 || n_bitmaps > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "n_bitmaps must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (words_per_bitmap < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_words(n_rows, words_per_bitmap)) != RASS_OK) return rc;
    rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, (size_t)n_bitmaps * sizeof(int64_t), st);
    if (rc != RASS_OK) return rc;
    int64_t* d_counts = reinterpret_cast<int64_t*>(eng->d_allow_io);
    HIP_TRY(rass::launch_allow_count(d_allow, words_per_bitmap, n_bitmaps, n_rows, d_counts, st));
    HIP_TRY(hipMemcpyAsync(out_counts, d_counts, (size_t)n_bitmaps * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RASS_OK;
}

}  // extern "C"
