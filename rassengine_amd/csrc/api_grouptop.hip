// api_grouptop.hip — the C ABI of include/rass_engine.h: the grouped search with inner hits over a key column,
// rass_index_search_group_hits_keys(_device): the group_size best rows of each of a query's k best groups and, where asked
// for, the capped list (the exact top-k with at most group_size rows of any group).  Host-side C++ only: the kernels are
// scan_grouptop.hip (the one-pass scan into a level-major table) and group_topk.hip (the unchanged select over plane 0 of it,
// then group_hits_finish_kernel).  The table lives in the engine-owned block of the grouped search (eng->d_group).  The
// objects and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {
namespace {

// One launch group (<= 32 queries).  Everything is a device pointer.
struct HitsRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    int k = 0;
    int32_t n_groups = 0;
    int group_size = 0;
    const int32_t* keys = nullptr;
    int64_t n_keys = 0;
    const uint32_t* allow = nullptr;    // this launch group's bitmap(s); allow_q_stride 0: one shared by all of them
    int64_t allow_q_stride = 0, allow_words = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    float* out_scores = nullptr;        // [nq][k][group_size]
    int64_t* out_ids = nullptr;
    int32_t* out_groups = nullptr;      // [nq][k]
    int64_t* total = nullptr;           // [nq]
    float* cap_scores = nullptr;        // [nq][k] or nullptr
    int64_t* cap_ids = nullptr;
    int32_t* status = nullptr;          // [1]
    bool accumulate = false;            // a later launch group of the call: the status word is only raised
};

// What the caller passed, whole.
struct HitsArgs {
    int k;
    const int32_t* keys;
    int64_t n_keys;
    int32_t n_groups;
    int group_size;
    const uint32_t* allow;
    int n_bitmaps;
    int64_t words;
    const int32_t* q_filter;
    const int32_t* q_filter_mask;
    bool capped;
};

// ... and a launch group's part of it.
void hits_request(HitsRequest& r, const HitsArgs& a, int done) {
    r.k = a.k, r.n_groups = a.n_groups, r.group_size = a.group_size;
    r.keys = a.keys, r.n_keys = a.n_keys;
    if (a.allow) {
        r.allow_q_stride = a.n_bitmaps == 1 ? 0 : a.words;
        r.allow = a.allow + (int64_t)done * r.allow_q_stride;
        r.allow_words = a.words;
    }
}

// The argument checks the two entry points share (everything that does not need the row count).
int check_hits(const rass_index* idx, const HitsArgs& a, int nq) {
    if (a.k < 1 || a.k > rass::kGroupMaxK) return fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K_MULTIPASS]");
    if (a.n_groups < 1 || a.n_groups > rass::kGroupMaxGroups) return fail(RASS_ERR_INVALID, "n_groups must be in [1, 1048576]");
    if (a.group_size < 1 || a.group_size > RASS_MAX_GROUP_SIZE) return fail(RASS_ERR_INVALID, "group_size must be in [1, RASS_MAX_GROUP_SIZE]");
    if ((int64_t)a.n_groups * a.group_size > rass::kGroupMaxGroups)
        return fail(RASS_ERR_INVALID, "n_groups * group_size must not exceed 1048576 (the table of a launch group stays within 256 MiB)");
    if (a.capped && (int64_t)a.k * a.group_size > rass::kGroupMaxK)
        return fail(RASS_ERR_INVALID, "the capped list needs k * group_size <= RASS_MAX_K_MULTIPASS");
    if (a.q_filter_mask && !a.q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (!a.keys) return fail(RASS_ERR_INVALID, "d_keys is NULL");
    if (a.n_keys < 0) return fail(RASS_ERR_INVALID, "n_keys is negative");
    if (a.allow) {
        if (a.n_bitmaps != 1 && a.n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
        if (a.words < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    }
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "group-hits search needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "group-hits search needs dim <= 1024 (no wide-row form)");
    return RASS_OK;
}

// normalise -> ONE memset over the status word and every level of the table -> the group-top scan -> the select over plane 0
// -> the finish.  Always the exact fp32 scan: the prefilter mode of the index is not looked at.  The caller holds eng->mu and
// has set the device.
int hits_device_group(rass_index* idx, const HitsRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, /*filtered=*/true, r.id_base);   // tombstones and filters: always read the tags
    if (r.n_keys < iv.rows)
        return fail(RASS_ERR_INVALID, "n_keys (" + std::to_string(r.n_keys) + ") is smaller than the index's rows (" + std::to_string(iv.rows) + ")");
    if (r.allow)
        if (int rc = check_words(iv.rows, r.allow_words)) return rc;
    if (iv.rows < 0 || iv.rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    const RangeView S = range_layout(nullptr);
    if (S.total > eng->scratch_bytes) return fail(RASS_ERR_INVALID, "scan workspace too small");
    float* q_padded = range_layout(eng->d_scratch).q_padded;   // where every scan keeps its queries
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, q_padded, idx->stride, r.nq, idx->dim, st, pad_nq(r.nq)));
    // level-major: group_size planes of [nq][n_groups] slots behind the status line — the grouped search's layout, group_size times over
    const int planes = r.nq * r.group_size;
    if (int rc = grow_group_table(eng, group_layout(nullptr, planes, r.n_groups).total, st, "group-hits search")) return rc;
    const GroupView G = group_layout(eng->d_group, planes, r.n_groups);
    HIP_TRY(hipMemsetAsync(G.status, 0, G.total, st));
    if (iv.rows > 0) {   // an empty index is not scanned: the zeroed table is the answer
        const int grid = scan_grid((iv.rows + 31) / 32, 1, eng->n_cus);
        rass::GroupTopArgs a;
        a.scan.corpus = iv.corpus;
        a.scan.row_tag = iv.row_tag;
        a.scan.q_padded = q_padded;
        a.scan.q_filter = r.q_filter;
        a.scan.q_filter_mask = r.q_filter_mask;
        a.scan.part_scores = nullptr;
        a.scan.part_ids = nullptr;
        a.scan.row_stride = idx->stride;
        a.scan.id_base = 0;   // the keys name rows of the slab: the finishing launches translate them
        a.scan.n_rows = (int)iv.rows;
        a.scan.nq = r.nq;
        a.scan.k = 1;
        a.scan.group_table = G.table;
        a.scan.group_status = G.status;
        a.scan.group_n = r.n_groups;
        a.scan.group_keys = r.keys;
        a.scan.group_key_rows = (int)iv.rows;
        a.scan.allow = r.allow;
        a.scan.allow_q_stride = r.allow_q_stride;
        a.level_stride = (int64_t)r.nq * r.n_groups;
        a.group_size = r.group_size;
        const int rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_grouptop_f32(a, grid, st)); });
        if (rc != RASS_OK) return rc;
    }
    // The select's own [nq][k] scores and ids (each group's best row) land in the head of the three-dimensional outputs, which
    // the finish then overwrites whole without reading them; its copy of the status word goes to the spare word of the status line.
    HIP_TRY(rass::launch_group_select(G.table, r.nq, r.n_groups, r.k, iv.id_base, iv.id_map, r.out_scores, r.out_ids, r.out_groups,
                                      r.total, G.status, reinterpret_cast<int32_t*>(G.status + 1), st));
    HIP_TRY(rass::launch_group_hits_finish(G.table, r.nq, r.n_groups, r.k, r.group_size, iv.id_base, iv.id_map, r.out_groups,
                                           r.out_scores, r.out_ids, r.cap_scores, r.cap_ids, G.status, r.status, r.accumulate, st));
    return RASS_OK;
}

// The device staging of the host variant's lists (eng->d_allow_io), sized by the call.
struct HitsIoView {
    float* out_scores;      // [32][k][group_size]
    int64_t* out_ids;
    float* cap_scores;      // [32][k]
    int64_t* cap_ids;
    size_t bytes;
};
HitsIoView hits_io_layout(unsigned char* base, int k, int group_size) {
    Carver c{base};
    HitsIoView L;
    const size_t cells = (size_t)RASS_MAX_QBATCH * k * group_size;
    L.out_scores = c.take<float>(cells * sizeof(float));
    L.out_ids = c.take<int64_t>(cells * sizeof(int64_t));
    L.cap_scores = c.take<float>((size_t)RASS_MAX_QBATCH * k * sizeof(float));
    L.cap_ids = c.take<int64_t>((size_t)RASS_MAX_QBATCH * k * sizeof(int64_t));
    L.bytes = c.off;
    return L;
}

// One attempt of the host search.  Totals, status and groups go through the grouped search's pinned staging (GroupIoView); the
// lists through the engine's own staging block, straight to the caller's arrays.  A group whose scan met a key >= n_groups
// ends the call.
int search_hits_once(rass_index* idx, const float* queries, int nq, const HitsArgs& a, float* out_scores, int64_t* out_ids,
                     int32_t* out_groups, int64_t* out_total, float* cap_scores, int64_t* cap_ids) {
    rass_engine* eng = idx->eng;
    const int k = a.k, gs = a.group_size;
    return host_groups(
        idx, queries, nq, a.q_filter, a.q_filter_mask, group_io_layout(nullptr).bytes, no_fill,
        [&](HostSlot* sl, int done, int b) -> int {
            hipStream_t st = eng->stream;
            const GroupIoView H = group_io_layout(static_cast<unsigned char*>(sl->h_io)), D = group_io_layout(eng->d_io);
            if (int rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, hits_io_layout(nullptr, k, gs).bytes, st)) return rc;
            const HitsIoView L = hits_io_layout(eng->d_allow_io, k, gs);
            const size_t cells = (size_t)b * k;
            HitsRequest r;
            hits_request(r, a, done);
            r.queries = eng->d_qraw, r.nq = b;
            r.q_filter = a.q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = a.q_filter_mask ? eng->d_qmask : nullptr;
            r.out_scores = L.out_scores, r.out_ids = L.out_ids, r.out_groups = D.out_groups, r.total = D.total, r.status = D.status;
            if (a.capped) r.cap_scores = L.cap_scores, r.cap_ids = L.cap_ids;
            if (int grc = hits_device_group(idx, r)) return grc;
            HIP_TRY(hipMemcpyAsync(H.total, D.total, (size_t)b * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.status, D.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(H.out_groups, D.out_groups, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_scores + (int64_t)done * k * gs, L.out_scores, cells * gs * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_ids + (int64_t)done * k * gs, L.out_ids, cells * gs * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (a.capped) {
                HIP_TRY(hipMemcpyAsync(cap_scores + (int64_t)done * k, L.cap_scores, cells * sizeof(float), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(cap_ids + (int64_t)done * k, L.cap_ids, cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            }
            return RASS_OK;
        },
        [&](HostSlot* sl, int done, int b) -> int {
            const GroupIoView H = group_io_layout(static_cast<unsigned char*>(sl->h_io));
            if (*H.status != 0)
                return fail(RASS_ERR_INVALID, "group-hits search: a matching row's group key is >= n_groups (" + std::to_string(a.n_groups) + ")");
            memcpy(out_total + done, H.total, (size_t)b * sizeof(int64_t));
            memcpy(out_groups + (int64_t)done * k, H.out_groups, (size_t)b * k * sizeof(int32_t));
            return RASS_OK;
        });
}

}  // namespace
}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_group_hits_keys(rass_index_t* idx, const float* queries, int nq, int k, const int32_t* d_keys, int64_t n_keys,
                                      int32_t n_groups, int group_size, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                      const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids,
                                      int32_t* out_groups, int64_t* out_group_total, float* out_capped_scores,
                                      int64_t* out_capped_ids) {
    if (!idx || !out_scores || !out_ids || !out_groups || !out_group_total) return fail(RASS_ERR_INVALID, "NULL argument");
    if ((out_capped_scores == nullptr) != (out_capped_ids == nullptr))
        return fail(RASS_ERR_INVALID, "out_capped_scores and out_capped_ids go together");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    const HitsArgs a{k, d_keys, n_keys, n_groups, group_size, d_allow, n_bitmaps, words_per_bitmap, q_filter, q_filter_mask,
                     out_capped_scores != nullptr};
    if (int rc = check_hits(idx, a, nq)) return rc;
    if (nq == 0) return RASS_OK;
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); }, [&] {
        return search_hits_once(idx, queries, nq, a, out_scores, out_ids, out_groups, out_group_total, out_capped_scores, out_capped_ids);
    });
}

int rass_index_search_group_hits_keys_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_keys,
                                             int64_t n_keys, int32_t n_groups, int group_size, const uint32_t* d_allow, int n_bitmaps,
                                             int64_t words_per_bitmap, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                             int64_t id_base, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_groups,
                                             int64_t* d_group_total, float* d_out_capped_scores, int64_t* d_out_capped_ids,
                                             int32_t* d_status) {
    if (!idx || !d_queries || !d_out_scores || !d_out_ids || !d_out_groups || !d_group_total || !d_status)
        return fail(RASS_ERR_INVALID, "NULL argument");
    if ((d_out_capped_scores == nullptr) != (d_out_capped_ids == nullptr))
        return fail(RASS_ERR_INVALID, "d_out_capped_scores and d_out_capped_ids go together");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    const HitsArgs a{k, d_keys, n_keys, n_groups, group_size, d_allow, n_bitmaps, words_per_bitmap, d_q_filter, d_q_filter_mask,
                     d_out_capped_scores != nullptr};
    if (int rc = check_hits(idx, a, nq)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    for (int done = 0; done < nq; done += RASS_MAX_QBATCH) {
        const int64_t cells = (int64_t)done * k;
        HitsRequest r;
        hits_request(r, a, done);
        r.queries = d_queries + (int64_t)done * idx->dim, r.nq = std::min(RASS_MAX_QBATCH, nq - done);
        r.q_filter = d_q_filter ? d_q_filter + done : nullptr, r.q_filter_mask = d_q_filter_mask ? d_q_filter_mask + done : nullptr;
        r.id_base = id_base;
        r.out_scores = d_out_scores + cells * group_size, r.out_ids = d_out_ids + cells * group_size;
        r.out_groups = d_out_groups + cells, r.total = d_group_total + done;
        if (a.capped) r.cap_scores = d_out_capped_scores + cells, r.cap_ids = d_out_capped_ids + cells;
        r.status = d_status, r.accumulate = done > 0;
        rc = hits_device_group(idx, r);
        if (rc != RASS_OK) return rc;
    }
    return RASS_OK;
}

}  // extern "C"
