// api_compact.hip — the C ABI of include/rass_engine.h: compaction of a flat index (rass_index_compact), its layout epoch
// and the stateless wrappers of the two kernels behind it (compact.hip).  Host-side C++ only.  The objects and the threading
// rules: api_internal.h.
//
// Out of place: a new set of slabs sized for the live rows is filled from the old one on the engine's stream and swapped in
// under idx->mu + eng->mu; every search enqueued earlier is ordered before the gather on that stream and has finished on the
// old slabs before they are freed.  A row ordinal is only meaningful together with the layout epoch: the host search entry
// points (api_search.hip) read it around their launch groups and run again when it moved.

#include "api_internal.h"

using namespace rass::host;

namespace {

// Everything a compaction allocates; what is still set when it goes out of scope is released.
struct CompactBlocks {
    void* main = nullptr;          // the dtype's own slab
    int32_t* tags = nullptr;
    int64_t* gid = nullptr;
    unsigned short* b16 = nullptr; // the candidate copies of an fp32 index
    signed char* i8 = nullptr;
    float* scale = nullptr;
    int32_t* attr[RASS_MAX_ATTRS] = {};   // the attribute columns the index has allocated
    int64_t *new_row = nullptr, *src_row = nullptr, *n_live = nullptr;
    void* ws = nullptr;
    ~CompactBlocks() {
        for (int32_t* p : attr)
            if (p) (void)hipFree(p);
        for (void* p : {main, (void*)tags, (void*)gid, (void*)b16, (void*)i8, (void*)scale, (void*)new_row, (void*)src_row,
                        (void*)n_live, ws})
            if (p) (void)hipFree(p);
    }
};

template <class T>
hipError_t dev_alloc(T** p, size_t bytes) {
    return hipMalloc(reinterpret_cast<void**>(p), bytes ? bytes : 1);
}

}  // namespace

extern "C" {

int64_t rass_index_layout_epoch(const rass_index_t* idx) { return idx ? idx->layout_epoch.load(std::memory_order_acquire) : 0; }

int rass_index_compact(rass_index_t* idx, int64_t* new_row_of, int64_t map_capacity, int64_t* rows_before,
                       int64_t* rows_after) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(idx->mu);
    const int64_t rows = idx->rows.load();
    const int64_t live = rows - idx->deleted.load();
    if (rows_before) *rows_before = rows;
    if (rows_after) *rows_after = rows;
    if (new_row_of && map_capacity < rows)
        return fail(RASS_ERR_INVALID, "map_capacity is smaller than the rows of the index (rass_index_rows)");
    if (live == rows) {   // no tombstone: identity, nothing moves, the layout epoch stays
        if (new_row_of)
            for (int64_t r = 0; r < rows; ++r) new_row_of[r] = r;
        return RASS_OK;
    }
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const bool f32 = idx->dtype == RASS_F32;
    const bool want_b16 = f32 && idx->prefilter == 1;
    const bool want_i8 = idx->prefilter >= 2;
    const size_t elem = f32 ? sizeof(float) : 2;
    const int64_t used = pad16(live);
    const int64_t cap = std::max<int64_t>(used, 1024);   // what index_reserve starts from; growth afterwards is its own

    // the whole enqueue + synchronise + swap under the engine lock: a search sees the old layout or the new one
    std::lock_guard<std::mutex> elk(eng->mu);
    hipStream_t st = eng->stream;
    CompactBlocks nb;
    hipError_t e = hipMalloc(&nb.main, (size_t)cap * idx->stride * elem);
    if (e == hipSuccess) e = dev_alloc(&nb.tags, (size_t)cap * sizeof(int32_t));
    if (e == hipSuccess) e = dev_alloc(&nb.gid, (size_t)cap * sizeof(int64_t));
    if (e == hipSuccess && want_b16) e = dev_alloc(&nb.b16, (size_t)cap * idx->stride * 2);
    if (e == hipSuccess && want_i8) e = dev_alloc(&nb.i8, (size_t)cap * idx->stride_i8);
    if (e == hipSuccess && want_i8) e = dev_alloc(&nb.scale, (size_t)cap * sizeof(float));
    for (int c = 0; e == hipSuccess && c < RASS_MAX_ATTRS; ++c)
        if (idx->d_attr[c]) e = dev_alloc(&nb.attr[c], (size_t)cap * sizeof(int32_t));
    if (e == hipSuccess) e = dev_alloc(&nb.new_row, (size_t)rows * sizeof(int64_t));
    if (e == hipSuccess) e = dev_alloc(&nb.src_row, (size_t)rows * sizeof(int64_t));   // rows, not live: in bounds whatever the tags say
    if (e == hipSuccess) e = dev_alloc(&nb.n_live, sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(&nb.ws, rass::compact_plan_workspace_bytes(rows));
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RASS_ERR_OOM : RASS_ERR_HIP,
                    std::string("compact: allocating the compacted index next to the old one failed: ") + hipGetErrorString(e));

    HIP_TRY(rass::launch_compact_plan(idx->d_tags, rows, nb.new_row, nb.src_row, nb.n_live, nb.ws, st));
    // The host's count sized src_row and the new slabs: nothing may be gathered through a plan that disagrees with it.
    int64_t n_live_dev = -1;
    HIP_TRY(hipMemcpyAsync(&n_live_dev, nb.n_live, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_live_dev != live) {
        char b[200];
        snprintf(b, sizeof(b), "compact: the device counts %lld live rows, the host %lld: the index is left as it was",
                 (long long)n_live_dev, (long long)live);
        return fail(RASS_ERR_HIP, b);
    }
    // rows past the last block the gather writes must read as finite zeros (see index_reserve)
    if (cap > used)
        HIP_TRY(hipMemsetAsync(static_cast<unsigned char*>(nb.main) + (size_t)used * idx->stride * elem, 0,
                               (size_t)(cap - used) * idx->stride * elem, st));
    if (f32)
        HIP_TRY(rass::launch_compact_rows_tile16(idx->d_rows, static_cast<float*>(nb.main), idx->stride, nb.src_row, live, rows, st));
    else
        HIP_TRY(rass::launch_compact_rows_tile16b(idx->d_rows_bf16, nb.main, idx->stride, nb.src_row, live, rows, st));
    HIP_TRY(rass::launch_gather_i32(idx->d_tags, nb.tags, nb.src_row, live, rows, st));
    // the attribute columns travel with their rows; the capacity past them reads MISSING, as after a growth
    for (int c = 0; c < RASS_MAX_ATTRS; ++c) {
        if (!nb.attr[c]) continue;
        HIP_TRY(rass::launch_gather_i32(idx->d_attr[c], nb.attr[c], nb.src_row, live, rows, st));
        HIP_TRY(rass::launch_fill_i32(nb.attr[c] + live, cap - live, RASS_ATTR_MISSING, st));
    }
    // the id a search reports: caller-assigned ids travel with their rows, plain ordinals are the new ordinals
    if (idx->has_gid.load()) HIP_TRY(rass::launch_gather_i64(idx->d_gid, nb.gid, nb.src_row, live, rows, st));
    else HIP_TRY(rass::launch_iota_i64(nb.gid, live, 0, st));
    if (want_b16) HIP_TRY(hipMemsetAsync(nb.b16, 0, (size_t)cap * idx->stride * 2, st));
    if (want_i8) {
        HIP_TRY(hipMemsetAsync(nb.i8, 0, (size_t)cap * idx->stride_i8, st));
        HIP_TRY(hipMemsetAsync(nb.scale, 0, (size_t)cap * sizeof(float), st));
    }
    if (new_row_of) HIP_TRY(hipMemcpyAsync(new_row_of, nb.new_row, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // swap; the candidate copies are rebuilt from the new fp32 slab by the converters that made them (the same bytes by
    // construction).  Mode 3's certificate maxima are monotone upper bounds over every row ever quantised: still valid.
    auto swap_slabs = [&] {
        std::swap(idx->d_tags, nb.tags);
        for (int c = 0; c < RASS_MAX_ATTRS; ++c) std::swap(idx->d_attr[c], nb.attr[c]);
        std::swap(idx->d_gid, nb.gid);
        std::swap(idx->d_rows_i8, nb.i8);
        std::swap(idx->d_row_scale, nb.scale);
        void* mine = nb.main;
        if (f32) {
            nb.main = idx->d_rows;
            idx->d_rows = static_cast<float*>(mine);
            std::swap(idx->d_rows_bf16, nb.b16);
        } else {
            nb.main = idx->d_rows_bf16;
            idx->d_rows_bf16 = static_cast<unsigned short*>(mine);
        }
    };
    swap_slabs();
    rc = index_refresh_copies(idx, 0, live, st);
    if (rc == RASS_OK) rc = HIP_RC(hipStreamSynchronize(st));
    if (rc != RASS_OK) {   // put the old layout back: the blocks `nb` holds now are the new ones and go with it
        const std::string why = rass_last_error();
        (void)hipStreamSynchronize(st);
        swap_slabs();
        return fail(rc, "compact: rebuilding the candidate copies failed, the index is left as it was: " + why);
    }
    idx->capacity = cap;
    idx->rows = live;
    idx->deleted = 0;
    idx->host_deleted.assign((size_t)((live + 7) / 8), 0);
    idx->layout_epoch.fetch_add(1, std::memory_order_release);
    if (rows_after) *rows_after = live;
    return RASS_OK;   // ~CompactBlocks frees the old slabs and the plan
}

size_t rass_compact_plan_workspace_bytes(int64_t n_rows) { return n_rows < 0 ? 0 : rass::compact_plan_workspace_bytes(n_rows); }

int rass_compact_plan(const int32_t* d_tags, int64_t n_rows, int64_t* d_new_row, int64_t* d_src_row, int64_t* d_n_live,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n_rows < 0) return fail(RASS_ERR_INVALID, "n_rows < 0");
    if (!d_n_live || !d_workspace) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_rows > 0 && (!d_tags || !d_new_row || !d_src_row)) return fail(RASS_ERR_INVALID, "NULL argument");
    if (workspace_bytes < rass::compact_plan_workspace_bytes(n_rows))
        return fail(RASS_ERR_INVALID, "workspace too small (rass_compact_plan_workspace_bytes)");
    HIP_TRY(rass::launch_compact_plan(d_tags, n_rows, d_new_row, d_src_row, d_n_live, d_workspace,
                                      reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_compact_rows_f32(const float* d_src, float* d_dst, int64_t row_stride, const int64_t* d_src_row, int64_t n_dst,
                          int64_t n_src_rows, void* stream) {
    if (n_dst < 0 || n_src_rows < 0 || row_stride < 128 || row_stride % 128 != 0) return fail(RASS_ERR_INVALID, "bad shape");
    if (n_dst > 0 && (!d_src || !d_dst || !d_src_row)) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_compact_rows_tile16(d_src, d_dst, row_stride, d_src_row, n_dst, n_src_rows,
                                             reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

}  // extern "C"
