// api.hip — the C ABI of include/rass_engine.h: the objects that own HBM and everything that is not a search.  The
// error text of a thread, the engine (create / destroy / stream), the flat index (open / drop / grow / add / delete / rows /
// prefilter modes / save / load), timers and the kernel-timing bracket's begin / end, the stateless wrappers around single
// kernels, k-means and the peer buffers.  Host-side C++ only; the kernels live in the other .hip files.
// The searches: api_search.hip and api_ivf.hip over api_scan.hip.  The objects and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    // A failed HIP call (e.g. an out-of-memory hipMalloc) stays behind as the runtime's "last error" and the
    // NEXT kernel launch's hipGetLastError() would report it as its own: every failure path ends here, clear it.
    (void)hipGetLastError();
    return code;
}


int hip_fail(hipError_t e, const char* expr, const char* file, int line) {
    char b[512];
    snprintf(b, sizeof(b), "%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
    return fail(e == hipErrorOutOfMemory ? RASS_ERR_OOM : RASS_ERR_HIP, b);
}

int check_nq(int nq) {
    return nq < 1 || nq > RASS_MAX_QBATCH ? fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_QBATCH]") : RASS_OK;
}
int check_k(int k) { return k < 1 || k > RASS_MAX_K ? fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K]") : RASS_OK; }

int device_cus(int device) {
    static std::mutex mu;
    static std::map<int, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(device);
    if (it != cache.end()) return it->second;
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    cache[device] = cus;
    return cus;
}

int set_device(const rass_engine* eng) {
    HIP_TRY(hipSetDevice(eng->device));
    return RASS_OK;
}

int index_reserve(rass_index* idx, int64_t need_rows) {
    if (need_rows <= idx->capacity) return RASS_OK;
    int64_t cap = std::max<int64_t>(idx->capacity * 2, std::max<int64_t>(need_rows, 1024));
    cap = pad16(cap);  // tile16: whole 16-row blocks
    float* nrows = nullptr;
    int32_t* ntags = nullptr;
    hipStream_t st = idx->eng->stream;
    const bool want_f32 = idx->dtype == RASS_F32;                  // a bf16 index holds the bf16 slab ONLY
    const bool want_b16 = idx->dtype == RASS_BF16 || idx->prefilter == 1;
    const bool want_i8 = idx->prefilter >= 2;
    const size_t elem = want_f32 ? sizeof(float) : 2;
    void* nmain = nullptr;  // the dtype's own slab
    hipError_t e = hipMalloc(&nmain, (size_t)cap * idx->stride * elem);
    if (e != hipSuccess) {
        // retry with the exact size before giving up
        cap = pad16(need_rows);
        e = hipMalloc(&nmain, (size_t)cap * idx->stride * elem);
        if (e != hipSuccess) return fail(RASS_ERR_OOM, "index grow: hipMalloc of corpus slab failed");
    }
    if (want_f32) nrows = static_cast<float*>(nmain);
    int64_t* ngid = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&ntags), (size_t)cap * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ngid), (size_t)cap * sizeof(int64_t));
    int32_t* nattr[RASS_MAX_ATTRS] = {};   // the attribute columns that exist grow with the rows
    auto free_nattr = [&] {
        for (int32_t* p : nattr)
            if (p) (void)hipFree(p);
    };
    for (int c = 0; e == hipSuccess && c < RASS_MAX_ATTRS; ++c)
        if (idx->d_attr[c]) e = hipMalloc(reinterpret_cast<void**>(&nattr[c]), (size_t)cap * sizeof(int32_t));
    if (e != hipSuccess) {
        (void)hipFree(nmain);
        if (ntags) (void)hipFree(ntags);
        if (ngid) (void)hipFree(ngid);
        free_nattr();
        return fail(RASS_ERR_OOM, "index grow: hipMalloc of tag / id / attribute arrays failed");
    }
    // rows of a block past the last appended one must read as finite zeros (they are masked,
    // never ranked): zero the part of the slab the copy below does not overwrite
    const int64_t used_rows = pad16(idx->rows);
    unsigned short* nb16 = want_f32 ? nullptr : static_cast<unsigned short*>(nmain);
    signed char* ni8 = nullptr;
    float* nscale = nullptr;
    auto copy_over = [&]() -> hipError_t {
        hipError_t c = hipSuccess;
        if (want_f32) {
            c = hipMemsetAsync(nrows + used_rows * idx->stride, 0, (size_t)(cap - used_rows) * idx->stride * sizeof(float), st);
            if (c == hipSuccess && idx->rows > 0)
                c = hipMemcpyAsync(nrows, idx->d_rows, (size_t)used_rows * idx->stride * sizeof(float),
                                   hipMemcpyDeviceToDevice, st);
        }
        if (c == hipSuccess && idx->rows > 0)
            c = hipMemcpyAsync(ntags, idx->d_tags, (size_t)idx->rows * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (c == hipSuccess && idx->rows > 0)
            c = hipMemcpyAsync(ngid, idx->d_gid, (size_t)idx->rows * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
        for (int a = 0; c == hipSuccess && a < RASS_MAX_ATTRS; ++a) {   // the old rows' values, MISSING in the new capacity
            if (!nattr[a]) continue;
            c = rass::launch_fill_i32(nattr[a] + idx->rows, cap - idx->rows, RASS_ATTR_MISSING, st);
            if (c == hipSuccess && idx->rows > 0)
                c = hipMemcpyAsync(nattr[a], idx->d_attr[a], (size_t)idx->rows * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        }
        if (c == hipSuccess && want_b16) {
            if (want_f32) c = hipMalloc(reinterpret_cast<void**>(&nb16), (size_t)cap * idx->stride * 2);
            if (c == hipSuccess) c = hipMemsetAsync(nb16, 0, (size_t)cap * idx->stride * 2, st);
            if (c == hipSuccess && idx->rows > 0)
                c = hipMemcpyAsync(nb16, idx->d_rows_bf16, (size_t)used_rows * idx->stride * 2,
                                   hipMemcpyDeviceToDevice, st);
        }
        if (c == hipSuccess && want_i8) {
            c = hipMalloc(reinterpret_cast<void**>(&ni8), (size_t)cap * idx->stride_i8);
            if (c == hipSuccess) c = hipMalloc(reinterpret_cast<void**>(&nscale), (size_t)cap * sizeof(float));
            if (c == hipSuccess) c = hipMemsetAsync(ni8, 0, (size_t)cap * idx->stride_i8, st);
            if (c == hipSuccess) c = hipMemsetAsync(nscale, 0, (size_t)cap * sizeof(float), st);
            if (c == hipSuccess && idx->rows > 0)
                c = hipMemcpyAsync(ni8, idx->d_rows_i8, (size_t)used_rows * idx->stride_i8, hipMemcpyDeviceToDevice, st);
            if (c == hipSuccess && idx->rows > 0)
                c = hipMemcpyAsync(nscale, idx->d_row_scale, (size_t)used_rows * sizeof(float), hipMemcpyDeviceToDevice, st);
        }
        if (c == hipSuccess) c = hipStreamSynchronize(st);
        return c;
    };
    e = copy_over();
    if (e != hipSuccess) {  // nothing of the old index was touched: release the new allocations and report
        (void)hipStreamSynchronize(st);
        (void)hipFree(nmain);
        (void)hipFree(ntags);
        (void)hipFree(ngid);
        free_nattr();
        if (nb16 && want_f32) (void)hipFree(nb16);
        if (ni8) (void)hipFree(ni8);
        if (nscale) (void)hipFree(nscale);
        return fail(e == hipErrorOutOfMemory ? RASS_ERR_OOM : RASS_ERR_HIP,
                    std::string("index grow failed: ") + hipGetErrorString(e));
    }
    if (idx->d_rows) (void)hipFree(idx->d_rows);
    if (idx->d_tags) (void)hipFree(idx->d_tags);
    if (idx->d_gid) (void)hipFree(idx->d_gid);
    if (idx->d_rows_bf16) (void)hipFree(idx->d_rows_bf16);
    if (idx->d_rows_i8) (void)hipFree(idx->d_rows_i8);
    if (idx->d_row_scale) (void)hipFree(idx->d_row_scale);
    idx->d_rows_i8 = ni8;
    idx->d_row_scale = nscale;
    idx->d_rows = nrows;
    idx->d_tags = ntags;
    idx->d_gid = ngid;
    for (int a = 0; a < RASS_MAX_ATTRS; ++a) {
        if (idx->d_attr[a]) (void)hipFree(idx->d_attr[a]);
        idx->d_attr[a] = nattr[a];
    }
    idx->d_rows_bf16 = nb16;
    idx->capacity = cap;
    return RASS_OK;
}

void index_free_slabs(rass_index* idx) {
    for (void* p : {(void*)idx->d_rows, (void*)idx->d_tags, (void*)idx->d_gid, (void*)idx->d_rows_bf16, (void*)idx->d_rows_i8,
                    (void*)idx->d_row_scale, (void*)idx->d_cert_stats, (void*)idx->d_cert_counts})
        if (p) (void)hipFree(p);
    idx->d_rows = nullptr, idx->d_tags = nullptr, idx->d_gid = nullptr, idx->d_rows_bf16 = nullptr;
    idx->d_rows_i8 = nullptr, idx->d_row_scale = nullptr, idx->d_cert_stats = nullptr, idx->d_cert_counts = nullptr;
    for (int32_t*& p : idx->d_attr) {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
}

// Attribute column `col` exists afterwards: allocated over the whole capacity and filled with RASS_ATTR_MISSING on first use.
// The caller holds idx->mu and eng->mu (a bitmap builder reads the pointer under eng->mu).
int index_attr_ensure(rass_index* idx, int col) {
    if (idx->d_attr[col]) return RASS_OK;
    if (idx->capacity == 0) {
        if (int rc = index_reserve(idx, 1)) return rc;
    }
    int32_t* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), (size_t)idx->capacity * sizeof(int32_t)) != hipSuccess)
        return fail(RASS_ERR_OOM, "attribute column: hipMalloc failed");
    const hipError_t e = rass::launch_fill_i32(p, idx->capacity, RASS_ATTR_MISSING, idx->eng->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "launch_fill_i32", __FILE__, __LINE__);
    }
    idx->d_attr[col] = p;
    return RASS_OK;
}

// The candidate copies of rows [first, first + n) that the index's prefilter mode keeps next to the fp32 slab.
int index_refresh_copies(rass_index* idx, int64_t first, int64_t n, hipStream_t st) {
    if (idx->prefilter == 1 && idx->dtype == RASS_F32)
        HIP_TRY(rass::launch_convert_tile16_bf16(idx->d_rows, idx->d_rows_bf16, idx->stride, first >> 4, (first + n + 15) >> 4, st));
    if (idx->prefilter >= 2)   // whole blocks: the earlier rows of a partially filled block quantise to the same bytes again
        HIP_TRY(rass::launch_quantize_tile16_i8(idx->d_rows, idx->d_rows_i8, idx->d_row_scale, idx->stride, idx->stride_i8,
                                                first >> 4, (first + n + 15) >> 4, st,
                                                idx->prefilter == 3 ? idx->d_cert_stats : nullptr));
    return RASS_OK;
}

// Rows [first, first + n) of the index, unpacked row-major into the engine's staging buffer (the caller holds eng->mu).
hipError_t index_unpack_to_stage(rass_index* idx, int64_t first, int64_t n, hipStream_t st) {
    if (idx->dtype == RASS_BF16)
        return rass::launch_unpack_rows_tile16b(idx->d_rows_bf16, idx->stride, first, n, idx->dim, idx->eng->d_stage, idx->dim, st);
    return rass::launch_unpack_rows_tile16(idx->d_rows, idx->stride, first, n, idx->dim, idx->eng->d_stage, idx->dim, st);
}

}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" void rassint_set_last_error(const char* msg) { g_err = msg ? msg : ""; }

extern "C" {

int rass_abi_version(void) { return RASS_ABI_VERSION; }

const char* rass_last_error(void) { return g_err.c_str(); }

int rass_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(RASS_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

int rass_engine_create(int device, int dim, rass_engine_t** out) {
    if (out == nullptr) return fail(RASS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (dim < 1 || pad_stride(dim) > kMaxStride)
        return fail(RASS_ERR_UNSUPPORTED, "dim must be in [1, 2048] for the fused scan");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(RASS_ERR_INVALID, "no such HIP device");
    rass_engine* eng = new (std::nothrow) rass_engine();
    if (!eng) return fail(RASS_ERR_OOM, "host allocation failed");
    eng->device = device;
    eng->dim = dim;
    auto init = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        eng->n_cus = device_cus(device);
        HIP_TRY(hipStreamCreateWithFlags(&eng->own_stream, hipStreamNonBlocking));
        eng->stream = eng->own_stream;
        eng->scratch_bytes = scratch_layout(nullptr, RASS_MAX_QBATCH, RASS_MAX_K).total;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_scratch), eng->scratch_bytes));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_qraw), (size_t)RASS_MAX_QBATCH * dim * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_qfilter), RASS_MAX_QBATCH * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_out_scores), RASS_MAX_QBATCH * RASS_MAX_K * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_out_ids), RASS_MAX_QBATCH * RASS_MAX_K * sizeof(int64_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_stage), (size_t)kStageRows * dim * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_stage_tags), (size_t)kStageRows * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_qmask), RASS_MAX_QBATCH * sizeof(int32_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_after_s), RASS_MAX_QBATCH * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_after_i), RASS_MAX_QBATCH * sizeof(int64_t)));
        eng->slots.resize(kHostSlots);
        for (HostSlot& sl : eng->slots) {
            // one pinned block per slot: [out_i 32x32 i64][after_i 32 i64][scanned i64][q 32xdim f32][out_s][after_s][filter][mask]
            const size_t B = RASS_MAX_QBATCH, K = RASS_MAX_K;
            const size_t bytes = B * K * 8 + B * 8 + 8 + B * (size_t)dim * 4 + B * K * 4 + B * 4 + B * 4 + B * 4;
            HIP_TRY(hipHostMalloc(&sl.base, bytes, hipHostMallocDefault));
            unsigned char* p = static_cast<unsigned char*>(sl.base);
            sl.h_out_i = reinterpret_cast<int64_t*>(p), p += B * K * 8;
            sl.h_after_i = reinterpret_cast<int64_t*>(p), p += B * 8;
            sl.h_scanned = reinterpret_cast<int64_t*>(p), p += 8;
            sl.h_q = reinterpret_cast<float*>(p), p += B * (size_t)dim * 4;
            sl.h_out_s = reinterpret_cast<float*>(p), p += B * K * 4;
            sl.h_after_s = reinterpret_cast<float*>(p), p += B * 4;
            sl.h_filter = reinterpret_cast<int32_t*>(p), p += B * 4;
            sl.h_mask = reinterpret_cast<int32_t*>(p), p += B * 4;
            HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        }
        return RASS_OK;
    };
    const int rc = init();
    if (rc != RASS_OK) {
        const std::string why = g_err;  // destroy() must not lose the reason
        rass_engine_destroy(eng);
        return fail(rc, why);
    }
    *out = eng;
    return RASS_OK;
}

void rass_engine_destroy(rass_engine_t* eng) {
    if (!eng) return;
    (void)hipSetDevice(eng->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : eng->indices) {
        rass_index* idx = kv.second;
        index_free_slabs(idx);
        delete idx;
    }
    eng->indices.clear();
    for (void* p : {(void*)eng->d_scratch, (void*)eng->d_batch, (void*)eng->d_cert, (void*)eng->d_io, (void*)eng->d_group, (void*)eng->d_allow, (void*)eng->d_allow_io, (void*)eng->d_mmr, (void*)eng->d_qraw, (void*)eng->d_qfilter,
                    (void*)eng->d_out_scores, (void*)eng->d_out_ids, (void*)eng->d_stage, (void*)eng->d_stage_tags,
                    (void*)eng->d_stage_t16, (void*)eng->d_mw_tile, (void*)eng->d_mw_rows, (void*)eng->d_mw_n, (void*)eng->d_mw_mask,
                    (void*)eng->d_mw_base, (void*)eng->d_mw_tags, (void*)eng->d_qmask, (void*)eng->d_after_s, (void*)eng->d_after_i})
        if (p) (void)hipFree(p);
    for (HostSlot& sl : eng->slots) {
        if (sl.base) (void)hipHostFree(sl.base);
        if (sl.h_items) (void)hipHostFree(sl.h_items);
        if (sl.h_io) (void)hipHostFree(sl.h_io);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    for (hipEvent_t e : eng->ev_pool) (void)hipEventDestroy(e);
    if (eng->own_stream) (void)hipStreamDestroy(eng->own_stream);
    delete eng;
}

int rass_engine_dim(const rass_engine_t* eng) { return eng ? eng->dim : fail(RASS_ERR_INVALID, "engine is NULL"); }
int rass_engine_device(const rass_engine_t* eng) {
    return eng ? eng->device : fail(RASS_ERR_INVALID, "engine is NULL");
}

int rass_engine_set_stream(rass_engine_t* eng, void* stream) {
    if (!eng) return fail(RASS_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(eng->mu);
    HIP_TRY(hipSetDevice(eng->device));
    HIP_TRY(hipStreamSynchronize(eng->stream));
    eng->stream = reinterpret_cast<hipStream_t>(stream);
    return RASS_OK;
}

int rass_engine_reset_stream(rass_engine_t* eng) {
    if (!eng) return fail(RASS_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(eng->mu);
    HIP_TRY(hipSetDevice(eng->device));
    HIP_TRY(hipStreamSynchronize(eng->stream));
    eng->stream = eng->own_stream;
    return RASS_OK;
}

void* rass_engine_get_stream(rass_engine_t* eng) { return eng ? reinterpret_cast<void*>(eng->stream) : nullptr; }

int rass_engine_synchronize(rass_engine_t* eng) {
    if (!eng) return fail(RASS_ERR_INVALID, "engine is NULL");
    HIP_TRY(hipSetDevice(eng->device));
    HIP_TRY(hipStreamSynchronize(eng->stream));
    return RASS_OK;
}

int rass_index_open(rass_engine_t* eng, const char* name, rass_dtype dtype, int64_t initial_capacity_rows,
                    rass_index_t** out) {
    if (!eng || !name || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (dtype != RASS_F32 && dtype != RASS_BF16) return fail(RASS_ERR_INVALID, "unknown corpus dtype");
    if (dtype == RASS_BF16 && pad128(eng->dim) % 256 != 0)
        return fail(RASS_ERR_UNSUPPORTED, "a bf16 corpus needs dim padded to a multiple of 256 (the bf16 scan's K split)");
    if (dtype == RASS_BF16 && eng->dim > kNarrowStride)
        return fail(RASS_ERR_UNSUPPORTED, "a bf16 corpus needs dim <= 1024 (wide rows are served by the fp32 scan only)");
    std::lock_guard<std::mutex> lk(eng->mu);
    auto it = eng->indices.find(name);
    if (it != eng->indices.end()) {
        if (it->second->dtype != dtype) return fail(RASS_ERR_INVALID, "index exists with another dtype");
        *out = it->second;
        return RASS_OK;
    }
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    rass_index* idx = new (std::nothrow) rass_index();
    if (!idx) return fail(RASS_ERR_OOM, "host allocation failed");
    idx->eng = eng;
    idx->name = name;
    idx->dtype = dtype;
    idx->dim = eng->dim;
    idx->stride = pad_stride(eng->dim);
    if (initial_capacity_rows > 0) {
        rc = index_reserve(idx, initial_capacity_rows);
        if (rc != RASS_OK) {
            delete idx;
            return rc;
        }
    }
    eng->indices[name] = idx;
    *out = idx;
    return RASS_OK;
}

int rass_index_drop(rass_engine_t* eng, const char* name) {
    if (!eng || !name) return fail(RASS_ERR_INVALID, "NULL argument");
    std::unique_lock<std::mutex> lk(eng->mu);
    auto it = eng->indices.find(name);
    if (it == eng->indices.end()) return fail(RASS_ERR_NOT_FOUND, "no such index");
    HIP_TRY(hipSetDevice(eng->device));
    rass_index* idx = it->second;
    eng->indices.erase(it);
    lk.unlock();
    {   // an add / delete / get_row / save that already holds the index runs to its end first (lock order
        // everywhere: index mutex, then engine mutex).  Using the handle AFTER drop returns is the caller's bug.
        std::lock_guard<std::mutex> ilk(idx->mu);
        std::lock_guard<std::mutex> elk(eng->mu);
        (void)hipStreamSynchronize(eng->stream);
        index_free_slabs(idx);
    }
    delete idx;
    return RASS_OK;
}

int rass_index_set_prefilter(rass_index_t* idx, int enable) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    if (enable < 0 || enable > 3)
        return fail(RASS_ERR_INVALID, "prefilter mode must be 0 (off), 1 (bf16), 2 (int8) or 3 (int8, certified exact)");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(idx->mu);
    std::lock_guard<std::mutex> elk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    if (enable && idx->dtype == RASS_BF16) return fail(RASS_ERR_UNSUPPORTED, "a bf16 corpus IS the bf16 scan: no prefilter mode");
    if (enable == idx->prefilter) return RASS_OK;
    if (enable == 1 && idx->stride % 256 != 0) return fail(RASS_ERR_UNSUPPORTED, "prefilter needs dim padded to a multiple of 256");
    if (enable == 1 && idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "the bf16 prefilter needs dim <= 1024 (wide rows: int8 candidates or the fp32 flat scan)");
    // leave the current mode (a switch between the two candidate copies goes through "off")
    HIP_TRY(hipStreamSynchronize(st));
    if (idx->d_rows_bf16) (void)hipFree(idx->d_rows_bf16);
    if (idx->d_rows_i8) (void)hipFree(idx->d_rows_i8);
    if (idx->d_row_scale) (void)hipFree(idx->d_row_scale);
    idx->d_rows_bf16 = nullptr;
    idx->d_rows_i8 = nullptr;
    idx->d_row_scale = nullptr;
    idx->prefilter = 0;
    if (!enable) return RASS_OK;
    if (enable == 1 && idx->capacity > 0) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&idx->d_rows_bf16), (size_t)idx->capacity * idx->stride * 2));
        HIP_TRY(hipMemsetAsync(idx->d_rows_bf16, 0, (size_t)idx->capacity * idx->stride * 2, st));
        HIP_TRY(rass::launch_convert_tile16_bf16(idx->d_rows, idx->d_rows_bf16, idx->stride, 0, (idx->rows + 15) >> 4,
                                                 st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (enable == 3) {   // the certificate's row maxima are recomputed from the rows; the counters start at zero
        if (!idx->d_cert_stats) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&idx->d_cert_stats), 3 * sizeof(unsigned)));
        if (!idx->d_cert_counts) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&idx->d_cert_counts), 3 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(idx->d_cert_stats, 0, 3 * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(idx->d_cert_counts, 0, 3 * sizeof(unsigned long long), st));
    }
    if (enable >= 2) {
        idx->stride_i8 = pad512(idx->stride);
        if (idx->capacity > 0) {
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&idx->d_rows_i8), (size_t)idx->capacity * idx->stride_i8));
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&idx->d_row_scale), (size_t)idx->capacity * sizeof(float)));
            HIP_TRY(hipMemsetAsync(idx->d_rows_i8, 0, (size_t)idx->capacity * idx->stride_i8, st));
            HIP_TRY(hipMemsetAsync(idx->d_row_scale, 0, (size_t)idx->capacity * sizeof(float), st));
            HIP_TRY(rass::launch_quantize_tile16_i8(idx->d_rows, idx->d_rows_i8, idx->d_row_scale, idx->stride, idx->stride_i8, 0,
                                                    (idx->rows + 15) >> 4, st, enable == 3 ? idx->d_cert_stats : nullptr));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    idx->prefilter = enable;
    return RASS_OK;
}

int rass_index_get_prefilter(const rass_index_t* idx) { return idx ? idx->prefilter : 0; }

int64_t rass_index_count(const rass_index_t* idx) { return idx ? idx->rows.load() - idx->deleted.load() : 0; }
int64_t rass_index_rows(const rass_index_t* idx) { return idx ? idx->rows.load() : (int64_t)0; }
int rass_index_dim(const rass_index_t* idx) { return idx ? idx->dim : fail(RASS_ERR_INVALID, "index is NULL"); }
int rass_index_dtype(const rass_index_t* idx) { return idx ? (int)idx->dtype : fail(RASS_ERR_INVALID, "index is NULL"); }
int rass_index_has_global_ids(const rass_index_t* idx) {
    return idx ? (idx->has_gid.load() ? 1 : 0) : fail(RASS_ERR_INVALID, "index is NULL");
}
int rass_index_row_stride(const rass_index_t* idx) {
    return idx ? (int)idx->stride : fail(RASS_ERR_INVALID, "index is NULL");
}

static int add_common(rass_index_t* idx, const float* vecs, const int32_t* tags, int64_t n, int normalize,
                      int64_t* first_row, bool device_src, int64_t first_global_id = -1) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    if (n < 0 || (n > 0 && !vecs)) return fail(RASS_ERR_INVALID, "bad vecs / n");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(idx->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    if (!device_src && tags) {
        for (int64_t i = 0; i < n; ++i)
            if (tags[i] < 0) return fail(RASS_ERR_INVALID, "row tags must be >= 0");
    }
    if (first_row) *first_row = idx->rows;
    if (n == 0) return RASS_OK;
    {
        std::lock_guard<std::mutex> elk(eng->mu);  // grow swaps pointers searches read
        rc = index_reserve(idx, idx->rows + n);
        if (rc != RASS_OK) return rc;
    }
    hipStream_t st = eng->stream;
    const int dim = idx->dim;
    for (int64_t done = 0; done < n;) {
        const int64_t m = std::min<int64_t>(kStageRows, n - done);
        int32_t* tdst = idx->d_tags + idx->rows + done;
        const float* src = vecs + done * dim;
        const float* dsrc = src;
        // host source: the staging buffer is ENGINE scratch, shared with the other indices (users) of
        // this engine and with get_row(s) / save — hold the engine lock for the chunk's round trip
        std::unique_lock<std::mutex> elk(eng->mu, std::defer_lock);
        if (!device_src) elk.lock();
        if (!device_src) {
            HIP_TRY(hipMemcpyAsync(eng->d_stage, src, (size_t)m * dim * sizeof(float), hipMemcpyHostToDevice, st));
            dsrc = eng->d_stage;
        }
        if (idx->dtype == RASS_BF16) {
            // normalise + pack into the fp32 staging slab at the destination's phase inside a 16-row block, then round
            // the chunk's rows (and only them) into the bf16 slab
            if (!elk.owns_lock()) elk.lock();
            if (!eng->d_stage_t16)
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_stage_t16), (size_t)(kStageRows + 32) * kMaxStride * sizeof(float)));
            const int64_t at = idx->rows + done, phase = at & 15;
            HIP_TRY(rass::launch_pack_rows_tile16(dsrc, dim, eng->d_stage_t16, idx->stride, phase, m, dim,
                                                  normalize ? 1 : 0, st));
            HIP_TRY(rass::launch_convert_tile16_bf16(eng->d_stage_t16, idx->d_rows_bf16, idx->stride, at >> 4,
                                                     (at + m + 15) >> 4, st, 0, at, at + m));
        } else
        HIP_TRY(rass::launch_pack_rows_tile16(dsrc, dim, idx->d_rows, idx->stride, idx->rows + done, m, dim,
                                              normalize ? 1 : 0, st));
        if (tags && device_src) {
            HIP_TRY(rass::launch_copy_tags_clamped(tdst, tags + done, m, st));
        } else if (tags) {
            HIP_TRY(hipMemcpyAsync(tdst, tags + done, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(rass::launch_fill_i32(tdst, m, 0, st));
        }
        // the staging buffer is reused by the next chunk
        if (!device_src || idx->dtype == RASS_BF16) HIP_TRY(hipStreamSynchronize(st));
        done += m;
    }
    rc = index_refresh_copies(idx, idx->rows, n, st);
    if (rc != RASS_OK) return rc;
    // the id a search reports for these rows: their ordinal, or the caller's global ids (ascending with the
    // ordinal, so the (score desc, id asc) tie order inside the shard is the global one)
    HIP_TRY(rass::launch_iota_i64(idx->d_gid + idx->rows, n, first_global_id >= 0 ? first_global_id : idx->rows.load(), st));
    if (first_global_id >= 0 && first_global_id != idx->rows) idx->has_gid = true;
    if (tags) idx->has_tags = true;
    idx->rows += n;
    idx->host_deleted.resize((size_t)((idx->rows + 7) / 8), 0);
    return RASS_OK;
}

int rass_index_add(rass_index_t* idx, const float* vecs, const int32_t* tags, int64_t n, int normalize,
                   int64_t* first_row) {
    return add_common(idx, vecs, tags, n, normalize, first_row, false);
}

int rass_index_add_device(rass_index_t* idx, const float* d_vecs, const int32_t* d_tags, int64_t n, int normalize,
                          int64_t* first_row) {
    return add_common(idx, d_vecs, d_tags, n, normalize, first_row, true);
}

int rass_index_add_ex(rass_index_t* idx, const float* vecs, const int32_t* tags, int64_t n, int normalize,
                      int64_t first_global_id, int device_source, int64_t* first_row) {
    if (first_global_id < -1) return fail(RASS_ERR_INVALID, "first_global_id must be >= 0, or -1 for row ordinals");
    return add_common(idx, vecs, tags, n, normalize, first_row, device_source != 0, first_global_id);
}

int rass_index_delete(rass_index_t* idx, int64_t row) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (row < 0 || row >= idx->rows) return fail(RASS_ERR_NOT_FOUND, "row out of range");
    uint8_t& byte = idx->host_deleted[(size_t)(row >> 3)];
    const uint8_t bit = (uint8_t)(1u << (row & 7));
    if (byte & bit) return RASS_OK;  // idempotent
    int rc = set_device(idx->eng);
    if (rc != RASS_OK) return rc;
    {
        // A search holds eng->mu for its whole enqueue sequence (sample-floor pass, scan, further passes of a k > 32
        // search): without it this fill could land BETWEEN them — the floor was computed from k rows, one of which is
        // now a tombstone, and the scan would reject live rows below it and return fewer than k hits.  Lock order
        // idx->mu then eng->mu, as in add_common: a search sees a tombstone before its first pass or after its merge.
        std::lock_guard<std::mutex> elk(idx->eng->mu);
        HIP_TRY(rass::launch_fill_i32(idx->d_tags + row, 1, RASS_ROW_TAG_DELETED, idx->eng->stream));
    }
    byte |= bit;
    idx->deleted += 1;
    return RASS_OK;
}

int rass_index_get_row(rass_index_t* idx, int64_t row, float* out) {
    if (!idx || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (row < 0 || row >= idx->rows) return fail(RASS_ERR_NOT_FOUND, "row out of range");
    int rc = set_device(idx->eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = idx->eng->stream;
    {
        std::lock_guard<std::mutex> elk(idx->eng->mu);  // d_stage is shared engine scratch
        HIP_TRY(index_unpack_to_stage(idx, row, 1, st));
        HIP_TRY(hipMemcpyAsync(out, idx->eng->d_stage, (size_t)idx->dim * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RASS_OK;
}

int rass_index_get_rows(rass_index_t* idx, int64_t first_row, int64_t n, float* out) {
    if (!idx || (n > 0 && !out)) return fail(RASS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (first_row < 0 || n < 0 || first_row + n > idx->rows) return fail(RASS_ERR_NOT_FOUND, "rows out of range");
    int rc = set_device(idx->eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = idx->eng->stream;
    std::lock_guard<std::mutex> elk(idx->eng->mu);  // d_stage is shared engine scratch
    for (int64_t done = 0; done < n; done += kStageRows) {
        const int64_t m = std::min<int64_t>(kStageRows, n - done);
        HIP_TRY(index_unpack_to_stage(idx, first_row + done, m, st));
        HIP_TRY(hipMemcpyAsync(out + done * idx->dim, idx->eng->d_stage, (size_t)m * idx->dim * sizeof(float),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return RASS_OK;
}

// ---- persistence: header + unpadded fp32 rows + tags [+ ids] [+ attribute columns]
// SaveHeader.reserved: bit 0 = rows x int64 caller-assigned ids follow the tags; bit 1 = the attribute section follows
// them: int32 n_cols, then per allocated column int32 col and rows x int32 values.  No column: today's bytes.
struct SaveHeader {
    char magic[8];
    int32_t version;
    int32_t dim;
    int32_t dtype;
    int32_t reserved;
    int64_t rows;
    int64_t deleted;
};

int rass_index_save(rass_index_t* idx, const char* path) {
    if (!idx || !path) return fail(RASS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(idx->mu);
    int rc = set_device(idx->eng);
    if (rc != RASS_OK) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) return fail(RASS_ERR_IO, std::string("cannot open for write: ") + path);
    SaveHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "RASSIDX1", 8);
    h.version = 1;
    h.dim = idx->dim;
    h.dtype = (int32_t)idx->dtype;
    h.rows = idx->rows;
    h.deleted = idx->deleted;
    const bool save_gid = idx->has_gid.load();
    int attr_cols = 0;
    for (const int32_t* col : idx->d_attr) attr_cols += col ? 1 : 0;
    h.reserved = (save_gid ? 1 : 0) | (attr_cols ? 2 : 0);
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    hipStream_t st = idx->eng->stream;
    std::vector<float> buf((size_t)kStageRows * idx->dim);
    for (int64_t r = 0; ok && r < idx->rows; r += kStageRows) {
        const int64_t m = std::min<int64_t>(kStageRows, idx->rows - r);
        std::lock_guard<std::mutex> elk(idx->eng->mu);  // d_stage is shared engine scratch
        hipError_t e = index_unpack_to_stage(idx, r, m, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(buf.data(), idx->eng->d_stage, (size_t)m * idx->dim * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            fclose(f);
            return fail(RASS_ERR_HIP, std::string("save: device read failed: ") + hipGetErrorString(e));
        }
        ok = fwrite(buf.data(), sizeof(float), (size_t)m * idx->dim, f) == (size_t)m * idx->dim;
    }
    if (ok && idx->rows > 0) {
        std::vector<int32_t> tags((size_t)idx->rows);
        hipError_t e = hipMemcpyAsync(tags.data(), idx->d_tags, (size_t)idx->rows * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            fclose(f);
            return fail(RASS_ERR_HIP, std::string("save: tag read failed: ") + hipGetErrorString(e));
        }
        ok = fwrite(tags.data(), 4, (size_t)idx->rows, f) == (size_t)idx->rows;
    }
    if (ok && idx->rows > 0 && save_gid) {
        std::vector<int64_t> gids((size_t)idx->rows);
        hipError_t e = hipMemcpyAsync(gids.data(), idx->d_gid, (size_t)idx->rows * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            fclose(f);
            return fail(RASS_ERR_HIP, std::string("save: id read failed: ") + hipGetErrorString(e));
        }
        ok = fwrite(gids.data(), 8, (size_t)idx->rows, f) == (size_t)idx->rows;
    }
    if (ok && attr_cols) {
        const int32_t n_cols = attr_cols;
        ok = fwrite(&n_cols, 4, 1, f) == 1;
        std::vector<int32_t> vals((size_t)idx->rows);
        for (int32_t c = 0; ok && c < RASS_MAX_ATTRS; ++c) {
            if (!idx->d_attr[c]) continue;
            hipError_t e = hipSuccess;
            if (idx->rows > 0) e = hipMemcpyAsync(vals.data(), idx->d_attr[c], (size_t)idx->rows * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                fclose(f);
                return fail(RASS_ERR_HIP, std::string("save: attribute read failed: ") + hipGetErrorString(e));
            }
            ok = fwrite(&c, 4, 1, f) == 1 && fwrite(vals.data(), 4, (size_t)idx->rows, f) == (size_t)idx->rows;
        }
    }
    // durable before the caller renames it into place (docstore.py's manifest scheme)
    ok = ok && fflush(f) == 0 && fsync(fileno(f)) == 0;
    ok = (fclose(f) == 0) && ok;
    return ok ? RASS_OK : fail(RASS_ERR_IO, std::string("short write: ") + path);
}

int rass_index_load(rass_engine_t* eng, const char* name, const char* path, rass_index_t** out) {
    if (!eng || !name || !path || !out) return fail(RASS_ERR_INVALID, "NULL argument");
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return fail(RASS_ERR_IO, std::string("cannot open for read: ") + path);
    SaveHeader h;
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "RASSIDX1", 8) != 0 || h.version != 1) {
        fclose(f);
        return fail(RASS_ERR_IO, "not a rass index file");
    }
    if (h.dim != eng->dim || (h.dtype != RASS_F32 && h.dtype != RASS_BF16) || h.rows < 0 || (h.reserved & ~3) != 0) {
        fclose(f);
        return fail(RASS_ERR_INVALID, "index file does not match the engine (dim / dtype)");
    }
    {   // the header's row count must agree with the file length before anything is allocated from it
        const long body = ftell(f);
        int64_t file_len = -1;
        if (body >= 0 && fseek(f, 0, SEEK_END) == 0) file_len = (int64_t)ftell(f);
        int64_t need = (int64_t)sizeof(SaveHeader) + h.rows * ((int64_t)h.dim * 4 + 4 + ((h.reserved & 1) ? 8 : 0));
        bool bad = body < 0 || h.rows > ((int64_t)1 << 40) || file_len < need;
        if (!bad && (h.reserved & 2)) {   // the attribute section's own count sizes the rest of it
            int32_t n_cols = 0;
            bad = file_len < need + 4 || fseek(f, (long)need, SEEK_SET) != 0 || fread(&n_cols, 4, 1, f) != 1 || n_cols < 1 ||
                  n_cols > RASS_MAX_ATTRS;
            need += 4 + (int64_t)n_cols * (4 + h.rows * 4);
            bad = bad || file_len < need;
        }
        if (bad || fseek(f, body, SEEK_SET) != 0) {
            fclose(f);
            return fail(RASS_ERR_IO, "truncated index file (shorter than its header says)");
        }
    }
    {
        std::lock_guard<std::mutex> lk(eng->mu);
        if (eng->indices.count(name)) {
            fclose(f);
            return fail(RASS_ERR_INVALID, "an index of that name is already open");
        }
    }
    rass_index_t* idx = nullptr;
    int rc = rass_index_open(eng, name, (rass_dtype)h.dtype, h.rows, &idx);  // a bf16 corpus was saved as its exact
                                                                              // fp32 upcast: re-rounding is lossless
    if (rc != RASS_OK) {
        fclose(f);
        return rc;
    }
    std::vector<float> buf((size_t)kStageRows * h.dim);
    for (int64_t r = 0; r < h.rows; r += kStageRows) {
        const int64_t m = std::min<int64_t>(kStageRows, h.rows - r);
        if (fread(buf.data(), sizeof(float), (size_t)m * h.dim, f) != (size_t)m * h.dim) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return fail(RASS_ERR_IO, "truncated index file (rows)");
        }
        rc = rass_index_add(idx, buf.data(), nullptr, m, /*normalize*/ 0, nullptr);
        if (rc != RASS_OK) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return rc;
        }
    }
    if (h.rows > 0) {
        std::vector<int32_t> tags((size_t)h.rows);
        if (fread(tags.data(), 4, (size_t)h.rows, f) != (size_t)h.rows) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return fail(RASS_ERR_IO, "truncated index file (tags)");
        }
        hipError_t e;
        {
            std::lock_guard<std::mutex> lk(idx->mu);
            e = hipMemcpyAsync(idx->d_tags, tags.data(), (size_t)h.rows * 4, hipMemcpyHostToDevice, eng->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(eng->stream);
        }
        if (e != hipSuccess) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return fail(RASS_ERR_HIP, std::string("load: tag upload failed: ") + hipGetErrorString(e));
        }
        std::lock_guard<std::mutex> lk(idx->mu);
        for (int64_t r = 0; r < h.rows; ++r) {
            if (tags[(size_t)r] == RASS_ROW_TAG_DELETED) {
                idx->host_deleted[(size_t)(r >> 3)] |= (uint8_t)(1u << (r & 7));
                idx->deleted += 1;
            } else if (tags[(size_t)r] != 0) {
                idx->has_tags = true;
            }
        }
    }
    if (h.rows > 0 && (h.reserved & 1)) {
        std::vector<int64_t> gids((size_t)h.rows);
        hipError_t e = hipSuccess;
        if (fread(gids.data(), 8, (size_t)h.rows, f) != (size_t)h.rows) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return fail(RASS_ERR_IO, "truncated index file (ids)");
        }
        {
            std::lock_guard<std::mutex> lk(idx->mu);
            e = hipMemcpyAsync(idx->d_gid, gids.data(), (size_t)h.rows * 8, hipMemcpyHostToDevice, eng->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(eng->stream);
            idx->has_gid = true;
        }
        if (e != hipSuccess) {
            fclose(f);
            (void)rass_index_drop(eng, name);
            return fail(RASS_ERR_HIP, std::string("load: id upload failed: ") + hipGetErrorString(e));
        }
    }
    if (h.reserved & 2) {
        int32_t n_cols = 0;
        bool ok = fread(&n_cols, 4, 1, f) == 1 && n_cols >= 1 && n_cols <= RASS_MAX_ATTRS;
        std::vector<int32_t> vals((size_t)h.rows);
        int rc2 = RASS_OK;
        for (int32_t i = 0; ok && rc2 == RASS_OK && i < n_cols; ++i) {
            int32_t c = -1;
            ok = fread(&c, 4, 1, f) == 1 && c >= 0 && c < RASS_MAX_ATTRS &&
                 fread(vals.data(), 4, (size_t)h.rows, f) == (size_t)h.rows;
            if (!ok) break;
            std::lock_guard<std::mutex> lk(idx->mu);
            std::lock_guard<std::mutex> elk(eng->mu);
            rc2 = index_attr_ensure(idx, c);
            if (rc2 == RASS_OK && h.rows > 0) {
                hipError_t e = hipMemcpyAsync(idx->d_attr[c], vals.data(), (size_t)h.rows * 4, hipMemcpyHostToDevice, eng->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(eng->stream);
                if (e != hipSuccess) rc2 = fail(RASS_ERR_HIP, std::string("load: attribute upload failed: ") + hipGetErrorString(e));
            }
        }
        if (!ok || rc2 != RASS_OK) {
            const std::string why = rass_last_error();
            fclose(f);
            (void)rass_index_drop(eng, name);
            return ok ? fail(rc2, why) : fail(RASS_ERR_IO, "truncated index file (attribute columns)");
        }
    }
    fclose(f);
    *out = idx;
    return RASS_OK;
}

int rass_index_fill_synthetic(rass_index_t* idx, int64_t n, uint64_t seed, int64_t row_id_base) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    if (n < 0) return fail(RASS_ERR_INVALID, "n < 0");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(idx->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    if (n == 0) return RASS_OK;
    {
        std::lock_guard<std::mutex> elk(eng->mu);
        rc = index_reserve(idx, idx->rows + n);
        if (rc != RASS_OK) return rc;
    }
    hipStream_t st = eng->stream;
    if (idx->dtype == RASS_BF16) {
        std::lock_guard<std::mutex> elk(eng->mu);
        if (!eng->d_stage_t16)
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_stage_t16), (size_t)(kStageRows + 32) * kMaxStride * sizeof(float)));
        for (int64_t done = 0; done < n; done += kStageRows) {
            const int64_t m = std::min<int64_t>(kStageRows, n - done);
            const int64_t at = idx->rows + done, phase = at & 15;
            // the generator keys a row by row_id_base + its slab row: shift the base so staging row `phase` is row `at`
            HIP_TRY(rass::launch_fill_synthetic_f32(eng->d_stage_t16, idx->stride, phase, m, idx->dim, seed,
                                                    row_id_base + at - phase, st));
            HIP_TRY(rass::launch_convert_tile16_bf16(eng->d_stage_t16, idx->d_rows_bf16, idx->stride, at >> 4,
                                                     (at + m + 15) >> 4, st, 0, at, at + m));
        }
        HIP_TRY(hipStreamSynchronize(st));
    } else
    HIP_TRY(rass::launch_fill_synthetic_f32(idx->d_rows, idx->stride, idx->rows, n, idx->dim, seed, row_id_base, st));
    HIP_TRY(rass::launch_fill_i32(idx->d_tags + idx->rows, n, 0, st));
    for (int32_t* col : idx->d_attr)
        if (col) HIP_TRY(rass::launch_fill_i32(col + idx->rows, n, RASS_ATTR_MISSING, st));
    HIP_TRY(rass::launch_iota_i64(idx->d_gid + idx->rows, n, idx->rows.load(), st));
    rc = index_refresh_copies(idx, idx->rows, n, st);
    if (rc != RASS_OK) return rc;
    idx->rows += n;
    idx->host_deleted.resize((size_t)((idx->rows + 7) / 8), 0);
    return RASS_OK;
}

size_t rass_scan_workspace_bytes(int nq, int k) {
    if (nq < 1 || nq > RASS_MAX_QBATCH || k < 1 || k > RASS_MAX_K) return 0;
    return scratch_layout(nullptr, nq, k).total;
}

int rass_scan_topk_f32(const float* d_corpus, int64_t n_rows, int dim, int64_t row_stride,
                       const int32_t* d_row_tag, const float* d_queries, int nq, const int32_t* d_q_filter, int k,
                       int64_t id_base, float* d_out_scores, int64_t* d_out_ids, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
    if (!d_queries || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_rows > 0 && !d_corpus) return fail(RASS_ERR_INVALID, "corpus is NULL");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const float* corpus = d_corpus ? d_corpus : reinterpret_cast<const float*>(d_workspace);
    ScanRequest r;
    r.corpus = corpus, r.n_rows = n_rows, r.stride = row_stride, r.row_tag = d_row_tag;
    r.queries = d_queries, r.q_dim = dim, r.q_stride = dim, r.nq = nq, r.q_filter = d_q_filter;
    r.k = k, r.id_base = id_base, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    r.ws = reinterpret_cast<unsigned char*>(d_workspace), r.ws_bytes = workspace_bytes;
    r.n_cus = device_cus(dev), r.st = reinterpret_cast<hipStream_t>(stream);
    return scan_launch(r);
}

int rass_pack_rows_f32(const float* d_in, int64_t in_stride, float* d_packed, int64_t row_stride, int64_t first_row,
                       int64_t n, int dim, int normalize, void* stream) {
    if (n < 0 || dim < 1 || in_stride < dim || row_stride < dim || row_stride % 128 != 0 || first_row < 0)
        return fail(RASS_ERR_INVALID, "bad shape");
    if (n > 0 && (!d_in || !d_packed)) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_pack_rows_tile16(d_in, in_stride, d_packed, row_stride, first_row, n, dim, normalize ? 1 : 0,
                                          reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_unpack_rows_f32(const float* d_packed, int64_t row_stride, int64_t first_row, int64_t n, int dim,
                         float* d_out, int64_t out_stride, void* stream) {
    if (n < 0 || dim < 1 || out_stride < dim || row_stride < dim || row_stride % 128 != 0 || first_row < 0)
        return fail(RASS_ERR_INVALID, "bad shape");
    if (n > 0 && (!d_out || !d_packed)) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_unpack_rows_tile16(d_packed, row_stride, first_row, n, dim, d_out, out_stride,
                                            reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_gather_rows_f32(const float* d_packed, int64_t row_stride, int64_t n_rows, const int64_t* d_row_ids, int64_t n,
                         int dim, float* d_out, int64_t out_stride, void* stream) {
    if (n < 0 || n_rows < 0 || dim < 1 || out_stride < dim || row_stride < dim || row_stride % 128 != 0)
        return fail(RASS_ERR_INVALID, "bad shape");
    if (n > 0 && (!d_out || !d_packed || !d_row_ids)) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_gather_rows_tile16(d_packed, row_stride, d_row_ids, n, n_rows, dim, d_out, out_stride,
                                            reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_topk_merge(const float* d_scores, const int64_t* d_ids, int n_lists, int nq, int k, float* d_out_scores,
                    int64_t* d_out_ids, void* stream) {
    if (!d_scores || !d_ids || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_lists < 1 || nq < 1 || k < 1 || k > RASS_MAX_K) return fail(RASS_ERR_INVALID, "bad n_lists / nq / k");
    if ((int64_t)n_lists * k > rass::kMergeMaxCandidates)
        return fail(RASS_ERR_UNSUPPORTED, "n_lists * k exceeds 8192 candidates");
    HIP_TRY(rass::launch_merge_topk(d_scores, d_ids, n_lists, nq, k, d_out_scores, d_out_ids,
                                    reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_topk_merge_strided(const float* d_scores, const int64_t* d_ids, int64_t score_list_stride,
                            int64_t id_list_stride, int n_lists, int nq, int k, float* d_out_scores,
                            int64_t* d_out_ids, void* stream) {
    if (!d_scores || !d_ids || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_lists < 1 || nq < 1 || k < 1 || k > RASS_MAX_K) return fail(RASS_ERR_INVALID, "bad n_lists / nq / k");
    if (score_list_stride < (int64_t)nq * k || id_list_stride < (int64_t)nq * k)
        return fail(RASS_ERR_INVALID, "list strides must be >= nq * k elements");
    if ((int64_t)n_lists * k > rass::kMergeMaxCandidates)
        return fail(RASS_ERR_UNSUPPORTED, "n_lists * k exceeds 8192 candidates");
    HIP_TRY(rass::launch_merge_topk(d_scores, d_ids, n_lists, nq, k, d_out_scores, d_out_ids,
                                    reinterpret_cast<hipStream_t>(stream), nullptr, score_list_stride,
                                    id_list_stride));
    return RASS_OK;
}

int rass_topk_merge_strided_batch(const float* d_scores, const int64_t* d_ids, int64_t score_list_stride,
                                  int64_t id_list_stride, int n_lists, int nq_total, int group_size,
                                  int64_t score_group_stride, int64_t id_group_stride, int k, float* d_out_scores,
                                  int64_t* d_out_ids, void* stream) {
    if (!d_scores || !d_ids || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_lists < 1 || nq_total < 1 || k < 1 || k > RASS_MAX_K || group_size < 1 || group_size > RASS_MAX_QBATCH)
        return fail(RASS_ERR_INVALID, "bad n_lists / nq_total / group_size / k");
    if (score_group_stride < (int64_t)group_size * k || id_group_stride < (int64_t)group_size * k ||
        score_list_stride < (int64_t)group_size * k || id_list_stride < (int64_t)group_size * k)
        return fail(RASS_ERR_INVALID, "list and group strides must be >= group_size * k elements");
    if ((int64_t)n_lists * k > rass::kMergeMaxCandidates)
        return fail(RASS_ERR_UNSUPPORTED, "n_lists * k exceeds 8192 candidates");
    rass::MergeGroups mg;
    mg.size = group_size;
    mg.nq_total = nq_total;
    mg.lists_are_dense = false;
    mg.score_stride = score_group_stride;
    mg.id_stride = id_group_stride;
    mg.out_score_stride = mg.out_id_stride = (int64_t)group_size * k;
    HIP_TRY(rass::launch_merge_topk(d_scores, d_ids, n_lists, nq_total, k, d_out_scores, d_out_ids,
                                    reinterpret_cast<hipStream_t>(stream), nullptr, score_list_stride, id_list_stride,
                                    &mg));
    return RASS_OK;
}

int rass_normalize_rows_f32(const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int64_t n,
                            int dim, void* stream) {
    if (n < 0 || dim < 1 || in_stride < dim || out_stride < dim) return fail(RASS_ERR_INVALID, "bad shape");
    if (n > 0 && (!d_in || !d_out)) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_normalize_rows_f32(d_in, in_stride, d_out, out_stride, n, dim,
                                            reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

struct rass_timer {
    hipEvent_t start = nullptr, stop = nullptr;
};

int rass_timer_create(rass_timer_t** out) {
    if (!out) return fail(RASS_ERR_INVALID, "out is NULL");
    rass_timer* t = new (std::nothrow) rass_timer();
    if (!t) return fail(RASS_ERR_OOM, "host allocation failed");
    hipError_t e = hipEventCreate(&t->start);
    if (e == hipSuccess) e = hipEventCreate(&t->stop);
    if (e != hipSuccess) {
        rass_timer_destroy(t);
        return fail(RASS_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
    *out = t;
    return RASS_OK;
}

void rass_timer_destroy(rass_timer_t* t) {
    if (!t) return;
    if (t->start) (void)hipEventDestroy(t->start);
    if (t->stop) (void)hipEventDestroy(t->stop);
    delete t;
}

int rass_timer_start(rass_timer_t* t, void* stream) {
    if (!t) return fail(RASS_ERR_INVALID, "timer is NULL");
    HIP_TRY(hipEventRecord(t->start, reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_timer_stop(rass_timer_t* t, void* stream) {
    if (!t) return fail(RASS_ERR_INVALID, "timer is NULL");
    HIP_TRY(hipEventRecord(t->stop, reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_timer_elapsed_ms(rass_timer_t* t, float* ms) {
    if (!t || !ms) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(hipEventSynchronize(t->stop));
    HIP_TRY(hipEventElapsedTime(ms, t->start, t->stop));
    return RASS_OK;
}

int rass_engine_kernel_timing_begin(rass_engine_t* eng, int max_launches) {
    if (!eng || max_launches < 1) return fail(RASS_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    HIP_TRY(hipSetDevice(eng->device));
    while (eng->ev_pool.size() < (size_t)max_launches * 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        eng->ev_pool.push_back(e);
    }
    eng->ev_used = 0;
    eng->ev_extra = 0;
    eng->ev_on = true;
    return RASS_OK;
}

int rass_engine_kernel_timing_end(rass_engine_t* eng, double* total_ms, int* launches) {
    if (!eng || !total_ms || !launches) return fail(RASS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(eng->mu);
    HIP_TRY(hipSetDevice(eng->device));
    eng->ev_on = false;
    double sum = 0.0;
    for (int i = 0; i < eng->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(eng->ev_pool[2 * i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, eng->ev_pool[2 * i], eng->ev_pool[2 * i + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *launches = eng->ev_used + eng->ev_extra;
    eng->ev_used = 0;
    eng->ev_extra = 0;
    return RASS_OK;
}

void* rass_index_device_rows(rass_index_t* idx) { return idx ? reinterpret_cast<void*>(idx->d_rows) : nullptr; }
void* rass_index_device_tags(rass_index_t* idx) { return idx ? reinterpret_cast<void*>(idx->d_tags) : nullptr; }

// ---- K9(i): k-means over rows resident in an index's slab
static int kmeans_range_ok(const rass_index* idx, int64_t first_block, int64_t block_step, int64_t n_blocks) {
    if (first_block < 0 || block_step < 1 || n_blocks < 0) return 0;
    if (n_blocks == 0) return 1;
    const int64_t last = first_block + (n_blocks - 1) * block_step;
    return last * 32 < idx->rows.load();  // the last processed block must hold at least one appended row
}

int rass_kmeans_assign(rass_index_t* idx, int64_t first_block, int64_t block_step, int64_t n_blocks,
                       const float* d_centroids_tile16, int nlist, int32_t* d_assign, float* d_best) {
    if (!idx || !d_centroids_tile16 || !d_assign) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nlist < 1 || nlist > 65536) return fail(RASS_ERR_INVALID, "nlist must be in [1, 65536]");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "k-means needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "k-means needs dim <= 1024 (wide rows: flat scan only)");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!kmeans_range_ok(idx, first_block, block_step, n_blocks) || n_blocks > 0x7fffffff)
        return fail(RASS_ERR_INVALID, "block range outside the index");
    rass_engine* eng = idx->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> elk(eng->mu);
    rass::AssignArgs a;
    a.rows = idx->d_rows;
    a.centroids = d_centroids_tile16;
    a.assign = d_assign;
    a.best = d_best;
    a.row_stride = idx->stride;
    a.slab_rows = idx->capacity;
    a.first_block = first_block;
    a.block_step = block_step;
    a.n_blocks = (int)n_blocks;
    a.nlist = nlist;
    HIP_TRY(rass::launch_kmeans_assign_f32(a, eng->n_cus, eng->stream));
    return RASS_OK;
}

int rass_kmeans_accumulate(rass_index_t* idx, int64_t first_block, int64_t block_step, int64_t n_blocks,
                           const int32_t* d_assign, float* d_sums, float* d_counts, int nlist) {
    if (!idx || !d_assign || !d_sums || !d_counts) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nlist < 1) return fail(RASS_ERR_INVALID, "nlist < 1");
    if (idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "k-means needs an fp32 index");
    if (idx->stride > kNarrowStride) return fail(RASS_ERR_UNSUPPORTED, "k-means needs dim <= 1024 (wide rows: flat scan only)");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (!kmeans_range_ok(idx, first_block, block_step, n_blocks) || n_blocks > 0x7fffffff)
        return fail(RASS_ERR_INVALID, "block range outside the index");
    rass_engine* eng = idx->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> elk(eng->mu);
    HIP_TRY(rass::launch_kmeans_accumulate(idx->d_rows, idx->stride, first_block, block_step, (int)n_blocks,
                                           idx->rows.load(), d_assign, d_sums, d_counts, idx->dim, nlist, eng->stream));
    return RASS_OK;
}

// ---- §8f-4: peer-store exchange (no collective on the search path)
int rass_peer_buffer_create(int device, size_t bytes, void** d_ptr, unsigned char* handle64) {
    if (!d_ptr || !handle64 || bytes == 0) return fail(RASS_ERR_INVALID, "bad argument");
    *d_ptr = nullptr;
    HIP_TRY(hipSetDevice(device));
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // the flags must BE zero before any peer (or stream) touches them
    hipIpcMemHandle_t h;
    if (e == hipSuccess) e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(RASS_ERR_HIP, std::string("peer buffer: ") + hipGetErrorString(e) +
                                      " (multi-process GPU memory sharing needs HSA_ENABLE_IPC_MODE_LEGACY=0 here)");
    }
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the ABI carries the IPC handle as 64 bytes");
    memcpy(handle64, &h, 64);
    *d_ptr = p;
    return RASS_OK;
}

int rass_peer_buffer_open(int device, const unsigned char* handle64, void** d_ptr) {
    if (!d_ptr || !handle64) return fail(RASS_ERR_INVALID, "NULL argument");
    *d_ptr = nullptr;
    HIP_TRY(hipSetDevice(device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, 64);
    HIP_TRY(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return RASS_OK;
}

int rass_peer_buffer_close(void* d_ptr, int opened_from_handle) {
    if (!d_ptr) return RASS_OK;
    if (opened_from_handle)
        HIP_TRY(hipIpcCloseMemHandle(d_ptr));
    else
        HIP_TRY(hipFree(d_ptr));
    return RASS_OK;
}

int rass_peer_post(const void* d_record, size_t bytes, void* d_remote_slot, void* d_remote_flag, uint64_t seq,
                   void* stream) {
    if (!d_record || !d_remote_slot || !d_remote_flag) return fail(RASS_ERR_INVALID, "NULL argument");
    HIP_TRY(rass::launch_peer_post(d_record, bytes, d_remote_slot, d_remote_flag, seq, reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

int rass_peer_wait(const void* d_flags, int n, int flag_stride_bytes, uint64_t seq, int* d_status, int64_t max_spins,
                   void* stream) {
    if (!d_flags || !d_status || max_spins < 1) return fail(RASS_ERR_INVALID, "bad argument");
    HIP_TRY(rass::launch_peer_wait(d_flags, n, flag_stride_bytes, seq, d_status, max_spins,
                                   reinterpret_cast<hipStream_t>(stream)));
    return RASS_OK;
}

const char* rass_scan_kernel_name(int dim, int nq) {
    static thread_local char buf[64];
    const int64_t stride = pad_stride(dim);
    if (dim < 1 || !rass::scan_supported_stride(stride) || stride > kMaxStride || nq < 1 || nq > RASS_MAX_QBATCH)
        return "";
    if (stride > kNarrowStride) {
        const int ch = (int)(stride / 128);
        // <CHP, P, EXT, RANGE, GROUP, COUNT>: the plain top-k instantiation of launch_wide (scan_topk.hip)
        snprintf(buf, sizeof(buf), "scan_topk_f32_wide_kernel<%d, %d, false, false, false, false>", ch == 16 ? 4 : ch / 2,
                 ch == 16 ? 4 : 2);
        return buf;
    }
    snprintf(buf, sizeof(buf), "scan_topk_f32_kernel<%d, %d, 0, false>", (int)(stride / 128), nq <= 16 ? 1 : 2);
    return buf;
}

}  // extern "C"
