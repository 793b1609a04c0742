// api_keys.hip — the C ABI of include/rass_engine.h: the builders of key columns from the attribute columns of a flat index
// (rass_index_keys_from_attr, rass_index_keys_from_attr_edges) and from the tag (rass_index_keys_from_tag) and the reduction a histogram is laid out with
// (rass_index_attr_minmax).  A key column feeds rass_index_search_grouped_keys / rass_index_aggregate_keys (api_emit.hip).
// Host-side C++ only: the kernels are group_keys.hip.  The objects and the threading rules: api_internal.h.

#include "api_internal.h"

using namespace rass::host;

namespace {

int check_key_col(int col) {
    return col < 0 || col >= RASS_MAX_ATTRS ? fail(RASS_ERR_INVALID, "col must be in [0, RASS_MAX_ATTRS)") : (int)RASS_OK;
}

// What the two builders check alike, under eng->mu: the rows the keys must cover.
int check_key_room(int64_t n_rows, int64_t n_keys) {
    if (n_keys < n_rows)
        return fail(RASS_ERR_INVALID, "n_keys (" + std::to_string(n_keys) + ") is smaller than the index's rows (" + std::to_string(n_rows) + ")");
    return RASS_OK;
}

}  // namespace

extern "C" {

int rass_index_keys_from_attr(rass_index_t* idx, int col, int32_t base, int32_t missing_key, int32_t* d_keys, int64_t n_keys) {
    if (!idx || !d_keys) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_key_col(col)) return rc;
    if (missing_key < RASS_KEY_NONE) return fail(RASS_ERR_INVALID, "missing_key must be >= RASS_KEY_NONE (-1)");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_key_room(n_rows, n_keys)) != RASS_OK) return rc;
    HIP_TRY(rass::launch_keys_from_attr(idx->d_attr[col], n_rows, n_keys, base, missing_key, d_keys, eng->stream));
    return RASS_OK;
}

int rass_index_keys_from_tag(rass_index_t* idx, int32_t mask, int32_t* d_keys, int64_t n_keys) {
    if (!idx || !d_keys) return fail(RASS_ERR_INVALID, "NULL argument");
    if (mask <= 0) return fail(RASS_ERR_INVALID, "mask must be non-zero and within 0x7fffffff");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_key_room(n_rows, n_keys)) != RASS_OK) return rc;
    HIP_TRY(rass::launch_keys_from_tag(idx->d_tags, n_rows, n_keys, mask, d_keys, eng->stream));
    return RASS_OK;
}

int rass_index_keys_from_attr_edges(rass_index_t* idx, int col, const int32_t* edges, int n_edges, int32_t missing_key,
                                    int32_t* d_keys, int64_t n_keys) {
    if (!idx || !d_keys || !edges) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_key_col(col)) return rc;
    if (missing_key < RASS_KEY_NONE) return fail(RASS_ERR_INVALID, "missing_key must be >= RASS_KEY_NONE (-1)");
    if (n_edges < 2 || n_edges > RASS_MAX_KEY_EDGES) return fail(RASS_ERR_INVALID, "n_edges must be in [2, RASS_MAX_KEY_EDGES]");
    for (int j = 1; j < n_edges; ++j)
        if (edges[j] <= edges[j - 1]) return fail(RASS_ERR_INVALID, "edges must be strictly ascending");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if ((rc = check_key_room(n_rows, n_keys)) != RASS_OK) return rc;
    const size_t bytes = (size_t)n_edges * sizeof(int32_t);
    if ((rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, bytes, st)) != RASS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(eng->d_allow_io, edges, bytes, hipMemcpyHostToDevice, st));
    rc = HIP_RC(rass::launch_keys_from_attr_edges(idx->d_attr[col], n_rows, n_keys, reinterpret_cast<const int32_t*>(eng->d_allow_io),
                                                  n_edges, missing_key, d_keys, st));
    const hipError_t e = hipStreamSynchronize(st);   // `edges` has been read, whatever became of the launch
    return rc != RASS_OK ? rc : HIP_RC(e);
}

int rass_index_attr_minmax(rass_index_t* idx, int col, int32_t* out_min, int32_t* out_max, int64_t* out_n_present) {
    if (!idx || !out_min || !out_max || !out_n_present) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_key_col(col)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    int32_t h[4] = {INT32_MAX, INT32_MIN, 0, 0};   // min, max, the count's two halves
    if (n_rows > 0 && idx->d_attr[col]) {
        if ((rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, sizeof(h), st)) != RASS_OK) return rc;
        int32_t* d = reinterpret_cast<int32_t*>(eng->d_allow_io);
        HIP_TRY(hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, st));
        rc = HIP_RC(rass::launch_attr_minmax(idx->d_attr[col], idx->d_tags, n_rows, d, st));
        if (rc == RASS_OK) rc = HIP_RC(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st));
        const hipError_t e = hipStreamSynchronize(st);   // `h` has been read and written, whatever became of the launch
        if (rc != RASS_OK) return rc;
        if (e != hipSuccess) return HIP_RC(e);
    }
    int64_t n = 0;
    memcpy(&n, h + 2, sizeof(n));
    *out_min = h[0], *out_max = h[1], *out_n_present = n;
    return RASS_OK;
}

}  // extern "C"
