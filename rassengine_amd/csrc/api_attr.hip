// api_attr.hip — the C ABI of include/rass_engine.h: the attribute columns of a flat index (rass_index_set_attr / _get_attr /
// _attr_mask / _device_attr), the predicate builder rass_index_allow_from_attr_clauses, whose bitmaps feed the allow-list
// search of api_allow.hip, and the word-wise merge of two bitmaps rass_index_allow_combine.  Host-side C++ only: the kernel is attr.hip.  The columns are members of rass_index; growth, free,
// persistence and the synthetic fill carry them in api.hip, compaction in api_compact.hip.  The objects and the threading
// rules: api_internal.h.

#include <tuple>

#include "api_internal.h"

using namespace rass::host;

namespace {

int check_col(int col) {
    return col < 0 || col >= RASS_MAX_ATTRS ? fail(RASS_ERR_INVALID, "col must be in [0, RASS_MAX_ATTRS)") : (int)RASS_OK;
}

}  // namespace

extern "C" {

int rass_index_set_attr(rass_index_t* idx, int col, int64_t first_row, int64_t n, const int32_t* values) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    if (int rc = check_col(col)) return rc;
    if (n < 0 || (n > 0 && !values)) return fail(RASS_ERR_INVALID, "bad values / n");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(idx->mu);
    if (first_row < 0 || first_row > idx->rows || n > idx->rows - first_row)
        return fail(RASS_ERR_INVALID, "rows [first_row, first_row + n) lie outside the index");
    if (n == 0) return RASS_OK;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    std::lock_guard<std::mutex> elk(eng->mu);   // the allocation publishes a pointer the predicate builder reads
    if ((rc = index_attr_ensure(idx, col)) != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    HIP_TRY(hipMemcpyAsync(idx->d_attr[col] + first_row, values, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the caller's array has been read
    return RASS_OK;
}

int rass_index_get_attr(rass_index_t* idx, int col, int64_t first_row, int64_t n, int32_t* out) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    if (int rc = check_col(col)) return rc;
    if (n < 0 || (n > 0 && !out)) return fail(RASS_ERR_INVALID, "bad out / n");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (first_row < 0 || first_row > idx->rows || n > idx->rows - first_row)
        return fail(RASS_ERR_INVALID, "rows [first_row, first_row + n) lie outside the index");
    if (n == 0) return RASS_OK;
    if (!idx->d_attr[col]) {   // never set: all missing
        std::fill(out, out + n, (int32_t)RASS_ATTR_MISSING);
        return RASS_OK;
    }
    int rc = set_device(idx->eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = idx->eng->stream;
    HIP_TRY(hipMemcpyAsync(out, idx->d_attr[col] + first_row, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RASS_OK;
}

int rass_index_attr_mask(const rass_index_t* idx) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(const_cast<rass_index_t*>(idx)->mu);
    int mask = 0;
    for (int c = 0; c < RASS_MAX_ATTRS; ++c) mask |= idx->d_attr[c] ? (1 << c) : 0;
    return mask;
}

void* rass_index_device_attr(rass_index_t* idx, int col) {
    return idx && col >= 0 && col < RASS_MAX_ATTRS ? reinterpret_cast<void*>(idx->d_attr[col]) : nullptr;
}

int rass_index_allow_from_attr_clauses(rass_index_t* idx, const int32_t* clauses, int64_t n_clauses, int nq, int n_bitmaps, int mode,
                                       int combine, uint32_t* d_allow, int64_t words_per_bitmap) {
    if (!idx || !d_allow) return fail(RASS_ERR_INVALID, "NULL argument");
    if (n_clauses < 0 || (n_clauses > 0 && !clauses)) return fail(RASS_ERR_INVALID, "bad clauses / n_clauses");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (n_bitmaps != 1 && n_bitmaps != nq) return fail(RASS_ERR_INVALID, "n_bitmaps must be 1 (shared) or nq (one per query)");
    if (mode != RASS_ATTR_ALL && mode != RASS_ATTR_ANY) return fail(RASS_ERR_INVALID, "mode must be RASS_ATTR_ALL or RASS_ATTR_ANY");
    if (combine != RASS_ATTR_REPLACE && combine != RASS_ATTR_AND && combine != RASS_ATTR_OR)
        return fail(RASS_ERR_INVALID, "combine must be RASS_ATTR_REPLACE, RASS_ATTR_AND or RASS_ATTR_OR");
    if (words_per_bitmap < 0) return fail(RASS_ERR_INVALID, "words_per_bitmap is negative");
    if (n_clauses > (int64_t)n_bitmaps * RASS_MAX_ATTR_CLAUSES)
        return fail(RASS_ERR_INVALID, "more than RASS_MAX_ATTR_CLAUSES clauses for one query");
    // the clauses of launch group g (queries 32 g .. 32 g + 31, rebased), ordered by column, query, bounds: one upload for all
    const int groups = (n_bitmaps + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    struct Clause {
        int32_t group, col, q, lo, hi, neg;
    };
    std::vector<Clause> sorted((size_t)n_clauses);
    std::vector<int> per_query((size_t)n_bitmaps, 0);
    for (int64_t i = 0; i < n_clauses; ++i) {
        const int32_t* c = clauses + i * 5;
        if (c[0] < 0 || c[0] >= n_bitmaps)
            return fail(RASS_ERR_INVALID, n_bitmaps == 1 && nq > 1 ? "a clause of a shared bitmap must name query 0"
                                                                     : "a clause names a query outside [0, nq)");
        if (check_col(c[1]) != RASS_OK) return fail(RASS_ERR_INVALID, "a clause names a column outside [0, RASS_MAX_ATTRS)");
        if (++per_query[(size_t)c[0]] > RASS_MAX_ATTR_CLAUSES)
            return fail(RASS_ERR_INVALID, "more than RASS_MAX_ATTR_CLAUSES clauses for query " + std::to_string(c[0]));
        sorted[(size_t)i] = {c[0] / RASS_MAX_QBATCH, c[1], c[0] % RASS_MAX_QBATCH, c[2], c[3], c[4] != 0 ? 1 : 0};
    }
    std::sort(sorted.begin(), sorted.end(), [](const Clause& x, const Clause& y) {
        return std::tie(x.group, x.col, x.q, x.lo, x.hi, x.neg) < std::tie(y.group, y.col, y.q, y.lo, y.hi, y.neg);
    });
    std::vector<int32_t> packed((size_t)n_clauses * 4);
    for (size_t i = 0; i < sorted.size(); ++i)
        packed[4 * i] = sorted[i].q, packed[4 * i + 1] = sorted[i].lo, packed[4 * i + 2] = sorted[i].hi, packed[4 * i + 3] = sorted[i].neg;

    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    hipStream_t st = eng->stream;
    const int64_t n_rows = idx->rows.load(std::memory_order_acquire);
    if (words_per_bitmap < (n_rows + 31) / 32)
        return fail(RASS_ERR_INVALID, "words_per_bitmap (" + std::to_string(words_per_bitmap) + ") is smaller than ceil(rows / 32) = " +
                                          std::to_string((n_rows + 31) / 32));
    const int4* d_clauses = nullptr;
    if (n_clauses > 0) {
        rc = grow_block(&eng->d_allow_io, &eng->allow_io_bytes, packed.size() * sizeof(int32_t), st);
        if (rc != RASS_OK) return rc;
        HIP_TRY(hipMemcpyAsync(eng->d_allow_io, packed.data(), packed.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        d_clauses = reinterpret_cast<const int4*>(eng->d_allow_io);
    }
    size_t at = 0;   // the first clause of the group
    rc = RASS_OK;
    for (int g = 0; g < groups && rc == RASS_OK; ++g) {
        rass::AttrArgs a;
        a.tags = idx->d_tags;
        for (int c = 0; c < RASS_MAX_ATTRS; ++c) a.col[c] = idx->d_attr[c];
        a.clauses = d_clauses ? d_clauses + at : nullptr;
        size_t end = at;
        for (int c = 0; c < RASS_MAX_ATTRS; ++c) {
            while (end < sorted.size() && sorted[end].group == g && sorted[end].col == c) ++end;
            a.col_off[c + 1] = (int)(end - at);
        }
        at = end;
        a.n_rows = n_rows;
        // replace / and: the tail bits and the surplus words come out 0; or: they stay as they were
        a.span_rows = combine == RASS_ATTR_OR ? n_rows : words_per_bitmap * 32;
        a.allow = d_allow + (int64_t)g * RASS_MAX_QBATCH * words_per_bitmap;
        a.q_stride = words_per_bitmap;
        a.nq = std::min(RASS_MAX_QBATCH, n_bitmaps - g * RASS_MAX_QBATCH);
        a.mode_any = mode == RASS_ATTR_ANY ? 1 : 0;
        a.combine = combine;
        rc = HIP_RC(rass::launch_attr_clauses(a, st));
    }
    if (n_clauses > 0) {   // `packed` has been read, whatever became of the launches
        const hipError_t e = hipStreamSynchronize(st);
        if (rc == RASS_OK) rc = HIP_RC(e);
    }
    return rc;
}

int rass_index_allow_combine(rass_index_t* idx, uint32_t* d_dst, const uint32_t* d_src, int64_t words, int op) {
    if (!idx || !d_dst || !d_src) return fail(RASS_ERR_INVALID, "NULL argument");
    if (words < 0) return fail(RASS_ERR_INVALID, "words is negative");
    if (op != RASS_ATTR_AND && op != RASS_ATTR_OR && op != RASS_ATTR_ANDNOT)
        return fail(RASS_ERR_INVALID, "op must be RASS_ATTR_AND, RASS_ATTR_OR or RASS_ATTR_ANDNOT");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_allow_combine(d_dst, d_src, words, op, eng->stream));
    return RASS_OK;
}

}  // extern "C"
