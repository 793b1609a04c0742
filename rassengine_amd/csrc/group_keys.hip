// group_keys.hip — the builders of KEY COLUMNS: int32[n_keys] arrays that give every row of a flat index its group (>= 0) or
// none (kKeyNone = -1), which scan_topk.hip's ScanModes kGroupMaxKeys / kGroupCountKeys read in the place of a bit field of
// the tag.  A key comes from one int32 attribute column: the value itself, moved by a base (keys_from_attr_kernel: keyword
// codes, ints, days), the tag's own group field (keys_from_tag_kernel), or the bucket a set of ascending edges puts it in (keys_from_attr_edges_kernel: histograms; the edges
// sit in LDS and are binary searched, as allow_from_tag_values_kernel does with its value set).  attr_minmax_kernel is the
// small reduction a histogram is laid out with: min, max and count of the present values over the live rows.
//
// One thread per key, grid-stride, coalesced.  The attribute builders do not read the tags — the scan skips tombstones
// itself —, the tag builder and the reduction do.  Plain vector loads, stores and atomics; no workgroup waits on another.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kKeyThreads = 256;
constexpr int32_t kAttrMissing = INT32_MIN;   // = RASS_ATTR_MISSING
constexpr int32_t kKeyNone = -1;              // = RASS_KEY_NONE

// keys[i] = col[i] - base where that lies in [0, INT32_MAX] (64-bit: no overflow), missing_key for a missing value (a null
// column is all missing), kKeyNone otherwise and for i in [n_rows, n_keys).
__global__ __launch_bounds__(kKeyThreads) void keys_from_attr_kernel(const int32_t* __restrict__ col, int64_t n_rows, int64_t n_keys,
                                                                     int32_t base, int32_t missing_key, int32_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * kKeyThreads + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * kKeyThreads) {
        int32_t key = kKeyNone;
        if (i < n_rows) {
            const int32_t v = col != nullptr ? col[i] : kAttrMissing;
            const int64_t d = (int64_t)v - (int64_t)base;
            key = v == kAttrMissing ? missing_key : (d < 0 || d > (int64_t)INT32_MAX ? kKeyNone : (int32_t)d);
        }
        keys[i] = key;
    }
}

// keys[i] = j where edges[j] <= col[i] < edges[j + 1] (edges strictly ascending, n_edges >= 2), kKeyNone below the first edge
// and at or above the last, missing_key for a missing value, kKeyNone for i in [n_rows, n_keys).
__global__ __launch_bounds__(kKeyThreads) void keys_from_attr_edges_kernel(const int32_t* __restrict__ col, int64_t n_rows,
                                                                           int64_t n_keys, const int32_t* __restrict__ edges,
                                                                           int n_edges, int32_t missing_key,
                                                                           int32_t* __restrict__ keys) {
    __shared__ int32_t sh_edges[kKeyMaxEdges];
    for (int j = threadIdx.x; j < n_edges; j += kKeyThreads) sh_edges[j] = edges[j];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kKeyThreads + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * kKeyThreads) {
        int32_t key = kKeyNone;
        if (i < n_rows) {
            const int32_t v = col != nullptr ? col[i] : kAttrMissing;
            // the number of edges <= v (an upper bound search), minus one
            int lo = 0, hi = n_edges;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sh_edges[mid] <= v) lo = mid + 1;
                else hi = mid;
            }
            key = v == kAttrMissing ? missing_key : (lo == 0 || lo == n_edges ? kKeyNone : lo - 1);
        }
        keys[i] = key;
    }
}

// keys[i] = (tags[i] & mask) >> shift for a live row, kKeyNone for a tombstone (tag -1) and for i in [n_rows, n_keys): the
// tag-keyed searches' own group, as a key column (so that they can run within a bitmap).
__global__ __launch_bounds__(kKeyThreads) void keys_from_tag_kernel(const int32_t* __restrict__ tags, int64_t n_rows, int64_t n_keys,
                                                                    int32_t mask, int shift, int32_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * kKeyThreads + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * kKeyThreads) {
        int32_t key = kKeyNone;
        if (i < n_rows) {
            const int32_t tag = tags[i];
            key = tag == -1 ? kKeyNone : (int32_t)((uint32_t)(tag & mask) >> shift);
        }
        keys[i] = key;
    }
}

// out[0] = min, out[1] = max (as int32), out[2..3] = the count (64-bit) of the values that are not missing over the rows whose
// tag is not -1.  The caller sets out to {INT32_MAX, INT32_MIN, 0, 0} first.  A wave folds its lanes' partial results by
// __shfl_xor, its first lane adds them in with three atomics.
__global__ __launch_bounds__(kKeyThreads) void attr_minmax_kernel(const int32_t* __restrict__ col, const int32_t* __restrict__ tags,
                                                                  int64_t n_rows, int32_t* __restrict__ out) {
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    unsigned n = 0;   // per thread: n_rows / the grid's threads, far below 2^32
    for (int64_t i = (int64_t)blockIdx.x * kKeyThreads + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * kKeyThreads) {
        const int32_t v = col[i];
        if (v != kAttrMissing && tags[i] != -1) {
            mn = min(mn, v);
            mx = max(mx, v);
            ++n;
        }
    }
    unsigned long long cnt = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = min(mn, __shfl_xor(mn, off));
        mx = max(mx, __shfl_xor(mx, off));
        cnt += __shfl_xor(cnt, off);
    }
    if ((threadIdx.x & 63) == 0 && cnt != 0) {
        atomicMin(out, mn);
        atomicMax(out + 1, mx);
        atomicAdd(reinterpret_cast<unsigned long long*>(out + 2), cnt);
    }
}

int key_grid(int64_t n) { return (int)std::min<int64_t>((n + kKeyThreads - 1) / kKeyThreads, 2048); }

}  // namespace

hipError_t launch_keys_from_attr(const int32_t* col, int64_t n_rows, int64_t n_keys, int32_t base, int32_t missing_key, int32_t* keys,
                                 hipStream_t stream) {
    if (n_rows < 0 || n_keys < n_rows || missing_key < kKeyNone) return hipErrorInvalidValue;
    if (n_keys == 0) return hipSuccess;
    if (!keys) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_from_attr_kernel, dim3(key_grid(n_keys)), dim3(kKeyThreads), 0, stream, col, n_rows, n_keys, base,
                       missing_key, keys);
    return hipGetLastError();
}

hipError_t launch_keys_from_attr_edges(const int32_t* col, int64_t n_rows, int64_t n_keys, const int32_t* edges, int n_edges,
                                       int32_t missing_key, int32_t* keys, hipStream_t stream) {
    if (n_rows < 0 || n_keys < n_rows || missing_key < kKeyNone || n_edges < 2 || n_edges > kKeyMaxEdges) return hipErrorInvalidValue;
    if (n_keys == 0) return hipSuccess;
    if (!keys || !edges) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_from_attr_edges_kernel, dim3(key_grid(n_keys)), dim3(kKeyThreads), 0, stream, col, n_rows, n_keys, edges,
                       n_edges, missing_key, keys);
    return hipGetLastError();
}

hipError_t launch_keys_from_tag(const int32_t* tags, int64_t n_rows, int64_t n_keys, int32_t mask, int32_t* keys, hipStream_t stream) {
    if (n_rows < 0 || n_keys < n_rows || mask <= 0) return hipErrorInvalidValue;
    if (n_keys == 0) return hipSuccess;
    if (!keys || (n_rows > 0 && !tags)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_from_tag_kernel, dim3(key_grid(n_keys)), dim3(kKeyThreads), 0, stream, tags, n_rows, n_keys, mask,
                       __builtin_ctz((unsigned)mask), keys);
    return hipGetLastError();
}

hipError_t launch_attr_minmax(const int32_t* col, const int32_t* tags, int64_t n_rows, int32_t* out, hipStream_t stream) {
    if (n_rows < 0 || !out) return hipErrorInvalidValue;
    if (n_rows == 0 || !col) return hipSuccess;   // a column never set: nothing is present
    if (!tags) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attr_minmax_kernel, dim3(key_grid(n_rows)), dim3(kKeyThreads), 0, stream, col, tags, n_rows, out);
    return hipGetLastError();
}

}  // namespace rass
