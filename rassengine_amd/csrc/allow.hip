// allow.hip — the small kernels around the allow-list scan (scan_topk.hip, ScanMode kAllow): building a row bitmap from a
// row list or from a set of tag values, turning the bitmaps of one launch group into the scan's work list, and storing a
// pass of a k > 32 search together with the next pass's continuation bound.
//
// A bitmap is uint32 words, row-major per query: bit (r & 31) of word r >> 5 allows row r, so one word covers exactly one
// 32-row scan tile.  Everything here is plain vector loads, stores and atomics; no workgroup waits on another.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kAllowThreads = 256;

__global__ __launch_bounds__(kAllowThreads) void allow_from_rows_kernel(const int64_t* __restrict__ rows, int64_t n, int64_t n_rows,
                                                                        uint32_t* __restrict__ allow) {
    const int64_t i = (int64_t)blockIdx.x * kAllowThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i];
    if (r < 0 || r >= n_rows) return;   // ids outside the index allow nothing
    atomicOr(&allow[r >> 5], 1u << (r & 31));
}

// One thread per row, a half-wave per word: the word is the half's ballot.  The value set is searched in LDS when it fits.
__global__ __launch_bounds__(kAllowThreads) void allow_from_tag_values_kernel(const int32_t* __restrict__ tags, int64_t n_rows,
                                                                              const int32_t* __restrict__ values, int n_values,
                                                                              int32_t mask, uint32_t* __restrict__ allow) {
    __shared__ int32_t sh_values[kAllowLdsValues];
    const bool in_lds = n_values <= kAllowLdsValues;
    if (in_lds)
        for (int i = threadIdx.x; i < n_values; i += kAllowThreads) sh_values[i] = values[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // block-uniform trip count: every lane reaches the ballot
    for (int64_t base = (int64_t)blockIdx.x * kAllowThreads; base < n_rows; base += (int64_t)gridDim.x * kAllowThreads) {
        const int64_t r = base + threadIdx.x;
        bool hit = false;
        if (r < n_rows) {
            const int32_t tag = tags[r];
            if (tag != -1) {
                const int32_t v = tag & mask;
                int lo = 0, hi = n_values;   // the first value >= v
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const int32_t x = in_lds ? sh_values[mid] : values[mid];
                    if (x < v) lo = mid + 1;
                    else hi = mid;
                }
                hit = lo < n_values && (in_lds ? sh_values[lo] : values[lo]) == v;
            }
        }
        const unsigned long long b = __ballot(hit);
        if ((lane & 31) == 0 && r < n_rows) allow[r >> 5] = (lane & 32) ? (unsigned)(b >> 32) : (unsigned)b;
    }
}

// Plan, step 1: tile_mask[t] = the queries of the group with a bit set in tile t below n_rows; block_count[b] = the tiles of
// block b with a non-zero mask.
__global__ __launch_bounds__(kAllowThreads) void allow_plan_mask_kernel(const uint32_t* __restrict__ allow, int64_t q_stride, int nq,
                                                                        int64_t n_rows, int n_tiles, uint32_t* __restrict__ tile_mask,
                                                                        int32_t* __restrict__ block_count) {
    const int t = blockIdx.x * kAllowThreads + threadIdx.x;
    uint32_t m = 0;
    if (t < n_tiles) {
        const int64_t rows_here = n_rows - (int64_t)t * 32;
        const uint32_t valid = rows_here >= 32 ? 0xffffffffu : ((1u << rows_here) - 1u);   // the last word's bits past n_rows allow nothing
        if (q_stride == 0) {
            m = (allow[t] & valid) ? (nq >= 32 ? 0xffffffffu : ((1u << nq) - 1u)) : 0u;
        } else {
            for (int q = 0; q < nq; ++q) m |= ((allow[(int64_t)q * q_stride + t] & valid) != 0u ? 1u : 0u) << q;
        }
        tile_mask[t] = m;
    }
    const int c = __syncthreads_count(m != 0u);
    if (threadIdx.x == 0) block_count[blockIdx.x] = c;
}

// Plan, step 2: block b places its tiles behind those of blocks 0 .. b-1 (it sums their counts itself), in tile order.
__global__ __launch_bounds__(kAllowThreads) void allow_plan_place_kernel(const uint32_t* __restrict__ tile_mask,
                                                                         const int32_t* __restrict__ block_count, int64_t n_rows,
                                                                         int n_tiles, int32_t* __restrict__ work_tile,
                                                                         int32_t* __restrict__ work_rows, uint32_t* __restrict__ work_mask,
                                                                         int32_t* __restrict__ n_work) {
    __shared__ int sh_wave[kAllowThreads / 64];
    __shared__ int sh_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // items of the blocks before this one
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kAllowThreads) before += block_count[b];
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if (lane == 0) sh_wave[wave] = before;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kAllowThreads / 64; ++w) s += sh_wave[w];
        sh_base = s;
    }
    __syncthreads();
    const int base = sh_base;
    __syncthreads();   // sh_wave is reused below
    const int t = blockIdx.x * kAllowThreads + threadIdx.x;
    const uint32_t m = t < n_tiles ? tile_mask[t] : 0u;
    const unsigned long long b = __ballot(m != 0u);
    if (lane == 0) sh_wave[wave] = __popcll(b);
    __syncthreads();
    int pos = base + __popcll(b & ((1ull << lane) - 1ull));
    int total = 0;
    for (int w = 0; w < kAllowThreads / 64; ++w) {
        const int c = sh_wave[w];
        if (w < wave) pos += c;
        total += c;
    }
    if (m != 0u) {   // pos < the number of non-empty tiles <= n_tiles: inside the lists
        const int64_t rows_here = n_rows - (int64_t)t * 32;
        work_tile[pos] = t;
        work_rows[pos] = rows_here >= 32 ? 32 : (int32_t)rows_here;
        work_mask[pos] = m;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_work = base + total;
}

__global__ void allow_store_kernel(const float* __restrict__ scores, const int64_t* __restrict__ rows, int kk, int k, int kdone,
                                   int64_t id_base, const int64_t* __restrict__ id_map, float* __restrict__ out_scores,
                                   int64_t* __restrict__ out_ids, float* __restrict__ after_s, int64_t* __restrict__ after_i) {
    const int q = blockIdx.x, j = threadIdx.x;
    if (j >= kk) return;
    const int64_t row = rows[(int64_t)q * kk + j];
    const float s = row >= 0 ? scores[(int64_t)q * kk + j] : -INFINITY;
    const int64_t o = (int64_t)q * k + kdone + j;
    out_scores[o] = s;
    out_ids[o] = row < 0 ? (int64_t)-1 : (id_map ? id_map[row] : id_base + row);
    if (j == kk - 1) {
        after_s[q] = s;
        after_i[q] = row >= 0 ? row : INT64_MAX;
    }
}

// counts[b] += the set bits of bitmap b below n_rows (blockIdx.y = b; the caller zeroes counts).  One atomic per wave.
__global__ __launch_bounds__(kAllowThreads) void allow_count_kernel(const uint32_t* __restrict__ allow, int64_t q_stride, int64_t n_rows,
                                                                    unsigned long long* __restrict__ counts) {
    const int64_t n_words = (n_rows + 31) / 32;
    const uint32_t* bits = allow + (int64_t)blockIdx.y * q_stride;
    unsigned long long c = 0;
    for (int64_t w = (int64_t)blockIdx.x * kAllowThreads + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * kAllowThreads) {
        const int64_t rows_here = n_rows - w * 32;
        const uint32_t valid = rows_here >= 32 ? 0xffffffffu : ((1u << rows_here) - 1u);   // the last word's bits past n_rows do not count
        c += (unsigned long long)__popc(bits[w] & valid);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(&counts[blockIdx.y], c);
}

inline int plan_blocks(int64_t n_rows) { return (int)(((n_rows + 31) / 32 + kAllowThreads - 1) / kAllowThreads); }

}  // namespace

hipError_t launch_allow_from_rows(const int64_t* rows, int64_t n, int64_t n_rows, uint32_t* allow, hipStream_t stream) {
    if (n < 0 || n_rows < 0 || n > 0x7fffffffLL * kAllowThreads) return hipErrorInvalidValue;
    if (n == 0 || n_rows == 0) return hipSuccess;
    if (!rows || !allow) return hipErrorInvalidValue;
    const int grid = (int)((n + kAllowThreads - 1) / kAllowThreads);
    hipLaunchKernelGGL(allow_from_rows_kernel, dim3(grid), dim3(kAllowThreads), 0, stream, rows, n, n_rows, allow);
    return hipGetLastError();
}

hipError_t launch_allow_from_tag_values(const int32_t* tags, int64_t n_rows, const int32_t* values, int n_values, int32_t mask,
                                        uint32_t* allow, hipStream_t stream) {
    if (n_rows < 0 || n_values < 0) return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    if (!tags || !allow || (n_values > 0 && !values)) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((n_rows + kAllowThreads - 1) / kAllowThreads, 2048);
    hipLaunchKernelGGL(allow_from_tag_values_kernel, dim3(grid), dim3(kAllowThreads), 0, stream, tags, n_rows, values, n_values, mask,
                       allow);
    return hipGetLastError();
}

size_t allow_plan_workspace_bytes(int64_t n_rows) {
    const size_t tiles = (size_t)((n_rows + 31) / 32);
    return (tiles * sizeof(uint32_t) + 255) / 256 * 256 + (size_t)std::max(plan_blocks(n_rows), 1) * sizeof(int32_t);
}

hipError_t launch_allow_plan(const uint32_t* allow, int64_t q_stride, int nq, int64_t n_rows, int32_t* work_tile, int32_t* work_rows,
                             uint32_t* work_mask, int32_t* n_work, void* workspace, hipStream_t stream) {
    if (!n_work || nq < 1 || nq > 32 || n_rows < 0 || n_rows > 0x7fffffc0LL || q_stride < 0) return hipErrorInvalidValue;
    if (n_rows == 0) return hipMemsetAsync(n_work, 0, sizeof(int32_t), stream);
    if (!allow || !work_tile || !work_rows || !work_mask || !workspace) return hipErrorInvalidValue;
    const int n_tiles = (int)((n_rows + 31) / 32);
    const int blocks = plan_blocks(n_rows);
    uint32_t* tile_mask = static_cast<uint32_t*>(workspace);
    int32_t* block_count =
        reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace) + ((size_t)n_tiles * sizeof(uint32_t) + 255) / 256 * 256);
    hipLaunchKernelGGL(allow_plan_mask_kernel, dim3(blocks), dim3(kAllowThreads), 0, stream, allow, q_stride, nq, n_rows, n_tiles,
                       tile_mask, block_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(allow_plan_place_kernel, dim3(blocks), dim3(kAllowThreads), 0, stream, tile_mask, block_count, n_rows, n_tiles,
                       work_tile, work_rows, work_mask, n_work);
    return hipGetLastError();
}

hipError_t launch_allow_count(const uint32_t* allow, int64_t q_stride, int n_bitmaps, int64_t n_rows, int64_t* counts, hipStream_t stream) {
    if (n_bitmaps < 1 || n_bitmaps > 65535 || n_rows < 0 || q_stride < 0 || !counts) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_bitmaps * sizeof(int64_t), stream);
    if (e != hipSuccess || n_rows == 0) return e;
    if (!allow) return hipErrorInvalidValue;
    const int64_t n_words = (n_rows + 31) / 32;
    const int grid = (int)std::min<int64_t>((n_words + kAllowThreads - 1) / kAllowThreads, 1024);
    hipLaunchKernelGGL(allow_count_kernel, dim3(grid, n_bitmaps), dim3(kAllowThreads), 0, stream, allow, q_stride, n_rows,
                       reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError();
}

hipError_t launch_allow_store(const float* scores, const int64_t* rows, int nq, int kk, int k, int kdone, int64_t id_base,
                              const int64_t* id_map, float* out_scores, int64_t* out_ids, float* after_s, int64_t* after_i,
                              hipStream_t stream) {
    if (nq < 1 || kk < 1 || kk > 32 || kdone < 0 || kdone + kk > k || !scores || !rows || !out_scores || !out_ids || !after_s || !after_i)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(allow_store_kernel, dim3(nq), dim3(32), 0, stream, scores, rows, kk, k, kdone, id_base, id_map, out_scores, out_ids,
                       after_s, after_i);
    return hipGetLastError();
}

}  // namespace rass
