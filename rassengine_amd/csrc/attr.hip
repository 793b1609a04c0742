// attr.hip — the predicate kernel behind rass_index_allow_from_attr_clauses: range / term clauses over the int32 attribute
// columns of a flat index, evaluated for up to 32 queries per row in one pass, written as the allow-list bitmaps that
// scan_topk.hip's ScanMode kAllow consumes (bit (r & 31) of word r >> 5 allows row r; see allow.hip).
//
// One thread per row, block-uniform strides as in allow_from_tag_values_kernel.  A thread keeps ONE 32-bit register for its
// row: bit q is query q's verdict so far (1 under ALL, 0 under ANY to start with).  The host has ordered the clause list by
// column (AttrArgs::col_off): the kernel walks the eight columns with a fully unrolled loop — so no array is indexed by a
// run-time column number and nothing goes to scratch —, skips a column no clause names, loads a named column's value once
// (coalesced) and walks that column's clauses, whose {query, lo, hi, negate} sit at wave-uniform addresses (scalar loads).
// Afterwards the ballot of bit q is 64 rows of query q's bitmap = two words, which lanes 0 and 32 combine with what the
// bitmap already holds and store.  allow_combine_kernel is the word-wise and / or / and-not of two whole bitmaps, for the
// formulas one builder call cannot fold.  Plain vector loads, stores and ballots; no workgroup waits on another; every branch
// that leads to a ballot is wave-uniform.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kAttrThreads = 256;
constexpr int32_t kAttrMissing = INT32_MIN;

// `clauses` and `allow` are a.clauses and a.allow again, as parameters of their own: only there does __restrict__ tell the
// compiler that the bitmap stores cannot change the clause list, which is what lets it read the clauses with scalar loads.
__global__ __launch_bounds__(kAttrThreads) void attr_clauses_kernel(const AttrArgs a, const int4* __restrict__ clauses,
                                                                    uint32_t* __restrict__ allow) {
    const int lane = threadIdx.x & 63;
    const int64_t span_words = (a.span_rows + 31) >> 5;
    // block-uniform trip count: every lane reaches the ballots
    for (int64_t base = (int64_t)blockIdx.x * kAttrThreads; base < a.span_rows; base += (int64_t)gridDim.x * kAttrThreads) {
        const int64_t r = base + threadIdx.x;
        const bool in_rows = r < a.n_rows;
        uint32_t bits = a.mode_any ? 0u : 0xffffffffu;
#pragma unroll
        for (int c = 0; c < kAttrCols; ++c) {
            const int first = a.col_off[c], last = a.col_off[c + 1];
            if (first == last) continue;   // kernel arguments: uniform
            const int32_t* col = a.col[c];
            const int32_t v = (col != nullptr && in_rows) ? col[r] : kAttrMissing;   // a column never set is all-missing
            for (int j = first; j < last; ++j) {
                const int4 cl = clauses[j];   // {query, lo, hi, negate}: the same address in every lane
                const bool holds = (v != kAttrMissing && cl.y <= v && v <= cl.z) != (cl.w != 0);
                const uint32_t bit = 1u << cl.x;
                if (a.mode_any) bits |= holds ? bit : 0u;
                else bits &= holds ? 0xffffffffu : ~bit;
            }
        }
        const bool live = in_rows && a.tags[r] != -1;
        if (!live) bits = 0u;   // tombstones and the positions past the rows allow nothing
        const int64_t w = r >> 5;
        const bool writer = (lane & 31) == 0 && w < span_words;
        for (int q = 0; q < a.nq; ++q) {
            const unsigned long long b = __ballot((bits >> q) & 1u);
            if (writer) {
                uint32_t* dst = allow + (int64_t)q * a.q_stride + w;
                const uint32_t mine = (lane & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
                if (a.combine == 0) *dst = mine;
                else if (a.combine == 1) *dst = *dst & mine;
                else *dst = *dst | mine;
            }
        }
    }
}

// dst[i] = dst[i] op src[i] over the words of a bitmap: 1 = and, 2 = or, 3 = and-not (dst & ~src).
__global__ __launch_bounds__(kAttrThreads) void allow_combine_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                                     int64_t words, int op) {
    for (int64_t i = (int64_t)blockIdx.x * kAttrThreads + threadIdx.x; i < words; i += (int64_t)gridDim.x * kAttrThreads) {
        const uint32_t d = dst[i], s = src[i];
        dst[i] = op == 1 ? (d & s) : op == 2 ? (d | s) : (d & ~s);
    }
}

}  // namespace

hipError_t launch_allow_combine(uint32_t* dst, const uint32_t* src, int64_t words, int op, hipStream_t stream) {
    if (words < 0 || op < 1 || op > 3) return hipErrorInvalidValue;
    if (words == 0) return hipSuccess;
    if (!dst || !src) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((words + kAttrThreads - 1) / kAttrThreads, 2048);
    hipLaunchKernelGGL(allow_combine_kernel, dim3(grid), dim3(kAttrThreads), 0, stream, dst, src, words, op);
    return hipGetLastError();
}

hipError_t launch_attr_clauses(const AttrArgs& a, hipStream_t stream) {
    if (a.n_rows < 0 || a.span_rows < 0 || a.nq < 1 || a.nq > 32 || a.combine < 0 || a.combine > 2 || a.q_stride < 0)
        return hipErrorInvalidValue;
    if (a.span_rows == 0) return hipSuccess;
    if (!a.allow || (a.n_rows > 0 && !a.tags) || a.col_off[0] != 0) return hipErrorInvalidValue;
    for (int c = 0; c < kAttrCols; ++c)
        if (a.col_off[c + 1] < a.col_off[c]) return hipErrorInvalidValue;
    if (a.col_off[kAttrCols] > 0 && !a.clauses) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((a.span_rows + kAttrThreads - 1) / kAttrThreads, 2048);
    hipLaunchKernelGGL(attr_clauses_kernel, dim3(grid), dim3(kAttrThreads), 0, stream, a, a.clauses, a.allow);
    return hipGetLastError();
}

}  // namespace rass
