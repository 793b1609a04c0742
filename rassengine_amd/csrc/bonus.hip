// bonus.hip — the builders of the dense fp32 bonus columns that the boosted scan (scan_boost.hip) adds to boost * T(cos):
// scatter of (query, row, value) triples (text hits), weighted clauses over the int32 attribute columns (should-clauses:
// term / terms / range / exists), and the mask that writes -inf where a row bitmap has no bit (a `where` filter).  A column
// block is [n_bonus][stride] floats owned by the caller; zero-filling is a hipMemsetAsync on the engine's stream.
//
// Every value is built from separately rounded fp32 adds in a stated order, so a numpy restatement reproduces a column word
// for word (tests/boost_ref.py).  One thread per row, coalesced loads and stores over rows; clause records sit at
// wave-uniform addresses.  Plain vector loads and stores only; no atomics (scatter's pairs are unique by contract); no
// workgroup waits on another.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kBonusThreads = 256;
constexpr int32_t kAttrMissing = INT32_MIN;

__global__ __launch_bounds__(kBonusThreads) void bonus_scatter_kernel(const int32_t* __restrict__ q_of, const int64_t* __restrict__ rows,
                                                                      const float* __restrict__ values, int64_t n,
                                                                      float* __restrict__ bonus, int64_t stride) {
    for (int64_t i = (int64_t)blockIdx.x * kBonusThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBonusThreads) {
        float* cell = bonus + (int64_t)q_of[i] * stride + rows[i];
        *cell = __fadd_rn(*cell, values[i]);
    }
}

// `clauses`, `weights`, `q_off` and `bonus` are a's fields again, as parameters of their own: only there does __restrict__
// tell the compiler that the column stores cannot change the clause list, which lets it read the clauses with scalar loads.
__global__ __launch_bounds__(kBonusThreads) void bonus_clauses_kernel(const BonusClauseArgs a, const int4* __restrict__ clauses,
                                                                      const float* __restrict__ weights,
                                                                      const int32_t* __restrict__ q_off, float* __restrict__ bonus) {
    for (int64_t r = (int64_t)blockIdx.x * kBonusThreads + threadIdx.x; r < a.n_rows; r += (int64_t)gridDim.x * kBonusThreads) {
        // the row's eight attribute values, fully unrolled over the kernel arguments: no array is indexed by a run-time column
        int32_t v[kAttrCols];
#pragma unroll
        for (int c = 0; c < kAttrCols; ++c) v[c] = a.col[c] != nullptr ? a.col[c][r] : kAttrMissing;
        for (int q = 0; q < a.nq; ++q) {
            float* cell = bonus + (int64_t)q * a.stride + r;
            float acc = a.add ? *cell : 0.f;
            const int first = q_off[q], last = q_off[q + 1];
            for (int j = first; j < last; ++j) {
                const int4 cl = clauses[j];   // {col, lo, hi, negate}: the same address in every lane
                int32_t x = kAttrMissing;
#pragma unroll
                for (int c = 0; c < kAttrCols; ++c) x = cl.x == c ? v[c] : x;   // a uniform select chain
                const bool holds = (x != kAttrMissing && cl.y <= x && x <= cl.z) != (cl.w != 0);
                const float sum = __fadd_rn(acc, weights[j]);
                acc = holds ? sum : acc;
            }
            *cell = acc;
        }
    }
}

__global__ __launch_bounds__(kBonusThreads) void bonus_mask_kernel(float* __restrict__ bonus, int64_t stride, int64_t n_rows,
                                                                   const uint32_t* __restrict__ allow, int64_t allow_q_stride) {
    const int q = blockIdx.y;
    for (int64_t r = (int64_t)blockIdx.x * kBonusThreads + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kBonusThreads) {
        const uint32_t w = allow[(int64_t)q * allow_q_stride + (r >> 5)];
        if (((w >> (r & 31)) & 1u) == 0u) bonus[(int64_t)q * stride + r] = -INFINITY;
    }
}

int grid_for(int64_t n) { return (int)std::min<int64_t>((n + kBonusThreads - 1) / kBonusThreads, 2048); }

}  // namespace

hipError_t launch_bonus_scatter(const int32_t* q_of, const int64_t* rows, const float* values, int64_t n, float* bonus, int64_t stride,
                                hipStream_t stream) {
    if (n < 0 || stride < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (!q_of || !rows || !values || !bonus) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bonus_scatter_kernel, dim3(grid_for(n)), dim3(kBonusThreads), 0, stream, q_of, rows, values, n, bonus, stride);
    return hipGetLastError();
}

hipError_t launch_bonus_clauses(const BonusClauseArgs& a, hipStream_t stream) {
    if (a.n_rows < 0 || a.nq < 1 || a.nq > 32 || a.stride < a.n_rows || (a.add != 0 && a.add != 1)) return hipErrorInvalidValue;
    if (a.n_rows == 0) return hipSuccess;
    if (!a.bonus || !a.q_off) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bonus_clauses_kernel, dim3(grid_for(a.n_rows)), dim3(kBonusThreads), 0, stream, a, a.clauses, a.weights, a.q_off,
                       a.bonus);
    return hipGetLastError();
}

hipError_t launch_bonus_mask(float* bonus, int n_bonus, int64_t stride, int64_t n_rows, const uint32_t* allow, int64_t allow_q_stride,
                             hipStream_t stream) {
    if (n_bonus < 1 || n_bonus > 65535 || n_rows < 0 || stride < n_rows || allow_q_stride < 0) return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    if (!bonus || !allow) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bonus_mask_kernel, dim3(grid_for(n_rows), n_bonus), dim3(kBonusThreads), 0, stream, bonus, stride, n_rows, allow,
                       allow_q_stride);
    return hipGetLastError();
}

}  // namespace rass
