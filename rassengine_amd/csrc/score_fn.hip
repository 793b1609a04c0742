// score_fn.hip — the builder of the function columns that the function-score scan (scan_fscore.hip) combines with the
// similarity: OpenSearch's function_score.functions — decay (gauss / exp / linear), field_value_factor and weight, each with
// an optional filter bitmap and a weight — over the int32 attribute columns, folded per row by a score_mode and capped by
// max_boost.  A column block is [nq][stride] floats owned by the caller, as a bonus block is.
//
// ALL arithmetic is double and each operation is rounded on its own (the Makefile turns contraction off for this object); the
// one rounding to fp32 is the store.  Cells built only from + - * / sqrt, max / min and comparisons are therefore what an IEEE
// fp64 restatement gives, bit for bit; cells that pass through exp or a logarithm differ from it by what two libm's differ
// by, a few fp64 ulps, before the rounding to fp32 (tests/fscore_ref.py).  max / min are a compare and a select.  The
// per-function constants (ln(decay) / scale^2 and the like) come ready-made from the host (api_fscore.hip).
//
// One thread per row, coalesced loads and stores over rows; function records and the row's bitmap word sit at wave-uniform
// or coalesced addresses.  Plain vector loads and stores only; no atomics; no workgroup waits on another.  The builder moves
// 4 bytes per (row, column) plus the attribute columns: next to a corpus pass it is nothing, whatever the fp64 rate.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace rass {

namespace {

constexpr int kFnThreads = 256;
constexpr int32_t kAttrMissing = INT32_MIN;

// modifier(x), OpenSearch's FieldValueFactorFunction.Modifier: 0 none, 1 log, 2 log1p, 3 log2p, 4 ln, 5 ln1p, 6 ln2p,
// 7 square, 8 sqrt, 9 reciprocal.  A non-positive argument of a logarithm gives -inf / NaN: the scan drops the row.
__device__ __forceinline__ double apply_modifier(int mod, double x) {
    switch (mod) {
        case 1: return log10(x);
        case 2: return log10(1.0 + x);
        case 3: return log10(2.0 + x);
        case 4: return log(x);
        case 5: return log(1.0 + x);
        case 6: return log(2.0 + x);
        case 7: return x * x;
        case 8: return sqrt(x);
        case 9: return 1.0 / x;
        default: return x;
    }
}

// `recs`, `q_off`, `filters` and `out` are a's fields again, as parameters of their own: only there does __restrict__ tell the
// compiler that the column stores cannot change the records (bonus.hip).
__global__ __launch_bounds__(kFnThreads) void score_fn_kernel(const ScoreFnArgs a, const ScoreFnRec* __restrict__ recs,
                                                              const int32_t* __restrict__ q_off, const uint32_t* __restrict__ filters,
                                                              float* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * kFnThreads + threadIdx.x; r < a.n_rows; r += (int64_t)gridDim.x * kFnThreads) {
        int32_t v[kAttrCols];
#pragma unroll
        for (int c = 0; c < kAttrCols; ++c) v[c] = a.col[c] != nullptr ? a.col[c][r] : kAttrMissing;
        for (int q = 0; q < a.nq; ++q) {
            const int first = q_off[q], last = q_off[q + 1];
            double acc = 1.0, wsum = 0.0;   // acc: the fold so far (avg: the sum of the values); wsum: avg's sum of weights
            bool any = false;
            for (int j = first; j < last; ++j) {
                const ScoreFnRec f = recs[j];   // the same address in every lane
                int32_t xi = kAttrMissing;
#pragma unroll
                for (int c = 0; c < kAttrCols; ++c) xi = f.col == c ? v[c] : xi;   // a uniform select chain
                bool applies = true;
                if (f.filter >= 0) applies = ((filters[(int64_t)f.filter * a.words + (r >> 5)] >> (r & 31)) & 1u) != 0u;
                const bool miss = xi == kAttrMissing;
                double x;
                if (f.kind <= 2) {   // decay
                    const double dist = fabs((double)xi - f.p0) - f.p1;
                    const double d = dist > 0.0 ? dist : 0.0;
                    if (f.kind == 0) {
                        x = exp(d * d * f.c);
                    } else if (f.kind == 1) {
                        x = exp(d * f.c);
                    } else {
                        const double l = (f.c - d) / f.c;
                        x = l > 0.0 ? l : 0.0;
                    }
                    x = miss ? 1.0 : x;
                } else if (f.kind == 3) {   // field_value_factor
                    applies = applies && !(miss && f.missing != f.missing);
                    x = apply_modifier(f.modifier, f.p0 * (miss ? f.missing : (double)xi));
                } else {
                    x = 1.0;
                }
                x = f.weight * x;
                if (!applies) continue;
                double next;
                switch (a.score_mode) {   // a kernel argument
                    case 0: next = acc * x; break;
                    case 1:
                    case 2: next = acc + x; break;
                    case 3: next = acc; break;
                    case 4: next = x > acc ? x : acc; break;
                    default: next = x < acc ? x : acc; break;
                }
                acc = any ? next : x;       // the first applying function starts the fold with its own value
                wsum = wsum + f.weight;
                any = true;
            }
            double val = 1.0;
            if (any) {
                val = a.score_mode == 2 ? acc / wsum : acc;
                val = val > a.max_boost ? a.max_boost : val;
            }
            out[(int64_t)q * a.stride + r] = (float)val;
        }
    }
}

}  // namespace

hipError_t launch_score_fn(const ScoreFnArgs& a, hipStream_t stream) {
    if (a.n_rows < 0 || a.nq < 1 || a.nq > 32 || a.stride < a.n_rows || a.score_mode < 0 || a.score_mode > 5 || a.words < 0)
        return hipErrorInvalidValue;
    if (a.max_boost != a.max_boost) return hipErrorInvalidValue;
    if (a.n_rows == 0) return hipSuccess;
    if (!a.out || !a.q_off) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((a.n_rows + kFnThreads - 1) / kFnThreads, 2048);
    hipLaunchKernelGGL(score_fn_kernel, dim3(grid), dim3(kFnThreads), 0, stream, a, a.recs, a.q_off, a.filters, a.out);
    return hipGetLastError();
}

}  // namespace rass
