// exact_score.h — one K slice of a row's exact fp32 score from the tile16 slab, in the flat kernel's order: the fmaf chain
// of v_mfma_f32_16x16x4_f32 (chunk j, component i, lane group g) from zero.  The 8 slice partials added in slice order
// (p0 + ... + p7) are the flat scan's score of the row, bit for bit.  Shared by the exact re-rank (scan_bf16.hip) and the
// sample floor's rescore (sample_rep.hip).  Not part of any ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_core.h"

namespace rass {

// Slice w (0..7) of `row` against query q of q_padded ([..][stride] normalised floats).  CH = chunks per slice (stride / 128; wide
// rows: stride / 256 with HALVES = 2, the slice walked in two halves of CH chunks, the chain running on across them), a template
// parameter so that a half's 4 CH row loads are all in flight before the first fmaf.
template <int CH, int HALVES>
__device__ __forceinline__ float flat_score_slice(const float* __restrict__ slab, int64_t stride, const float* __restrict__ q_padded,
                                                  int q, int64_t row, int w) {
    float acc = 0.f;
#pragma unroll
    for (int half = 0; half < HALVES; ++half) {
        const float* xb = slab + (row >> 4) * 16 * stride + (int64_t)(w * HALVES * CH + half * CH) * 256 + (int)(row & 15) * 4;
        const float* qv = q_padded + (int64_t)q * stride + (w * HALVES * CH + half * CH) * 16;
        f32x4 xv[CH][4];
#pragma unroll
        for (int j = 0; j < CH; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) xv[j][g] = *reinterpret_cast<const f32x4*>(xb + j * 256 + g * 64);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            f32x4 qq[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) qq[g] = *reinterpret_cast<const f32x4*>(qv + j * 16 + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc = fmaf(xv[j][g][i], qq[g][i], acc);
        }
    }
    return acc;
}

}  // namespace rass
