// gemm_common.h — what the encoder GEMM units share (gemm_tile128.hip, gemm_fewrows.hip, gemm_p5.hip, gemm_p4.hip and the
// entry points in encoder_gemm.hip): vector types, bf16 conversion, GELU, the 128 x 64 operand tile's staging and fragment
// read, the tile constants, LnFold, and the per-family launchers that encoder_gemm.hip switches over (gemm_route.h decides).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "encoder_kernels.h"

namespace rass {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int GBM = 128, GBN = 128, GBK = 64;
constexpr int kGemmThreads = 256;
constexpr int kTileBytes = 128 * GBK * 2;  // one operand tile: 128 rows x 64 bf16 = 16 KiB

__device__ __forceinline__ float bf16_to_f32(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ u16 f32_to_bf16(float f) {
    // round-to-nearest-even; NaN stays NaN through the plain conversion instruction
    __hip_bfloat16 h = __float2bfloat16(f);
    return *reinterpret_cast<u16*>(&h);
}

// GELU(x) = x/2 * (1 + erf(x/sqrt2)) (the erf form of BERT's "gelu").  libm's erff costs ~3x the epilogue budget (the FFN-up
// GEMM ran at 510 TF/s with it vs 780 without); rounds 1-3 used Abramowitz-Stegun 7.1.26 (a reciprocal and an exponential).
__device__ __forceinline__ float gelu_erf(float x) {
    // With h = |x|/2 and z = |x|/sqrt2:  GELU(x) = max(x, 0) - h * erfc(z).  Round 4: erfc(z) = exp2(Q(h)), Q the degree-7
    // least-squares fit of log2(erfc(h sqrt2)) on z in [0, 5] (|rel. error| of erfc < 1.2e-5, so |error| of GELU < 1.5e-6
    // everywhere, two orders below the bf16 resolution of the output; beyond z = 5 erfc < 2e-12 and h is clamped): one
    // transcendental and 12 plain instructions per element, all of them packable — the Abramowitz-Stegun form it replaces
    // (|error| 2e-7) took 12 + a reciprocal + an exponential, and the GELU epilogue of FFN-up is VALU-bound (8-11 us per
    // 256 x 256 tile, profiles/r04_gemm_epilogue_experiments.txt).  scripts/fit_gelu_poly.py derives and checks the constants.
#ifdef RASS_GELU_AS   // rounds 1-3 (the A/B build): Abramowitz-Stegun 7.1.26, 1 - erf(z) = p(t) exp(-z^2), t = 1 / (1 + 0.3275911 z)
    {
        const float h = 0.5f * fabsf(x);
        const float t = __builtin_amdgcn_rcpf(fmaf(0.46328375849f, h, 1.0f));
        float p = fmaf(1.061405429f, t, -1.453152027f);
        p = fmaf(p, t, 1.421413741f);
        p = fmaf(p, t, -0.284496736f);
        p = fmaf(p, t, 0.254829592f);
        p *= t;
        const float zz = h * 1.69864357838f;
        return fmaf(-h, p * __builtin_amdgcn_exp2f(-zz * zz), fmaxf(x, 0.0f));
    }
#endif
    const float h = 0.5f * fabsf(x);
    const float hc = fminf(h, 3.5355339f);
    float q = -2.0300099e-04f;
    q = fmaf(q, hc, 3.5955482e-03f);
    q = fmaf(q, hc, -2.8301010e-02f);
    q = fmaf(q, hc, 1.3302942e-01f);
    q = fmaf(q, hc, -4.2836797e-01f);
    q = fmaf(q, hc, -1.8355303e+00f);
    q = fmaf(q, hc, -2.3021889e+00f);
    q = fmaf(q, hc, -4.7392123e-06f);
    const float e = __builtin_amdgcn_exp2f(q);
    return fmaf(-h, e, fmaxf(x, 0.0f));
}

// Stage one 128 x 64 bf16 operand tile (rows row0.., columns k0..k0+63 of a [rows][ld] matrix)
// into LDS: 16 wave-instructions of 1 KiB; wave w issues pieces w, w+4, w+8, w+12.
__device__ __forceinline__ void stage_tile(const u16* __restrict__ g, int64_t ld, int row0, int k0,
                                           unsigned char* lds_tile, int wave, int lane) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int piece = wave + 4 * p;           // 8 rows per piece
        const int r = piece * 8 + (lane >> 3);    // tile row this lane fills
        const int c_store = lane & 7;             // chunk position in the LDS row (lane-linear)
        const int c_src = c_store ^ ((r >> 1) & 7);
        const u16* src = g + (int64_t)(row0 + r) * ld + k0 + c_src * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(lds_tile + piece * 1024), 16, 0, 0);
    }
}

__device__ __forceinline__ bf16x8 read_frag(const unsigned char* lds_tile, int row, int chunk) {
    const int c = chunk ^ ((row >> 1) & 7);
    return *reinterpret_cast<const bf16x8*>(lds_tile + row * 128 + c * 16);
}

#define RASS_DS_READ_B128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))

constexpr int RBM = 256, RBN = 256;       // tile of the persistent kernel
constexpr int kRingThreads = 512;         // 2 (N) x 4 (M) waves, each 128 x 64 = 8 x 4 MFMA tiles
constexpr int kPStageTokens = 32;         // tokens per epilogue staging chunk (8 704 B per wave at a pitch of 68 floats)
constexpr int kP5HalfBytes = 32768;
constexpr int kP5LdsBytes = 5 * kP5HalfBytes;

// ---- LayerNorm folded into the GEMMs around it (round 4; EPI 3 / 4 / 5) ------------------------------------------------
// The post-LN encoder layer is  h1 = LN1(x + attn(x) Wo),  h2 = LN2(h1 + gelu(h1 Wup) Wdown).  The stand-alone LayerNorm kernel
// is HBM-bound (read + write of [T, 1024] bf16 at 5.9 TB/s = 90.7 us, twice per layer = 5.2 % of the forward) and a "thin"
// normalise pass would move the same bytes; what removes the pass is algebra:
//     LN(r) W^T = rstd * (r W'^T  -  mu * colsum(W'))  +  (beta W^T + b),      W' = W diag(gamma)  (bf16, prepared at load)
// so the CONSUMER GEMM (QKV / FFN-up) runs on the raw, un-normalised sums r with pre-scaled weights and applies the row's
// (mu, rstd) and a rank-1 correction in its epilogue (EPI 4: + bias', EPI 5: + bias' + GELU), and the RESIDUAL GEMM
// (attn-out / FFN-down, EPI 3) rebuilds the normalised residual LN_prev(r_prev) element by element from (r_prev, mu, rstd,
// gamma, beta) on the fly, writes the raw sum r (bf16) and, per row and 128-column chunk, the partial sums (S r, S r^2) of the
// ROUNDED values — no atomics: [row][chunk][2] floats, summed in fixed order by ln_stats_finalize_kernel into (mu, rstd).
struct LnFold {
    const float* mr = nullptr;        // EPI 3 / 4 / 5: [rows][2] (mean, rstd) of the rows of `residual` (EPI 3) or of X (EPI 4 / 5)
    const float* gamma = nullptr;     // EPI 3: gamma / beta of the LayerNorm that produced the residual, [N]
    const float* beta = nullptr;
    float* stats = nullptr;           // EPI 3: out, [rows][N / 128][2] partial (sum, sum of squares) of the stored bf16 values
    const float* colsum = nullptr;    // EPI 4 / 5: [N] column sums of W' (fp32 sums of its bf16 values)
};

// xor-reductions inside groups of 8 consecutive lanes on DPP (quad_perm [1,0,3,2], [2,3,0,1], then row_half_mirror)
__device__ __forceinline__ float sum8_dpp(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));
    return v;
}

// A kernel whose dynamic LDS exceeds 64 KiB needs the attribute once per process (per kernel instantiation).
template <auto Kernel>
inline hipError_t allow_dynamic_lds(int bytes) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    return hipSuccess;
}

// ---- the per-family launchers: one launch each, of the kernel and with the parameters a GemmRoute names ----
struct GemmOperands {
    const u16* X;
    const u16* W;
    const float* bias;
    const u16* residual;
    u16* Y;
    int M, N, K;
};
// gemm_tile128.hip: `grid` tiles of 128 x 128 (two-buffer kernel) or of bm x 128 (four-stage kernel); the split-K pair:
// S slices of fp32 partial tiles [S][rows_pad][N] into `ws`, then the reducing epilogue (epilogue < 0: the caller reduces)
hipError_t launch_tile128(int epilogue, const GemmOperands& a, int grid, hipStream_t stream);
hipError_t launch_mid(int epilogue, int bm, const GemmOperands& a, int grid, hipStream_t stream);
hipError_t launch_splitk_pair(int epilogue, const GemmOperands& a, float* ws, int rows_pad, int S, hipStream_t stream);
// gemm_fewrows.hip: epilogue -1 writes `slices` fp32 partial tiles [slice][rows_pad][N] (4-wave workgroups only)
hipError_t launch_fewrows(int epilogue, int waves, const GemmOperands& a, hipStream_t stream, float* partial = nullptr,
                          int rows_pad = 0, int slices = 1);
hipError_t launch_lnin(int epilogue, int waves, const u16* yin, const float* gamma, const float* beta, float eps, u16* x_out,
                       const u16* w, const float* bias, u16* y, int M, int N, hipStream_t stream);
// gemm_p5.hip / gemm_p4.hip: the persistent 256 x 256 kernels, `grid` workgroups over `tiles` tiles; epilogue 0 .. 5
hipError_t launch_p5(int epilogue, int policy, const GemmOperands& a, int tiles, int grid, hipStream_t stream, const LnFold& fold);
hipError_t launch_p4(int epilogue, const GemmOperands& a, int tiles, int grid, hipStream_t stream, const LnFold& fold);

}  // namespace rass
