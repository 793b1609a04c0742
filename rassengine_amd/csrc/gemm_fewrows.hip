// gemm_fewrows.hip — the few-rows family of the encoder GEMM: a query's rows against a wide weight matrix straight from
// global memory, and the same kernel with the LayerNorm of its input inside.
#include "gemm_common.h"

namespace rass {

// ------------------------------------------------------------------------------------------
// A few rows against a WIDE weight matrix (one query: QKV, N = 3072, and FFN-up, N = 4096, at K = 1024): no split-K and
// no second kernel.  One wave per 16 output features walks all of K straight from global memory / L2 — its 16 weight
// rows are 32 KiB, read once, 16 B per lane and MFMA (A = W rows, B = X rows: D[feature][token]) with 8 loads in
// flight — and applies the epilogue itself; N / 16 >= 128 waves stream the matrix.  Every launch of a one-query forward
// costs ~5 us whatever it does (a hipGraph replay does not change that), so the two launches saved per layer are a
// fifth of the forward.  ROWS = number of 16-token blocks (tokens <= 64).
template <int EPI, int ROWS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void gemm_bf16_fewrows_kernel(const u16* __restrict__ X, const u16* __restrict__ W,
                                                                const float* __restrict__ bias,
                                                                const u16* __restrict__ residual, u16* __restrict__ Y,
                                                                int M, int N, int K, float* __restrict__ partial,
                                                                int rows_pad) {
    // EPI = -1: K is also cut over gridDim.y workgroups; each writes its fp32 partial tile [slice][rows_pad][N] and the
    // fused reduce + residual + LayerNorm kernel follows (FFN-down: K = 4096 needs more than 64 workgroups)
    // a workgroup = 16 output features; its WAVES (4, or 16 for K >= 4096) waves take an equal share of K each (8 weight
    // loads of 16 B per lane in flight per trip), then wave 0 adds the partial tiles in wave order
    __shared__ f32x4 part[WAVES][ROWS][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 16;
    const int g = lane >> 4, i = lane & 15;
    const int kq = K / (WAVES * (int)gridDim.y), k_lo = ((int)blockIdx.y * WAVES + wave) * kq;
    const u16* wrow = W + (int64_t)(n0 + i) * K + k_lo + 8 * g;   // A operand: W[n0 + i][k_lo + 32 ks + 8 g .. +7]
    const u16* xrow = X + (int64_t)i * K + k_lo + 8 * g;          // B operand: X[16 rb + i][..] (rows < M_pad exist)
    // wave 0's epilogue operands leave with the first weight loads, not after the barrier (a dependent L2 / HBM round trip
    // at the very end of a kernel whose whole duration is 4-5 us)
    const int n = n0 + 4 * g;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    uint2 rres[ROWS];
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) rres[rb] = make_uint2(0, 0);
    if (EPI >= 0 && wave == 0) {
        bv = *reinterpret_cast<const f32x4*>(bias + n);
        if (EPI == 1) {
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) {
                const int m = 16 * rb + i;
                rres[rb] = *reinterpret_cast<const uint2*>(residual + (int64_t)(m < M ? m : 0) * N + n);
            }
        }
    }
    f32x4 acc[ROWS];
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;
    for (int k0 = 0; k0 < kq; k0 += 32 * U) {   // one trip at K = 1024 (4 waves) and 4096 (16 waves)
        bf16x8 a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const bf16x8*>(wrow + k0 + 32 * u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int rb = 0; rb < ROWS; ++rb) {
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(xrow + (int64_t)rb * 16 * K + k0 + 32 * u);
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b, acc[rb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) part[wave][rb][lane] = acc[rb];
    __syncthreads();
    if (wave != 0) return;
    // token m = 16 rb + i, features n0 + 4 g + {0..3}
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) {
        const int m = 16 * rb + i;
        if (m >= M) continue;
        f32x4 v = part[0][rb][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += part[w][rb][lane];
        if constexpr (EPI < 0) {
            *reinterpret_cast<f32x4*>(partial + ((int64_t)blockIdx.y * rows_pad + m) * N + n) = v;
            continue;
        }
        v += bv;
        if (EPI == 1) {
            const uint2 r = rres[rb];
            v.x += bf16_to_f32((u16)(r.x & 0xffff));
            v.y += bf16_to_f32((u16)(r.x >> 16));
            v.z += bf16_to_f32((u16)(r.y & 0xffff));
            v.w += bf16_to_f32((u16)(r.y >> 16));
        }
        if (EPI == 2) {
            v.x = gelu_erf(v.x);
            v.y = gelu_erf(v.y);
            v.z = gelu_erf(v.z);
            v.w = gelu_erf(v.w);
        }
        uint2 o;
        o.x = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
        o.y = (unsigned)f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
        *reinterpret_cast<uint2*>(Y + (int64_t)m * N + n) = o;
    }
}

// The few-rows GEMM whose input is LayerNorm(Yin), recomputed by EVERY workgroup into its LDS X tile (<= 16 rows of
// K = 1024: 32 KiB of L2 reads, issued behind the weight loads already in flight) instead of a LayerNorm launch in
// front (WAVES = 16, the default: a wave normalises ONE row of 16 and owns a 64-deep slice of K — normalising four rows took a
// 4-wave workgroup ~1.5 us of vector issue, in every workgroup; RASS_GEMM_LNIN_WAVES=4 keeps that form): a launch costs ~4 us here whatever it does.  Workgroup 0 also stores the normalised rows (x_out: the next
// residual).  The row arithmetic is layernorm_kernel's (wave per row, lane = 8 columns + 512 s, fp32 two-pass,
// xor-shuffle sums), so x_out has the bits the separate launch would have written.
template <int EPI, int ROWS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void gemm_bf16_lnin_kernel(const u16* __restrict__ Yin, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             u16* __restrict__ x_out, const u16* __restrict__ W,
                                                             const float* __restrict__ bias, u16* __restrict__ Y, int M,
                                                             int N) {
    constexpr int K = 1024, kPitch = K + 8;   // + 16 B: the 16 rows of a B fragment fall on different banks
    extern __shared__ __attribute__((aligned(16))) unsigned char lnin_lds[];
    u16 (*xs)[kPitch] = reinterpret_cast<u16 (*)[kPitch]>(lnin_lds);                       // [16 ROWS][kPitch]
    f32x4 (*part)[ROWS][64] = reinterpret_cast<f32x4 (*)[ROWS][64]>(lnin_lds + (size_t)16 * ROWS * kPitch * 2);  // [WAVES]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 16;
    const int g = lane >> 4, i = lane & 15;
    constexpr int UW = 32 / WAVES;   // 32-deep MFMA steps of a wave's K slice (K / WAVES)
    const int k_lo = wave * (K / WAVES);
    const u16* wrow = W + (int64_t)(n0 + i) * K + k_lo + 8 * g;
    bf16x8 a[UW];
#pragma unroll
    for (int u = 0; u < UW; ++u) a[u] = *reinterpret_cast<const bf16x8*>(wrow + 32 * u);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n0 + 4 * g);   // (wave 0's epilogue: not a round trip at the end)
    // rows wave, wave + WAVES, ...: all their loads first
    constexpr int RPW = 16 * ROWS / WAVES;   // rows per wave
    constexpr int G = RPW < 4 ? RPW : 4;     // rows reduced side by side
    uint4 raw[RPW][2];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int r = wave + WAVES * j;
        const int rc = r < M ? r : 0;
#pragma unroll
        for (int st = 0; st < 2; ++st)
            raw[j][st] = *reinterpret_cast<const uint4*>(Yin + (int64_t)rc * K + lane * 8 + 512 * st);
    }
    f32x4 gm[2][2], bt[2][2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const int c = lane * 8 + 512 * st;
        gm[st][0] = *reinterpret_cast<const f32x4*>(gamma + c);
        gm[st][1] = *reinterpret_cast<const f32x4*>(gamma + c + 4);
        bt[st][0] = *reinterpret_cast<const f32x4*>(beta + c);
        bt[st][1] = *reinterpret_cast<const f32x4*>(beta + c + 4);
    }
    __builtin_amdgcn_sched_barrier(0);   // every load above is issued before the first wait
    // four rows at a time, their wave reductions side by side: a row's arithmetic and its order are layernorm_kernel's, but
    // the 12 dependent cross-lane steps of a row (2 sums x 6 butterfly steps) overlap with the other rows' instead of running 48
    // deep, and they are DPP / permlane-swap moves, not ds_bpermute round trips (encoder_kernels.h; round 4: 8.2 -> ~5 us per launch)
#pragma unroll
    for (int j0 = 0; j0 < RPW; j0 += G) {
        float x[G][2][8], sum[G], mean[G], sq[G], rstd[G];
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const uint4 w = raw[j0 + jj][st];
                x[jj][st][0] = bf16_to_f32((u16)(w.x & 0xffff)); x[jj][st][1] = bf16_to_f32((u16)(w.x >> 16));
                x[jj][st][2] = bf16_to_f32((u16)(w.y & 0xffff)); x[jj][st][3] = bf16_to_f32((u16)(w.y >> 16));
                x[jj][st][4] = bf16_to_f32((u16)(w.z & 0xffff)); x[jj][st][5] = bf16_to_f32((u16)(w.z >> 16));
                x[jj][st][6] = bf16_to_f32((u16)(w.w & 0xffff)); x[jj][st][7] = bf16_to_f32((u16)(w.w >> 16));
            }
            sum[jj] = 0.f;
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int e = 0; e < 8; ++e) sum[jj] += x[jj][st][e];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int jj = 0; jj < G; ++jj) sum[jj] += wave_xor_partner_dpp(sum[jj], lane, off);
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
            mean[jj] = sum[jj] / (float)K;
            sq[jj] = 0.f;
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = x[jj][st][e] - mean[jj];
                    sq[jj] = fmaf(d, d, sq[jj]);
                }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int jj = 0; jj < G; ++jj) sq[jj] += wave_xor_partner_dpp(sq[jj], lane, off);
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
            rstd[jj] = rsqrtf(sq[jj] / (float)K + eps);
            const int r = wave + WAVES * (j0 + jj);
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const int c = lane * 8 + 512 * st;
                float o[8];
                o[0] = (x[jj][st][0] - mean[jj]) * rstd[jj] * gm[st][0].x + bt[st][0].x;
                o[1] = (x[jj][st][1] - mean[jj]) * rstd[jj] * gm[st][0].y + bt[st][0].y;
                o[2] = (x[jj][st][2] - mean[jj]) * rstd[jj] * gm[st][0].z + bt[st][0].z;
                o[3] = (x[jj][st][3] - mean[jj]) * rstd[jj] * gm[st][0].w + bt[st][0].w;
                o[4] = (x[jj][st][4] - mean[jj]) * rstd[jj] * gm[st][1].x + bt[st][1].x;
                o[5] = (x[jj][st][5] - mean[jj]) * rstd[jj] * gm[st][1].y + bt[st][1].y;
                o[6] = (x[jj][st][6] - mean[jj]) * rstd[jj] * gm[st][1].z + bt[st][1].z;
                o[7] = (x[jj][st][7] - mean[jj]) * rstd[jj] * gm[st][1].w + bt[st][1].w;
                uint4 pk;
                pk.x = (unsigned)f32_to_bf16(o[0]) | ((unsigned)f32_to_bf16(o[1]) << 16);
                pk.y = (unsigned)f32_to_bf16(o[2]) | ((unsigned)f32_to_bf16(o[3]) << 16);
                pk.z = (unsigned)f32_to_bf16(o[4]) | ((unsigned)f32_to_bf16(o[5]) << 16);
                pk.w = (unsigned)f32_to_bf16(o[6]) | ((unsigned)f32_to_bf16(o[7]) << 16);
#ifdef RASS_ELIM_LN   // elimination build (timing only, wrong results): the raw row instead of the normalised one
                pk = raw[j0 + jj][st];
#endif
                if (r >= M) pk = make_uint4(0, 0, 0, 0);   // rows past the batch: finite zeros in the operand tile
                *reinterpret_cast<uint4*>(&xs[r][c]) = pk;
                if (blockIdx.x == 0 && r < M) *reinterpret_cast<uint4*>(x_out + (int64_t)r * K + c) = pk;
            }
        }
    }
    __syncthreads();
    f32x4 acc[ROWS];
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < UW; ++u) {
#pragma unroll
        for (int rb = 0; rb < ROWS; ++rb) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&xs[16 * rb + i][k_lo + 32 * u + 8 * g]);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b, acc[rb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) part[wave][rb][lane] = acc[rb];
    __syncthreads();
    if (wave != 0) return;
    const int n = n0 + 4 * g;
#pragma unroll
    for (int rb = 0; rb < ROWS; ++rb) {
        const int m = 16 * rb + i;
        if (m >= M) continue;
        f32x4 v = part[0][rb][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += part[w][rb][lane];   // in wave order
        v += bv;
        if (EPI == 2) {
            v.x = gelu_erf(v.x);
            v.y = gelu_erf(v.y);
            v.z = gelu_erf(v.z);
            v.w = gelu_erf(v.w);
        }
        uint2 o;
        o.x = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
        o.y = (unsigned)f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
        *reinterpret_cast<uint2*>(Y + (int64_t)m * N + n) = o;
    }
}

template <int EPI, int WAVES>
static hipError_t launch_fewrows_w(const u16* x, const u16* w, const float* bias, const u16* r, u16* y, int M, int N, int K,
                                   hipStream_t stream, float* partial = nullptr, int rows_pad = 0, int slices = 1) {
    const dim3 grid(N / 16, slices), block(64 * WAVES);
    switch ((M + 15) / 16) {
        case 1: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 1, WAVES>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
        case 2: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 2, WAVES>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
        case 3: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 3, WAVES>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
        case 4: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 4, WAVES>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
        default:
            if constexpr (WAVES == 4) {   // 65 .. 128 rows: 4-wave workgroups only (fewrows_waves)
                switch ((M + 15) / 16) {
                    case 5: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 5, 4>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
                    case 6: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 6, 4>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
                    case 7: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 7, 4>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
                    default: hipLaunchKernelGGL((gemm_bf16_fewrows_kernel<EPI, 8, 4>), grid, block, 0, stream, x, w, bias, r, y, M, N, K, partial, rows_pad); break;
                }
            } else {
                return hipErrorInvalidValue;
            }
            break;
    }
    return hipGetLastError();
}

template <int EPI>
static hipError_t launch_fewrows_epi(int waves, const GemmOperands& a, hipStream_t stream) {
    return waves == 16 ? launch_fewrows_w<EPI, 16>(a.X, a.W, a.bias, a.residual, a.Y, a.M, a.N, a.K, stream)
                       : launch_fewrows_w<EPI, 4>(a.X, a.W, a.bias, a.residual, a.Y, a.M, a.N, a.K, stream);
}

hipError_t launch_fewrows(int epilogue, int waves, const GemmOperands& a, hipStream_t stream, float* partial, int rows_pad,
                          int slices) {
    switch (epilogue) {
        case -1:
            return waves == 4 ? launch_fewrows_w<-1, 4>(a.X, a.W, nullptr, nullptr, nullptr, a.M, a.N, a.K, stream, partial, rows_pad, slices)
                              : hipErrorInvalidValue;
        case 0: return launch_fewrows_epi<0>(waves, a, stream);
        case 1: return launch_fewrows_epi<1>(waves, a, stream);
        case 2: return launch_fewrows_epi<2>(waves, a, stream);
        default: return hipErrorInvalidValue;
    }
}

template <int EPI, int ROWS, int WAVES>
static hipError_t launch_lnin_rw(const u16* yin, const float* gamma, const float* beta, float eps, u16* x_out, const u16* w,
                                 const float* bias, u16* y, int M, int N, hipStream_t stream) {
    constexpr int lds_bytes = 16 * ROWS * (1024 + 8) * 2 + WAVES * ROWS * 64 * 16;
    if (hipError_t e = allow_dynamic_lds<&gemm_bf16_lnin_kernel<EPI, ROWS, WAVES>>(lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((gemm_bf16_lnin_kernel<EPI, ROWS, WAVES>), dim3(N / 16), dim3(64 * WAVES), lds_bytes, stream, yin, gamma,
                       beta, eps, x_out, w, bias, y, M, N);
    return hipGetLastError();
}

template <int EPI, int WAVES>
static hipError_t launch_lnin_rows(const u16* yin, const float* gamma, const float* beta, float eps, u16* xo, const u16* w,
                                   const float* bias, u16* y, int M, int N, hipStream_t stream) {
    return M <= 16 ? launch_lnin_rw<EPI, 1, WAVES>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream)
                   : launch_lnin_rw<EPI, 2, WAVES>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream);
}

hipError_t launch_lnin(int epilogue, int waves, const u16* yin, const float* gamma, const float* beta, float eps, u16* xo,
                       const u16* w, const float* bias, u16* y, int M, int N, hipStream_t stream) {
    if (waves == 4)   // the 4-wave workgroups of rounds 2-3 (RASS_GEMM_LNIN_WAVES=4: the A/B)
        return epilogue == 0 ? launch_lnin_rows<0, 4>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream)
                             : launch_lnin_rows<2, 4>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream);
    return epilogue == 0 ? launch_lnin_rows<0, 16>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream)
                         : launch_lnin_rows<2, 16>(yin, gamma, beta, eps, xo, w, bias, y, M, N, stream);
}

}  // namespace rass
