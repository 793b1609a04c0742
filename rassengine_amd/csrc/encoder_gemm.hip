// encoder_gemm.hip — K5 of SURVEY §8a: bf16 MFMA GEMM with fused epilogues for the
// sentence encoder (replaces llama.cpp's matmuls behind Ollama's /embeddings,
// reference app/main.py:225-237).
//
//   Y[M, N] = epilogue( X[M, K] (bf16, tokens x features) * W[N, K]^T (bf16, nn.Linear layout) + bias[N] )
//   epilogue: 0 = bias            (QKV projection)
//             1 = bias + residual (attention-out, FFN-down; the sum is formed in fp32)
//             2 = bias + GELU(erf) (FFN-up)
//
// This file holds the entry points only: each validates its arguments, asks gemm_route.cpp which kernel the shape gets, and
// switches on the answer.  The kernels and their launchers: gemm_tile128.hip (two-buffer, four-stage "mid", split-K pair),
// gemm_fewrows.hip (few rows, LayerNorm input), gemm_p5.hip / gemm_p4.hip (persistent); shared pieces in gemm_common.h.
#include "gemm_common.h"
#include "gemm_route.h"

namespace rass {

static int device_cus() {
    static int n_cus = 0;
    if (n_cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0)
            n_cus = 256;
    }
    return n_cus;
}

static hipError_t launch_route(const GemmRoute& r, int epilogue, const GemmOperands& a, float* ws, hipStream_t stream,
                               const LnFold& fold = LnFold{}) {
    switch (r.kind) {
        case GemmKind::FewRows: return launch_fewrows(epilogue, r.waves, a, stream);
        case GemmKind::SplitK: return launch_splitk_pair(epilogue, a, ws, r.rows_pad, r.slices, stream);
        case GemmKind::Mid: return launch_mid(epilogue, r.bm, a, r.grid, stream);
        case GemmKind::Tile128: return launch_tile128(epilogue, a, r.grid, stream);
        case GemmKind::P4: return launch_p4(epilogue, a, r.tiles, r.grid, stream, fold);
        case GemmKind::P5: return launch_p5(epilogue, r.policy, a, r.tiles, r.grid, stream, fold);
        default: return hipErrorInvalidValue;
    }
}

bool gemm_bf16_fold_shape_ok(int M, int M_pad, int N, int K) {
    return route_gemm({M, M_pad, N, K}, 3, false, 0, gemm_switches(), 256).kind != GemmKind::Unsupported;
}

bool gemm_bf16_fold_ok(int M, int M_pad, int hidden, int intermediate) {
    return gemm_fold_ok(M, M_pad, hidden, intermediate, gemm_switches());
}

bool gemm_bf16_ln_input_ok(int M, int N, int K) { return gemm_ln_input_shape_ok(M, N, K, gemm_switches()); }

// ---- LN fold: the big-batch forward without the stand-alone LayerNorm passes (see LnFold, gemm_common.h) ----------------
hipError_t launch_gemm_bf16_fold(const void* X, const void* W, const float* bias, const void* residual_raw, void* Y, int M,
                                 int M_pad, int N, int K, int epilogue, const float* mr, const float* gamma, const float* beta,
                                 float* stats, const float* colsum, hipStream_t stream) {
    if (epilogue < 3 || epilogue > 5 || !mr) return hipErrorInvalidValue;
    const GemmRoute route = route_gemm({M, M_pad, N, K}, epilogue, false, 0, gemm_switches(), device_cus());
    if (route.kind == GemmKind::Unsupported) return hipErrorInvalidValue;
    if (epilogue == 3 ? !(residual_raw && gamma && beta && stats) : !colsum) return hipErrorInvalidValue;
    LnFold f;
    f.mr = mr;
    f.gamma = gamma;
    f.beta = beta;
    f.stats = stats;
    f.colsum = colsum;
    const GemmOperands a{static_cast<const u16*>(X), static_cast<const u16*>(W), bias,
                         epilogue == 3 ? static_cast<const u16*>(residual_raw) : nullptr, static_cast<u16*>(Y), M, N, K};
    return launch_route(route, epilogue, a, nullptr, stream, f);
}

hipError_t launch_gemm_bf16(const void* X, const void* W, const float* bias, const void* residual, void* Y, int M,
                            int M_pad, int N, int K, int epilogue, hipStream_t stream, float* splitk_ws,
                            size_t splitk_ws_bytes) {
    if (M < 0 || M_pad < M || N <= 0 || K <= 0) return hipErrorInvalidValue;
    // every kernel here works on whole 128-row / 128-column tiles and 64-deep K steps (include/rass_engine.h)
    if (M_pad % GBM != 0 || N % GBN != 0 || K % GBK != 0) return hipErrorInvalidValue;
    if (M == 0) return hipSuccess;
    if (epilogue < 0 || epilogue > 2 || (epilogue == 1 && !residual)) return hipErrorInvalidValue;
    const GemmOperands a{static_cast<const u16*>(X), static_cast<const u16*>(W), bias, static_cast<const u16*>(residual),
                         static_cast<u16*>(Y), M, N, K};
    const GemmRoute route = route_gemm({M, M_pad, N, K}, epilogue, splitk_ws != nullptr, splitk_ws_bytes, gemm_switches(), device_cus());
    return launch_route(route, epilogue, a, splitk_ws, stream);
}

hipError_t launch_gemm_bf16_residual_layernorm(const void* X, const void* W, const float* bias, const void* residual,
                                               void* y, const float* gamma, const float* beta, float eps, void* out,
                                               int M, int M_pad, int N, int K, hipStream_t stream, float* splitk_ws,
                                               size_t splitk_ws_bytes) {
    if (M < 0 || M_pad < M || N <= 0 || K <= 0 || !residual) return hipErrorInvalidValue;
    if (M == 0) return hipSuccess;
    const ResidualRoute route = route_gemm_residual_layernorm({M, M_pad, N, K}, splitk_ws != nullptr, splitk_ws_bytes, gemm_switches());
    if (route.tail == ResidualTail::GemmThenLn) {
        hipError_t e = launch_gemm_bf16(X, W, bias, residual, y, M, M_pad, N, K, 1, stream, splitk_ws, splitk_ws_bytes);
        if (e != hipSuccess) return e;
        return launch_layernorm(y, gamma, beta, eps, M, N, out, stream);
    }
    // partial tiles into the scratch, then ONE kernel that reduces them, adds bias and residual and normalises
    const GemmOperands a{static_cast<const u16*>(X), static_cast<const u16*>(W), nullptr, nullptr, nullptr, M, N, K};
    hipError_t e = route.tail == ResidualTail::FewRows4Ln
                       ? launch_fewrows(-1, 4, a, stream, splitk_ws, route.rows_pad, route.slices)
                       : launch_splitk_pair(-1, a, splitk_ws, route.rows_pad, route.slices, stream);
    if (e != hipSuccess) return e;
    return launch_splitk_residual_layernorm(splitk_ws, route.slices, M, route.rows_pad, N, bias, residual, gamma, beta, eps, out, stream);
}

hipError_t launch_gemm_bf16_ln_input(const void* Yin, const float* gamma, const float* beta, float eps, void* x_out,
                                     const void* W, const float* bias, void* Y, int M, int N, int K, int epilogue,
                                     hipStream_t stream) {
    const GemmSwitches& sw = gemm_switches();
    if (!gemm_ln_input_shape_ok(M, N, K, sw) || (epilogue != 0 && epilogue != 2)) return hipErrorInvalidValue;
    return launch_lnin(epilogue, sw.lnin_waves, static_cast<const u16*>(Yin), gamma, beta, eps, static_cast<u16*>(x_out),
                       static_cast<const u16*>(W), bias, static_cast<u16*>(Y), M, N, stream);
}

}  // namespace rass
