// gemm_tile128.hip — the 128^2 family of the encoder GEMM (K5 of SURVEY §8a): the two-buffer kernel, its four-stage "mid"
// form and the split-K pair.  (encoder_gemm.hip holds the entry points, gemm_route.cpp the rule that picks a kernel.)
// sentence encoder (replaces llama.cpp's matmuls behind Ollama's /embeddings,
// reference app/main.py:225-237).
//
//   Y[M, N] = epilogue( X[M, K] (bf16, tokens x features) * W[N, K]^T (bf16, nn.Linear layout) + bias[N] )
//   epilogue: 0 = bias            (QKV projection)
//             1 = bias + residual (attention-out, FFN-down; the sum is formed in fp32)
//             2 = bias + GELU(erf) (FFN-up)
//
// Structure (guide §5, LDS-staged, both operands K-contiguous):
//   * 128 (N) x 128 (M) x 64 (K) block tile, 256 threads = 2x2 waves, each wave 64 x 64 =
//     4 x 4 tiles of v_mfma_f32_16x16x32_bf16; fp32 accumulators (64 VGPRs)
//   * W is the MFMA A operand (rows = output features), X the B operand (cols = tokens): the
//     accumulator then holds 4 CONSECUTIVE output features of one token per tile, so the
//     epilogue reads bias / residual and writes Y as 8-byte pieces along N
//   * staging by global_load_lds (16 B per lane, 1 KiB per wave instruction: 8 rows x 128 B),
//     two LDS buffers, one barrier per K step; the LDS image is lane-linear, the bank-conflict
//     swizzle (16-B chunk c of row r stored at chunk c ^ ((r>>1)&7)) is applied to the global
//     SOURCE address and to the ds_read_b128 address (guide rule 21)
//   * M is padded to 128 by the caller (activations workspace); rows are independent, so
//     padding rows only ever produce padding rows.

#include "gemm_common.h"

namespace rass {

template <int EPI>
__global__ __launch_bounds__(kGemmThreads, 2) void gemm_bf16_kernel(const u16* __restrict__ X, const u16* __restrict__ W,
                                                                   const float* __restrict__ bias,
                                                                   const u16* __restrict__ residual,
                                                                   u16* __restrict__ Y, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [2 buf][W tile | X tile]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave >> 1, wm = wave & 1;
    // XCD-aware remap: blocks b and b+8 share an L2, so give each XCD a contiguous run of
    // token tiles that re-use the same weight panel (guide T1, bijective form)
    const int nblk = gridDim.x;
    const int orig = blockIdx.x;
    const int q = nblk / 8, rr = nblk % 8, xcd = orig % 8;
    const int bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
    const int tiles_n = N / GBN;
    const int bn = bid % tiles_n, bm = bid / tiles_n;
    const int n0 = bn * GBN, m0 = bm * GBM;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / GBK;
    stage_tile(W, K, n0, 0, lds, wave, lane);
    stage_tile(X, K, m0, 0, lds + kTileBytes, wave, lane);
    __syncthreads();  // hipcc drains the pending LDS-DMA (vmcnt(0)) at the barrier
    int cur = 0;
    for (int t = 0; t < nk; ++t) {
        unsigned char* buf = lds + cur * 2 * kTileBytes;
        if (t + 1 < nk) {
            unsigned char* nxt = lds + (cur ^ 1) * 2 * kTileBytes;
            stage_tile(W, K, n0, (t + 1) * GBK, nxt, wave, lane);
            stage_tile(X, K, m0, (t + 1) * GBK, nxt + kTileBytes, wave, lane);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = read_frag(buf, wn * 64 + i * 16 + (lane & 15), ks * 4 + (lane >> 4));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                b[j] = read_frag(buf + kTileBytes, wm * 64 + j * 16 + (lane & 15), ks * 4 + (lane >> 4));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        cur ^= 1;
    }

    // Epilogue.  acc[i][j]: token m = m0 + wm*64 + j*16 + (lane&15); features
    // n = n0 + wn*64 + i*16 + (lane>>4)*4 + {0,1,2,3}.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + wn * 64 + i * 16 + (lane >> 4) * 4;
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n);
            f32x4 v = acc[i][j] + bv;
            if (EPI == 1) {
                const uint2 r = *reinterpret_cast<const uint2*>(residual + (int64_t)m * N + n);
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
}

// ------------------------------------------------------------------------------------------
// "mid" (round 4): gemm_bf16_kernel's 128 x 128 x 64 tile with a FOUR-stage LDS-DMA ring instead of two buffers behind a
// draining barrier.  Shapes too small for the persistent kernels (65 .. ~2 000 rows: the embed micro-batcher's coalesced
// queries, small uploads) are latency-bound, not bandwidth-bound: the two-buffer kernel takes ~1.2 us per 64-deep step (one
// operand tile in flight, its global -> LDS latency exposed every step), and the split-K pair that replaced it in round 2
// (more workgroups, fewer steps each) pays an fp32 partial tile per slice plus a second launch — 12.8 + 5.3 us for the QKV
// projection of 384 tokens.  With three tiles in flight a step is its 32 MFMAs per wave plus one LDS round trip (~0.4 us),
// the epilogue is fused, and K <= 1 024 needs no split: one launch of ~9 us.  Counted waits (vmcnt) and asm fragment reads as
// in p5 (hipcc would drain the DMA queue before every LDS read it can see).
constexpr int kMidStages = 4;
constexpr int kMidLdsBytes = kMidStages * 2 * kTileBytes;   // 128 KiB

typedef int mid_i32x4 __attribute__((ext_vector_type(4)));
#define MID_MFMA(acc, a, b) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b))

// The K loop is hand-scheduled like p4's (one wave per SIMD issues in order: whatever is not an MFMA goes, one instruction at
// a time, into the gaps between the MFMAs): a 64-deep step is two sub-steps of 16 MFMAs per wave; under sub-step u run the 8
// fragment reads of sub-step u + 1 and four of the wave's eight DMA pieces of a tile three to four steps ahead (buffer_load
// ... lds on whole-matrix descriptors: an SGPR offset per piece, one VGPR for the lane part); one s_barrier per step, between
// its sub-steps (tile t + 1 is published there and tile t's stage is free from there on).
// BM = token rows per tile (128 or 64): per-workgroup operand traffic (BM + 128) x K x 2 B moves through a latency-bound pipe
// (~4 tiles in flight per CU), so a mid-size batch wants MORE, smaller tiles than CUs it would otherwise leave idle.
template <int EPI, int BM>
__global__ __launch_bounds__(kGemmThreads, 1) void gemm_bf16_mid_kernel(const u16* __restrict__ X, const u16* __restrict__ W,
                                                                       const float* __restrict__ bias,
                                                                       const u16* __restrict__ residual,
                                                                       u16* __restrict__ Y, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [stage][W tile | X tile]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave >> 1, wm = wave & 1;
    const int nblk = gridDim.x;
    const int orig = blockIdx.x;
    const int q = nblk / 8, rr = nblk % 8, xcd = orig % 8;
    const int bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
    const int tiles_n = N / GBN;
    const int bn = bid % tiles_n, bm = bid / tiles_n;
    constexpr int NJ = BM / 32;              // 16-token MFMA tiles per wave (the wave's tokens: wm * BM/2 ..)
    constexpr int kXTile = BM * 128;         // bytes of an X tile
    constexpr int kStage = kTileBytes + kXTile;
    const int n0 = bn * GBN, m0 = bm * BM;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const int nk = K / GBK;   // >= 4 (launcher)

    // operand delivery: a tile = 16 W pieces + 16 X pieces of 8 rows x 128 B; this wave moves pieces wave + 4p, p = 0..3, of each
    auto make_desc = [](const void* base, unsigned bytes) {
        const uint64_t b = reinterpret_cast<uint64_t>(base);
        mid_i32x4 d;
        d[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)b);
        d[1] = __builtin_amdgcn_readfirstlane((int)((uint32_t)(b >> 32) & 0xffffu));
        d[2] = __builtin_amdgcn_readfirstlane((int)bytes);
        d[3] = 0x00020000;
        return d;
    };
    const mid_i32x4 wdesc = make_desc(W, (unsigned)N * (unsigned)K * 2u);
    const mid_i32x4 xdesc = make_desc(X, (unsigned)(gridDim.x / tiles_n * BM) * (unsigned)K * 2u);   // the row tiles launched are allocated
    const int dma_voff = ((lane >> 3) * K + (((lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7)) * 8)) * 2;
    const unsigned piece_step = (unsigned)K * 64u;   // 32 rows of K bf16
    const unsigned soW0 = __builtin_amdgcn_readfirstlane(((unsigned)(n0 + wave * 8) * (unsigned)K) * 2u);
    const unsigned soX0 = __builtin_amdgcn_readfirstlane(((unsigned)(m0 + wave * 8) * (unsigned)K) * 2u);
    const unsigned mbase = lds_base + wave * 1024;
    // piece `which` (0..3 W, 4..7 X; a 64-row X tile has two per wave: 4, 5) of tile t into stage t % 4
    auto dma = [&](int t, int which) {
        if (which >= 4 + NJ) return;
        const unsigned m0v = mbase + (t & (kMidStages - 1)) * kStage + (which < 4 ? 0 : kTileBytes) + (which & 3) * 4096;
        const unsigned so = (which < 4 ? soW0 : soX0) + (which & 3) * piece_step + (unsigned)t * 128u;
        asm volatile("s_mov_b32 m0, %0" ::"s"(m0v));
        if (which < 4) asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(dma_voff), "s"(wdesc), "s"(so) : "memory");
        else asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(dma_voff), "s"(xdesc), "s"(so) : "memory");
    };
    // the epilogue's operands leave FIRST: a workgroup has one tile, so loads issued after the K loop are a dependent L2 / HBM
    // round trip at the end of every launch (~1 us of 15).  They are older than every tile piece and loads complete in order,
    // so the counted vmcnt waits below mean what they meant.
    f32x4 ebias[4];
    uint2 eres[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + (lane >> 4) * 4;
        ebias[i] = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            eres[i][j] = make_uint2(0, 0);
            if (EPI == 1) {
                const int m = m0 + wm * (BM / 2) + j * 16 + (lane & 15);
                eres[i][j] = *reinterpret_cast<const uint2*>(residual + (int64_t)(m < M ? m : M - 1) * N + n);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // prologue: tiles 0, 1, 2 and the W pieces of tile 3
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) dma(t, w8);
#pragma unroll
    for (int w8 = 0; w8 < 4; ++w8) dma(3, w8);
    if (NJ == 4) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");     // tile 0 landed (tiles 1, 2 and the W half of 3 may fly)
    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // fragment addresses inside a stage: row r of a tile at r * 128, 16-B chunk c at c ^ ((r >> 1) & 7)
    const int fr = lane & 15, sw = (fr >> 1) & 7;
    unsigned offA[2], offB[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int ch = (ks * 4 + (lane >> 4)) ^ sw;
        offA[ks] = (wn * 64 + fr) * 128 + ch * 16;
        offB[ks] = kTileBytes + (wm * (BM / 2) + fr) * 128 + ch * 16;
    }
    f32x4 acc[4][4];   // [i][j]: j < NJ used
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 a0[4], b0[4], a1[4], b1[4];
    {
        const unsigned aa = lds_base + offA[0], bb = lds_base + offB[0];
        RASS_DS_READ_B128(a0[0], aa, 0); RASS_DS_READ_B128(a0[1], aa, 2048); RASS_DS_READ_B128(a0[2], aa, 4096); RASS_DS_READ_B128(a0[3], aa, 6144);
        RASS_DS_READ_B128(b0[0], bb, 0); RASS_DS_READ_B128(b0[1], bb, 2048);
        if (NJ == 4) { RASS_DS_READ_B128(b0[2], bb, 4096); RASS_DS_READ_B128(b0[3], bb, 6144); }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    for (int t = 0; t < nk; ++t) {
        const unsigned sb = lds_base + (t & (kMidStages - 1)) * kStage;
        const unsigned sn = lds_base + ((t + 1) & (kMidStages - 1)) * kStage;
        const bool x3 = t + 3 < nk, w4 = t + 4 < nk;
        // ---- sub-step 0: (t, 0) out of a0 / b0; reads (t, 1) into a1 / b1; the X pieces of tile t + 3
        {
            const unsigned aa = sb + offA[1], bb = sb + offB[1];
#define MID_SUB(AC, BC, AN, BN, DMA_T, DMA_BASE, DMA_ON)                                                                        \
    MID_MFMA(acc[0][0], AC[0], BC[0]); RASS_DS_READ_B128(AN[0], aa, 0);                                                          \
    MID_MFMA(acc[0][1], AC[0], BC[1]); RASS_DS_READ_B128(BN[0], bb, 0);                                                          \
    if (NJ == 4) { MID_MFMA(acc[0][2], AC[0], BC[2]); }                                                                          \
    if (DMA_ON) dma(DMA_T, DMA_BASE);                                                                                            \
    if (NJ == 4) { MID_MFMA(acc[0][3], AC[0], BC[3]); }                                                                          \
    RASS_DS_READ_B128(AN[1], aa, 2048);                                                                                          \
    MID_MFMA(acc[1][0], AC[1], BC[0]); RASS_DS_READ_B128(BN[1], bb, 2048);                                                       \
    MID_MFMA(acc[1][1], AC[1], BC[1]);                                                                                           \
    if (NJ == 4) { MID_MFMA(acc[1][2], AC[1], BC[2]); }                                                                          \
    if (DMA_ON) dma(DMA_T, DMA_BASE + 1);                                                                                        \
    if (NJ == 4) { MID_MFMA(acc[1][3], AC[1], BC[3]); }                                                                          \
    RASS_DS_READ_B128(AN[2], aa, 4096);                                                                                          \
    MID_MFMA(acc[2][0], AC[2], BC[0]); if (NJ == 4) { RASS_DS_READ_B128(BN[2], bb, 4096); }                                      \
    MID_MFMA(acc[2][1], AC[2], BC[1]);                                                                                           \
    if (NJ == 4) { MID_MFMA(acc[2][2], AC[2], BC[2]); }                                                                          \
    if (DMA_ON) dma(DMA_T, DMA_BASE + 2);                                                                                        \
    if (NJ == 4) { MID_MFMA(acc[2][3], AC[2], BC[3]); }                                                                          \
    RASS_DS_READ_B128(AN[3], aa, 6144);                                                                                          \
    MID_MFMA(acc[3][0], AC[3], BC[0]); if (NJ == 4) { RASS_DS_READ_B128(BN[3], bb, 6144); }                                      \
    MID_MFMA(acc[3][1], AC[3], BC[1]);                                                                                           \
    if (NJ == 4) { MID_MFMA(acc[3][2], AC[3], BC[2]); }                                                                          \
    if (DMA_ON) dma(DMA_T, DMA_BASE + 3);                                                                                        \
    if (NJ == 4) { MID_MFMA(acc[3][3], AC[3], BC[3]); }
            MID_SUB(a0, b0, a1, b1, t + 3, 4, x3)
        }
        // ---- the mid-step barrier: this wave's reads of tile t are done, its pieces of tile t + 1 have landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // (outstanding behind tile t + 1: tile t + 2 and both halves of tile t + 3 = 2 x (4 + NJ) instructions)
        if (x3 && NJ == 4) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (x3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- sub-step 1: (t, 1) out of a1 / b1; reads (t + 1, 0) into a0 / b0; the W pieces of tile t + 4
        {
            const unsigned aa = sn + offA[0], bb = sn + offB[0];
            MID_SUB(a1, b1, a0, b0, t + 4, 0, w4)
#undef MID_SUB
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }

    // Epilogue (as gemm_bf16_kernel).  acc[i][j]: token m = m0 + wm*64 + j*16 + (lane&15); features
    // n = n0 + wn*64 + i*16 + (lane>>4)*4 + {0,1,2,3}.
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int m = m0 + wm * (BM / 2) + j * 16 + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + wn * 64 + i * 16 + (lane >> 4) * 4;
            f32x4 v = acc[i][j] + ebias[i];
            if (EPI == 1) {
                const uint2 r = eres[i][j];
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
}

// ------------------------------------------------------------------------------------------
// Split-K form of the 128 x 128 kernel for FEW rows (a query or a handful of chunks: embed_query / ollama_embed_text,
// reference app/main.py:225-237, 266-274).  With M <= 256 the plain kernel launches N/128 x M/128 = 8-32 workgroups, each
// walking all of K behind one barrier per 64-deep step: FFN-down (K = 4096) took 60 us, attn-out 13 us, a one-query
// forward 2.9 ms of which 60 % were these two (profiles/r02_encoder_b1_s16_kernel_stats.csv).  Here the K range is cut
// into S slices so that >= ~128 workgroups stream the weights; every slice writes its fp32 partial tile (rows < M
// only) to a scratch [S][M_pad][N], and splitk_epilogue_kernel sums the slices IN FIXED ORDER (deterministic: no
// atomics), adds bias / residual, applies GELU and rounds to bf16 — the same arithmetic as the fused epilogue up to
// the order of the fp32 partial sums.
__global__ __launch_bounds__(kGemmThreads, 2) void gemm_bf16_splitk_kernel(const u16* __restrict__ X,
                                                                          const u16* __restrict__ W,
                                                                          float* __restrict__ partial, int M, int M_pad,
                                                                          int N, int K, int k_per_slice) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // [2 buf][W tile | X tile]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave >> 1, wm = wave & 1;
    const int tiles_n = N / GBN;
    const int bn = blockIdx.x % tiles_n, bm = blockIdx.x / tiles_n;
    const int slice = blockIdx.y;
    const int n0 = bn * GBN, m0 = bm * GBM, k_lo = slice * k_per_slice;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = k_per_slice / GBK;
    stage_tile(W, K, n0, k_lo, lds, wave, lane);
    stage_tile(X, K, m0, k_lo, lds + kTileBytes, wave, lane);
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nk; ++t) {
        unsigned char* buf = lds + cur * 2 * kTileBytes;
        if (t + 1 < nk) {
            unsigned char* nxt = lds + (cur ^ 1) * 2 * kTileBytes;
            stage_tile(W, K, n0, k_lo + (t + 1) * GBK, nxt, wave, lane);
            stage_tile(X, K, m0, k_lo + (t + 1) * GBK, nxt + kTileBytes, wave, lane);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = read_frag(buf, wn * 64 + i * 16 + (lane & 15), ks * 4 + (lane >> 4));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                b[j] = read_frag(buf + kTileBytes, wm * 64 + j * 16 + (lane & 15), ks * 4 + (lane >> 4));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        cur ^= 1;
    }
    // acc[i][j]: token m = m0 + wm*64 + j*16 + (lane&15); features n0 + wn*64 + i*16 + (lane>>4)*4 + {0..3}
    float* P = partial + (int64_t)slice * M_pad * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<f32x4*>(P + (int64_t)m * N + n0 + wn * 64 + i * 16 + (lane >> 4) * 4) = acc[i][j];
    }
}

// y[m][n..n+3] = epi(sum over the S slices (ascending) + bias [+ residual]); one thread per 4 features
template <int EPI>
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const float* __restrict__ partial, int S, int M, int M_pad,
                                                              int N, const float* __restrict__ bias,
                                                              const u16* __restrict__ residual, u16* __restrict__ Y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over M * N/4
    const int n4 = N / 4;
    if (idx >= (int64_t)M * n4) return;
    const int m = (int)(idx / n4), n = (int)(idx % n4) * 4;
    // the slices' loads go out together (S <= 16), the sum runs in ascending slice order
    f32x4 pv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s)
        pv[s] = s < S ? *reinterpret_cast<const f32x4*>(partial + ((int64_t)s * M_pad + m) * N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v = pv[0];
#pragma unroll
    for (int s = 1; s < 16; ++s)
        if (s < S) v += pv[s];
    v += *reinterpret_cast<const f32x4*>(bias + n);
    if (EPI == 1) {
        const uint2 r = *reinterpret_cast<const uint2*>(residual + (int64_t)m * N + n);
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

// ---- launchers (gemm_common.h) ----
template <int EPI>
static hipError_t launch_tile128_epi(const GemmOperands& a, int grid, hipStream_t stream) {
    constexpr int lds_bytes = 4 * kTileBytes;  // 64 KiB
    if (hipError_t e = allow_dynamic_lds<&gemm_bf16_kernel<EPI>>(lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((gemm_bf16_kernel<EPI>), dim3(grid), dim3(kGemmThreads), lds_bytes, stream, a.X, a.W, a.bias,
                       a.residual, a.Y, a.M, a.N, a.K);
    return hipGetLastError();
}

hipError_t launch_tile128(int epilogue, const GemmOperands& a, int grid, hipStream_t stream) {
    switch (epilogue) {
        case 0: return launch_tile128_epi<0>(a, grid, stream);
        case 1: return launch_tile128_epi<1>(a, grid, stream);
        case 2: return launch_tile128_epi<2>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

// the four-stage form of the tile, over the row tiles that hold real rows
template <int EPI, int BM>
static hipError_t launch_mid_epi(const GemmOperands& a, int grid, hipStream_t stream) {
    if (hipError_t e = allow_dynamic_lds<&gemm_bf16_mid_kernel<EPI, BM>>(kMidLdsBytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((gemm_bf16_mid_kernel<EPI, BM>), dim3(grid), dim3(kGemmThreads), kMidLdsBytes, stream, a.X, a.W, a.bias,
                       a.residual, a.Y, a.M, a.N, a.K);
    return hipGetLastError();
}

hipError_t launch_mid(int epilogue, int bm, const GemmOperands& a, int grid, hipStream_t stream) {
    switch (epilogue) {
        case 0: return bm == 64 ? launch_mid_epi<0, 64>(a, grid, stream) : launch_mid_epi<0, 128>(a, grid, stream);
        case 1: return bm == 64 ? launch_mid_epi<1, 64>(a, grid, stream) : launch_mid_epi<1, 128>(a, grid, stream);
        case 2: return bm == 64 ? launch_mid_epi<2, 64>(a, grid, stream) : launch_mid_epi<2, 128>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_splitk_pair(int epilogue, const GemmOperands& a, float* ws, int rows_pad, int S, hipStream_t stream) {
    constexpr int lds_bytes = 4 * kTileBytes;
    if (hipError_t e = allow_dynamic_lds<&gemm_bf16_splitk_kernel>(lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(gemm_bf16_splitk_kernel, dim3((a.N / GBN) * (rows_pad / GBM), S), dim3(kGemmThreads), lds_bytes, stream,
                       a.X, a.W, ws, a.M, rows_pad, a.N, a.K, a.K / S);
    if (epilogue < 0) return hipGetLastError();
    const int64_t work = (int64_t)a.M * (a.N / 4);
    const unsigned blocks = (unsigned)((work + 255) / 256);
    if (epilogue == 0)
        hipLaunchKernelGGL(splitk_epilogue_kernel<0>, dim3(blocks), dim3(256), 0, stream, ws, S, a.M, rows_pad, a.N, a.bias, a.residual, a.Y);
    else if (epilogue == 1)
        hipLaunchKernelGGL(splitk_epilogue_kernel<1>, dim3(blocks), dim3(256), 0, stream, ws, S, a.M, rows_pad, a.N, a.bias, a.residual, a.Y);
    else
        hipLaunchKernelGGL(splitk_epilogue_kernel<2>, dim3(blocks), dim3(256), 0, stream, ws, S, a.M, rows_pad, a.N, a.bias, a.residual, a.Y);
    return hipGetLastError();
}

}  // namespace rass
