// gemm_p5.hip — the persistent family of the encoder GEMM, first unit: the 8-wave "p5" kernel, the diagnostics of the
// microbenchmark builds (RASS_GEMM_CLOCKS / _PHASE_TIMERS / _STAMPS) and the two small kernels of the LayerNorm fold.
// (gemm_p4.hip holds the 4-wave form that is the default for big shapes.)
#include "gemm_common.h"

namespace rass {

// ------------------------------------------------------------------------------------------
// Large shapes (>= 192 tiles of 256 x 256): the persistent kernel below ("p5").  Its predecessors — the one-tile-per-block
// 3-slot ring kernel, its persistent form (pring), the two-slot 64-deep form (p64) and the 4-wave 128x128-per-wave kernel
// (w4l), each measured slower than p5 (profiles/r01_gemm_*.txt, profiles/r02_gemm_w4_experiments.txt) — were retired from
// the product library in round 3 and live on as an archive that still builds: scripts/microbench/gemm_retired_kernels.hip.
#ifdef RASS_GEMM_CLOCKS  // scripts/microbench builds only
__device__ unsigned long long g_gemm_clocks[4 * 16384];
__device__ unsigned long long g_gemm_core_cycles[64];
#ifdef RASS_GEMM_PHASE_TIMERS
__device__ unsigned long long g_gemm_phase_cycles[64 * 2 * 4];
#endif
#endif
#ifdef RASS_GEMM_STAMPS   // diagnostic builds only (scripts/probe_gemm_stamps.py): wall-clock (100 MHz) stamps of workgroups 0..7
__device__ unsigned long long g_p5_stamps[8 * 64 * 4];   // [block][tile][K loop start, K loop end, epilogue stores issued, tile end]
extern "C" int rassdiag_gemm_stamps(unsigned long long* out, int n) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned long long h[8 * 64 * 4];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_p5_stamps), sizeof(h)) != hipSuccess) return -2;
    for (int i = 0; i < n && i < 8 * 64 * 4; ++i) out[i] = h[i];
    return 0;
}
#define P5_STAMP(slot)                                                                                   \
    do {                                                                                                 \
        if (threadIdx.x == 0 && orig < 8 && tile_no < 64) g_p5_stamps[(orig * 64 + tile_no) * 4 + (slot)] = wall_clock64(); \
    } while (0)
#else
#define P5_STAMP(slot) do {} while (0)
#endif

// K-loop fragment read as opaque asm: hipcc's waitcnt pass orders every LDS access it can see after
// the LDS-DMA (global_load_lds) ops still in flight — in two of the three epilogue variants of the
// persistent kernel it put a vmcnt(0) in front of the fragment reads of EVERY K step (K loop 45 us
// instead of 28).  The DMA / read ordering is this kernel's own protocol (counted vmcnt + barrier).

// ------------------------------------------------------------------------------------------
// "p5": gemm_bf16_p64_kernel's whole-line operand stream with a ring of FIVE 32-KiB HALF-slots instead of two 64-KiB
// slots.  Half-load q = 2T + h holds rows 128h .. 128h+127 of both operand tiles of the 64-deep step T (W half at
// +0, X half at +16 KiB, rows of 128 B, swizzled as in p64) and lives in half-slot (q0 + q) % 5.  A wave's A
// fragments come from half wn of the step, its B fragments from half wm>>1.  While step T is multiplied (two
// half-slots), (T+1, 0) and (T+1, 1) and (T+2, 0) are in flight or landed: 1.5 steps ahead where two whole slots
// allowed one, and the DMA issues spread evenly — every load phase issues one half of a half-load (4 pieces per
// wave, as in the 32-deep kernel): step T issues (T+1, 1) in its first load phase and (T+2, 0) in its second, into
// the half-slots step T-1 was read from.  The stream runs on across tiles; only the next tile's third half-load
// waits for the epilogue to end (its 8 staging areas need three free half-slots).  Exactly 160 KiB of LDS.

// POL = cache policy of the three streams, one decimal digit each (x w y): operand loads 0 = default, 2 = nt (streaming), 1 = sc0,
// 3 = sc0 nt (the aux bits of global_load_lds); output stores 0 = default, 1 = nontemporal.  Measured in round 3
// (profiles/r03_gemm_power_limit.txt §6, RASS_P5_POLICY): nt on either operand stream costs 1-8 %, nontemporal OUTPUT stores
// win 3 % on the wide-output shapes (QKV 790 -> 763 us, FFN-up 1 115 -> 1 080; the 0.8-1.1 GB of output no longer push the
// operands out of L2) and nothing on the N = 1024 ones: POL = 1 is the default, RASS_P5_POLICY=0 the A/B.
template <int EPI, int POL = 1>
__global__ __launch_bounds__(kRingThreads, 2) void gemm_bf16_p5_kernel(const u16* __restrict__ X,
                                                                      const u16* __restrict__ W,
                                                                      const float* __restrict__ bias,
                                                                      const u16* __restrict__ residual,
                                                                      u16* __restrict__ Y, int M, int N, int K,
                                                                      int tiles_total, LnFold fold) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave >> 2, wm = wave & 3;
    const int G = gridDim.x, orig = blockIdx.x;
    const int pos = (G % 8 == 0) ? (orig % 8) * (G / 8) + orig / 8 : orig;
    int tile = pos;
    if (tile >= tiles_total) return;
    const int tiles_n = N / RBN;
    const int nk = K / 64;   // >= 2 (launcher)

    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    // fragment offsets inside a half-slot (rows of 128 B; chunk c of row r at c ^ ((r>>1)&7); sub-step s = chunks 4s..4s+3)
    unsigned offA[2], offB[2];
    {
        const int sw = ((lane & 15) >> 1) & 7;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int ch = (sub * 4 + (lane >> 4)) ^ sw;
            offA[sub] = (lane & 15) * 128 + ch * 16;
            offB[sub] = 16384 + ((wm & 1) * 64 + (lane & 15)) * 128 + ch * 16;
        }
    }
    const int hA = wn, hB = wm >> 1;  // which half of a step this wave's A / B fragments live in
    // DMA: a half-load is 16 W pieces + 16 X pieces of 8 rows x 128 B; this wave moves pieces wave and wave + 8 of each
    const u16* srcW[2][2];
    const u16* srcX[2][2];
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
    auto point_half = [&](int t, auto h_c) {   // sources of half h of tile t's step 0
        constexpr int h = decltype(h_c)::value;
        const int tn0 = (t % tiles_n) * RBN, tm0 = (t / tiles_n) * RBM;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = (wave + 8 * p) * 8 + (lane >> 3);   // row inside the half
            const int c_src = (lane & 7) ^ ((r >> 1) & 7);
            srcW[h][p] = W + (int64_t)(tn0 + 128 * h + r) * K + c_src * 8;
            srcX[h][p] = X + (int64_t)(tm0 + 128 * h + r) * K + c_src * 8;
        }
    };
    auto stage_half = [&](int hs, auto h_c) {   // hs: half-slot index 0..4
        constexpr int h = decltype(h_c)::value;
#ifdef RASS_GEMM_EXP_NO_DMA      // timing experiment: no operand delivery at all (stale LDS)
        (void)hs;
        return;
#endif
        unsigned char* base = lds + hs * kP5HalfBytes;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcX[h][p],
                                             (__attribute__((address_space(3))) void*)(base + 16384 + (wave + 8 * p) * 1024),
                                             16, 0, (POL / 100) % 10);
            srcX[h][p] += 64;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)srcW[h][p],
                                             (__attribute__((address_space(3))) void*)(base + (wave + 8 * p) * 1024), 16, 0,
                                             (POL / 10) % 10);
            srcW[h][p] += 64;
        }
    };
    auto mod5 = [](int v) { return v >= 5 ? v - 5 : v; };
    const bool grpB = wave >= 4;

    // half-slot of the current tile's half-load 0; every tile advances it by 2 * nk (mod 5)
    int q0 = 0;
    const int tile_adv = (2 * nk) % 5;
    point_half(tile, H0{});
    point_half(tile, H1{});
    stage_half(0, H0{});
    stage_half(1, H1{});
    stage_half(2, H0{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    int tile_no = 0;
    (void)tile_no;
    for (;;) {
        const int n0 = (tile % tiles_n) * RBN, m0 = (tile / tiles_n) * RBM;
        const int next = tile + G;
        const bool has_next = next < tiles_total;
        P5_STAMP(0);
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        if (grpB) __builtin_amdgcn_s_barrier();   // group B runs one phase behind group A
        int hs0 = q0;                              // half-slot of (t, 0)
        for (int t = 0; t < nk; ++t) {
            const int hs1 = mod5(hs0 + 1), hs2 = mod5(hs0 + 2), hs3 = mod5(hs0 + 3), hs4 = mod5(hs0 + 4);
            // half-loads this step issues: q = 2t+3 = (t+1, 1) into hs3 and q = 2t+4 = (t+2, 0) into hs4; beyond the
            // tile they are the next tile's (whose third half-load waits for the epilogue)
            const bool iss1 = (t + 1 < nk) || has_next;
            const bool iss2 = (t + 2 < nk) || (has_next && t + 2 == nk);
            const unsigned aslot = lds_base + (hA ? hs1 : hs0) * kP5HalfBytes;
            const unsigned bslot = lds_base + (hB ? hs1 : hs0) * kP5HalfBytes;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                // ---- load phase
                if (sub == 0 && iss1) {
                    if (t + 1 == nk) point_half(next, H1{});   // the half-load is the next tile's (0, 1)
                    stage_half(hs3, H1{});
                }
                if (sub == 1 && iss2) {
                    if (t + 2 == nk) point_half(next, H0{});   // the next tile's (0, 0)
                    stage_half(hs4, H0{});
                }
                bf16x8 a[8], b[4];
#ifdef RASS_GEMM_EXP_NO_MFMA    // timing experiment: the operand stream alone (DMA + waits + barriers)
                for (int i = 0; i < 8; ++i) a[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                for (int j = 0; j < 4; ++j) b[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                (void)aslot; (void)bslot;
#else
                {
                    const unsigned ab = aslot + offA[sub];
                    const unsigned bb = bslot + offB[sub];
                    RASS_DS_READ_B128(b[0], bb, 0);
                    RASS_DS_READ_B128(b[1], bb, 2048);
                    RASS_DS_READ_B128(b[2], bb, 4096);
                    RASS_DS_READ_B128(b[3], bb, 6144);
                    RASS_DS_READ_B128(a[0], ab, 0);
                    RASS_DS_READ_B128(a[1], ab, 2048);
                    RASS_DS_READ_B128(a[2], ab, 4096);
                    RASS_DS_READ_B128(a[3], ab, 6144);
                    RASS_DS_READ_B128(a[4], ab, 8192);
                    RASS_DS_READ_B128(a[5], ab, 10240);
                    RASS_DS_READ_B128(a[6], ab, 12288);
                    RASS_DS_READ_B128(a[7], ab, 14336);
                }
#endif
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                // before the barrier that ends the step: this wave's pieces of (t+1, 1) have landed; (t+2, 0)'s four may fly
                if (sub == 1 && grpB) {
                    if (iss2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                // ---- compute phase
                __builtin_amdgcn_s_setprio(1);
#ifndef RASS_GEMM_EXP_NO_MFMA
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
#endif
                __builtin_amdgcn_s_setprio(0);
                if (sub == 1 && !grpB) {
                    if (iss2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
            hs0 = hs2;
        }
        if (!grpB) __builtin_amdgcn_s_barrier();  // groups re-aligned: every ring read of this tile is done
        P5_STAMP(1);
        // the next tile's half-loads 0 and 1 are landing in hs0, hs0+1 (= its q0); staging: three free half-slots
        q0 = mod5(q0 + tile_adv);
        float* const stg = reinterpret_cast<float*>(lds + mod5(q0 + 2 + wave / 3) * kP5HalfBytes + (wave % 3) * 8704);

        // ---- epilogue (see gemm_bf16_ring_kernel): LDS transpose per wave, coalesced 16-B stores
        {
            constexpr int kPitchF = 68;
            const int tl = lane >> 3, nq = lane & 7;
            // Bias through opaque asm loads, retired by the explicit vmcnt(0) below: a load hipcc can
            // see stays "possibly pending" on its destination registers across the tile loop, and
            // when the K loop's fragment reads get the same registers the waitcnt pass protects them
            // with a vmcnt(0) in EVERY K step (seen in two of the three epilogue variants).
            f32x4 bv[2][2];
            // Output / residual rows go through BUFFER ops on per-tile descriptors (base = the tile's first row, size = its
            // rows below M): rows past M are dropped / read as zero by the bounds check instead of by a branch.  With
            // `if (m < M)` around every global load and store hipcc's waitcnt pass lost count at the block boundaries and put
            // an s_waitcnt vmcnt(0) in front of EVERY store of the residual epilogues: 16 store round trips per tile,
            // 9-10 us against 3.4 for the bias-only epilogue (scripts/probe_gemm_stamps.py, ISA).
            typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
            const int rows_here = M - m0 < RBM ? (M - m0 > 0 ? M - m0 : 0) : RBM;
            const unsigned tile_bytes = __builtin_amdgcn_readfirstlane((unsigned)rows_here * (unsigned)N * 2u);
            auto tile_desc = [&](const u16* base) {
                const uint64_t bu = reinterpret_cast<uint64_t>(base + (int64_t)m0 * N);
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)bu), hi = __builtin_amdgcn_readfirstlane((uint32_t)(bu >> 32));
                return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<u16*>(((uint64_t)hi << 32) | lo), 0, (int)tile_bytes, 0x00020000);
            };
            const __amdgpu_buffer_rsrc_t ydesc = tile_desc(Y);
            const __amdgpu_buffer_rsrc_t rdesc = tile_desc((EPI == 1 || EPI == 3) ? residual : Y);
            // LN fold: per-column vectors of the lane's 2 x 8 columns (EPI 3: gamma / beta of the residual's LayerNorm;
            // EPI 4 / 5: colsum(W')), loaded like the bias
            // (the LN fold's per-column vectors — EPI 3: gamma / beta, EPI 4 / 5: colsum(W') — are loaded per 64-column chunk
            // inside the loop: held across the whole epilogue like the bias they spilled)
#pragma unroll
            for (int ic = 0; ic < 2; ++ic) {
                const float* bp = bias + n0 + wn * 128 + ic * 64 + nq * 8;
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bv[ic][0]) : "v"(bp));
                asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(bv[ic][1]) : "v"(bp));
            }
            // LN fold: this wave's per-token (mean, rstd) pairs (its 64 tokens) and per-column vectors (its 128 columns: EPI 3
            // gamma / beta, EPI 4 / 5 colsum(W')) are fetched ONCE per tile — one 8-byte piece per lane and array, opaque
            // loads like the bias, retired by the same vmcnt(0) — and parked in the 2 KiB of LDS behind the wave's staging
            // area: as loads inside the (jc, ic) loop they put a memory round trip into each of the tile's four iterations
            // (QKV + 54 us, FFN-up + 89 us per call).
            float* const aux = reinterpret_cast<float*>(lds + mod5(q0 + 2 + wave / 3) * kP5HalfBytes + 26112 + (wave % 3) * 2048);
            float2 aux_mr = float2{0.f, 1.f}, aux_c0 = float2{0.f, 0.f}, aux_c1 = float2{0.f, 0.f};
            if constexpr (EPI >= 3) {
                const int mt = m0 + wm * 64 + lane;
                const float* mp = fold.mr + 2 * (int64_t)(mt < M ? mt : 0);
                asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(aux_mr) : "v"(mp));
                const float* c0 = (EPI == 3 ? fold.gamma : fold.colsum) + n0 + wn * 128 + 2 * lane;
                asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(aux_c0) : "v"(c0));
                if constexpr (EPI == 3) {
                    const float* c1 = fold.beta + n0 + wn * 128 + 2 * lane;
                    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(aux_c1) : "v"(c1));
                }
            }
            uint4 resbuf[2][4];   // residual rows of the current and of the next (jc, ic) iteration
#pragma unroll
            for (int jc = 0; jc < 64 / kPStageTokens; ++jc) {
                float st_s[kPStageTokens / 8], st_q[kPStageTokens / 8];   // EPI 3: this wave's 128-column partial sums per token
#pragma unroll
                for (int pass = 0; pass < kPStageTokens / 8; ++pass) st_s[pass] = st_q[pass] = 0.f;
#pragma unroll
                for (int ic = 0; ic < 2; ++ic) {
                    const int nbase = n0 + wn * 128 + ic * 64 + nq * 8;
                    float mu[kPStageTokens / 8], rs[kPStageTokens / 8];   // EPI >= 3: (mean, rstd) of the token's row
                    f32x4 cv[2];          // EPI 4 / 5: colsum(W') of this chunk's 8 columns
                    f32x4 gv[2], ev[2];   // EPI 3: gamma / beta of the residual's LayerNorm for this chunk's 8 columns
                    // Residual rows (EPI 1 / 3): iteration it's 4 x 16 B per lane are loaded one iteration AHEAD, right after
                    // iteration it - 1's transposes (their accumulators are dead by then) and BEFORE its stores: a wait for
                    // them then leaves those stores in flight (vmcnt counts both, in order).  Loaded at the top of their
                    // own iteration they queued behind the previous iteration's stores and every iteration paid a store
                    // round trip: 9-10 us per tile against 3.4 for the bias-only epilogue (scripts/probe_gemm_stamps.py).
                    const int it = jc * 2 + ic;
                    auto load_res = [&](int jc2, int ic2, uint4 (&dst)[4]) {
                        const int nb2 = n0 + wn * 128 + ic2 * 64 + nq * 8;   // (column inside the row; the descriptor starts at row m0)
#pragma unroll
                        for (int pass = 0; pass < kPStageTokens / 8; ++pass) {
                            const int row = wm * 64 + jc2 * kPStageTokens + pass * 8 + tl;
                            // read once, like the output: nontemporal keeps it out of the operands' way (POL; always for EPI 3)
                            const u32x4_t rv = __builtin_amdgcn_raw_buffer_load_b128(rdesc, (row * N + nb2) * 2, 0,
                                                                                     (POL % 10 == 1 || EPI == 3) ? 2 : 0);
                            dst[pass] = uint4{rv[0], rv[1], rv[2], rv[3]};
                        }
                    };
                    uint4 (&res)[4] = resbuf[it & 1];
                    if ((EPI == 1 || EPI == 3) && it == 0) load_res(0, 0, resbuf[0]);
#ifndef RASS_GEMM_EXP_NO_TRANSPOSE
#pragma unroll
                    for (int jj = 0; jj < kPStageTokens / 16; ++jj)
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii)
                            *reinterpret_cast<f32x4*>(stg + (jj * 16 + (lane & 15)) * kPitchF + ii * 16 + (lane >> 4) * 4) =
                                acc[4 * ic + ii][(kPStageTokens / 16) * jc + jj];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                    if ((EPI == 1 || EPI == 3) && it < 3) load_res((it + 1) >> 1, (it + 1) & 1, resbuf[(it + 1) & 1]);
                    if (jc == 0 && ic == 0) {
                        // Explicit: this wave's prefetch DMAs (and the bias / first residual reads issued
                        // after them) are complete before anything below consumes them and before the
                        // publishing barrier after the epilogue.  No store is outstanding yet.
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        if constexpr (EPI >= 3) {   // park the tile's LN-fold scalars in LDS (wave-private: no barrier)
                            *reinterpret_cast<float2*>(aux + 2 * lane) = aux_c0;
                            if constexpr (EPI == 3) *reinterpret_cast<float2*>(aux + 128 + 2 * lane) = aux_c1;
                            *reinterpret_cast<float2*>(aux + 256 + 2 * lane) = aux_mr;
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        }
                    }
                    if constexpr (EPI >= 3) {
#pragma unroll
                        for (int pass = 0; pass < kPStageTokens / 8; ++pass) {
                            const float2 v = *reinterpret_cast<const float2*>(aux + 256 + 2 * (jc * kPStageTokens + pass * 8 + tl));
                            mu[pass] = v.x;
                            rs[pass] = v.y;
                        }
                        if constexpr (EPI == 3) {
                            gv[0] = *reinterpret_cast<const f32x4*>(aux + ic * 64 + nq * 8);
                            gv[1] = *reinterpret_cast<const f32x4*>(aux + ic * 64 + nq * 8 + 4);
                            ev[0] = *reinterpret_cast<const f32x4*>(aux + 128 + ic * 64 + nq * 8);
                            ev[1] = *reinterpret_cast<const f32x4*>(aux + 128 + ic * 64 + nq * 8 + 4);
                        } else {
                            cv[0] = *reinterpret_cast<const f32x4*>(aux + ic * 64 + nq * 8);
                            cv[1] = *reinterpret_cast<const f32x4*>(aux + ic * 64 + nq * 8 + 4);
                        }
                    }
#pragma unroll
                    for (int pass = 0; pass < kPStageTokens / 8; ++pass) {
                        const int tok = pass * 8 + tl;
#ifdef RASS_GEMM_EXP_NO_TRANSPOSE   // timing experiment: the epilogue without its LDS round trip (values from the wrong lanes)
                        f32x4 v0 = acc[4 * ic + (pass & 3)][2 * jc];
                        f32x4 v1 = acc[4 * ic + (pass & 3)][2 * jc + 1];
#else
                        f32x4 v0 = *reinterpret_cast<const f32x4*>(stg + tok * kPitchF + nq * 8);
                        f32x4 v1 = *reinterpret_cast<const f32x4*>(stg + tok * kPitchF + nq * 8 + 4);
#endif
                        if constexpr (EPI >= 4) {   // LN folded into this GEMM: rstd * (x W'^T - mu * colsum(W')) + bias'
                            // two fused ops per element: (b * colsum + bias') first, then acc * rstd + that
                            const float a = rs[pass], b = -mu[pass] * rs[pass];
                            v0.x = fmaf(v0.x, a, fmaf(b, cv[0].x, bv[ic][0].x)); v0.y = fmaf(v0.y, a, fmaf(b, cv[0].y, bv[ic][0].y));
                            v0.z = fmaf(v0.z, a, fmaf(b, cv[0].z, bv[ic][0].z)); v0.w = fmaf(v0.w, a, fmaf(b, cv[0].w, bv[ic][0].w));
                            v1.x = fmaf(v1.x, a, fmaf(b, cv[1].x, bv[ic][1].x)); v1.y = fmaf(v1.y, a, fmaf(b, cv[1].y, bv[ic][1].y));
                            v1.z = fmaf(v1.z, a, fmaf(b, cv[1].z, bv[ic][1].z)); v1.w = fmaf(v1.w, a, fmaf(b, cv[1].w, bv[ic][1].w));
                        } else {
                            v0 += bv[ic][0];
                            v1 += bv[ic][1];
                        }
                        if constexpr (EPI == 3) {   // residual = LayerNorm_prev(raw row), rebuilt from (raw, mu, rstd, gamma, beta)
                            const uint4 r = res[pass];
                            const float a = rs[pass], b = -mu[pass] * rs[pass];
                            v0.x += fmaf(fmaf(bf16_to_f32((u16)(r.x & 0xffff)), a, b), gv[0].x, ev[0].x);
                            v0.y += fmaf(fmaf(bf16_to_f32((u16)(r.x >> 16)), a, b), gv[0].y, ev[0].y);
                            v0.z += fmaf(fmaf(bf16_to_f32((u16)(r.y & 0xffff)), a, b), gv[0].z, ev[0].z);
                            v0.w += fmaf(fmaf(bf16_to_f32((u16)(r.y >> 16)), a, b), gv[0].w, ev[0].w);
                            v1.x += fmaf(fmaf(bf16_to_f32((u16)(r.z & 0xffff)), a, b), gv[1].x, ev[1].x);
                            v1.y += fmaf(fmaf(bf16_to_f32((u16)(r.z >> 16)), a, b), gv[1].y, ev[1].y);
                            v1.z += fmaf(fmaf(bf16_to_f32((u16)(r.w & 0xffff)), a, b), gv[1].z, ev[1].z);
                            v1.w += fmaf(fmaf(bf16_to_f32((u16)(r.w >> 16)), a, b), gv[1].w, ev[1].w);
                        }
                        if (EPI == 1) {
                            const uint4 r = res[pass];
                            v0.x += bf16_to_f32((u16)(r.x & 0xffff));
                            v0.y += bf16_to_f32((u16)(r.x >> 16));
                            v0.z += bf16_to_f32((u16)(r.y & 0xffff));
                            v0.w += bf16_to_f32((u16)(r.y >> 16));
                            v1.x += bf16_to_f32((u16)(r.z & 0xffff));
                            v1.y += bf16_to_f32((u16)(r.z >> 16));
                            v1.z += bf16_to_f32((u16)(r.w & 0xffff));
                            v1.w += bf16_to_f32((u16)(r.w >> 16));
                        }
                        if (EPI == 2 || EPI == 5) {
                            v0.x = gelu_erf(v0.x); v0.y = gelu_erf(v0.y); v0.z = gelu_erf(v0.z); v0.w = gelu_erf(v0.w);
                            v1.x = gelu_erf(v1.x); v1.y = gelu_erf(v1.y); v1.z = gelu_erf(v1.z); v1.w = gelu_erf(v1.w);
                        }
                        if constexpr (EPI == 3) {   // the row statistics of what is STORED (the bf16 values the consumers read)
                            const float q0 = bf16_to_f32(f32_to_bf16(v0.x)), q1 = bf16_to_f32(f32_to_bf16(v0.y)),
                                        q2 = bf16_to_f32(f32_to_bf16(v0.z)), q3 = bf16_to_f32(f32_to_bf16(v0.w)),
                                        q4 = bf16_to_f32(f32_to_bf16(v1.x)), q5 = bf16_to_f32(f32_to_bf16(v1.y)),
                                        q6 = bf16_to_f32(f32_to_bf16(v1.z)), q7 = bf16_to_f32(f32_to_bf16(v1.w));
                            const float s = ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7));
                            float q = q0 * q0;
                            q = fmaf(q1, q1, q); q = fmaf(q2, q2, q); q = fmaf(q3, q3, q);
                            q = fmaf(q4, q4, q); q = fmaf(q5, q5, q); q = fmaf(q6, q6, q); q = fmaf(q7, q7, q);
                            st_s[pass] += sum8_dpp(s);
                            st_q[pass] += sum8_dpp(q);
                        }
#ifdef RASS_GEMM_EXP_NO_STORE   // timing experiment: everything but the output stores (one store per 2^20 keeps the math alive)
                        if (v0.x == 12345.678f)
#endif
                        {
                            uint4 o;
                            o.x = (unsigned)f32_to_bf16(v0.x) | ((unsigned)f32_to_bf16(v0.y) << 16);
                            o.y = (unsigned)f32_to_bf16(v0.z) | ((unsigned)f32_to_bf16(v0.w) << 16);
                            o.z = (unsigned)f32_to_bf16(v1.x) | ((unsigned)f32_to_bf16(v1.y) << 16);
                            o.w = (unsigned)f32_to_bf16(v1.z) | ((unsigned)f32_to_bf16(v1.w) << 16);
                            const int voff = ((wm * 64 + jc * kPStageTokens + tok) * N + nbase) * 2;   // bytes from the tile's first row
                            __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{o.x, o.y, o.z, o.w}, ydesc, voff, 0, POL % 10 == 1 ? 2 : 0);
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                if constexpr (EPI == 3) {   // one (sum, sum of squares) pair per token and 128-column chunk of this wave
                    if (nq == 0) {
#pragma unroll
                        for (int pass = 0; pass < kPStageTokens / 8; ++pass) {
                            const int m = m0 + wm * 64 + jc * kPStageTokens + pass * 8 + tl;
                            if (m < M)
                                *reinterpret_cast<float2*>(fold.stats + ((int64_t)m * (N / 128) + (n0 / 128 + wn)) * 2) =
                                    float2{st_s[pass], st_q[pass]};
                        }
                    }
                }
            }
        }
        P5_STAMP(2);
#ifdef RASS_GEMM_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // diagnostic: when have this wave's stores left?
        P5_STAMP(3);
#endif
        if (!has_next) break;
        // every wave is done with its staging area: the next tile's third half-load may overwrite it
        __builtin_amdgcn_s_barrier();
        stage_half(mod5(q0 + 2), H0{});
        tile = next;
        ++tile_no;
    }
}

template <int EPI, int POL>
static hipError_t launch_p5_pol(const GemmOperands& a, int tiles_total, int grid, hipStream_t stream, const LnFold& fold) {
    if (hipError_t e = allow_dynamic_lds<&gemm_bf16_p5_kernel<EPI, POL>>(kP5LdsBytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((gemm_bf16_p5_kernel<EPI, POL>), dim3(grid), dim3(kRingThreads), kP5LdsBytes, stream, a.X, a.W, a.bias,
                       a.residual, a.Y, a.M, a.N, a.K, tiles_total, fold);
    return hipGetLastError();
}

template <int EPI>
static hipError_t launch_p5_epi(int policy, const GemmOperands& a, int tiles, int grid, hipStream_t stream, const LnFold& fold) {
    return policy == 0 ? launch_p5_pol<EPI, 0>(a, tiles, grid, stream, fold) : launch_p5_pol<EPI, 1>(a, tiles, grid, stream, fold);
}

hipError_t launch_p5(int epilogue, int policy, const GemmOperands& a, int tiles, int grid, hipStream_t stream, const LnFold& fold) {
    switch (epilogue) {
        case 0: return launch_p5_epi<0>(policy, a, tiles, grid, stream, fold);
        case 1: return launch_p5_epi<1>(policy, a, tiles, grid, stream, fold);
        case 2: return launch_p5_epi<2>(policy, a, tiles, grid, stream, fold);
        case 3: return launch_p5_epi<3>(policy, a, tiles, grid, stream, fold);
        case 4: return launch_p5_epi<4>(policy, a, tiles, grid, stream, fold);
        case 5: return launch_p5_epi<5>(policy, a, tiles, grid, stream, fold);
        default: return hipErrorInvalidValue;
    }
}

// (mean, rstd) per row from the residual GEMM's per-chunk partial sums, in fixed order
__global__ __launch_bounds__(256) void ln_stats_finalize_kernel(const float* __restrict__ stats, int chunks, int n, float eps,
                                                                float* __restrict__ mr, int rows) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= rows) return;
    const float2* p = reinterpret_cast<const float2*>(stats) + (int64_t)m * chunks;
    float s = 0.f, q = 0.f;
    for (int c = 0; c < chunks; ++c) {
        const float2 v = p[c];
        s += v.x;
        q += v.y;
    }
    const float mean = s / (float)n;
    const float var = fmaxf(q / (float)n - mean * mean, 0.f);
    *reinterpret_cast<float2*>(mr + 2 * (int64_t)m) = float2{mean, rsqrtf(var + eps)};
}

hipError_t launch_ln_stats_finalize(const float* stats, int rows, int n, float eps, float* mr, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (n % 128 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, stats, n / 128, n, eps, mr, rows);
    return hipGetLastError();
}

// W'[n][k] = bf16(W[n][k] * gamma[k]);  colsum[n] = sum_k W'[n][k];  bias2[n] = bias[n] + sum_k beta[k] * W[n][k].  One wave per row.
__global__ __launch_bounds__(256) void fold_gamma_kernel(const u16* __restrict__ W, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ bias,
                                                         int N, int K, u16* __restrict__ W2, float* __restrict__ colsum,
                                                         float* __restrict__ bias2) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float cs = 0.f, bs = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = bf16_to_f32(W[(int64_t)n * K + k]);
        const u16 w2 = f32_to_bf16(w * gamma[k]);
        W2[(int64_t)n * K + k] = w2;
        cs += bf16_to_f32(w2);
        bs = fmaf(beta[k], w, bs);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cs += __shfl_xor(cs, off);
        bs += __shfl_xor(bs, off);
    }
    if (lane == 0) {
        colsum[n] = cs;
        bias2[n] = bias[n] + bs;
    }
}

hipError_t launch_fold_gamma(const void* W, const float* gamma, const float* beta, const float* bias, int N, int K, void* W2,
                             float* colsum, float* bias2, hipStream_t stream) {
    hipLaunchKernelGGL(fold_gamma_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, static_cast<const u16*>(W), gamma, beta, bias,
                       N, K, static_cast<u16*>(W2), colsum, bias2);
    return hipGetLastError();
}

}  // namespace rass
