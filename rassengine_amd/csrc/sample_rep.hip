// sample_rep.hip — the sample floor of a fused fp32 batch (api_search.hip, scan_launch_batch) without fp32 MFMAs.
//
// The floor of a query is the k-th largest of 32 scores, each the EXACT flat-kernel score of a different eligible row of
// the slab: k rows reach it, so the final k-th best does too (kernels.h, ScanArgs::sample_best).  Which 32 rows is free.
// The fp32 sample pass took each block's true maximum and paid 34 GFLOP of fp32 MFMAs per 1 024 queries for it; here bf16
// MFMAs CHOOSE one representative row per (query, block) and the fp32 fmaf chain scores only those 32 rows per query:
//
//   1. sample_queries_frag_kernel: the normalised queries -> bf16, in B-fragment order of v_mfma_f32_16x16x32_bf16.
//   2. sample_rep_bf16_kernel: one workgroup per 64 sample rows.  The rows go to LDS as bf16 A fragments once, then every
//      wave streams 16-query tiles past them (4 x KS MFMAs per tile) and keeps, per query, the eligible row with the
//      largest bf16 score (lowest row on ties): rep_part[q][workgroup] = (score, row).
//   3. sample_rescore_f32_kernel: a block's representative = the best of its grid / 32 workgroups' (score, row) pairs; its
//      score is recomputed as the flat kernel computes it (exact_score.h) and written to
//      sample_best[group][32][kMaxSampleGroups], entries 0..31, -inf where a block has no representative or the score is
//      not finite.  Block by block, so that the gathered rows come out of L2.
//
// A representative that is not its block's true maximum only lowers the floor; no bf16 score reaches it, so no error bound
// is needed.  The K slots of a bf16 MFMA may hold any columns as long as A and B agree: a lane's fp32 chunks 2 ks and
// 2 ks + 1 of the tile16 slab ([g][row][4] floats, columns 16 j + 4 g + i) make A's 8 slots of k-group g at k-step ks, and
// the query fragment carries the same 8 columns.
//
// Also here: step_floors_kernel, which turns a query's sample_best entries (this stage's, or a sample pass's) into its ONE
// floor, once per batch call, for the step kernel (scan_step.hip).

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"
#include "exact_score.h"

namespace rass {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kRepThreads = 512;   // 8 waves: a tile of 16 queries each, round-robin
constexpr int kRepRows = 64;       // sample rows of a workgroup: 4 blocks of 16

__device__ __forceinline__ bf16x8 pack_bf16(const f32x4 a, const f32x4 b) {
    const bf16x4 lo = __builtin_convertvector(a, bf16x4), hi = __builtin_convertvector(b, bf16x4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// (score, row) order of the representatives: larger score first, lower row on ties; a NaN never wins.
__device__ __forceinline__ void take_better(float& s, int& r, float os, int orow) {
    const bool take = (os > s) | ((os == s) & (orow < r));
    s = take ? os : s;
    r = take ? orow : r;
}

// q_padded [nq][stride] fp32 -> q_frag [nq / 16][KS][64 lanes][8] bf16: lane (n = lane & 15, g = lane >> 4) of k-step ks holds
// columns 32 ks + 4 g .. + 3 and 32 ks + 16 + 4 g .. + 3 of query 16 tile + n.
__global__ __launch_bounds__(256) void sample_queries_frag_kernel(const float* __restrict__ q_padded, int64_t stride,
                                                                  bf16x8* __restrict__ q_frag, int n_frag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frag) return;
    const int ks_per_tile = (int)(stride >> 5);
    const int lane = i & 63, ks = (i >> 6) % ks_per_tile, tile = (i >> 6) / ks_per_tile;
    const float* src = q_padded + (int64_t)(tile * 16 + (lane & 15)) * stride + 32 * ks + 4 * (lane >> 4);
    q_frag[i] = pack_bf16(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 16));
}

// CH = stride / 128; KS = 4 CH k-steps of 32 columns.  grid = sample rows / 64; all of those rows exist (the caller's rule).
template <int CH>
__global__ __launch_bounds__(kRepThreads, 2) void sample_rep_bf16_kernel(const float* __restrict__ slab,
                                                                         const int32_t* __restrict__ row_tag,
                                                                         const bf16x8* __restrict__ q_frag,
                                                                         const int32_t* __restrict__ q_filter, int n_tiles,
                                                                         int2* __restrict__ rep_part) {
    constexpr int KS = 4 * CH;
    constexpr int64_t stride = 128 * CH;
    __shared__ bf16x8 rows[KS * 4 * 64];   // [k-step ks][block rb][lane]: 16 KiB x CH
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4;
    const int row0 = blockIdx.x * kRepRows;

    // the rows: each wave converts 2 CH of the 16 CH (block, k-step) fragments, in two rounds (64 registers at CH = 8)
    {
        const float* base = slab + (int64_t)row0 * stride + lane * 4;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[CH][2];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int item = wid + 8 * (half * CH + u), rb = item / KS, ks = item % KS;
                const float* c = base + (int64_t)rb * 16 * stride + ks * 512;
                v[u][0] = *reinterpret_cast<const f32x4*>(c);
                v[u][1] = *reinterpret_cast<const f32x4*>(c + 256);
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int item = wid + 8 * (half * CH + u), rb = item / KS, ks = item % KS;
                rows[(ks * 4 + rb) * 64 + lane] = pack_bf16(v[u][0], v[u][1]);
            }
        }
    }
    // the tags of the 16 rows this lane's accumulators hold: row0 + 16 rb + 4 g + r.  Tags and filters come through buffer
    // descriptors with zero records where the array is absent (0 comes back, no traffic): straight-line code, so that the
    // s_waitcnt counts of the tile loop stay exact.
    const __amdgpu_buffer_rsrc_t trs = make_rsrc(reinterpret_cast<uint64_t>(row_tag ? row_tag + row0 : nullptr), row_tag ? kRepRows * 4u : 0u);
    const __amdgpu_buffer_rsrc_t frs = make_rsrc(reinterpret_cast<uint64_t>(q_filter), q_filter ? (unsigned)n_tiles * 64u : 0u);
    int tag[4][4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) tag[rb][r] = (int)__builtin_amdgcn_raw_buffer_load_b32(trs, (16 * rb + 4 * g + r) * 4, 0, 0);
    __syncthreads();
    if (wid >= n_tiles) return;   // (behind the only barrier)

    // This wave's first query tile.  A sched_barrier per load keeps these the last loads ahead of the loop, in k order, as
    // the loop's refills are (hipcc reorders them otherwise): its s_waitcnt counts, merged over the entry and the back edge,
    // then wait for one fragment at a time instead of for nearly all of them at every tile's first MFMA.
    bf16x8 qf[KS];
    int t = wid;
    {
        const bf16x8* qp = q_frag + (int64_t)t * KS * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            __builtin_amdgcn_sched_barrier(0);
            qf[ks] = qp[ks * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    do {
        // the row fragments are the same for every tile: without this hipcc keeps all 16 CH of them in registers and spills
        asm volatile("" ::: "memory");
        const int q = t * 16 + (lane & 15);
        const int qraw = (int)__builtin_amdgcn_raw_buffer_load_b32(frs, q * 4, 0, 0);   // used behind the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        // the next tile's fragments replace this one's as they are consumed (the last tile re-reads itself: in bounds)
        const bf16x8* qn = q_frag + (int64_t)min(t + 8, n_tiles - 1) * KS * 64 + lane;
        f32x4 acc[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the A fragments come from LDS two k-steps ahead of their MFMAs (a ring of three): read at their first use, every
        // MFMA waited for a full LDS round trip
        bf16x8 a[3][4];
#pragma unroll
        for (int pre = 0; pre < 2; ++pre)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) a[pre][rb] = rows[(pre * 4 + rb) * 64 + lane];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 2 < KS) {
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) a[(ks + 2) % 3][rb] = rows[((ks + 2) * 4 + rb) * 64 + lane];
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks % 3][rb], qf[ks], acc[rb], 0, 0, 0);
            qf[ks] = qn[ks * 64];
            __builtin_amdgcn_sched_barrier(0);   // reads, MFMAs and the refill stay in this order: no second set of registers
        }
        // accumulator register r of block rb: (row 16 rb + 4 g + r, query lane & 15); rows ascend, so > keeps the lowest
        const int qfil = q_filter ? qraw : -1;
        float bs = -INFINITY;
        int br = INT_MAX;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tg = tag[rb][r];
                const bool ok = (tg != -1) & ((qfil < 0) | (qfil == tg));
                const float s = acc[rb][r];
                const bool take = ok & (s > bs);
                bs = take ? s : bs;
                br = take ? row0 + 16 * rb + 4 * g + r : br;
            }
        // over the 4 lane groups of a query
        take_better(bs, br, __int_as_float(xor_lane<16>(__float_as_int(bs), lane)), xor_lane<16>(br, lane));
        take_better(bs, br, __int_as_float(xor_lane<32>(__float_as_int(bs), lane)), xor_lane<32>(br, lane));
        if (lane < 16) rep_part[(int64_t)q * gridDim.x + blockIdx.x] = make_int2(__float_as_int(bs), br);
        t += 8;
    } while (t < n_tiles);
}

// 8 x 32 workgroups; thread (c = tid >> 3, w = tid & 7): query c of a launch group, then K slice w of its representative.
// Workgroup i takes the blocks x, x + 8, x + 16, x + 24 one after the other (x = i % 8, the XCD it lands on) and, of each, the
// launch groups j, j + 32, ... (j = i / 8): the 32 workgroups of an XCD gather from ONE block of 2 grid rows at a time, which its
// L2 holds.  A row of the tile16 slab is 16 B of every 256: gathered query by query — a workgroup per query, its 32 rows
// anywhere in the sample — every row cost 256 cache lines from the Infinity Cache, 1 GiB per 1 024 queries, and the kernel
// ran 128 us; the lines of a block serve all the queries whose representatives share them.  A block's rows belong to `subs` =
// grid / 32 consecutive workgroups of the kernel above.
// One workgroup per CU, one wave per SIMD: the register budget is spent on loads in flight (amdgpu_waves_per_eu: aiming at 8
// waves per SIMD, hipcc walks a slice chunk by chunk, 8 dependent round trips per step at CH = 8).
template <int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void sample_rescore_f32_kernel(const float* __restrict__ slab,
                                                                 const float* __restrict__ q_padded,
                                                                 const int2* __restrict__ rep_part, int grid, int n_groups,
                                                                 int* __restrict__ rep_row, float* __restrict__ sample_best) {
    constexpr int64_t stride = 128 * CH;
    __shared__ float part[32][9];
    __shared__ int rw[32];
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int c = threadIdx.x >> 3, w = threadIdx.x & 7;
    const int subs = grid >> 5;
    const int lane = lane_id();
    if (j >= n_groups) return;
    // the representative of (query grp * 32 + c, block b): every thread of its 8 ends up with it
    auto pick = [&](int b, int grp) {
        float bs = -INFINITY;
        int br = INT_MAX;
        if (w < subs) {
            const int2 v = rep_part[(int64_t)(grp * 32 + c) * grid + b * subs + w];
            bs = __int_as_float(v.x), br = v.y;
        }
        take_better(bs, br, __int_as_float(xor_lane<1>(__float_as_int(bs), lane)), xor_lane<1>(br, lane));
        take_better(bs, br, __int_as_float(xor_lane<2>(__float_as_int(bs), lane)), xor_lane<2>(br, lane));
        take_better(bs, br, __int_as_float(xor_lane<4>(__float_as_int(bs), lane)), xor_lane<4>(br, lane));
        return br == INT_MAX ? -1 : br;
    };
    int b = x, grp = j;
    int row = pick(b, grp);
    for (;;) {
        // the next step's representative is asked for ahead of this step's gather: one memory round trip per step, not two
        int nb = b, ng = grp + 32;
        if (ng >= n_groups) nb = b + 8, ng = j;
        const bool more = nb < 32;
        const int row_next = more ? pick(nb, ng) : -1;
        float acc = 0.f;
        if (row >= 0) acc = flat_score_slice<CH, 1>(slab, stride, q_padded, grp * 32 + c, row, w);
        part[c][w] = acc;
        if (w == 0) rw[c] = row;
        __syncthreads();
        if (threadIdx.x < 32) {
            const int cc = threadIdx.x, qq = grp * 32 + cc;
            float s = part[cc][0];
#pragma unroll
            for (int ww = 1; ww < 8; ++ww) s += part[cc][ww];
            const int r = rw[cc];
            const bool ok = r >= 0 && fabsf(s) < INFINITY;   // false for NaN
            sample_best[(int64_t)qq * kMaxSampleGroups + b] = ok ? s : -INFINITY;
            rep_row[qq * 32 + b] = r;
        }
        if (!more) break;
        __syncthreads();
        b = nb, grp = ng, row = row_next;
    }
}

bool sample_rep_supported(int64_t stride, int grid) {
    return stride >= 128 && stride <= 1024 && stride % 128 == 0 && grid >= 32 && grid % 32 == 0 && grid <= kMaxSampleGroups;
}

hipError_t launch_sample_rep(const float* slab, const int32_t* row_tag, int64_t stride, int grid, const float* q_padded,
                             const int32_t* q_filter, int nq, void* q_frag, void* rep_part, int* rep_row, float* sample_best,
                             hipStream_t stream) {
    if (!sample_rep_supported(stride, grid) || nq < 32 || nq % 32 != 0) return hipErrorInvalidValue;
    bf16x8* const qf = static_cast<bf16x8*>(q_frag);
    int2* const part = static_cast<int2*>(rep_part);
    const int n_frag = (int)((int64_t)nq * stride / 8);
    hipLaunchKernelGGL(sample_queries_frag_kernel, dim3((n_frag + 255) / 256), dim3(256), 0, stream, q_padded, stride, qf, n_frag);
#define RASS_REP_CASE(C)                                                                                                      \
    case C:                                                                                                                   \
        hipLaunchKernelGGL(sample_rep_bf16_kernel<C>, dim3(grid), dim3(kRepThreads), 0, stream, slab, row_tag, qf, q_filter,  \
                           nq / 16, part);                                                                                    \
        hipLaunchKernelGGL(sample_rescore_f32_kernel<C>, dim3(256), dim3(256), 0, stream, slab, q_padded, part, grid, nq / 32, \
                           rep_row, sample_best);                                                                             \
        break;
    switch ((int)(stride >> 7)) {
        RASS_REP_CASE(1) RASS_REP_CASE(2) RASS_REP_CASE(3) RASS_REP_CASE(4)
        RASS_REP_CASE(5) RASS_REP_CASE(6) RASS_REP_CASE(7) RASS_REP_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef RASS_REP_CASE
    return hipGetLastError();
}

// One floor per query, once per batch.  The scans of scan_topk.hip select a query's floor from its sample_best entries in their
// prologue: every wave of every workgroup of every launch, 2 * kFloorBits ballot rounds over kMaxSampleGroups slots for each
// of its queries — the same 1 024 floors found by 256 workgroups in 16 launches of a step.  Here a wave takes one query and
// does that selection once, in the same words: score_key of every entry above -inf (0 otherwise), the largest value of the top
// kFloorBits key bits that at least k keys reach, key_score of it, -inf when there is none.  The step kernel (scan_step.hip)
// reads floors[q] where the others select.
__global__ __launch_bounds__(256) void step_floors_kernel(const float* __restrict__ sample_best, int sample_groups, int nq, int k,
                                                          float* __restrict__ floors) {
    const int lane = lane_id();
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;   // wave-uniform
    unsigned key[kMaxSampleGroups / 64];
#pragma unroll
    for (int j = 0; j < kMaxSampleGroups / 64; ++j) {
        const int grp = lane + 64 * j;
        const float v = grp < sample_groups ? sample_best[(int64_t)q * kMaxSampleGroups + grp] : -INFINITY;
        key[j] = v == -INFINITY ? 0u : score_key(v);
    }
    unsigned T = 0;
#pragma unroll 1
    for (int b = 31; b >= 32 - kFloorBits; --b) {
        const unsigned cand = T | (1u << b);
        int c = 0;
#pragma unroll
        for (int j = 0; j < kMaxSampleGroups / 64; ++j) c += __popcll(__ballot(key[j] >= cand));
        T = c >= k ? cand : T;
    }
    if (lane == 0) floors[q] = T ? key_score(T) : -INFINITY;
}

hipError_t launch_step_floors(const float* sample_best, int sample_groups, int nq, int k, float* floors, hipStream_t stream) {
    if (sample_groups < 1 || sample_groups > kMaxSampleGroups || nq < 1 || k < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(step_floors_kernel, dim3((nq + 3) / 4), dim3(256), 0, stream, sample_best, sample_groups, nq, k, floors);
    return hipGetLastError();
}

}  // namespace rass
