// mmr.hip — the two kernels of the diversified (MMR) search and of rass_index_rows_gram (include/rass_engine.h):
//   rows_gram_kernel   G = R Rt of short row lists, the rows read straight out of the tile16 slab
//   mmr_select_kernel  the greedy maximal-marginal-relevance selection over one query's candidates
// Both are latency-sized (a 32-query group is 32 x 128 rows and ~1 GFLOP next to the scan's 65): one wave per unit of work,
// no LDS, no workspace.  Built with -ffp-contract=off (Makefile): the selection's objective is two products and a
// difference, each rounded on its own, which tests/mmr_ref.py restates in numpy bit for bit.

#include <algorithm>

#include "kernels.h"

namespace rass {
namespace {

typedef float float4v __attribute__((ext_vector_type(4)));

// Ordinal r of a list names a row that contributes: inside the slab's rows and not tombstoned.
__device__ __forceinline__ bool gram_row_live(int64_t r, int64_t n_rows, const int32_t* __restrict__ tags) {
    return r >= 0 && r < n_rows && (tags == nullptr || tags[r] != -1);
}

// One wave per (list, pair of 16-row tiles ti <= tj): D = A Bt over the whole row, A = rows of tile ti, B = rows of tile tj.
// The gather is fused into the operand loads: in the tile16 layout (kernels.h) the four columns 16 j + 4 g .. + 3 of row r
// are ONE 16-byte word at block(r) + j * 256 + (g * 16 + (r & 15)) * 4, and lane g * 16 + m holding them for row m IS the
// A (and B) operand of four v_mfma_f32_16x16x4_f32 k-steps: step t multiplies columns {16 j + 4 g + t, g = 0..3}.  Every
// (i, j) is ONE k-ordered fma chain from zero, chunk after chunk, whatever the list length or the grid: the MMR call and the
// public entry point get the same bits.  Element (i, j) with ti < tj is computed once and stored twice; on a diagonal tile
// the upper triangle is mirrored: G is bitwise symmetric.  Padding lanes (ordinal outside the slab, tombstoned row, index
// past list_len) load nothing and hold zeros; their rows and columns are stored as +0.0.
__global__ __launch_bounds__(64) void rows_gram_kernel(const float* __restrict__ slab, int64_t stride,
                                                       const int32_t* __restrict__ tags, int64_t n_rows,
                                                       const int64_t* __restrict__ rows, int list_len,
                                                       float* __restrict__ out) {
    const int lane = threadIdx.x, m = lane & 15, g = lane >> 4;
    const int tiles = (list_len + 15) >> 4;
    int ti = 0, rem = blockIdx.x;   // pair index -> (ti, tj), row-major over the upper triangle
    while (rem >= tiles - ti) {
        rem -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int64_t list = blockIdx.y;
    const int64_t* my_rows = rows + list * list_len;
    const int ia = ti * 16 + m, ib = tj * 16 + m;
    const int64_t ra = ia < list_len ? my_rows[ia] : -1;
    const int64_t rb = ib < list_len ? my_rows[ib] : -1;
    const bool va = gram_row_live(ra, n_rows, tags), vb = gram_row_live(rb, n_rows, tags);
    const float* pa = va ? slab + (ra >> 4) * 16 * stride + ((g * 16 + (int)(ra & 15)) * 4) : nullptr;
    const float* pb = vb ? slab + (rb >> 4) * 16 * stride + ((g * 16 + (int)(rb & 15)) * 4) : nullptr;
    const bool diag = ti == tj;   // wave-uniform

    const float4v zero = {0.0f, 0.0f, 0.0f, 0.0f};
    float4v acc = zero;
    const int chunks = (int)(stride >> 4);   // stride is a multiple of 128: a multiple of 4 chunks
    for (int j = 0; j < chunks; j += 4) {
        float4v a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = va ? *reinterpret_cast<const float4v*>(pa + (int64_t)(j + u) * 256) : zero;
            b[u] = diag ? a[u] : (vb ? *reinterpret_cast<const float4v*>(pb + (int64_t)(j + u) * 256) : zero);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc, 0, 0, 0);
        }
    }

    // D[i][j]: column j = lane & 15, row i = 4 * (lane >> 4) + register
    const unsigned live_a = (unsigned)__ballot(va) & 0xffffu;   // lanes 0..15: row m of tile ti
    const unsigned live_b = (unsigned)__ballot(vb) & 0xffffu;
    float* g_out = out + list * list_len * list_len;
    const int gj = tj * 16 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * g + r, gi = ti * 16 + i;
        if (gi >= list_len || gj >= list_len) continue;
        if (diag && i > m) continue;   // the lower triangle of a diagonal tile is the mirror of the upper
        const bool live = ((live_a >> i) & 1u) && ((live_b >> m) & 1u);
        const float v = live ? acc[r] : 0.0f;
        g_out[(int64_t)gi * list_len + gj] = v;
        if (gi != gj) g_out[(int64_t)gj * list_len + gi] = v;
    }
}

// One wave per query, two candidates per lane (ranks lane and lane + 64).  Candidates are a prefix of the list: rows >= 0.
// Step t: obj_i = lambda * s_i - (1 - lambda) * pen_i (the second product +0.0 at the first step), each operation rounded
// to fp32 on its own; the largest wins, ties to the lowest rank (a butterfly of __shfl_xor: every lane ends with the
// winner); pen_i = G[p][i] at first, then the larger of pen_i and G[p][i] (`>`: no clipping, no fmax).  A lambda that
// is NaN or outside [0, 1] selects nothing.
__global__ __launch_bounds__(64) void mmr_select_kernel(const float* __restrict__ cand_s, const int64_t* __restrict__ cand_rows,
                                                        const float* __restrict__ gram, const float* __restrict__ lambda,
                                                        int fetch_k, int k, int64_t id_base, const int64_t* __restrict__ id_map,
                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                        int32_t* __restrict__ out_rank) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int i0 = lane, i1 = lane + 64;
    const float* my_s = cand_s + (int64_t)q * fetch_k;
    const int64_t* my_rows = cand_rows + (int64_t)q * fetch_k;
    const float* my_g = gram + (int64_t)q * fetch_k * fetch_k;
    const float l = lambda[q];
    const bool l_ok = l >= 0.0f && l <= 1.0f;   // false for NaN
    const float mcoef = __fsub_rn(1.0f, l);
    const int64_t row0 = i0 < fetch_k ? my_rows[i0] : -1, row1 = i1 < fetch_k ? my_rows[i1] : -1;
    const float s0 = row0 >= 0 ? my_s[i0] : 0.0f, s1 = row1 >= 0 ? my_s[i1] : 0.0f;
    bool free0 = l_ok && row0 >= 0, free1 = l_ok && row1 >= 0;
    const int c = __popcll(__ballot(free0)) + __popcll(__ballot(free1));
    const int steps = k < c ? k : c;
    const float rel0 = __fmul_rn(l, s0), rel1 = __fmul_rn(l, s1);
    float pen0 = 0.0f, pen1 = 0.0f;
    constexpr int kNone = 0x7fffffff;
    for (int t = 0; t < steps; ++t) {
        const float o0 = __fsub_rn(rel0, t == 0 ? 0.0f : __fmul_rn(mcoef, pen0));
        const float o1 = __fsub_rn(rel1, t == 0 ? 0.0f : __fmul_rn(mcoef, pen1));
        float best = free0 ? o0 : -INFINITY;
        int arg = free0 ? i0 : kNone;
        if (free1 && (arg == kNone || o1 > best)) best = o1, arg = i1;   // i0 < i1: a tie stays with i0
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (oa != kNone && (arg == kNone || ob > best || (ob == best && oa < arg))) best = ob, arg = oa;
        }
        const int p = arg;   // wave-uniform; t < c: some candidate was free
        const float sp = __shfl(p < 64 ? s0 : s1, p & 63);
        const int64_t rp = __shfl(p < 64 ? row0 : row1, p & 63);
        if (lane == 0) {
            out_scores[(int64_t)q * k + t] = sp;
            out_ids[(int64_t)q * k + t] = id_map ? id_map[rp] : id_base + rp;
            if (out_rank) out_rank[(int64_t)q * k + t] = p;
        }
        if (p == i0) free0 = false;
        if (p == i1) free1 = false;
        const float* g_row = my_g + (int64_t)p * fetch_k;
        if (i0 < fetch_k) {
            const float gv = g_row[i0];
            pen0 = (t == 0 || gv > pen0) ? gv : pen0;
        }
        if (i1 < fetch_k) {
            const float gv = g_row[i1];
            pen1 = (t == 0 || gv > pen1) ? gv : pen1;
        }
    }
    for (int t = steps + lane; t < k; t += 64) {
        out_scores[(int64_t)q * k + t] = -INFINITY;
        out_ids[(int64_t)q * k + t] = -1;
        if (out_rank) out_rank[(int64_t)q * k + t] = -1;
    }
}

}  // namespace

hipError_t launch_rows_gram(const float* slab, int64_t stride, const int32_t* tags, int64_t n_rows, const int64_t* rows,
                            int64_t n_lists, int list_len, float* out, hipStream_t stream) {
    if (n_lists < 0 || list_len < 1 || list_len > kMmrMaxFetch || n_rows < 0 || stride < 128 || stride % 128 != 0)
        return hipErrorInvalidValue;
    if (n_lists == 0) return hipSuccess;
    if (!rows || !out || (n_rows > 0 && !slab)) return hipErrorInvalidValue;
    const int tiles = (list_len + 15) / 16;
    const int pairs = tiles * (tiles + 1) / 2;
    constexpr int64_t kMaxGridY = 32768;
    for (int64_t done = 0; done < n_lists; done += kMaxGridY) {
        const int64_t b = std::min(kMaxGridY, n_lists - done);
        hipLaunchKernelGGL(rows_gram_kernel, dim3(pairs, (unsigned)b), dim3(64), 0, stream, slab, stride, tags, n_rows,
                           rows + done * list_len, list_len, out + done * list_len * list_len);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_mmr_select(const float* cand_s, const int64_t* cand_rows, const float* gram, const float* lambda, int nq,
                             int fetch_k, int k, int64_t id_base, const int64_t* id_map, float* out_scores, int64_t* out_ids,
                             int32_t* out_rank, hipStream_t stream) {
    if (nq < 1 || fetch_k < 1 || fetch_k > kMmrMaxFetch || k < 1 || k > fetch_k || !cand_s || !cand_rows || !gram || !lambda ||
        !out_scores || !out_ids)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmr_select_kernel, dim3(nq), dim3(64), 0, stream, cand_s, cand_rows, gram, lambda, fetch_k, k, id_base, id_map,
                       out_scores, out_ids, out_rank);
    return hipGetLastError();
}

}  // namespace rass
