// scan_grouptop.hip — the group-top scan: the group_size best rows of every (query, group) of a flat fp32 index in ONE corpus
// pass (api_grouptop.hip, rass_index_search_group_hits_keys): the inner hits of a collapsed search.  The group-max scan
// (scan_topk.hip, kGroupMaxKeys) keeps one 64-bit slot per (query, group); this one keeps a chain of group_size of them
// (scan_core.h emit_group_top), level-major in the table, so that plane 0 is byte for byte what the group-max scan leaves and
// group_select_kernel (group_topk.hip) runs on it unchanged.
//
// scan_grouptop_f32_kernel<CH, NT> is scan_topk_f32_kernel's flat loop (scan_topk.hip) built from the same blocks of
// scan_core.h: the K axis split over the 8 waves, two 16-row blocks of a tile against NT N-tiles of queries, one
// v_mfma_f32_16x16x4_f32 chain per (row, query) in k order from zero, the partials summed p0 + ... + p7 out of LDS, two
// tiles per barrier, the previous pair emitted between the MFMA chunks of the next — so a score is that kernel's bit for bit.
// Nothing is ranked: no TopList, no sample floor, no continuation bound.  A row is folded in for query q when it is live,
// passes q's masked filter, has a group (key >= 0, row < group_key_rows), has its bit in q's bitmap where there is one, and
// s > -inf (a NaN or -inf score never ranks); a key >= group_n on such a row sets the status word instead.
//
// The row's group travels as the tag does (the KEYS modes of scan_topk.hip): one 32-lane buffer load per tile through a
// descriptor of its own, requested AHEAD of the tile's corpus loads so that the wait that parks the tile's tags in LDS has
// seen it come back, and parked next to them.  The bitmap words of a wave's two queries of a step are wave-uniform and come
// by scalar loads through the constant address space: the kernel writes global memory, so a plain load would come out as a
// vector load whose wait drains the corpus stream between the MFMA chunks.
//
// Plain vector loads, stores and atomics only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

template <int CH, int NT>
__global__ __launch_bounds__(kThreads, 2) void scan_grouptop_f32_kernel(GroupTopArgs a) {
    const ScanArgs& p = a.scan;
    constexpr int NQ = NT * 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int G = gridDim.x, bid = blockIdx.x;
    const int n_tiles = (p.n_rows + kTileRows - 1) / kTileRows;

    // Query fragments: lane (n = m, g) holds Qn[nt*16 + n][slice + 16j + 4g .. +3].
    f32x4 qf[NT][CH];
    {
        const float* qbase = p.q_padded + (int64_t)m * p.row_stride + wid * 16 * CH + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < CH; ++j)
                qf[nt][j] = *reinterpret_cast<const f32x4*>(qbase + (int64_t)nt * 16 * p.row_stride + 16 * j);
    }
    const int voff_lane = wid * CH * 1024 + lane * 16;

    __shared__ int sh_qfilt[32];
    __shared__ int sh_qmask[32];
    __shared__ int sh_tags[4][32];
    __shared__ int sh_keys[4][32];   // the dumped tiles' group keys, next to their tags
    if (threadIdx.x < 32) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
    }
    __syncthreads();

    const int mt_step = 16 * (int)p.row_stride * 4;
    TileRegs<CH> R0, R1;
    int t = bid;          // the item R0 holds; R1 holds t + G, then every workgroup steps by 2 G
    auto work = [&](int i) {
        int rows = p.n_rows - i * kTileRows;
        rows = rows < 0 ? 0 : (rows > kTileRows ? kTileRows : rows);
        WorkItem w;
        w.tile = i < n_tiles ? i : 0;
        w.rows = i < n_tiles ? rows : 0;
        w.mask = 0xffffffffu;
        return w;
    };
    WorkItem W0 = work(t), W1 = work(t + G);
    // the two tiles' group keys, one register each, requested ahead of the tiles' own loads here and in the main loop
    int K0 = load_tile_keys(p.group_keys, p.group_key_rows, W0);
    int K1 = load_tile_keys(p.group_keys, p.group_key_rows, W1);
    issue_tile_loads<CH>(R0, make_tile_desc(p.corpus, p.row_stride, p.row_tag, W0), voff_lane, mt_step);
    issue_tile_loads<CH>(R1, make_tile_desc(p.corpus, p.row_stride, p.row_tag, W1), voff_lane, mt_step);
    __builtin_amdgcn_sched_barrier(0);

    auto dump_tile = [&](const f32x4 (&acc)[2][NT], int buf) {
        float* P = lds + buf * (kWaves * NQ * kPitch);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                *reinterpret_cast<f32x4*>(P + (wid * NQ + nt * 16 + m) * kPitch + mt * 16 + 4 * g) = acc[mt][nt];
    };
    // Emit one (tile, query group pq) of a dumped tile: the score as scan_topk_f32_kernel sums it, then the row's key into
    // the chain of its (query, group).
    // The lane's offsets and LDS addresses are derived, where they are used, from a lane id hipcc cannot see through: left
    // visible they are loop invariants, hoisted and kept live across the tile loop, which has no register to spare at
    // CH = 8 / NT = 2 (scan_boost.hip).
    auto hidden = [](int v) {
        asm volatile("" : "+v"(v));
        return v;
    };
    auto rank_part = [&](const WorkItem& w, int buf, int pq) {
        const int lane = hidden(lane_id());
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        const int r = lane & 31;
        const int row = w.tile * kTileRows + r;
        const int tag = sh_tags[buf][r];
        const int key = sh_keys[buf][r];
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        const int qf1 = sh_qfilt[q];
        const float* src = P + q * kPitch + r;
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NQ * kPitch];
        // no group: not a match, whatever the key's size
        bool ok = (r < w.rows) & (tag != -1) & ((qf1 < 0) | (qf1 == (tag & sh_qmask[q]))) & (key >= 0) & (row < p.group_key_rows) &
                  (q < p.nq);
        if (p.allow != nullptr) {   // a kernel argument: a scalar branch
            typedef const __attribute__((address_space(4))) unsigned* const_words;
            const const_words allow = (const_words)reinterpret_cast<uintptr_t>(p.allow);
            // queries past nq (zero rows, never emitted) read the last live query's word: in bounds
            const int qa = min(pq * 16 + wid, p.nq - 1), qb = min(pq * 16 + 8 + wid, p.nq - 1);
            const unsigned wa = allow[(int64_t)qa * p.allow_q_stride + w.tile];
            const unsigned wb = allow[(int64_t)qb * p.allow_q_stride + w.tile];
            ok = ok && ((((lane & 32) ? wb : wa) >> r) & 1u);
        }
        emit_group_top(ok, s, row, key, p.group_n, p.group_table, (unsigned)q * (unsigned)p.group_n, (unsigned)a.level_stride,
                       a.group_size, p.group_status);
    };

    constexpr int kParts = 2 * NT;
    auto slot_of = [](int part) { return max(((part + 1) * 2 * CH) / kParts - 1, 0); };
    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};  // the previous pair (rows = 0: nothing is emitted in the first iteration)
    int pair = 0;  // 0 / 2: which two LDS images this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[2][NT];
        if (wid == 0 && lane < 32) {
            sh_tags[pair][lane] = R0.tag;
            sh_tags[pair + 1][lane] = R1.tag;
            sh_keys[pair][lane] = K0;
            sh_keys[pair + 1][lane] = K1;
        }
        const WorkItem Wa = W0;
        t += 2 * G;
        WorkItem Wn = work(t);
        K0 = load_tile_keys(p.group_keys, p.group_key_rows, Wn);
        auto rank_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < kParts; ++part)
                if (slot_of(part) == slot) {
                    if (part < NT)
                        rank_part(Pa, pair ^ 2, part);
                    else
                        rank_part(Pb, (pair ^ 2) + 1, part - NT);
                }
        };
        multiply_and_refill<CH, NT>(R0, qf, acc, make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn), voff_lane, mt_step,
                                    [&](int j) { rank_prev(j); });
        dump_tile(acc, pair);
        W0 = Wn;
        const WorkItem Wb = W1;
        Wn = work(t + G);
        K1 = load_tile_keys(p.group_keys, p.group_key_rows, Wn);
        multiply_and_refill<CH, NT>(R1, qf, acc, make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn), voff_lane, mt_step,
                                    [&](int j) { rank_prev(CH + j); });
        dump_tile(acc, pair + 1);
        W1 = Wn;
        Pa = Wa;
        Pb = Wb;
        __syncthreads();
        pair ^= 2;
    }
    // the last pair
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pa, pair ^ 2, pq);
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pb, (pair ^ 2) + 1, pq);
}

template <int CH, int NT>
static hipError_t launch_grouptop_variant(const GroupTopArgs& a, int grid, hipStream_t stream) {
    constexpr size_t lds_bytes = (size_t)4 * kWaves * NT * 16 * kPitch * sizeof(float);  // 144 KiB at NT = 2
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_grouptop_f32_kernel<CH, NT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_grouptop_f32_kernel<CH, NT>), dim3(grid), dim3(kThreads), lds_bytes, stream, a);
    return hipGetLastError();
}

template <int NT>
static hipError_t launch_grouptop_ch(int ch, const GroupTopArgs& a, int grid, hipStream_t stream) {
    switch (ch) {
        case 1: return launch_grouptop_variant<1, NT>(a, grid, stream);
        case 2: return launch_grouptop_variant<2, NT>(a, grid, stream);
        case 3: return launch_grouptop_variant<3, NT>(a, grid, stream);
        case 4: return launch_grouptop_variant<4, NT>(a, grid, stream);
        case 5: return launch_grouptop_variant<5, NT>(a, grid, stream);
        case 6: return launch_grouptop_variant<6, NT>(a, grid, stream);
        case 7: return launch_grouptop_variant<7, NT>(a, grid, stream);
        case 8: return launch_grouptop_variant<8, NT>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_grouptop_f32(const GroupTopArgs& a, int grid, hipStream_t stream) {
    const ScanArgs& s = a.scan;
    if (s.row_stride % 128 != 0 || s.row_stride < 128 || s.row_stride > 1024) return hipErrorInvalidValue;   // narrow rows only
    if (s.nq < 1 || s.nq > 32 || s.n_rows < 1 || grid < 1) return hipErrorInvalidValue;
    if (!s.corpus || !s.q_padded || !s.group_table || !s.group_status || !s.group_keys) return hipErrorInvalidValue;
    if (s.group_n < 1 || s.group_n > kGroupMaxGroups || s.group_key_rows < 0) return hipErrorInvalidValue;
    // every slot a lane can name lies inside the table: (group_size - 1) planes, then (nq - 1) rows of group_n, then a key < group_n
    if (a.group_size < 1 || a.group_size > kGroupHitsMaxSize || (int64_t)s.group_n * a.group_size > kGroupMaxGroups ||
        a.level_stride < (int64_t)s.nq * s.group_n || a.level_stride * a.group_size > ((int64_t)1 << 25))   // one 32-bit slot index
        return hipErrorInvalidValue;
    if (s.q_filter_mask != nullptr && s.q_filter == nullptr) return hipErrorInvalidValue;
    if (s.q_filter != nullptr && s.row_tag == nullptr) return hipErrorInvalidValue;
    if (s.allow_q_stride < 0) return hipErrorInvalidValue;
    if (s.work_tile || s.work_base || s.sample_pass || s.sample_best || s.wgs_per_group || s.live_nq || s.range_count || s.count_table ||
        s.q_after_score || s.q_after_id || s.range_thr || s.id_base != 0)
        return hipErrorInvalidValue;
    const int ch = (int)(s.row_stride / 128);
    return s.nq <= 16 ? launch_grouptop_ch<1>(ch, a, grid, stream) : launch_grouptop_ch<2>(ch, a, grid, stream);
}

}  // namespace rass
