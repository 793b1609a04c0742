// scan_flat.h — the flat pair loop of the boosted, function-score and stats scans (scan_boost.hip, scan_fscore.hip, scan_stats.hip), written once:
// scan_topk_f32_kernel's flat loop (scan_topk.hip) built from the blocks of scan_core.h.  The K axis is split over the 8
// waves, two 16-row blocks of a tile run against NT N-tiles of queries, one v_mfma_f32_16x16x4_f32 chain per (row, query) in
// k order from zero, the partials are summed p0 + ... + p7 out of LDS, two tiles go per barrier and the previous pair is
// ranked between the MFMA chunks of the next — so a score is that kernel's bit for bit, whichever family asks.  What a
// family does with a score is its policy (below); the launcher and the argument checks the families share are at the end.
// Not part of any ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

// The dynamic LDS of a flat pair kernel: the partial images [4][kWaves][NT * 16][kPitch], 144 KiB at NT = 2.
constexpr size_t flat_lds_bytes(int nt) { return (size_t)4 * kWaves * nt * 16 * kPitch * sizeof(float); }

// Per-lane offsets and LDS addresses are derived, where they are used, from a lane id hipcc cannot see through: left visible
// they are loop invariants, hoisted and kept live across the tile loop, which has no register to spare at CH = 8 / NT = 2.
__device__ __forceinline__ int hidden(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// One lane's share of a ranking step: row r of a dumped tile for query q = pq * 16 + (lane >> 5) * 8 + wave.  The row's tag
// and the query's filter word have been read; the score and the query's mask are read where the policy asks for them.
// (Lazy on purpose: a policy reads its own LDS words, the score and the mask in the order the kernels always did, and hipcc's
// schedule and register count for the ranking step stay what they were; reading everything up front cost 1 - 2 VGPRs.)
template <int NT>
struct FlatPart {
    int tid, lane;       // hidden(threadIdx.x) and its low six bits
    int rows;            // how many of the tile's rows exist
    int r, row, q;
    int tag, qfilt;
    const float* src;    // LDS: wave 0's partial of (q, r)
    const int* qmask;    // LDS: the queries' filter masks
    // the score as scan_topk_f32_kernel sums it
    __device__ __forceinline__ float score() const {
        float s = src[0];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) s += src[wv * NT * 16 * kPitch];
        return s;
    }
    // the row exists, is no tombstone and passes q's masked filter
    __device__ __forceinline__ bool live() const {
        return (r < rows) & (tag != -1) & ((qfilt < 0) | (qfilt == (tag & qmask[q])));
    }
};

// The continuation bound of a multi-pass top-k, per query in LDS (s, i: the kernel's __shared__ float [32] and int64_t [32]):
// a candidate must rank strictly after (s[q], i[q]).
struct AfterBound {
    float* s;
    int64_t* i;
    __device__ __forceinline__ void setup(const ScanArgs& p, int q, bool live) {
        s[q] = (p.q_after_score != nullptr && live) ? p.q_after_score[q] : INFINITY;
        i[q] = (p.q_after_id != nullptr && live) ? p.q_after_id[q] : (int64_t)-1;
    }
    // as: s[q], read by the caller ahead of the step's arithmetic so that the wait for it is not exposed behind it
    __device__ __forceinline__ bool passes(int q, float as, float score, int row) const {
        return (score < as) | ((score == as) & ((int64_t)row > i[q]));
    }
};

// A dense fp32 column, per query or shared, that a ranking step reads next to the score (the boosted scan's bonus, the
// function-score scan's function column).  Lane (r = lane & 31, half = lane >> 5) of wave w ranks row r of a tile for query
// pq * 16 + half * 8 + w, so the lane that ranks a (row, query) can fetch its own value: NT coalesced 64-lane loads per tile,
// two 128-byte runs each, and no lane exchange.  Issued inside the ranking step, such a load would make the step wait on
// vmcnt, which counts in order: the wait would drain the two tiles of corpus loads in flight (the trap the KEYS bitmap read
// of scan_topk.hip describes).  So a pair's 2 * NT values are requested at the TOP of the iteration that multiplies the
// pair, ahead of that iteration's refill loads; one iteration later, where the pair is ranked, the wait for the refilled
// tags has seen them come back.  There they are parked in LDS — [2 tiles][NT][512 threads] floats, 8 KiB at NT = 2 beside
// the 144 KiB of partial images, each lane writing and reading its own slot, so no barrier is involved — and the registers
// take the next pair's request: 2 * NT VGPRs live across the loop instead of 4 * NT, which CH = 8 / NT = 2 does not have.
// Every load goes through one buffer descriptor over the launch group's column(s); a lane at or past the `n` rows the caller
// grants a tile (past the tile's rows, past the column's, a run-ahead tile) gets an offset past the records: 0 comes back and
// no memory request is made.
// THREADED picks between the two shapes hipcc gives the requests, each family keeping the one its own kernels had and were
// measured with.  false (function-score): a request's address arithmetic sits under an exec-mask branch on the lane's
// validity and the 2 * NT requests go out in a block ahead of the first MFMA.  true (boosted): the offset is built ahead of
// the validity select and hidden from it, so the requests are threaded between the first MFMA chunks, and tile B's values,
// requested last, are parked first, so that one wait serves the stores.  Swapped, either family measured slower or carried
// more s_waitcnt than its parent (profiles/flat_loop_probe_parent_vs_new.json.txt).
template <int NT, bool THREADED>
struct PairColumn {
    __amdgpu_buffer_rsrc_t rsrc;
    int64_t q_stride;
    int nq, wid;
    float (*parked)[NT][kThreads];   // LDS: the pair being ranked, [tile of the pair][pq][thread], lane-private
    float A[NT], B[NT];              // the values of the pair last requested (tile A, tile B)

    __device__ __forceinline__ void setup(const float* column, unsigned bytes, int64_t q_stride_, int nq_, float (*lds)[NT][kThreads]) {
        rsrc = make_rsrc(reinterpret_cast<uint64_t>(column), bytes);
        q_stride = q_stride_, nq = nq_, wid = wave_id(), parked = lds;
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) A[pq] = B[pq] = 0.f;
    }
    // The value of this lane's (row, query) of a tile.  Queries past nq (zero rows, never written) read the last live
    // query's column: in bounds.  The two halves' column offsets are wave-uniform; one select picks the lane's.
    __device__ __forceinline__ float load(int tile, int n, int pq) const {
        const int lane = hidden(lane_id());
        const unsigned r4 = (unsigned)(lane & 31) * 4u;
        const int qa = min(pq * 16 + wid, nq - 1), qb = min(pq * 16 + 8 + wid, nq - 1);
        const unsigned tile_off = (unsigned)tile * (unsigned)(kTileRows * 4);
        const unsigned offa = (unsigned)((int64_t)qa * q_stride * 4) + tile_off;
        const unsigned offb = (unsigned)((int64_t)qb * q_stride * 4) + tile_off;
        const bool valid = (lane & 31) < n;
        unsigned voff;
        if constexpr (THREADED) {
            const unsigned off = (unsigned)hidden((int)(((lane & 32) ? offb : offa) + r4));
            voff = valid ? off : 0xffffffffu;
        } else {
            voff = valid ? ((lane & 32) ? offb : offa) + r4 : 0xffffffffu;
        }
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, 0, 0));
    }
    __device__ __forceinline__ void park() {
        const int tid = hidden((int)threadIdx.x);
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            if (THREADED) parked[1][pq][tid] = B[pq];
            parked[0][pq][tid] = A[pq];
            if (!THREADED) parked[1][pq][tid] = B[pq];
        }
    }
    // the previous pair's values have arrived (requested before the loads whose tags were just stored): park them for this
    // iteration's ranking, then request this pair's, ahead of the refills
    __device__ __forceinline__ void park_and_request(int tile0, int n0, int tile1, int n1) {
        park();
#pragma unroll
        for (int pq = 0; pq < NT; ++pq) {
            A[pq] = load(tile0, n0, pq);
            B[pq] = load(tile1, n1, pq);
        }
    }
};

// The loop's own LDS words, declared by the kernel next to its policy's (one place lists a kernel's static LDS, and hipcc lays
// the words out — and pairs their reads in the ranking step — as it did when each kernel held the loop itself).
struct FlatShared {
    int* qfilt;        // __shared__ int [32]: the queries' filter words, -1 = none
    int* qmask;        // __shared__ int [32]: their masks
    int (*tags)[32];   // __shared__ int [4][32]: the dumped tiles' row tags
};

// The loop.  A Policy is an object in the kernel's registers with
//     setup(q, live)            thread q < 32 fills the policy's per-query LDS words (live: q < nq); a barrier follows
//     tile_ahead(which, w)      tile w is about to be requested into register set `which` (0 / 1): ahead of its corpus loads,
//                               in the prologue and before each refill; every thread
//     pair_top(w0, w1)          the top of the iteration that multiplies (w0, w1), ahead of its refills; every thread
//     rank(part, buf, which, pq)  rank or emit one lane's FlatPart of tile `which` of the previous pair, dumped in image buf
//     last_pair()               before the last pair is ranked, behind the loop
// and the order of these against the corpus loads is the loop's: requests ahead of the refills, parking before the
// requests, one barrier per iteration.
// Both column scans leave tile_ahead empty (their columns are requested a pair at a time, in pair_top) and fill every other
// hook; the stats scan (scan_stats.hip) requests its key and value words there, as the group-top scan does.  The group-top scan (scan_grouptop.hip) keeps a loop of its own: on this one it measured
// 0.66 % slower at group_size 3 over 100 groups, or, with its key read first, carried one s_waitcnt more in 4 kernels.
template <int CH, int NT, typename Policy>
__device__ __forceinline__ void flat_pair_scan(const ScanArgs& p, const FlatShared& sh, Policy& pol) {
    constexpr int NQ = NT * 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][kWaves][NQ][kPitch]

    const int lane = lane_id();
    const int wid = wave_id();
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

    int* const sh_qfilt = sh.qfilt;
    int* const sh_qmask = sh.qmask;
    int (*const sh_tags)[32] = sh.tags;
    if (threadIdx.x < 32) {
        const int q = threadIdx.x;
        const bool live = q < p.nq;
        sh_qfilt[q] = (p.q_filter != nullptr && live) ? p.q_filter[q] : -1;
        sh_qmask[q] = (p.q_filter_mask != nullptr && live) ? p.q_filter_mask[q] : -1;
        pol.setup(q, live);
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
    pol.tile_ahead(0, W0);
    pol.tile_ahead(1, W1);
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
    // One (tile, query group pq) of a dumped tile, handed to the policy's ranking.
    auto rank_part = [&](const WorkItem& w, int buf, int which, int pq) {
        FlatPart<NT> c;
        c.tid = hidden((int)threadIdx.x), c.lane = c.tid & 63;
        const float* P = lds + buf * (kWaves * NQ * kPitch);
        c.rows = w.rows;
        c.r = c.lane & 31;
        c.row = w.tile * kTileRows + c.r;
        c.tag = sh_tags[buf][c.r];
        c.q = pq * 16 + (c.lane >> 5) * 8 + wid;
        c.qfilt = sh_qfilt[c.q];
        c.src = P + c.q * kPitch + c.r;
        c.qmask = sh_qmask;
        pol.rank(c, buf, which, pq);
    };

    constexpr int kParts = 2 * NT;
    auto slot_of = [](int part) { return max(((part + 1) * 2 * CH) / kParts - 1, 0); };
    WorkItem Pa{0, 0, 0u}, Pb{0, 0, 0u};  // the previous pair (rows = 0: nothing ranks in the first iteration)
    int pair = 0;  // 0 / 2: which two LDS images this iteration dumps into
    while (t < n_tiles) {
        f32x4 acc[2][NT];
        if (wid == 0 && lane < 32) {
            sh_tags[pair][lane] = R0.tag;
            sh_tags[pair + 1][lane] = R1.tag;
        }
        pol.pair_top(W0, W1);
        const WorkItem Wa = W0;
        t += 2 * G;
        WorkItem Wn = work(t);
        pol.tile_ahead(0, Wn);
        auto rank_prev = [&](int slot) {
#pragma unroll
            for (int part = 0; part < kParts; ++part)
                if (slot_of(part) == slot) {
                    if (part < NT)
                        rank_part(Pa, pair ^ 2, 0, part);
                    else
                        rank_part(Pb, (pair ^ 2) + 1, 1, part - NT);
                }
        };
        multiply_and_refill<CH, NT>(R0, qf, acc, make_tile_desc(p.corpus, p.row_stride, p.row_tag, Wn), voff_lane, mt_step,
                                    [&](int j) { rank_prev(j); });
        dump_tile(acc, pair);
        W0 = Wn;
        const WorkItem Wb = W1;
        Wn = work(t + G);
        pol.tile_ahead(1, Wn);
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
    pol.last_pair();
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pa, pair ^ 2, 0, pq);
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) rank_part(Pb, (pair ^ 2) + 1, 1, pq);
}

// Top-k state of a ranking policy: pass pq handles query pq*16 + (lane>>5)*8 + wave for row lane&31.
// (the threshold of a list — its k-th score — is re-read from the list at every ranking step, not carried: two readlanes
// against a register per list that CH = 8 / NT = 2 does not have)
template <int NT>
__device__ __forceinline__ void init_lists(TopList (&L)[NT]) {
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        L[pq].s = -INFINITY;
        L[pq].i = 0x7fffffff;
    }
}

// Per-workgroup sorted lists -> [gridDim.x][nq][k]
template <int NT>
__device__ __forceinline__ void store_lists(const ScanArgs& p, const TopList (&L)[NT]) {
    const int lane = lane_id(), wid = wave_id();
    const int lpos = lane & 31;
#pragma unroll
    for (int pq = 0; pq < NT; ++pq) {
        const int q = pq * 16 + (lane >> 5) * 8 + wid;
        if (q < p.nq && lpos < p.k) {
            const int64_t o = ((int64_t)blockIdx.x * p.nq + q) * p.k + lpos;
            const bool filled = L[pq].i != 0x7fffffff;
            p.part_scores[o] = filled ? L[pq].s : -INFINITY;
            p.part_ids[o] = filled ? (int64_t)L[pq].i : (int64_t)-1;
        }
    }
}

// ---- host side: one launcher for the families on this loop ------------------------------------------------------------------------
// A Family names its kernels (the group-top scan keeps its own launcher with its own loop): template <int CH, int NT>
// static constexpr auto kernel() returns &its_kernel<CH, NT>, a
// __global__ function of one argument struct whose first member is the ScanArgs `scan`.

template <typename Family, int CH, int NT, typename Args>
hipError_t launch_flat_variant(const Args& a, int grid, hipStream_t stream) {
    void (*const kernel)(Args) = Family::template kernel<CH, NT>();
    static bool attr_set = false;   // once per instantiation
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)flat_lds_bytes(NT));
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), flat_lds_bytes(NT), stream, a);
    return hipGetLastError();
}

template <typename Family, int NT, typename Args>
hipError_t launch_flat_ch(const Args& a, int grid, hipStream_t stream) {
    switch ((int)(a.scan.row_stride / 128)) {
        case 1: return launch_flat_variant<Family, 1, NT>(a, grid, stream);
        case 2: return launch_flat_variant<Family, 2, NT>(a, grid, stream);
        case 3: return launch_flat_variant<Family, 3, NT>(a, grid, stream);
        case 4: return launch_flat_variant<Family, 4, NT>(a, grid, stream);
        case 5: return launch_flat_variant<Family, 5, NT>(a, grid, stream);
        case 6: return launch_flat_variant<Family, 6, NT>(a, grid, stream);
        case 7: return launch_flat_variant<Family, 7, NT>(a, grid, stream);
        case 8: return launch_flat_variant<Family, 8, NT>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

// The instantiation for a.scan's row stride (CH) and query count (NT = 1: <= 16 queries, 2: 17 .. 32).
template <typename Family, typename Args>
hipError_t launch_flat_family(const Args& a, int grid, hipStream_t stream) {
    return a.scan.nq <= 16 ? launch_flat_ch<Family, 1>(a, grid, stream) : launch_flat_ch<Family, 2>(a, grid, stream);
}

// What the launchers of the families on this loop check of their ScanArgs alike; what differs stays in the unit.
inline bool flat_scan_args_ok(const ScanArgs& s, int grid) {
    if (s.row_stride % 128 != 0 || s.row_stride < 128 || s.row_stride > 1024) return false;   // narrow rows only
    if (s.nq < 1 || s.nq > 32 || s.n_rows < 1 || grid < 1) return false;
    if (!s.corpus || !s.q_padded) return false;
    if (s.q_filter_mask != nullptr && s.q_filter == nullptr) return false;
    if (s.q_filter != nullptr && s.row_tag == nullptr) return false;
    // fields that must stay at their default in every family
    if (s.work_tile || s.work_base || s.sample_pass || s.sample_best || s.wgs_per_group || s.live_nq || s.range_count || s.count_table ||
        s.id_base != 0)
        return false;
    return true;
}

}  // namespace rass
