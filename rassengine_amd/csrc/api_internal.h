// api_internal.h — what the host-side translation units of the C ABI (include/rass_engine.h) share: the engine / index /
// IVF objects, the error plumbing, the limits, and the building blocks every launch path is made of.  Host C++ only; the
// kernels live behind kernels.h.  Not part of the public ABI.
//
//   api.hip          errors; the engine and the flat index: create / grow / add / delete / persist / destroy; timers, the
//                    stateless wrappers, k-means, peer buffers
//   api_scan.hip     the tuning switches, the shared launch helpers declared below, and the four flat launch paths
//   api_search.hip   flat top-k search entry points: one group, the fused batches, the candidates hooks, the host API with
//                    its pinned slots (k > 32 in passes), search_multi
//   api_emit.hip     the searches that ride the exact scan and emit instead of ranking: the score-threshold (range) search,
//                    the grouped (collapsed) search, the terms aggregation; their shared device-group driver
//   api_ivf.hip      IVF: the host-planned and the device-planned build on one build tail, persistence over one section
//                    list, the probe and the batch on one fine scan, the delta, the host API (host_groups)
//   api_ivf_allow.hip  the IVF probe within a row bitmap (probe plan -> slab-order bitmap words -> the allow-list scan), the probed lists
//   api_allow.hip    the allow-list search (top-k within a per-query row bitmap), its bitmap builders, its plan, a bitmap's popcount
//   api_boost.hip    the boosted search (top-k of boost * T(cos) + a per-row bonus column) and the builders of its columns;
//                    its checks, group loops and pass driver (boost_search_host / _device, boost_device_group) also run the
//                    function-score search
//   api_fscore.hip   the function-score search (top-k of combine(boost * T(cos), a function column), gated by similarity): its
//                    entry points on api_boost.hip's search path, and the builder of its columns
//   api_grouptop.hip the grouped search with inner hits (the group_size best rows of each top group, the capped list) over a
//                    key column, on a scan family of its own (scan_grouptop.hip) and the grouped search's table block
//   api_keys.hip     the key columns built from the attribute columns (what the grouped search and the aggregation group by)
//   api_attr.hip     the attribute columns of a flat index and the predicate builder that turns clauses over them into bitmaps
//   api_mmr.hip      the diversified (MMR) search and the Gram matrices of row lists
//   api_compact.hip  compaction of a flat index, its layout epoch, the stateless wrappers of compact.hip
//
// Ownership model: the engine singleton of a process owns the corpus slabs
// for process lifetime; callers own every host buffer they pass in or get filled.
// Threading: add/delete/grow take the index mutex; searches take the engine mutex only
// while ENQUEUING (all GPU work of an engine is ordered on one stream, so the shared device
// scratch and staging are safe by stream order) and wait for their results on a per-call
// event outside of it, on a pinned host slot taken from a small pool: searches on different
// indices (users) overlap their host round trips instead of serialising on a stream sync.
// rows / deleted / has_tags are atomics: searches read them without the index mutex.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rass_engine.h"
#include "kernels.h"

namespace rass {
namespace host {

// Stores the calling thread's error text (rass_last_error) and returns `code`.  ONE thread_local object, in api.hip.
int fail(int code, const std::string& msg);

// RASS_OK, or fail() with the failed call, the HIP error's text and the place: HIP_RC(expr) as a value, HIP_TRY(expr)
// returning it from the enclosing function.
int hip_fail(hipError_t e, const char* expr, const char* file, int line);
inline int hip_rc(hipError_t e, const char* expr, const char* file, int line) {
    return e == hipSuccess ? (int)RASS_OK : hip_fail(e, expr, file, line);
}
#define HIP_RC(expr) ::rass::host::hip_rc((expr), #expr, __FILE__, __LINE__)
#define HIP_TRY(expr) do { const int _rc = HIP_RC(expr); if (_rc != RASS_OK) return _rc; } while (0)

constexpr int kPrefilterMaxK = 16;     // prefilter keeps 32 bf16 candidates: only k <= 16 uses it, wider k scans fp32
constexpr int kMaxGrid = 1024;        // upper bound on scan workgroups (sizing of scratch)
constexpr int kMaxStride = 2048;      // dim_padded limit of the fused scan (128 * {1..8}; wide rows: 256 * {5..8})
constexpr int kNarrowStride = 1024;   // above it a row is "wide": flat fp32 scans of <= 16 queries per launch only
constexpr int64_t kStageRows = 8192;  // host -> device staging granule for add()
constexpr int kHostSlots = 8;
constexpr int kMultiMaxItems = 65536;  // 32-row tiles per cross-index batch (2 M rows over all its indices)
constexpr int kIvfMaxLists = 32768;    // lists of one IVF
constexpr int64_t kMaxScanRows = 0x7fffffc0LL;   // rows of one scan / one IVF slab (ivf_build.hip: kSlabLimit)

inline int64_t pad128(int64_t d) { return (d + 127) / 128 * 128; }
// The row stride of an index of `dim` columns: whole 128-column units (8 waves x one 16-column chunk); above 1 024
// columns whole 256-column units (the wide-row scan walks a wave's slice in an even number of chunks per panel).
inline int64_t pad_stride(int64_t d) { return d <= kNarrowStride ? pad128(d) : (d + 255) / 256 * 256; }
constexpr const char* kStrideMsg = "row_stride must be 128*{1..8} elements (dim <= 1024) or 256*{5..8} (dim <= 2048)";
inline int64_t pad512(int64_t d) { return (d + 511) / 512 * 512; }   // bytes per row of an int8 copy (stride_i8)
inline int64_t pad16(int64_t rows) { return (rows + 15) / 16 * 16; }  // rows of a tile16 slab: whole 16-row blocks
inline int pad_nq(int nq) { return nq <= 16 ? 16 : 32; }   // query rows a launch group's kernels read: whole 16-wide MFMA N tiles

int device_cus(int device);   // compute units of a device, asked once per device (one cache, api.hip)

// The shared range checks of a launch group: RASS_OK, or RASS_ERR_INVALID with the message every entry point gives.
int check_nq(int nq);   // [1, RASS_MAX_QBATCH]
int check_k(int k);     // [1, RASS_MAX_K]

// An IVF probe's work list (ScanArgs::work_*); max_tiles sizes the grid, the item count is only known on the device.
struct IvfPlan {
    const int32_t* work_tile;
    const int32_t* work_rows;
    const uint32_t* work_mask;
    const int32_t* n_work;
    int64_t max_tiles;
};
template <class Args>
void set_plan(Args& a, const IvfPlan& p) {
    a.work_tile = p.work_tile;
    a.work_rows = p.work_rows;
    a.work_mask = p.work_mask;
    a.n_work = p.n_work;
}

// What every bf16 / int8 candidate scan adds per launch group to bf16_args / i8_args (declared below): the converted queries,
// the filters (mask: nullptr = exact compare), the per-workgroup lists and nq.
template <class Args>
void set_group(Args& a, const void* q, const int32_t* q_filter, const int32_t* q_filter_mask, float* part_scores, int64_t* part_ids,
               int nq) {
    if constexpr (std::is_same<Args, rass::ScanBf16Args>::value) a.q_bf16 = static_cast<const unsigned short*>(q);
    else a.q_i8 = static_cast<const signed char*>(q);
    a.q_filter = q_filter;
    a.q_filter_mask = q_filter_mask;
    a.part_scores = part_scores;
    a.part_ids = part_ids;
    a.nq = nq;
}

// Extended per-query filters of a scan (kernels.h ScanArgs): all-null = the plain kernel variant.
struct ScanExt {
    const int32_t* d_q_mask = nullptr;
    const float* d_after_s = nullptr;
    const int64_t* d_after_i = nullptr;
    const int32_t* d_live = nullptr;   // device scalar: 0 = every workgroup exits (the certified mode's fallback)
};

// ---- workspace views: typed pointers into a block at `base`; base = nullptr to learn `total` only.  Every area starts on
// a 256-byte boundary.
struct Carver {
    unsigned char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t bytes) {
        T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off);
        off = (off + bytes + 255) / 256 * 256;
        return p;
    }
};

// ---- per-launch-group offsets of a list of `n` records sorted by the query (of `n_queries`) that query_of(i) names: what a
// column builder uploads once for all its launch groups of <= RASS_MAX_QBATCH queries.  Group g's records start at
// group_at[g] (group_at[groups] = n); its nq_g + 1 offsets, rebased to that start, are q_off[group_off[g] ..]: query q of the
// group owns records [q_off[.. + q], q_off[.. + q + 1]).
struct GroupOffsets {
    std::vector<int32_t> q_off;
    std::vector<size_t> group_at, group_off;
};
template <class QueryOf>
GroupOffsets group_offsets(int n_queries, size_t n, QueryOf query_of) {
    const int groups = (n_queries + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    GroupOffsets o;
    o.group_at.assign((size_t)groups + 1, 0), o.group_off.assign((size_t)groups, 0);
    size_t at = 0;
    for (int g = 0; g < groups; ++g) {
        o.group_at[(size_t)g] = at;
        o.group_off[(size_t)g] = o.q_off.size();
        const int q0 = g * RASS_MAX_QBATCH, q1 = std::min(n_queries, q0 + RASS_MAX_QBATCH);
        o.q_off.push_back(0);
        for (int q = q0; q < q1; ++q) {
            while (at < n && query_of(at) == q) ++at;
            o.q_off.push_back((int32_t)(at - o.group_at[(size_t)g]));
        }
    }
    o.group_at[(size_t)groups] = at;
    return o;
}

// The engine scratch of one launch group (and the caller's workspace of rass_scan_topk_f32: rass_scan_workspace_bytes).
struct ScratchView {
    float* q_padded;               // [32][kMaxStride] normalised, zero-padded queries
    float* part_scores;            // [kMaxGrid][nq][k] per-workgroup lists
    int64_t* part_ids;
    unsigned short* q_bf16;        // prefilter mode: bf16 queries (int8 queries live here too: half the bytes)
    float* cand_scores;            // ... and the 32 candidates per query handed to the exact re-rank
    int64_t* cand_ids;
    float* sample_best;            // the sample pass's per-workgroup best scores [32][kMaxSampleGroups]
    size_t total;
};
ScratchView scratch_layout(unsigned char* base, int nq, int k);

// The block of a fused batch (eng->d_batch): every group's queries, lists and sample bests; with `candidates` (the prefilter
// batch) also the converted queries and the merged candidates.
struct BatchView {
    float* q_padded;               // [groups][32][stride]
    float* part_scores;            // [groups] x part_per_group
    int64_t* part_ids;
    float* sample_best;            // [groups][32][kMaxSampleGroups]
    unsigned char* q_small;        // [groups][32] bf16 / int8 queries
    float* cand_scores;            // [groups][32][32]
    int64_t* cand_rows;
    unsigned char* rep_qfrag;      // the fp32 batch's sample stage (sample_rep.hip): [groups][32][stride] bf16 query fragments,
    unsigned char* rep_part;       // [groups][32][kMaxSampleGroups] (score, row) pairs
    int* rep_row;                  // and the representatives [groups][32][32]
    float* step_floor;             // [groups][32]: one sample floor per query, for the step kernel (launch_step_floors)
    size_t total;
    size_t part_per_group;         // elements of one group's [grid][32][k] lists
    float* group_sample(int g) const { return sample_best + (int64_t)g * 32 * rass::kMaxSampleGroups; }
};
BatchView batch_layout(unsigned char* base, int groups, int grid, int k, int64_t stride, bool candidates = false);

// The workspace of the certified int8 search (eng->d_cert): one pass of kCertQ queries.
struct CertView {
    float* q_padded;               // x 4: one copy per re-ranked chunk of 32 candidates
    signed char* q8;
    rass::CertQInfo* qinfo;
    float* sample;
    float* list_s;
    int32_t* list_r;
    int32_t* list_n;
    float* list_floor;
    int64_t* cand_rows;
    float* rr_s;
    int64_t* rr_i;
    float* tau;
    int32_t *fail_idx, *fail_flag, *fail_n;
    float* fb_q;
    int32_t *fb_filter, *fb_mask;
    float* fb_s;
    int64_t* fb_i;
    float* hook_s;                 // the parity hook's own search result
    int64_t* hook_i;
    size_t total;
};
CertView cert_layout(unsigned char* base, int grid, int64_t stride, int64_t stride_i8, int dim);

// A range search's share of the engine scratch (one launch group): the queries where every scan keeps them, one counter line
// per query and the unsorted hits [32][kRangeMaxHits] — about 1.3 MiB of the scratch's 12.
struct RangeView {
    float* q_padded;
    unsigned* count;               // [32][kRangeCountStride]
    uint2* hits;                   // [32][kRangeMaxHits] (score bits, row); a call uses [nq][max_hits]
    size_t total;
};
RangeView range_layout(unsigned char* base);

// The host range search's staging (a view of eng->d_io, and of the slot's h_io): thresholds in, totals and lists out, of one launch group.
struct RangeIoView {
    float* thr;                    // [32]
    int64_t* total;                // [32]
    float* out_scores;             // [32][kRangeMaxHits]; a call uses [nq][max_hits]
    int64_t* out_ids;
    size_t bytes;
};
RangeIoView range_io_layout(unsigned char* base);

// A grouped search's table block (eng->d_group, one launch group): the status word, then one 64-bit slot per (query, group).
// Status and table are adjacent: one memset zeroes both.  Up to 256 MiB, so it is a block of its own, grown on demand.
struct GroupView {
    unsigned* status;              // [1] on a 256-byte line
    unsigned long long* table;     // [nq][n_groups]
    size_t total;
};
GroupView group_layout(unsigned char* base, int nq, int n_groups);

// The host grouped search's staging (eng->d_io / the slot's h_io): totals, status and lists out, of one launch group.
struct GroupIoView {
    int64_t* total;                // [32]
    int32_t* status;               // [1]
    float* out_scores;             // [32][kGroupMaxK]; a call uses [nq][k]
    int64_t* out_ids;
    int32_t* out_groups;
    size_t bytes;
};
GroupIoView group_io_layout(unsigned char* base);

// An aggregation's table block (eng->d_group as well, one launch group): the status word, one 64-bit best-row slot and one
// 32-bit counter per (query, group).  All adjacent: one memset zeroes the three.  Up to 384 MiB.
struct AggView {
    unsigned* status;              // [1] on a 256-byte line
    unsigned long long* best;      // [nq][n_groups]
    unsigned* count;               // [nq][n_groups]
    size_t total;
};
AggView agg_layout(unsigned char* base, int nq, int n_groups);

// The host aggregation's staging (eng->d_io / the slot's h_io): thresholds in,
// per-query figures, status and bucket lists out, of one launch group.
struct AggIoView {
    float* thr;                    // [32]
    int64_t* n_buckets;            // [32]
    int64_t* total_hits;           // [32]
    int32_t* status;               // [1]
    int32_t* out_groups;           // [32][kGroupMaxK]; a call uses [nq][size]
    int64_t* out_counts;
    float* out_scores;
    int64_t* out_ids;
    size_t bytes;
};
AggIoView agg_io_layout(unsigned char* base);

// A grow-on-demand device block (eng->d_batch, eng->d_cert, rass_ivf::d_batch): at least `need` bytes afterwards.  Growth
// waits for the stream first: an earlier call on it may still read the old block.
int grow_block(unsigned char** block, size_t* bytes, size_t need, hipStream_t st);

// One host search call in flight: pinned staging for a batch of <= 32 queries and its results, and
// the event recorded behind the batch's last copy.
struct HostSlot {
    float* h_q = nullptr;          // [32][dim]
    int32_t* h_filter = nullptr;   // [32]
    int32_t* h_mask = nullptr;     // [32]
    float* h_after_s = nullptr;    // [32]
    int64_t* h_after_i = nullptr;  // [32]
    float* h_out_s = nullptr;      // [32][32]
    int64_t* h_out_i = nullptr;    // [32][32]
    int64_t* h_scanned = nullptr;  // [1]
    void* base = nullptr;          // the one hipHostMalloc behind all of the above
    void* h_items = nullptr;       // pinned work list of a cross-index batch (lazily allocated, kMultiMaxItems)
    void* h_io = nullptr;          // pinned image of a Range / Group / AggIoView: the group of the call that owns the slot
    size_t io_bytes = 0;           // (slot_grow_io: grown to the layout that call needs)
    hipEvent_t done = nullptr;
    bool busy = false;
};

}  // namespace host
}  // namespace rass

struct rass_engine {
    int device = 0;
    int dim = 0;
    int n_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::map<std::string, rass_index*> indices;
    // scratch for searches (sized for nq = RASS_MAX_QBATCH, k = RASS_MAX_K)
    unsigned char* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    // scratch of rass_index_search_device_batch (every launch group's queries, lists and sample bests), grown on demand
    unsigned char* d_batch = nullptr;
    size_t batch_bytes = 0;
    // workspace of the certified int8 search (prefilter mode 3): one pass of kCertQ queries, grown on demand
    unsigned char* d_cert = nullptr;
    size_t cert_bytes = 0;
    // device staging of the host range / grouped / aggregation searches (Range / Group / AggIoView), grown to the layout a call
    // needs; used under mu and in stream order, like d_scratch
    unsigned char* d_io = nullptr;
    size_t io_bytes = 0;
    // the table block of the grouped search and the aggregation (GroupView / AggView, grown on demand, up to 384 MiB); used
    // under mu and in stream order
    unsigned char* d_group = nullptr;
    size_t group_bytes = 0;
    // the allow-list search (api_allow.hip): the work list and plan workspace of one launch group (AllowView), and the host
    // entry points' device staging (bitmaps, row / value lists in; lists out); both grown on demand, used under mu in stream order
    unsigned char* d_allow = nullptr;
    size_t allow_bytes = 0;
    unsigned char* d_allow_io = nullptr;
    size_t allow_io_bytes = 0;
    // the diversified (MMR) search and rass_index_rows_gram (api_mmr.hip): the candidates, Gram matrices and staging of one
    // launch group (MmrView, 2.3 MiB), allocated on first use; used under mu in stream order
    unsigned char* d_mmr = nullptr;
    size_t mmr_bytes = 0;
    // host-API staging
    float* d_qraw = nullptr;        // [32][dim]
    int32_t* d_qfilter = nullptr;   // [32]
    float* d_out_scores = nullptr;  // [32][32]
    int64_t* d_out_ids = nullptr;   // [32][32]
    float* d_stage = nullptr;       // [kStageRows][dim]
    int32_t* d_stage_tags = nullptr;
    // cross-index batches (rass_index_search_multi): device work list, lazily allocated
    int32_t *d_mw_tile = nullptr, *d_mw_rows = nullptr, *d_mw_n = nullptr;
    uint32_t* d_mw_mask = nullptr;
    const float** d_mw_base = nullptr;
    const int32_t** d_mw_tags = nullptr;
    float* d_stage_t16 = nullptr;   // bf16 indices: (kStageRows + 32) x kMaxStride fp32 tile16 staging, lazily allocated
    int32_t* d_qmask = nullptr;     // [32] masked-filter masks
    float* d_after_s = nullptr;     // [32] continuation bound of a multi-pass top-k (k > 32)
    int64_t* d_after_i = nullptr;   // [32]
    // pinned host slots of the host search API (one per call in flight)
    std::vector<rass::host::HostSlot> slots;
    std::mutex slot_mu;
    std::condition_variable slot_cv;
    // optional HIP-event bracket around every scan kernel launch (bench.py's roofline leg)
    std::vector<hipEvent_t> ev_pool;  // pairs: [2i] before, [2i+1] after
    int ev_used = 0;                  // pairs recorded since timing_begin
    int ev_extra = 0;                 // launch groups beyond one that recorded launches served (a 64-query pair pass: +1)
    bool ev_on = false;
};

struct rass_index {
    rass_engine* eng = nullptr;
    std::string name;
    rass_dtype dtype = RASS_F32;
    int dim = 0;
    int64_t stride = 0;
    std::atomic<int64_t> rows{0};      // published after the rows' pack kernels are enqueued
    int64_t capacity = 0;
    std::atomic<int64_t> deleted{0};
    std::atomic<bool> has_tags{false};  // any non-zero tag ever stored
    float* d_rows = nullptr;
    int32_t* d_tags = nullptr;
    int64_t* d_gid = nullptr;               // [capacity] id reported for a row: its ordinal, or the caller's
                                            // GLOBAL id (rass_index_add_ex: a shard of a multi-GPU index)
    std::atomic<bool> has_gid{false};       // any row carries a caller-assigned id
    unsigned short* d_rows_bf16 = nullptr;  // tile16b copy for the prefilter mode (nullptr = off)
    int prefilter = 0;                      // 0 off | 1 bf16 candidate copy | 2 int8 candidate copy (+ a scale per row)
    signed char* d_rows_i8 = nullptr;       // tile16i copy (prefilter mode 2), rows of stride_i8 bytes
    float* d_row_scale = nullptr;           // [capacity] max|x| / 127 of every row (prefilter mode 2)
    int64_t stride_i8 = 0;                  // stride rounded up to 512
    // prefilter mode 3 (certified int8 search): [R, V, Y] as float bits (monotone maxima over every row ever quantised) and
    // the counters [queries, certified, fallbacks]; allocated when the mode is first set
    unsigned* d_cert_stats = nullptr;
    unsigned long long* d_cert_counts = nullptr;
    // attribute columns (api_attr.hip): column c is int32 [capacity], nullptr until its first rass_index_set_attr, which
    // fills it with RASS_ATTR_MISSING; every path that moves a row (grow, compact, save / load) carries the allocated ones
    int32_t* d_attr[RASS_MAX_ATTRS] = {};
    std::vector<uint8_t> host_deleted;  // tombstone bitmap mirror (host)
    // compactions that moved rows (rass_index_compact): a row ordinal is only meaningful together with this value.
    // Written under mu + eng->mu; the host search entry points read it around their launch groups
    std::atomic<int64_t> layout_epoch{0};
    std::mutex mu;
};

// ------------------------------------------------------------------------------------ IVF (K9)
struct rass_ivf {
    rass_engine* eng = nullptr;
    int dim = 0, nlist = 0;
    int64_t stride = 0, rows = 0, slab_rows = 0, total_tiles = 0;
    int dtype = RASS_F32;           // RASS_F32: d_slab (tile16, 32-row tiles) | RASS_BF16: d_slab_b16 (tile16b, 64-row tiles)
    int tile_rows = 32;             // rows per plan tile = the fine scan kernel's tile
    float* d_slab = nullptr;        // tile16, lists contiguous, each starting on a 32-row tile
    unsigned short* d_slab_b16 = nullptr;  // bf16 slab: the rows rounded to bf16, lists starting on 64-row tiles
    // RASS_I8: d_slab (fp32, lists on 64-row tiles: read by the exact re-rank only) + its int8 copy (tile16i) and row scales:
    // the fine scan keeps 32 int8 candidates per query, the re-rank rescores them exactly and returns the best k <= 16
    signed char* d_slab_i8 = nullptr;
    float* d_slab_scale = nullptr;
    int64_t stride_i8 = 0;
    float* d_cand_scores = nullptr;        // [32][32] candidates of one launch group (RASS_I8)
    int64_t* d_cand_rows = nullptr;
    int32_t* d_tags = nullptr;      // [slab_rows] permuted row tags (0 on padding)
    int64_t* d_ids = nullptr;       // [slab_rows] source row id, -1 on padding
    float* d_centroids = nullptr;   // tile16 slab of nlist normalised centroids
    int32_t *d_list_tile0 = nullptr, *d_list_len = nullptr;
    int32_t *d_work_tile = nullptr, *d_work_rows = nullptr, *d_n_work = nullptr;
    uint32_t* d_work_mask = nullptr;
    int64_t* d_scanned = nullptr;   // rows touched by the last fine scan
    float* d_probe_scores = nullptr;  // [32][32]
    int64_t* d_probe_ids = nullptr;   // [32][32]
    uint32_t* d_tau = nullptr;        // [32] nprobe > 32: per-query threshold keys
    uint32_t* d_list_mask = nullptr;  // [nlist] nprobe > 32: probe masks from the score matrix
    bool any_tags = false;
    // IVF + flat delta (rass_ivf_search_delta*): the IVF covers source rows [0, src_rows); rows the source index took
    // afterwards are scanned exactly from its own slab and merged with the probe's list
    int64_t src_rows = 0;
    int64_t src_epoch = -1;           // layout epoch of the source index the ids name; -1 (a loaded IVF): adopted from the first source searched
    std::vector<int32_t> pos_of;      // host: slab position of source row r (< src_rows), -1 = not in the slab (tombstoned)
    float* d_pair_scores = nullptr;   // [2][32][32] the probe's list and the delta scan's list of one launch group
    int64_t* d_pair_ids = nullptr;
    unsigned char* d_batch = nullptr; // rass_ivf_search_device_batch: queries, coarse / fine lists and work lists of <= 32 groups
    size_t batch_bytes = 0;
    // the probe within a row bitmap (api_ivf_allow.hip): the slab-order words [32][total_tiles], the compacted work list and
    // the compaction's block counts of one launch group (IvfAllowView); grown on first use, used under eng->mu in stream order
    unsigned char* d_allow_ws = nullptr;
    size_t allow_ws_bytes = 0;
};

namespace rass {
namespace host {

int set_device(const rass_engine* eng);
int index_reserve(rass_index* idx, int64_t need_rows);   // api.hip; the caller holds idx->mu and eng->mu
void index_free_slabs(rass_index* idx);                  // every device array of the index, freed and nulled
int index_attr_ensure(rass_index* idx, int col);         // api.hip; attribute column `col` allocated (all MISSING) if it was not; same locks
int index_refresh_copies(rass_index* idx, int64_t first, int64_t n, hipStream_t st);   // the prefilter mode's candidate copies of rows [first, first + n)

// ---- the tuning switches (api_scan.hip: the only place of the host layer that reads the environment)
int scan_xcd_skew(int nq, int grid, int n_cus);   // ScanArgs::xcd_skew of a launch; RASS_SCAN_XCD_SKEW, read once
int64_t scan_sample_floor_min_share();            // RASS_SCAN_SAMPLE_FLOOR, read per call
bool i8_sample_floor(int64_t rows, int grid);     // RASS_I8_SAMPLE_FLOOR, read per call
enum { kBatchSampleGroups = 0, kBatchSampleF32 = 1, kBatchSampleRep = 2 };
int scan_batch_sample_mode();                   // RASS_SCAN_BATCH_SAMPLE, read per call: a kBatchSample* value
bool scan_batch_pair();                           // RASS_SCAN_BATCH_PAIR, read once
bool scan_batch_step();                           // RASS_SCAN_BATCH_STEP, read per call
bool ivf_batch_one_launch();                      // RASS_IVF_BATCH_FINE, read per call

// Workgroups of a scan over `tiles` tiles whose merge takes `lists_kept_per_wg` entries per query from each of them: one per
// CU, at most kMaxGrid, and no more lists than one merge launch takes (kMergeMaxCandidates).  (The certified scan sizes its
// own grid: its selection kernel takes kMaxGridSel slices.)
int scan_grid(int64_t tiles, int lists_kept_per_wg, int n_cus);

// The optional event bracket of rass_engine_kernel_timing_*: records the before / after events around `launch` (which
// returns a status: HIP_RC of the launcher's) and counts it; extra_groups = launch groups beyond one that it served (a pair pass: 1;
// a step-kernel launch over `pairs` pairs: 2 * pairs - 1).
// eng = nullptr: no bracket.
template <class F>
int timed_launch(rass_engine* eng, hipStream_t st, F&& launch, int extra_groups = 0) {
    const bool timed = eng && eng->ev_on && (size_t)(2 * eng->ev_used + 1) < eng->ev_pool.size();
    if (timed) HIP_TRY(hipEventRecord(eng->ev_pool[2 * eng->ev_used], st));
    const int rc = launch();
    if (rc != RASS_OK) return rc;
    if (timed) {
        HIP_TRY(hipEventRecord(eng->ev_pool[2 * eng->ev_used + 1], st));
        eng->ev_used += 1;
        eng->ev_extra += extra_groups;   // kernel_timing_end counts launch GROUPS
    }
    return RASS_OK;
}

// The sample pre-launch of a scan (ScanArgs / ScanBf16Args / ScanI8Args ::sample_best): the launch `a` describes, over the
// slab's first 64 * grid rows only, keeping each workgroup's best score per query in `best`; `a` then takes the k-th
// largest of those as its floor.  The int8 and bf16 kernels sample with k = 1, the fp32 kernel as its own variant.
// launch_grid (a grouped sample: `a` carries wgs_per_group and the group strides): workgroups of the sample launch.
inline void as_sample(rass::ScanArgs& s) { s.xcd_skew = 0, s.sample_pass = true; }
inline void as_sample(rass::ScanBf16Args& s) { s.k = 1; }
inline void as_sample(rass::ScanI8Args& s) { s.k = 1; }
template <class Args>
int sample_prelaunch(Args& a, int grid, float* best, hipError_t (*launch)(const Args&, int, hipStream_t), hipStream_t st,
                     int launch_grid = 0) {
    Args s = a;   // same queries, filters, continuation bound and id space: only the row count differs
    s.n_rows = 64 * grid;
    as_sample(s);
    s.part_scores = best;
    s.part_ids = nullptr;
    HIP_TRY(launch(s, launch_grid ? launch_grid : grid, st));
    a.sample_best = best;
    a.sample_groups = grid;
    return RASS_OK;
}

// What one search call reads of a flat index, taken once (the atomics without the index mutex, in this order).
// (The bf16, prefilter and certified launch paths read the row count again themselves, as before: it only grows.)
struct IndexView {
    int64_t rows;
    const int32_t* row_tag;   // the tags where some row is deleted or the call filters, else nullptr
    const int64_t* id_map;    // the caller-assigned ids where any row has one, else nullptr
    int64_t id_base;          // 0 under an id map or a continuation bound (which names ROWS): ids are translated in the merge
    const float* corpus;      // the fp32 slab; an empty index scans zero rows of the engine scratch
};
IndexView index_view(const rass_index* idx, bool filtered, int64_t id_base = 0, bool continued = false);

// The fields a bf16 / int8 candidate scan takes from its corpus — a flat index, or an IVF slab.  The caller adds what
// differs per launch: queries, filters, lists, nq (and the work list of a probe).
rass::ScanBf16Args bf16_args(const rass_index* idx, int64_t rows, const int32_t* row_tag, int k);
rass::ScanBf16Args bf16_args(const rass_ivf* v, const int32_t* row_tag, int k);
rass::ScanI8Args i8_args(const rass_index* idx, int64_t rows, const int32_t* row_tag, int k);
rass::ScanI8Args i8_args(const rass_ivf* v, const int32_t* row_tag, int k);

// The grouped merge of a fused batch: dense per-workgroup lists of `part_per_group` elements per group.
rass::MergeGroups dense_groups(int nq_total, int64_t part_per_group, int64_t out_score_stride, int64_t out_id_stride);

// ---- the flat launch paths (api_scan.hip).  The caller holds eng->mu and has set the device.
// The exact fp32 scan of one launch group: normalise -> (sample) -> scan -> merge.  Stateless: any slab, any workspace.
struct ScanRequest {
    const float* corpus = nullptr;     // tile16 slab, 16-byte aligned
    int64_t n_rows = 0;
    int64_t stride = 0;
    const int32_t* row_tag = nullptr;
    const float* queries = nullptr;    // [nq] rows of q_dim columns, q_stride apart
    int q_dim = 0;
    int64_t q_stride = 0;
    int nq = 0;
    const int32_t* q_filter = nullptr;
    int k = 0;
    int64_t id_base = 0;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    unsigned char* ws = nullptr;       // scratch_layout(nq, k)
    size_t ws_bytes = 0;
    int n_cus = 0;
    hipStream_t st = nullptr;
    rass_engine* timing = nullptr;     // the engine whose kernel timing counts this scan, if any
    const IvfPlan* plan = nullptr;     // the fine scan of a probe
    const int64_t* id_map = nullptr;   // id reported for row r, instead of id_base + r
    ScanExt ext;
    bool queries_prepared = false;     // see scan_launch
};
ScanRequest scan_request(rass_engine* eng);   // on the engine's scratch and stream (timing stays off)
int scan_launch(const ScanRequest& r);

// One launch group on a flat index, for the three paths that need the index: the bf16 corpus, the prefilter modes 1 / 2
// and the certified mode 3.
struct FlatRequest {
    const float* queries = nullptr;    // [nq][dim]
    int nq = 0;
    int k = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;   // masked tag compare ((tag & mask) == filter)
    const float* after_score = nullptr;       // continuation bound of a k > 32 pass (bf16 corpus and fp32 scan only)
    const int64_t* after_row = nullptr;
    float* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    const int32_t* row_tag = nullptr;         // from the call's IndexView
    const int64_t* id_map = nullptr;          // ascending with the row: the tie order is unchanged
    int64_t id_base = 0;
    // optional extra outputs (the candidates hooks): the merged candidate lists [nq][32] (modes 1 / 2) or [nq][128] with
    // tau [nq] and the certificate flags [nq] (mode 3)
    float* cand_scores = nullptr;
    int64_t* cand_rows = nullptr;
    float* tau = nullptr;
    int32_t* certified = nullptr;
    void use(const IndexView& iv) { row_tag = iv.row_tag, id_map = iv.id_map, id_base = iv.id_base; }
};
int bf16_scan_launch(rass_index* idx, const FlatRequest& r);
int prefilter_launch(rass_index* idx, const FlatRequest& r);
int cert_launch(rass_index* idx, const FlatRequest& r);

// One layout per answer.  The host search entry points release eng->mu between launch groups and between the passes of a
// k > 32 search, and a pass's continuation bound names a row ORDINAL: a compaction (rass_index_compact) landing in between
// would mix two layouts in one answer.  They read the layout epoch(s) first and run again when it moved meanwhile — bounded:
// a compaction is rare and takes far longer than a search.
constexpr int kLayoutAttempts = 8;
template <class Epoch, class Once>
int one_layout(Epoch&& epoch, Once&& once) {
    for (int attempt = 0; attempt < kLayoutAttempts; ++attempt) {
        const int64_t before = epoch();
        const int rc = once();
        if (rc != RASS_OK || epoch() == before) return rc;
    }
    return fail(RASS_ERR_UNSUPPORTED, "the index was compacted during every attempt of this search: try again");
}

// A pinned host slot for one search call in flight (blocks while all kHostSlots are taken); api_search.hip.
HostSlot* slot_acquire(rass_engine* eng);
void slot_release(rass_engine* eng, HostSlot* sl);
struct SlotGuard {
    rass_engine* eng;
    HostSlot* sl;
    SlotGuard(rass_engine* e) : eng(e), sl(slot_acquire(e)) {}
    ~SlotGuard() { slot_release(eng, sl); }
};
// The host API's round trip of one launch group through the slot `sl`: the caller's queries (and filters / masks, where
// given) to the slot and on to the engine's device staging; the group's k results per query (and a probe's scanned rows)
// back to the slot.  The caller holds eng->mu for both enqueues and records the slot's event behind them (host_groups does).
void slot_fill(HostSlot* sl, int dim, const float* queries, const int32_t* q_filter, const int32_t* q_filter_mask, int b);
int slot_upload(rass_engine* eng, HostSlot* sl, int dim, bool filter, bool mask, int b);
int slot_download(rass_engine* eng, HostSlot* sl, int b, int k, const int64_t* d_scanned = nullptr);
// The slot's pinned staging block (h_io) at least `need` bytes.  Only the call that owns the slot touches the block; growth
// waits for the slot's event first, so the block it frees has no copy in flight.
int slot_grow_io(HostSlot* sl, size_t need);

// One attempt of a host search that goes group by group (<= 32 queries) through a pinned slot; one_layout runs it again when
// a compaction landed meanwhile.  Per group: the queries (filters, masks) to the slot and `fill(sl, done, b)` (what else the
// group uploads from the slot's h_io), then under eng->mu -- held while ENQUEUING only: device staging and scratch are shared
// by stream order -- their upload, `enqueue(sl, done, b)` (the group's own uploads, its device search, its downloads) and the
// slot's event; the wait happens on that event without the lock, and `collect(sl, done, b)` hands the group's answer to the
// caller.  io_bytes > 0: the slot's h_io holds at least that many bytes from the first `fill` on, eng->d_io when `enqueue`
// runs (0: neither block is touched).  The slot is released on return.  The (engine, dim) form serves a search that has no
// flat index of its own (the IVF); the index form forwards to it.
inline void no_fill(HostSlot*, int, int) {}
template <class Fill, class Enqueue, class Collect>
int host_groups(rass_engine* eng, int dim, const float* queries, int nq, const int32_t* q_filter, const int32_t* q_filter_mask,
                size_t io_bytes, Fill&& fill, Enqueue&& enqueue, Collect&& collect) {
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    SlotGuard guard(eng);
    HostSlot* sl = guard.sl;
    if ((rc = slot_grow_io(sl, io_bytes)) != RASS_OK) return rc;
    for (int done = 0; done < nq;) {
        const int b = std::min(RASS_MAX_QBATCH, nq - done);
        slot_fill(sl, dim, queries + (int64_t)done * dim, q_filter ? q_filter + done : nullptr,
                  q_filter_mask ? q_filter_mask + done : nullptr, b);
        fill(sl, done, b);
        {
            std::lock_guard<std::mutex> lk(eng->mu);
            if ((rc = grow_block(&eng->d_io, &eng->io_bytes, io_bytes, eng->stream)) != RASS_OK) return rc;
            if ((rc = slot_upload(eng, sl, dim, q_filter != nullptr, q_filter_mask != nullptr, b)) != RASS_OK) return rc;
            if ((rc = enqueue(sl, done, b)) != RASS_OK) return rc;
            HIP_TRY(hipEventRecord(sl->done, eng->stream));
        }
        HIP_TRY(hipEventSynchronize(sl->done));
        if ((rc = collect(sl, done, b)) != RASS_OK) return rc;
        done += b;
    }
    return RASS_OK;
}
template <class Fill, class Enqueue, class Collect>
int host_groups(rass_index* idx, const float* queries, int nq, const int32_t* q_filter, const int32_t* q_filter_mask, size_t io_bytes,
                Fill&& fill, Enqueue&& enqueue, Collect&& collect) {
    return host_groups(idx->eng, idx->dim, queries, nq, q_filter, q_filter_mask, io_bytes, fill, enqueue, collect);
}

// One attempt of rass_index_search_ex (api_search.hip).  exact = true: every pass on the exact fp32 scan, whatever the index's
// prefilter mode (the overflow fallback of the range search, whose answer may not depend on a candidate scan).
int search_ex_once(rass_index* idx, const float* queries, int nq, int k, const int32_t* q_filter, const int32_t* q_filter_mask,
                   float* out_scores, int64_t* out_ids, bool exact = false);

// ---- what the probe within a row bitmap (api_ivf_allow.hip) shares with api_allow.hip and api_ivf.hip
// The work list of one launch group of an allowed search and the plan's workspace (eng->d_allow), sized by the rows scanned.
struct AllowView {
    int32_t* work_tile;
    int32_t* work_rows;
    uint32_t* work_mask;
    int32_t* n_work;
    unsigned char* plan_ws;
    size_t total;
};
AllowView allow_layout(unsigned char* base, int64_t rows);
int check_words(int64_t rows, int64_t words);   // RASS_ERR_INVALID where words < ceil(rows / 32)
// The engine's table block (eng->d_group) at least `need` bytes (api_emit.hip): allocated before the old block is let go, so
// RASS_ERR_OOM leaves the engine as it was; `who` names the search in the message.
int grow_group_table(rass_engine* eng, size_t need, hipStream_t st, const char* who);
// One launch group (<= 32 queries) of a boosted or a function-score search (api_boost.hip): normalise -> per pass of <= 32
// hits: the scan over every tile, merge, store (which also leaves the next pass's continuation bound, on the fused score).
// combine < 0: the boosted scan (scan_boost.hip), rows at or past bonus_rows read 0.  combine = RASS_COMBINE_*: the
// function-score scan (scan_fscore.hip) with that mode and the gate min_score ([nq] or nullptr); bonus_rows must then equal the
// index's rows at the call (RASS_ERR_INVALID otherwise).  Everything is a device pointer; the caller holds eng->mu, has set
// the device and has checked the arguments that do not depend on the row count.
struct BoostRequest {
    const float* queries = nullptr;     // [nq][dim]
    int nq = 0;
    int k = 0;
    const float* boost = nullptr;       // [nq] or nullptr
    int transform = 0;
    const float* bonus = nullptr;       // query q's column at bonus + q * q_stride
    int64_t q_stride = 0;               // 0: one column shared by every query
    int64_t bonus_rows = 0;
    const int32_t* q_filter = nullptr;
    const int32_t* q_filter_mask = nullptr;
    int64_t id_base = 0;
    float* out_scores = nullptr;        // [nq][k]
    int64_t* out_ids = nullptr;
    int combine = -1;
    const float* min_score = nullptr;   // [nq] or nullptr (function-score scan only)
};
int boost_device_group(rass_index* idx, const BoostRequest& r);
// The whole of rass_index_search_boosted / _scored (host pointers; checks boost and min_score, retries on a layout change) and
// of their _device forms (takes eng->mu): `c` describes the CALL — nq <= RASS_MAX_DEVICE_BATCH queries, c.bonus the block of
// n_cols columns (1: shared, or nq) of col_stride floats, q_stride not read — and is cut into launch groups for
// boost_device_group.  scored: the function-score search (c.combine is checked and the messages name fn_*), else the boosted
// one (c.combine stays < 0).
int boost_search_host(rass_index* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored);
int boost_search_device(rass_index* idx, const BoostRequest& c, int n_cols, int64_t col_stride, bool scored);
// The first two stages of a probe of one launch group (api_ivf.hip; the caller holds eng->mu): the top-nprobe centroids per
// query — the flat fused scan for nprobe <= RASS_MAX_K (the lists, best first, stay at v->d_probe_ids [nq][min(nprobe, nlist)]),
// the threshold path above — and the plan: the union of the probed lists as the work list v->d_work_* / d_n_work with per-tile
// query masks, its rows in *v->d_scanned.  Leaves the group's normalised queries, zero-padded to pad_nq(nq) rows, at the head
// of the engine scratch.  plan = false (nprobe <= RASS_MAX_K only): the coarse stage alone.
int ivf_coarse_plan_locked(rass_ivf* v, const float* d_queries, int nq, int nprobe, bool plan = true);

}  // namespace host
}  // namespace rass
