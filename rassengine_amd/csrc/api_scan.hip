// api_scan.hip — the launch layer of the flat search: the tuning switches, the building blocks every launch path shares
// (grid sizing, workspace views, the grow-on-demand block, the index snapshot, the argument builders; declared in
// api_internal.h) and the four paths of one launch group: the exact fp32 scan, the bf16 corpus, the bf16 / int8
// prefilter and the certified int8 search.  Host-side C++ only: each path enqueues kernels of the other .hip files.
// Who calls them: api_search.hip (flat entry points), api_ivf.hip (coarse / fine scans), api.hip (the stateless scan).

#include "api_internal.h"

namespace rass {
namespace host {

// ---- the tuning switches.  Every environment variable the host layer reads is read here; "read once" ones are fixed
// at their first use in the process, "read per call" ones can be flipped between calls (the tests do).

// XCD skew of the scan's tile order (kernels.h ScanArgs::xcd_skew; measured in
// scripts/microbench/scan_tail.hip and with bench.py).  RASS_SCAN_XCD_SKEW="a" or "a,b" overrides
// the defaults for query batches <= 16 / > 16 (0 = plain round-robin).  Read once.
int scan_xcd_skew(int nq, int grid, int n_cus) {
    struct Skew {
        int b16 = 4, b32 = 0;  // bench.py sweeps: B<=16 603 -> 582 us at skew 4; no gain at B=32 (MFMA/power-bound)
        Skew() {
            if (const char* e = getenv("RASS_SCAN_XCD_SKEW")) {
                int a = 0, b = 0;
                const int n = sscanf(e, "%d,%d", &a, &b);
                if (n == 1) b = a;
                if (n >= 1 && a >= 0 && b >= 0 && a <= 4096 && b <= 4096) b16 = a, b32 = b;
            }
        }
    };
    // one workgroup per CU on every XCD: only then does blockIdx parity = XCD parity
    if (grid != n_cus || grid % 8 != 0) return 0;
    static const Skew skew;  // C++11: initialised once, thread-safe
    return nq <= 16 ? skew.b16 : skew.b32;
}

// The sample floor (ScanArgs::sample_best): before a large flat scan with more than 16 queries, the first tile pair of
// every workgroup (64 * grid rows, 16,384 on MI355X) is scanned on its own, keeping only each workgroup's best score
// per query, and the k-th largest of those becomes the big scan's floor: k different rows reach it, so the final
// k-th best does too.  A row of the slab ranks above that floor with probability ~k / 16,384, so a 1M-row scan feeds
// ~600 candidates per query to the sorted insertion instead of ~18,000 (256 lists x ~70), for one short extra launch
// (the sample scan, which does no sorted insertion; the selection runs in the big scan's prologue).  Only worth it where the insertion is on the critical path: with <= 16 queries the scan
// is HBM-bound and the ranking hides under the loads.  RASS_SCAN_SAMPLE_FLOOR=0 switches it off and =force lowers
// the size threshold to twice the sample (A/B and tests; results are identical either way).  Read per call, so
// that one process can compare the settings.
int64_t scan_sample_floor_min_share() {  // the slab must hold at least this many samples; 0 = never sample
    const char* e = getenv("RASS_SCAN_SAMPLE_FLOOR");
    if (e && e[0] == '0') return 0;
    if (e && e[0] == 'f') return 2;
    return 32;
}

// The sample floor of the int8 and bf16 scans (scan_i8.hip, scan_bf16.hip): worth a short extra launch when the slab is many samples long.
// RASS_I8_SAMPLE_FLOOR=0 turns it off and =force lowers the size rule from eight samples to two, as RASS_SCAN_SAMPLE_FLOOR=force
// does for the fp32 scan (the A/B and the tests; results do not depend on it).  Read per call, so that one process can compare
// the settings: tests/test_gpu_lowprec_floor.py checks 0 / force / default against the CPU oracle and against each other.
bool i8_sample_floor(int64_t rows, int grid) {
    const char* e = getenv("RASS_I8_SAMPLE_FLOOR");
    const bool force = e && e[0] == 'f';
    if (e && !force && atoi(e) == 0) return false;
    return grid <= rass::kMaxSampleGroups && rows >= (int64_t)(force ? 2 : 8) * 64 * grid;
}

// How the fused fp32 batch samples.  Default: representatives chosen by bf16 MFMAs and scored exactly (sample_rep.hip);
// RASS_SCAN_BATCH_SAMPLE=f32: the one-launch fp32 sample pass (kFlatSampleGroups) it replaced; =groups: group by group (the
// A/Bs; results do not depend on it).  Read per call.
int scan_batch_sample_mode() {
    const char* e = getenv("RASS_SCAN_BATCH_SAMPLE");
    if (e && e[0] == 'g') return kBatchSampleGroups;
    if (e && e[0] == 'f') return kBatchSampleF32;
    return kBatchSampleRep;
}

// RASS_SCAN_BATCH_PAIR=0: the fused fp32 batch launches one scan per group instead of one per two full groups (the A/B).  Read once.
bool scan_batch_pair() {
    static const bool on = [] {
        const char* e = getenv("RASS_SCAN_BATCH_PAIR");
        return !(e && e[0] == '0');
    }();
    return on;
}

// RASS_SCAN_BATCH_STEP=0: the fused fp32 batch launches one scan per pair of full groups instead of one per run of up to
// kStepMaxPairs pairs (scan_step.hip; the A/B and the tests' reference; results do not depend on it).  Read per call.
bool scan_batch_step() {
    const char* e = getenv("RASS_SCAN_BATCH_STEP");
    return !(e && e[0] == '0');
}

// RASS_IVF_BATCH_FINE=groups: one fine-scan launch per group (the A/B of kIvfGroups); default: one launch for all groups.  Read per call.
bool ivf_batch_one_launch() {
    const char* e = getenv("RASS_IVF_BATCH_FINE");
    return !(e && e[0] == 'g');
}

// ---- shared building blocks

int scan_grid(int64_t tiles, int lists_kept_per_wg, int n_cus) {
    int grid = (int)std::min<int64_t>(std::max<int64_t>(tiles, 1), std::min(n_cus, kMaxGrid));
    if ((int64_t)grid * lists_kept_per_wg > rass::kMergeMaxCandidates) grid = rass::kMergeMaxCandidates / lists_kept_per_wg;
    return grid;
}

ScratchView scratch_layout(unsigned char* base, int nq, int k) {
    Carver c{base};
    ScratchView L;
    L.q_padded = c.take<float>((size_t)RASS_MAX_QBATCH * kMaxStride * sizeof(float));
    L.part_scores = c.take<float>((size_t)kMaxGrid * nq * k * sizeof(float));
    L.part_ids = c.take<int64_t>((size_t)kMaxGrid * nq * k * sizeof(int64_t));
    L.q_bf16 = c.take<unsigned short>((size_t)RASS_MAX_QBATCH * kMaxStride * 2);
    L.cand_scores = c.take<float>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(float));
    L.cand_ids = c.take<int64_t>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(int64_t));
    L.sample_best = c.take<float>((size_t)rass::kMaxSampleGroups * 32 * sizeof(float));
    L.total = c.off;
    return L;
}

BatchView batch_layout(unsigned char* base, int groups, int grid, int k, int64_t stride, bool candidates) {
    Carver c{base};
    BatchView L;
    L.part_per_group = (size_t)grid * 32 * k;
    L.q_padded = c.take<float>((size_t)groups * 32 * stride * sizeof(float));
    L.part_scores = c.take<float>((size_t)groups * L.part_per_group * sizeof(float));
    L.part_ids = c.take<int64_t>((size_t)groups * L.part_per_group * sizeof(int64_t));
    L.sample_best = c.take<float>((size_t)groups * 32 * rass::kMaxSampleGroups * sizeof(float));
    L.q_small = candidates ? c.take<unsigned char>((size_t)groups * 32 * kMaxStride * 2) : nullptr;
    L.cand_scores = candidates ? c.take<float>((size_t)groups * 32 * k * sizeof(float)) : nullptr;
    L.cand_rows = candidates ? c.take<int64_t>((size_t)groups * 32 * k * sizeof(int64_t)) : nullptr;
    L.rep_qfrag = candidates ? nullptr : c.take<unsigned char>((size_t)groups * 32 * stride * 2);
    L.rep_part = candidates ? nullptr : c.take<unsigned char>((size_t)groups * 32 * rass::kMaxSampleGroups * 8);
    L.rep_row = candidates ? nullptr : c.take<int>((size_t)groups * 32 * 32 * sizeof(int));
    L.step_floor = candidates ? nullptr : c.take<float>((size_t)groups * 32 * sizeof(float));
    L.total = c.off;
    return L;
}

CertView cert_layout(unsigned char* base, int grid, int64_t stride, int64_t stride_i8, int dim) {
    Carver c{base};
    CertView L;
    const size_t Q = rass::kCertQ, slots = (size_t)grid * Q * rass::kCertWgCap;
    L.q_padded = c.take<float>(4 * Q * stride * sizeof(float));
    L.q8 = c.take<signed char>(2 * Q * stride_i8);
    L.qinfo = c.take<rass::CertQInfo>(Q * sizeof(rass::CertQInfo));
    L.sample = c.take<float>((size_t)rass::kMaxSampleGroups * Q * sizeof(float));
    L.list_s = c.take<float>(slots * sizeof(float));
    L.list_r = c.take<int32_t>(slots * sizeof(int32_t));
    L.list_n = c.take<int32_t>((size_t)grid * Q * sizeof(int32_t));
    L.list_floor = c.take<float>((size_t)grid * Q * sizeof(float));
    L.cand_rows = c.take<int64_t>(Q * rass::kCertC * sizeof(int64_t));
    L.rr_s = c.take<float>(Q * rass::kCertC * sizeof(float));
    L.rr_i = c.take<int64_t>(Q * rass::kCertC * sizeof(int64_t));
    L.tau = c.take<float>(Q * sizeof(float));
    L.fail_idx = c.take<int32_t>(Q * sizeof(int32_t));
    L.fail_flag = c.take<int32_t>(Q * sizeof(int32_t));
    L.fail_n = c.take<int32_t>(sizeof(int32_t));
    L.fb_q = c.take<float>(Q * dim * sizeof(float));
    L.fb_filter = c.take<int32_t>(Q * sizeof(int32_t));
    L.fb_mask = c.take<int32_t>(Q * sizeof(int32_t));
    L.fb_s = c.take<float>(Q * RASS_MAX_K * sizeof(float));
    L.fb_i = c.take<int64_t>(Q * RASS_MAX_K * sizeof(int64_t));
    L.hook_s = c.take<float>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(float));
    L.hook_i = c.take<int64_t>((size_t)RASS_MAX_QBATCH * RASS_MAX_K * sizeof(int64_t));
    L.total = c.off;
    return L;
}

RangeView range_layout(unsigned char* base) {
    Carver c{base};
    RangeView L;
    L.q_padded = c.take<float>((size_t)RASS_MAX_QBATCH * kMaxStride * sizeof(float));   // = ScratchView::q_padded
    L.count = c.take<unsigned>((size_t)RASS_MAX_QBATCH * rass::kRangeCountStride * sizeof(unsigned));
    L.hits = c.take<uint2>((size_t)RASS_MAX_QBATCH * rass::kRangeMaxHits * sizeof(uint2));
    L.total = c.off;
    return L;
}

RangeIoView range_io_layout(unsigned char* base) {
    Carver c{base};
    RangeIoView L;
    L.thr = c.take<float>(RASS_MAX_QBATCH * sizeof(float));
    L.total = c.take<int64_t>(RASS_MAX_QBATCH * sizeof(int64_t));
    L.out_scores = c.take<float>((size_t)RASS_MAX_QBATCH * rass::kRangeMaxHits * sizeof(float));
    L.out_ids = c.take<int64_t>((size_t)RASS_MAX_QBATCH * rass::kRangeMaxHits * sizeof(int64_t));
    L.bytes = c.off;
    return L;
}

GroupView group_layout(unsigned char* base, int nq, int n_groups) {
    Carver c{base};
    GroupView L;
    L.status = c.take<unsigned>(sizeof(unsigned));
    L.table = c.take<unsigned long long>((size_t)nq * n_groups * sizeof(unsigned long long));
    L.total = c.off;
    return L;
}

GroupIoView group_io_layout(unsigned char* base) {
    Carver c{base};
    GroupIoView L;
    L.total = c.take<int64_t>(RASS_MAX_QBATCH * sizeof(int64_t));
    L.status = c.take<int32_t>(sizeof(int32_t));
    L.out_scores = c.take<float>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(float));
    L.out_ids = c.take<int64_t>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(int64_t));
    L.out_groups = c.take<int32_t>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(int32_t));
    L.bytes = c.off;
    return L;
}

AggView agg_layout(unsigned char* base, int nq, int n_groups) {
    Carver c{base};
    AggView L;
    L.status = c.take<unsigned>(sizeof(unsigned));
    L.best = c.take<unsigned long long>((size_t)nq * n_groups * sizeof(unsigned long long));
    L.count = c.take<unsigned>((size_t)nq * n_groups * sizeof(unsigned));
    L.total = c.off;
    return L;
}

AggIoView agg_io_layout(unsigned char* base) {
    Carver c{base};
    AggIoView L;
    L.thr = c.take<float>(RASS_MAX_QBATCH * sizeof(float));
    L.n_buckets = c.take<int64_t>(RASS_MAX_QBATCH * sizeof(int64_t));
    L.total_hits = c.take<int64_t>(RASS_MAX_QBATCH * sizeof(int64_t));
    L.status = c.take<int32_t>(sizeof(int32_t));
    L.out_groups = c.take<int32_t>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(int32_t));
    L.out_counts = c.take<int64_t>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(int64_t));
    L.out_scores = c.take<float>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(float));
    L.out_ids = c.take<int64_t>((size_t)RASS_MAX_QBATCH * rass::kGroupMaxK * sizeof(int64_t));
    L.bytes = c.off;
    return L;
}

int grow_block(unsigned char** block, size_t* bytes, size_t need, hipStream_t st) {
    if (*bytes >= need) return RASS_OK;
    HIP_TRY(hipStreamSynchronize(st));   // growth only: the block may still be read by an earlier call
    if (*block) HIP_TRY(hipFree(*block));
    *block = nullptr;
    *bytes = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(block), need));
    *bytes = need;
    return RASS_OK;
}

IndexView index_view(const rass_index* idx, bool filtered, int64_t id_base, bool continued) {
    IndexView iv;
    iv.rows = idx->rows.load(std::memory_order_acquire);
    const bool need_tags = (idx->deleted.load(std::memory_order_acquire) > 0) || filtered;
    const bool gid = idx->has_gid.load(std::memory_order_acquire);  // caller-assigned ids: reported instead of id_base + row
    iv.row_tag = need_tags ? idx->d_tags : nullptr;
    iv.id_map = gid ? idx->d_gid : nullptr;
    iv.id_base = (gid || continued) ? 0 : id_base;
    iv.corpus = idx->d_rows ? idx->d_rows : reinterpret_cast<const float*>(idx->eng->d_scratch);
    return iv;
}

rass::ScanBf16Args bf16_args(const rass_index* idx, int64_t rows, const int32_t* row_tag, int k) {
    rass::ScanBf16Args a{};
    a.corpus = idx->d_rows_bf16 ? idx->d_rows_bf16 : reinterpret_cast<const unsigned short*>(idx->eng->d_scratch);
    a.row_tag = row_tag;
    a.row_stride = idx->stride;
    a.n_rows = (int)rows;
    a.k = k;
    return a;
}

rass::ScanBf16Args bf16_args(const rass_ivf* v, const int32_t* row_tag, int k) {
    rass::ScanBf16Args a{};
    a.corpus = v->d_slab_b16;
    a.row_tag = row_tag;
    a.row_stride = v->stride;
    a.n_rows = (int)v->slab_rows;
    a.k = k;
    return a;
}

rass::ScanI8Args i8_args(const rass_index* idx, int64_t rows, const int32_t* row_tag, int k) {
    rass::ScanI8Args a{};
    a.corpus = idx->d_rows_i8;
    a.row_scale = idx->d_row_scale;
    a.row_tag = row_tag;
    a.row_stride = idx->stride_i8;
    a.n_rows = (int)rows;
    a.k = k;
    return a;
}

rass::ScanI8Args i8_args(const rass_ivf* v, const int32_t* row_tag, int k) {
    rass::ScanI8Args a{};
    a.corpus = v->d_slab_i8;
    a.row_scale = v->d_slab_scale;
    a.row_tag = row_tag;
    a.row_stride = v->stride_i8;
    a.n_rows = (int)v->slab_rows;
    a.k = k;
    return a;
}

rass::MergeGroups dense_groups(int nq_total, int64_t part_per_group, int64_t out_score_stride, int64_t out_id_stride) {
    rass::MergeGroups mg;
    mg.size = RASS_MAX_QBATCH, mg.nq_total = nq_total, mg.lists_are_dense = true;
    mg.score_stride = mg.id_stride = part_per_group;
    mg.out_score_stride = out_score_stride, mg.out_id_stride = out_id_stride;
    return mg;
}

ScanRequest scan_request(rass_engine* eng) {
    ScanRequest r;
    r.ws = eng->d_scratch, r.ws_bytes = eng->scratch_bytes, r.n_cus = eng->n_cus, r.st = eng->stream;
    return r;
}

// ---- the exact fp32 scan
int scan_launch(const ScanRequest& r) {
    const int nq = r.nq, k = r.k;
    const int64_t stride = r.stride;
    hipStream_t st = r.st;
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_k(k)) return rc;
    if (r.n_rows < 0 || r.n_rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (!rass::scan_supported_stride(stride) || stride > kMaxStride)
        return fail(RASS_ERR_UNSUPPORTED, kStrideMsg);
    if (r.q_dim > stride) return fail(RASS_ERR_INVALID, "dim exceeds row_stride");
    if (stride > kNarrowStride) {
        if (r.plan) return fail(RASS_ERR_UNSUPPORTED, "IVF needs dim <= 1024");
        if (nq > 16) {
            // the wide-row kernel answers 16 queries per launch (its query fragments fill the registers): two launches,
            // one after the other on the stream (they share the workspace)
            ScanRequest lo = r, hi = r;
            lo.nq = 16;
            hi.nq = nq - 16;
            hi.queries = r.queries + 16 * r.q_stride;
            hi.q_filter = r.q_filter ? r.q_filter + 16 : nullptr;
            hi.out_scores = r.out_scores + (int64_t)16 * k;
            hi.out_ids = r.out_ids + (int64_t)16 * k;
            hi.ext = ScanExt();
            hi.ext.d_q_mask = r.ext.d_q_mask ? r.ext.d_q_mask + 16 : nullptr;
            hi.ext.d_after_s = r.ext.d_after_s ? r.ext.d_after_s + 16 : nullptr;
            hi.ext.d_after_i = r.ext.d_after_i ? r.ext.d_after_i + 16 : nullptr;
            const int rc = scan_launch(lo);
            if (rc != RASS_OK) return rc;
            return scan_launch(hi);
        }
    }
    if (r.ws == nullptr || r.ws_bytes < scratch_layout(nullptr, nq, k).total) return fail(RASS_ERR_INVALID, "scan workspace too small");
    if ((reinterpret_cast<uintptr_t>(r.corpus) & 15) != 0) return fail(RASS_ERR_INVALID, "corpus not 16-B aligned");
    const ScratchView L = scratch_layout(r.ws, nq, k);

    // a4 on the query side (reference app/main.py:1536-1537), written zero-padded.  (`queries_prepared`: the workspace
    // already holds these very queries normalised at this stride — the fine scan of an IVF probe right after its coarse scan.)
    if (!r.queries_prepared)
        HIP_TRY(rass::launch_normalize_rows_f32(r.queries, r.q_stride, L.q_padded, stride, nq, r.q_dim, st, pad_nq(nq)));

    // IVF: the number of work tiles is only known on the device; size the grid by the slab
    const int grid = scan_grid(r.plan ? r.plan->max_tiles : (r.n_rows + 31) / 32, k, r.n_cus);

    rass::ScanArgs a;
    a.corpus = r.corpus;
    a.row_tag = r.row_tag;
    a.q_padded = L.q_padded;
    a.q_filter = r.q_filter;
    a.part_scores = L.part_scores;
    a.part_ids = L.part_ids;
    a.row_stride = stride;
    a.id_base = r.id_base;
    a.n_rows = (int)r.n_rows;
    a.nq = nq;
    a.k = k;
    a.xcd_skew = scan_xcd_skew(nq, grid, r.n_cus);
    a.q_filter_mask = r.ext.d_q_mask;
    a.q_after_score = r.ext.d_after_s;
    a.q_after_id = r.ext.d_after_i;
    a.live_nq = r.ext.d_live;
    if (r.plan) set_plan(a, *r.plan);
    const int64_t min_share = scan_sample_floor_min_share();
    if (min_share > 0 && !r.plan && nq > 16 && grid <= rass::kMaxSampleGroups && r.n_rows >= min_share * 64 * grid) {
        const int rc = sample_prelaunch(a, grid, L.sample_best, rass::launch_scan_topk_f32, st);
        if (rc != RASS_OK) return rc;
    }
    const int rc = timed_launch(r.timing, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, k, r.out_scores, r.out_ids, st, r.id_map, 0, 0, nullptr,
                                    r.ext.d_live));
    return RASS_OK;
}

// A bf16 corpus (RASS_BF16): the bf16 scan IS the search — normalise the queries, round them to bf16,
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation over the bf16 slab, per-workgroup top-k, merge.
int bf16_scan_launch(rass_index* idx, const FlatRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_k(k)) return rc;
    const int64_t stride = idx->stride;
    const int64_t rows = idx->rows.load(std::memory_order_acquire);
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, pad_nq(nq)));
    HIP_TRY(rass::launch_queries_to_bf16(L.q_padded, L.q_bf16, (int64_t)pad_nq(nq) * stride, st));
    const int grid = scan_grid((rows + 63) / 64, k, eng->n_cus);
    rass::ScanBf16Args a = bf16_args(idx, rows, r.row_tag, k);
    set_group(a, L.q_bf16, r.q_filter, r.q_filter_mask, L.part_scores, L.part_ids, nq);
    a.id_base = r.id_map ? 0 : r.id_base;
    a.q_after_score = r.after_score;
    a.q_after_id = r.after_row;
    // the sample floor pays where many candidates are kept (k = 10: 96.1 k queries/s without it, 89.9 k with its extra launch;
    // the prefilter's 32 candidates: 85.5 k -> 92.4 k); RASS_I8_SAMPLE_FLOOR=0: the A/B for both scans
    const bool ext = r.q_filter_mask || r.after_score;
    if (!ext && k >= 24 && i8_sample_floor(rows, grid)) {
        const int rc = sample_prelaunch(a, grid, L.sample_best, rass::launch_scan_bf16_topk, st);
        if (rc != RASS_OK) return rc;
    }
    const int rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_bf16_topk(a, grid, st)); });
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, k, r.out_scores, r.out_ids, st, r.id_map));
    return RASS_OK;
}

// Prefilter mode: bf16 (mode 1) or int8 (mode 2) candidate scan (32 per query) -> merge -> exact fp32 re-rank.
// r.cand_scores / r.cand_rows (optional, [nq][32]): the merged candidate lists as well (rass_index_candidates_device).
int prefilter_launch(rass_index* idx, const FlatRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_k(k)) return rc;
    const int64_t stride = idx->stride;
    const int64_t rows = idx->rows;
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    float* cand_scores = r.cand_scores ? r.cand_scores : L.cand_scores;
    int64_t* cand_ids = r.cand_rows ? r.cand_rows : L.cand_ids;
    const int nq_pad = pad_nq(nq);
    const int kc = RASS_MAX_K;  // candidates per query
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, nq_pad));
    const int grid = scan_grid((rows + 63) / 64, kc, eng->n_cus);
    int rc;
    if (idx->prefilter == 2) {
        HIP_TRY(rass::launch_queries_to_i8(L.q_padded, L.q_bf16, nq_pad, stride, idx->stride_i8, st));
        rass::ScanI8Args a = i8_args(idx, rows, r.row_tag, kc);
        set_group(a, L.q_bf16, r.q_filter, r.q_filter_mask, L.part_scores, L.part_ids, nq);
        if (i8_sample_floor(rows, grid)) {   // the sample launch: the first 64 * grid rows, the best score per workgroup
            rc = sample_prelaunch(a, grid, L.sample_best, rass::launch_scan_i8_topk, st);
            if (rc != RASS_OK) return rc;
        }
        rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_i8_topk(a, grid, st)); });
    } else {
        HIP_TRY(rass::launch_queries_to_bf16(L.q_padded, L.q_bf16, (int64_t)nq_pad * stride, st));
        rass::ScanBf16Args a = bf16_args(idx, rows, r.row_tag, kc);
        set_group(a, L.q_bf16, r.q_filter, r.q_filter_mask, L.part_scores, L.part_ids, nq);
        if (!r.q_filter_mask && i8_sample_floor(rows, grid)) {
            rc = sample_prelaunch(a, grid, L.sample_best, rass::launch_scan_bf16_topk, st);
            if (rc != RASS_OK) return rc;
        }
        rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_bf16_topk(a, grid, st)); });
    }
    if (rc != RASS_OK) return rc;
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, kc, cand_scores, cand_ids, st));
    HIP_TRY(rass::launch_rerank_f32(idx->d_rows, stride, L.q_padded, cand_ids, nq, kc, k, r.id_map ? 0 : r.id_base, r.out_scores,
                                    r.out_ids, st, 0, 0, r.id_map));
    return RASS_OK;
}

// ---- prefilter mode 3: certified int8 search (DESIGN.md §3 "certified int8 search") ---------------------------------------
// Mode 3, k <= 32: per pass of <= 16 queries — hi + lo int8 queries, the sample floor, the int8 candidate scan, the selection of
// 128 candidates and tau, their exact re-rank, the certificate, the fp32 flat scan of the failed queries (exits on the device
// when none failed) and its scatter.  Stream-ordered: the host reads nothing back.  The optional outputs (the parity hook
// rass_index_candidates_exact_device) are r.cand_scores / r.cand_rows [nq][128], r.tau [nq] and r.certified [nq].
int cert_launch(rass_index* idx, const FlatRequest& r) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_k(k)) return rc;
    if (r.q_filter_mask && !r.q_filter) return fail(RASS_ERR_INVALID, "a filter mask needs a filter");
    const int64_t rows = idx->rows.load(std::memory_order_acquire);
    const int64_t stride = idx->stride;
    const int dim = idx->dim;
    const int64_t n_tiles = (rows + 63) / 64;
    // not scan_grid: the selection kernel takes kMaxGridSel slices, and no merge launch follows
    const int grid = (int)std::min<int64_t>(std::max<int64_t>(n_tiles, 1), std::min(eng->n_cus, rass::kMaxGridSel));
    int rc = grow_block(&eng->d_cert, &eng->cert_bytes, cert_layout(nullptr, grid, stride, idx->stride_i8, dim).total, st);
    if (rc != RASS_OK) return rc;
    const CertView L = cert_layout(eng->d_cert, grid, stride, idx->stride_i8, dim);
    // the parity hook: the search's result is not reported
    float* out_scores = r.out_scores && r.out_ids ? r.out_scores : L.hook_s;
    int64_t* out_ids = r.out_scores && r.out_ids ? r.out_ids : L.hook_i;
    // the sample floor: the 128th of the per-workgroup maxima of a sample launch over the first S tiles of every workgroup (S grows
    // with the slab so that the floor keeps the candidates under the selection's capacity); none where every row fits anyway
    const bool floor_on = grid >= rass::kCertC && rows > rass::kCertSelCap && grid <= rass::kMaxSampleGroups;
    const int64_t per_wg = n_tiles / std::max(grid, 1);
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(8, per_wg / 16));
    for (int p0 = 0; p0 < nq; p0 += rass::kCertQ) {
        const int b = std::min(rass::kCertQ, nq - p0);
        HIP_TRY(rass::launch_normalize_rows_f32(r.queries + (int64_t)p0 * dim, dim, L.q_padded, stride, b, dim, st, rass::kCertQ));
        HIP_TRY(rass::launch_queries_to_i8_hilo(L.q_padded, L.q8, L.qinfo, stride, idx->stride_i8, st));
        rass::ScanI8CertArgs a{};   // no sample_out, no sample_best
        a.corpus = idx->d_rows_i8;
        a.row_scale = idx->d_row_scale;
        a.row_tag = r.row_tag;
        a.q_i8 = L.q8;
        a.qinfo = L.qinfo;
        a.q_filter = r.q_filter ? r.q_filter + p0 : nullptr;
        a.q_filter_mask = r.q_filter_mask ? r.q_filter_mask + p0 : nullptr;
        a.row_stride = idx->stride_i8;
        a.n_rows = (int)rows;
        a.nq = b;
        a.list_s = L.list_s;
        a.list_r = L.list_r;
        a.list_n = L.list_n;
        a.list_floor = L.list_floor;
        if (floor_on) {
            rass::ScanI8CertArgs sa = a;
            sa.n_rows = (int)std::min<int64_t>(rows, (int64_t)64 * grid * S);
            sa.sample_out = L.sample;
            HIP_TRY(rass::launch_scan_i8_cert(sa, grid, st));
            a.sample_best = sa.sample_out;
            a.sample_groups = grid;
            a.floor_rank = rass::kCertC;
        }
        rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_i8_cert(a, grid, st)); });
        if (rc != RASS_OK) return rc;
        float* tau = r.tau ? r.tau + p0 : L.tau;
        HIP_TRY(rass::launch_cert_select(a.list_s, a.list_r, a.list_n, a.list_floor, grid, b, L.cand_rows,
                                         r.cand_scores ? r.cand_scores + (int64_t)p0 * rass::kCertC : nullptr,
                                         r.cand_rows ? r.cand_rows + (int64_t)p0 * rass::kCertC : nullptr, tau, st));
        // the four chunks of 32 candidates in ONE re-rank launch of 64 "queries": chunk c of query q is entry 16 c + q, its
        // query vector the c-th copy of q_padded
        for (int ch = 1; ch < rass::kCertC / 32; ++ch)
            HIP_TRY(hipMemcpyAsync(L.q_padded + (int64_t)ch * rass::kCertQ * stride, L.q_padded, (size_t)rass::kCertQ * stride * sizeof(float),
                                   hipMemcpyDeviceToDevice, st));
        HIP_TRY(rass::launch_rerank_f32(idx->d_rows, stride, L.q_padded, L.cand_rows, (rass::kCertC / 32) * rass::kCertQ, 32, 32,
                                        r.id_map ? 0 : r.id_base, L.rr_s, L.rr_i, st, 0, 0, r.id_map));
        rass::CertFinishArgs f;
        f.rr_s = L.rr_s;
        f.rr_i = L.rr_i;
        f.tau = tau;
        f.qinfo = L.qinfo;
        f.stats = idx->d_cert_stats;
        f.dim = dim;
        f.nq = b;
        f.k = k;
        f.out_s = out_scores + (int64_t)p0 * k;
        f.out_i = out_ids + (int64_t)p0 * k;
        f.certified = r.certified ? r.certified + p0 : nullptr;
        f.fail_idx = L.fail_idx;
        f.fail_flag = L.fail_flag;
        f.fail_n = L.fail_n;
        f.q_raw = r.queries + (int64_t)p0 * dim;
        f.q_filter = a.q_filter;
        f.q_filter_mask = a.q_filter_mask;
        f.fb_q = L.fb_q;
        f.fb_filter = L.fb_filter;
        f.fb_mask = L.fb_mask;
        f.counters = idx->d_cert_counts;
        HIP_TRY(rass::launch_cert_finish(f, st));
        // the exact fp32 flat scan of the failed queries (compacted to the front): its workgroups exit when none failed
        ScanRequest fb = scan_request(eng);
        fb.corpus = idx->d_rows, fb.n_rows = rows, fb.stride = stride, fb.row_tag = r.row_tag;
        fb.queries = f.fb_q, fb.q_dim = dim, fb.q_stride = dim, fb.nq = b, fb.q_filter = r.q_filter ? f.fb_filter : nullptr;
        fb.k = k, fb.id_base = r.id_map ? 0 : r.id_base, fb.id_map = r.id_map;
        fb.out_scores = L.fb_s, fb.out_ids = L.fb_i;
        fb.ext.d_q_mask = r.q_filter_mask ? f.fb_mask : nullptr;
        fb.ext.d_live = L.fail_n;
        rc = scan_launch(fb);
        if (rc != RASS_OK) return rc;
        HIP_TRY(rass::launch_cert_scatter(L.fb_s, L.fb_i, f.fail_idx, L.fail_n, k, f.out_s, f.out_i, st));
    }
    return RASS_OK;
}

}  // namespace host
}  // namespace rass
