// api_search.hip — the C ABI of include/rass_engine.h: top-k search of a flat index.  The dispatch of one launch group
// to its launch path (api_scan.hip), the two fused batches (fp32 and prefilter), the device entry points and the
// candidates hooks, the host search API with its pinned slots (k > 32 in passes) and the cross-index batch
// rass_index_search_multi.  The searches that emit instead of ranking live in api_emit.hip, the allow-list search in
// api_allow.hip.  Host-side C++ only.  The objects and the threading rules: api_internal.h.

#include "api_internal.h"

namespace rass {
namespace host {

HostSlot* slot_acquire(rass_engine* eng) {
    std::unique_lock<std::mutex> lk(eng->slot_mu);
    for (;;) {
        for (HostSlot& sl : eng->slots)
            if (!sl.busy) {
                sl.busy = true;
                return &sl;
            }
        eng->slot_cv.wait(lk);
    }
}

void slot_release(rass_engine* eng, HostSlot* sl) {
    {
        std::lock_guard<std::mutex> lk(eng->slot_mu);
        sl->busy = false;
    }
    eng->slot_cv.notify_one();
}

void slot_fill(HostSlot* sl, int dim, const float* queries, const int32_t* q_filter, const int32_t* q_filter_mask, int b) {
    memcpy(sl->h_q, queries, (size_t)b * dim * sizeof(float));
    if (q_filter) memcpy(sl->h_filter, q_filter, (size_t)b * sizeof(int32_t));
    if (q_filter_mask) memcpy(sl->h_mask, q_filter_mask, (size_t)b * sizeof(int32_t));
}

int slot_upload(rass_engine* eng, HostSlot* sl, int dim, bool filter, bool mask, int b) {
    hipStream_t st = eng->stream;
    HIP_TRY(hipMemcpyAsync(eng->d_qraw, sl->h_q, (size_t)b * dim * sizeof(float), hipMemcpyHostToDevice, st));
    if (filter) HIP_TRY(hipMemcpyAsync(eng->d_qfilter, sl->h_filter, (size_t)b * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (mask) HIP_TRY(hipMemcpyAsync(eng->d_qmask, sl->h_mask, (size_t)b * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return RASS_OK;
}

int slot_download(rass_engine* eng, HostSlot* sl, int b, int k, const int64_t* d_scanned) {
    hipStream_t st = eng->stream;
    HIP_TRY(hipMemcpyAsync(sl->h_out_s, eng->d_out_scores, (size_t)b * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sl->h_out_i, eng->d_out_ids, (size_t)b * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (d_scanned) HIP_TRY(hipMemcpyAsync(sl->h_scanned, d_scanned, 8, hipMemcpyDeviceToHost, st));
    return RASS_OK;
}

int slot_grow_io(HostSlot* sl, size_t need) {
    if (sl->io_bytes >= need) return RASS_OK;
    HIP_TRY(hipEventSynchronize(sl->done));   // growth only: the last group staged through the old block has landed
    if (sl->h_io) HIP_TRY(hipHostFree(sl->h_io));
    sl->h_io = nullptr;
    sl->io_bytes = 0;
    HIP_TRY(hipHostMalloc(&sl->h_io, need, hipHostMallocDefault));
    sl->io_bytes = need;
    return RASS_OK;
}

namespace {

// One launch group (<= 32 queries) of a device search; the caller holds eng->mu and has set the device.  r.id_base is the
// caller's; row_tag / id_map come from the index.  one_pass = false: a pass of a k > RASS_MAX_K host search, which stays
// on the exact scan whatever the prefilter mode.  exact = true: the exact scan whatever the mode and k (search_ex_once).
int search_device_group(rass_index* idx, FlatRequest r, bool one_pass = true, bool exact = false) {
    rass_engine* eng = idx->eng;
    const IndexView iv = index_view(idx, r.q_filter != nullptr, r.id_base, r.after_score != nullptr);
    r.use(iv);
    if (idx->dtype == RASS_BF16) return bf16_scan_launch(idx, r);
    if (!exact && idx->prefilter == 3 && iv.rows > 0 && !r.after_score && one_pass) return cert_launch(idx, r);
    if (!exact && idx->prefilter && idx->prefilter != 3 && iv.rows > 0 && r.k <= kPrefilterMaxK && !r.after_score)
        return prefilter_launch(idx, r);
    // the continuation bound names ROWS of this index (the kernel compares id_base + row): the scan runs with
    // id_base 0 and the ids are translated afterwards, as for caller-assigned ids
    ScanRequest s = scan_request(eng);
    s.corpus = iv.corpus, s.n_rows = iv.rows, s.stride = idx->stride, s.row_tag = iv.row_tag;
    s.queries = r.queries, s.q_dim = idx->dim, s.q_stride = idx->dim, s.nq = r.nq, s.q_filter = r.q_filter;
    s.k = r.k, s.id_base = iv.id_base, s.id_map = iv.id_map, s.out_scores = r.out_scores, s.out_ids = r.out_ids;
    s.timing = eng;
    s.ext.d_q_mask = r.q_filter_mask, s.ext.d_after_s = r.after_score, s.ext.d_after_i = r.after_row;
    return scan_launch(s);
}

// Group g of a batch request: its queries, filters and outputs (gs / gi: the output group strides).
FlatRequest batch_group(const rass_index* idx, const FlatRequest& r, int g, int64_t gs, int64_t gi) {
    FlatRequest q = r;
    q.nq = std::min(RASS_MAX_QBATCH, r.nq - g * RASS_MAX_QBATCH);
    q.queries = r.queries + (int64_t)g * RASS_MAX_QBATCH * idx->dim;
    q.q_filter = r.q_filter ? r.q_filter + g * RASS_MAX_QBATCH : nullptr;
    q.out_scores = r.out_scores + g * gs;
    q.out_ids = r.out_ids + g * gi;
    return q;
}

// How a fused fp32 batch finds its sample floors: nothing (small slab, RASS_SCAN_SAMPLE_FLOOR=0), group by group, or for
// all groups at once when the batch has several full groups — representatives chosen by bf16 MFMAs and scored exactly
// (sample_rep.hip: `rep`) or, where that stage has no kernel (a grid that is no multiple of 32) and under
// RASS_SCAN_BATCH_SAMPLE=f32, one fp32 sample launch (kFlatSampleGroups).  Either way the floor is the k-th largest of 32
// scores of different rows of the slab's first 64 * grid; results do not depend on it (rows tying with it are kept).
struct BatchSamplePlan {
    int grid;
    bool sample, one_sample, rep;
};
BatchSamplePlan batch_sample_plan(const rass_engine* eng, int64_t rows, int64_t stride, int nq, int k) {
    BatchSamplePlan p;
    p.grid = scan_grid((rows + 31) / 32, k, eng->n_cus);
    const int groups = (nq + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    const int64_t min_share = scan_sample_floor_min_share();
    const int mode = scan_batch_sample_mode();
    p.sample = min_share > 0 && p.grid <= rass::kMaxSampleGroups && rows >= min_share * 64 * p.grid;
    p.one_sample = p.sample && groups >= 2 && nq % 32 == 0 && mode != kBatchSampleGroups && p.grid >= 32;
    p.rep = p.one_sample && mode == kBatchSampleRep && rass::sample_rep_supported(stride, p.grid);
    return p;
}

// The fused batch of rass_index_search_device_batch on an fp32 flat index: the per-group steps of scan_launch, but
// ONE normalise launch and ONE merge launch for the whole batch, and the groups' sample passes back to back (their
// 64 * grid rows stay in the Infinity Cache between them) ahead of the big scans.  Per 32 queries the serial tail
// of a search (normalise 4.8 us + merge 17 us on 32 of 256 CUs + launch gaps) shrinks to the sample pass.
// r: the whole batch (nq queries); gs / gi: the output group strides.
int scan_launch_batch(rass_index* idx, const FlatRequest& r, int64_t gs, int64_t gi) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq, k = r.k;
    const IndexView iv = index_view(idx, r.q_filter != nullptr, r.id_base);
    const int64_t rows = iv.rows;
    const int64_t stride = idx->stride;
    if (int rc = check_k(k)) return rc;
    if (rows < 0 || rows > kMaxScanRows) return fail(RASS_ERR_INVALID, "n_rows out of range for one scan");
    if (!rass::scan_supported_stride(stride) || stride > kMaxStride)
        return fail(RASS_ERR_UNSUPPORTED, kStrideMsg);
    const int groups = (nq + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    if (stride > kNarrowStride) {
        // wide rows: group by group through scan_launch (16 queries per kernel launch; no fused normalise / merge)
        for (int g = 0; g < groups; ++g) {
            const int rc = search_device_group(idx, batch_group(idx, r, g, gs, gi));
            if (rc != RASS_OK) return rc;
        }
        return RASS_OK;
    }
    const BatchSamplePlan plan = batch_sample_plan(eng, rows, stride, nq, k);
    const int grid = plan.grid;
    int rc = grow_block(&eng->d_batch, &eng->batch_bytes, batch_layout(nullptr, groups, grid, k, stride).total, st);
    if (rc != RASS_OK) return rc;
    const BatchView L = batch_layout(eng->d_batch, groups, grid, k, stride);

    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, (int64_t)groups * 32));

    auto group_args = [&](int g) {
        rass::ScanArgs a;
        a.corpus = iv.corpus;
        a.row_tag = iv.row_tag;
        a.q_padded = L.q_padded + (int64_t)g * 32 * stride;
        a.q_filter = r.q_filter ? r.q_filter + g * 32 : nullptr;
        a.part_scores = L.part_scores + (int64_t)g * L.part_per_group;
        a.part_ids = L.part_ids + (int64_t)g * L.part_per_group;
        a.row_stride = stride;
        a.id_base = iv.id_base;
        a.n_rows = (int)rows;
        a.nq = std::min(RASS_MAX_QBATCH, nq - g * 32);
        a.k = k;
        a.xcd_skew = scan_xcd_skew(a.nq, grid, eng->n_cus);
        return a;
    };
    const int64_t sample_rows = (int64_t)64 * grid;
    const bool sample = plan.sample, one_sample = plan.one_sample;
    // The sample stage (batch_sample_plan): for all groups at once — the representatives' stage, or ONE fp32 launch
    // (kFlatSampleGroups, 32 workgroups of 16 tiles per group: the floor = the k-th largest of 32 block maxima instead of
    // `grid` of them) — when the batch has several full groups; group by group otherwise.  Outside the timing brackets.
    const int sample_wgs = one_sample ? 32 : grid;
    if (plan.rep) {
        HIP_TRY(rass::launch_sample_rep(iv.corpus, iv.row_tag, stride, grid, L.q_padded, r.q_filter, nq, L.rep_qfrag, L.rep_part,
                                        L.rep_row, L.sample_best, st));
    } else if (one_sample) {   // not sample_prelaunch: 32 workgroups per group share the 64 * grid sample rows
        rass::ScanArgs s = group_args(0);
        s.n_rows = (int)sample_rows;
        s.xcd_skew = 0;
        s.sample_pass = true;
        s.nq = 32;
        s.part_scores = L.sample_best;
        s.part_ids = nullptr;
        s.wgs_per_group = sample_wgs;
        s.q_group_stride = 32 * stride;
        s.part_group_stride = (int64_t)32 * rass::kMaxSampleGroups;
        s.nq_total = nq;
        HIP_TRY(rass::launch_scan_topk_f32(s, groups * sample_wgs, st));
    } else if (sample)
        for (int g = 0; g < groups; ++g) {
            rass::ScanArgs a = group_args(g);
            if (a.nq <= 16) continue;
            rc = sample_prelaunch(a, grid, L.group_sample(g), rass::launch_scan_topk_f32, st);
            if (rc != RASS_OK) return rc;
        }
    // Consecutive FULL groups go two per corpus pass (scan_topk_f32_pair_kernel: 64 queries per launch, the lists of both
    // groups written where the two launches would write them, bit for bit the same); an odd last full group and a ragged
    // last group keep the 32-query kernel.  RASS_SCAN_BATCH_PAIR=0: one launch per group (the A/B).
    // Runs of 2..kStepMaxPairs consecutive pairs go to ONE launch of the step kernel (scan_step.hip: the pair kernel's loop over
    // pairs x tiles, the same lists bit for bit; a 4 096-query call is four launches, which bounds a launch's duration on a
    // 10 M-row slab); a single pair left over keeps the pair kernel.  The step kernel reads one ready-made floor per query:
    // launch_step_floors, once, outside the timing brackets as the sample stage is.  RASS_SCAN_BATCH_STEP=0: one launch per pair.
    const bool pairs = scan_batch_pair() && rass::scan_pair_supported_stride(stride);
    const int n_pairs = pairs ? nq / (2 * RASS_MAX_QBATCH) : 0;
    const bool step = scan_batch_step() && n_pairs >= 2 && grid <= (rows + 31) / 32;
    if (step && sample) HIP_TRY(rass::launch_step_floors(L.sample_best, sample_wgs, n_pairs * 64, k, L.step_floor, st));
    for (int g = 0; g < groups; ++g) {
        rass::ScanArgs a = group_args(g);
        if (sample && a.nq > 16) {
            a.sample_best = L.group_sample(g);
            a.sample_groups = sample_wgs;
        }
        const bool pair = pairs && a.nq == RASS_MAX_QBATCH && (g + 2) * RASS_MAX_QBATCH <= nq;
        const int run = pair && step ? std::min(rass::kStepMaxPairs, n_pairs - g / 2) : 1;   // pairs start at even groups
        if (pair) {
            a.nq = 2 * RASS_MAX_QBATCH;
            a.q_group_stride = 32 * stride;
            a.part_group_stride = (int64_t)L.part_per_group;
            a.xcd_skew = scan_xcd_skew(a.nq, grid, eng->n_cus);
        }
        if (run >= 2) {
            a.sample_best = nullptr, a.sample_groups = 0;
            a.step_floors = sample ? L.step_floor + g * 32 : nullptr;
            a.nq_total = 64 * run;
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32_step(a, grid, st)); }, /*extra_groups=*/2 * run - 1);
            g += 2 * run - 1;   // this launch served 2 * run groups
        } else if (pair) {
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32_pair(a, grid, st)); }, /*extra_groups=*/1);
            ++g;   // this pass served two groups
        } else
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
        if (rc != RASS_OK) return rc;
    }
    const rass::MergeGroups mg = dense_groups(nq, (int64_t)L.part_per_group, gs, gi);
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, k, r.out_scores, r.out_ids, st, iv.id_map, 0, 0, &mg));
    return RASS_OK;
}

// The parity hook of the batch's sample stage (rass_index_sample_floor_device): the normalise launch and the stage as
// scan_launch_batch enqueues them for this index, batch and k, then the representatives and their scores copied out.
// d_floors != nullptr (rass_index_step_floors_device): the one floor per query the step kernel reads (launch_step_floors), [nq],
// in place of the representatives.
int sample_floor_hook(rass_index* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter, int32_t* d_rows,
                      float* d_scores, float* d_floors = nullptr) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const IndexView iv = index_view(idx, d_q_filter != nullptr, 0);
    const int64_t stride = idx->stride;
    if (idx->dtype != RASS_F32 || idx->prefilter || nq <= RASS_MAX_QBATCH || iv.rows <= 0 || iv.rows > kMaxScanRows ||
        stride > kNarrowStride || !rass::scan_supported_stride(stride))
        return fail(RASS_ERR_UNSUPPORTED, "not a fused fp32 batch");
    const BatchSamplePlan plan = batch_sample_plan(eng, iv.rows, stride, nq, k);
    if (!plan.rep) return fail(RASS_ERR_UNSUPPORTED, "this batch does not take the representatives' sample stage");
    const int groups = nq / RASS_MAX_QBATCH;
    int rc = grow_block(&eng->d_batch, &eng->batch_bytes, batch_layout(nullptr, groups, plan.grid, k, stride).total, st);
    if (rc != RASS_OK) return rc;
    const BatchView L = batch_layout(eng->d_batch, groups, plan.grid, k, stride);
    HIP_TRY(rass::launch_normalize_rows_f32(d_queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, nq));
    HIP_TRY(rass::launch_sample_rep(iv.corpus, iv.row_tag, stride, plan.grid, L.q_padded, d_q_filter, nq, L.rep_qfrag, L.rep_part,
                                    L.rep_row, L.sample_best, st));
    if (d_floors) {
        HIP_TRY(rass::launch_step_floors(L.sample_best, 32, nq, k, L.step_floor, st));
        HIP_TRY(hipMemcpyAsync(d_floors, L.step_floor, (size_t)nq * sizeof(float), hipMemcpyDeviceToDevice, st));
        return RASS_OK;
    }
    HIP_TRY(hipMemcpyAsync(d_rows, L.rep_row, (size_t)nq * 32 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(d_scores, 32 * sizeof(float), L.sample_best, rass::kMaxSampleGroups * sizeof(float), 32 * sizeof(float),
                             (size_t)nq, hipMemcpyDeviceToDevice, st));
    return RASS_OK;
}

// The prefilter mode's batch (rass_index_search_device_batch on an index in mode 1 / 2): ONE normalise, ONE query
// conversion, the groups' candidate scans back to back, ONE grouped merge of their [grid][32][32] lists and ONE re-rank
// launch over all queries.  Group by group the serial tail of a 32-query search (normalise 5 + convert 7 + merge 34 on 32 of
// 256 CUs + re-rank 26 us) was a quarter of the int8 mode's time.  Same results as the group-by-group path, bit for bit.
int prefilter_launch_batch(rass_index* idx, const FlatRequest& r, int64_t gs, int64_t gi) {
    rass_engine* eng = idx->eng;
    hipStream_t st = eng->stream;
    const int nq = r.nq;
    const IndexView iv = index_view(idx, r.q_filter != nullptr, r.id_base);
    const int64_t rows = iv.rows;
    const int64_t stride = idx->stride;
    const int kc = RASS_MAX_K;
    const int groups = (nq + RASS_MAX_QBATCH - 1) / RASS_MAX_QBATCH;
    const int grid = scan_grid((rows + 63) / 64, kc, eng->n_cus);
    int rc = grow_block(&eng->d_batch, &eng->batch_bytes, batch_layout(nullptr, groups, grid, kc, stride, true).total, st);
    if (rc != RASS_OK) return rc;
    const BatchView L = batch_layout(eng->d_batch, groups, grid, kc, stride, true);
    const int nq_pad = groups * 32;
    HIP_TRY(rass::launch_normalize_rows_f32(r.queries, idx->dim, L.q_padded, stride, nq, idx->dim, st, nq_pad));
    const bool i8 = idx->prefilter == 2;
    const int64_t qs_stride = i8 ? idx->stride_i8 : stride * 2;   // bytes per converted query
    if (i8) HIP_TRY(rass::launch_queries_to_i8(L.q_padded, L.q_small, nq_pad, stride, idx->stride_i8, st));
    else HIP_TRY(rass::launch_queries_to_bf16(L.q_padded, L.q_small, (int64_t)nq_pad * stride, st));
    // the int8 scans' sample launches: ONE grouped launch for all groups when every group is full (32 launches of ~10 us each
    // otherwise: 5 % of a 1 024-query step)
    const bool floor_on = i8_sample_floor(rows, grid);
    const bool one_sample = i8 && floor_on && groups >= 2 && nq % 32 == 0;
    if (one_sample) {
        rass::ScanI8Args all = i8_args(idx, rows, iv.row_tag, kc);
        all.q_i8 = reinterpret_cast<const signed char*>(L.q_small);
        all.q_filter = r.q_filter;
        all.nq = 32;
        all.wgs_per_group = grid;
        all.q_group_stride = (int64_t)32 * qs_stride;
        all.part_group_stride = (int64_t)32 * rass::kMaxSampleGroups;
        rc = sample_prelaunch(all, grid, L.sample_best, rass::launch_scan_i8_topk, st, groups * grid);
        if (rc != RASS_OK) return rc;
    }
    for (int g = 0; g < groups; ++g) {
        const int b = std::min(RASS_MAX_QBATCH, nq - g * 32);
        const unsigned char* q_g = L.q_small + (int64_t)g * 32 * qs_stride;
        const int32_t* q_filter_g = r.q_filter ? r.q_filter + g * 32 : nullptr;   // (a batch takes no filter mask)
        float* part_scores_g = L.part_scores + (int64_t)g * L.part_per_group;
        int64_t* part_ids_g = L.part_ids + (int64_t)g * L.part_per_group;
        // the bracket holds a group's own sample launch too
        rc = timed_launch(eng, st, [&]() -> int {
            if (i8) {
                rass::ScanI8Args a = i8_args(idx, rows, iv.row_tag, kc);
                set_group(a, q_g, q_filter_g, nullptr, part_scores_g, part_ids_g, b);
                if (one_sample) {
                    a.sample_best = L.group_sample(g);
                    a.sample_groups = grid;
                } else if (floor_on) {
                    const int src = sample_prelaunch(a, grid, L.group_sample(g), rass::launch_scan_i8_topk, st);
                    if (src != RASS_OK) return src;
                }
                return HIP_RC(rass::launch_scan_i8_topk(a, grid, st));
            }
            rass::ScanBf16Args a = bf16_args(idx, rows, iv.row_tag, kc);
            set_group(a, q_g, q_filter_g, nullptr, part_scores_g, part_ids_g, b);
            if (floor_on) {
                const int src = sample_prelaunch(a, grid, L.group_sample(g), rass::launch_scan_bf16_topk, st);
                if (src != RASS_OK) return src;
            }
            return HIP_RC(rass::launch_scan_bf16_topk(a, grid, st));
        });
        if (rc != RASS_OK) return rc;
    }
    const rass::MergeGroups mg = dense_groups(nq, (int64_t)L.part_per_group, (int64_t)32 * kc, (int64_t)32 * kc);
    HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, nq, kc, L.cand_scores, L.cand_rows, st, nullptr, 0, 0, &mg));
    HIP_TRY(rass::launch_rerank_f32(idx->d_rows, stride, L.q_padded, L.cand_rows, nq, kc, r.k, iv.id_base, r.out_scores, r.out_ids, st,
                                    gs, gi, iv.id_map));
    return RASS_OK;
}

// What the device entry points of one launch group share: argument checks, the engine lock, the device.
int search_device_locked(rass_index_t* idx, const FlatRequest& r) {
    if (!idx || !r.queries || !r.out_scores || !r.out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (r.q_filter_mask && !r.q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    return search_device_group(idx, r);
}

}  // namespace

// One attempt of rass_index_search_ex.  Not on host_groups, and with search_multi_once the only host search that is not (the
// IVF's host round trip rides it too): its groups run PASSES, each with its own lock, upload and wait, and the cross-index batch
// builds a work list under the lock — folding either in would add flags there.  Both record the slot's event themselves.
int search_ex_once(rass_index* idx, const float* queries, int nq, int k, const int32_t* q_filter, const int32_t* q_filter_mask,
                   float* out_scores, int64_t* out_ids, bool exact) {
    rass_engine* eng = idx->eng;
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int dim = idx->dim;
    SlotGuard guard(eng);
    HostSlot* sl = guard.sl;
    for (int done = 0; done < nq;) {
        const int b = std::min(RASS_MAX_QBATCH, nq - done);
        slot_fill(sl, dim, queries + (int64_t)done * dim, q_filter ? q_filter + done : nullptr,
                  q_filter_mask ? q_filter_mask + done : nullptr, b);
        // k > RASS_MAX_K: passes of <= 32; pass p ranks only the rows strictly AFTER pass p-1's last hit
        for (int kdone = 0; kdone < k;) {
            const int kk = std::min(RASS_MAX_K, k - kdone);
            const bool cont = kdone > 0;
            {
                // the engine lock is held while ENQUEUING only: device staging and scratch are shared by
                // stream order, the wait happens on this call's own event
                std::lock_guard<std::mutex> lk(eng->mu);
                hipStream_t st = eng->stream;
                rc = slot_upload(eng, sl, dim, q_filter != nullptr, q_filter_mask != nullptr, b);
                if (rc != RASS_OK) return rc;
                FlatRequest r;
                r.queries = eng->d_qraw, r.nq = b, r.k = kk;
                r.q_filter = q_filter ? eng->d_qfilter : nullptr, r.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
                r.out_scores = eng->d_out_scores, r.out_ids = eng->d_out_ids;
                if (cont) {
                    HIP_TRY(hipMemcpyAsync(eng->d_after_s, sl->h_after_s, (size_t)b * sizeof(float), hipMemcpyHostToDevice, st));
                    HIP_TRY(hipMemcpyAsync(eng->d_after_i, sl->h_after_i, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice, st));
                    r.after_score = eng->d_after_s, r.after_row = eng->d_after_i;
                }
                if (cont && idx->has_gid.load(std::memory_order_acquire))  // the continuation bound compares row ordinals, the caller would hand back global ids
                    return fail(RASS_ERR_UNSUPPORTED, "k > RASS_MAX_K on an index with caller-assigned row ids");
                rc = search_device_group(idx, r, /*one_pass=*/k <= RASS_MAX_K, exact);
                if (rc != RASS_OK) return rc;
                rc = slot_download(eng, sl, b, kk);
                if (rc != RASS_OK) return rc;
                HIP_TRY(hipEventRecord(sl->done, st));
            }
            HIP_TRY(hipEventSynchronize(sl->done));
            for (int q = 0; q < b; ++q) {
                memcpy(out_scores + (int64_t)(done + q) * k + kdone, sl->h_out_s + (int64_t)q * kk, (size_t)kk * sizeof(float));
                memcpy(out_ids + (int64_t)(done + q) * k + kdone, sl->h_out_i + (int64_t)q * kk, (size_t)kk * sizeof(int64_t));
                // continuation bound for the next pass: this pass's last hit, or "nothing left" (-inf) when the
                // pass came back short
                const int64_t last_id = sl->h_out_i[(int64_t)q * kk + kk - 1];
                sl->h_after_s[q] = last_id >= 0 ? sl->h_out_s[(int64_t)q * kk + kk - 1] : -INFINITY;
                sl->h_after_i[q] = last_id >= 0 ? last_id : INT64_MAX;
            }
            kdone += kk;
        }
        done += b;
    }
    return RASS_OK;
}

}  // namespace host
}  // namespace rass

using namespace rass::host;

extern "C" {

int rass_index_search_device_ex(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                const int32_t* d_q_filter_mask, int64_t id_base, float* d_out_scores,
                                int64_t* d_out_ids) {
    FlatRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask;
    r.id_base = id_base, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    return search_device_locked(idx, r);
}

int rass_index_search_device_after(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                   const int32_t* d_q_filter_mask, const float* d_after_score,
                                   const int64_t* d_after_row, float* d_out_scores, int64_t* d_out_ids) {
    if (!d_after_score || !d_after_row) return fail(RASS_ERR_INVALID, "NULL argument");
    FlatRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.q_filter = d_q_filter, r.q_filter_mask = d_q_filter_mask;
    r.after_score = d_after_score, r.after_row = d_after_row, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    return search_device_locked(idx, r);
}

int rass_index_search_device_batch(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                   int64_t id_base, float* d_out_scores, int64_t* d_out_ids,
                                   int64_t out_scores_group_stride, int64_t out_ids_group_stride) {
    if (!idx || !d_queries || !d_out_scores || !d_out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (int rc = check_k(k)) return rc;
    const int64_t gs = out_scores_group_stride > 0 ? out_scores_group_stride : (int64_t)RASS_MAX_QBATCH * k;
    const int64_t gi = out_ids_group_stride > 0 ? out_ids_group_stride : (int64_t)RASS_MAX_QBATCH * k;
    if (gs < (int64_t)RASS_MAX_QBATCH * k || gi < (int64_t)RASS_MAX_QBATCH * k)
        return fail(RASS_ERR_INVALID, "output group strides must be >= 32 * k elements");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    FlatRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.q_filter = d_q_filter;
    r.id_base = id_base, r.out_scores = d_out_scores, r.out_ids = d_out_ids;
    const bool fused = idx->dtype == RASS_F32 && !idx->prefilter && nq > RASS_MAX_QBATCH;
    if (fused) return scan_launch_batch(idx, r, gs, gi);
    if (idx->prefilter && idx->prefilter != 3 && idx->dtype == RASS_F32 && nq > RASS_MAX_QBATCH && k <= kPrefilterMaxK &&
        idx->rows.load(std::memory_order_acquire) > 0)
        return prefilter_launch_batch(idx, r, gs, gi);
    // bf16 / prefilter corpora and single groups: the same result group by group
    for (int g = 0; g * RASS_MAX_QBATCH < nq; ++g) {
        rc = search_device_group(idx, batch_group(idx, r, g, gs, gi));
        if (rc != RASS_OK) return rc;
    }
    return RASS_OK;
}

int rass_index_search_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                             int64_t id_base, float* d_out_scores, int64_t* d_out_ids) {
    return rass_index_search_device_ex(idx, d_queries, nq, k, d_q_filter, nullptr, id_base, d_out_scores, d_out_ids);
}

int rass_index_candidates_device(rass_index_t* idx, const float* d_queries, int nq, const int32_t* d_q_filter,
                                 float* d_cand_scores, int64_t* d_cand_rows) {
    if (!idx || !d_queries || !d_cand_scores || !d_cand_rows) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    if (!idx->prefilter || idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "the index is not in a prefilter mode");
    if (idx->prefilter == 3)
        return fail(RASS_ERR_UNSUPPORTED, "mode 3 keeps 128 candidates per query: rass_index_candidates_exact_device");
    if (idx->rows.load(std::memory_order_acquire) <= 0) return fail(RASS_ERR_INVALID, "the index is empty");
    const ScratchView L = scratch_layout(eng->d_scratch, RASS_MAX_QBATCH, RASS_MAX_K);
    FlatRequest r;
    r.queries = d_queries, r.nq = nq, r.k = 1, r.q_filter = d_q_filter;
    r.row_tag = index_view(idx, d_q_filter != nullptr).row_tag;
    // the re-rank's own output (top-1 of every query) goes to the scratch's candidate area: not reported here
    r.out_scores = L.cand_scores, r.out_ids = L.cand_ids;
    r.cand_scores = d_cand_scores, r.cand_rows = d_cand_rows;
    return prefilter_launch(idx, r);
}

int rass_index_certify_stats(rass_index_t* idx, int64_t* queries, int64_t* certified, int64_t* fallbacks, float* R, float* V) {
    if (!idx) return fail(RASS_ERR_INVALID, "index is NULL");
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    unsigned long long c[3] = {0, 0, 0};
    unsigned st3[3] = {0, 0, 0};
    HIP_TRY(hipStreamSynchronize(eng->stream));
    if (idx->d_cert_counts) HIP_TRY(hipMemcpy(c, idx->d_cert_counts, sizeof(c), hipMemcpyDeviceToHost));
    if (idx->d_cert_stats) HIP_TRY(hipMemcpy(st3, idx->d_cert_stats, sizeof(st3), hipMemcpyDeviceToHost));
    float f[3];
    memcpy(f, st3, sizeof(f));
    if (queries) *queries = (int64_t)c[0];
    if (certified) *certified = (int64_t)c[1];
    if (fallbacks) *fallbacks = (int64_t)c[2];
    if (R) *R = f[0];
    if (V) *V = f[1];
    return RASS_OK;
}

int rass_index_candidates_exact_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                       float* d_cand_scores, int64_t* d_cand_rows, float* d_tau, int32_t* d_certified) {
    if (!idx || !d_queries || !d_cand_scores || !d_cand_rows || !d_tau || !d_certified) return fail(RASS_ERR_INVALID, "NULL argument");
    if (int rc = check_nq(nq)) return rc;
    if (int rc = check_k(k)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    if (idx->prefilter != 3 || idx->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "the index is not in prefilter mode 3");
    if (idx->rows.load(std::memory_order_acquire) <= 0) return fail(RASS_ERR_INVALID, "the index is empty");
    // the search's own result goes to a slot of the mode's workspace (no outputs given): not reported here
    FlatRequest r;
    r.queries = d_queries, r.nq = nq, r.k = k, r.q_filter = d_q_filter;
    r.row_tag = index_view(idx, d_q_filter != nullptr).row_tag;
    r.cand_scores = d_cand_scores, r.cand_rows = d_cand_rows, r.tau = d_tau, r.certified = d_certified;
    return cert_launch(idx, r);
}

int rass_index_sample_floor_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                   int32_t* d_out_rows, float* d_out_scores) {
    if (!idx || !d_queries || !d_out_rows || !d_out_scores) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (int rc = check_k(k)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    return sample_floor_hook(idx, d_queries, nq, k, d_q_filter, d_out_rows, d_out_scores);
}

int rass_index_step_floors_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                  float* d_out_floors) {
    if (!idx || !d_queries || !d_out_floors) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 1 || nq > RASS_MAX_DEVICE_BATCH) return fail(RASS_ERR_INVALID, "nq must be in [1, RASS_MAX_DEVICE_BATCH]");
    if (int rc = check_k(k)) return rc;
    rass_engine* eng = idx->eng;
    std::lock_guard<std::mutex> lk(eng->mu);
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    return sample_floor_hook(idx, d_queries, nq, k, d_q_filter, nullptr, nullptr, d_out_floors);
}

int rass_index_search_ex(rass_index_t* idx, const float* queries, int nq, int k, const int32_t* q_filter,
                         const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    if (!idx || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (k < 1 || k > RASS_MAX_K_MULTIPASS) return fail(RASS_ERR_INVALID, "k must be in [1, RASS_MAX_K_MULTIPASS]");
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    return one_layout([&] { return idx->layout_epoch.load(std::memory_order_acquire); },
                      [&] { return search_ex_once(idx, queries, nq, k, q_filter, q_filter_mask, out_scores, out_ids); });
}

static int search_multi_once(rass_engine* eng, rass_index_t* const* idxs, const float* queries, int nq, int k,
                             const int32_t* q_filter, const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    int rc = set_device(eng);
    if (rc != RASS_OK) return rc;
    const int dim = eng->dim;
    SlotGuard guard(eng);
    HostSlot* sl = guard.sl;
    const size_t item_bytes = 4 + 4 + 4 + 8 + 8;
    if (!sl->h_items) HIP_TRY(hipHostMalloc(&sl->h_items, (size_t)kMultiMaxItems * item_bytes, hipHostMallocDefault));
    int32_t* h_tile = static_cast<int32_t*>(sl->h_items);
    int32_t* h_rows = h_tile + kMultiMaxItems;
    uint32_t* h_mask = reinterpret_cast<uint32_t*>(h_rows + kMultiMaxItems);
    const float** h_base = reinterpret_cast<const float**>(h_mask + kMultiMaxItems);
    const int32_t** h_tags = reinterpret_cast<const int32_t**>(h_base + kMultiMaxItems);
    for (int done = 0; done < nq;) {
        const int b = std::min(RASS_MAX_QBATCH, nq - done);
        slot_fill(sl, dim, queries + (int64_t)done * dim, q_filter ? q_filter + done : nullptr,
                  q_filter_mask ? q_filter_mask + done : nullptr, b);
        {
            std::lock_guard<std::mutex> lk(eng->mu);  // slab pointers and row counts are stable under it
            hipStream_t st = eng->stream;
            if (!eng->d_mw_tile) {
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_tile), (size_t)kMultiMaxItems * 4));
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_rows), (size_t)kMultiMaxItems * 4));
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_mask), (size_t)kMultiMaxItems * 4));
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_base), (size_t)kMultiMaxItems * 8));
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_tags), (size_t)kMultiMaxItems * 8));
                HIP_TRY(hipMalloc(reinterpret_cast<void**>(&eng->d_mw_n), 4));
            }
            // the work list: for every DISTINCT index of the batch its tiles, each with the mask of the batch's
            // queries that belong to that index (a tile is fetched once however many of them there are)
            int n_items = 0;
            for (int q = 0; q < b; ++q) {
                rass_index* idx = idxs[done + q];
                bool seen = false;
                for (int p = 0; p < q && !seen; ++p) seen = idxs[done + p] == idx;
                if (seen) continue;
                uint32_t mask = 0;
                for (int p = q; p < b; ++p)
                    if (idxs[done + p] == idx) mask |= 1u << p;
                const IndexView iv = index_view(idx, q_filter != nullptr);
                const int64_t tiles = (iv.rows + 31) / 32;
                if (n_items + tiles > kMultiMaxItems)
                    return fail(RASS_ERR_UNSUPPORTED, "cross-index batch exceeds 65536 tiles (2 M rows): search the large index on its own");
                for (int64_t t = 0; t < tiles; ++t) {
                    h_tile[n_items] = (int32_t)t;
                    h_rows[n_items] = (int32_t)std::min<int64_t>(32, iv.rows - 32 * t);
                    h_mask[n_items] = mask;
                    h_base[n_items] = idx->d_rows;
                    h_tags[n_items] = iv.row_tag;
                    ++n_items;
                }
            }
            sl->h_scanned[0] = n_items;  // reused as the pinned source of the item count
            if (n_items > 0) {
                HIP_TRY(hipMemcpyAsync(eng->d_mw_tile, h_tile, (size_t)n_items * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(eng->d_mw_rows, h_rows, (size_t)n_items * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(eng->d_mw_mask, h_mask, (size_t)n_items * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(eng->d_mw_base, h_base, (size_t)n_items * 8, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(eng->d_mw_tags, h_tags, (size_t)n_items * 8, hipMemcpyHostToDevice, st));
            }
            HIP_TRY(hipMemcpyAsync(eng->d_mw_n, sl->h_scanned, 4, hipMemcpyHostToDevice, st));
            rc = slot_upload(eng, sl, dim, q_filter != nullptr, q_filter_mask != nullptr, b);
            if (rc != RASS_OK) return rc;
            // launch: normalise -> MULTI scan over the work list -> merge (ids are rows of each query's own index)
            const int64_t stride = pad_stride(dim);
            const ScratchView L = scratch_layout(eng->d_scratch, b, k);
            HIP_TRY(rass::launch_normalize_rows_f32(eng->d_qraw, dim, L.q_padded, stride, b, dim, st, pad_nq(b)));
            const int grid = scan_grid(n_items, k, eng->n_cus);
            rass::ScanArgs a;
            a.corpus = reinterpret_cast<const float*>(eng->d_scratch);
            a.row_tag = nullptr;
            a.q_padded = L.q_padded;
            a.q_filter = q_filter ? eng->d_qfilter : nullptr;
            a.q_filter_mask = q_filter_mask ? eng->d_qmask : nullptr;
            a.part_scores = L.part_scores;
            a.part_ids = L.part_ids;
            a.row_stride = stride;
            a.id_base = 0;
            a.n_rows = 0;
            a.nq = b;
            a.k = k;
            set_plan(a, IvfPlan{eng->d_mw_tile, eng->d_mw_rows, eng->d_mw_mask, eng->d_mw_n, 0});
            a.work_base = eng->d_mw_base;
            a.work_tags = eng->d_mw_tags;
            // counted by rass_engine_kernel_timing_* like every other scan launch
            rc = timed_launch(eng, st, [&] { return HIP_RC(rass::launch_scan_topk_f32(a, grid, st)); });
            if (rc != RASS_OK) return rc;
            HIP_TRY(rass::launch_merge_topk(L.part_scores, L.part_ids, grid, b, k, eng->d_out_scores, eng->d_out_ids, st));
            rc = slot_download(eng, sl, b, k);
            if (rc != RASS_OK) return rc;
            HIP_TRY(hipEventRecord(sl->done, st));
        }
        HIP_TRY(hipEventSynchronize(sl->done));
        memcpy(out_scores + (int64_t)done * k, sl->h_out_s, (size_t)b * k * sizeof(float));
        memcpy(out_ids + (int64_t)done * k, sl->h_out_i, (size_t)b * k * sizeof(int64_t));
        done += b;
    }
    return RASS_OK;
}

int rass_index_search_multi(rass_index_t* const* idxs, const float* queries, int nq, int k, const int32_t* q_filter,
                            const int32_t* q_filter_mask, float* out_scores, int64_t* out_ids) {
    if (!idxs || !out_scores || !out_ids) return fail(RASS_ERR_INVALID, "NULL argument");
    if (nq < 0 || (nq > 0 && !queries)) return fail(RASS_ERR_INVALID, "bad queries / nq");
    if (int rc = check_k(k)) return rc;
    if (q_filter_mask && !q_filter) return fail(RASS_ERR_INVALID, "q_filter_mask without q_filter");
    if (nq == 0) return RASS_OK;
    rass_engine* eng = idxs[0] ? idxs[0]->eng : nullptr;
    for (int q = 0; q < nq; ++q) {
        if (!idxs[q]) return fail(RASS_ERR_INVALID, "NULL index");
        if (idxs[q]->eng != eng) return fail(RASS_ERR_INVALID, "the indices of one batch must share an engine (one GPU)");
        if (idxs[q]->dtype != RASS_F32) return fail(RASS_ERR_UNSUPPORTED, "cross-index batches are fp32-only");
        if (idxs[q]->has_gid.load()) return fail(RASS_ERR_UNSUPPORTED, "cross-index batches need plain row ids");
    }
    if (eng && eng->dim > kNarrowStride)
        return fail(RASS_ERR_UNSUPPORTED, "cross-index batches need dim <= 1024: search wide-row indices one by one");
    // epochs only grow: their sum over the batch's indices stands still exactly when every one of them does
    auto epochs = [&] {
        int64_t sum = 0;
        for (int q = 0; q < nq; ++q) sum += idxs[q]->layout_epoch.load(std::memory_order_acquire);
        return sum;
    };
    return one_layout(epochs, [&] { return search_multi_once(eng, idxs, queries, nq, k, q_filter, q_filter_mask, out_scores, out_ids); });
}

int rass_index_search(rass_index_t* idx, const float* queries, int nq, int k, const int32_t* q_filter,
                      float* out_scores, int64_t* out_ids) {
    if (int rc = check_k(k)) return rc;
    return rass_index_search_ex(idx, queries, nq, k, q_filter, nullptr, out_scores, out_ids);
}

}  // extern "C"
