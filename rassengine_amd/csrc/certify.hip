// certify.hip — the device half of the certified int8 search (prefilter mode 3; DESIGN.md §3 "certified int8 search"):
//   1. cert_select_kernel: per query, the kCertC best candidates (score desc, row asc) of the int8 scan's per-workgroup slices
//      (scan_i8_cert_kernel) by an exact radix select over 64-bit keys, and tau_q: the largest candidate score the selection
//      discarded, raised to the sample floor where the floor dropped a row (+inf where a slice overflowed);
//   2. (the four chunks of 32 are re-ranked exactly by rerank_f32_kernel, scan_bf16.hip: the flat kernel's fmaf order)
//   3. cert_finish_kernel: the top-k of the 128 exact scores, the certificate  up(tau_q) + B_q < t_k  per query, the failed
//      queries compacted (with their raw vectors and filters) for the fp32 fallback, and the device counters;
//   4. (the fp32 flat scan of those queries: every workgroup exits when the failed count is 0)
//   5. cert_scatter_kernel: the fallback's top-k over the failed queries' rows of the result.
// Nothing here is read back by the host: the device-pointer search APIs stay stream-ordered.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "scan_core.h"

namespace rass {

constexpr int kSelThreads = 1024;

__global__ __launch_bounds__(kSelThreads) void cert_select_kernel(const float* __restrict__ list_s, const int32_t* __restrict__ list_r,
                                                                  const int32_t* __restrict__ list_n, const float* __restrict__ list_floor,
                                                                  int grid, int nq, int64_t* __restrict__ cand_rows,
                                                                  float* __restrict__ cand_s, int64_t* __restrict__ cand_r,
                                                                  float* __restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];   // [kCertSelCap]
    __shared__ int off[kMaxGridSel + 1];
    __shared__ unsigned hist[256];
    __shared__ unsigned floor_key, ovf;
    __shared__ int sh_digit, sh_rank, n_sel;
    __shared__ uint64_t sel[kCertC];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (q >= nq) {   // a pass of fewer than 16 queries: the re-rank's entries of the absent ones hold no candidate
        if (tid < kCertC) cand_rows[((int64_t)(tid >> 5) * kCertQ + q) * 32 + (tid & 31)] = -1;
        return;
    }
    if (tid == 0) {
        floor_key = 0u;
        ovf = 0u;
        n_sel = 0;
    }
    __syncthreads();   // the initial values before any wave's atomics on them
    // per-slice counts -> exclusive offsets (Hillis-Steele over <= 1024 slices)
    int c = 0;
    if (tid < grid) {
        const int n = list_n[(int64_t)tid * kCertQ + q];
        const float f = list_floor[(int64_t)tid * kCertQ + q];
        c = n < kCertWgCap ? n : kCertWgCap;
        if (n > kCertWgCap) atomicOr(&ovf, 1u);
        if (f != -INFINITY) atomicMax(&floor_key, score_key(f));
    }
    off[tid + 1] = c;
    if (tid == 0) off[0] = 0;
    __syncthreads();
    for (int d = 1; d < kSelThreads; d <<= 1) {
        const int v = (tid + 1 - d >= 1) ? off[tid + 1 - d] : 0;
        __syncthreads();
        off[tid + 1] += v;
        __syncthreads();
    }
    int total = off[kSelThreads];
    if (total > kCertSelCap) {
        total = kCertSelCap;
        if (tid == 0) ovf = 1u;
    }
    // gather: flat index i -> slice w (the last w with off[w] <= i), entry i - off[w]
    for (int i = tid; i < total; i += kSelThreads) {
        int lo = 0, hi = grid - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const int64_t o = ((int64_t)lo * kCertQ + q) * kCertWgCap + (i - off[lo]);
        keys[i] = cand_key(list_s[o], list_r[o]);
    }
    __syncthreads();
    // the (kCertC + 1)-th largest key T (rows are distinct: keys are unique); selected = keys > T
    uint64_t T = 0;
    float tau_tr = -INFINITY;
    if (total > kCertC) {
        uint64_t prefix = 0, pmask = 0;
        int rank = kCertC + 1;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            for (int i = tid; i < total; i += kSelThreads) {
                const uint64_t k = keys[i];
                if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1u);
            }
            __syncthreads();
            if (wid == 0) {   // lane l: digits 4l .. 4l+3; the largest digit d with #(digit >= d) >= rank
                const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                const unsigned mine = c0 + c1 + c2 + c3;
                unsigned suf = mine;   // inclusive suffix over lanes >= l
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned v = __shfl_down(suf, o, 64);
                    if (lane + o < 64) suf += v;
                }
                const unsigned above = suf - mine;
                const unsigned s3 = above + c3, s2 = s3 + c2, s1 = s2 + c1, s0 = s1 + c0;
                const unsigned r = (unsigned)rank;
                int d = -1;
                unsigned sup = 0;   // #(digit > d)
                if (s0 >= r) { d = 4 * lane; sup = s1; }
                if (s1 >= r) { d = 4 * lane + 1; sup = s2; }
                if (s2 >= r) { d = 4 * lane + 2; sup = s3; }
                if (s3 >= r) { d = 4 * lane + 3; sup = above; }
                const unsigned long long b = __ballot(d >= 0);
                const int top = 63 - __clzll(b);
                if (lane == top) {
                    sh_digit = d;
                    sh_rank = rank - (int)sup;
                }
            }
            __syncthreads();
            prefix |= (uint64_t)sh_digit << shift;
            pmask |= (uint64_t)255 << shift;
            rank = sh_rank;
            __syncthreads();
        }
        T = prefix;
        tau_tr = key_score((unsigned)(T >> 32));
    }
    for (int i = tid; i < total; i += kSelThreads) {
        const uint64_t k = keys[i];
        if (k > T) sel[atomicAdd(&n_sel, 1)] = k;
    }
    __syncthreads();
    const int ns = n_sel;
    if (tid < kCertC) {
        float s = -INFINITY;
        int64_t r = -1;
        int pos = tid;
        if (tid < ns) {
            const uint64_t k = sel[tid];
            pos = 0;
            for (int o = 0; o < ns; ++o) pos += sel[o] > k ? 1 : 0;
            s = key_score((unsigned)(k >> 32));
            r = (int64_t)(0xffffffffu - (uint32_t)k);
        }
        cand_rows[((int64_t)(pos >> 5) * kCertQ + q) * 32 + (pos & 31)] = r;
        if (cand_s) cand_s[(int64_t)q * kCertC + pos] = s;
        if (cand_r) cand_r[(int64_t)q * kCertC + pos] = r;
    }
    if (tid == 0) {
        float t = tau_tr;
        if (floor_key) t = fmaxf(t, key_score(floor_key));
        tau[q] = ovf ? INFINITY : t;
    }
}

hipError_t launch_cert_select(const float* list_s, const int32_t* list_r, const int32_t* list_n, const float* list_floor, int grid,
                              int nq, int64_t* cand_rows, float* cand_s, int64_t* cand_r, float* tau, hipStream_t stream) {
    if (grid < 1 || grid > kMaxGridSel || nq < 1 || nq > kCertQ) return hipErrorInvalidValue;
    constexpr size_t lds = (size_t)kCertSelCap * sizeof(uint64_t);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cert_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(cert_select_kernel, dim3(kCertQ), dim3(kSelThreads), lds, stream, list_s, list_r, list_n, list_floor, grid, nq,
                       cand_rows, cand_s, cand_r, tau);
    return hipGetLastError();
}

// One workgroup of 128 threads per query: thread c holds candidate c's exact score and reported id.
__global__ __launch_bounds__(128) void cert_finish_kernel(CertFinishArgs p) {
    __shared__ float sc[kCertC];
    __shared__ int64_t id[kCertC];
    __shared__ float sh_tk;
    const int c = threadIdx.x;
    const double u = 1.0 / 16777216.0;   // 2^-24
    const double D = (double)p.dim;
    const double gD = D * u / (1.0 - D * u), g4 = 4.0 * u / (1.0 - 4.0 * u);
    const double R = (double)__uint_as_float(p.stats[0]), V = (double)__uint_as_float(p.stats[1]), Y = (double)__uint_as_float(p.stats[2]);
    {
        const int q = blockIdx.x;
        const int chunk = c >> 5, e = c & 31;
        sc[c] = p.rr_s[((int64_t)chunk * kCertQ + q) * 32 + e];
        id[c] = p.rr_i[((int64_t)chunk * kCertQ + q) * 32 + e];
        __syncthreads();
        // (score desc, id asc), entries without an id last: exactly rerank_f32_kernel's order over 128 instead of 32
        const float s = sc[c];
        const int64_t r = id[c];
        int rank = 0, valid = 0;
        for (int o = 0; o < kCertC; ++o) {
            const float so = sc[o];
            const int64_t ro = id[o];
            valid += ro >= 0 ? 1 : 0;
            const bool better = ro >= 0 && (r < 0 || so > s || (so == s && ro < r));
            rank += (o != c && better) ? 1 : 0;
        }
        float* os = p.out_s + (int64_t)q * p.k;
        int64_t* oi = p.out_i + (int64_t)q * p.k;
        if (r >= 0 && rank < p.k) {
            os[rank] = s;
            oi[rank] = r;
        }
        if (c >= valid && c < p.k) {
            os[c] = -INFINITY;
            oi[c] = -1;
        }
        if (c == 0) sh_tk = -INFINITY;
        __syncthreads();
        // t_k: the k-th exact score (-inf when fewer than k candidates: then tau is -inf too, nothing lies outside)
        if (r >= 0 && rank == p.k - 1) sh_tk = s;
        __syncthreads();
        if (c == 0) {
            const float tk = sh_tk;
            const float t = p.tau[q];
            bool ok;
            if (t == -INFINITY) {
                ok = true;
            } else if (!(t < INFINITY) || tk == -INFINITY) {
                ok = false;
            } else {
                const CertQInfo qi = p.qinfo[q];
                double B = R * qi.qnorm + V * qi.rho + gD * Y * qi.qnorm + g4 * V * qi.qa;
                B = B * (1.0 + 1e-12) + 1e-30;   // the double rounding of B's own terms; fp32 underflow of any score
                double lhs = (double)t + B;
                lhs += fabs(lhs) * 1e-15 + 1e-30;
                ok = lhs < (double)tk;
            }
            p.fail_flag[q] = ok ? 0 : 1;
            if (p.certified) p.certified[q] = ok ? 1 : 0;
        }
    }
}

// One workgroup: the failed queries compacted with their inputs for the fp32 fallback, and the counters.
__global__ __launch_bounds__(128) void cert_compact_kernel(CertFinishArgs p) {
    const int c = threadIdx.x;
    const int32_t* fail_flag = p.fail_flag;
    __shared__ int fidx[kCertQ];
    __shared__ int nfail;
    if (c == 0) {
        int n = 0;
        for (int q = 0; q < p.nq; ++q)
            if (fail_flag[q]) fidx[n++] = q;
        nfail = n;
        *p.fail_n = n;
        atomicAdd(p.counters + 0, (unsigned long long)p.nq);
        atomicAdd(p.counters + 1, (unsigned long long)(p.nq - n));
        atomicAdd(p.counters + 2, (unsigned long long)n);
    }
    __syncthreads();
    const int n = nfail;
    if (c < kCertQ) {
        p.fail_idx[c] = c < n ? fidx[c] : 0;
        p.fb_filter[c] = (c < n && p.q_filter) ? p.q_filter[fidx[c]] : -1;
        p.fb_mask[c] = (c < n && p.q_filter_mask) ? p.q_filter_mask[fidx[c]] : -1;
    }
    for (int i = 0; i < kCertQ; ++i) {
        const float* srcq = i < n ? p.q_raw + (int64_t)fidx[i] * p.dim : nullptr;
        for (int d = c; d < p.dim; d += 128) p.fb_q[(int64_t)i * p.dim + d] = srcq ? srcq[d] : 0.f;
    }
}

hipError_t launch_cert_finish(const CertFinishArgs& a, hipStream_t stream) {
    if (a.nq < 1 || a.nq > kCertQ || a.k < 1 || a.k > 32 || a.dim < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cert_finish_kernel, dim3(a.nq), dim3(128), 0, stream, a);
    hipLaunchKernelGGL(cert_compact_kernel, dim3(1), dim3(128), 0, stream, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void cert_scatter_kernel(const float* __restrict__ fb_s, const int64_t* __restrict__ fb_i,
                                                          const int32_t* __restrict__ fail_idx, const int32_t* __restrict__ fail_n, int k,
                                                          float* __restrict__ out_s, int64_t* __restrict__ out_i) {
    const int n = *fail_n;
    for (int i = 0; i < n; ++i) {
        const int q = fail_idx[i];
        for (int j = threadIdx.x; j < k; j += 64) {
            out_s[(int64_t)q * k + j] = fb_s[(int64_t)i * k + j];
            out_i[(int64_t)q * k + j] = fb_i[(int64_t)i * k + j];
        }
    }
}

hipError_t launch_cert_scatter(const float* fb_s, const int64_t* fb_i, const int32_t* fail_idx, const int32_t* fail_n, int k,
                               float* out_s, int64_t* out_i, hipStream_t stream) {
    hipLaunchKernelGGL(cert_scatter_kernel, dim3(1), dim3(64), 0, stream, fb_s, fb_i, fail_idx, fail_n, k, out_s, out_i);
    return hipGetLastError();
}

}  // namespace rass
