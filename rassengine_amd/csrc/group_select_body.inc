// group_select_body.inc — the body of the select kernels of group_topk.hip, included inside each of them (textually, so that
// each kernel compiles as if it held the code itself).  The kernel provides its parameters — table, counts, n_groups, k,
// id_base, id_map, the outputs, status — and, in scope, COUNT (the sort key comes from the counters), METRIC (it comes from a
// plane of a stats table: `mo`, a MetricOrder) and, where METRIC, mo.
    __shared__ unsigned long long keys[kGroupMaxK];
    __shared__ int grp[kGroupMaxK];
    __shared__ unsigned hist[256];
    __shared__ int sh_digit, sh_rank, n_sel, n_live;
    __shared__ unsigned long long n_hits;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned long long* tab = table + (int64_t)q * n_groups;
    const unsigned* cnt = COUNT ? counts + (int64_t)q * n_groups : nullptr;
    // the sort key of slot i: the group's best candidate key, or (count, 0xffffffff - i); 0 = an empty slot
    auto key_of = [&](int i) -> unsigned long long {
        if (!COUNT) return tab[i];
        const unsigned c = cnt[i];
        if (METRIC) {   // 1 << 53 | has_value << 52 | metric << 20 | (2^20 - 1 - i); a slot without a value: metric 0
            if (c == 0u) return 0ull;
            const bool has = mo.has[(int64_t)q * n_groups + i] != 0u;
            const unsigned m = mo.metric[(int64_t)q * n_groups + i];
            const unsigned field = has ? (mo.flip ? ~m : m) : 0u;
            return (1ull << 53) | ((unsigned long long)(has ? 1u : 0u) << 52) | ((unsigned long long)field << 20) |
                   (unsigned long long)((unsigned)(kGroupMaxGroups - 1) - (unsigned)i);
        }
        return c != 0u ? ((unsigned long long)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)i) : 0ull;
    };
    if (tid == 0) {
        n_sel = 0;
        n_live = 0;
        n_hits = 0ull;
    }
    __syncthreads();
    int mine = 0;
    unsigned long long hits = 0ull;
    for (int i = tid; i < n_groups; i += kGroupSelThreads) {
        if (COUNT) {
            const unsigned c = cnt[i];
            mine += c != 0u ? 1 : 0;
            hits += c;
        } else {
            mine += tab[i] != 0ull ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&n_live, mine);
    if (COUNT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
        if (lane == 0 && hits) atomicAdd(&n_hits, hits);
    }
    __syncthreads();
    const int live = n_live;
    if (tid == 0) total[q] = (int64_t)live;
    if (COUNT && tid == 0) total_hits[q] = (int64_t)n_hits;
    if (tid == 0 && q == 0) *out_status = *status != 0u ? 1 : 0;   // the scan's out-of-range flag, handed to the caller

    // T: the k-th largest key where more than k slots are taken (selected = keys >= T), else 1 (every non-zero slot)
    unsigned long long T = 1ull;
    if (live > k) {
        unsigned long long prefix = 0, pmask = 0;
        int rank = k;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            // whole rounds of the workgroup: hist_add's ballots need every lane of a wave in the same iteration
            for (int i0 = 0; i0 < n_groups; i0 += kGroupSelThreads) {
                const int i = i0 + tid;
                const unsigned long long key = i < n_groups ? key_of(i) : 0ull;
                hist_add(hist, key != 0ull && (key & pmask) == prefix, (unsigned)(key >> shift) & 255u);
            }
            __syncthreads();
            if (wid == 0) {   // lane l: digits 4l .. 4l+3; the largest digit d with #(digit >= d) >= rank
                const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                const unsigned own = c0 + c1 + c2 + c3;
                unsigned suf = own;   // inclusive suffix over lanes >= l
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned v = __shfl_down(suf, o, 64);
                    if (lane + o < 64) suf += v;
                }
                const unsigned above = suf - own;
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
            prefix |= (unsigned long long)sh_digit << shift;
            pmask |= 255ull << shift;
            rank = sh_rank;
            __syncthreads();
        }
        T = prefix;
    }
    // gather the taken keys with their slots (min(live, k) of them), pad to a power of two with key 0, sort descending
    const int n = live < k ? live : k;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n_groups; i += kGroupSelThreads) {
        const unsigned long long key = key_of(i);
        if (key >= T) {
            const int pos = atomicAdd(&n_sel, 1);
            if (pos < kGroupMaxK) {
                keys[pos] = key;
                grp[pos] = i;
            }
        }
    }
    for (int i = n + tid; i < n2; i += kGroupSelThreads) keys[i] = 0ull;   // [n, n2): no gathered key lands there
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += kGroupSelThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keys[i], b = keys[j];
                    const bool descending = (i & size) == 0;
                    if ((a < b) == descending) {
                        keys[i] = b, keys[j] = a;
                        const int ga = grp[i];
                        grp[i] = grp[j], grp[j] = ga;
                    }
                }
            }
            __syncthreads();
        }
    float* os = out_scores + (int64_t)q * k;
    int64_t* oi = out_ids + (int64_t)q * k;
    int32_t* og = out_groups + (int64_t)q * k;
    for (int i = tid; i < k; i += kGroupSelThreads) {
        float s = -INFINITY;
        int64_t id = -1, c = 0;
        int32_t g = -1;
        if (i < n) {
            g = grp[i];
            c = METRIC ? (int64_t)cnt[g] : (COUNT ? (int64_t)(keys[i] >> 32) : 0);
            const unsigned long long key = COUNT ? tab[g] : keys[i];   // the bucket's best row: a counted slot has one
            const int64_t row = (int64_t)(0xffffffffu - (unsigned)key);
            s = key_score((unsigned)(key >> 32));
            id = id_map ? id_map[row] : id_base + row;
        }
        os[i] = s;
        oi[i] = id;
        og[i] = g;
        if (COUNT) out_counts[(int64_t)q * k + i] = c;
    }
