// catalog.hip — recommending from an item catalogue: the user x item candidate grid, written and ranked tile by tile.
//
// No counterpart in the reference.  cdc_eval_topk (metrics.hip) ranks rows that already exist; here the rows are the cross product
// of U contexts (full id rows with the user side filled in) and I catalogue items, which is never held as a whole: a tile of
// Ub contexts x Ib items is written (cdc_catalog_rows), goes through the model's eval forward, and its scores are folded into every
// context's running list of k entries (cdc_catalog_topk).  The contract — pool row, excluded candidates, the total order, the
// running lists — is stated in include/cdcmdr.h and restated in tests/catalog_exact.py.
//
// Both calls are stream-ordered single launches: no allocation, no workspace, nothing synchronised or read back, and launch
// dimensions that depend on the tile shape alone.
#include <algorithm>
#include "common.h"

#define CAT_THREADS 256

// ---------------------------------------------------------------------------------------------------------------------
// The tile of pool rows.  A pure store stream: a workgroup owns a run of whole rows (about 2048 store units), a thread a unit — 16
// bytes (four columns of one row) where F * 4 and X's alignment allow, one column otherwise — and consecutive threads write
// consecutive units.  What it reads is small and re-read from cache: Ub context rows, Ib catalogue rows, the column map (a kernel
// argument).  The thread that holds the domain column of a row also writes the row's tower group and its domain.
struct CatMap {
    int16_t src[CDC_CATALOG_MAX_F];     // per column of X: -1 = the context's value, c = catalogue column c
};

__device__ __forceinline__ int32_t cat_flag_word(int64_t u) { return (int32_t)(u < 0x7ffffffe ? u + 1 : 0x7fffffff); }

template <bool VEC>
__global__ void __launch_bounds__(CAT_THREADS) k_catalog_rows(const int32_t* __restrict__ context, int64_t ld_context,
                                                              const int32_t* __restrict__ catalog, int64_t ld_catalog, CatMap map, int32_t F,
                                                              int64_t u0, int64_t i0, uint32_t Ib, uint32_t rows, uint32_t rows_per_block,
                                                              int32_t* __restrict__ X, int64_t* __restrict__ group,
                                                              const int64_t* __restrict__ group_of_domain, int32_t n_domain, int32_t domain_col,
                                                              int32_t* __restrict__ domain_out, int32_t* __restrict__ err) {
    const uint32_t upr = VEC ? (uint32_t)F >> 2 : (uint32_t)F;             // store units per row
    const uint32_t r0 = blockIdx.x * rows_per_block;                       // the host keeps r0 < rows < 2^31
    const uint32_t nr = rows - r0 < rows_per_block ? rows - r0 : rows_per_block;
    for (uint32_t q = threadIdx.x; q < nr * upr; q += CAT_THREADS) {
        const uint32_t rl = q / upr, c = q - rl * upr;
        const uint32_t r = r0 + rl, ul = r / Ib, il = r - ul * Ib;
        const int32_t* __restrict__ crow = context + (u0 + ul) * ld_context;
        const int32_t* __restrict__ irow = catalog + (i0 + il) * ld_catalog;
        int32_t dom = 0;
        bool has_dom = false;
        if constexpr (VEC) {
            int32_t v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int32_t f = (int32_t)(c << 2) + e;
                const int32_t s = map.src[f];
                v[e] = s < 0 ? crow[f] : irow[s];
                if (f == domain_col) { dom = v[e]; has_dom = true; }
            }
            *reinterpret_cast<int4*>(X + (int64_t)r * F + (c << 2)) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
            const int32_t s = map.src[c];
            const int32_t v = s < 0 ? crow[c] : irow[s];
            X[(int64_t)r * F + c] = v;
            if ((int32_t)c == domain_col) { dom = v; has_dom = true; }
        }
        if (has_dom) {                                                     // domain_col is -1 when neither output is wanted
            if (domain_out) domain_out[r] = dom;
            if (group) {
                const bool ok = dom >= 0 && dom < n_domain;
                group[r] = ok ? group_of_domain[dom] : 0;
                if (!ok && err) atomicMax(err, cat_flag_word(u0 + ul));
            }
        }
    }
}

static int cat_tile_ok(const char* what, int64_t U, int64_t I, int64_t u0, int64_t Ub, int64_t i0, int64_t Ib) {
    CDC_CHECK_ARG(U >= 1 && I >= 1 && U < (1ll << 31) && I < (1ll << 31), CDC_E_BADARG, "%s: bad sizes U=%ld I=%ld", what, (long)U, (long)I);
    CDC_CHECK_ARG(u0 >= 0 && Ub >= 1 && Ub <= U && u0 <= U - Ub && i0 >= 0 && Ib >= 1 && Ib <= I && i0 <= I - Ib, CDC_E_BADARG,
                  "%s: tile [%ld, %ld + %ld) x [%ld, %ld + %ld) lies outside [0, %ld) x [0, %ld)", what, (long)u0, (long)u0, (long)Ub, (long)i0,
                  (long)i0, (long)Ib, (long)U, (long)I);
    CDC_CHECK_ARG(Ub * Ib < (1ll << 31), CDC_E_BADARG, "%s: a tile of %ld x %ld rows reaches 2^31", what, (long)Ub, (long)Ib);   // both < 2^31
    return 0;
}

extern "C" int cdc_catalog_rows(const int32_t* context, int64_t ld_context, int64_t U, const int32_t* catalog, int64_t ld_catalog, int64_t I,
                                const int32_t* item_cols, int32_t C, int32_t F, int64_t u0, int64_t Ub, int64_t i0, int64_t Ib, int32_t* X,
                                int64_t* group, const int64_t* group_of_domain, int32_t n_domain, int32_t domain_col, int32_t* domain_out,
                                int32_t* err_flag, void* stream) {
    CDC_CHECK_ARG(context && catalog && item_cols && X, CDC_E_BADARG, "catalog_rows: null pointer");
    CDC_CHECK_ARG(F >= 1 && F <= CDC_CATALOG_MAX_F && C >= 1 && C <= F && ld_context >= F && ld_catalog >= C, CDC_E_BADARG,
                  "catalog_rows: bad sizes F=%d C=%d ld_context=%ld ld_catalog=%ld", F, C, (long)ld_context, (long)ld_catalog);
    const int rc = cat_tile_ok("catalog_rows", U, I, u0, Ub, i0, Ib);
    if (rc != 0) return rc;
    CatMap map;
    for (int f = 0; f < F; ++f) map.src[f] = -1;
    for (int c = 0; c < C; ++c) {
        const int32_t f = item_cols[c];
        CDC_CHECK_ARG(f >= 0 && f < F, CDC_E_BADARG, "catalog_rows: item_cols[%d]=%d lies outside [0, %d)", c, f, F);
        CDC_CHECK_ARG(map.src[f] < 0, CDC_E_BADARG, "catalog_rows: item_cols[%d]=%d repeats column %d", c, f, f);
        map.src[f] = (int16_t)c;
    }
    if (group || domain_out) {
        CDC_CHECK_ARG(domain_col >= 0 && domain_col < F, CDC_E_BADARG, "catalog_rows: domain_col=%d lies outside [0, %d)", domain_col, F);
        CDC_CHECK_ARG(!group || (group_of_domain && n_domain >= 1), CDC_E_BADARG, "catalog_rows: the group output needs group_of_domain and n_domain >= 1");
    } else {
        domain_col = -1;
    }
    const bool vec = (F & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    const uint32_t upr = vec ? (uint32_t)F >> 2 : (uint32_t)F;
    const uint32_t rows = (uint32_t)(Ub * Ib), rpb = std::max<uint32_t>(1u, 2048u / upr);
    const uint32_t blocks = (rows + rpb - 1) / rpb;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_catalog_rows<true>, dim3(blocks), dim3(CAT_THREADS), 0, st, context, ld_context, catalog, ld_catalog, map, F, u0, i0,
                           (uint32_t)Ib, rows, rpb, X, group, group_of_domain, n_domain, domain_col, domain_out, err_flag);
    else
        hipLaunchKernelGGL(k_catalog_rows<false>, dim3(blocks), dim3(CAT_THREADS), 0, st, context, ld_context, catalog, ld_catalog, map, F, u0, i0,
                           (uint32_t)Ib, rows, rpb, X, group, group_of_domain, n_domain, domain_col, domain_out, err_flag);
    CDC_LAUNCH_CHECK("catalog_rows");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Select inside a tile and fold into the running lists.  One workgroup per context of the tile; its LDS holds CAT_CAP entries
// (score bits, item id, catalogue row: three arrays, 48 KB): the context's running list in front, this tile's candidates behind it.
//
//   order     an entry's key is (~score_key(score), item, catalogue row), ascending = best first; an empty slot (row -1) has the first
//             part all ones, which no live score reaches (~score_key of a non-NaN score is at most 0xff800000).  A total order.
//   threshold while the list is full its last entry's key, otherwise open.  The workgroup streams the context's Ib scores (16-byte
//             loads where the tile allows, the next round's load in flight under this round's work); a score whose first key part
//             lies above the threshold's is dropped there and then, the others fetch their item id, drop negative ids, compare the
//             full key, and only what still stands looks itself up in the context's seen slice (a binary search).
//   append    what passes takes a slot behind the list: a ballot and ONE LDS add per wave.  That add decides where an entry waits,
//             never whether or where it ends up: every list is cut from a sort under the total order.
//   compact   when the next round could overflow the buffer, and as soon as an open threshold can be closed (k entries are there:
//             an empty list then pays for a sort of one round's candidates, not of a full buffer) — a bound kept in registers says
//             when to look at the real count — the entries are sorted (bitonic, in LDS, padded with empty slots to a power of
//             two), the first k stay, the threshold rises.  After that almost nothing passes, and the launch is a read stream of
//             the scores.
//   output    one last sort, then k entries per context: the list, then -1 / -1 / NaN, written on every call.
// A NaN score is flagged per context; a negative id in the tile's item range makes EVERY context of the tile hold a bad candidate,
// so the workgroups share one scan of the id column and flag the tile's last context.  The error word's atomicMax is the only
// global atomic (a maximum: order-free).  seen_start comes from device memory: whatever it holds is clamped into [0, n_seen].
#define CAT_CAP 4096
#define CAT_CHUNK (4 * CAT_THREADS)
#define CAT_PAD_SCORE 0x7fc00000u

__device__ __forceinline__ uint32_t cat_key(float s, int32_t row) { return row < 0 ? 0xffffffffu : ~score_key(s); }
__device__ __forceinline__ bool cat_before(uint32_t ak, int32_t ai, int32_t ar, uint32_t bk, int32_t bi, int32_t br) {
    if (ak != bk) return ak < bk;
    if (ai != bi) return ai < bi;
    return ar < br;
}

// sorts the first cnt entries best first; every thread of the workgroup calls it with the same cnt; ends on a barrier
__device__ __forceinline__ void cat_sort(float* s, int32_t* it, int32_t* ct, int cnt, int tid) {
    int P = 64;
    while (P < cnt) P <<= 1;                                               // cnt <= CAT_CAP, a power of two
    for (int t = cnt + tid; t < P; t += CAT_THREADS) {
        s[t] = __uint_as_float(CAT_PAD_SCORE);
        it[t] = -1;
        ct[t] = -1;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += CAT_THREADS) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const float sa = s[a], sb = s[b];
                const int32_t ia = it[a], ib = it[b], ra = ct[a], rb = ct[b];
                const bool b_first = cat_before(cat_key(sb, rb), ib, rb, cat_key(sa, ra), ia, ra);
                if (b_first == ((a & kk) == 0)) {                          // ascending run: b must not stand before a
                    s[a] = sb; s[b] = sa;
                    it[a] = ib; it[b] = ia;
                    ct[a] = rb; ct[b] = ra;
                }
            }
            __syncthreads();
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void cat_load4(const float* __restrict__ srow, int64_t c0, int32_t Ib, int tid, float (&v)[4]) {
    if constexpr (VEC) {                                                   // Ib % 4 == 0: a lane's four scores are inside or outside together
        const int64_t at = c0 + (tid << 2);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (at < Ib) x = *reinterpret_cast<const float4*>(srow + at);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t at = c0 + j * CAT_THREADS + tid;
            v[j] = at < Ib ? srow[at] : 0.f;
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(CAT_THREADS) k_catalog_topk(const float* __restrict__ score, const int32_t* __restrict__ cat_id,
                                                              int64_t ld_catalog, int64_t u0, int32_t i0, int32_t Ib,
                                                              const int32_t* __restrict__ seen_start, const int32_t* __restrict__ seen_item,
                                                              int64_t n_seen, int32_t k, int32_t* __restrict__ item, int32_t* __restrict__ cat,
                                                              float* __restrict__ out_score, int32_t* __restrict__ n_out,
                                                              int32_t* __restrict__ err) {
    __shared__ float sh_s[CAT_CAP];
    __shared__ int32_t sh_it[CAT_CAP];
    __shared__ int32_t sh_ct[CAT_CAP];
    __shared__ int sh_cnt;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t u = u0 + blockIdx.x;
    const float* __restrict__ srow = score + (int64_t)blockIdx.x * Ib;

    if (err) {                                                             // the tile's id column, shared out over the workgroups
        bool bad = false;
        for (int64_t j = (int64_t)blockIdx.x * CAT_THREADS + tid; j < Ib; j += (int64_t)gridDim.x * CAT_THREADS)
            bad |= cat_id[(i0 + j) * ld_catalog] < 0;
        if (bad) atomicMax(err, cat_flag_word(u0 + gridDim.x - 1));
    }

    int64_t seen_lo = 0, seen_hi = 0;
    if (seen_start) {
        seen_lo = seen_start[u];
        seen_hi = seen_start[u + 1];
        seen_lo = seen_lo < 0 ? 0 : (seen_lo > n_seen ? n_seen : seen_lo);
        seen_hi = seen_hi < seen_lo ? seen_lo : (seen_hi > n_seen ? n_seen : seen_hi);
    }

    int n_list = n_out[u];
    n_list = n_list < 0 ? 0 : (n_list > k ? k : n_list);
    for (int t = tid; t < n_list; t += CAT_THREADS) {
        sh_s[t] = out_score[u * k + t];
        sh_it[t] = item[u * k + t];
        sh_ct[t] = cat[u * k + t];
    }
    if (tid == 0) sh_cnt = n_list;
    __syncthreads();

    uint32_t thr_k = 0xffffffffu;                                          // open: every live key lies below
    int32_t thr_i = 0x7fffffff, thr_r = 0x7fffffff;
    if (n_list == k) {
        thr_r = sh_ct[k - 1];
        thr_i = sh_it[k - 1];
        thr_k = cat_key(sh_s[k - 1], thr_r);
    }
    int sorted = n_list;                                                   // entries known to stand in order
    int bound = n_list;                                                    // the count is at most this
    bool nan_seen = false;

    float cur[4], nxt[4];
    cat_load4<VEC>(srow, 0, Ib, tid, cur);
    for (int64_t c0 = 0; c0 < Ib; c0 += CAT_CHUNK) {                       // 64-bit: Ib may stand within a round of 2^31
        cat_load4<VEC>(srow, c0 + CAT_CHUNK, Ib, tid, nxt);                 // zeros past the row's end
        const bool open = thr_k == 0xffffffffu;                            // uniform, like bound: every lane holds the same values
        if (bound + CAT_CHUNK > CAT_CAP || (open && bound >= k)) {
            __syncthreads();                                               // the appends so far are done
            int cnt = sh_cnt;
            __syncthreads();                                               // everyone has read it before anyone appends again
            if (cnt + CAT_CHUNK > CAT_CAP || (open && cnt >= k)) {
                cat_sort(sh_s, sh_it, sh_ct, cnt, tid);
                cnt = cnt < k ? cnt : k;
                if (tid == 0) sh_cnt = cnt;
                if (cnt == k) {
                    thr_r = sh_ct[k - 1];
                    thr_i = sh_it[k - 1];
                    thr_k = cat_key(sh_s[k - 1], thr_r);
                }
                sorted = cnt;
                __syncthreads();
            }
            bound = cnt;
        }
        bound += CAT_CHUNK;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t at = VEC ? c0 + (tid << 2) + j : c0 + j * CAT_THREADS + tid;
            const float p = cur[j];
            bool cand = at < Ib;
            if (cand && p != p) { nan_seen = true; cand = false; }
            const uint32_t key = ~score_key(p);
            cand = cand && key <= thr_k;
            const int32_t row = (int32_t)(i0 + at);                        // < I < 2^31 wherever cand holds
            int32_t id = 0;
            if (cand) {
                id = cat_id[(int64_t)row * ld_catalog];
                cand = id >= 0 && cat_before(key, id, row, thr_k, thr_i, thr_r);
            }
            if (cand && seen_hi > seen_lo) {
                int64_t lo = seen_lo, hi = seen_hi;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (seen_item[mid] < id) lo = mid + 1; else hi = mid;
                }
                cand = !(lo < seen_hi && seen_item[lo] == id);
            }
            const unsigned long long m = __ballot(cand);
            if (m != 0ull) {                                               // wave-uniform
                const int first = __ffsll((long long)m) - 1;
                int base = 0;
                if (lane == first) base = atomicAdd(&sh_cnt, __popcll(m));
                base = __shfl(base, first, 64);
                if (cand) {
                    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));      // < CAT_CAP: bound + CAT_CHUNK <= CAT_CAP
                    sh_s[pos] = p;
                    sh_it[pos] = id;
                    sh_ct[pos] = row;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    __syncthreads();
    int cnt = sh_cnt;
    if (cnt != sorted) cat_sort(sh_s, sh_it, sh_ct, cnt, tid);             // uniform; entries appended since the last sort
    cnt = cnt < k ? cnt : k;
    for (int t = tid; t < k; t += CAT_THREADS) {
        const bool live = t < cnt;
        out_score[u * k + t] = live ? sh_s[t] : __uint_as_float(CAT_PAD_SCORE);
        item[u * k + t] = live ? sh_it[t] : -1;
        cat[u * k + t] = live ? sh_ct[t] : -1;
    }
    if (tid == 0) n_out[u] = cnt;
    if (nan_seen && err) atomicMax(err, cat_flag_word(u));
}

extern "C" int cdc_catalog_topk(const float* score, const int32_t* catalog_id, int64_t ld_catalog, int64_t U, int64_t I, int64_t u0,
                                int64_t Ub, int64_t i0, int64_t Ib, const int32_t* seen_start, const int32_t* seen_item, int64_t n_seen,
                                int32_t k, int32_t* item, int32_t* cat, float* out_score, int32_t* n, int32_t* err_flag, void* stream) {
    CDC_CHECK_ARG(score && catalog_id && item && cat && out_score && n, CDC_E_BADARG, "catalog_topk: null pointer");
    CDC_CHECK_ARG(k >= 1 && k <= CDC_CATALOG_MAX_K, CDC_E_BADARG, "catalog_topk: k=%d lies outside [1, %d]", k, CDC_CATALOG_MAX_K);
    CDC_CHECK_ARG(ld_catalog >= 1, CDC_E_BADARG, "catalog_topk: bad sizes ld_catalog=%ld", (long)ld_catalog);
    const int rc = cat_tile_ok("catalog_topk", U, I, u0, Ub, i0, Ib);
    if (rc != 0) return rc;
    CDC_CHECK_ARG((seen_start == nullptr) == (seen_item == nullptr) && n_seen >= 0 && n_seen < (1ll << 31) && (seen_start || n_seen == 0),
                  CDC_E_BADARG, "catalog_topk: the seen set is seen_start AND seen_item with 0 <= n_seen < 2^31, or neither");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (Ib & 3) == 0 && (((uintptr_t)score) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_catalog_topk<true>, dim3((uint32_t)Ub), dim3(CAT_THREADS), 0, st, score, catalog_id, ld_catalog, u0, (int32_t)i0,
                           (int32_t)Ib, seen_start, seen_item, n_seen, k, item, cat, out_score, n, err_flag);
    else
        hipLaunchKernelGGL(k_catalog_topk<false>, dim3((uint32_t)Ub), dim3(CAT_THREADS), 0, st, score, catalog_id, ld_catalog, u0, (int32_t)i0,
                           (int32_t)Ib, seen_start, seen_item, n_seen, k, item, cat, out_score, n, err_flag);
    CDC_LAUNCH_CHECK("catalog_topk");
    return 0;
}
