// metrics.hip — evaluation metrics of the reference's test loop on the device.
//
// Stands in for run.py:684-711 (Run.test / evaluate_multi_domain): sklearn.metrics.roc_auc_score and log_loss over the
// whole evaluation set and per domain (pandas groupby).  The reference moves every batch's predictions to the host and
// computes there; here predictions stay on the GPU and one call returns all figures.
//
//   AUC  = Mann-Whitney U with mid-ranks (ties share the average rank) — what roc_auc_score's trapezoid over the ROC
//          curve equals.  Rank sums are accumulated as INTEGERS (twice the mid-rank), so the result does not depend on
//          the order of accumulation: (S2/2 - P(P+1)/2) / (P*N) is formed once, in double.
//   loss = -mean(log(y ? p : 1-p)) with sklearn 1.7's arithmetic: 1-p and the clip to [eps, 1-eps] in float32 (the dtype
//          of the predictions), logarithm and mean in double; one workgroup per domain sums its contiguous, sorted
//          segment in a fixed order.
//
// Every row is keyed twice — (its domain, score) and (pseudo-domain n_domain = "all rows", score) — and ONE radix sort
// (rocPRIM) of the 2n keys lays out every domain's rows, and the whole set, as contiguous score-ordered segments.
#include <algorithm>
#include <cstring>
#include "common.h"
#include <rocprim/rocprim.hpp>

#define MET_THREADS 256
#define MET_LOSS_THREADS 1024

// score_key (monotone float -> uint32): common.h, shared with catalog.hip
__device__ __forceinline__ float key_score(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t* a, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t upper_bound_u64(const uint64_t* a, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// What every evaluation call below shares.  On the device: a family's key kernel keeps its own "bad row" predicate and what it
// puts in place of a bad score, and uses these for the rest.
// the error word (the caller has checked that one was passed): the largest bad row + 1, saturated; a maximum, so order-free
__device__ __forceinline__ void met_flag_row(int32_t* err, int64_t i) { atomicMax(err, (int32_t)(i < 0x7ffffffe ? i + 1 : 0x7fffffff)); }
// an id out of range is clamped whether or not the flag is wanted: the id becomes the upper half of a key, and that indexes start[]
// (a user: user_weight)
template <class T>
__device__ __forceinline__ T met_clamp_id(T v, T n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// row i twice: under its own segment (or group) `up` and under the one of the pseudo-domain "all rows", up_all
__device__ __forceinline__ void met_write_pair(uint64_t* keys, int64_t n, int64_t i, uint64_t up, uint64_t up_all, int shift,
                                               uint64_t low) {
    keys[i] = (up << shift) | low;
    keys[n + i] = (up_all << shift) | low;
}
// the same with the sort's payload: the label byte, or the copy index j in [0, 2n)
template <class V>
__device__ __forceinline__ void met_write_pair(uint64_t* keys, V* pay, int64_t n, int64_t i, uint64_t up, uint64_t up_all, int shift, uint64_t low,
                                               V pay_own, V pay_all) {
    keys[i] = (up << shift) | low;         // written out, not the call above: through two levels of inlining the compiler keeps
    keys[n + i] = (up_all << shift) | low; // keys + n in registers of its own
    pay[i] = pay_own;
    pay[n + i] = pay_all;
}
// first sorted position of segment t, whose keys begin at first_key (not looked at for t = n_seg: the end of the array)
template <class T>
__device__ __forceinline__ int64_t met_seg_start(const uint64_t* keys, int64_t n2, T t, int32_t n_seg, uint64_t first_key) {
    return t == n_seg ? n2 : lower_bound_u64(keys, 0, n2, first_key);
}

// On the host: the workspace of every call is a chain of 256-byte aligned regions — the unsorted and the sorted keys, their payloads,
// start[], the family's own arrays, then rocPRIM's temporary storage.  Everything in front of the temporary storage is plain
// arithmetic, and the argument checks use it before any HIP or rocPRIM call.
static int64_t align_up(int64_t v) { return (v + 255) & ~(int64_t)255; }

struct MetCursor {
    int64_t off = 0;
    int64_t take(int64_t bytes) { const int64_t at = off; off += align_up(bytes); return at; }
};
struct MetWs {
    char* base;
    template <class T> T* ptr(int64_t off) const { return (T*)(base + off); }
};
struct MetLayout {                      // the part every family's layout embeds
    int64_t keys_in, keys_out, pay_in, pay_out, start, temp, temp_bytes, total;
    void keys(MetCursor& c, int64_t n_keys, int pay_width) {               // pay_width 0: the sort carries no payload
        keys_in = c.take(n_keys * 8);
        keys_out = c.take(n_keys * 8);
        pay_in = c.take(n_keys * pay_width);
        pay_out = c.take(n_keys * pay_width);
    }
    void starts(MetCursor& c, int64_t n_seg) { start = c.take((n_seg + 1) * 8); }
    void end_fixed(const MetCursor& c) { temp = total = c.off; temp_bytes = 0; }
    void set_temp(int64_t bytes) { temp_bytes = bytes; total = temp + align_up(bytes); }
};

// rocPRIM over 64-bit keys, with a payload or without; temp = nullptr asks for the size of the temporary storage
template <class V>
static hipError_t met_radix(void* temp, size_t& bytes, const uint64_t* kin, uint64_t* kout, const V* vin, V* vout, size_t n, int end_bit,
                            hipStream_t st) {
    return rocprim::radix_sort_pairs(temp, bytes, kin, kout, vin, vout, n, 0, end_bit, st, false);
}
static hipError_t met_radix(void* temp, size_t& bytes, const uint64_t* kin, uint64_t* kout, size_t n, int end_bit, hipStream_t st) {
    return rocprim::radix_sort_keys(temp, bytes, kin, kout, n, 0, end_bit, st, false);
}
// the temporary storage of a call's sorts and scans: they run one after the other, so the largest need serves all
struct MetTemp {
    size_t bytes = 0;
    hipError_t e = hipSuccess;
    void seen(size_t t) { bytes = std::max(bytes, t); }
    template <class V> void sort_pairs(size_t n) {
        size_t t = 0;
        if (e == hipSuccess) e = met_radix<V>(nullptr, t, nullptr, nullptr, nullptr, nullptr, n, 64, (hipStream_t)0);
        seen(t);
    }
    void sort_keys(size_t n) {
        size_t t = 0;
        if (e == hipSuccess) e = met_radix(nullptr, t, nullptr, nullptr, n, 64, (hipStream_t)0);
        seen(t);
    }
    template <class Out, class In, class Op> void scan(In in, size_t n, Op op) {
        size_t t = 0;
        if (e == hipSuccess) e = rocprim::inclusive_scan(nullptr, t, in, (Out*)nullptr, n, op, (hipStream_t)0, false);
        seen(t);
    }
    int done(const char* what, MetLayout* m) {                             // completes a fixed layout
        if (e != hipSuccess) { cdc_set_error("%s: rocprim size query failed: %s", what, hipGetErrorString(e)); return (int)e; }
        m->set_temp((int64_t)bytes);
        return 0;
    }
};
// the sort only has to look at the bits a key can have: low_bits below the upper part + the bits of the largest upper part
static int met_end_bit(uint64_t max_upper, int low_bits) {
    int end_bit = low_bits + 1;
    while (end_bit < 64 && (max_upper >> (end_bit - low_bits)) != 0) ++end_bit;
    return end_bit;
}
// the call's main sort, keys_in -> keys_out (and, given two payload pointers, pay_in -> pay_out)
template <class... A>
static int met_sort(const char* what, char* base, const MetLayout& m, A... a) {
    size_t bytes = (size_t)m.temp_bytes;
    const hipError_t e = met_radix(base + m.temp, bytes, (const uint64_t*)(base + m.keys_in), (uint64_t*)(base + m.keys_out), a...);
    if (e != hipSuccess) { cdc_set_error("%s: radix sort failed: %s", what, hipGetErrorString(e)); return (int)e; }
    return 0;
}

#define MET_TRY(call)                   \
    do {                                \
        const int rc__ = (call);        \
        if (rc__ != 0) return rc__;     \
    } while (0)

static int met_need_domain(const char* what, const int32_t* domain, int32_t n_domain) {
    CDC_CHECK_ARG(domain || n_domain == 1, CDC_E_BADARG, "%s: n_domain=%d needs the domain column", what, n_domain);
    return 0;
}
static int met_ws_aligned(const char* what, const void* workspace) {
    CDC_CHECK_ARG((((uintptr_t)workspace) & 255) == 0, CDC_E_BADARG, "%s: workspace must be 256-byte aligned", what);
    return 0;
}
// the workspace against m->total as the fixed layout left it (no HIP or rocPRIM call has been made, so a workspace that is too
// small is refused where no device is present), then `complete` adds rocPRIM's part TO THE SAME LAYOUT, then against the new m->total
template <class F>
static int met_ws_fits(const char* what, int64_t workspace_bytes, const MetLayout* m, F complete) {
    const auto fits = [&]() -> int {
        CDC_CHECK_ARG(workspace_bytes >= m->total, CDC_E_BADARG, "%s: workspace %ld < %ld bytes", what, (long)workspace_bytes, (long)m->total);
        return 0;
    };
    MET_TRY(fits());
    MET_TRY(complete());
    return fits();
}
template <class F>
static int met_gate(const char* what, const void* workspace, int64_t workspace_bytes, const MetLayout* m, F complete) {
    MET_TRY(met_ws_aligned(what, workspace));
    return met_ws_fits(what, workspace_bytes, m, complete);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MET_THREADS) k_metric_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                             const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                             int32_t n_domain, uint64_t* __restrict__ keys,
                                                             uint8_t* __restrict__ vals, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        if (p != p || d < 0 || d >= n_domain || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
        }
        met_write_pair(keys, vals, n, i, (uint32_t)d, (uint32_t)n_domain, 32, score_key(p), (uint8_t)(y != 0), (uint8_t)(y != 0));
    }
}

// start[d] = first sorted position of (pseudo-)domain d, d in [0, n_domain + 1]; start[n_domain + 1] = 2n
__global__ void k_metric_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg, int64_t* __restrict__ start,
                                unsigned long long* __restrict__ s2, unsigned long long* __restrict__ npos) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d <= n_seg) start[d] = met_seg_start(keys, n2, d, n_seg, (uint64_t)(uint32_t)d << 32);
    if (d < n_seg) { s2[d] = 0ull; npos[d] = 0ull; }
}

// every positive row adds twice its mid-rank inside its segment: (first + last position of its score) + 2, 0-based -> 1-based
__global__ void __launch_bounds__(MET_THREADS) k_metric_ranks(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ vals,
                                                              int64_t n2, const int64_t* __restrict__ start,
                                                              unsigned long long* __restrict__ s2,
                                                              unsigned long long* __restrict__ npos) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        if (!vals[i]) continue;
        const uint64_t key = keys[i];
        const int d = (int)(key >> 32);
        const int64_t s0 = start[d], s1 = start[d + 1];
        const int64_t first = lower_bound_u64(keys, s0, i + 1, key);
        const int64_t last = upper_bound_u64(keys, i, s1, key) - 1;
        atomicAdd(&s2[d], (unsigned long long)((first - s0) + (last - s0) + 2));
        atomicAdd(&npos[d], 1ull);
    }
}

// one workgroup per segment: sum of the clipped log-loss terms in a fixed order (strided per thread, then a tree)
__global__ void __launch_bounds__(MET_LOSS_THREADS) k_metric_loss(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ vals,
                                                                  const int64_t* __restrict__ start, double* __restrict__ loss_sum) {
    __shared__ double part[MET_LOSS_THREADS];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1];
    // sklearn forms [1-p, p] and clips it in the predictions' dtype (float32); only log and mean are double
    const float eps = 1.1920928955078125e-07f, hi = 1.0f - eps;            // numpy.finfo(float32).eps
    double acc = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += MET_LOSS_THREADS) {
        const float p = key_score((uint32_t)keys[i]);
        float c = vals[i] ? p : __fsub_rn(1.0f, p);
        c = c < eps ? eps : (c > hi ? hi : c);
        acc -= log((double)c);
    }
    part[tid] = acc;
    __syncthreads();
    for (int off = MET_LOSS_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) loss_sum[d] = part[0];
}

__global__ void k_metric_final(const int64_t* __restrict__ start, const unsigned long long* __restrict__ s2,
                               const unsigned long long* __restrict__ npos, const double* __restrict__ loss_sum, int32_t n_seg,
                               double* __restrict__ out, int64_t* __restrict__ counts) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_seg) return;
    const int64_t rows = start[d + 1] - start[d];
    const int64_t P = (int64_t)npos[d], N = rows - P;
    counts[d] = rows;
    counts[n_seg + d] = P;
    double auc = __longlong_as_double(0x7ff8000000000000ll), loss = auc;        // NaN: run.py:699-704's ValueError branch
    if (rows > 0 && P > 0 && N > 0) {
        const double u = ((double)s2[d] - (double)P * (double)(P + 1)) * 0.5;   // both terms exact integers < 2^53
        auc = u / ((double)P * (double)N);
        loss = loss_sum[d] / (double)rows;
    }
    out[d] = auc;
    out[n_seg + d] = loss;
}

struct MetricLayout {
    MetLayout m;
    int64_t s2, npos, loss;
};
static void metric_fixed_layout(int64_t n, int32_t n_domain, MetricLayout* L) {
    const int64_t seg = (int64_t)n_domain + 1;
    MetCursor c;
    L->m.keys(c, 2 * n, 1);
    L->m.starts(c, seg);
    L->s2 = c.take(seg * 8);
    L->npos = c.take(seg * 8);
    L->loss = c.take(seg * 8);
    L->m.end_fixed(c);
}
static int metric_layout(int64_t n, int32_t n_domain, MetricLayout* L) {
    metric_fixed_layout(n, n_domain, L);
    MetTemp t;
    t.sort_pairs<uint8_t>((size_t)(2 * n));
    return t.done("eval_metrics", &L->m);
}

extern "C" int64_t cdc_eval_workspace_bytes(int64_t n, int32_t n_domain) {
    if (n <= 0 || n_domain <= 0) return 0;
    MetricLayout L;
    if (metric_layout(n, n_domain, &L) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_metrics(const float* pred, const int16_t* label, const int32_t* domain, int64_t ld_domain, int64_t n,
                                int32_t n_domain, double* out, int64_t* counts, int32_t* err_flag, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred && label && out && counts && workspace, CDC_E_BADARG, "eval_metrics: null pointer");
    CDC_CHECK_ARG(n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20) && (domain || n_domain == 1) && ld_domain >= 0,
                  CDC_E_BADARG, "eval_metrics: bad sizes n=%ld n_domain=%d", (long)n, n_domain);
    MetricLayout L;
    metric_fixed_layout(n, n_domain, &L);
    MET_TRY(met_ws_fits("eval_metrics", workspace_bytes, &L.m, [&] { return metric_layout(n, n_domain, &L); }));
    MET_TRY(met_ws_aligned("eval_metrics", workspace));                    // this call has always looked at the size first
    const MetWs ws{(char*)workspace};
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    uint8_t* vals_out = ws.ptr<uint8_t>(L.m.pay_out);
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    unsigned long long* s2 = ws.ptr<unsigned long long>(L.s2);
    unsigned long long* npos = ws.ptr<unsigned long long>(L.npos);
    double* loss = ws.ptr<double>(L.loss);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_metric_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, domain, ld_domain, n, n_domain,
                       ws.ptr<uint64_t>(L.m.keys_in), ws.ptr<uint8_t>(L.m.pay_in), err_flag);
    CDC_LAUNCH_CHECK("eval_metrics(keys)");
    MET_TRY(met_sort("eval_metrics", ws.base, L.m, ws.ptr<const uint8_t>(L.m.pay_in), vals_out, (size_t)n2, met_end_bit((uint64_t)n_domain, 32), st));
    hipLaunchKernelGGL(k_metric_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, keys_out, n2, seg, start, s2, npos);
    CDC_LAUNCH_CHECK("eval_metrics(starts)");
    blocks = (int)std::min<int64_t>(cdc_ceil_div(n2, MET_THREADS), 8192);
    hipLaunchKernelGGL(k_metric_ranks, dim3(blocks), dim3(MET_THREADS), 0, st, keys_out, vals_out, n2, start, s2, npos);
    CDC_LAUNCH_CHECK("eval_metrics(ranks)");
    hipLaunchKernelGGL(k_metric_loss, dim3(seg), dim3(MET_LOSS_THREADS), 0, st, keys_out, vals_out, start, loss);
    CDC_LAUNCH_CHECK("eval_metrics(loss)");
    hipLaunchKernelGGL(k_metric_final, dim3((int)cdc_ceil_div(seg, 64)), dim3(64), 0, st, start, s2, npos, loss, seg, out, counts);
    CDC_LAUNCH_CHECK("eval_metrics(final)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// GAUC (base.py:33-64, gauc_score): the AUC of every user's rows, averaged over the users that have both classes with a
// weight (the user's row count, or a caller-supplied value per user).  Per domain the groups are (domain, user) pairs, for
// the pseudo-domain "all rows" they are users — millions of sparse ids, so nothing here is indexed by a group id:
//
//   keys    every row twice, key = (d * n_user + u) << 32 | score_key; ONE radix sort over the bits a key can have lays every
//           group out as a contiguous, score-ordered run, the groups of one (pseudo-)domain next to each other
//   scan 1  (rocPRIM, one pass, elements formed on the fly from the sorted keys): for every sorted position i the first
//           position of its group h(i), the first position of its tie run f(i) (running maxima of the positions where the
//           group / the whole key changes) and cn(i) = negatives at positions <= i
//   scan 2  (rocPRIM) W = running sum of every row's share of 2U, an integer formed from scan 1 alone: a positive adds twice the
//           negatives of its group below its tie run plus the negatives of the run in front of it, a negative adds the positives
//           of its tie run in front of it — every (positive, negative) pair counts 2 when ordered, 1 when tied (by whichever
//           of the two stands later in the run), so the total per group does not depend on the order of tied rows
//   sum     a group's (2U, N, rows) are differences of W and cn between its last row and the row before its first: no
//           atomics, no per-group array.  Every (pseudo-)domain's stretch of the sorted array is cut into GAUC_SLICES equal
//           slices; one workgroup per slice adds w * U/(P*N) and w of the groups ENDING in its slice (strided per thread, then
//           a tree), a last launch adds the slices' partial sums in a tree.  The order of every addition is a function of the
//           sorted keys alone, and those do not depend on the order of the rows: same rows, same bits.
// All launches have host-known dimensions; nothing is allocated, synchronised or read back.
#define GAUC_THREADS 256
#define GAUC_SLICES 64

struct GaucScan { uint32_t h, f, cn; };
struct GaucScanOp {
    __host__ __device__ GaucScan operator()(const GaucScan& a, const GaucScan& b) const {
        GaucScan r;
        r.h = a.h > b.h ? a.h : b.h;
        r.f = a.f > b.f ? a.f : b.f;
        r.cn = a.cn + b.cn;
        return r;
    }
};
struct GaucScanIn {                     // element i of scan 1
    const uint64_t* keys;
    const uint8_t* vals;
    __host__ __device__ GaucScan operator()(uint32_t i) const {
        GaucScan r;
        const uint64_t k = keys[i], kp = i ? keys[i - 1] : 0ull;
        r.h = (i && (k >> 32) != (kp >> 32)) ? i : 0u;
        r.f = (i && k != kp) ? i : 0u;
        r.cn = vals[i] ? 0u : 1u;
        return r;
    }
};
struct GaucShareIn {                    // element i of scan 2: row i's share of its group's 2U
    const GaucScan* sc;
    const uint8_t* vals;
    __host__ __device__ unsigned long long operator()(uint32_t i) const {
        const GaucScan s = sc[i];
        const uint32_t cn_f = s.f ? sc[s.f - 1].cn : 0u;
        if (vals[i]) {
            const uint32_t cn_h = s.h ? sc[s.h - 1].cn : 0u;
            return 2ull * (cn_f - cn_h) + (s.cn - cn_f);
        }
        return (unsigned long long)(i - s.f) - (s.cn - 1u - cn_f);
    }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, GaucScanIn, GaucScan> GaucScanIt;
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, GaucShareIn, unsigned long long> GaucShareIt;

__global__ void __launch_bounds__(MET_THREADS) k_gauc_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                           const int32_t* __restrict__ user, int64_t ld_user, int64_t n_user,
                                                           const int32_t* __restrict__ domain, int64_t ld_domain, int32_t n_domain,
                                                           int64_t n, uint64_t* __restrict__ keys, uint8_t* __restrict__ vals,
                                                           int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        int64_t u = user[i * ld_user];
        const int16_t y = label[i];
        if (p != p || d < 0 || d >= n_domain || u < 0 || u >= n_user || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
            u = met_clamp_id(u, n_user);
        }
        met_write_pair(keys, vals, n, i, (uint64_t)d * (uint64_t)n_user + (uint64_t)u, (uint64_t)n_domain * (uint64_t)n_user + (uint64_t)u, 32,
                       score_key(p), (uint8_t)(y != 0), (uint8_t)(y != 0));
    }
}

// start[d] = first sorted position of (pseudo-)domain d's groups, d in [0, n_seg]; start[n_seg] = 2n
__global__ void k_gauc_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg, int64_t n_user, int64_t* __restrict__ start) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d <= n_seg) start[d] = met_seg_start(keys, n2, d, n_seg, ((uint64_t)d * (uint64_t)n_user) << 32);
}

// workgroup (d, slice): the groups of (pseudo-)domain d whose LAST row lies in the slice
__global__ void __launch_bounds__(GAUC_THREADS) k_gauc_sum(const uint64_t* __restrict__ keys, const GaucScan* __restrict__ sc,
                                                           const unsigned long long* __restrict__ W, const int64_t* __restrict__ start,
                                                           const double* __restrict__ user_weight, int64_t n_user, int64_t n2,
                                                           double* __restrict__ part, int64_t* __restrict__ part_cnt) {
    __shared__ double s_num[GAUC_THREADS], s_den[GAUC_THREADS];
    __shared__ int64_t s_in[GAUC_THREADS], s_out[GAUC_THREADS];
    const int d = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1];
    const int64_t per = (s1 - s0 + GAUC_SLICES - 1) / GAUC_SLICES;
    const int64_t a = s0 + (int64_t)sl * per, b = a + per < s1 ? a + per : s1;
    const uint64_t base = (uint64_t)d * (uint64_t)n_user;
    double num = 0.0, den = 0.0;
    int64_t n_in = 0, n_out = 0;
    for (int64_t i = a + tid; i < b; i += GAUC_THREADS) {
        const uint64_t g = keys[i] >> 32;
        if (i + 1 < n2 && (keys[i + 1] >> 32) == g) continue;              // not the last row of its group
        const GaucScan e = sc[i];
        const int64_t h = e.h;
        const int64_t rows = i - h + 1;
        const int64_t N = (int64_t)(e.cn - (h ? sc[h - 1].cn : 0u)), P = rows - N;
        if (P == 0 || N == 0) { ++n_out; continue; }
        const unsigned long long u2 = W[i] - (h ? W[h - 1] : 0ull);         // twice the Mann-Whitney U of the group
        const double auc = (double)u2 / (2.0 * (double)P * (double)N);      // exact integers below 2^53: one rounding
        const double w = user_weight ? user_weight[g - base] : (double)rows;
        num += w * auc;
        den += w;
        ++n_in;
    }
    s_num[tid] = num; s_den[tid] = den; s_in[tid] = n_in; s_out[tid] = n_out;
    __syncthreads();
    for (int off = GAUC_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_num[tid] += s_num[tid + off]; s_den[tid] += s_den[tid + off];
            s_in[tid] += s_in[tid + off];   s_out[tid] += s_out[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = ((int64_t)d * GAUC_SLICES + sl) * 2;
        part[o] = s_num[0];     part[o + 1] = s_den[0];
        part_cnt[o] = s_in[0];  part_cnt[o + 1] = s_out[0];
    }
}

__global__ void __launch_bounds__(GAUC_SLICES) k_gauc_final(const double* __restrict__ part, const int64_t* __restrict__ part_cnt,
                                                            int32_t n_seg, double* __restrict__ out, int64_t* __restrict__ counts) {
    __shared__ double s_num[GAUC_SLICES], s_den[GAUC_SLICES];
    __shared__ int64_t s_in[GAUC_SLICES], s_out[GAUC_SLICES];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t o = ((int64_t)d * GAUC_SLICES + tid) * 2;
    s_num[tid] = part[o];    s_den[tid] = part[o + 1];
    s_in[tid] = part_cnt[o]; s_out[tid] = part_cnt[o + 1];
    __syncthreads();
    for (int off = GAUC_SLICES / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_num[tid] += s_num[tid + off]; s_den[tid] += s_den[tid + off];
            s_in[tid] += s_in[tid + off];   s_out[tid] += s_out[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[d] = s_in[0] > 0 ? s_num[0] / s_den[0] : __longlong_as_double(0x7ff8000000000000ll);   // no countable group: NaN
        counts[d] = s_in[0];
        counts[n_seg + d] = s_out[0];
    }
}

struct GaucLayout {
    MetLayout m;                        // keys_in is W, the running sum of scan 2, once the sort has run
    int64_t scan, part, part_cnt;
};
static void gauc_fixed_layout(int64_t n, int32_t n_domain, GaucLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1;
    MetCursor c;
    L->m.keys(c, n2, 1);
    L->scan = c.take(n2 * (int64_t)sizeof(GaucScan));
    L->m.starts(c, seg);
    L->part = c.take(seg * GAUC_SLICES * 2 * 8);
    L->part_cnt = c.take(seg * GAUC_SLICES * 2 * 8);
    L->m.end_fixed(c);
}
// rocPRIM's temporary storage for gauc_order's sort and two scans of 2n keys; completes a layout whose m.temp the caller has placed
static int gauc_temp(int64_t n, const char* what, MetLayout* m, MetTemp t = MetTemp()) {
    const size_t n2 = (size_t)(2 * n);
    t.sort_pairs<uint8_t>(n2);
    t.scan<GaucScan>(GaucScanIt(rocprim::counting_iterator<uint32_t>(0), GaucScanIn{nullptr, nullptr}), n2, GaucScanOp());
    t.scan<unsigned long long>(GaucShareIt(rocprim::counting_iterator<uint32_t>(0), GaucShareIn{nullptr, nullptr}), n2,
                               rocprim::plus<unsigned long long>());
    return t.done(what, m);
}
static int gauc_layout(int64_t n, int32_t n_domain, GaucLayout* L) {
    gauc_fixed_layout(n, n_domain, L);
    return gauc_temp(n, "eval_gauc", &L->m);
}
// (n_domain + 1) * n_user group ids must fit the upper half of a key
static bool gauc_sizes_ok(int64_t n, int32_t n_domain, int64_t n_user) {
    return n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20) && n_user > 0 && n_user <= (1ll << 32) &&
           ((int64_t)n_domain + 1) * n_user <= (1ll << 32);
}

extern "C" int64_t cdc_eval_gauc_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_user) {
    if (!gauc_sizes_ok(n, n_domain, n_user)) return 0;
    GaucLayout L;
    if (gauc_layout(n, n_domain, &L) != 0) return -1;
    return L.m.total;
}

// keys, sort, the two scans and the segment bounds of one score vector: leaves keys_out, sc and start describing its order and W, the
// running sum of scan 2 (the caller says where: by default over the unsorted keys, dead once the sort has run; nullptr: scan 2 is
// skipped — cdc_eval_rank needs the order and scan 1 alone)
static int gauc_order(const float* pred, const int16_t* label, const int32_t* user, int64_t ld_user, int64_t n_user, const int32_t* domain,
                      int64_t ld_domain, int32_t n_domain, int64_t n, int32_t* err_flag, char* base, const GaucLayout& L,
                      unsigned long long* W, const char* what, hipStream_t st) {
    const MetWs ws{base};
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    uint8_t* vals_in = ws.ptr<uint8_t>(L.m.pay_in);
    uint8_t* vals_out = ws.ptr<uint8_t>(L.m.pay_out);
    GaucScan* sc = ws.ptr<GaucScan>(L.scan);
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    const int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_gauc_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, user, ld_user, n_user, domain, ld_domain,
                       n_domain, n, ws.ptr<uint64_t>(L.m.keys_in), vals_in, err_flag);
    CDC_LAUNCH_CHECK("eval_gauc(keys)");
    MET_TRY(met_sort(what, base, L.m, (const uint8_t*)vals_in, vals_out, (size_t)n2,
                     met_end_bit((uint64_t)seg * (uint64_t)n_user - 1, 32), st));             // the upper half holds a group id below seg * n_user
    size_t temp_bytes = (size_t)L.m.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes,
                                           GaucScanIt(rocprim::counting_iterator<uint32_t>(0), GaucScanIn{keys_out, vals_out}), sc, (size_t)n2,
                                           GaucScanOp(), st, false);
    if (e != hipSuccess) { cdc_set_error("%s: group scan failed: %s", what, hipGetErrorString(e)); return (int)e; }
    if (W) {
        temp_bytes = (size_t)L.m.temp_bytes;
        e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes, GaucShareIt(rocprim::counting_iterator<uint32_t>(0), GaucShareIn{sc, vals_out}),
                                    W, (size_t)n2, rocprim::plus<unsigned long long>(), st, false);
        if (e != hipSuccess) { cdc_set_error("%s: rank scan failed: %s", what, hipGetErrorString(e)); return (int)e; }
    }
    hipLaunchKernelGGL(k_gauc_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, (const uint64_t*)keys_out, n2, seg, n_user,
                       ws.ptr<int64_t>(L.m.start));
    CDC_LAUNCH_CHECK("eval_gauc(starts)");
    return 0;
}

extern "C" int cdc_eval_gauc(const float* pred, const int16_t* label, const int32_t* user, int64_t ld_user, int64_t n_user,
                             const int32_t* domain, int64_t ld_domain, int32_t n_domain, const double* user_weight, int64_t n,
                             double* out, int64_t* counts, int32_t* err_flag, void* workspace, int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred && label && user && out && counts && workspace, CDC_E_BADARG, "eval_gauc: null pointer");
    CDC_CHECK_ARG(n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20) && n_user > 0 && ld_user >= 0 && ld_domain >= 0,
                  CDC_E_BADARG, "eval_gauc: bad sizes n=%ld n_domain=%d n_user=%ld", (long)n, n_domain, (long)n_user);
    MET_TRY(met_need_domain("eval_gauc", domain, n_domain));
    CDC_CHECK_ARG(gauc_sizes_ok(n, n_domain, n_user), CDC_E_BADARG,
                  "eval_gauc: (n_domain + 1) * n_user = %ld * %ld group ids exceed 2^32", (long)n_domain + 1, (long)n_user);
    GaucLayout L;
    gauc_fixed_layout(n, n_domain, &L);
    MET_TRY(met_gate("eval_gauc", workspace, workspace_bytes, &L.m, [&] { return gauc_temp(n, "eval_gauc", &L.m); }));
    const MetWs ws{(char*)workspace};
    const uint64_t* keys_out = ws.ptr<const uint64_t>(L.m.keys_out);
    const GaucScan* sc = ws.ptr<const GaucScan>(L.scan);
    unsigned long long* W = ws.ptr<unsigned long long>(L.m.keys_in);
    const int64_t* start = ws.ptr<const int64_t>(L.m.start);
    double* part = ws.ptr<double>(L.part);
    int64_t* part_cnt = ws.ptr<int64_t>(L.part_cnt);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    MET_TRY(gauc_order(pred, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, ws.base, L, W, "eval_gauc", st));
    hipLaunchKernelGGL(k_gauc_sum, dim3(seg, GAUC_SLICES), dim3(GAUC_THREADS), 0, st, keys_out, sc, W, start, user_weight, n_user, n2,
                       part, part_cnt);
    CDC_LAUNCH_CHECK("eval_gauc(sum)");
    hipLaunchKernelGGL(k_gauc_final, dim3(seg), dim3(GAUC_SLICES), 0, st, part, part_cnt, seg, out, counts);
    CDC_LAUNCH_CHECK("eval_gauc(final)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-user top-K figures: NDCG@K, Recall@K, Precision@K, HitRate@K and MRR@K over GAUC's groups, every figure the EXPECTATION over
// a uniformly random order of the rows that tie in score (McSherry & Najork 2008; sklearn's ndcg_score(ignore_ties=False)).
// gauc_order() without its second scan leaves every group as one ascending score-ordered run with h, f and cn per position, so
// the group's ranking is read from its LAST row downwards:
//
//   walk    the thread that finds a group's last row i (rank 0) steps from tie run to tie run: from position p the run is
//           [sc[p].f, p], T = p - f + 1 rows at ranks [a, b) = [i - p, i - p + T), of which P_t = T - (cn(p) - cn(f - 1)) are
//           positive; the next position is f - 1 (whose scan element is the one cn(f - 1) came from: one dependent load per run).
//           It stops below the group's first row h or once a reaches the largest K: O(1) per run, at most ks[n_k-1] runs.
//   H, dcg  a run inside the top K adds the integer P_t to H, the one run that straddles K adds P_t (K - a) / T; a run with
//           positives adds (P_t / T) (D[min(b, K)] - D[a]) to the DCG.  ndcg = dcg / D[min(P, K)], recall = H / P, precision = H / K.
//   hit, mrr depend on the FIRST run with a positive alone: a later run with a positive lies behind one that is wholly inside the
//           top K or is not reached, so the product of q_t over the runs collapses to that run's q.  One loop over j < min(c, N_t + 1)
//           (N_t = T - P_t, c = min(b, K) - a) carries q_j = prod_{i<j} (N_t - i) / (T - i), pr_j and the reciprocal-rank sum from
//           one K to the next larger one; the factor at i = N_t is 0, which is the case c > N_t.
//   sum     as k_gauc_sum: every (pseudo-)domain's stretch is cut into RANK_SLICES slices, a workgroup adds w m of the groups ENDING
//           in its slice per thread, then over the threads in a fixed tree (a wave butterfly, then the waves in order); a last launch
//           adds the slices in a tree and divides.  No atomics: the same rows in any order give the same bits.
// K is clamped into [1, RANK_MAX_K] where it is read, so a launch reads at most discounts[RANK_MAX_K] whatever ks holds: the
// caller validates ks (it lives on the device, and nothing here reads it back).
#define RANK_MAX_NK 8
#define RANK_MAX_K 1024
#define RANK_FIGS 5                     // ndcg, recall, precision, hit, mrr
#define RANK_SLICES 256                 // a walk is a chain of dependent loads and divisions: more, shorter slices than k_gauc_sum's

// one group's figures m[figure][k]: the walk above from the group's last row i (e = sc[i], first row h, P positives), shared by
// k_rank_sum and k_rank_ci_pass so that both form a group's value with the same operations
template <int NK>
__device__ __forceinline__ void rank_group(const GaucScan* __restrict__ sc, const double* __restrict__ D, const int32_t (&K)[NK],
                                           const double (&DK)[NK], int64_t k_max, int64_t i, GaucScan e, int64_t h, int64_t P,
                                           double (&m)[RANK_FIGS][NK]) {
    int64_t H[NK];
    double Hf[NK], dcg[NK], hit[NK], mrr[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { H[k] = 0; Hf[k] = 0.0; dcg[k] = 0.0; hit[k] = 0.0; mrr[k] = 0.0; }
    bool first = true;
    int64_t p = i;
    while (p >= h && i - p < k_max) {
        const int64_t f = e.f;                                         // >= h: a group change is a key change
        GaucScan below;
        below.h = below.f = below.cn = 0u;
        if (f) below = sc[f - 1];
        const int64_t T = p - f + 1, a = i - p, b = a + T;
        const int64_t Nt = (int64_t)(e.cn - below.cn), Pt = T - Nt;
        if (Pt > 0) {
            const double share = (double)Pt / (double)T;
            const double Da = D[a], Db = D[b < k_max ? b : k_max];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                if (a >= K[k]) continue;
                if (b <= K[k]) {
                    H[k] += Pt;
                    dcg[k] += share * (Db - Da);                       // b <= K[k] <= k_max: Db is D[b]
                } else {
                    Hf[k] = (double)(Pt * (K[k] - a)) / (double)T;
                    dcg[k] += share * (DK[k] - Da);
                }
            }
            if (first) {
                first = false;
                double q = 1.0, pr = share, rr = 0.0;
                int64_t j = 0;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    if (a >= K[k]) continue;
                    const int64_t c = (b < K[k] ? b : K[k]) - a;
                    const int64_t lim = c < Nt + 1 ? c : Nt + 1;
                    for (; j < lim; ++j) {
                        rr += pr / (double)(a + 1 + j);
                        q *= (double)(Nt - j) / (double)(T - j);
                        if (j < Nt) pr *= (double)(Nt - j) / (double)(T - 1 - j);
                    }
                    hit[k] = 1.0 - q;
                    mrr[k] = rr;
                }
            }
        }
        e = below;
        p = f - 1;
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const double hh = (double)H[k] + Hf[k];
        m[0][k] = dcg[k] / (P < K[k] ? D[P] : DK[k]);
        m[1][k] = hh / (double)P;
        m[2][k] = hh / (double)K[k];
        m[3][k] = hit[k];
        m[4][k] = mrr[k];
    }
}

template <int NK>
__global__ void __launch_bounds__(GAUC_THREADS) k_rank_sum(const uint64_t* __restrict__ keys, const GaucScan* __restrict__ sc,
                                                           const int64_t* __restrict__ start, const double* __restrict__ user_weight,
                                                           const int32_t* __restrict__ ks, const double* __restrict__ D, int64_t n_user,
                                                           int64_t n2, double* __restrict__ part, int64_t* __restrict__ part_cnt) {
    constexpr int NV = RANK_FIGS * NK + 1;
    __shared__ double s_w[GAUC_THREADS / 64][NV];
    __shared__ int64_t s_c[GAUC_THREADS / 64][2];
    const int d = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1];
    const int64_t per = (s1 - s0 + RANK_SLICES - 1) / RANK_SLICES;
    const int64_t a0 = s0 + (int64_t)sl * per, b0 = a0 + per < s1 ? a0 + per : s1;
    const uint64_t base = (uint64_t)d * (uint64_t)n_user;
    int32_t K[NK];
    double DK[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        int32_t v = ks[k];
        v = v < 1 ? 1 : (v > RANK_MAX_K ? RANK_MAX_K : v);
        K[k] = v;
        DK[k] = D[v];
    }
    const int64_t k_max = K[NK - 1];
    double acc[RANK_FIGS][NK];
#pragma unroll
    for (int f = 0; f < RANK_FIGS; ++f)
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[f][k] = 0.0;
    double den = 0.0;
    int64_t n_in = 0, n_out = 0;
    for (int64_t i = a0 + tid; i < b0; i += GAUC_THREADS) {
        const uint64_t g = keys[i] >> 32;
        if (i + 1 < n2 && (keys[i + 1] >> 32) == g) continue;              // not the last row of its group
        const GaucScan e = sc[i];
        const int64_t h = e.h;
        const int64_t rows = i - h + 1;
        const int64_t P = rows - (int64_t)(e.cn - (h ? sc[h - 1].cn : 0u));
        if (P == 0) { ++n_out; continue; }
        double m[RANK_FIGS][NK];
        rank_group<NK>(sc, D, K, DK, k_max, i, e, h, P, m);
        const double w = user_weight ? user_weight[g - base] : 1.0;
#pragma unroll
        for (int f = 0; f < RANK_FIGS; ++f)
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[f][k] += w * m[f][k];
        den += w;
        ++n_in;
    }
    const int wv = tid >> 6;
#pragma unroll
    for (int f = 0; f < RANK_FIGS; ++f)
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const double v = wave_sum_d(acc[f][k]);
            if ((tid & 63) == 0) s_w[wv][f * NK + k] = v;
        }
    den = wave_sum_d(den);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_in += __shfl_xor(n_in, o, 64);
        n_out += __shfl_xor(n_out, o, 64);
    }
    if ((tid & 63) == 0) { s_w[wv][NV - 1] = den; s_c[wv][0] = n_in; s_c[wv][1] = n_out; }
    __syncthreads();
    const int64_t o = (int64_t)d * RANK_SLICES + sl;
    if (tid < NV) {
        double v = s_w[0][tid];
        for (int w = 1; w < GAUC_THREADS / 64; ++w) v += s_w[w][tid];
        part[o * NV + tid] = v;
    }
    if (tid < 2) {
        int64_t v = s_c[0][tid];
        for (int w = 1; w < GAUC_THREADS / 64; ++w) v += s_c[w][tid];
        part_cnt[o * 2 + tid] = v;
    }
}

// workgroup d: the tree over the slices, one sum after the other, then figure = numerator / denominator; out [RANK_FIGS, n_k, n_seg]
__global__ void __launch_bounds__(RANK_SLICES) k_rank_final(const double* __restrict__ part, const int64_t* __restrict__ part_cnt,
                                                            int32_t n_k, int32_t n_seg, double* __restrict__ out,
                                                            int64_t* __restrict__ counts) {
    __shared__ double s_v[RANK_SLICES], s_sum[RANK_FIGS * RANK_MAX_NK + 1];
    __shared__ int64_t s_in[RANK_SLICES], s_out[RANK_SLICES];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int nv = RANK_FIGS * n_k + 1;
    const int64_t o = (int64_t)d * RANK_SLICES + tid;
    s_in[tid] = part_cnt[o * 2];
    s_out[tid] = part_cnt[o * 2 + 1];
    for (int v = 0; v < nv; ++v) {
        s_v[tid] = part[o * nv + v];
        __syncthreads();
        for (int off = RANK_SLICES / 2; off > 0; off >>= 1) {
            if (tid < off) {
                s_v[tid] += s_v[tid + off];
                if (v == 0) { s_in[tid] += s_in[tid + off]; s_out[tid] += s_out[tid + off]; }
            }
            __syncthreads();
        }
        if (tid == 0) s_sum[v] = s_v[0];
        __syncthreads();
    }
    if (tid < nv - 1)                                                       // tid = figure * n_k + k
        out[(int64_t)tid * n_seg + d] = s_in[0] > 0 ? s_sum[tid] / s_sum[nv - 1] : __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) {
        counts[d] = s_in[0];
        counts[n_seg + d] = s_out[0];
    }
}

struct RankLayout {
    GaucLayout g;                       // g.m.temp / g.m.total lie behind the ones below
    int64_t part, part_cnt;
};
// the slices' sums stand between GAUC's fixed part and rocPRIM's temporary storage
static void rank_fixed_layout(int64_t n, int32_t n_domain, int32_t n_k, RankLayout* L) {
    gauc_fixed_layout(n, n_domain, &L->g);
    const int64_t seg = (int64_t)n_domain + 1;
    MetCursor c{L->g.m.temp};
    L->part = c.take(seg * RANK_SLICES * (RANK_FIGS * n_k + 1) * 8);
    L->part_cnt = c.take(seg * RANK_SLICES * 2 * 8);
    L->g.m.end_fixed(c);
}

extern "C" int64_t cdc_eval_rank_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_user, int32_t n_k) {
    if (!gauc_sizes_ok(n, n_domain, n_user) || n_k < 1 || n_k > RANK_MAX_NK) return 0;
    RankLayout L;
    rank_fixed_layout(n, n_domain, n_k, &L);
    if (gauc_temp(n, "eval_rank", &L.g.m) != 0) return -1;
    return L.g.m.total;
}

template <int NK>
static void rank_sum_launch(int seg, hipStream_t st, const uint64_t* keys, const GaucScan* sc, const int64_t* start, const double* user_weight,
                            const int32_t* ks, const double* D, int64_t n_user, int64_t n2, double* part, int64_t* part_cnt) {
    hipLaunchKernelGGL(k_rank_sum<NK>, dim3(seg, RANK_SLICES), dim3(GAUC_THREADS), 0, st, keys, sc, start, user_weight, ks, D, n_user, n2,
                       part, part_cnt);
}

extern "C" int cdc_eval_rank(const float* pred, const int16_t* label, const int32_t* user, int64_t ld_user, int64_t n_user,
                             const int32_t* domain, int64_t ld_domain, int32_t n_domain, const double* user_weight, const int32_t* ks,
                             int32_t n_k, const double* discounts, int64_t n, double* out, int64_t* counts, int32_t* err_flag,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred && label && user && ks && discounts && out && counts && workspace, CDC_E_BADARG, "eval_rank: null pointer");
    CDC_CHECK_ARG(n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20) && n_user > 0 && ld_user >= 0 && ld_domain >= 0,
                  CDC_E_BADARG, "eval_rank: bad sizes n=%ld n_domain=%d n_user=%ld", (long)n, n_domain, (long)n_user);
    CDC_CHECK_ARG(n_k >= 1 && n_k <= RANK_MAX_NK, CDC_E_BADARG, "eval_rank: n_k=%d cut-offs, 1 to %d are served", n_k, RANK_MAX_NK);
    MET_TRY(met_need_domain("eval_rank", domain, n_domain));
    CDC_CHECK_ARG(gauc_sizes_ok(n, n_domain, n_user), CDC_E_BADARG,
                  "eval_rank: (n_domain + 1) * n_user = %ld * %ld group ids exceed 2^32", (long)n_domain + 1, (long)n_user);
    RankLayout L;
    rank_fixed_layout(n, n_domain, n_k, &L);
    MET_TRY(met_gate("eval_rank", workspace, workspace_bytes, &L.g.m, [&] { return gauc_temp(n, "eval_rank", &L.g.m); }));
    const MetWs ws{(char*)workspace};
    const uint64_t* keys_out = ws.ptr<const uint64_t>(L.g.m.keys_out);
    const GaucScan* sc = ws.ptr<const GaucScan>(L.g.scan);
    const int64_t* start = ws.ptr<const int64_t>(L.g.m.start);
    double* part = ws.ptr<double>(L.part);
    int64_t* part_cnt = ws.ptr<int64_t>(L.part_cnt);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    MET_TRY(gauc_order(pred, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, ws.base, L.g, nullptr, "eval_rank", st));
    switch (n_k) {
#define RANK_CASE(NK) case NK: rank_sum_launch<NK>(seg, st, keys_out, sc, start, user_weight, ks, discounts, n_user, n2, part, part_cnt); break;
        RANK_CASE(1) RANK_CASE(2) RANK_CASE(3) RANK_CASE(4) RANK_CASE(5) RANK_CASE(6) RANK_CASE(7) RANK_CASE(8)
#undef RANK_CASE
    }
    CDC_LAUNCH_CHECK("eval_rank(sum)");
    hipLaunchKernelGGL(k_rank_final, dim3(seg), dim3(RANK_SLICES), 0, st, part, part_cnt, n_k, seg, out, counts);
    CDC_LAUNCH_CHECK("eval_rank(final)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-user top-K LISTS: for every (domain, user) group its K best-scored rows, best first, no item twice.  The order inside a group is
// total — descending score (score_key: -0.0 is +0.0), then ascending item, then ascending row index — and every step below realises
// it by a STABLE radix sort (rocPRIM) over keys that carry the row index as the value, so nothing depends on how a sort leaves ties:
//
//   keys    one key per row: group << 32 | ~score_key (no item) or group << 32 | item; a row that belongs to no list (NaN score, an
//           id out of range, a negative item) gets TOPK_DEAD = all ones, which no live row can have (~score_key of a non-NaN score is
//           below 0xff800001, an item is below 2^31) and which sorts behind every live key.  No id is clamped.
//   no item one sort over all 64 bits: a group's rows stand in rank order, equal scores in row order (the rows enter in row order).
//   item    sort 1 on (group, item) lays every (group, item) run out in row order; a segmented scan (rocPRIM, elements formed on the fly:
//           run head, ~score_key and row in one word, the operator keeps the smaller (~score_key, row) inside a run) leaves the run's
//           best row at the run's LAST position; k_topk_rekey keys that position (group << 32 | the best row's ~score_key, value = the
//           best row) and every other position TOPK_DEAD; sort 2 over these keys is the score sort — its input stands in (group, item)
//           order, so equal scores of a group come out in item order.
//   scan 1  over the sorted keys: h(i) = first position of i's group (a running maximum), g(i) = groups that begin at or before i.
//   scan 2  running count of the positions with rank i - h(i) < k: a kept row's place in the entry arrays.
//   emit    a group's first row writes the group's id and start, its last row the survivor count, every kept row its entry; the thread
//           of position n - 1 writes G, E and group_start[G].  Every output index is below n (group_start: n) by construction.
// The only atomic is err_flag's atomicMax (a maximum: order-free).  All launches have dimensions that depend on (n, item != NULL)
// alone — the sorts always cover all 64 bits, TOPK_DEAD needs them; nothing is allocated, synchronised or read back.
#define TOPK_DEAD (~0ull)

typedef unsigned long long TopkPick;    // ~score_key << 32 | row << 1 | run head: one word (a three-field struct spills in rocPRIM's scan)
struct TopkPickOp {                     // the segmented minimum of (~score_key, row); row < 2^31
    __host__ __device__ TopkPick operator()(const TopkPick& a, const TopkPick& b) const {
        if (b & 1ull) return b;
        const TopkPick m = (b >> 1) < (a >> 1) ? b : a;
        return (m & ~1ull) | (a & 1ull);
    }
};
struct TopkPickIn {                     // element i of the pick scan: position i of the (group, item) order
    const uint64_t* keys;
    const uint32_t* rows;
    const float* pred;
    __device__ TopkPick operator()(uint32_t i) const {
        const uint32_t row = rows[i];
        return ((TopkPick)~score_key(pred[row]) << 32) | ((TopkPick)row << 1) | ((i == 0 || keys[i] != keys[i - 1]) ? 1ull : 0ull);
    }
};
struct TopkScan { uint32_t h, g; };
struct TopkScanOp {
    __host__ __device__ TopkScan operator()(const TopkScan& a, const TopkScan& b) const {
        TopkScan r;
        r.h = a.h > b.h ? a.h : b.h;
        r.g = a.g + b.g;
        return r;
    }
};
struct TopkScanIn {                     // element i of scan 1
    const uint64_t* keys;
    __host__ __device__ TopkScan operator()(uint32_t i) const {
        const uint64_t k = keys[i];
        const bool head = k != TOPK_DEAD && (i == 0 || (k >> 32) != (keys[i - 1] >> 32));
        TopkScan r;
        r.h = head ? i : 0u;
        r.g = head ? 1u : 0u;
        return r;
    }
};
struct TopkKeptIn {                     // element i of scan 2: 1 when position i is among its group's first k
    const uint64_t* keys;
    const TopkScan* sc;
    uint32_t k;
    __host__ __device__ uint32_t operator()(uint32_t i) const { return (keys[i] != TOPK_DEAD && i - sc[i].h < k) ? 1u : 0u; }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, TopkPickIn, TopkPick> TopkPickIt;
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, TopkScanIn, TopkScan> TopkScanIt;
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, TopkKeptIn, uint32_t> TopkKeptIt;

template <bool ITEM>
__global__ void __launch_bounds__(MET_THREADS) k_topk_keys(const float* __restrict__ pred, const int32_t* __restrict__ user, int64_t ld_user,
                                                           int64_t n_user, const int32_t* __restrict__ domain, int64_t ld_domain,
                                                           int32_t n_domain, const int32_t* __restrict__ item, int64_t ld_item, int64_t n,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ rows,
                                                           int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        const int32_t d = domain ? domain[i * ld_domain] : 0;
        const int64_t u = user[i * ld_user];
        const int32_t it = ITEM ? item[i * ld_item] : 0;
        uint64_t key = TOPK_DEAD;
        if (p != p || d < 0 || d >= n_domain || u < 0 || u >= n_user || it < 0) {
            if (err) met_flag_row(err, i);
        } else {
            const uint64_t g = (uint64_t)d * (uint64_t)n_user + (uint64_t)u;
            key = (g << 32) | (ITEM ? (uint32_t)it : ~score_key(p));
        }
        keys[i] = key;
        rows[i] = (uint32_t)i;
    }
}

// position i of the (group, item) order -> its key and row for the score sort: the run's last position stands for the run's best row
__global__ void __launch_bounds__(MET_THREADS) k_topk_rekey(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rows,
                                                            const TopkPick* __restrict__ pick, int64_t n, uint64_t* __restrict__ keys2,
                                                            uint32_t* __restrict__ rows2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        uint64_t out = TOPK_DEAD;
        uint32_t row = rows[i];
        if (k != TOPK_DEAD && (i + 1 == n || keys[i + 1] != k)) {
            const TopkPick best = pick[i];
            out = (k & 0xffffffff00000000ull) | (best >> 32);
            row = (uint32_t)(best >> 1) & 0x7fffffffu;
        }
        keys2[i] = out;
        rows2[i] = row;
    }
}

__global__ void __launch_bounds__(MET_THREADS) k_topk_emit(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rows,
                                                           const TopkScan* __restrict__ sc, const uint32_t* __restrict__ kept,
                                                           const float* __restrict__ pred, int64_t n_user, uint32_t k, int64_t n,
                                                           int64_t* __restrict__ n_out, int32_t* __restrict__ group_domain,
                                                           int32_t* __restrict__ group_user, int32_t* __restrict__ group_start,
                                                           int32_t* __restrict__ group_rows, int32_t* __restrict__ entry_row,
                                                           float* __restrict__ entry_score) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const TopkScan s = sc[i];
        const uint32_t e = kept[i];                                        // kept positions up to and including i
        if (i == n - 1) {                                                  // s.g <= n and e <= n: group_start holds n + 1 entries
            n_out[0] = (int64_t)s.g;
            n_out[1] = (int64_t)e;
            group_start[s.g] = (int32_t)e;
        }
        if (key == TOPK_DEAD) continue;
        const uint64_t g = key >> 32;
        const uint32_t rank = (uint32_t)i - s.h, j = s.g - 1u;             // a live position lies in group j < G
        if (rank == 0) {                                                   // k >= 1: the first row is kept, it is entry e - 1
            const uint64_t d = g / (uint64_t)n_user;
            group_domain[j] = (int32_t)d;
            group_user[j] = (int32_t)(g - d * (uint64_t)n_user);
            group_start[j] = (int32_t)(e - 1u);
        }
        if (i + 1 == n || keys[i + 1] == TOPK_DEAD || (keys[i + 1] >> 32) != g) group_rows[j] = (int32_t)(rank + 1u);
        if (rank < k) {
            const uint32_t row = rows[i];
            entry_row[e - 1u] = (int32_t)row;
            entry_score[e - 1u] = pred[row];
        }
    }
}

struct TopkLayout {
    MetLayout m;                        // n keys with their rows, sorted to and fro; no start[]
    int64_t scan, kept;
};
static void topk_fixed_layout(int64_t n, int32_t has_item, TopkLayout* L) {
    MetCursor c;
    L->m.keys(c, n, 4);
    L->scan = c.take(n * (int64_t)(has_item ? sizeof(TopkPick) : sizeof(TopkScan)));                  // the pick scan, then scan 1
    L->kept = c.take(n * 4);
    L->m.end_fixed(c);
}
// rocPRIM's temporary storage for the sorts and scans of n keys
static int topk_temp(int64_t n, int32_t has_item, TopkLayout* L) {
    const size_t sz = (size_t)n;
    MetTemp t;
    t.sort_pairs<uint32_t>(sz);
    if (has_item) t.scan<TopkPick>(TopkPickIt(rocprim::counting_iterator<uint32_t>(0), TopkPickIn{nullptr, nullptr, nullptr}), sz, TopkPickOp());
    t.scan<TopkScan>(TopkScanIt(rocprim::counting_iterator<uint32_t>(0), TopkScanIn{nullptr}), sz, TopkScanOp());
    t.scan<uint32_t>(TopkKeptIt(rocprim::counting_iterator<uint32_t>(0), TopkKeptIn{nullptr, nullptr, 1u}), sz, rocprim::plus<uint32_t>());
    return t.done("eval_topk", &L->m);
}
// n_domain * n_user group ids must fit the upper half of a key
static bool topk_sizes_ok(int64_t n, int32_t n_domain, int64_t n_user) {
    return n > 0 && n < (1ll << 31) && n_domain > 0 && n_user > 0 && n_user <= (1ll << 32) && (int64_t)n_domain * n_user <= (1ll << 32);
}

extern "C" int64_t cdc_eval_topk_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_user, int32_t has_item) {
    if (!topk_sizes_ok(n, n_domain, n_user)) return 0;
    TopkLayout L;
    topk_fixed_layout(n, has_item != 0, &L);
    if (topk_temp(n, has_item != 0, &L) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_topk(const float* pred, const int32_t* user, int64_t ld_user, int64_t n_user, const int32_t* domain,
                             int64_t ld_domain, int32_t n_domain, const int32_t* item, int64_t ld_item, int32_t k, int64_t n,
                             int64_t* n_out, int32_t* group_domain, int32_t* group_user, int32_t* group_start, int32_t* group_rows,
                             int32_t* entry_row, float* entry_score, int32_t* err_flag, void* workspace, int64_t workspace_bytes,
                             void* stream) {
    CDC_CHECK_ARG(pred && user && n_out && group_domain && group_user && group_start && group_rows && entry_row && entry_score && workspace,
                  CDC_E_BADARG, "eval_topk: null pointer");
    CDC_CHECK_ARG(n > 0 && n < (1ll << 31) && n_domain > 0 && n_user > 0 && ld_user >= 0 && ld_domain >= 0 && ld_item >= 0, CDC_E_BADARG,
                  "eval_topk: bad sizes n=%ld n_domain=%d n_user=%ld", (long)n, n_domain, (long)n_user);
    CDC_CHECK_ARG(k >= 1, CDC_E_BADARG, "eval_topk: k=%d, a list holds at least one row", k);
    MET_TRY(met_need_domain("eval_topk", domain, n_domain));
    CDC_CHECK_ARG(topk_sizes_ok(n, n_domain, n_user), CDC_E_BADARG, "eval_topk: n_domain * n_user = %ld * %ld group ids exceed 2^32",
                  (long)n_domain, (long)n_user);
    const int32_t has_item = item != nullptr;
    TopkLayout L;
    topk_fixed_layout(n, has_item, &L);
    MET_TRY(met_gate("eval_topk", workspace, workspace_bytes, &L.m, [&] { return topk_temp(n, has_item, &L); }));
    const MetWs ws{(char*)workspace};
    char* base = ws.base;
    uint64_t* keys_a = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys_b = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* rows_a = ws.ptr<uint32_t>(L.m.pay_in);
    uint32_t* rows_b = ws.ptr<uint32_t>(L.m.pay_out);
    uint32_t* kept = ws.ptr<uint32_t>(L.kept);
    hipStream_t st = (hipStream_t)stream;
    const size_t sz = (size_t)n;
    const int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    size_t temp_bytes;
    hipError_t e;
    if (has_item)
        hipLaunchKernelGGL(k_topk_keys<true>, dim3(blocks), dim3(MET_THREADS), 0, st, pred, user, ld_user, n_user, domain, ld_domain, n_domain,
                           item, ld_item, n, keys_a, rows_a, err_flag);
    else
        hipLaunchKernelGGL(k_topk_keys<false>, dim3(blocks), dim3(MET_THREADS), 0, st, pred, user, ld_user, n_user, domain, ld_domain, n_domain,
                           item, ld_item, n, keys_a, rows_a, err_flag);
    CDC_LAUNCH_CHECK("eval_topk(keys)");
    MET_TRY(met_sort("eval_topk", base, L.m, (const uint32_t*)rows_a, rows_b, sz, 64, st));
    if (has_item) {
        TopkPick* pick = ws.ptr<TopkPick>(L.scan);
        temp_bytes = (size_t)L.m.temp_bytes;
        e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes, TopkPickIt(rocprim::counting_iterator<uint32_t>(0), TopkPickIn{keys_b, rows_b, pred}),
                                    pick, sz, TopkPickOp(), st, false);
        if (e != hipSuccess) { cdc_set_error("eval_topk: pick scan failed: %s", hipGetErrorString(e)); return (int)e; }
        hipLaunchKernelGGL(k_topk_rekey, dim3(blocks), dim3(MET_THREADS), 0, st, keys_b, rows_b, pick, n, keys_a, rows_a);
        CDC_LAUNCH_CHECK("eval_topk(rekey)");
        temp_bytes = (size_t)L.m.temp_bytes;
        e = met_radix(base + L.m.temp, temp_bytes, (const uint64_t*)keys_a, keys_b, (const uint32_t*)rows_a, rows_b, sz, 64, st);
        if (e != hipSuccess) { cdc_set_error("eval_topk: score sort failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    TopkScan* sc = ws.ptr<TopkScan>(L.scan);
    temp_bytes = (size_t)L.m.temp_bytes;
    e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes, TopkScanIt(rocprim::counting_iterator<uint32_t>(0), TopkScanIn{keys_b}), sc, sz,
                                TopkScanOp(), st, false);
    if (e != hipSuccess) { cdc_set_error("eval_topk: group scan failed: %s", hipGetErrorString(e)); return (int)e; }
    temp_bytes = (size_t)L.m.temp_bytes;
    e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes, TopkKeptIt(rocprim::counting_iterator<uint32_t>(0), TopkKeptIn{keys_b, sc, (uint32_t)k}),
                                kept, sz, rocprim::plus<uint32_t>(), st, false);
    if (e != hipSuccess) { cdc_set_error("eval_topk: offset scan failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(k_topk_emit, dim3(blocks), dim3(MET_THREADS), 0, st, keys_b, rows_b, sc, kept, pred, n_user, (uint32_t)k, n, n_out,
                       group_domain, group_user, group_start, group_rows, entry_row, entry_score);
    CDC_LAUNCH_CHECK("eval_topk(emit)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-segment BCE of CDC's probe evaluation (run.py:549-558): every domain's batch went through ONE eval forward, its rows
// form a contiguous segment of the [rows, n_cols] tower probabilities, and segment s is scored by column seg_col[s].  One
// workgroup per segment; the per-element loss is the expression of the step's BCE kernels (rowops.hip k_bce: ATen's, pinned
// by golden g7) in fp32, widened to double; a thread adds its strided share, a wave butterfly and a serial pass over the
// waves' sums follow — no atomics on the way to a result, the same inputs give the same bits.  A thread's loads of a round
// are issued before its logarithms.  Rows at or past seg_start[n_seg] belong to no workgroup and are never touched.
#define SEGS_THREADS 256
#define SEGS_RB 4

__global__ void __launch_bounds__(SEGS_THREADS) k_eval_segments(const float* __restrict__ probs, int64_t ld, const int16_t* __restrict__ label,
                                                                const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_col,
                                                                double* __restrict__ loss, float* __restrict__ sel_pred,
                                                                int32_t* __restrict__ seg_of_row, int32_t* __restrict__ err, int64_t rows,
                                                                int32_t n_cols) {
    __shared__ double sh[SEGS_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    // the bounds come from device memory: whatever they hold, no access leaves [0, rows) x [0, n_cols)
    int64_t s0 = seg_start[s], s1 = seg_start[s + 1];
    s0 = s0 < 0 ? 0 : (s0 > rows ? rows : s0);
    s1 = s1 < s0 ? s0 : (s1 > rows ? rows : s1);
    int32_t col = seg_col ? seg_col[s] : 0;
    col = col < 0 ? 0 : (col >= n_cols ? n_cols - 1 : col);
    double acc = 0.0;
    for (int64_t i0 = s0 + tid; i0 < s1; i0 += (int64_t)SEGS_RB * SEGS_THREADS) {
        float x[SEGS_RB];
        int16_t y[SEGS_RB];
#pragma unroll
        for (int q = 0; q < SEGS_RB; ++q) {
            const int64_t i = i0 + (int64_t)q * SEGS_THREADS;
            x[q] = i < s1 ? probs[i * ld + col] : 0.5f;
            y[q] = i < s1 ? label[i] : (int16_t)0;
        }
#pragma unroll
        for (int q = 0; q < SEGS_RB; ++q) {
            const int64_t i = i0 + (int64_t)q * SEGS_THREADS;
            if (i >= s1) continue;
            const float t = (float)y[q];
            acc += (double)((t - 1.f) * fmaxf(log1pf(-x[q]), -100.f) - t * fmaxf(logf(x[q]), -100.f));
            if (err && (x[q] != x[q] || (y[q] != 0 && y[q] != 1))) met_flag_row(err, i);
            if (sel_pred) sel_pred[i] = x[q];
            if (seg_of_row) seg_of_row[i] = s;
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int w = 0; w < SEGS_THREADS / 64; ++w) sum += sh[w];
        loss[s] = s1 > s0 ? sum / (double)(s1 - s0) : __longlong_as_double(0x7ff8000000000000ll);   // torch's mean of nothing
    }
}

extern "C" int cdc_eval_segments(const float* probs, int64_t ld_probs, const int16_t* label, const int32_t* seg_start, int32_t n_seg,
                                 const int32_t* seg_col, double* loss, float* sel_pred, int32_t* seg_of_row, int32_t* err_flag,
                                 int64_t rows, int32_t n_cols, void* stream) {
    CDC_CHECK_ARG(probs && label && seg_start && loss, CDC_E_BADARG, "eval_segments: null pointer");
    CDC_CHECK_ARG(n_seg > 0 && n_cols > 0 && ld_probs >= n_cols && rows >= 0 && rows < (1ll << 31), CDC_E_BADARG,
                  "eval_segments: bad sizes n_seg=%d n_cols=%d ld_probs=%ld rows=%ld", n_seg, n_cols, (long)ld_probs, (long)rows);
    hipLaunchKernelGGL(k_eval_segments, dim3(n_seg), dim3(SEGS_THREADS), 0, (hipStream_t)stream, probs, ld_probs, label, seg_start,
                       seg_col, loss, sel_pred, seg_of_row, err_flag, rows, n_cols);
    CDC_LAUNCH_CHECK("eval_segments");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// DeLong variance of the AUC and of the difference of two AUCs on the same rows (DeLong, DeLong & Clarke-Pearson 1988).
// Per segment (a domain's rows, or all rows) with positives x_1..x_P, negatives y_1..y_N and psi = 1 / 0.5 / 0 for > / = / <
// in score_key's order, the INTEGER placements are
//     a_i = 2 sum_j psi(x_i, y_j) in [0, 2N]          c_j = 2 sum_i psi(x_i, y_j) in [0, 2P]
// and  auc = sum a / (2 P N),   S10 = [P sum a^2 - (sum a)^2] / [P (P-1) 4 N^2],   S01 = [N sum c^2 - (sum c)^2] / [N (N-1) 4 P^2],
// var = S10 / P + S01 / N.  With a second score vector (placements b_i, e_j) the variance of auc_a - auc_b is the same formula
// on d = a - b and f = c - e: formed from the differences, never as var_a + var_b - 2 cov, which cancels when the vectors are close.
//
//   keys    every row twice, as k_metric_keys does, payload = the copy index j in [0, 2n); one radix sort per score vector
//   scan    (rocPRIM, elements formed on the fly) per sorted position: f = first position of its tie run, cp = positives at
//           positions <= i (the label is fetched through the payload)
//   runend  the last position of every tie run, stored at the run's first position
//   place   a row's placement is a difference of cp's at the bounds of its tie run and of its segment.  The second vector's
//           placements are scattered to pl_b[j]; the first vector's are formed where they are consumed
//   reduce  a workgroup walks a fixed stretch of the first vector's sorted order, adds per (segment, class) sum a, sum a^2
//           (low and high 32 bits of every square in separate 64-bit sums: a square is below 2^64, n of them below 2^95) and,
//           paired, the same of b and of d, in registers and a shuffle tree, and hands each stretch's sums over with INTEGER
//           atomic adds — associative, so the totals do not depend on any order
//   final   a thread per segment forms the numerators (< 2^126) and denominators (< 2^124) exactly in 128-bit integers,
//           converts each to double with ONE rounding, and divides
// Same rows in any order: same bits.  Launch dimensions depend on (n, n_domain, paired) alone.
#define DL_THREADS 256
#define DL_ITEMS 16                     // sorted positions per thread of the reduce launch
#define DL_NSUM 9                       // per class: (sum, low and high half of the sum of squares) of a, of b and of a - b
typedef unsigned __int128 dl_u128;

struct DlScan { uint32_t f, cp; };
struct DlScanOp {
    __host__ __device__ DlScan operator()(const DlScan& a, const DlScan& b) const {
        DlScan r;
        r.f = a.f > b.f ? a.f : b.f;
        r.cp = a.cp + b.cp;
        return r;
    }
};
struct DlScanIn {                       // element i of the scan
    const uint64_t* keys;
    const uint32_t* idx;
    const int16_t* label;
    uint32_t n;
    __host__ __device__ DlScan operator()(uint32_t i) const {
        DlScan r;
        r.f = (i && keys[i] != keys[i - 1]) ? i : 0u;
        const uint32_t j = idx[i];
        r.cp = label[j >= n ? j - n : j] != 0 ? 1u : 0u;
        return r;
    }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, DlScanIn, DlScan> DlScanIt;

__global__ void __launch_bounds__(MET_THREADS) k_delong_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                             const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                             int32_t n_domain, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ idx, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        if (p != p || d < 0 || d >= n_domain || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
        }
        met_write_pair(keys, idx, n, i, (uint32_t)d, (uint32_t)n_domain, 32, score_key(p), (uint32_t)i, (uint32_t)(n + i));
    }
}

// start[d] as k_metric_starts; with acc given, the segment's sums are cleared for the reduce launch
__global__ void k_delong_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg, int64_t* __restrict__ start,
                                unsigned long long* __restrict__ acc) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d <= n_seg) start[d] = met_seg_start(keys, n2, d, n_seg, (uint64_t)(uint32_t)d << 32);
    if (d < n_seg && acc)
        for (int k = 0; k < 2 * DL_NSUM; ++k) acc[(int64_t)d * 2 * DL_NSUM + k] = 0ull;
}

__global__ void __launch_bounds__(MET_THREADS) k_delong_runend(const DlScan* __restrict__ sc, int64_t n2, uint32_t* __restrict__ runend) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x)
        if (i + 1 == n2 || sc[i + 1].f == (uint32_t)(i + 1)) runend[sc[i].f] = (uint32_t)i;      // one writer per run
}

// placement of the row at sorted position i of the segment [s0, s1): a_i of a positive, c_j of a negative
__device__ __forceinline__ uint32_t dl_placement(const DlScan* __restrict__ sc, const uint32_t* __restrict__ runend, uint32_t i,
                                                 uint32_t s0, uint32_t s1, bool* positive) {
    const DlScan e = sc[i];
    const uint32_t f = e.f, l = runend[f];
    const uint32_t cp_s0 = s0 ? sc[s0 - 1].cp : 0u, cp_f = f ? sc[f - 1].cp : 0u, cp_l = sc[l].cp;
    const uint32_t pos_below = cp_f - cp_s0, pos_run = cp_l - cp_f;
    *positive = e.cp != (i ? sc[i - 1].cp : 0u);
    if (*positive) return 2u * ((f - s0) - pos_below) + ((l - f + 1u) - pos_run);       // negatives below the run twice + in it
    const uint32_t P = sc[s1 - 1].cp - cp_s0;
    return 2u * (P - pos_below - pos_run) + pos_run;                                    // positives above the run twice + in it
}

__global__ void __launch_bounds__(MET_THREADS) k_delong_place(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                              const DlScan* __restrict__ sc, const uint32_t* __restrict__ runend,
                                                              const int64_t* __restrict__ start, int64_t n2, uint32_t* __restrict__ pl) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(keys[i] >> 32);
        bool positive;
        pl[idx[i]] = dl_placement(sc, runend, (uint32_t)i, (uint32_t)start[d], (uint32_t)start[d + 1], &positive);
    }
}

__device__ __forceinline__ unsigned long long dl_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup b owns the sorted positions [b, b + 1) * DL_THREADS * DL_ITEMS of the FIRST score vector and adds, segment by segment,
// what they contribute to acc[segment][class: positive, negative][DL_NSUM]
template <bool PAIRED>
__global__ void __launch_bounds__(DL_THREADS) k_delong_reduce(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                              const DlScan* __restrict__ sc, const uint32_t* __restrict__ runend,
                                                              const uint32_t* __restrict__ pl_b, const int64_t* __restrict__ start,
                                                              int64_t n2, unsigned long long* __restrict__ acc) {
    constexpr int NS = PAIRED ? DL_NSUM : 3;
    __shared__ unsigned long long sh[DL_THREADS / 64][2 * DL_NSUM];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * (DL_THREADS * DL_ITEMS);
    const int64_t c1 = c0 + DL_THREADS * DL_ITEMS < n2 ? c0 + DL_THREADS * DL_ITEMS : n2;
    if (c0 >= c1) return;
    const int d_first = (int)(keys[c0] >> 32), d_last = (int)(keys[c1 - 1] >> 32);
    for (int d = d_first; d <= d_last; ++d) {                                   // uniform over the workgroup
        const int64_t s0 = start[d], s1 = start[d + 1];
        const int64_t lo = s0 > c0 ? s0 : c0, hi = s1 < c1 ? s1 : c1;
        if (lo >= hi) continue;                                                 // an empty segment
        unsigned long long s[2][NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) s[0][k] = s[1][k] = 0ull;
        for (int64_t i = lo + tid; i < hi; i += DL_THREADS) {
            bool positive;
            const unsigned long long a = dl_placement(sc, runend, (uint32_t)i, (uint32_t)s0, (uint32_t)s1, &positive);
            unsigned long long v[NS];
            v[0] = a; v[1] = (a * a) & 0xffffffffull; v[2] = (a * a) >> 32;
            if constexpr (PAIRED) {
                const unsigned long long b = pl_b[idx[i]];
                const unsigned long long df = a - b;                            // two's complement: the sum is read back signed
                const unsigned long long ad = a > b ? a - b : b - a;            // |a - b| < 2^32: its square fits 64 bits
                v[3] = b;  v[4] = (b * b) & 0xffffffffull;   v[5] = (b * b) >> 32;
                v[6] = df; v[7] = (ad * ad) & 0xffffffffull; v[8] = (ad * ad) >> 32;
            }
            const unsigned long long mp = positive ? ~0ull : 0ull, mn = ~mp;
#pragma unroll
            for (int k = 0; k < NS; ++k) { s[0][k] += v[k] & mp; s[1][k] += v[k] & mn; }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const unsigned long long w = dl_wave_sum(s[c][k]);
                if ((tid & 63) == 0) sh[tid >> 6][c * DL_NSUM + k] = w;
            }
        __syncthreads();
        if (tid < 2 * DL_NSUM && (tid % DL_NSUM) < NS) {
            unsigned long long w = 0ull;
#pragma unroll
            for (int q = 0; q < DL_THREADS / 64; ++q) w += sh[q][tid];
            if (w) atomicAdd(&acc[(int64_t)d * 2 * DL_NSUM + tid], w);
        }
        __syncthreads();
    }
}

// an unsigned 128-bit integer as the nearest double (ties to even): ONE rounding.  Above 64 bits the value is cut to its top 64
// bits with everything below OR-ed into the lowest of them — 11 bits under the rounding position, so the cut decides nothing
__device__ __forceinline__ double dl_to_double(dl_u128 v) {
    const uint64_t hi = (uint64_t)(v >> 64);
    if (hi == 0) return (double)(uint64_t)v;
    const int s = 64 - __clzll((long long)hi);
    uint64_t top = (uint64_t)(v >> s);
    if ((v & ((((dl_u128)1) << s) - 1)) != 0) top |= 1ull;
    return ldexp((double)top, s);
}
__device__ __forceinline__ dl_u128 dl_sum_sq(const unsigned long long* t) { return ((dl_u128)t[2] << 32) + (dl_u128)t[1]; }

// S10 / P + S01 / N from the exact sums of one placement vector: t1 = |sum|, t2 = sum of squares, positives then negatives.
// Roundings: numerator and denominator to double (1 each), their quotient (1), the division by P resp. N (1; P, N are exact) —
// 4 per term, each term >= 0, and the addition: the result is within (1 + 2^-53)^5 of the exact value
__device__ __forceinline__ double dl_var(uint64_t P, uint64_t N, uint64_t p1, dl_u128 p2, uint64_t n1, dl_u128 n2) {
    if (P < 2 || N < 2) return __longlong_as_double(0x7ff8000000000000ll);
    const dl_u128 num10 = (dl_u128)P * p2 - (dl_u128)p1 * (dl_u128)p1;                 // < 2^126; >= 0 (Cauchy-Schwarz)
    const dl_u128 num01 = (dl_u128)N * n2 - (dl_u128)n1 * (dl_u128)n1;
    const dl_u128 den10 = (dl_u128)(P * (P - 1)) * (dl_u128)(4 * N * N);               // each factor < 2^64
    const dl_u128 den01 = (dl_u128)(N * (N - 1)) * (dl_u128)(4 * P * P);
    const double t10 = dl_to_double(num10) / dl_to_double(den10) / (double)P;
    const double t01 = dl_to_double(num01) / dl_to_double(den01) / (double)N;
    return t10 + t01;
}

__global__ void k_delong_final(const int64_t* __restrict__ start, const DlScan* __restrict__ sc, const unsigned long long* __restrict__ acc,
                               int32_t n_seg, int32_t paired, double* __restrict__ out, int64_t* __restrict__ counts) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_seg) return;
    const int64_t s0 = start[d], s1 = start[d + 1], rows = s1 - s0;
    const uint64_t P = rows > 0 ? (uint64_t)(sc[s1 - 1].cp - (s0 ? sc[s0 - 1].cp : 0u)) : 0ull, N = (uint64_t)rows - P;
    counts[d] = rows;
    counts[n_seg + d] = (int64_t)P;
    const unsigned long long* p = acc + (int64_t)d * 2 * DL_NSUM;
    const unsigned long long* q = p + DL_NSUM;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool both = P > 0 && N > 0;
    const double pn = (double)P * (double)N;
    out[d] = both ? (double)p[0] * 0.5 / pn : nan;                                     // cdc_eval_metrics' expression
    out[n_seg + d] = dl_var(P, N, p[0], dl_sum_sq(p), q[0], dl_sum_sq(q));
    if (!paired) return;
    out[2 * n_seg + d] = both ? (double)p[3] * 0.5 / pn : nan;
    out[3 * n_seg + d] = dl_var(P, N, p[3], dl_sum_sq(p + 3), q[3], dl_sum_sq(q + 3));
    const long long dp = (long long)p[6], dq = (long long)q[6];
    out[4 * n_seg + d] = both ? (double)dp * 0.5 / pn : nan;                           // sum (a - b) / (2 P N): no cancellation of two rounded AUCs
    out[5 * n_seg + d] = dl_var(P, N, (uint64_t)(dp < 0 ? -dp : dp), dl_sum_sq(p + 6), (uint64_t)(dq < 0 ? -dq : dq), dl_sum_sq(q + 6));
}

struct DelongLayout {
    MetLayout m;                        // once the sort has run, keys_in holds the scan's (f, cp) and pay_in runend
    int64_t pl_b, acc;
};
static void delong_fixed_layout(int64_t n, int32_t n_domain, int32_t paired, DelongLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1;
    MetCursor c;
    L->m.keys(c, n2, 4);
    L->pl_b = c.take(paired ? n2 * 4 : 0);
    L->m.starts(c, seg);
    L->acc = c.take(seg * 2 * DL_NSUM * 8);
    L->m.end_fixed(c);
}
static int delong_temp(int64_t n, DelongLayout* L) {
    const size_t n2 = (size_t)(2 * n);
    MetTemp t;
    t.sort_pairs<uint32_t>(n2);
    t.scan<DlScan>(DlScanIt(rocprim::counting_iterator<uint32_t>(0), DlScanIn{nullptr, nullptr, nullptr, 0u}), n2, DlScanOp());
    return t.done("eval_auc_delong", &L->m);
}
static bool delong_sizes_ok(int64_t n, int32_t n_domain) { return n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20); }

extern "C" int64_t cdc_eval_auc_delong_workspace_bytes(int64_t n, int32_t n_domain, int32_t paired) {
    if (!delong_sizes_ok(n, n_domain)) return 0;
    DelongLayout L;
    delong_fixed_layout(n, n_domain, paired != 0, &L);
    if (delong_temp(n, &L) != 0) return -1;
    return L.m.total;
}

// sort one score vector's 2n keys, scan them, mark the tie runs' ends: leaves keys_out, idx_out, sc, runend and start describing it
static int delong_order(const float* pred, const int16_t* label, const int32_t* domain, int64_t ld_domain, int64_t n, int32_t n_domain,
                        int32_t* err_flag, const MetWs& ws, const DelongLayout& L, unsigned long long* acc, hipStream_t st) {
    char* base = ws.base;
    uint64_t* keys_in = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* idx_in = ws.ptr<uint32_t>(L.m.pay_in);
    uint32_t* idx_out = ws.ptr<uint32_t>(L.m.pay_out);
    DlScan* sc = (DlScan*)keys_in;                                  // the unsorted keys and payloads are dead once the sort has run
    uint32_t* runend = idx_in;
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_delong_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, domain, ld_domain, n, n_domain, keys_in, idx_in,
                       err_flag);
    CDC_LAUNCH_CHECK("eval_auc_delong(keys)");
    MET_TRY(met_sort("eval_auc_delong", base, L.m, (const uint32_t*)idx_in, idx_out, (size_t)n2, met_end_bit((uint64_t)n_domain, 32), st));
    hipLaunchKernelGGL(k_delong_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, keys_out, n2, seg, start, acc);
    CDC_LAUNCH_CHECK("eval_auc_delong(starts)");
    size_t temp_bytes = (size_t)L.m.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(base + L.m.temp, temp_bytes,
                                DlScanIt(rocprim::counting_iterator<uint32_t>(0), DlScanIn{keys_out, idx_out, label, (uint32_t)n}), sc,
                                (size_t)n2, DlScanOp(), st, false);
    if (e != hipSuccess) { cdc_set_error("eval_auc_delong: scan failed: %s", hipGetErrorString(e)); return (int)e; }
    blocks = (int)std::min<int64_t>(cdc_ceil_div(n2, MET_THREADS), 8192);
    hipLaunchKernelGGL(k_delong_runend, dim3(blocks), dim3(MET_THREADS), 0, st, sc, n2, runend);
    CDC_LAUNCH_CHECK("eval_auc_delong(runend)");
    return 0;
}

extern "C" int cdc_eval_auc_delong(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* domain, int64_t ld_domain,
                                   int64_t n, int32_t n_domain, double* out, int64_t* counts, int32_t* err_flag, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred_a && label && out && counts && workspace, CDC_E_BADARG, "eval_auc_delong: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_auc_delong: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    MET_TRY(met_need_domain("eval_auc_delong", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_auc_delong: n=%ld exceeds the 2^31 rows a placement counts in 32 bits", (long)n);
    const int32_t paired = pred_b != nullptr;
    DelongLayout L;
    delong_fixed_layout(n, n_domain, paired, &L);
    MET_TRY(met_gate("eval_auc_delong", workspace, workspace_bytes, &L.m, [&] { return delong_temp(n, &L); }));
    const MetWs ws{(char*)workspace};
    const uint64_t* keys = ws.ptr<const uint64_t>(L.m.keys_out);
    const uint32_t* idx = ws.ptr<const uint32_t>(L.m.pay_out);
    const DlScan* sc = ws.ptr<const DlScan>(L.m.keys_in);
    const uint32_t* runend = ws.ptr<const uint32_t>(L.m.pay_in);
    uint32_t* pl_b = ws.ptr<uint32_t>(L.pl_b);
    const int64_t* start = ws.ptr<const int64_t>(L.m.start);
    unsigned long long* acc = ws.ptr<unsigned long long>(L.acc);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    if (paired) {                                                   // the second vector first: its placements wait in pl_b
        MET_TRY(delong_order(pred_b, label, domain, ld_domain, n, n_domain, err_flag, ws, L, nullptr, st));
        const int blocks = (int)std::min<int64_t>(cdc_ceil_div(n2, MET_THREADS), 8192);
        hipLaunchKernelGGL(k_delong_place, dim3(blocks), dim3(MET_THREADS), 0, st, keys, idx, sc, runend, start, n2, pl_b);
        CDC_LAUNCH_CHECK("eval_auc_delong(place)");
    }
    MET_TRY(delong_order(pred_a, label, domain, ld_domain, n, n_domain, err_flag, ws, L, acc, st));
    const int blocks = (int)cdc_ceil_div(n2, DL_THREADS * DL_ITEMS);
    if (paired)
        hipLaunchKernelGGL(k_delong_reduce<true>, dim3(blocks), dim3(DL_THREADS), 0, st, keys, idx, sc, runend, (const uint32_t*)pl_b, start, n2, acc);
    else
        hipLaunchKernelGGL(k_delong_reduce<false>, dim3(blocks), dim3(DL_THREADS), 0, st, keys, idx, sc, runend, (const uint32_t*)nullptr, start, n2, acc);
    CDC_LAUNCH_CHECK("eval_auc_delong(reduce)");
    hipLaunchKernelGGL(k_delong_final, dim3((int)cdc_ceil_div(seg, 64)), dim3(64), 0, st, start, sc, acc, seg, paired, out, counts);
    CDC_LAUNCH_CHECK("eval_auc_delong(final)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Standard error of the log-loss and of the difference of two log-losses on the same rows.  Per segment (a domain's rows, or all
// rows) of m rows with l_i the per-row term of k_metric_loss:
//     loss = sum l / m        var = sum (l_i - loss)^2 / (m (m - 1))        (rows taken as independent, as DeLong's variance does)
// and with a second vector (terms k_i):  delta = loss_a - loss_b,  var_delta = the formula of var on d_i = l_i - k_i, centred on
// sum d / m — formed from the differences, never as var_a + var_b - 2 cov, which cancels when the two vectors are close.
//
//   keys    every row twice, as k_metric_keys does, payload = the copy index j in [0, 2n): ONE stable radix sort of the first vector
//           gives cdc_eval_metrics' order of the rows (tied keys keep their row order there too); label and pred_b of a sorted
//           position are fetched through the payload
//   pass    one workgroup per segment walks it twice in k_metric_loss' order (strided per thread, then a tree over the threads): first
//           sum l (sum k, sum d) and the positives, then — with the means broadcast through shared memory — the centred squares.
//           The first sum is k_metric_loss' sum addition for addition, so loss equals cdc_eval_metrics' figure bit for bit.  A
//           thread keeps its terms in the workspace for its second walk: the logarithms are taken once
// No floating-point atomics: every addition's order follows from the sorted order and the launch dimensions, and those depend on
// (n, n_domain) alone.
__global__ void __launch_bounds__(MET_THREADS) k_lossci_keys(const float* __restrict__ pred_a, const float* __restrict__ pred_b,
                                                             const int16_t* __restrict__ label, const int32_t* __restrict__ domain,
                                                             int64_t ld_domain, int64_t n, int32_t n_domain, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ idx, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred_a[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        bool bad = !(p >= 0.f && p <= 1.f) || (y != 0 && y != 1);           // a NaN too
        if (pred_b) { const float q = pred_b[i]; bad = bad || !(q >= 0.f && q <= 1.f); }
        if (bad || d < 0 || d >= n_domain) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
        }
        met_write_pair(keys, idx, n, i, (uint32_t)d, (uint32_t)n_domain, 32, score_key(p), (uint32_t)i, (uint32_t)(n + i));
    }
}

// k_metric_loss' term: 1 - p and the clip in float32, the logarithm in double
__device__ __forceinline__ double lossci_term(float p, bool positive) {
    const float eps = 1.1920928955078125e-07f, hi = 1.0f - eps;            // numpy.finfo(float32).eps
    float c = positive ? p : __fsub_rn(1.0f, p);
    c = c < eps ? eps : (c > hi ? hi : c);
    return -log((double)c);
}

// k_metric_loss' tree over the workgroup's threads; every thread gets the total
__device__ __forceinline__ double lossci_tree(double v, double* part, int tid) {
    part[tid] = v;
    __syncthreads();
    for (int off = MET_LOSS_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}

template <bool PAIRED>
__global__ void __launch_bounds__(MET_LOSS_THREADS) k_lossci(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                             const int16_t* __restrict__ label, const float* __restrict__ pred_b,
                                                             const int64_t* __restrict__ start, int64_t n, int32_t n_seg,
                                                             double* __restrict__ term_a, double* __restrict__ term_b,
                                                             double* __restrict__ out, int64_t* __restrict__ counts) {
    __shared__ double part[MET_LOSS_THREADS];
    __shared__ unsigned long long s_pos;
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1], rows = s1 - s0;
    if (tid == 0) s_pos = 0ull;
    double sa = 0.0, sb = 0.0, sd = 0.0;
    unsigned long long npos = 0ull;
    for (int64_t i = s0 + tid; i < s1; i += MET_LOSS_THREADS) {
        const int64_t j = idx[i], row = j >= n ? j - n : j;
        const bool positive = label[row] != 0;
        const double la = lossci_term(key_score((uint32_t)keys[i]), positive);
        sa += la;
        term_a[i] = la;
        if constexpr (PAIRED) {
            const double lb = lossci_term(pred_b[row], positive);
            sb += lb;
            sd += la - lb;
            term_b[i] = lb;
        }
        npos += positive ? 1ull : 0ull;
    }
    sa = lossci_tree(sa, part, tid);                                        // the sync inside also publishes s_pos = 0
    if constexpr (PAIRED) { sb = lossci_tree(sb, part, tid); sd = lossci_tree(sd, part, tid); }
    if (npos) atomicAdd(&s_pos, npos);                                      // an integer: no order to keep
    const double m = (double)rows;
    const double mean_a = sa / m, mean_b = sb / m, mean_d = sd / m;         // mean_a: k_metric_final's expression
    double qa = 0.0, qb = 0.0, qd = 0.0;
    for (int64_t i = s0 + tid; i < s1; i += MET_LOSS_THREADS) {           // the positions this thread wrote itself
        const double la = term_a[i];
        const double ca = la - mean_a;
        qa += ca * ca;
        if constexpr (PAIRED) {
            const double lb = term_b[i];
            const double cb = lb - mean_b, cd = (la - lb) - mean_d;
            qb += cb * cb;
            qd += cd * cd;
        }
    }
    qa = lossci_tree(qa, part, tid);
    if constexpr (PAIRED) { qb = lossci_tree(qb, part, tid); qd = lossci_tree(qd, part, tid); }
    if (tid != 0) return;
    const int64_t P = (int64_t)s_pos, N = rows - P;
    counts[d] = rows;
    counts[n_seg + d] = P;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool ok = rows > 0 && P > 0 && N > 0;                             // cdc_eval_metrics' rule; it implies rows >= 2
    const double mm = m * (double)(rows - 1);
    out[d] = ok ? mean_a : nan;
    out[n_seg + d] = ok ? qa / mm : nan;
    if constexpr (PAIRED) {
        out[2 * n_seg + d] = ok ? mean_b : nan;
        out[3 * n_seg + d] = ok ? qb / mm : nan;
        out[4 * n_seg + d] = ok ? mean_a - mean_b : nan;
        out[5 * n_seg + d] = ok ? qd / mm : nan;
    }
}

struct LossCiLayout {
    MetLayout m;                        // once the sort has run, keys_in holds the first vector's terms
    int64_t term_b;
};
static void lossci_fixed_layout(int64_t n, int32_t n_domain, int32_t paired, LossCiLayout* L) {
    const int64_t n2 = 2 * n;
    MetCursor c;
    L->m.keys(c, n2, 4);
    L->term_b = c.take(paired ? n2 * 8 : 0);
    L->m.starts(c, (int64_t)n_domain + 1);
    L->m.end_fixed(c);
}
// rocPRIM's temporary storage of a call whose only rocPRIM work is one sort of 2n keys with 32-bit payloads
static int met_pairs32_temp(int64_t n, const char* what, MetLayout* m) {
    MetTemp t;
    t.sort_pairs<uint32_t>((size_t)(2 * n));
    return t.done(what, m);
}

extern "C" int64_t cdc_eval_loss_ci_workspace_bytes(int64_t n, int32_t n_domain, int32_t paired) {
    if (!delong_sizes_ok(n, n_domain)) return 0;
    LossCiLayout L;
    lossci_fixed_layout(n, n_domain, paired != 0, &L);
    if (met_pairs32_temp(n, "eval_loss_ci", &L.m) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_loss_ci(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* domain, int64_t ld_domain,
                                int64_t n, int32_t n_domain, double* out, int64_t* counts, int32_t* err_flag, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred_a && label && out && counts && workspace, CDC_E_BADARG, "eval_loss_ci: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_loss_ci: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    MET_TRY(met_need_domain("eval_loss_ci", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_loss_ci: n=%ld exceeds the 2^31 rows a sorted position counts in 32 bits", (long)n);
    const int32_t paired = pred_b != nullptr;
    LossCiLayout L;
    lossci_fixed_layout(n, n_domain, paired, &L);
    MET_TRY(met_gate("eval_loss_ci", workspace, workspace_bytes, &L.m, [&] { return met_pairs32_temp(n, "eval_loss_ci", &L.m); }));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_in = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* idx_in = ws.ptr<uint32_t>(L.m.pay_in);
    uint32_t* idx_out = ws.ptr<uint32_t>(L.m.pay_out);
    double* term_a = (double*)keys_in;                              // the unsorted keys are dead once the sort has run
    double* term_b = ws.ptr<double>(L.term_b);
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    const int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_lossci_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred_a, pred_b, label, domain, ld_domain, n, n_domain, keys_in,
                       idx_in, err_flag);
    CDC_LAUNCH_CHECK("eval_loss_ci(keys)");
    MET_TRY(met_sort("eval_loss_ci", ws.base, L.m, (const uint32_t*)idx_in, idx_out, (size_t)n2, met_end_bit((uint64_t)n_domain, 32), st));
    hipLaunchKernelGGL(k_delong_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, (const uint64_t*)keys_out, n2, seg, start,
                       (unsigned long long*)nullptr);
    CDC_LAUNCH_CHECK("eval_loss_ci(starts)");
    if (paired)
        hipLaunchKernelGGL(k_lossci<true>, dim3(seg), dim3(MET_LOSS_THREADS), 0, st, (const uint64_t*)keys_out, (const uint32_t*)idx_out, label,
                           pred_b, (const int64_t*)start, n, seg, term_a, term_b, out, counts);
    else
        hipLaunchKernelGGL(k_lossci<false>, dim3(seg), dim3(MET_LOSS_THREADS), 0, st, (const uint64_t*)keys_out, (const uint32_t*)idx_out, label,
                           (const float*)nullptr, (const int64_t*)start, n, seg, term_a, (double*)nullptr, out, counts);
    CDC_LAUNCH_CHECK("eval_loss_ci(pass)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// User-clustered standard error of GAUC and of the difference of two GAUCs on the same rows.  The sampling unit is the user: per
// segment, over the K counted groups with weight w_g and AUC A_g, G = sum w A / sum w is a ratio of two sums over users, and its
// linearised variance with clusters = users is
//     var = K / (K - 1) * sum_g (w_g (A_g - G))^2 / (sum_g w_g)^2
// and, with B_g the groups' AUCs under a second vector:  delta = G_a - G_b,  var_delta = the same formula on (A_g - B_g) - delta.
//
//   order   cdc_eval_gauc's keys, sort and two scans, once per vector.  The upper key halves of the two vectors are the same multiset,
//           so a group occupies the SAME sorted positions in both orders, with the same h and cn at its ends: of the second vector's
//           order only W, the running sum of scan 2, is kept
//   pass 1  k_gauc_sum / k_gauc_final as cdc_eval_gauc launches them, once per vector (the second with its own W): G and G_b, the
//           first cdc_eval_gauc's figure bit for bit
//   pass 2  the same slices: the workgroup that finds a group's last row reads (W_a, W_b) there, forms A_g (B_g, A_g - B_g), reads G
//           from device memory and adds the centred squares strided per thread, then in a tree; a last launch adds the slices' sums
//           (and, again, the slices' sum w) in a tree and forms the variances
// No per-group array, nothing indexed by a user id, no atomics on the way to a result: the order of every addition is a function of
// the sorted keys alone — same rows, same bits.  The launch dimensions depend on (n, n_domain, paired) alone.
template <bool PAIRED>
__global__ void __launch_bounds__(GAUC_THREADS) k_gauc_ci_sq(const uint64_t* __restrict__ keys, const GaucScan* __restrict__ sc,
                                                             const unsigned long long* __restrict__ W,
                                                             const unsigned long long* __restrict__ W_b, const int64_t* __restrict__ start,
                                                             const double* __restrict__ user_weight, int64_t n_user, int64_t n2,
                                                             int32_t n_seg, const double* __restrict__ out, double* __restrict__ part_sq) {
    __shared__ double s_sq[3][GAUC_THREADS];
    const int d = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1];
    const int64_t per = (s1 - s0 + GAUC_SLICES - 1) / GAUC_SLICES;
    const int64_t a = s0 + (int64_t)sl * per, b = a + per < s1 ? a + per : s1;
    const uint64_t base = (uint64_t)d * (uint64_t)n_user;
    const double G = out[d], G_b = PAIRED ? out[2 * n_seg + d] : 0.0, delta = G - G_b;     // NaN when no group is counted: then none is added
    double qa = 0.0, qb = 0.0, qd = 0.0;
    for (int64_t i = a + tid; i < b; i += GAUC_THREADS) {
        const uint64_t g = keys[i] >> 32;
        if (i + 1 < n2 && (keys[i + 1] >> 32) == g) continue;              // not the last row of its group
        const GaucScan e = sc[i];
        const int64_t h = e.h;
        const int64_t rows = i - h + 1;
        const int64_t N = (int64_t)(e.cn - (h ? sc[h - 1].cn : 0u)), P = rows - N;
        if (P == 0 || N == 0) continue;
        const double pn2 = 2.0 * (double)P * (double)N;
        const double w = user_weight ? user_weight[g - base] : (double)rows;
        const double auc = (double)(W[i] - (h ? W[h - 1] : 0ull)) / pn2;    // k_gauc_sum's expression
        const double ta = w * (auc - G);
        qa += ta * ta;
        if constexpr (PAIRED) {
            const double auc_b = (double)(W_b[i] - (h ? W_b[h - 1] : 0ull)) / pn2;
            const double tb = w * (auc_b - G_b), td = w * ((auc - auc_b) - delta);
            qb += tb * tb;
            qd += td * td;
        }
    }
    s_sq[0][tid] = qa; s_sq[1][tid] = qb; s_sq[2][tid] = qd;
    __syncthreads();
    for (int off = GAUC_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_sq[0][tid] += s_sq[0][tid + off];
            if constexpr (PAIRED) { s_sq[1][tid] += s_sq[1][tid + off]; s_sq[2][tid] += s_sq[2][tid + off]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = ((int64_t)d * GAUC_SLICES + sl) * 3;
        part_sq[o] = s_sq[0][0]; part_sq[o + 1] = s_sq[1][0]; part_sq[o + 2] = s_sq[2][0];
    }
}

// out: gauc, var (paired: gauc_b, var_b, delta, var_delta), each [n_seg]; gauc and gauc_b are in place (k_gauc_final wrote them)
__global__ void __launch_bounds__(GAUC_SLICES) k_gauc_ci_final(const double* __restrict__ part, const int64_t* __restrict__ part_cnt,
                                                               const double* __restrict__ part_sq, int32_t n_seg, int32_t paired,
                                                               double* __restrict__ out) {
    __shared__ double s_den[GAUC_SLICES], s_sq[3][GAUC_SLICES];
    __shared__ int64_t s_in[GAUC_SLICES];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t o = (int64_t)d * GAUC_SLICES + tid;
    s_den[tid] = part[2 * o + 1];
    s_in[tid] = part_cnt[2 * o];
    for (int k = 0; k < 3; ++k) s_sq[k][tid] = part_sq[3 * o + k];
    __syncthreads();
    for (int off = GAUC_SLICES / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_den[tid] += s_den[tid + off];
            s_in[tid] += s_in[tid + off];
            for (int k = 0; k < 3; ++k) s_sq[k][tid] += s_sq[k][tid + off];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int64_t K = s_in[0];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double scale = K >= 2 ? (double)K / (double)(K - 1) / (s_den[0] * s_den[0]) : nan;
    out[n_seg + d] = K >= 2 ? scale * s_sq[0][0] : nan;
    if (!paired) return;
    out[3 * n_seg + d] = K >= 2 ? scale * s_sq[1][0] : nan;
    out[4 * n_seg + d] = out[d] - out[2 * n_seg + d];                       // NaN - NaN when no group is counted
    out[5 * n_seg + d] = K >= 2 ? scale * s_sq[2][0] : nan;
}

struct GaucCiLayout {
    GaucLayout g;                       // cdc_eval_gauc's arrays; g.m.temp / g.m.total lie behind the ones below
    int64_t w_b, part_b, part_cnt_b, counts_b, part_sq;
};
static void gauc_ci_fixed_layout(int64_t n, int32_t n_domain, int32_t paired, GaucCiLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1;
    gauc_fixed_layout(n, n_domain, &L->g);
    MetCursor c{L->g.m.temp};
    L->w_b = c.take(paired ? n2 * 8 : 0);
    L->part_b = c.take(paired ? seg * GAUC_SLICES * 2 * 8 : 0);
    L->part_cnt_b = c.take(paired ? seg * GAUC_SLICES * 2 * 8 : 0);
    L->counts_b = c.take(paired ? seg * 2 * 8 : 0);
    L->part_sq = c.take(seg * GAUC_SLICES * 3 * 8);
    L->g.m.end_fixed(c);
}

extern "C" int64_t cdc_eval_gauc_ci_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_user, int32_t paired) {
    if (!gauc_sizes_ok(n, n_domain, n_user)) return 0;
    GaucCiLayout L;
    gauc_ci_fixed_layout(n, n_domain, paired != 0, &L);
    if (gauc_temp(n, "eval_gauc_ci", &L.g.m) != 0) return -1;
    return L.g.m.total;
}

extern "C" int cdc_eval_gauc_ci(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* user, int64_t ld_user,
                                int64_t n_user, const int32_t* domain, int64_t ld_domain, int32_t n_domain, const double* user_weight,
                                int64_t n, double* out, int64_t* counts, int32_t* err_flag, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    CDC_CHECK_ARG(pred_a && label && user && out && counts && workspace, CDC_E_BADARG, "eval_gauc_ci: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && n_user > 0 && ld_user >= 0 && ld_domain >= 0, CDC_E_BADARG,
                  "eval_gauc_ci: bad sizes n=%ld n_domain=%d n_user=%ld", (long)n, n_domain, (long)n_user);
    MET_TRY(met_need_domain("eval_gauc_ci", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_gauc_ci: n=%ld exceeds the 2^31 rows a sorted position counts in 32 bits", (long)n);
    CDC_CHECK_ARG(gauc_sizes_ok(n, n_domain, n_user), CDC_E_BADARG,
                  "eval_gauc_ci: (n_domain + 1) * n_user = %ld * %ld group ids exceed 2^32", (long)n_domain + 1, (long)n_user);
    const int32_t paired = pred_b != nullptr;
    GaucCiLayout L;
    gauc_ci_fixed_layout(n, n_domain, paired, &L);
    MET_TRY(met_gate("eval_gauc_ci", workspace, workspace_bytes, &L.g.m, [&] { return gauc_temp(n, "eval_gauc_ci", &L.g.m); }));
    const MetWs ws{(char*)workspace};
    char* base = ws.base;
    const uint64_t* keys = ws.ptr<const uint64_t>(L.g.m.keys_out);
    const GaucScan* sc = ws.ptr<const GaucScan>(L.g.scan);
    unsigned long long* W = ws.ptr<unsigned long long>(L.g.m.keys_in);
    unsigned long long* W_b = ws.ptr<unsigned long long>(L.w_b);
    const int64_t* start = ws.ptr<const int64_t>(L.g.m.start);
    double* part = ws.ptr<double>(L.g.part);
    int64_t* part_cnt = ws.ptr<int64_t>(L.g.part_cnt);
    double* part_b = ws.ptr<double>(L.part_b);
    int64_t* part_cnt_b = ws.ptr<int64_t>(L.part_cnt_b);
    int64_t* counts_b = ws.ptr<int64_t>(L.counts_b);
    double* part_sq = ws.ptr<double>(L.part_sq);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    if (paired) {                                                   // the second vector first: of its order only W_b stays
        MET_TRY(gauc_order(pred_b, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, base, L.g, W_b, "eval_gauc_ci", st));
    }
    MET_TRY(gauc_order(pred_a, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, base, L.g, W, "eval_gauc_ci", st));
    hipLaunchKernelGGL(k_gauc_sum, dim3(seg, GAUC_SLICES), dim3(GAUC_THREADS), 0, st, keys, sc, (const unsigned long long*)W, start,
                       user_weight, n_user, n2, part, part_cnt);
    CDC_LAUNCH_CHECK("eval_gauc_ci(sum)");
    hipLaunchKernelGGL(k_gauc_final, dim3(seg), dim3(GAUC_SLICES), 0, st, (const double*)part, (const int64_t*)part_cnt, seg, out, counts);
    CDC_LAUNCH_CHECK("eval_gauc_ci(final)");
    if (paired) {                                                   // the counts follow from the labels alone: the second set is dropped
        hipLaunchKernelGGL(k_gauc_sum, dim3(seg, GAUC_SLICES), dim3(GAUC_THREADS), 0, st, keys, sc, (const unsigned long long*)W_b, start,
                           user_weight, n_user, n2, part_b, part_cnt_b);
        CDC_LAUNCH_CHECK("eval_gauc_ci(sum b)");
        hipLaunchKernelGGL(k_gauc_final, dim3(seg), dim3(GAUC_SLICES), 0, st, (const double*)part_b, (const int64_t*)part_cnt_b, seg,
                           out + 2 * seg, counts_b);
        CDC_LAUNCH_CHECK("eval_gauc_ci(final b)");
        hipLaunchKernelGGL(k_gauc_ci_sq<true>, dim3(seg, GAUC_SLICES), dim3(GAUC_THREADS), 0, st, keys, sc, (const unsigned long long*)W,
                           (const unsigned long long*)W_b, start, user_weight, n_user, n2, seg, (const double*)out, part_sq);
    } else {
        hipLaunchKernelGGL(k_gauc_ci_sq<false>, dim3(seg, GAUC_SLICES), dim3(GAUC_THREADS), 0, st, keys, sc, (const unsigned long long*)W,
                           (const unsigned long long*)nullptr, start, user_weight, n_user, n2, seg, (const double*)out, part_sq);
    }
    CDC_LAUNCH_CHECK("eval_gauc_ci(squares)");
    hipLaunchKernelGGL(k_gauc_ci_final, dim3(seg), dim3(GAUC_SLICES), 0, st, (const double*)part, (const int64_t*)part_cnt,
                       (const double*)part_sq, seg, paired, out);
    CDC_LAUNCH_CHECK("eval_gauc_ci(variances)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Calibration per segment (a domain's rows, or all rows): mean prediction, CTR, predicted over observed CTR, Brier score, and a
// reliability table with ECE / MCE for K equal-width and K equal-mass bins.  A prediction enters every sum as the INTEGER
// q = rint(double(p) * 2^32) in [0, 2^32], so every sum is exact and no result depends on an order of accumulation.
//
//   keys    every row twice, as k_metric_keys does: key = segment << 33 | score_key << 1 | label.  Score and label come back out of
//           the key, so the radix sort carries no payload; the label in the key makes rows that tie identical
//   cells   a row's equal-width bin is min(K-1, floor(double(p) * K)) (exact for K <= 1024), its equal-mass bin follows from its rank r
//           among its segment's m rows: floor(((r+1) K - 1) / m), the b with floor(b m / K) <= r < floor((b+1) m / K).  Both are
//           non-decreasing along a segment; (segment, width bin, mass bin) is a row's CELL
//   pass    a wave owns CAL_ROUNDS rounds of 64 * CAL_ITEMS consecutive sorted keys (a lane loads its CAL_ITEMS keys as 16-byte words).
//           While a round lies inside the wave's open cell — its last key's segment and width bin match and it ends before the mass
//           bin does: one comparison per round, a division only where a cell opens — every lane adds q, the label and the two
//           halves of (q - y 2^32)^2 to registers.  Where the cell changes the wave adds the lanes' registers in a shuffle tree and
//           one lane hands them over with INTEGER atomic adds; a round with a boundary inside is walked lane by lane
//   final   a workgroup per segment, a thread per bin: bounds of a width bin by binary search on the bin index, of a mass bin by
//           rank arithmetic, count = their difference, pred_min / pred_max = the scores at the bounds; ECE's numerator
//           sum_b |sum q_b - positives_b 2^32| is one integer, added in a tree.  Every double is (numerator -> double) /
//           (denominator -> double, exact): two roundings at the most
// Same rows in any order: same bits.  Launch dimensions depend on (n, n_domain, n_bins) alone.
#define CAL_THREADS 256
#define CAL_ITEMS 4
#define CAL_ROUNDS 8
#define CAL_MAX_BINS 1024
#define CAL_SEG_OUT 8                   // mean_pred, ctr, pcoc, brier, ece, mce, ece_q, mce_q

__device__ __forceinline__ float cal_score(uint64_t key) { return key_score((uint32_t)(key >> 1)); }
__device__ __forceinline__ unsigned long long cal_quant(float p) { return (unsigned long long)rint((double)p * 4294967296.0); }
__device__ __forceinline__ int32_t cal_bin(float p, int32_t K) {
    const int32_t b = (int32_t)((double)p * (double)K);                   // p in [0, 1]: truncation is floor
    return b < K - 1 ? b : K - 1;
}

__global__ void __launch_bounds__(MET_THREADS) k_calib_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                            const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                            int32_t n_domain, uint64_t* __restrict__ keys, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        const bool bad_p = !(p >= 0.f && p <= 1.f);                       // a NaN too
        if (bad_p || d < 0 || d >= n_domain || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
            if (bad_p) p = p > 1.f ? 1.f : 0.f;                           // the bins and q are only defined on [0, 1]
        }
        met_write_pair(keys, n, i, (uint32_t)d, (uint32_t)n_domain, 33, ((uint64_t)score_key(p) << 1) | (uint64_t)(y != 0));
    }
}

// start[d] as k_metric_starts; clears the cells' sums acc_w, acc_q [n_cells][2] and the segments' acc_seg [n_seg][2]
__global__ void __launch_bounds__(MET_THREADS) k_calib_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg, int64_t n_cells,
                                                              int64_t* __restrict__ start, unsigned long long* __restrict__ acc_w,
                                                              unsigned long long* __restrict__ acc_q, unsigned long long* __restrict__ acc_seg) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_seg) start[t] = met_seg_start(keys, n2, t, n_seg, (uint64_t)t << 33);
    if (t < n_seg) acc_seg[2 * t] = acc_seg[2 * t + 1] = 0ull;
    if (t < n_cells) acc_w[2 * t] = acc_w[2 * t + 1] = acc_q[2 * t] = acc_q[2 * t + 1] = 0ull;
}

struct CalSums { unsigned long long q, pos, sq_lo, sq_hi; };
struct CalCell { int32_t seg, bw, bq; int64_t q_end; };                   // q_end: the sorted position at which mass bin bq ends

__device__ __forceinline__ void cal_add(CalSums& s, uint64_t key) {
    const unsigned long long q = cal_quant(cal_score(key)), y = key & 1ull;
    const unsigned long long e = y ? 4294967296ull - q : q;               // |q - y 2^32| <= 2^32
    const unsigned long long e2 = e * e;                                  // wraps (to 0) for e = 2^32 alone: the high half is put back below
    s.q += q;
    s.pos += y;
    s.sq_lo += e2 & 0xffffffffull;
    s.sq_hi += (e2 >> 32) + ((e >> 32) << 32);
}

// the cell of the key at sorted position pos (which lies inside its segment: m >= 1)
__device__ __forceinline__ CalCell cal_cell(uint64_t key, int64_t pos, const int64_t* __restrict__ start, int32_t K) {
    CalCell c;
    c.seg = (int32_t)(key >> 33);
    const int64_t s0 = start[c.seg], m = start[c.seg + 1] - s0;
    c.bw = cal_bin(cal_score(key), K);
    c.bq = (int32_t)(((pos - s0 + 1) * K - 1) / m);                       // < 2^31 * 2^10
    c.q_end = s0 + ((int64_t)(c.bq + 1) * m) / K;
    return c;
}

__device__ __forceinline__ void cal_hand_over(const CalSums& s, const CalCell& c, int32_t K, unsigned long long* __restrict__ acc_w,
                                              unsigned long long* __restrict__ acc_q, unsigned long long* __restrict__ acc_seg) {
    const int64_t cw = ((int64_t)c.seg * K + c.bw) * 2, cq = ((int64_t)c.seg * K + c.bq) * 2;
    atomicAdd(&acc_w[cw], s.q);
    atomicAdd(&acc_q[cq], s.q);
    if (s.pos) { atomicAdd(&acc_w[cw + 1], s.pos); atomicAdd(&acc_q[cq + 1], s.pos); }
    atomicAdd(&acc_seg[2 * c.seg], s.sq_lo);
    atomicAdd(&acc_seg[2 * c.seg + 1], s.sq_hi);
}

__global__ void __launch_bounds__(CAL_THREADS) k_calib_pass(const uint64_t* __restrict__ keys, int64_t n2, const int64_t* __restrict__ start,
                                                            int32_t K, unsigned long long* __restrict__ acc_w,
                                                            unsigned long long* __restrict__ acc_q, unsigned long long* __restrict__ acc_seg) {
    constexpr int64_t ROUND = 64 * CAL_ITEMS;
    const int lane = threadIdx.x & 63;
    const int64_t w0 = ((int64_t)blockIdx.x * (CAL_THREADS / 64) + (threadIdx.x >> 6)) * (ROUND * CAL_ROUNDS);
    CalSums s = {0ull, 0ull, 0ull, 0ull};
    CalCell cur = {0, 0, 0, 0};                                           // the wave's open cell: the same in every lane
    bool open = false;
    for (int r = 0; r < CAL_ROUNDS; ++r) {
        const int64_t c0 = w0 + (int64_t)r * ROUND, c1 = c0 + ROUND;
        if (c0 >= n2) break;
        const int64_t p0 = c0 + (int64_t)lane * CAL_ITEMS;
        uint64_t k[CAL_ITEMS];
        const bool full = c1 <= n2;
        bool inside = false;
        if (full) {
            const ulonglong2* v = reinterpret_cast<const ulonglong2*>(keys + p0);      // 32-byte aligned: p0 is a multiple of CAL_ITEMS
#pragma unroll
            for (int j = 0; j < CAL_ITEMS / 2; ++j) { const ulonglong2 t = v[j]; k[2 * j] = t.x; k[2 * j + 1] = t.y; }
            const uint64_t kl = (uint64_t)__shfl((unsigned long long)k[CAL_ITEMS - 1], 63, 64);
            const int32_t seg_l = (int32_t)(kl >> 33), bw_l = cal_bin(cal_score(kl), K);
            // the keys are sorted: a round whose LAST key is in the open cell lies inside it
            inside = open && seg_l == cur.seg && bw_l == cur.bw && c1 <= cur.q_end;
            if (!inside) {
                if (open) {
                    s.q = dl_wave_sum(s.q); s.pos = dl_wave_sum(s.pos); s.sq_lo = dl_wave_sum(s.sq_lo); s.sq_hi = dl_wave_sum(s.sq_hi);
                    if (lane == 0) cal_hand_over(s, cur, K, acc_w, acc_q, acc_seg);
                    open = false;
                }
                const uint64_t kf = (uint64_t)__shfl((unsigned long long)k[0], 0, 64);
                const CalCell c = cal_cell(kf, c0, start, K);
                if (seg_l == c.seg && bw_l == c.bw && c1 <= c.q_end) {   // the round opens a cell and stays in it
                    cur = c;
                    open = inside = true;
                    s.q = s.pos = s.sq_lo = s.sq_hi = 0ull;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < CAL_ITEMS; ++j) k[j] = p0 + j < n2 ? keys[p0 + j] : 0ull;
            if (open) {
                s.q = dl_wave_sum(s.q); s.pos = dl_wave_sum(s.pos); s.sq_lo = dl_wave_sum(s.sq_lo); s.sq_hi = dl_wave_sum(s.sq_hi);
                if (lane == 0) cal_hand_over(s, cur, K, acc_w, acc_q, acc_seg);
                open = false;
            }
        }
        if (inside) {
#pragma unroll
            for (int j = 0; j < CAL_ITEMS; ++j) cal_add(s, k[j]);
            continue;
        }
        // a cell boundary inside the round (or the array's end): every lane walks its own keys
        CalSums t = {0ull, 0ull, 0ull, 0ull};
        CalCell c = {0, 0, 0, 0};
        bool have = false;
#pragma unroll
        for (int j = 0; j < CAL_ITEMS; ++j) {
            if (p0 + j >= n2) break;
            const CalCell cj = cal_cell(k[j], p0 + j, start, K);
            if (have && (cj.seg != c.seg || cj.bw != c.bw || cj.bq != c.bq)) {
                cal_hand_over(t, c, K, acc_w, acc_q, acc_seg);
                t.q = t.pos = t.sq_lo = t.sq_hi = 0ull;
            }
            c = cj;
            have = true;
            cal_add(t, k[j]);
        }
        if (have) cal_hand_over(t, c, K, acc_w, acc_q, acc_seg);
    }
    if (open) {
        s.q = dl_wave_sum(s.q); s.pos = dl_wave_sum(s.pos); s.sq_lo = dl_wave_sum(s.sq_lo); s.sq_hi = dl_wave_sum(s.sq_hi);
        if (lane == 0) cal_hand_over(s, cur, K, acc_w, acc_q, acc_seg);
    }
}

// first position in [lo, hi) (one segment) whose width bin is >= b
__device__ __forceinline__ int64_t cal_width_bound(const uint64_t* __restrict__ keys, int64_t lo, int64_t hi, int32_t b, int32_t K) {
    if (b >= K) return hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cal_bin(cal_score(keys[mid]), K) < b) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// pcoc, brier, ece and ece_q of a segment with m >= 1 (weighted) rows below 2^32 from its exact sums: P positives, Q = sum q, the
// two halves of sum (q - y 2^32)^2 and the two binnings' sum_b |sum q_b - positives_b 2^32|.  pcoc is left alone when P == 0.
// k_calib_final and the bootstrap's k_cboot_final both form their doubles here: equal sums give equal bits
__device__ __forceinline__ void cal_seg_figures(unsigned long long m, unsigned long long P, unsigned long long Q, unsigned long long sq_lo,
                                                unsigned long long sq_hi, unsigned long long gap_w, unsigned long long gap_q,
                                                double* pcoc, double* brier, double* ece, double* ece_q) {
    const double den = (double)m * 4294967296.0;                          // exact
    const dl_u128 sq = ((dl_u128)sq_hi << 32) + (dl_u128)sq_lo;           // < 2^96
    if (P > 0) *pcoc = (double)Q / ((double)P * 4294967296.0);
    *brier = dl_to_double(sq) / ((double)m * 18446744073709551616.0);
    *ece = (double)gap_w / den;
    *ece_q = (double)gap_q / den;
}

// tab_counts [2 binnings][count, positives][n_seg][K], tab_out [2][mean_pred, pos_rate][n_seg][K], tab_range [2][pred_min, pred_max][n_seg][K]
__global__ void __launch_bounds__(CAL_THREADS) k_calib_final(const uint64_t* __restrict__ keys, const int64_t* __restrict__ start,
                                                             const unsigned long long* __restrict__ acc_w,
                                                             const unsigned long long* __restrict__ acc_q,
                                                             const unsigned long long* __restrict__ acc_seg, int32_t n_seg, int32_t K,
                                                             double* __restrict__ seg_out, int64_t* __restrict__ seg_counts,
                                                             double* __restrict__ tab_out, int64_t* __restrict__ tab_counts,
                                                             float* __restrict__ tab_range) {
    __shared__ unsigned long long sh_u[4][CAL_THREADS];
    __shared__ double sh_m[2][CAL_THREADS];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = start[d], s1 = start[d + 1], m = s1 - s0, cells = (int64_t)n_seg * K;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const float nanf = __uint_as_float(0x7fc00000u);
    unsigned long long sum_q = 0ull, sum_p = 0ull, ece[2] = {0ull, 0ull};
    double mce[2] = {-1.0, -1.0};
    for (int b = tid; b < K; b += CAL_THREADS) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            int64_t lo, hi;
            if (t == 0) {
                lo = cal_width_bound(keys, s0, s1, b, K);
                hi = cal_width_bound(keys, lo, s1, b + 1, K);
            } else {
                lo = s0 + ((int64_t)b * m) / K;
                hi = s0 + ((int64_t)(b + 1) * m) / K;
            }
            const int64_t o = (int64_t)d * K + b, cnt = hi - lo;
            const unsigned long long* a = (t ? acc_q : acc_w) + 2 * o;
            const unsigned long long q = a[0], ps = a[1];
            double mean = nan, rate = nan;
            float mn = nanf, mx = nanf;
            if (cnt > 0) {
                const double den = (double)cnt * 4294967296.0;            // exact
                mean = (double)q / den;
                rate = (double)ps / (double)cnt;
                mn = cal_score(keys[lo]);
                mx = cal_score(keys[hi - 1]);
                const unsigned long long obs = ps << 32, gap = q > obs ? q - obs : obs - q;
                ece[t] += gap;
                const double g = (double)gap / den;
                mce[t] = g > mce[t] ? g : mce[t];
                if (t == 0) { sum_q += q; sum_p += ps; }
            }
            tab_counts[(2 * t) * cells + o] = cnt;
            tab_counts[(2 * t + 1) * cells + o] = (int64_t)ps;
            tab_out[(2 * t) * cells + o] = mean;
            tab_out[(2 * t + 1) * cells + o] = rate;
            tab_range[(2 * t) * cells + o] = mn;
            tab_range[(2 * t + 1) * cells + o] = mx;
        }
    }
    sh_u[0][tid] = sum_q; sh_u[1][tid] = sum_p; sh_u[2][tid] = ece[0]; sh_u[3][tid] = ece[1];
    sh_m[0][tid] = mce[0]; sh_m[1][tid] = mce[1];
    __syncthreads();
    for (int off = CAL_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sh_u[k][tid] += sh_u[k][tid + off];
#pragma unroll
            for (int k = 0; k < 2; ++k) sh_m[k][tid] = sh_m[k][tid + off] > sh_m[k][tid] ? sh_m[k][tid + off] : sh_m[k][tid];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const unsigned long long Q = sh_u[0][0], P = sh_u[1][0];
    seg_counts[d] = m;
    seg_counts[n_seg + d] = (int64_t)P;
    double o[CAL_SEG_OUT];
#pragma unroll
    for (int k = 0; k < CAL_SEG_OUT; ++k) o[k] = nan;
    if (m > 0) {
        const double den = (double)m * 4294967296.0;                      // exact
        o[0] = (double)Q / den;
        o[1] = (double)P / (double)m;
        cal_seg_figures((unsigned long long)m, P, Q, acc_seg[2 * d], acc_seg[2 * d + 1], sh_u[2][0], sh_u[3][0], &o[2], &o[3], &o[4],
                        &o[6]);
        o[5] = sh_m[0][0];
        o[7] = sh_m[1][0];
    }
#pragma unroll
    for (int k = 0; k < CAL_SEG_OUT; ++k) seg_out[(int64_t)k * n_seg + d] = o[k];
}

struct CalibLayout {
    MetLayout m;
    int64_t acc_w, acc_q, acc_seg;
};
static void calib_fixed_layout(int64_t n, int32_t n_domain, int32_t n_bins, CalibLayout* L) {
    const int64_t seg = (int64_t)n_domain + 1;
    MetCursor c;
    L->m.keys(c, 2 * n, 0);
    L->m.starts(c, seg);
    L->acc_w = c.take(seg * n_bins * 16);
    L->acc_q = c.take(seg * n_bins * 16);
    L->acc_seg = c.take(seg * 16);
    L->m.end_fixed(c);
}
// rocPRIM's temporary storage of a call whose only rocPRIM work is one sort of 2n keys without a payload
static int met_keys_temp(int64_t n, const char* what, MetLayout* m) {
    MetTemp t;
    t.sort_keys((size_t)(2 * n));
    return t.done(what, m);
}
static bool calib_sizes_ok(int64_t n, int32_t n_domain, int32_t n_bins) {
    return n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20) && n_bins >= 1 && n_bins <= CAL_MAX_BINS;
}

extern "C" int64_t cdc_eval_calibration_workspace_bytes(int64_t n, int32_t n_domain, int32_t n_bins) {
    if (!calib_sizes_ok(n, n_domain, n_bins)) return 0;
    CalibLayout L;
    calib_fixed_layout(n, n_domain, n_bins, &L);
    if (met_keys_temp(n, "eval_calibration", &L.m) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_calibration(const float* pred, const int16_t* label, const int32_t* domain, int64_t ld_domain, int64_t n,
                                    int32_t n_domain, int32_t n_bins, double* seg_out, int64_t* seg_counts, double* tab_out,
                                    int64_t* tab_counts, float* tab_range, int32_t* err_flag, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    CDC_CHECK_ARG(pred && label && seg_out && seg_counts && tab_out && tab_counts && tab_range && workspace, CDC_E_BADARG,
                  "eval_calibration: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_calibration: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    CDC_CHECK_ARG(n_bins >= 1 && n_bins <= CAL_MAX_BINS, CDC_E_BADARG, "eval_calibration: n_bins=%d outside [1, %d]", n_bins, CAL_MAX_BINS);
    MET_TRY(met_need_domain("eval_calibration", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_calibration: n=%ld exceeds the 2^31 rows whose sums fit 64 bits", (long)n);
    CalibLayout L;
    calib_fixed_layout(n, n_domain, n_bins, &L);
    MET_TRY(met_gate("eval_calibration", workspace, workspace_bytes, &L.m, [&] { return met_keys_temp(n, "eval_calibration", &L.m); }));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    unsigned long long* acc_w = ws.ptr<unsigned long long>(L.acc_w);
    unsigned long long* acc_q = ws.ptr<unsigned long long>(L.acc_q);
    unsigned long long* acc_seg = ws.ptr<unsigned long long>(L.acc_seg);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n, cells = ((int64_t)n_domain + 1) * n_bins;
    const int seg = n_domain + 1;
    int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_calib_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, domain, ld_domain, n, n_domain,
                       ws.ptr<uint64_t>(L.m.keys_in), err_flag);
    CDC_LAUNCH_CHECK("eval_calibration(keys)");
    MET_TRY(met_sort("eval_calibration", ws.base, L.m, (size_t)n2, met_end_bit((uint64_t)n_domain, 33), st));     // low part: label + 32 score bits
    hipLaunchKernelGGL(k_calib_starts, dim3((int)cdc_ceil_div(std::max<int64_t>(seg + 1, cells), MET_THREADS)), dim3(MET_THREADS), 0, st,
                       keys_out, n2, seg, cells, start, acc_w, acc_q, acc_seg);
    CDC_LAUNCH_CHECK("eval_calibration(starts)");
    blocks = (int)cdc_ceil_div(n2, (int64_t)CAL_THREADS * CAL_ITEMS * CAL_ROUNDS);
    hipLaunchKernelGGL(k_calib_pass, dim3(blocks), dim3(CAL_THREADS), 0, st, (const uint64_t*)keys_out, n2, (const int64_t*)start, n_bins,
                       acc_w, acc_q, acc_seg);
    CDC_LAUNCH_CHECK("eval_calibration(pass)");
    hipLaunchKernelGGL(k_calib_final, dim3(seg), dim3(CAL_THREADS), 0, st, (const uint64_t*)keys_out, (const int64_t*)start,
                       (const unsigned long long*)acc_w, (const unsigned long long*)acc_q, (const unsigned long long*)acc_seg, seg, n_bins,
                       seg_out, seg_counts, tab_out, tab_counts, tab_range);
    CDC_LAUNCH_CHECK("eval_calibration(final)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Isotonic recalibration per segment (a domain's rows, or all rows): the non-decreasing least-squares fit of the 0/1 labels on
// the score (pool-adjacent-violators), in canonical form — blocks in ascending score order with strictly increasing means — and
// the map it defines (constant on a block, linear between blocks, clipped outside).  The fit is integer geometry: with the rows in
// score order the block ends are the vertices of the LOWER CONVEX HULL of the points (rows so far, positives so far) taken at the
// ends of the tie groups; two means are compared as integer products, nothing is rounded before the final division.
//
//   keys    every row twice, as k_calib_keys does (key = segment << 33 | score_key << 1 | label), any finite score; the same sort
//   scan    (rocPRIM) cp = positives at sorted positions <= i.  POINT b in [0, 2n] sits in front of sorted position b and is
//           (b, positives before b); it exists where key >> 1 changes (the end of a tie group), at 0 and at 2n
//   order   all segments are ONE hull problem.  Lift segment s by a slope s * 2^33 (continuously): inside a segment nothing
//           changes, every segment boundary becomes a strictly convex corner, and the lower hull of all points is the segments'
//           hulls one after the other.  The lift is never formed: for points a < b < c the corner at b is strictly convex when b
//           is a boundary, or a or c lies outside b's segment, else when (c.y - b.y)(b.x - a.x) > (b.y - a.y)(c.x - b.x) —
//           factors below 2^31, products below 2^62.  A point carries its segment's bounds (lo = hi = x for a boundary)
//   local   a workgroup owns ISO_CHUNK consecutive points and joins spans of 1, 2, 4, .. of them in LDS; a lane finds one join,
//           all lanes copy
//   merge   ceil(log2(chunks)) launches, a workgroup per pair of adjacent spans.  Joining two hulls keeps a PREFIX of the left
//           vertex list and a SUFFIX of the right one, bridged by their common lower tangent: the last left vertex that stays a
//           strict corner against its tangent point on the right (binary search; the tangent point by binary search per probe,
//           the farther one where two are collinear, so collinear points go); a wave probes 64 candidates of either search at
//           once.  The joined list is written compactly into the other of two buffers, so every level reads plain arrays
//   emit    consecutive vertices are one block of the segment they lie in: x_lo / x_hi from the keys at its first / last
//           position, count and positives as differences, value = positives / count; start[s] = the rank of segment s's first
//           point among the vertices (every boundary is a vertex)
// Same rows in any order: same bits.  Launch dimensions and the number of launches depend on (n, n_domain) alone; a lane's serial
// work is two nested binary searches over vertex lists and its share of a copy.
#define ISO_THREADS 256
#define ISO_CHUNK 1024                  // points per workgroup of the local launch: a power of two
#define ISO_CHUNK_LOG 10

struct __attribute__((aligned(16))) IsoPt { uint32_t x, y, lo, hi; };

struct IsoLabelIn {                     // element i of the scan: the label bit of the sorted key
    const uint64_t* keys;
    __host__ __device__ uint32_t operator()(uint32_t i) const { return (uint32_t)(keys[i] & 1ull); }
};
typedef rocprim::transform_iterator<rocprim::counting_iterator<uint32_t>, IsoLabelIn, uint32_t> IsoLabelIt;

__global__ void __launch_bounds__(MET_THREADS) k_iso_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                          const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                          int32_t n_domain, uint64_t* __restrict__ keys, int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        const bool bad_p = !(fabsf(p) <= 3.4028234663852886e38f);         // NaN, +inf, -inf
        if (bad_p || d < 0 || d >= n_domain || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
            if (bad_p) p = 0.f;
        }
        met_write_pair(keys, n, i, (uint32_t)d, (uint32_t)n_domain, 33, ((uint64_t)score_key(p) << 1) | (uint64_t)(y != 0));
    }
}

// pos[s] = first sorted position of segment s, s in [0, n_seg]; pos[n_seg] = 2n
__global__ void __launch_bounds__(MET_THREADS) k_iso_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg,
                                                            int64_t* __restrict__ pos) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_seg) pos[t] = met_seg_start(keys, n2, t, n_seg, (uint64_t)t << 33);
}

// a < b < c by position: is the corner at b strictly convex (b stays a vertex between a and c)?
__device__ __forceinline__ bool iso_convex(const IsoPt& a, const IsoPt& b, const IsoPt& c) {
    if (a.x < b.lo || c.x > b.hi) return true;
    return (uint64_t)(c.y - b.y) * (uint64_t)(b.x - a.x) > (uint64_t)(b.y - a.y) * (uint64_t)(c.x - b.x);
}

// the vertex of the convex chain R[0, nr) (nr >= 1) that the lower tangent from p, left of all of R, touches: the smallest j with
// a strict corner at R[j] between p and R[j+1] — false, .., false, true, .., true along a convex chain — else the last vertex
__device__ __forceinline__ uint32_t iso_tangent(const IsoPt& p, const IsoPt* R, uint32_t nr) {
    uint32_t lo = 0, hi = nr - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const IsoPt r0 = R[mid], r1 = R[mid + 1];
        if (iso_convex(p, r0, r1)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// joins the chains L[0, nl) and R[0, nr), L left of R: L[0, keep) and R[skip, nr) are the joined chain
__device__ __forceinline__ void iso_bridge(const IsoPt* L, uint32_t nl, const IsoPt* R, uint32_t nr, uint32_t* keep, uint32_t* skip) {
    if (nl == 0 || nr == 0) { *keep = nl; *skip = 0; return; }
    uint32_t lo = 0, hi = nl - 1;                                         // L[i] stays: true, .., true, false, .., false; L[0] stays
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        const IsoPt p = L[mid], q = L[mid - 1];
        const IsoPt r = R[iso_tangent(p, R, nr)];
        if (iso_convex(q, p, r)) lo = mid; else hi = mid - 1;
    }
    const IsoPt p = L[lo];
    *keep = lo + 1;
    *skip = iso_tangent(p, R, nr);
}

// iso_bridge by a whole wave (all 64 lanes call it with the same arguments): both searches probe 64 evenly spaced candidates at once,
// a lane finding its own candidate's tangent point, so lists of up to 4096 vertices take two rounds each instead of 12 halvings
__device__ __forceinline__ void iso_bridge_wave(const IsoPt* L, uint32_t nl, const IsoPt* R, uint32_t nr, uint32_t* keep, uint32_t* skip) {
    if (nl == 0 || nr == 0) { *keep = nl; *skip = 0; return; }
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = 0, hi = nl - 1;                                         // L[lo] stays; nothing past hi does
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63) >> 6, i = lo + (lane + 1) * step;
        bool stays = false;
        if (i <= hi) {
            const IsoPt p = L[i], q = L[i - 1];
            const IsoPt r = R[iso_tangent(p, R, nr)];
            stays = iso_convex(q, p, r);
        }
        const unsigned long long gone = ~__ballot(stays);
        const uint32_t c = gone ? (uint32_t)__ffsll((long long)gone) - 1u : 64u;      // the candidates that stay come first
        const uint32_t top = lo + (c + 1) * step - 1;
        lo += c * step;
        hi = top < hi ? top : hi;
    }
    *keep = lo + 1;
    const IsoPt p = L[lo];
    uint32_t a = 0, b = nr - 1;                                           // the tangent point lies in [a, b]
    while (a < b) {
        const uint32_t step = (b - a + 63) >> 6, j = a + lane * step;     // candidate j: is the corner at R[j] strict? false, .., true, ..
        bool strict = false;
        if (j < b) {
            const IsoPt r0 = R[j], r1 = R[j + 1];
            strict = iso_convex(p, r0, r1);
        }
        const unsigned long long hit = __ballot(strict);
        if (hit) {                                                        // the first strict candidate f: the answer is in (f - step, f]
            const uint32_t f = (uint32_t)__ffsll((long long)hit) - 1u, at = a + f * step;
            a = f ? at - step + 1 : at;
            b = at;
        } else {                                                          // none of the probed corners: behind the last candidate below b
            const uint32_t last = (b - 1 - a) / step;
            a = a + last * step + 1;
        }
    }
    *skip = a;
}

__global__ void __launch_bounds__(ISO_THREADS) k_iso_local(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cp,
                                                           const int64_t* __restrict__ pos, int64_t n2, IsoPt* __restrict__ verts,
                                                           uint32_t* __restrict__ cnt) {
    __shared__ IsoPt s_v[2][ISO_CHUNK];
    __shared__ uint32_t s_n[2][ISO_CHUNK];
    __shared__ uint32_t s_keep[ISO_CHUNK / 2], s_skip[ISO_CHUNK / 2];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * ISO_CHUNK;
    for (int t = tid; t < ISO_CHUNK; t += ISO_THREADS) {
        const int64_t b = base + t;
        IsoPt q = {0u, 0u, 0u, 0u};
        bool is = false;
        if (b <= n2) {
            const uint64_t k1 = b < n2 ? keys[b] : 0ull, k0 = b > 0 ? keys[b - 1] : 0ull;
            const bool boundary = b == 0 || b == n2 || (k0 >> 33) != (k1 >> 33);
            is = boundary || (k0 >> 1) != (k1 >> 1);
            if (is) {
                q.x = (uint32_t)b;
                q.y = b > 0 ? cp[b - 1] : 0u;
                if (boundary) q.lo = q.hi = (uint32_t)b;
                else { const int64_t s = (int64_t)(k1 >> 33); q.lo = (uint32_t)pos[s]; q.hi = (uint32_t)pos[s + 1]; }
            }
        }
        s_v[0][t] = q;
        s_n[0][t] = is ? 1u : 0u;
    }
    __syncthreads();
    int cur = 0;
    for (int k = 1; k <= ISO_CHUNK_LOG; ++k) {
        const int span = 1 << k, half = span >> 1, merges = ISO_CHUNK >> k;
        const IsoPt* src = s_v[cur];
        IsoPt* dst = s_v[cur ^ 1];
        const uint32_t* nsrc = s_n[cur];
        uint32_t* ndst = s_n[cur ^ 1];
        for (int m = tid; m < merges; m += ISO_THREADS) {
            const uint32_t nl = nsrc[2 * m], nr = nsrc[2 * m + 1];
            uint32_t keep, skip;
            iso_bridge(src + m * span, nl, src + m * span + half, nr, &keep, &skip);
            s_keep[m] = keep;
            s_skip[m] = skip;
            ndst[m] = keep + nr - skip;
        }
        __syncthreads();
        for (int slot = tid; slot < ISO_CHUNK; slot += ISO_THREADS) {
            const int m = slot >> k;
            const uint32_t o = (uint32_t)(slot & (span - 1)), keep = s_keep[m], tot = ndst[m];
            if (o < keep) dst[slot] = src[slot];
            else if (o < tot) dst[slot] = src[m * span + half + s_skip[m] + (o - keep)];
        }
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t nv = s_n[cur][0];
    for (uint32_t o = tid; o < nv; o += ISO_THREADS) verts[base + o] = s_v[cur][o];
    if (tid == 0) cnt[blockIdx.x] = nv;
}

// workgroup m joins the spans 2m and 2m + 1 of src (slots entries apart, nsrc vertices each) into span m of dst
__global__ void __launch_bounds__(ISO_THREADS) k_iso_merge(const IsoPt* __restrict__ src, const uint32_t* __restrict__ nsrc,
                                                           IsoPt* __restrict__ dst, uint32_t* __restrict__ ndst, int64_t spans_in,
                                                           int64_t slots) {
    __shared__ uint32_t sh[2];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const IsoPt* L = src + 2 * m * slots;
    const IsoPt* R = L + slots;
    const uint32_t nl = nsrc[2 * m], nr = 2 * m + 1 < spans_in ? nsrc[2 * m + 1] : 0u;
    if (tid < 64) {                                                       // the first wave searches, every wave copies
        uint32_t keep, skip;
        iso_bridge_wave(L, nl, R, nr, &keep, &skip);
        if (tid == 0) {
            sh[0] = keep;
            sh[1] = skip;
            ndst[m] = keep + nr - skip;
        }
    }
    __syncthreads();
    const uint32_t keep = sh[0], skip = sh[1];
    IsoPt* out = dst + 2 * m * slots;
    for (uint32_t o = tid; o < keep; o += ISO_THREADS) out[o] = L[o];
    for (uint32_t o = tid; o < nr - skip; o += ISO_THREADS) out[keep + o] = R[skip + o];
}

__global__ void __launch_bounds__(MET_THREADS) k_iso_emit(const uint64_t* __restrict__ keys, const IsoPt* __restrict__ V,
                                                          const uint32_t* __restrict__ nv, int64_t cap, float* __restrict__ x_lo,
                                                          float* __restrict__ x_hi, int64_t* __restrict__ count,
                                                          int64_t* __restrict__ positives, double* __restrict__ value) {
    int64_t nb = (int64_t)nv[0] - 1;
    nb = nb < cap ? nb : cap;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += (int64_t)gridDim.x * blockDim.x) {
        const IsoPt a = V[j], b = V[j + 1];
        const int64_t c = (int64_t)(b.x - a.x), p = (int64_t)(b.y - a.y);
        x_lo[j] = cal_score(keys[a.x]);
        x_hi[j] = cal_score(keys[b.x - 1u]);
        count[j] = c;
        positives[j] = p;
        value[j] = (double)p / (double)c;
    }
}

// start[s] = the rank of segment s's first point among the vertices (= its first block), start[n_seg] = the number of blocks
__global__ void __launch_bounds__(MET_THREADS) k_iso_segments(const IsoPt* __restrict__ V, const uint32_t* __restrict__ nv,
                                                              const int64_t* __restrict__ pos, const uint32_t* __restrict__ cp,
                                                              int32_t n_seg, int64_t* __restrict__ start, int64_t* __restrict__ seg_rows,
                                                              int64_t* __restrict__ seg_positives) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seg) return;
    const uint32_t x = (uint32_t)pos[s];
    uint32_t lo = 0, hi = nv[0];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (V[mid].x < x) lo = mid + 1; else hi = mid;
    }
    start[s] = (int64_t)lo;
    if (s < n_seg) {
        const int64_t p0 = pos[s], p1 = pos[s + 1];
        seg_rows[s] = p1 - p0;
        seg_positives[s] = (int64_t)(p1 > 0 ? cp[p1 - 1] : 0u) - (int64_t)(p0 > 0 ? cp[p0 - 1] : 0u);
    }
}

struct IsoLayout {
    MetLayout m;                        // m.start is pos
    int64_t cp, verts_a, verts_b, cnt_a, cnt_b, chunks;
};
static void iso_fixed_layout(int64_t n, int32_t n_domain, IsoLayout* L) {
    const int64_t n2 = 2 * n;
    L->chunks = (n2 + 1 + ISO_CHUNK - 1) / ISO_CHUNK;                      // the points 0 .. 2n
    MetCursor c;
    L->m.keys(c, n2, 0);
    L->cp = c.take(n2 * 4);
    L->m.starts(c, (int64_t)n_domain + 1);
    L->verts_a = c.take(L->chunks * ISO_CHUNK * (int64_t)sizeof(IsoPt));
    L->verts_b = c.take(L->chunks * ISO_CHUNK * (int64_t)sizeof(IsoPt));
    L->cnt_a = c.take(L->chunks * 4);
    L->cnt_b = c.take(L->chunks * 4);
    L->m.end_fixed(c);
}
static int iso_temp(int64_t n, IsoLayout* L) {
    const size_t n2 = (size_t)(2 * n);
    MetTemp t;
    t.sort_keys(n2);
    t.scan<uint32_t>(IsoLabelIt(rocprim::counting_iterator<uint32_t>(0), IsoLabelIn{nullptr}), n2, rocprim::plus<uint32_t>());
    return t.done("eval_isotonic_fit", &L->m);
}
static bool iso_sizes_ok(int64_t n, int32_t n_domain) { return n > 0 && n < (1ll << 31) && n_domain > 0 && n_domain < (1 << 20); }

extern "C" int64_t cdc_eval_isotonic_max_blocks(int64_t n, int32_t n_domain) {
    return iso_sizes_ok(n, n_domain) ? 2 * n : 0;
}

extern "C" int64_t cdc_eval_isotonic_fit_workspace_bytes(int64_t n, int32_t n_domain) {
    if (!iso_sizes_ok(n, n_domain)) return 0;
    IsoLayout L;
    iso_fixed_layout(n, n_domain, &L);
    if (iso_temp(n, &L) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_isotonic_fit(const float* pred, const int16_t* label, const int32_t* domain, int64_t ld_domain, int64_t n,
                                     int32_t n_domain, int64_t* start, float* x_lo, float* x_hi, int64_t* count, int64_t* positives,
                                     double* value, int64_t cap, int64_t* seg_rows, int64_t* seg_positives, int32_t* err_flag,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred && label && start && x_lo && x_hi && count && positives && value && seg_rows && seg_positives && workspace,
                  CDC_E_BADARG, "eval_isotonic_fit: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_isotonic_fit: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    MET_TRY(met_need_domain("eval_isotonic_fit", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_isotonic_fit: n=%ld exceeds the 2^31 rows whose products fit 64 bits", (long)n);
    CDC_CHECK_ARG(cap >= 2 * n, CDC_E_BADARG, "eval_isotonic_fit: cap=%ld < 2n = %ld blocks", (long)cap, (long)(2 * n));
    IsoLayout L;
    iso_fixed_layout(n, n_domain, &L);
    MET_TRY(met_gate("eval_isotonic_fit", workspace, workspace_bytes, &L.m, [&] { return iso_temp(n, &L); }));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* cp = ws.ptr<uint32_t>(L.cp);
    int64_t* pos = ws.ptr<int64_t>(L.m.start);
    IsoPt* va = ws.ptr<IsoPt>(L.verts_a);
    IsoPt* vb = ws.ptr<IsoPt>(L.verts_b);
    uint32_t* na = ws.ptr<uint32_t>(L.cnt_a);
    uint32_t* nb = ws.ptr<uint32_t>(L.cnt_b);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_iso_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, domain, ld_domain, n, n_domain,
                       ws.ptr<uint64_t>(L.m.keys_in), err_flag);
    CDC_LAUNCH_CHECK("eval_isotonic_fit(keys)");
    MET_TRY(met_sort("eval_isotonic_fit", ws.base, L.m, (size_t)n2, met_end_bit((uint64_t)n_domain, 33), st));
    size_t temp_bytes = (size_t)L.m.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(ws.base + L.m.temp, temp_bytes, IsoLabelIt(rocprim::counting_iterator<uint32_t>(0), IsoLabelIn{keys_out}),
                                           cp, (size_t)n2, rocprim::plus<uint32_t>(), st, false);
    if (e != hipSuccess) { cdc_set_error("eval_isotonic_fit: label scan failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(k_iso_starts, dim3((int)cdc_ceil_div(seg + 1, MET_THREADS)), dim3(MET_THREADS), 0, st, (const uint64_t*)keys_out, n2, seg, pos);
    CDC_LAUNCH_CHECK("eval_isotonic_fit(starts)");
    hipLaunchKernelGGL(k_iso_local, dim3((unsigned)L.chunks), dim3(ISO_THREADS), 0, st, (const uint64_t*)keys_out, (const uint32_t*)cp,
                       (const int64_t*)pos, n2, va, na);
    CDC_LAUNCH_CHECK("eval_isotonic_fit(local)");
    int64_t slots = ISO_CHUNK;
    for (int64_t spans = L.chunks; spans > 1; spans = (spans + 1) / 2, slots *= 2) {
        hipLaunchKernelGGL(k_iso_merge, dim3((unsigned)((spans + 1) / 2)), dim3(ISO_THREADS), 0, st, (const IsoPt*)va, (const uint32_t*)na, vb,
                           nb, spans, slots);
        CDC_LAUNCH_CHECK("eval_isotonic_fit(merge)");
        std::swap(va, vb);
        std::swap(na, nb);
    }
    blocks = (int)std::min<int64_t>(cdc_ceil_div(n2, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_iso_emit, dim3(blocks), dim3(MET_THREADS), 0, st, (const uint64_t*)keys_out, (const IsoPt*)va, (const uint32_t*)na, cap,
                       x_lo, x_hi, count, positives, value);
    CDC_LAUNCH_CHECK("eval_isotonic_fit(emit)");
    hipLaunchKernelGGL(k_iso_segments, dim3((int)cdc_ceil_div(seg + 1, MET_THREADS)), dim3(MET_THREADS), 0, st, (const IsoPt*)va,
                       (const uint32_t*)na, (const int64_t*)pos, (const uint32_t*)cp, seg, start, seg_rows, seg_positives);
    CDC_LAUNCH_CHECK("eval_isotonic_fit(segments)");
    return 0;
}

// a thread per row: the row's segment is seg_of_domain[its domain]; binary search for the last block that starts at or below the score
__global__ void __launch_bounds__(MET_THREADS) k_iso_apply(const float* __restrict__ pred, const int32_t* __restrict__ domain,
                                                           int64_t ld_domain, int64_t n, int32_t n_domain,
                                                           const int32_t* __restrict__ seg_of_domain, const int64_t* __restrict__ start,
                                                           const float* __restrict__ x_lo, const float* __restrict__ x_hi,
                                                           const double* __restrict__ value, float eps, float* __restrict__ out,
                                                           int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float xf = pred[i];
    const int32_t d = domain ? domain[i * ld_domain] : 0;
    int64_t b0 = 0, b1 = 0;
    if (xf == xf && d >= 0 && d < n_domain) {
        const int32_t s = seg_of_domain[d];
        if (s >= 0 && s <= n_domain) { b0 = start[s]; b1 = start[s + 1]; }
    }
    if (b1 <= b0) {                                                       // a NaN score, a domain outside range, a segment without blocks
        if (err) met_flag_row(err, i);
        out[i] = __uint_as_float(0x7fc00000u);
        return;
    }
    const double x = (double)xf;
    double r;
    if (x <= (double)x_lo[b0]) r = value[b0];
    else if (x >= (double)x_hi[b1 - 1]) r = value[b1 - 1];
    else {
        int64_t lo = b0, hi = b1 - 1;                                     // the largest k with x_lo[k] <= x; x_lo[b0] < x
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if ((double)x_lo[mid] <= x) lo = mid; else hi = mid - 1;
        }
        const double h = (double)x_hi[lo], v = value[lo];
        if (x <= h) r = v;
        else {
            const double t = (x - h) / ((double)x_lo[lo + 1] - h);
            r = v + t * (value[lo + 1] - v);
        }
    }
    float o = (float)r;
    if (eps > 0.f) {
        const float top = __fsub_rn(1.0f, eps);
        o = o < eps ? eps : (o > top ? top : o);
    }
    out[i] = o;
}

extern "C" int cdc_eval_isotonic_apply(const float* pred, const int32_t* domain, int64_t ld_domain, int64_t n, int32_t n_domain,
                                       const int32_t* seg_of_domain, const int64_t* start, const float* x_lo, const float* x_hi,
                                       const double* value, float eps, float* out, int32_t* err_flag, void* stream) {
    CDC_CHECK_ARG(pred && seg_of_domain && start && x_lo && x_hi && value && out, CDC_E_BADARG, "eval_isotonic_apply: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0 && eps >= 0.f && eps <= 0.5f, CDC_E_BADARG,
                  "eval_isotonic_apply: bad sizes n=%ld n_domain=%d ld_domain=%ld eps=%g", (long)n, n_domain, (long)ld_domain, (double)eps);
    MET_TRY(met_need_domain("eval_isotonic_apply", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_isotonic_apply: n=%ld exceeds 2^31 rows", (long)n);
    hipLaunchKernelGGL(k_iso_apply, dim3((unsigned)cdc_ceil_div(n, MET_THREADS)), dim3(MET_THREADS), 0, (hipStream_t)stream, pred, domain,
                       ld_domain, n, n_domain, seg_of_domain, start, x_lo, x_hi, value, eps, out, err_flag);
    CDC_LAUNCH_CHECK("eval_isotonic_apply");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Platt / temperature / bias scaling per segment (a domain's rows, or all rows): the map p' = sigmoid(a z + b) of the logit-scale
// score z that minimises the cross-entropy against Platt's smoothed targets, found by Newton steps with a backtracking line search,
// all of it on the device.
//
//   keys    every row twice, as k_calib_keys does (key = segment << 33 | score_key << 1 | label); the same sort, the same starts
//   prep    per sorted position the score z (float64) and the label byte; the positives of a segment are counted with INTEGER atomics,
//           one per chunk that lies inside one segment
//   pass    max_iter + 1 identical launches.  Workgroup c owns the sorted positions [c, c + 1) * PL_CHUNK and walks the segments that
//           cross them; a (chunk, segment) PIECE is reduced in a fixed order (a lane's items in order, a shuffle tree, the waves in
//           order) to PL_NV sums: at each of the four trial points theta + lambda d, lambda = 1, 1/2, 1/4, 1/8, the objective F, its
//           gradient, its Hessian and the plain cross-entropy.  A segment of one piece is finished by its workgroup; otherwise the
//           piece's sums go to slot (chunk + segment) — distinct for distinct pieces — and the workgroup that arrives LAST at the
//           segment's counter (release before the ticket, acquire after it; nobody waits for anybody) adds the slots in slot order.
//           Whoever holds the segment's sums takes the first lambda that satisfies Armijo's condition, moves there, and solves the
//           2x2 Newton system for the next direction, or, where none does, keeps the point and divides the direction by 16.  The
//           first pass has d = 0: it evaluates the start (1, 0).  A converged segment's workgroups skip it
//   final   a thread per segment writes the outputs
// The piece a position falls into, the order inside a piece and the slot order depend on the sorted keys alone: same rows in any
// order, same bits.  Launch dimensions and the number of launches depend on (n, n_domain, max_iter) alone.
#define PL_THREADS 256
#define PL_ITEMS 8
#define PL_CHUNK (PL_THREADS * PL_ITEMS)          // sorted positions per workgroup
#define PL_NT 4                                   // trial step lengths per pass
#define PL_NQ 7                                   // F, g_a, g_b, H_aa, H_ab, H_bb, plain BCE
#define PL_NV (PL_NT * PL_NQ)
#define PL_GROUPS 8                               // the last arriver adds the slots j = g, g + 8, .. in group g, then the groups in order
#define PL_CONVERGED 1
#define PL_EMPTY 2
#define PL_SLOPE_FIXED 4
#define PL_STARTED 0x100                          // internal: the start has been evaluated
#define PL_METHOD_PLATT 0
#define PL_METHOD_TEMPERATURE 1
#define PL_METHOD_BIAS 2
#define PL_ARMIJO 1e-4
#define PL_F_SLACK 1e-12                          // relative: below it a difference of two objective sums is rounding noise

struct __attribute__((aligned(16))) PlattSeg {
    double a, b, da, db;                          // the point and the direction tried from it
    double F, gd;                                 // the objective (a sum, not a mean) at the point, gradient . direction
    double bce, bce0, gnorm;                      // plain BCE sums at the point and at the start, inf-norm of the MEAN gradient
    unsigned long long P;                         // positives
    int32_t iters, status;
};

__device__ __forceinline__ double platt_z(float x, int32_t input, double Z) {
    const double v = (double)x;
    const double z = input == 0 ? log(v) - log1p(-v) : v;                 // x = 0: -inf, x = 1: +inf; both clamp
    return z < -Z ? -Z : (z > Z ? Z : z);
}

__global__ void __launch_bounds__(MET_THREADS) k_platt_keys(const float* __restrict__ score, const int16_t* __restrict__ label,
                                                            const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                            int32_t n_domain, int32_t input, uint64_t* __restrict__ keys,
                                                            int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float p = score[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int16_t y = label[i];
        bool positive = y == 1;
        const bool bad_p = input == 0 ? !(p >= 0.f && p <= 1.f) : p != p;
        if (bad_p || d < 0 || d >= n_domain || (y != 0 && y != 1)) {      // counted with z = 0, label 0, the domain clamped
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
            p = input == 0 ? 0.5f : 0.f;
            positive = false;
        }
        met_write_pair(keys, n, i, (uint32_t)d, (uint32_t)n_domain, 33, ((uint64_t)score_key(p) << 1) | (uint64_t)positive);
    }
}

// pos[s] = first sorted position of segment s, pos[n_seg] = 2n; every segment's state at the start (1, 0), its arrival counter at zero
__global__ void __launch_bounds__(MET_THREADS) k_platt_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg,
                                                              int64_t* __restrict__ pos, PlattSeg* __restrict__ st,
                                                              uint32_t* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_seg) return;
    const int64_t p0 = met_seg_start(keys, n2, t, n_seg, (uint64_t)t << 33);
    pos[t] = p0;
    if (t == n_seg) return;
    const int64_t p1 = t + 1 == n_seg ? n2 : lower_bound_u64(keys, p0, n2, (uint64_t)(t + 1) << 33);
    PlattSeg c;
    c.a = 1.0; c.b = 0.0; c.da = 0.0; c.db = 0.0; c.F = 0.0; c.gd = 0.0; c.bce = 0.0; c.bce0 = 0.0; c.gnorm = 0.0;
    c.P = 0ull; c.iters = 0; c.status = p1 == p0 ? PL_EMPTY : 0;
    st[t] = c;
    cnt[t] = 0u;
}

// workgroup c writes z and the label byte of the sorted positions [c, c + 1) * PL_CHUNK and counts their positives: one integer
// atomic per workgroup where the chunk lies inside one segment (one per positive row, on the row's own segment, in the few that do not)
__global__ void __launch_bounds__(PL_THREADS) k_platt_prep(const uint64_t* __restrict__ keys, int64_t n2, int32_t input, double Z,
                                                           double* __restrict__ zs, uint8_t* __restrict__ lab, PlattSeg* __restrict__ st) {
    __shared__ uint32_t s_cnt[PL_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * PL_CHUNK, hi = lo + PL_CHUNK < n2 ? lo + PL_CHUNK : n2;
    const uint64_t seg_lo = keys[lo] >> 33;
    const bool one = seg_lo == (keys[hi - 1] >> 33);
    uint32_t mine = 0;
    for (int it = 0; it < PL_ITEMS; ++it) {
        const int64_t i = lo + (int64_t)it * PL_THREADS + tid;
        if (i >= hi) break;
        const uint64_t key = keys[i];
        const bool y = (key & 1ull) != 0;
        zs[i] = platt_z(cal_score(key), input, Z);
        lab[i] = (uint8_t)y;
        if (y) {
            if (one) ++mine;
            else atomicAdd(&st[key >> 33].P, 1ull);
        }
    }
    if (!one) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        const uint32_t all = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (all) atomicAdd(&st[seg_lo].P, (unsigned long long)all);
    }
}

// one thread, holding the sums of a whole segment at the four trial points: the line search and the next Newton direction
__device__ void platt_advance(PlattSeg* sp, const double* tot, const double* zs, int64_t s0, int64_t s1, int32_t method, double gtol) {
    PlattSeg c = *sp;
    const double m = (double)(s1 - s0);
    const bool started = (c.status & PL_STARTED) != 0;
    int k = -1;
    if (!started) {                                                       // d = 0: the four trial points are the start itself
        c.status |= PL_STARTED;
        if (method == PL_METHOD_PLATT && zs[s0] == zs[s1 - 1]) c.status |= PL_SLOPE_FIXED;     // z ascends along a segment
        c.bce0 = tot[PL_NQ - 1];
        k = 0;
    } else {
        c.iters += 1;
        const double slack = PL_F_SLACK * fabs(c.F);
        double lam = 1.0;
        for (int j = 0; j < PL_NT; ++j, lam *= 0.5)
            if (tot[j * PL_NQ] <= c.F + PL_ARMIJO * lam * c.gd + slack) { k = j; break; }
    }
    if (k < 0) {                                                          // no trial length was good enough: a shorter direction
        c.da *= 0.0625; c.db *= 0.0625; c.gd *= 0.0625;
        *sp = c;
        return;
    }
    const bool free_a = method == PL_METHOD_TEMPERATURE || (method == PL_METHOD_PLATT && !(c.status & PL_SLOPE_FIXED));
    const bool free_b = method != PL_METHOD_TEMPERATURE;
    const double lam = k == 0 ? 1.0 : (k == 1 ? 0.5 : (k == 2 ? 0.25 : 0.125));
    const double* q = tot + k * PL_NQ;
    c.a = c.a + lam * c.da;                                               // the expressions of k_platt_pass
    c.b = c.b + lam * c.db;
    c.F = q[0];
    c.bce = q[6];
    const double ga = free_a ? q[1] : 0.0, gb = free_b ? q[2] : 0.0;
    const double haa = q[3], hab = q[4], hbb = q[5];
    c.gnorm = fmax(fabs(ga), fabs(gb)) / m;
    c.da = c.db = c.gd = 0.0;
    if (c.gnorm <= gtol) {
        c.status |= PL_CONVERGED;
    } else {
        const double det = haa * hbb - hab * hab;
        if (free_a && free_b && det > 1e-13 * haa * hbb) {
            c.da = -(hbb * ga - hab * gb) / det;
            c.db = -(haa * gb - hab * ga) / det;
        } else {                                                          // one free parameter, or a Hessian too close to singular
            if (free_a && haa > 0.0) c.da = -ga / haa;
            if (free_b && hbb > 0.0) c.db = -gb / hbb;
        }
        c.gd = ga * c.da + gb * c.db;
    }
    *sp = c;
}

// st, part and cnt are written and read across workgroups inside this launch: no const, no __restrict__ (they stay off the scalar path)
__global__ void __launch_bounds__(PL_THREADS) k_platt_pass(const double* __restrict__ zs, const uint8_t* __restrict__ lab,
                                                           const int64_t* __restrict__ pos, int64_t n2, int32_t n_seg, int32_t method,
                                                           double gtol, PlattSeg* st, double* part, uint32_t* cnt) {
    __shared__ double sh[PL_GROUPS][PL_NV];
    __shared__ double tot[PL_NV];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t lo = chunk * PL_CHUNK, hi = lo + PL_CHUNK < n2 ? lo + PL_CHUNK : n2;
    int32_t s;
    {                                                                     // the largest s with pos[s] <= lo: the segment that holds lo
        int32_t x = 0, y = n_seg - 1;
        while (x < y) {
            const int32_t mid = (x + y + 1) >> 1;
            if (pos[mid] <= lo) x = mid; else y = mid - 1;
        }
        s = x;
    }
    for (; s < n_seg; ++s) {
        const int64_t s0 = pos[s], s1 = pos[s + 1];
        if (s0 >= hi) break;
        const int64_t p0 = s0 > lo ? s0 : lo, p1 = s1 < hi ? s1 : hi;
        if (p1 <= p0) continue;                                           // an empty segment
        const PlattSeg cur = st[s];                                       // written by an earlier launch; this launch writes it only
        if (cur.status & PL_CONVERGED) continue;                          //   after every piece of the segment has arrived
        const bool started = (cur.status & PL_STARTED) != 0;
        const double P = (double)cur.P, N = (double)(s1 - s0) - P;
        const double t_pos = (P + 1.0) / (P + 2.0), t_neg = 1.0 / (N + 2.0);
        double ta[PL_NT], tb[PL_NT], acc[PL_NT][PL_NQ];
        {
            double lam = 1.0;
#pragma unroll
            for (int k = 0; k < PL_NT; ++k, lam *= 0.5) {
                ta[k] = cur.a + lam * cur.da;
                tb[k] = cur.b + lam * cur.db;
#pragma unroll
                for (int j = 0; j < PL_NQ; ++j) acc[k][j] = 0.0;
            }
        }
        int64_t i = p0 + tid;
        double z_next = 0.0;
        uint8_t y_next = 0;
        if (i < p1) { z_next = zs[i]; y_next = lab[i]; }
#pragma unroll 1
        for (int it = 0; it < PL_ITEMS && i < p1; ++it) {                 // the next item's loads fly while this one is evaluated
            const double z = z_next;
            const bool y = y_next != 0;
            i += PL_THREADS;
            if (i < p1) { z_next = zs[i]; y_next = lab[i]; }
            const double t = y ? t_pos : t_neg;
#pragma unroll
            for (int k = 0; k < PL_NT; ++k) {
                if (k == 0 || started) {                                  // the first pass has one point, four times
                    const double u = ta[k] * z + tb[k];
                    const double e = exp(-fabs(u));
                    const double sp = fmax(u, 0.0) + log1p(e);            // softplus(u)
                    const double p = (u >= 0.0 ? 1.0 : e) / (1.0 + e);    // sigmoid(u)
                    const double r = p - t, w = p * (1.0 - p);
                    acc[k][0] += sp - t * u;
                    acc[k][1] += r * z;
                    acc[k][2] += r;
                    acc[k][3] += w * z * z;
                    acc[k][4] += w * z;
                    acc[k][5] += w;
                    acc[k][6] += y ? sp - u : sp;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PL_NT; ++k)
#pragma unroll
            for (int j = 0; j < PL_NQ; ++j) {
                const double v = wave_sum_d(acc[k][j]);
                if (lane == 0) sh[wave][k * PL_NQ + j] = v;
            }
        __syncthreads();
        double mine = 0.0;
        if (tid < PL_NV) mine = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
        const int64_t c0 = s0 / PL_CHUNK, pieces = (s1 - 1) / PL_CHUNK - c0 + 1;
        bool finish = true;
        if (pieces > 1) {
            if (tid < PL_NV) part[(chunk + s) * PL_NV + tid] = mine;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // every storing wave, then the barrier, then ONE release
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const uint32_t ticket = __hip_atomic_fetch_add(&cnt[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int last = ticket == (uint32_t)(pieces - 1);
                if (last) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                s_last = last;
            }
            __syncthreads();
            finish = s_last != 0;
            if (finish) {                                                 // the slots c0 + s .. c0 + s + pieces - 1, in a fixed order
                const int j = tid & 31, g = tid >> 5;
                if (j < PL_NV) {
                    double v = 0.0;
                    for (int64_t k = g; k < pieces; k += PL_GROUPS) v += part[(c0 + s + k) * PL_NV + j];
                    sh[g][j] = v;
                }
                __syncthreads();
                if (tid < PL_NV) {
                    mine = 0.0;
#pragma unroll
                    for (int g2 = 0; g2 < PL_GROUPS; ++g2) mine += sh[g2][tid];
                }
            }
        }
        if (finish) {
            if (tid < PL_NV) tot[tid] = mine;
            __syncthreads();
            if (tid == 0) {
                platt_advance(&st[s], tot, zs, s0, s1, method, gtol);
                cnt[s] = 0u;                                              // the next pass counts from zero
            }
        }
        __syncthreads();                                                  // sh, tot and s_last are free for the next segment
    }
}

__global__ void __launch_bounds__(MET_THREADS) k_platt_final(const PlattSeg* __restrict__ st, const int64_t* __restrict__ pos, int32_t n_seg,
                                                             double* __restrict__ a, double* __restrict__ b, double* __restrict__ loss_before,
                                                             double* __restrict__ loss_after, double* __restrict__ grad,
                                                             int64_t* __restrict__ seg_rows, int64_t* __restrict__ seg_positives,
                                                             int32_t* __restrict__ iterations, int32_t* __restrict__ status) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const PlattSeg c = st[s];
    const int64_t m = pos[s + 1] - pos[s];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    a[s] = c.a;
    b[s] = c.b;
    loss_before[s] = m > 0 ? c.bce0 / (double)m : nan;
    loss_after[s] = m > 0 ? c.bce / (double)m : nan;
    grad[s] = m > 0 ? c.gnorm : nan;
    seg_rows[s] = m;
    seg_positives[s] = (int64_t)c.P;
    iterations[s] = c.iters;
    status[s] = c.status & (PL_CONVERGED | PL_EMPTY | PL_SLOPE_FIXED);
}

struct PlattLayout {
    MetLayout m;                        // once the sort has run, keys_in holds z per sorted position; m.start is pos
    int64_t lab, st, cnt, part, chunks;
};
static void platt_fixed_layout(int64_t n, int32_t n_domain, PlattLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1;
    L->chunks = cdc_ceil_div(n2, PL_CHUNK);
    MetCursor c;
    L->m.keys(c, n2, 0);
    L->lab = c.take(n2);
    L->m.starts(c, seg);
    L->st = c.take(seg * (int64_t)sizeof(PlattSeg));
    L->cnt = c.take(seg * 4);
    L->part = c.take((L->chunks + seg) * PL_NV * 8);           // slot = chunk + segment < chunks + seg
    L->m.end_fixed(c);
}
static bool platt_clip_ok(double clip) { return clip >= 1e-12 && clip <= 0.25; }

extern "C" int64_t cdc_eval_platt_fit_workspace_bytes(int64_t n, int32_t n_domain) {
    if (!iso_sizes_ok(n, n_domain)) return 0;
    PlattLayout L;
    platt_fixed_layout(n, n_domain, &L);
    if (met_keys_temp(n, "eval_platt_fit", &L.m) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_platt_fit(const float* score, const int16_t* label, const int32_t* domain, int64_t ld_domain, int64_t n,
                                  int32_t n_domain, int32_t method, int32_t input, double clip, double gtol, int32_t max_iter, double* a,
                                  double* b, double* loss_before, double* loss_after, double* grad, int64_t* seg_rows,
                                  int64_t* seg_positives, int32_t* iterations, int32_t* status, int32_t* err_flag, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(score && label && a && b && loss_before && loss_after && grad && seg_rows && seg_positives && iterations && status && workspace,
                  CDC_E_BADARG, "eval_platt_fit: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_platt_fit: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    MET_TRY(met_need_domain("eval_platt_fit", domain, n_domain));
    CDC_CHECK_ARG(method >= PL_METHOD_PLATT && method <= PL_METHOD_BIAS, CDC_E_BADARG, "eval_platt_fit: unknown method %d", method);
    CDC_CHECK_ARG(input == 0 || input == 1, CDC_E_BADARG, "eval_platt_fit: unknown input %d (0: probabilities, 1: logits)", input);
    CDC_CHECK_ARG(platt_clip_ok(clip), CDC_E_BADARG, "eval_platt_fit: clip=%g outside [1e-12, 0.25]", clip);
    CDC_CHECK_ARG(gtol > 0.0, CDC_E_BADARG, "eval_platt_fit: gtol=%g must be positive", gtol);
    CDC_CHECK_ARG(max_iter >= 1 && max_iter <= 1024, CDC_E_BADARG, "eval_platt_fit: max_iter=%d outside [1, 1024]", max_iter);
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_platt_fit: n=%ld exceeds 2^31 rows", (long)n);
    PlattLayout L;
    platt_fixed_layout(n, n_domain, &L);
    MET_TRY(met_gate("eval_platt_fit", workspace, workspace_bytes, &L.m, [&] { return met_keys_temp(n, "eval_platt_fit", &L.m); }));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_in = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys_out = ws.ptr<uint64_t>(L.m.keys_out);
    double* zs = (double*)keys_in;                                        // the unsorted keys are done with after the sort
    uint8_t* lab = ws.ptr<uint8_t>(L.lab);
    int64_t* pos = ws.ptr<int64_t>(L.m.start);
    PlattSeg* st = ws.ptr<PlattSeg>(L.st);
    double* part = ws.ptr<double>(L.part);
    uint32_t* cnt = ws.ptr<uint32_t>(L.cnt);
    hipStream_t sm = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1;
    const double Z = log((1.0 - clip) / clip);
    const int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
    hipLaunchKernelGGL(k_platt_keys, dim3(blocks), dim3(MET_THREADS), 0, sm, score, label, domain, ld_domain, n, n_domain, input, keys_in, err_flag);
    CDC_LAUNCH_CHECK("eval_platt_fit(keys)");
    MET_TRY(met_sort("eval_platt_fit", ws.base, L.m, (size_t)n2, met_end_bit((uint64_t)n_domain, 33), sm));
    hipLaunchKernelGGL(k_platt_starts, dim3((int)cdc_ceil_div(seg + 1, MET_THREADS)), dim3(MET_THREADS), 0, sm, (const uint64_t*)keys_out, n2, seg, pos, st, cnt);
    CDC_LAUNCH_CHECK("eval_platt_fit(starts)");
    hipLaunchKernelGGL(k_platt_prep, dim3((unsigned)L.chunks), dim3(PL_THREADS), 0, sm, (const uint64_t*)keys_out, n2, input, Z, zs, lab, st);
    CDC_LAUNCH_CHECK("eval_platt_fit(prep)");
    for (int it = 0; it <= max_iter; ++it) {                              // the start, then max_iter Newton steps
        hipLaunchKernelGGL(k_platt_pass, dim3((unsigned)L.chunks), dim3(PL_THREADS), 0, sm, (const double*)zs, (const uint8_t*)lab,
                           (const int64_t*)pos, n2, seg, method, gtol, st, part, cnt);
        CDC_LAUNCH_CHECK("eval_platt_fit(pass)");
    }
    hipLaunchKernelGGL(k_platt_final, dim3((int)cdc_ceil_div(seg, MET_THREADS)), dim3(MET_THREADS), 0, sm, (const PlattSeg*)st, (const int64_t*)pos, seg,
                       a, b, loss_before, loss_after, grad, seg_rows, seg_positives, iterations, status);
    CDC_LAUNCH_CHECK("eval_platt_fit(final)");
    return 0;
}

// a thread per row: out = sigmoid(a[s] z + b[s]) with s = seg_of_domain[the row's domain], float64 operations in this order, unfused
__global__ void __launch_bounds__(MET_THREADS) k_platt_apply(const float* __restrict__ score, const int32_t* __restrict__ domain,
                                                             int64_t ld_domain, int64_t n, int32_t n_domain,
                                                             const int32_t* __restrict__ seg_of_domain, const double* __restrict__ a,
                                                             const double* __restrict__ b, int32_t input, double Z, float eps,
                                                             float* __restrict__ out, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = score[i];
    const int32_t d = domain ? domain[i * ld_domain] : 0;
    int32_t s = -1;
    if ((input == 0 ? (x >= 0.f && x <= 1.f) : x == x) && d >= 0 && d < n_domain) s = seg_of_domain[d];
    if (s < 0 || s > n_domain) {                                          // a NaN score, a probability outside [0, 1], a domain or a segment outside range
        if (err) met_flag_row(err, i);
        out[i] = __uint_as_float(0x7fc00000u);
        return;
    }
    const double u = __dadd_rn(__dmul_rn(a[s], platt_z(x, input, Z)), b[s]);
    float o = (float)(1.0 / (1.0 + exp(-u)));
    if (eps > 0.f) {
        const float top = __fsub_rn(1.0f, eps);
        o = o < eps ? eps : (o > top ? top : o);
    }
    out[i] = o;
}

extern "C" int cdc_eval_platt_apply(const float* score, const int32_t* domain, int64_t ld_domain, int64_t n, int32_t n_domain,
                                    const int32_t* seg_of_domain, const double* a, const double* b, int32_t input, double clip, float eps,
                                    float* out, int32_t* err_flag, void* stream) {
    CDC_CHECK_ARG(score && seg_of_domain && a && b && out, CDC_E_BADARG, "eval_platt_apply: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_domain >= 0, CDC_E_BADARG,
                  "eval_platt_apply: bad sizes n=%ld n_domain=%d ld_domain=%ld", (long)n, n_domain, (long)ld_domain);
    MET_TRY(met_need_domain("eval_platt_apply", domain, n_domain));
    CDC_CHECK_ARG(input == 0 || input == 1, CDC_E_BADARG, "eval_platt_apply: unknown input %d (0: probabilities, 1: logits)", input);
    CDC_CHECK_ARG(platt_clip_ok(clip), CDC_E_BADARG, "eval_platt_apply: clip=%g outside [1e-12, 0.25]", clip);
    CDC_CHECK_ARG(eps >= 0.f && eps <= 0.5f, CDC_E_BADARG, "eval_platt_apply: eps=%g outside [0, 0.5]", (double)eps);
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_platt_apply: n=%ld exceeds 2^31 rows", (long)n);
    hipLaunchKernelGGL(k_platt_apply, dim3((unsigned)cdc_ceil_div(n, MET_THREADS)), dim3(MET_THREADS), 0, (hipStream_t)stream, score, domain,
                       ld_domain, n, n_domain, seg_of_domain, a, b, input, log((1.0 - clip) / clip), eps, out, err_flag);
    CDC_LAUNCH_CHECK("eval_platt_apply");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Clustered bootstrap of AUC, log-loss and GAUC.  Replicate r gives cluster c (a user, or a row when there is no cluster column)
// the weight w(seed, r, c), a Poisson(1) variate capped at 12 that is a pure function of its three arguments: it is formed from a
// hash wherever it is needed and never stored per row.  Every figure is recomputed with the row weight w_i = w(cluster of row i):
//
//   AUC   U2 / (2 Wp Wn) with U2 = sum over (positive i, negative j) of w_i w_j (2 [s_j < s_i] + [s_j = s_i]), Wp = sum w_i y_i,
//         Wn = W - Wp, all in 64-bit integers (order-free), one conversion and one division at the end
//   loss  sum w_i l_i / W with k_metric_loss's per-row term l_i, added in an order that the sorted keys alone decide
//   GAUC  sum_g w_g omega_g A_g / sum_g w_g omega_g over cdc_eval_gauc's counted groups: the user's own AUC A_g does not move
//
//   keys    every row twice, key = segment << 33 | score_key << 1 | label, payload = the copy index; one radix sort.  The label
//           bit puts a tie run's negatives in front of its positives, so for a positive at sorted position i
//               w_i * (weighted negatives at positions < i  +  weighted negatives in front of i's tie run)
//           is its share of U2 — counted over the WHOLE sorted array; a segment subtracts 2 Wp * (weighted negatives of the
//           segments in front of it) in the last launch.  Unsigned 64-bit sums wrap and the difference is exact
//   prep    once per sorted position: its cluster, its loss term and f, the first position of its tie run (replicate-free)
//   totals  workgroup = BOOT_CHUNK sorted positions, read once; for every tile of BOOT_REP_TILE replicates the weights are formed in
//           registers and the chunk's weighted negatives, and those of its LAST tie run, are summed
//   scan    per replicate an exclusive sum of the chunks' totals
//   pass    the same chunks: an in-chunk scan of the weighted negatives per replicate (two replicates to a 32-bit word), kept in
//           LDS as 16-bit in-chunk prefixes.  A tie run that began in an earlier chunk p takes the prefix in front of it from
//           off[p + 1] - tail[p].  Per segment present in the chunk the sums (W, Wp, U, loss) go through registers, a shuffle
//           tree and the waves in order, and are written — not added — to the chunk's head or tail slot (first / last segment of
//           the chunk) or to the segment's own slot (a segment inside one chunk)
//   reduce  a thread per (segment, replicate) adds its chunks' slots in order; final: a thread per replicate walks the segments
// No float atomics, nothing zeroed, no per-row weights in memory.  The launch count depends on (paired, gauc) alone: the replicate
// tiles are a loop inside the grid.  Integer figures do not depend on the row order; the loss depends on it only through the
// order of tied rows.
#define BOOT_THREADS 256
#define BOOT_ITEMS 4
#define BOOT_CHUNK 1024                 // sorted positions per workgroup: BOOT_THREADS * BOOT_ITEMS (12 * BOOT_CHUNK < 2^16)
#define BOOT_REP_TILE 8                 // replicates per pass over a chunk's registers: 8 weights of 4 bits to a word
#define BOOT_MAX_REP 4096
#define BOOT_WAVES (BOOT_THREADS / 64)
static_assert(BOOT_CHUNK == BOOT_THREADS * BOOT_ITEMS && 12 * BOOT_CHUNK < 65536 && BOOT_REP_TILE == 8, "bootstrap tile arithmetic");

__device__ __forceinline__ uint64_t boot_mix(uint64_t x) {                 // splitmix64's finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ uint64_t boot_rep_base(uint64_t seed, uint32_t r) {
    return boot_mix(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1u));
}
// #{k < 12 : u >= floor(2^32 e^-1 sum_{j <= k} 1/j!)}: Poisson(1) by inversion, capped at 12
__device__ __forceinline__ uint32_t boot_weight(uint64_t base, uint32_t c) {
    const uint32_t u = (uint32_t)(boot_mix(base + (uint64_t)c) >> 32);
    uint32_t w = (u >= 0x5e2d58d8u) + (u >= 0xbc5ab1b1u) + (u >= 0xeb715e1du) + (u >= 0xfb239797u);
    if (u >= 0xff1025f5u)
        w += 1u + (u >= 0xffd90f3bu) + (u >= 0xfffa8b71u) + (u >= 0xffff540cu) + (u >= 0xffffed1fu) + (u >= 0xfffffe21u) +
             (u >= 0xffffffd4u) + (u >= 0xfffffffcu);
    return w;
}

__global__ void __launch_bounds__(MET_THREADS) k_boot_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                           const int32_t* __restrict__ cluster, int64_t ld_cluster, int64_t n_cluster,
                                                           const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                           int32_t n_domain, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                           int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int64_t u = cluster ? (int64_t)cluster[i * ld_cluster] : 0;
        const int16_t y = label[i];
        if (p != p || d < 0 || d >= n_domain || u < 0 || (cluster && u >= n_cluster) || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
        }
        met_write_pair(keys, idx, n, i, (uint32_t)d, (uint32_t)n_domain, 33, ((uint64_t)score_key(p) << 1) | (uint64_t)(y != 0), (uint32_t)i,
                       (uint32_t)(n + i));
    }
}

__global__ void k_boot_starts(const uint64_t* __restrict__ keys, int64_t n2, int32_t n_seg, int64_t* __restrict__ start) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d <= n_seg) start[d] = met_seg_start(keys, n2, d, n_seg, (uint64_t)(uint32_t)d << 33);
}

// what a sorted position carries into every replicate: cluster (clamped as k_gauc_keys clamps a user), loss term, tie-run start
__global__ void __launch_bounds__(MET_THREADS) k_boot_prep(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ cluster, int64_t ld_cluster, int64_t n_cluster,
                                                           int64_t n, int64_t n2, uint32_t* __restrict__ cl, double* __restrict__ term,
                                                           uint32_t* __restrict__ f) {
    const float eps = 1.1920928955078125e-07f, hi = 1.0f - eps;            // k_metric_loss's clip
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const int64_t j = idx[i], row = j >= n ? j - n : j;
        int64_t u = row;
        if (cluster) {
            u = cluster[row * ld_cluster];
            u = u < 0 ? 0 : (u >= n_cluster ? n_cluster - 1 : u);
        }
        cl[i] = (uint32_t)u;
        const float p = key_score((uint32_t)(key >> 1));
        float c = (key & 1ull) ? p : __fsub_rn(1.0f, p);
        c = c < eps ? eps : (c > hi ? hi : c);
        term[i] = -log((double)c);
        f[i] = (uint32_t)lower_bound_u64(keys, 0, i + 1, key & ~1ull);
    }
}

// ntot[r][c]: weighted negatives of chunk c; ntail[r][c]: those of them in the chunk's last tie run
__global__ void __launch_bounds__(BOOT_THREADS) k_boot_totals(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cl,
                                                              const uint32_t* __restrict__ f, int64_t n2, int64_t nchunks,
                                                              int32_t n_rep, uint64_t seed, uint32_t* __restrict__ ntot,
                                                              uint32_t* __restrict__ ntail) {
    __shared__ uint32_t sh[BOOT_WAVES][BOOT_REP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = blockIdx.x, c0 = c * BOOT_CHUNK, c1 = c0 + BOOT_CHUNK < n2 ? c0 + BOOT_CHUNK : n2;
    const int64_t tail_lo = (int64_t)f[c1 - 1] > c0 ? (int64_t)f[c1 - 1] : c0;
    bool neg[BOOT_ITEMS], tail[BOOT_ITEMS];
    uint32_t clu[BOOT_ITEMS];
#pragma unroll
    for (int k = 0; k < BOOT_ITEMS; ++k) {
        const int64_t pos = c0 + tid * BOOT_ITEMS + k;
        neg[k] = false; tail[k] = false; clu[k] = 0u;
        if (pos < c1) {
            neg[k] = (keys[pos] & 1ull) == 0ull;
            clu[k] = cl[pos];
            tail[k] = pos >= tail_lo;
        }
    }
    const int ntiles = (n_rep + BOOT_REP_TILE - 1) / BOOT_REP_TILE;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        uint32_t v[BOOT_REP_TILE];
#pragma unroll
        for (int r = 0; r < BOOT_REP_TILE; ++r) {
            const uint64_t base = boot_rep_base(seed, (uint32_t)(t * BOOT_REP_TILE + r));
            uint32_t a = 0u;
#pragma unroll
            for (int k = 0; k < BOOT_ITEMS; ++k)
                if (neg[k]) {
                    const uint32_t w = boot_weight(base, clu[k]);
                    a += tail[k] ? w * 0x10001u : w;                       // low half: the chunk, high half: its last run
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            v[r] = a;
        }
        if (lane == 0)
            for (int r = 0; r < BOOT_REP_TILE; ++r) sh[wave][r] = v[r];
        __syncthreads();
        if (tid < BOOT_REP_TILE) {
            uint32_t s = 0u;
            for (int w = 0; w < BOOT_WAVES; ++w) s += sh[w][tid];
            const int rr = t * BOOT_REP_TILE + tid;
            if (rr < n_rep) {
                ntot[(int64_t)rr * nchunks + c] = s & 0xffffu;
                ntail[(int64_t)rr * nchunks + c] = s >> 16;
            }
        }
        __syncthreads();
    }
}

// off[r][c], c in [0, nchunks]: weighted negatives in front of chunk c.  One workgroup per replicate
__global__ void __launch_bounds__(BOOT_THREADS) k_boot_scan(const uint32_t* __restrict__ ntot, int64_t nchunks,
                                                            unsigned long long* __restrict__ off) {
    __shared__ unsigned long long sh[BOOT_THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    unsigned long long carry = 0ull;
    for (int64_t b = 0; b < nchunks; b += BOOT_THREADS) {
        const unsigned long long v = b + tid < nchunks ? (unsigned long long)ntot[r * nchunks + b + tid] : 0ull;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < BOOT_THREADS; o <<= 1) {
            const unsigned long long x = tid >= o ? sh[tid - o] : 0ull;
            __syncthreads();
            sh[tid] += x;
            __syncthreads();
        }
        if (b + tid < nchunks) off[r * (nchunks + 1) + b + tid] = carry + sh[tid] - v;
        carry += sh[BOOT_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) off[r * (nchunks + 1) + nchunks] = carry;
}

// slot layout of one chunk / one segment: 3 words per replicate — (W | Wp << 32) of at most BOOT_CHUNK rows, U, the loss sum's bits
__global__ void __launch_bounds__(BOOT_THREADS) k_boot_pass(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cl,
                                                            const double* __restrict__ term, const uint32_t* __restrict__ f,
                                                            const int64_t* __restrict__ start, int64_t n2, int64_t nchunks,
                                                            int32_t n_rep, uint64_t seed, const uint32_t* __restrict__ ntail,
                                                            const unsigned long long* __restrict__ off,
                                                            unsigned long long* __restrict__ parts,
                                                            unsigned long long* __restrict__ direct) {
    __shared__ uint16_t s_pre[BOOT_REP_TILE][BOOT_CHUNK];
    __shared__ uint32_t s_scan[BOOT_WAVES][BOOT_REP_TILE / 2];
    __shared__ unsigned long long s_off[BOOT_REP_TILE], s_head[BOOT_REP_TILE];
    __shared__ unsigned long long s_red[BOOT_WAVES][BOOT_REP_TILE * 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = blockIdx.x, c0 = c * BOOT_CHUNK, c1 = c0 + BOOT_CHUNK < n2 ? c0 + BOOT_CHUNK : n2;
    const int64_t d_first = (int64_t)(keys[c0] >> 33), d_last = (int64_t)(keys[c1 - 1] >> 33);
    const int64_t f_head = f[c0];
    const bool has_head = f_head < c0;                                     // the first tie run began in an earlier chunk
    const int64_t c_head = f_head / BOOT_CHUNK;
    bool ok[BOOT_ITEMS], posv[BOOT_ITEMS];
    uint32_t clu[BOOT_ITEMS], fl[BOOT_ITEMS];
    bool f_in[BOOT_ITEMS];
    double trm[BOOT_ITEMS];
#pragma unroll
    for (int k = 0; k < BOOT_ITEMS; ++k) {
        const int64_t pos = c0 + tid * BOOT_ITEMS + k;
        ok[k] = pos < c1; posv[k] = false; clu[k] = 0u; fl[k] = 0u; f_in[k] = true; trm[k] = 0.0;
        if (ok[k]) {
            posv[k] = (keys[pos] & 1ull) != 0ull;
            clu[k] = cl[pos];
            trm[k] = term[pos];
            const int64_t fk = f[pos];
            f_in[k] = fk >= c0;
            fl[k] = f_in[k] ? (uint32_t)(fk - c0) : 0u;
        }
    }
    const int ntiles = (n_rep + BOOT_REP_TILE - 1) / BOOT_REP_TILE;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        if (tid < BOOT_REP_TILE) {
            const int rr = t * BOOT_REP_TILE + tid < n_rep ? t * BOOT_REP_TILE + tid : n_rep - 1;
            const unsigned long long* o = off + (int64_t)rr * (nchunks + 1);
            s_off[tid] = o[c];
            s_head[tid] = has_head ? o[c_head + 1] - (unsigned long long)ntail[(int64_t)rr * nchunks + c_head] : 0ull;
        }
        // the tile's weights, 4 bits each, and this thread's weighted negatives, two replicates to a word
        uint32_t wpk[BOOT_ITEMS] = {0u, 0u, 0u, 0u};
        uint32_t tn[BOOT_REP_TILE / 2] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < BOOT_REP_TILE; ++r) {
            const uint64_t base = boot_rep_base(seed, (uint32_t)(t * BOOT_REP_TILE + r));
#pragma unroll
            for (int k = 0; k < BOOT_ITEMS; ++k) {
                const uint32_t w = ok[k] ? boot_weight(base, clu[k]) : 0u;
                wpk[k] |= w << (4 * r);
                if (!posv[k]) tn[r >> 1] += w << (16 * (r & 1));
            }
        }
        uint32_t ex[BOOT_REP_TILE / 2];
#pragma unroll
        for (int j = 0; j < BOOT_REP_TILE / 2; ++j) {
            uint32_t v = tn[j];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t x = __shfl_up(v, o, 64);
                if (lane >= o) v += x;
            }
            if (lane == 63) s_scan[wave][j] = v;
            ex[j] = v - tn[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < BOOT_REP_TILE / 2; ++j)
            for (int w = 0; w < wave; ++w) ex[j] += s_scan[w][j];
#pragma unroll
        for (int r = 0; r < BOOT_REP_TILE; ++r) {
            uint32_t e = (ex[r >> 1] >> (16 * (r & 1))) & 0xffffu;
#pragma unroll
            for (int k = 0; k < BOOT_ITEMS; ++k) {
                s_pre[r][tid * BOOT_ITEMS + k] = (uint16_t)e;              // weighted negatives of the chunk in front of the item
                if (!posv[k]) e += (wpk[k] >> (4 * r)) & 15u;
            }
        }
        __syncthreads();
        for (int64_t d = d_first; d <= d_last; ++d) {
            int64_t lo = c0, hi = c1;
            if (d_first != d_last) {
                lo = start[d] > c0 ? start[d] : c0;
                hi = start[d + 1] < c1 ? start[d + 1] : c1;
                if (lo >= hi) continue;                                    // uniform: no row of d in this chunk
            }
            bool in[BOOT_ITEMS];
#pragma unroll
            for (int k = 0; k < BOOT_ITEMS; ++k) {
                const int64_t pos = c0 + tid * BOOT_ITEMS + k;
                in[k] = pos >= lo && pos < hi;
            }
#pragma unroll
            for (int r = 0; r < BOOT_REP_TILE; ++r) {
                unsigned long long aw = 0ull, au = 0ull;
                double al = 0.0;
                const unsigned long long o_r = s_off[r], h_r = s_head[r];
#pragma unroll
                for (int k = 0; k < BOOT_ITEMS; ++k) {
                    const unsigned long long w = in[k] ? (wpk[k] >> (4 * r)) & 15u : 0u;
                    if (w == 0ull) continue;
                    al += (double)w * trm[k];
                    aw += w;
                    if (posv[k]) {
                        aw += w << 32;
                        const unsigned long long below = o_r + s_pre[r][tid * BOOT_ITEMS + k];
                        const unsigned long long below_run = f_in[k] ? o_r + s_pre[r][fl[k]] : h_r;
                        au += w * (below + below_run);
                    }
                }
                aw = dl_wave_sum(aw);
                au = dl_wave_sum(au);
                al = wave_sum_d(al);
                if (lane == 0) {
                    s_red[wave][r * 3] = aw;
                    s_red[wave][r * 3 + 1] = au;
                    s_red[wave][r * 3 + 2] = (unsigned long long)__double_as_longlong(al);
                }
            }
            __syncthreads();
            if (tid < BOOT_REP_TILE * 3) {
                const int r = tid / 3, q = tid - 3 * r, rr = t * BOOT_REP_TILE + r;
                unsigned long long v;
                if (q < 2) {
                    v = 0ull;
                    for (int w = 0; w < BOOT_WAVES; ++w) v += s_red[w][tid];
                } else {
                    double a = 0.0;
                    for (int w = 0; w < BOOT_WAVES; ++w) a += __longlong_as_double((long long)s_red[w][tid]);
                    v = (unsigned long long)__double_as_longlong(a);
                }
                if (rr < n_rep) {
                    if (d == d_first) parts[((c * 2 + 0) * 3 + q) * n_rep + rr] = v;
                    else if (d == d_last) parts[((c * 2 + 1) * 3 + q) * n_rep + rr] = v;
                    else direct[(d * 3 + q) * n_rep + rr] = v;
                }
            }
            __syncthreads();
        }
    }
}

// tot[d][4][r]: W, Wp, U (over the whole array's prefixes), loss sum — a thread per (segment, replicate), its chunks in order
__global__ void __launch_bounds__(BOOT_THREADS) k_boot_reduce(const uint64_t* __restrict__ keys, const int64_t* __restrict__ start,
                                                              int64_t n2, int32_t n_rep, int32_t n_seg,
                                                              const unsigned long long* __restrict__ parts,
                                                              const unsigned long long* __restrict__ direct,
                                                              unsigned long long* __restrict__ tot) {
    const int64_t id = (int64_t)blockIdx.x * BOOT_THREADS + threadIdx.x;
    const int64_t d = id / n_rep, r = id - d * n_rep;
    if (d >= n_seg) return;
    const int64_t s0 = start[d], s1 = start[d + 1];
    unsigned long long W = 0ull, Wp = 0ull, U = 0ull;
    double Ls = 0.0;
    if (s1 > s0) {
        const int64_t ca = s0 / BOOT_CHUNK, cb = (s1 - 1) / BOOT_CHUNK;
        for (int64_t c = ca; c <= cb; ++c) {
            const int64_t c0 = c * BOOT_CHUNK, c1 = c0 + BOOT_CHUNK < n2 ? c0 + BOOT_CHUNK : n2;
            const int64_t df = (int64_t)(keys[c0] >> 33), dl = (int64_t)(keys[c1 - 1] >> 33);
            const unsigned long long* p = df == d ? parts + (c * 2 + 0) * 3 * n_rep : (dl == d ? parts + (c * 2 + 1) * 3 * n_rep
                                                                                               : direct + d * 3 * n_rep);
            const unsigned long long wv = p[r];
            W += wv & 0xffffffffull;
            Wp += wv >> 32;
            U += p[n_rep + r];
            Ls += __longlong_as_double((long long)p[2 * n_rep + r]);
        }
    }
    unsigned long long* o = tot + d * 4 * n_rep;
    o[r] = W; o[n_rep + r] = Wp; o[2 * n_rep + r] = U; o[3 * n_rep + r] = (unsigned long long)__double_as_longlong(Ls);
}

// out: auc [n_rep, n_seg], loss [n_rep, n_seg]; counts (when given): W, Wp.  A thread per replicate walks the segments in sorted order
__global__ void __launch_bounds__(BOOT_THREADS) k_boot_final(const unsigned long long* __restrict__ tot, int32_t n_rep, int32_t n_seg,
                                                             double* __restrict__ out, int64_t* __restrict__ counts) {
    const int64_t r = (int64_t)blockIdx.x * BOOT_THREADS + threadIdx.x;
    if (r >= n_rep) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    unsigned long long before = 0ull;                                      // weighted negatives of the segments in front
    for (int64_t d = 0; d < n_seg; ++d) {
        const unsigned long long* t = tot + d * 4 * n_rep;
        const unsigned long long W = t[r], Wp = t[n_rep + r], Wn = W - Wp;
        const unsigned long long U2 = t[2 * n_rep + r] - 2ull * Wp * before;
        double auc = nan, loss = nan;
        if (Wp > 0ull && Wn > 0ull) {
            auc = (double)U2 / (double)(2ull * Wp * Wn);
            loss = __longlong_as_double((long long)t[3 * n_rep + r]) / (double)W;
        }
        out[r * n_seg + d] = auc;
        out[((int64_t)n_rep + r) * n_seg + d] = loss;
        if (counts) {
            counts[r * n_seg + d] = (int64_t)W;
            counts[((int64_t)n_rep + r) * n_seg + d] = (int64_t)Wp;
        }
        before += Wn;
    }
}

// k_gauc_sum under the replicates' weights: part[d][slice][r] = (sum w omega A, sum w omega), cnt = counted users with w > 0
__global__ void __launch_bounds__(GAUC_THREADS) k_boot_gauc(const uint64_t* __restrict__ keys, const GaucScan* __restrict__ sc,
                                                            const unsigned long long* __restrict__ W, const int64_t* __restrict__ start,
                                                            const double* __restrict__ user_weight, int64_t n_user, int64_t n2,
                                                            int32_t n_rep, uint64_t seed, double* __restrict__ part,
                                                            int64_t* __restrict__ part_cnt) {
    __shared__ double s_red[GAUC_THREADS / 64][BOOT_REP_TILE * 3];
    const int d = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s0 = start[d], s1 = start[d + 1];
    const int64_t per = (s1 - s0 + GAUC_SLICES - 1) / GAUC_SLICES;
    const int64_t a = s0 + (int64_t)sl * per, b = a + per < s1 ? a + per : s1;
    const uint64_t gbase = (uint64_t)d * (uint64_t)n_user;
    const int ntiles = (n_rep + BOOT_REP_TILE - 1) / BOOT_REP_TILE;
    for (int t = blockIdx.z; t < ntiles; t += gridDim.z) {
        uint64_t base[BOOT_REP_TILE];
        double num[BOOT_REP_TILE], den[BOOT_REP_TILE], cnt[BOOT_REP_TILE];     // cnt: a count below 2^31, exact in a double
#pragma unroll
        for (int r = 0; r < BOOT_REP_TILE; ++r) {
            base[r] = boot_rep_base(seed, (uint32_t)(t * BOOT_REP_TILE + r));
            num[r] = 0.0; den[r] = 0.0; cnt[r] = 0.0;
        }
        for (int64_t i = a + tid; i < b; i += GAUC_THREADS) {
            const uint64_t g = keys[i] >> 32;
            if (i + 1 < n2 && (keys[i + 1] >> 32) == g) continue;          // not the last row of its group
            const GaucScan e = sc[i];
            const int64_t h = e.h;
            const int64_t rows = i - h + 1;
            const int64_t N = (int64_t)(e.cn - (h ? sc[h - 1].cn : 0u)), P = rows - N;
            if (P == 0 || N == 0) continue;
            const unsigned long long u2 = W[i] - (h ? W[h - 1] : 0ull);
            const double auc = (double)u2 / (2.0 * (double)P * (double)N);  // k_gauc_sum's expression
            const double w = user_weight ? user_weight[g - gbase] : (double)rows;
            const uint32_t u = (uint32_t)(g - gbase);
#pragma unroll
            for (int r = 0; r < BOOT_REP_TILE; ++r) {
                const uint32_t wt = boot_weight(base[r], u);
                if (wt == 0u) continue;
                const double ww = (double)wt * w;
                num[r] += ww * auc;
                den[r] += ww;
                cnt[r] += 1.0;
            }
        }
#pragma unroll
        for (int r = 0; r < BOOT_REP_TILE; ++r) {
            const double x = wave_sum_d(num[r]), y = wave_sum_d(den[r]), z = wave_sum_d(cnt[r]);
            if (lane == 0) { s_red[wave][r * 3] = x; s_red[wave][r * 3 + 1] = y; s_red[wave][r * 3 + 2] = z; }
        }
        __syncthreads();
        if (tid < BOOT_REP_TILE * 3) {
            const int r = tid / 3, q = tid - 3 * r, rr = t * BOOT_REP_TILE + r;
            double v = 0.0;
            for (int w = 0; w < GAUC_THREADS / 64; ++w) v += s_red[w][tid];
            if (rr < n_rep) {
                const int64_t o = ((int64_t)d * GAUC_SLICES + sl) * n_rep + rr;
                if (q < 2) part[o * 2 + q] = v; else part_cnt[o] = (int64_t)v;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(BOOT_THREADS) k_boot_gauc_final(const double* __restrict__ part, const int64_t* __restrict__ part_cnt,
                                                                  int32_t n_rep, int32_t n_seg, double* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * BOOT_THREADS + threadIdx.x;
    const int64_t d = id / n_rep, r = id - d * n_rep;
    if (d >= n_seg) return;
    double num = 0.0, den = 0.0;
    int64_t cnt = 0;
    for (int sl = 0; sl < GAUC_SLICES; ++sl) {
        const int64_t o = (d * GAUC_SLICES + sl) * n_rep + r;
        num += part[o * 2]; den += part[o * 2 + 1]; cnt += part_cnt[o];
    }
    out[r * n_seg + d] = cnt > 0 ? num / den : __longlong_as_double(0x7ff8000000000000ll);
}

struct BootLayout {
    MetLayout m;                        // once the sort has run, keys_in holds the loss terms and pay_in the clusters
    int64_t f, ntot, ntail, off, parts, direct, tot, gauc, gpart, gcnt;
    int64_t nchunks;
    GaucLayout g;                       // cdc_eval_gauc's arrays, offsets from `gauc`
};
static void boot_fixed_layout(int64_t n, int32_t n_domain, int32_t n_rep, int32_t gauc, BootLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1, nc = cdc_ceil_div(n2, BOOT_CHUNK), R = n_rep;
    MetCursor c;
    L->nchunks = nc;
    L->m.keys(c, n2, 4);
    L->f = c.take(n2 * 4);
    L->m.starts(c, seg);
    L->ntot = c.take(R * nc * 4);
    L->ntail = c.take(R * nc * 4);
    L->off = c.take(R * (nc + 1) * 8);
    L->parts = c.take(nc * 2 * 3 * R * 8);
    L->direct = c.take(seg * 3 * R * 8);
    L->tot = c.take(seg * 4 * R * 8);
    L->gauc = L->gpart = L->gcnt = c.off;
    if (gauc) {
        gauc_fixed_layout(n, n_domain, &L->g);
        c.off += L->g.m.total;
        L->gpart = c.take(seg * GAUC_SLICES * R * 2 * 8);
        L->gcnt = c.take(seg * GAUC_SLICES * R * 8);
    }
    L->m.end_fixed(c);
}
static int boot_temp(int64_t n, int32_t gauc, BootLayout* L) {
    MetTemp t;
    t.sort_pairs<uint32_t>((size_t)(2 * n));
    const int rc = gauc ? gauc_temp(n, "eval_bootstrap", &L->m, t) : t.done("eval_bootstrap", &L->m);
    if (rc == 0 && gauc) {                                                  // as gauc_order reads them: from the sub-block's base
        L->g.m.temp = L->m.temp - L->gauc;
        L->g.m.temp_bytes = L->m.temp_bytes;
    }
    return rc;
}
// 72 n^2 bounds U2 and 2 Wp Wn (weights <= 12): it must fit 64 bits
static bool boot_sizes_ok(int64_t n, int32_t n_domain, int32_t n_rep) {
    return n > 0 && n < (1ll << 28) && n_domain > 0 && n_domain < (1 << 20) && n_rep >= 1 && n_rep <= BOOT_MAX_REP;
}

extern "C" int64_t cdc_eval_bootstrap_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_cluster, int32_t n_rep, int32_t gauc) {
    if (!boot_sizes_ok(n, n_domain, n_rep)) return 0;
    if (gauc && !gauc_sizes_ok(n, n_domain, n_cluster)) return 0;
    BootLayout L;
    boot_fixed_layout(n, n_domain, n_rep, gauc != 0, &L);
    if (boot_temp(n, gauc != 0, &L) != 0) return -1;
    return L.m.total;
}

extern "C" int cdc_eval_bootstrap(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* cluster, int64_t ld_cluster,
                                  int64_t n_cluster, const int32_t* domain, int64_t ld_domain, int32_t n_domain, const double* user_weight,
                                  int64_t n, int32_t n_rep, uint64_t seed, int32_t gauc, double* out, int64_t* counts, int32_t* err_flag,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred_a && label && out && counts && workspace, CDC_E_BADARG, "eval_bootstrap: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_cluster >= 0 && ld_domain >= 0 && (!cluster || n_cluster > 0),
                  CDC_E_BADARG, "eval_bootstrap: bad sizes n=%ld n_domain=%d n_cluster=%ld", (long)n, n_domain, (long)n_cluster);
    MET_TRY(met_need_domain("eval_bootstrap", domain, n_domain));
    CDC_CHECK_ARG(n_rep >= 1 && n_rep <= BOOT_MAX_REP, CDC_E_BADARG, "eval_bootstrap: n_rep=%d outside [1, %d]", n_rep, BOOT_MAX_REP);
    CDC_CHECK_ARG(!gauc || cluster, CDC_E_BADARG, "eval_bootstrap: GAUC needs the cluster column (a row's user)");
    CDC_CHECK_ARG(n < (1ll << 28), CDC_E_TOOBIG, "eval_bootstrap: n=%ld exceeds the 2^28 rows whose weighted pair count fits 64 bits", (long)n);
    CDC_CHECK_ARG(!gauc || gauc_sizes_ok(n, n_domain, n_cluster), CDC_E_BADARG,
                  "eval_bootstrap: (n_domain + 1) * n_cluster = %ld * %ld group ids exceed 2^32", (long)n_domain + 1, (long)n_cluster);
    gauc = gauc != 0;
    const int32_t paired = pred_b != nullptr;
    BootLayout L;
    boot_fixed_layout(n, n_domain, n_rep, gauc, &L);
    MET_TRY(met_gate("eval_bootstrap", workspace, workspace_bytes, &L.m, [&] { return boot_temp(n, gauc, &L); }));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_in = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* idx_in = ws.ptr<uint32_t>(L.m.pay_in);
    uint32_t* idx = ws.ptr<uint32_t>(L.m.pay_out);
    double* term = (double*)keys_in;                                // the unsorted keys and payloads are dead once the sort has run
    uint32_t* cl = idx_in;
    uint32_t* f = ws.ptr<uint32_t>(L.f);
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    uint32_t* ntot = ws.ptr<uint32_t>(L.ntot);
    uint32_t* ntail = ws.ptr<uint32_t>(L.ntail);
    unsigned long long* off = ws.ptr<unsigned long long>(L.off);
    unsigned long long* parts = ws.ptr<unsigned long long>(L.parts);
    unsigned long long* direct = ws.ptr<unsigned long long>(L.direct);
    unsigned long long* tot = ws.ptr<unsigned long long>(L.tot);
    char* gbase = ws.ptr<char>(L.gauc);
    double* gpart = ws.ptr<double>(L.gpart);
    int64_t* gcnt = ws.ptr<int64_t>(L.gcnt);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n, nc = L.nchunks;
    const int seg = n_domain + 1, n_stat = 2 + gauc;
    const int ntiles = (n_rep + BOOT_REP_TILE - 1) / BOOT_REP_TILE;
    // the chunk passes put replicate tiles side by side only while the grid is small: a chunk's rows are read once per workgroup.
    // GAUC's slices are uneven ("all rows" holds half the positions in 64 of them), so there the tiles go side by side much longer
    const int gy = (int)std::min<int64_t>(ntiles, std::max<int64_t>(1, 2048 / nc));
    const int gz = (int)std::min<int64_t>(ntiles, std::max<int64_t>(1, 131072 / ((int64_t)seg * GAUC_SLICES)));
    const int end_bit = met_end_bit((uint64_t)n_domain, 33);
    for (int v = 0; v <= paired; ++v) {
        const float* pred = v ? pred_b : pred_a;
        double* o = out + (int64_t)v * n_stat * n_rep * seg;
        int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
        hipLaunchKernelGGL(k_boot_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, cluster, ld_cluster, n_cluster, domain,
                           ld_domain, n, n_domain, keys_in, idx_in, err_flag);
        CDC_LAUNCH_CHECK("eval_bootstrap(keys)");
        MET_TRY(met_sort("eval_bootstrap", ws.base, L.m, (const uint32_t*)idx_in, idx, (size_t)n2, end_bit, st));
        hipLaunchKernelGGL(k_boot_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, (const uint64_t*)keys, n2, seg, start);
        CDC_LAUNCH_CHECK("eval_bootstrap(starts)");
        blocks = (int)std::min<int64_t>(cdc_ceil_div(n2, MET_THREADS), 8192);
        hipLaunchKernelGGL(k_boot_prep, dim3(blocks), dim3(MET_THREADS), 0, st, (const uint64_t*)keys, (const uint32_t*)idx, cluster,
                           ld_cluster, n_cluster, n, n2, cl, term, f);
        CDC_LAUNCH_CHECK("eval_bootstrap(prep)");
        hipLaunchKernelGGL(k_boot_totals, dim3((unsigned)nc, gy), dim3(BOOT_THREADS), 0, st, (const uint64_t*)keys, (const uint32_t*)cl,
                           (const uint32_t*)f, n2, nc, n_rep, seed, ntot, ntail);
        CDC_LAUNCH_CHECK("eval_bootstrap(totals)");
        hipLaunchKernelGGL(k_boot_scan, dim3(n_rep), dim3(BOOT_THREADS), 0, st, (const uint32_t*)ntot, nc, off);
        CDC_LAUNCH_CHECK("eval_bootstrap(scan)");
        hipLaunchKernelGGL(k_boot_pass, dim3((unsigned)nc, gy), dim3(BOOT_THREADS), 0, st, (const uint64_t*)keys, (const uint32_t*)cl,
                           (const double*)term, (const uint32_t*)f, (const int64_t*)start, n2, nc, n_rep, seed, (const uint32_t*)ntail,
                           (const unsigned long long*)off, parts, direct);
        CDC_LAUNCH_CHECK("eval_bootstrap(pass)");
        hipLaunchKernelGGL(k_boot_reduce, dim3((unsigned)cdc_ceil_div((int64_t)seg * n_rep, BOOT_THREADS)), dim3(BOOT_THREADS), 0, st,
                           (const uint64_t*)keys, (const int64_t*)start, n2, n_rep, seg, (const unsigned long long*)parts,
                           (const unsigned long long*)direct, tot);
        CDC_LAUNCH_CHECK("eval_bootstrap(reduce)");
        hipLaunchKernelGGL(k_boot_final, dim3((unsigned)cdc_ceil_div(n_rep, BOOT_THREADS)), dim3(BOOT_THREADS), 0, st,
                           (const unsigned long long*)tot, n_rep, seg, o, v ? (int64_t*)nullptr : counts);   // the counts follow from the
        CDC_LAUNCH_CHECK("eval_bootstrap(final)");                                                         // labels and weights alone
        if (!gauc) continue;
        const MetWs gws{gbase};
        unsigned long long* Wg = gws.ptr<unsigned long long>(L.g.m.keys_in);
        MET_TRY(gauc_order(pred, label, cluster, ld_cluster, n_cluster, domain, ld_domain, n_domain, n, err_flag, gbase, L.g, Wg,
                        "eval_bootstrap", st));
        hipLaunchKernelGGL(k_boot_gauc, dim3(seg, GAUC_SLICES, gz), dim3(GAUC_THREADS), 0, st, gws.ptr<const uint64_t>(L.g.m.keys_out),
                           gws.ptr<const GaucScan>(L.g.scan), (const unsigned long long*)Wg, gws.ptr<const int64_t>(L.g.m.start),
                           user_weight, n_cluster, n2, n_rep, seed, gpart, gcnt);
        CDC_LAUNCH_CHECK("eval_bootstrap(gauc)");
        hipLaunchKernelGGL(k_boot_gauc_final, dim3((unsigned)cdc_ceil_div((int64_t)seg * n_rep, BOOT_THREADS)), dim3(BOOT_THREADS), 0, st,
                           (const double*)gpart, (const int64_t*)gcnt, n_rep, seg, o + (int64_t)2 * n_rep * seg);
        CDC_LAUNCH_CHECK("eval_bootstrap(gauc final)");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Clustered bootstrap of the calibration figures: replicate r gives row i the weight w_i = boot_weight(boot_rep_base(seed, r),
// cluster_i) — cdc_eval_bootstrap's weight — and its figures are cdc_eval_calibration's on the multiset that holds row i w_i times.
// Per replicate and segment: W = sum w, Wp = sum w y, SQ = sum w q, the halves of sum w (q - y 2^32)^2, and per bin (sum w q,
// sum w y) for the equal-width bins (a function of p alone) and the equal-mass bins: with the segment's rows in (score, label) order
// row i holds the expanded positions [R_i, R_i + w_i), R_i the weight in front of it, and bin b the expanded positions
// [floor(b W / K), floor((b+1) W / K)) — a row's copies may lie in several bins.
//
//   keys    k_calib_keys' keys (the prediction clamped into [0, 1]) with the copy index as payload; one radix sort
//   prep    the cluster of every sorted position (replicate-free); q, the label and the width bin come back out of the key
//   totals  workgroup = CALBOOT_CHUNK sorted positions: the chunk's weight per replicate;  scan: k_boot_scan's exclusive sums
//   segoff  the weight in front of every segment's first position: the chunk's offset + the weights between the chunk's start and it
//   pass    the same chunks, a wave owns 4 rounds of 64 consecutive positions.  Per replicate: a wave scan gives R_i; a lane adds
//           (w q, w y) to its width cell, the Brier halves to its segment and (copies q, copies y) to every mass bin its copies lie
//           in (bin of an expanded position e: floor(((e + 1) K - 1) / W), estimated in double and corrected by integer products).
//           The lanes of one cell are added in a shuffle tree; the wave keeps ONE open cell per stream in registers across its
//           rounds and hands it over, with integer atomic adds, where the cell changes
//   final   a wave per (replicate, segment): sum_b |sum q_b - positives_b 2^32| over both binnings, then cal_seg_figures
// All sums are exact integers: the same rows in any order give the same bits, and a replicate's doubles are k_calib_final's on the
// expanded rows.  No per-row weights in memory, no workgroup waits for another; the launches depend on the sizes and pred_b alone.
#define CALBOOT_THREADS 256
#define CALBOOT_ROUNDS 4
#define CALBOOT_CHUNK 1024              // sorted positions per workgroup: CALBOOT_THREADS * CALBOOT_ROUNDS (12 * CALBOOT_CHUNK < 2^16)
#define CALBOOT_REP_TILE 8              // replicates whose weights a lane holds at a time: 8 weights of 4 bits to a word
#define CALBOOT_MAX_CELLS (1 << 22)     // n_rep * (n_domain + 1) * n_bins
#define CALBOOT_WAVES (CALBOOT_THREADS / 64)
static_assert(CALBOOT_CHUNK == CALBOOT_THREADS * CALBOOT_ROUNDS && CALBOOT_CHUNK == BOOT_CHUNK && CALBOOT_REP_TILE == 8 &&
              CALBOOT_THREADS == BOOT_THREADS, "k_boot_scan and the 4-bit weights serve both bootstraps");

__global__ void __launch_bounds__(MET_THREADS) k_cboot_keys(const float* __restrict__ pred, const int16_t* __restrict__ label,
                                                            const int32_t* __restrict__ cluster, int64_t ld_cluster, int64_t n_cluster,
                                                            const int32_t* __restrict__ domain, int64_t ld_domain, int64_t n,
                                                            int32_t n_domain, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                            int32_t* __restrict__ err) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float p = pred[i];
        int32_t d = domain ? domain[i * ld_domain] : 0;
        const int64_t u = cluster ? (int64_t)cluster[i * ld_cluster] : 0;
        const int16_t y = label[i];
        const bool bad_p = !(p >= 0.f && p <= 1.f);                       // a NaN too
        if (bad_p || d < 0 || d >= n_domain || u < 0 || (cluster && u >= n_cluster) || (y != 0 && y != 1)) {
            if (err) met_flag_row(err, i);
            d = met_clamp_id(d, n_domain);
            if (bad_p) p = p > 1.f ? 1.f : 0.f;                           // as k_calib_keys clamps
        }
        met_write_pair(keys, idx, n, i, (uint32_t)d, (uint32_t)n_domain, 33, ((uint64_t)score_key(p) << 1) | (uint64_t)(y != 0), (uint32_t)i,
                       (uint32_t)(n + i));
    }
}

// the cluster of every sorted position (clamped as k_boot_prep clamps it); clears the n_acc sums of the pass
__global__ void __launch_bounds__(MET_THREADS) k_cboot_prep(const uint32_t* __restrict__ idx, const int32_t* __restrict__ cluster,
                                                            int64_t ld_cluster, int64_t n_cluster, int64_t n, int64_t n2,
                                                            uint32_t* __restrict__ cl, unsigned long long* __restrict__ acc, int64_t n_acc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const int64_t j = idx[i], row = j >= n ? j - n : j;
        int64_t u = row;
        if (cluster) {
            u = cluster[row * ld_cluster];
            u = u < 0 ? 0 : (u >= n_cluster ? n_cluster - 1 : u);
        }
        cl[i] = (uint32_t)u;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_acc; i += stride) acc[i] = 0ull;
}

// the weight of a range of at most CALBOOT_CHUNK sorted positions, per replicate.  SEG false: workgroup c sums chunk c into
// ntot[r][c].  SEG true: workgroup d (d <= n_seg) sums the positions between the start of the chunk that holds start[d] and
// start[d], and writes segoff[r][d] = the weight in front of start[d] (off[r][nchunks] for an end at n2 on a chunk boundary)
template <bool SEG>
__global__ void __launch_bounds__(CALBOOT_THREADS) k_cboot_sums(const uint32_t* __restrict__ cl, const int64_t* __restrict__ start,
                                                                int64_t n2, int64_t nchunks, int32_t n_seg, int32_t n_rep, uint64_t seed,
                                                                const unsigned long long* __restrict__ off, uint32_t* __restrict__ ntot,
                                                                unsigned long long* __restrict__ segoff) {
    __shared__ uint32_t sh[CALBOOT_WAVES][CALBOOT_REP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t c, lo, hi;
    if (SEG) {
        hi = start[blockIdx.x];
        c = hi / CALBOOT_CHUNK;
        lo = c * CALBOOT_CHUNK;
    } else {
        c = blockIdx.x;
        lo = c * CALBOOT_CHUNK;
        hi = lo + CALBOOT_CHUNK < n2 ? lo + CALBOOT_CHUNK : n2;
    }
    bool ok[CALBOOT_ROUNDS];
    uint32_t clu[CALBOOT_ROUNDS];
#pragma unroll
    for (int k = 0; k < CALBOOT_ROUNDS; ++k) {
        const int64_t pos = lo + (int64_t)k * CALBOOT_THREADS + tid;
        ok[k] = pos < hi;
        clu[k] = ok[k] ? cl[pos] : 0u;
    }
    const int ntiles = (n_rep + CALBOOT_REP_TILE - 1) / CALBOOT_REP_TILE;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        uint32_t v[CALBOOT_REP_TILE];
#pragma unroll
        for (int r = 0; r < CALBOOT_REP_TILE; ++r) {
            const uint64_t base = boot_rep_base(seed, (uint32_t)(t * CALBOOT_REP_TILE + r));
            uint32_t a = 0u;
#pragma unroll
            for (int k = 0; k < CALBOOT_ROUNDS; ++k)
                if (ok[k]) a += boot_weight(base, clu[k]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            v[r] = a;
        }
        if (lane == 0)
            for (int r = 0; r < CALBOOT_REP_TILE; ++r) sh[wave][r] = v[r];
        __syncthreads();
        if (tid < CALBOOT_REP_TILE) {
            uint32_t s = 0u;
            for (int w = 0; w < CALBOOT_WAVES; ++w) s += sh[w][tid];
            const int64_t rr = (int64_t)t * CALBOOT_REP_TILE + tid;
            if (rr < n_rep) {
                if (SEG) segoff[rr * (n_seg + 1) + blockIdx.x] = off[rr * (nchunks + 1) + c] + (unsigned long long)s;
                else ntot[rr * nchunks + c] = s;
            }
        }
        __syncthreads();
    }
}

// floor(num / den) from the double estimate num * inv (inv close to 1 / den, num < 2^53), made exact by integer products
__device__ __forceinline__ unsigned long long cboot_floor_div(unsigned long long num, unsigned long long den, double inv) {
    unsigned long long v = (unsigned long long)((double)num * inv);
    while (v > 0ull && v * den > num) --v;
    while ((v + 1ull) * den <= num) ++v;
    return v;
}
// the mass bin of expanded position e of a segment of weight W (e < W < 2^32, K <= 1024): the b with
// floor(b W / K) <= e < floor((b+1) W / K), as cal_cell forms it from a rank
__device__ __forceinline__ int32_t cboot_mass_bin(unsigned long long e, unsigned long long K, unsigned long long W, double inv_w) {
    return (int32_t)cboot_floor_div((e + 1ull) * K - 1ull, W, inv_w);
}

// a stream's open cell: the same in every lane.  cell < 0: nothing open
struct CbOpen { int32_t cell; unsigned long long a, b; };

__device__ __forceinline__ void cboot_hand_over(const CbOpen& o, unsigned long long* __restrict__ acc, int lane) {
    if (o.cell >= 0 && lane == 0) {
        if (o.a) atomicAdd(&acc[2 * (int64_t)o.cell], o.a);
        if (o.b) atomicAdd(&acc[2 * (int64_t)o.cell + 1], o.b);
    }
}
// adds (a, b) of every active lane to acc[its cell]: the lanes of one cell through a shuffle tree into the open cell, which is
// handed over when another cell comes.  The positions are sorted, so a cell's lanes are neighbours and a wave inside one cell
// takes one turn of the loop; any order of cells gives the same sums
__device__ __forceinline__ void cboot_feed(CbOpen& o, bool act, int32_t cell, unsigned long long a, unsigned long long b,
                                           unsigned long long* __restrict__ acc, int lane) {
    unsigned long long todo = __ballot(act);
    while (todo) {
        const int32_t c = __shfl(cell, __ffsll((unsigned long long)todo) - 1, 64);
        const bool mine = act && cell == c;
        const unsigned long long sa = dl_wave_sum(mine ? a : 0ull), sb = dl_wave_sum(mine ? b : 0ull);
        if (c != o.cell) {
            cboot_hand_over(o, acc, lane);
            o.cell = c; o.a = 0ull; o.b = 0ull;
        }
        o.a += sa; o.b += sb;
        todo &= ~__ballot(mine);
    }
}

// acc_w, acc_q [n_rep][n_seg][K][sum w q, sum w y]; acc_seg [n_rep][n_seg][low, high half of sum w (q - y 2^32)^2]
__global__ void __launch_bounds__(CALBOOT_THREADS) k_cboot_pass(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cl,
                                                                int64_t n2, int64_t nchunks, int32_t n_seg, int32_t K, int32_t n_rep,
                                                                uint64_t seed, const unsigned long long* __restrict__ off,
                                                                const unsigned long long* __restrict__ segoff,
                                                                unsigned long long* __restrict__ acc_w,
                                                                unsigned long long* __restrict__ acc_q,
                                                                unsigned long long* __restrict__ acc_seg) {
    __shared__ uint32_t s_wave[CALBOOT_WAVES][CALBOOT_REP_TILE / 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = blockIdx.x, c0 = c * CALBOOT_CHUNK, c1 = c0 + CALBOOT_CHUNK < n2 ? c0 + CALBOOT_CHUNK : n2;
    const double inv_k = 1.0 / (double)K;
    // round k of a wave: the 64 consecutive positions from c0 + (wave * CALBOOT_ROUNDS + k) * 64
    bool ok[CALBOOT_ROUNDS], yv[CALBOOT_ROUNDS];
    uint32_t clu[CALBOOT_ROUNDS];
    int32_t seg[CALBOOT_ROUNDS], bw[CALBOOT_ROUNDS];
    unsigned long long q[CALBOOT_ROUNDS];
#pragma unroll
    for (int k = 0; k < CALBOOT_ROUNDS; ++k) {
        const int64_t pos = c0 + (int64_t)(wave * CALBOOT_ROUNDS + k) * 64 + lane;
        ok[k] = pos < c1; yv[k] = false; clu[k] = 0u; seg[k] = 0; bw[k] = 0; q[k] = 0ull;
        if (ok[k]) {
            const uint64_t key = keys[pos];
            const float p = cal_score(key);
            yv[k] = (key & 1ull) != 0ull;
            clu[k] = cl[pos];
            seg[k] = (int32_t)(key >> 33);
            bw[k] = cal_bin(p, K);
            q[k] = cal_quant(p);
        }
    }
    const int ntiles = (n_rep + CALBOOT_REP_TILE - 1) / CALBOOT_REP_TILE;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        // the tile's weights, 4 bits each, and the wave's weight per replicate, two replicates to a word (12 * 256 < 2^16)
        uint32_t wpk[CALBOOT_ROUNDS] = {0u, 0u, 0u, 0u};
        uint32_t tn[CALBOOT_REP_TILE / 2] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < CALBOOT_REP_TILE; ++r) {
            const uint64_t base = boot_rep_base(seed, (uint32_t)(t * CALBOOT_REP_TILE + r));
#pragma unroll
            for (int k = 0; k < CALBOOT_ROUNDS; ++k) {
                const uint32_t w = ok[k] ? boot_weight(base, clu[k]) : 0u;
                wpk[k] |= w << (4 * r);
                tn[r >> 1] += w << (16 * (r & 1));
            }
        }
#pragma unroll
        for (int j = 0; j < CALBOOT_REP_TILE / 2; ++j) {
            uint32_t v = tn[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) s_wave[wave][j] = v;
        }
        __syncthreads();
        for (int r = 0; r < CALBOOT_REP_TILE; ++r) {
            const int64_t rr = (int64_t)t * CALBOOT_REP_TILE + r;
            if (rr >= n_rep) break;                                        // the same in every thread
            unsigned long long front = off[rr * (nchunks + 1) + c];        // the weight in front of the wave's next round
            for (int w = 0; w < wave; ++w) front += (s_wave[w][r >> 1] >> (16 * (r & 1))) & 0xffffu;
            const unsigned long long* so = segoff + rr * (n_seg + 1);
            const int32_t seg0 = (int32_t)rr * n_seg;
            CbOpen ow = {-1, 0ull, 0ull}, oq = {-1, 0ull, 0ull}, os = {-1, 0ull, 0ull};
#pragma unroll
            for (int k = 0; k < CALBOOT_ROUNDS; ++k) {
                const uint32_t w = (wpk[k] >> (4 * r)) & 15u;
                uint32_t inc = w;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t x = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += x;
                }
                const unsigned long long R = front + (unsigned long long)(inc - w);
                front += (unsigned long long)__shfl(inc, 63, 64);
                const bool act = w != 0u;
                const int32_t sc = seg0 + seg[k];
                const unsigned long long y = yv[k] ? 1ull : 0ull;
                cboot_feed(ow, act, sc * K + bw[k], (unsigned long long)w * q[k], (unsigned long long)w * y, acc_w, lane);
                const unsigned long long e = yv[k] ? 4294967296ull - q[k] : q[k], e2 = e * e;      // cal_add's halves
                cboot_feed(os, act, sc, (unsigned long long)w * (e2 & 0xffffffffull),
                           (unsigned long long)w * ((e2 >> 32) + ((e >> 32) << 32)), acc_seg, lane);
                // the row's copies: expanded positions [pe, pe + rem) of its segment
                unsigned long long pe = 0ull, W = 1ull;
                if (act) {
                    const unsigned long long s0 = so[seg[k]];
                    W = so[seg[k] + 1] - s0;
                    W = W ? W : 1ull;                                      // w > 0 is part of W
                    pe = R - s0;
                }
                const double inv_w = __builtin_amdgcn_rcp((double)W);
                uint32_t rem = w;
                while (__ballot(rem != 0u)) {
                    int32_t b = 0;
                    uint32_t take = 0u;
                    if (rem != 0u) {
                        b = cboot_mass_bin(pe, (unsigned long long)K, W, inv_w);
                        take = rem;
                        if (rem > 1u && cboot_mass_bin(pe + rem - 1u, (unsigned long long)K, W, inv_w) != b)
                            take = (uint32_t)(cboot_floor_div((unsigned long long)(b + 1) * W, (unsigned long long)K, inv_k) - pe);
                        b = b < K - 1 ? b : K - 1;                         // pe < W: both hold by construction; they keep a
                        take = take >= 1u && take <= rem ? take : rem;     // broken invariant from leaving the arrays or the loop
                    }
                    cboot_feed(oq, rem != 0u, sc * K + b, (unsigned long long)take * q[k], (unsigned long long)take * y, acc_q, lane);
                    rem -= take;
                    pe += take;
                }
            }
            cboot_hand_over(ow, acc_w, lane);
            cboot_hand_over(oq, acc_q, lane);
            cboot_hand_over(os, acc_seg, lane);
        }
        __syncthreads();                                                   // s_wave is free for the next tile
    }
}

// out [4][n_rep][n_seg]: pcoc, brier, ece, ece_q; counts (when given) [2][n_rep][n_seg]: W, Wp.  A wave per (replicate, segment)
__global__ void __launch_bounds__(CALBOOT_THREADS) k_cboot_final(const unsigned long long* __restrict__ acc_w,
                                                                 const unsigned long long* __restrict__ acc_q,
                                                                 const unsigned long long* __restrict__ acc_seg,
                                                                 const unsigned long long* __restrict__ segoff, int32_t n_rep,
                                                                 int32_t n_seg, int32_t K, double* __restrict__ out,
                                                                 int64_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t id = (int64_t)blockIdx.x * CALBOOT_WAVES + (threadIdx.x >> 6), total = (int64_t)n_rep * n_seg;
    if (id >= total) return;                                               // a whole wave
    const int64_t rr = id / n_seg, d = id - rr * n_seg;
    const unsigned long long W = segoff[rr * (n_seg + 1) + d + 1] - segoff[rr * (n_seg + 1) + d];
    const unsigned long long* aw = acc_w + 2 * id * K;
    const unsigned long long* aq = acc_q + 2 * id * K;
    unsigned long long Q = 0ull, P = 0ull, gap_w = 0ull, gap_q = 0ull;
    for (int b = lane; b < K; b += 64) {
        unsigned long long s = aw[2 * b], ps = aw[2 * b + 1], obs = ps << 32;
        Q += s; P += ps;
        gap_w += s > obs ? s - obs : obs - s;
        s = aq[2 * b]; obs = aq[2 * b + 1] << 32;
        gap_q += s > obs ? s - obs : obs - s;
    }
    Q = dl_wave_sum(Q); P = dl_wave_sum(P); gap_w = dl_wave_sum(gap_w); gap_q = dl_wave_sum(gap_q);
    if (lane != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double o[4] = {nan, nan, nan, nan};
    if (W > 0ull) cal_seg_figures(W, P, Q, acc_seg[2 * id], acc_seg[2 * id + 1], gap_w, gap_q, &o[0], &o[1], &o[2], &o[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[(int64_t)k * total + id] = o[k];
    if (counts) {
        counts[id] = (int64_t)W;
        counts[total + id] = (int64_t)P;
    }
}

struct CalBootLayout {
    MetLayout m;                        // once the sort has run, pay_in holds the clusters
    int64_t ntot, off, segoff, acc, acc_words;
    int64_t nchunks, cells;
};
// plain arithmetic, rocPRIM's temporary storage included: the size query must answer where no device is present.  The sort gets
// 16 bytes per key and 1 MiB — a second copy of keys and payloads (12 bytes per key), digit histograms and the look-back states of
// its tiles; the call asks rocPRIM what it needs and refuses to run if that is ever more
static void calboot_layout(int64_t n, int32_t n_domain, int32_t n_bins, int32_t n_rep, CalBootLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1, nc = cdc_ceil_div(n2, CALBOOT_CHUNK), R = n_rep;
    MetCursor c;
    L->nchunks = nc;
    L->cells = R * seg * n_bins;
    L->acc_words = 2 * (2 * L->cells + R * seg);               // acc_w, acc_q, acc_seg: one block, cleared together
    L->m.keys(c, n2, 4);
    L->m.starts(c, seg);
    L->ntot = c.take(R * nc * 4);
    L->off = c.take(R * (nc + 1) * 8);
    L->segoff = c.take(R * (seg + 1) * 8);
    L->acc = c.take(L->acc_words * 8);
    L->m.end_fixed(c);
    L->m.set_temp(n2 * 16 + (1 << 20));
}
static bool calboot_sizes_ok(int64_t n, int32_t n_domain, int32_t n_bins, int32_t n_rep) {
    return n > 0 && n < (1ll << 28) && n_domain > 0 && n_domain < (1 << 20) && n_bins >= 1 && n_bins <= CAL_MAX_BINS && n_rep >= 1 &&
           n_rep <= BOOT_MAX_REP && (int64_t)n_rep * ((int64_t)n_domain + 1) * n_bins <= CALBOOT_MAX_CELLS;
}

extern "C" int64_t cdc_eval_calibration_bootstrap_workspace_bytes(int64_t n, int32_t n_domain, int32_t n_bins, int32_t n_rep,
                                                                  int32_t paired) {
    (void)paired;                                                          // the second vector reuses the first one's arrays
    if (!calboot_sizes_ok(n, n_domain, n_bins, n_rep)) return 0;
    CalBootLayout L;
    calboot_layout(n, n_domain, n_bins, n_rep, &L);
    return L.m.total;
}

extern "C" int cdc_eval_calibration_bootstrap(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* cluster,
                                              int64_t ld_cluster, int64_t n_cluster, const int32_t* domain, int64_t ld_domain,
                                              int32_t n_domain, int32_t n_bins, int64_t n, int32_t n_rep, uint64_t seed, double* out,
                                              int64_t* counts, int32_t* err_flag, void* workspace, int64_t workspace_bytes,
                                              void* stream) {
    CDC_CHECK_ARG(pred_a && label && out && counts && workspace, CDC_E_BADARG, "eval_calibration_bootstrap: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && ld_cluster >= 0 && ld_domain >= 0 && (!cluster || n_cluster > 0),
                  CDC_E_BADARG, "eval_calibration_bootstrap: bad sizes n=%ld n_domain=%d n_cluster=%ld", (long)n, n_domain, (long)n_cluster);
    CDC_CHECK_ARG(n_bins >= 1 && n_bins <= CAL_MAX_BINS, CDC_E_BADARG, "eval_calibration_bootstrap: n_bins=%d outside [1, %d]", n_bins,
                  CAL_MAX_BINS);
    CDC_CHECK_ARG(n_rep >= 1 && n_rep <= BOOT_MAX_REP, CDC_E_BADARG, "eval_calibration_bootstrap: n_rep=%d outside [1, %d]", n_rep,
                  BOOT_MAX_REP);
    MET_TRY(met_need_domain("eval_calibration_bootstrap", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 28), CDC_E_TOOBIG, "eval_calibration_bootstrap: n=%ld exceeds the 2^28 rows whose weighted sums fit 64 bits",
                  (long)n);
    CDC_CHECK_ARG((int64_t)n_rep * ((int64_t)n_domain + 1) * n_bins <= CALBOOT_MAX_CELLS, CDC_E_TOOBIG,
                  "eval_calibration_bootstrap: n_rep * (n_domain + 1) * n_bins = %ld cells exceed 2^22",
                  (long)((int64_t)n_rep * ((int64_t)n_domain + 1) * n_bins));
    const int32_t paired = pred_b != nullptr;
    CalBootLayout L;
    calboot_layout(n, n_domain, n_bins, n_rep, &L);
    const auto ask_rocprim = [&]() -> int {                                // the layout is complete: rocPRIM is only asked
        MetLayout asked = L.m;
        MET_TRY(met_pairs32_temp(n, "eval_calibration_bootstrap", &asked));
        CDC_CHECK_ARG(asked.temp_bytes <= L.m.temp_bytes, CDC_E_BADARG,
                      "eval_calibration_bootstrap: the sort needs %ld temporary bytes, %ld reserved", (long)asked.temp_bytes, (long)L.m.temp_bytes);
        return 0;
    };
    MET_TRY(met_gate("eval_calibration_bootstrap", workspace, workspace_bytes, &L.m, ask_rocprim));
    const MetWs ws{(char*)workspace};
    uint64_t* keys_in = ws.ptr<uint64_t>(L.m.keys_in);
    uint64_t* keys = ws.ptr<uint64_t>(L.m.keys_out);
    uint32_t* idx_in = ws.ptr<uint32_t>(L.m.pay_in);
    uint32_t* idx = ws.ptr<uint32_t>(L.m.pay_out);
    uint32_t* cl = idx_in;                                          // the unsorted payloads are dead once the sort has run
    int64_t* start = ws.ptr<int64_t>(L.m.start);
    uint32_t* ntot = ws.ptr<uint32_t>(L.ntot);
    unsigned long long* off = ws.ptr<unsigned long long>(L.off);
    unsigned long long* segoff = ws.ptr<unsigned long long>(L.segoff);
    unsigned long long* acc_w = ws.ptr<unsigned long long>(L.acc);
    unsigned long long* acc_q = acc_w + 2 * L.cells;
    unsigned long long* acc_seg = acc_q + 2 * L.cells;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n, nc = L.nchunks;
    const int seg = n_domain + 1;
    const int ntiles = (n_rep + CALBOOT_REP_TILE - 1) / CALBOOT_REP_TILE;
    // replicate tiles go side by side only while the grid is small, as in cdc_eval_bootstrap
    const int gy = (int)std::min<int64_t>(ntiles, std::max<int64_t>(1, 2048 / nc));
    const int gy_seg = (int)std::min<int64_t>(ntiles, std::max<int64_t>(1, 2048 / (seg + 1)));
    const int end_bit = met_end_bit((uint64_t)n_domain, 33);
    for (int v = 0; v <= paired; ++v) {
        const float* pred = v ? pred_b : pred_a;
        int blocks = (int)std::min<int64_t>(cdc_ceil_div(n, MET_THREADS), 4096);
        hipLaunchKernelGGL(k_cboot_keys, dim3(blocks), dim3(MET_THREADS), 0, st, pred, label, cluster, ld_cluster, n_cluster, domain,
                           ld_domain, n, n_domain, keys_in, idx_in, err_flag);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(keys)");
        MET_TRY(met_sort("eval_calibration_bootstrap", ws.base, L.m, (const uint32_t*)idx_in, idx, (size_t)n2, end_bit, st));
        hipLaunchKernelGGL(k_boot_starts, dim3((int)cdc_ceil_div(seg + 1, 64)), dim3(64), 0, st, (const uint64_t*)keys, n2, seg, start);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(starts)");
        blocks = (int)std::min<int64_t>(cdc_ceil_div(std::max<int64_t>(n2, L.acc_words), MET_THREADS), 8192);
        hipLaunchKernelGGL(k_cboot_prep, dim3(blocks), dim3(MET_THREADS), 0, st, (const uint32_t*)idx, cluster, ld_cluster, n_cluster, n, n2,
                           cl, acc_w, L.acc_words);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(prep)");
        hipLaunchKernelGGL(k_cboot_sums<false>, dim3((unsigned)nc, gy), dim3(CALBOOT_THREADS), 0, st, (const uint32_t*)cl,
                           (const int64_t*)start, n2, nc, seg, n_rep, seed, (const unsigned long long*)off, ntot, segoff);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(totals)");
        hipLaunchKernelGGL(k_boot_scan, dim3(n_rep), dim3(BOOT_THREADS), 0, st, (const uint32_t*)ntot, nc, off);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(scan)");
        hipLaunchKernelGGL(k_cboot_sums<true>, dim3((unsigned)(seg + 1), gy_seg), dim3(CALBOOT_THREADS), 0, st, (const uint32_t*)cl,
                           (const int64_t*)start, n2, nc, seg, n_rep, seed, (const unsigned long long*)off, ntot, segoff);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(segment offsets)");
        hipLaunchKernelGGL(k_cboot_pass, dim3((unsigned)nc, gy), dim3(CALBOOT_THREADS), 0, st, (const uint64_t*)keys, (const uint32_t*)cl,
                           n2, nc, seg, n_bins, n_rep, seed, (const unsigned long long*)off, (const unsigned long long*)segoff, acc_w,
                           acc_q, acc_seg);
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(pass)");
        hipLaunchKernelGGL(k_cboot_final, dim3((unsigned)cdc_ceil_div((int64_t)n_rep * seg, CALBOOT_WAVES)), dim3(CALBOOT_THREADS), 0, st,
                           (const unsigned long long*)acc_w, (const unsigned long long*)acc_q, (const unsigned long long*)acc_seg,
                           (const unsigned long long*)segoff, n_rep, seg, n_bins, out + (int64_t)v * 4 * n_rep * seg,
                           v ? (int64_t*)nullptr : counts);                 // the counts follow from the labels and weights alone
        CDC_LAUNCH_CHECK("eval_calibration_bootstrap(final)");
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// User-clustered standard errors, paired deltas and bootstrap replicates of the top-K figures.  Groups, walk and figures are
// cdc_eval_rank's, the variance is cdc_eval_gauc_ci's linearised ratio form with clusters = users, the replicate weights are
// cdc_eval_bootstrap's boot_weight(boot_rep_base(seed, r), user):
//
//   order   gauc_order() without its second scan, once per vector.  The upper key halves of the two vectors are the same multiset, so a
//           group ends at the SAME sorted position in both orders, with the same h and cn there; of the second vector's order only its
//           scan (the tie runs inside a group differ) is kept
//   pass 1  k_rank_sum / k_rank_final exactly as cdc_eval_rank launches them, once per vector: M and M_b are its figures bit for bit
//   pass 2  k_rank_ci_pass: a domain's stretch is cut into S = rank_ci_slices() slices and the "all rows" stretch — n of the 2 n
//           positions, which the host knows — into min(n_domain S, 512), so that the slices are of one length on average; a workgroup
//           walks its slice in chunks of
//           CH = rank_ci_chunk() sorted positions, at most one group end per thread (paired: one half of the threads walks the first
//           vector's order, the other half the second's, position for position).  The counted groups of a chunk are numbered in position
//           order (ballot + wave counts) and parked in LDS: 5 n_k values per vector, the weight and the user id — at most 61 KB
//           (n_k = 4, unpaired; CH halves above 4 cut-offs), so a CU of 160 KB holds two workgroups.  After a barrier the threads re-map:
//             squares     (replicate tile 0 only) lane = value, wave = every fourth group: (w (m - M))^2 with M read from device memory,
//                         paired also (w (m_b - M_b))^2 and (w ((m - m_b) - delta))^2, carried in registers across the slice's chunks
//             replicates  lane = replicate of the workgroup's tile of RANK_CI_REP_TILE = 64: the chunk's weights are hashed once into LDS
//                         (a byte each), then wave q adds w(seed, r, u_g) w_g m_g of the chunk's groups IN POSITION ORDER into the
//                         columns q, q + 4, .. — (5 n_k values per vector, sum of weights) / 4 register accumulators per thread
//           m_g does not depend on the replicate: a group is walked once per tile of 64 replicates (4 times for 200), not once per replicate
//   final   k_rank_ci_final: the slices' squares in slice order, cdc_eval_rank's tree for sum w, the variances and the delta;
//           k_rank_ci_rep_final: a thread per (segment, value, replicate) adds the slices' partials in slice order and divides
// The replicate partials are [slice, column, replicate] doubles: with S = 512 / (n_domain + 1) clamped into [8, 64] that is
// (50 * 10 + 500) * 21 * 200 * 8 = 34 MB at 50 domains, 200 replicates and 4 cut-offs (66 MB paired); RANK_SLICES = 256 slices per
// segment would be 439 MB.
// No per-group array, nothing indexed by a user id, no float atomics: every addition's order is a function of the sorted keys alone —
// same rows, same bits.  The launch dimensions depend on (n, n_domain, n_k, paired, n_rep) alone.
#define RANK_CI_REP_TILE 64
#define RANK_CI_MAX_CELLS (1 << 20)     // n_rep * (n_domain + 1) * n_k
#define RANK_CI_WAVES (GAUC_THREADS / 64)

__host__ __device__ constexpr int rank_ci_chunk(int n_k, bool paired) { return (n_k <= 4 ? 256 : 128) / (paired ? 2 : 1); }
static int rank_ci_slices(int32_t n_domain) {                              // per domain
    const int s = 512 / (n_domain + 1);
    return s < 8 ? 8 : (s > 64 ? 64 : s);
}
static int rank_ci_slices_all(int32_t n_domain) {                          // of the "all rows" stretch
    const int64_t s = (int64_t)n_domain * rank_ci_slices(n_domain);
    return (int)(s > 512 ? 512 : s);
}
// slice `cell` of the launch -> its (pseudo-)domain, its index there and the domain's slice count; a domain's first cell
__device__ __forceinline__ void rank_ci_cell(int cell, int n_domain, int n_sl, int n_sl_all, int* d, int* sl, int* n) {
    if (cell < n_domain * n_sl) { *d = cell / n_sl; *sl = cell - *d * n_sl; *n = n_sl; }
    else { *d = n_domain; *sl = cell - n_domain * n_sl; *n = n_sl_all; }
}

template <int NK, bool PAIRED>
__global__ void __launch_bounds__(GAUC_THREADS) k_rank_ci_pass(const uint64_t* __restrict__ keys, const GaucScan* __restrict__ sc,
                                                               const GaucScan* __restrict__ sc_b, const int64_t* __restrict__ start,
                                                               const double* __restrict__ user_weight, const int32_t* __restrict__ ks,
                                                               const double* __restrict__ D, int64_t n_user, int64_t n2, int32_t n_seg,
                                                               int32_t n_sl, int32_t n_sl_all, int32_t n_rep, uint64_t seed,
                                                               const double* __restrict__ out,
                                                               double* __restrict__ part_sq, double* __restrict__ part_rep,
                                                               int64_t* __restrict__ part_rep_cnt) {
    constexpr int NVAL = RANK_FIGS * NK, NVEC = PAIRED ? 2 : 1, NCV = NVEC * NVAL, NCOL = NCV + 1, NSQ = PAIRED ? 3 : 1;
    constexpr int CH = rank_ci_chunk(NK, PAIRED), WPV = CH / 64, NQ = (NCOL + RANK_CI_WAVES - 1) / RANK_CI_WAVES;
    static_assert(CH % 64 == 0 && NVEC * CH <= GAUC_THREADS && NVAL <= 64, "rank_ci chunk arithmetic");
    __shared__ double s_v[NCV][CH + 1];                                    // the odd row length spreads a column over the banks
    __shared__ double s_w[CH];
    __shared__ uint32_t s_u[CH];
    __shared__ uint8_t s_wt[CH][RANK_CI_REP_TILE];
    __shared__ double s_sq[RANK_CI_WAVES][NSQ][NVAL];
    __shared__ int s_wc[RANK_CI_WAVES];
    const int tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int d, sl, n_sl_d;
    rank_ci_cell(blockIdx.x, n_seg - 1, n_sl, n_sl_all, &d, &sl, &n_sl_d);
    const int vec = tid / CH, sidx = tid % CH, wv0 = vec * WPV;
    const bool walker = vec < NVEC;
    const GaucScan* __restrict__ scv = PAIRED && vec == 1 ? sc_b : sc;
    const int64_t s0 = start[d], s1 = start[d + 1];
    const int64_t per = (s1 - s0 + n_sl_d - 1) / n_sl_d;
    const int64_t a0 = s0 + (int64_t)sl * per, b0 = a0 + per < s1 ? a0 + per : s1;
    const uint64_t base = (uint64_t)d * (uint64_t)n_user;
    int32_t K[NK];
    double DK[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        int32_t v = ks[k];
        v = v < 1 ? 1 : (v > RANK_MAX_K ? RANK_MAX_K : v);
        K[k] = v;
        DK[k] = D[v];
    }
    const int64_t k_max = K[NK - 1];
    const bool squares = tile == 0 && lane < NVAL;
    double M = 0.0, M_b = 0.0;                                             // NaN when no group is counted: then none is added
    if (squares) {
        M = out[(int64_t)lane * n_seg + d];
        if constexpr (PAIRED) M_b = out[((int64_t)2 * NVAL + lane) * n_seg + d];
    }
    const double delta = M - M_b;
    double qa = 0.0, qb = 0.0, qd = 0.0;
    const uint64_t rbase = boot_rep_base(seed, (uint32_t)(tile * RANK_CI_REP_TILE + lane));
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    int64_t cnt = 0;
    for (int64_t cb = a0; cb < b0; cb += CH) {
        const int64_t i = cb + sidx;
        bool counted = false;
        GaucScan e;
        e.h = e.f = e.cn = 0u;
        int64_t h = 0, P = 0;
        uint64_t g = 0;
        if (walker && i < b0) {
            g = keys[i] >> 32;
            if (!(i + 1 < n2 && (keys[i + 1] >> 32) == g)) {               // the last row of its group
                e = scv[i];
                h = e.h;
                P = (i - h + 1) - (int64_t)(e.cn - (h ? scv[h - 1].cn : 0u));
                counted = P > 0;
            }
        }
        const unsigned long long bal = __ballot(counted);
        if (lane == 0) s_wc[wv] = __popcll(bal);
        __syncthreads();
        int ng = 0;                                                        // the chunk's counted groups: the first vector's waves
#pragma unroll
        for (int j = 0; j < WPV; ++j) ng += s_wc[j];
        if (counted) {
            int slot = __popcll(bal & ((1ull << lane) - 1ull));
            for (int j = wv0; j < wv; ++j) slot += s_wc[j];
            double m[RANK_FIGS][NK];
            rank_group<NK>(scv, D, K, DK, k_max, i, e, h, P, m);
#pragma unroll
            for (int f = 0; f < RANK_FIGS; ++f)
#pragma unroll
                for (int k = 0; k < NK; ++k) s_v[vec * NVAL + f * NK + k][slot] = m[f][k];
            if (vec == 0) {
                s_w[slot] = user_weight ? user_weight[g - base] : 1.0;
                s_u[slot] = (uint32_t)(g - base);
            }
        }
        __syncthreads();
        if (squares) {
            for (int gi = wv; gi < ng; gi += RANK_CI_WAVES) {
                const double w = s_w[gi], ma = s_v[lane][gi];
                const double ta = w * (ma - M);
                qa += ta * ta;
                if constexpr (PAIRED) {
                    const double mb = s_v[NVAL + lane][gi];
                    const double tb = w * (mb - M_b), td = w * ((ma - mb) - delta);
                    qb += tb * tb;
                    qd += td * td;
                }
            }
        }
        if (n_rep > 0) {
            for (int gi = wv; gi < ng; gi += RANK_CI_WAVES) s_wt[gi][lane] = (uint8_t)boot_weight(rbase, s_u[gi]);
            __syncthreads();
            for (int gi = 0; gi < ng; ++gi) {
                const uint32_t wt = s_wt[gi][lane];
                const double ww = (double)wt * s_w[gi];                    // a weight of 0 adds +0.0: the sums keep their bits
                cnt += wt != 0u;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int c = wv + RANK_CI_WAVES * q;
                    if (c < NCOL) acc[q] += ww * (c < NCV ? s_v[c < NCV ? c : 0][gi] : 1.0);
                }
            }
        }
        // no barrier here: nothing above is overwritten before the next chunk's first barrier, which every wave has to reach
    }
    const int64_t o = blockIdx.x;
    if (tile == 0) {
        if (lane < NVAL) {
            s_sq[wv][0][lane] = qa;
            if constexpr (PAIRED) { s_sq[wv][1][lane] = qb; s_sq[wv][2][lane] = qd; }
        }
        __syncthreads();
        if (tid < NSQ * NVAL) {
            const int s = tid / NVAL, v = tid - s * NVAL;
            double t = s_sq[0][s][v];
            for (int w = 1; w < RANK_CI_WAVES; ++w) t += s_sq[w][s][v];
            part_sq[(o * NSQ + s) * NVAL + v] = t;
        }
    }
    const int r = tile * RANK_CI_REP_TILE + lane;
    if (r < n_rep) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = wv + RANK_CI_WAVES * q;
            if (c < NCOL) part_rep[(o * NCOL + c) * n_rep + r] = acc[q];
        }
        if (wv == 0) part_rep_cnt[o * n_rep + r] = cnt;
    }
}

// workgroup d: sum w by k_rank_final's tree over k_rank_sum's slices, the squares in slice order; out [n_stat, 5, n_k, n_seg] with the
// figures (stat 0, paired also 2) in place: var (1), paired also var_b (3), delta (4), var_delta (5)
__global__ void __launch_bounds__(RANK_SLICES) k_rank_ci_final(const double* __restrict__ part, const int64_t* __restrict__ counts,
                                                               const double* __restrict__ part_sq, int32_t n_k, int32_t n_seg,
                                                               int32_t n_sl, int32_t n_sl_all, int32_t paired, double* __restrict__ out) {
    __shared__ double s_v[RANK_SLICES];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int nval = RANK_FIGS * n_k, nsq = paired ? 3 : 1;
    s_v[tid] = part[((int64_t)d * RANK_SLICES + tid) * (nval + 1) + nval];
    __syncthreads();
    for (int off = RANK_SLICES / 2; off > 0; off >>= 1) {
        if (tid < off) s_v[tid] += s_v[tid + off];
        __syncthreads();
    }
    if (tid >= nsq * nval) return;
    const int s = tid / nval, v = tid - s * nval;
    const int64_t G = counts[d];
    const double den = s_v[0];
    const int64_t c0 = (int64_t)d * n_sl, c1 = c0 + (d < n_seg - 1 ? n_sl : n_sl_all);       // the segment's cells
    double sq = 0.0;
    for (int64_t c = c0; c < c1; ++c) sq += part_sq[(c * nsq + s) * nval + v];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double scale = G >= 2 ? (double)G / (double)(G - 1) / (den * den) : nan;
    out[((int64_t)(2 * s + 1) * nval + v) * n_seg + d] = G >= 2 ? scale * sq : nan;
    if (s == 2)                                                             // NaN - NaN when no group is counted
        out[((int64_t)4 * nval + v) * n_seg + d] = out[(int64_t)v * n_seg + d] - out[((int64_t)2 * nval + v) * n_seg + d];
}

// a thread per (segment, vector and value, replicate): reps [n_vec, n_rep, 5 n_k, n_seg], rep_counts [n_rep, n_seg]
__global__ void __launch_bounds__(GAUC_THREADS) k_rank_ci_rep_final(const double* __restrict__ part_rep,
                                                                    const int64_t* __restrict__ part_rep_cnt, int32_t n_k, int32_t n_vec,
                                                                    int32_t n_seg, int32_t n_sl, int32_t n_sl_all, int32_t n_rep,
                                                                    double* __restrict__ reps,
                                                                    int64_t* __restrict__ rep_counts) {
    const int nval = RANK_FIGS * n_k, ncv = n_vec * nval, ncol = ncv + 1;
    const int64_t id = (int64_t)blockIdx.x * GAUC_THREADS + threadIdx.x;
    const int64_t r = id % n_rep, c = (id / n_rep) % ncv, d = id / ((int64_t)n_rep * ncv);
    if (d >= n_seg) return;
    double num = 0.0, den = 0.0;
    int64_t cnt = 0;
    const int64_t c0 = d * n_sl, c1 = c0 + (d < n_seg - 1 ? n_sl : n_sl_all);                  // the segment's cells
    for (int64_t o = c0; o < c1; ++o) {
        num += part_rep[(o * ncol + c) * n_rep + r];
        den += part_rep[(o * ncol + ncv) * n_rep + r];
        cnt += part_rep_cnt[o * n_rep + r];
    }
    const int64_t vec = c / nval, v = c - vec * nval;
    reps[((vec * n_rep + r) * nval + v) * n_seg + d] = cnt > 0 ? num / den : __longlong_as_double(0x7ff8000000000000ll);
    if (c == 0 && rep_counts) rep_counts[r * n_seg + d] = cnt;
}

struct RankCiLayout {
    RankLayout r;                       // cdc_eval_rank's arrays; r.g.m.temp / r.g.m.total lie behind the ones below
    int64_t scan_b, part_b, part_cnt_b, counts_b, part_sq, part_rep, part_rep_cnt;
};
static void rank_ci_fixed_layout(int64_t n, int32_t n_domain, int32_t n_k, int32_t paired, int32_t n_rep, RankCiLayout* L) {
    const int64_t n2 = 2 * n, seg = (int64_t)n_domain + 1, nval = RANK_FIGS * n_k, ncol = (paired ? 2 : 1) * nval + 1;
    const int64_t cells = (int64_t)n_domain * rank_ci_slices(n_domain) + rank_ci_slices_all(n_domain);
    rank_fixed_layout(n, n_domain, n_k, &L->r);
    MetCursor c{L->r.g.m.temp};
    L->scan_b = c.take(paired ? n2 * (int64_t)sizeof(GaucScan) : 0);
    L->part_b = c.take(paired ? seg * RANK_SLICES * (nval + 1) * 8 : 0);
    L->part_cnt_b = c.take(paired ? seg * RANK_SLICES * 2 * 8 : 0);
    L->counts_b = c.take(paired ? seg * 2 * 8 : 0);
    L->part_sq = c.take(cells * (paired ? 3 : 1) * nval * 8);
    L->part_rep = c.take(cells * ncol * n_rep * 8);
    L->part_rep_cnt = c.take(cells * n_rep * 8);
    L->r.g.m.end_fixed(c);
}
static bool rank_ci_sizes_ok(int64_t n, int32_t n_domain, int64_t n_user, int32_t n_k, int32_t n_rep) {
    return gauc_sizes_ok(n, n_domain, n_user) && n_k >= 1 && n_k <= RANK_MAX_NK && n_rep >= 0 && n_rep <= BOOT_MAX_REP &&
           (int64_t)n_rep * ((int64_t)n_domain + 1) * n_k <= RANK_CI_MAX_CELLS;
}

extern "C" int64_t cdc_eval_rank_ci_workspace_bytes(int64_t n, int32_t n_domain, int64_t n_user, int32_t n_k, int32_t paired,
                                                    int32_t n_rep) {
    if (!rank_ci_sizes_ok(n, n_domain, n_user, n_k, n_rep)) return 0;
    RankCiLayout L;
    rank_ci_fixed_layout(n, n_domain, n_k, paired != 0, n_rep, &L);
    if (gauc_temp(n, "eval_rank_ci", &L.r.g.m) != 0) return -1;
    return L.r.g.m.total;
}

template <int NK>
static void rank_ci_pass_launch(bool paired, dim3 grid, hipStream_t st, const uint64_t* keys, const GaucScan* sc, const GaucScan* sc_b,
                                const int64_t* start, const double* user_weight, const int32_t* ks, const double* D, int64_t n_user,
                                int64_t n2, int32_t n_seg, int32_t n_sl, int32_t n_sl_all, int32_t n_rep, uint64_t seed, const double* out,
                                double* part_sq, double* part_rep, int64_t* part_rep_cnt) {
    if (paired)
        hipLaunchKernelGGL((k_rank_ci_pass<NK, true>), grid, dim3(GAUC_THREADS), 0, st, keys, sc, sc_b, start, user_weight, ks, D, n_user,
                           n2, n_seg, n_sl, n_sl_all, n_rep, seed, out, part_sq, part_rep, part_rep_cnt);
    else
        hipLaunchKernelGGL((k_rank_ci_pass<NK, false>), grid, dim3(GAUC_THREADS), 0, st, keys, sc, sc_b, start, user_weight, ks, D, n_user,
                           n2, n_seg, n_sl, n_sl_all, n_rep, seed, out, part_sq, part_rep, part_rep_cnt);
}

extern "C" int cdc_eval_rank_ci(const float* pred_a, const float* pred_b, const int16_t* label, const int32_t* user, int64_t ld_user,
                                int64_t n_user, const int32_t* domain, int64_t ld_domain, int32_t n_domain, const double* user_weight,
                                const int32_t* ks, int32_t n_k, const double* discounts, int64_t n, int32_t n_rep, uint64_t seed,
                                double* out, double* reps, int64_t* counts, int64_t* rep_counts, int32_t* err_flag, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    CDC_CHECK_ARG(pred_a && label && user && ks && discounts && out && counts && workspace, CDC_E_BADARG, "eval_rank_ci: null pointer");
    CDC_CHECK_ARG(n > 0 && n_domain > 0 && n_domain < (1 << 20) && n_user > 0 && ld_user >= 0 && ld_domain >= 0, CDC_E_BADARG,
                  "eval_rank_ci: bad sizes n=%ld n_domain=%d n_user=%ld", (long)n, n_domain, (long)n_user);
    CDC_CHECK_ARG(n_k >= 1 && n_k <= RANK_MAX_NK, CDC_E_BADARG, "eval_rank_ci: n_k=%d cut-offs, 1 to %d are served", n_k, RANK_MAX_NK);
    CDC_CHECK_ARG(n_rep >= 0 && n_rep <= BOOT_MAX_REP, CDC_E_BADARG, "eval_rank_ci: n_rep=%d outside [0, %d]", n_rep, BOOT_MAX_REP);
    CDC_CHECK_ARG(n_rep == 0 || reps, CDC_E_BADARG, "eval_rank_ci: n_rep=%d needs the replicate array", n_rep);
    CDC_CHECK_ARG(n_rep > 0 || !reps, CDC_E_BADARG, "eval_rank_ci: a replicate array without replicates");
    CDC_CHECK_ARG((int64_t)n_rep * ((int64_t)n_domain + 1) * n_k <= RANK_CI_MAX_CELLS, CDC_E_BADARG,
                  "eval_rank_ci: n_rep * (n_domain + 1) * n_k = %ld cells exceed %d", (long)((int64_t)n_rep * ((int64_t)n_domain + 1) * n_k),
                  RANK_CI_MAX_CELLS);
    MET_TRY(met_need_domain("eval_rank_ci", domain, n_domain));
    CDC_CHECK_ARG(n < (1ll << 31), CDC_E_TOOBIG, "eval_rank_ci: n=%ld exceeds the 2^31 rows a sorted position counts in 32 bits", (long)n);
    CDC_CHECK_ARG(gauc_sizes_ok(n, n_domain, n_user), CDC_E_BADARG,
                  "eval_rank_ci: (n_domain + 1) * n_user = %ld * %ld group ids exceed 2^32", (long)n_domain + 1, (long)n_user);
    const int32_t paired = pred_b != nullptr;
    RankCiLayout L;
    rank_ci_fixed_layout(n, n_domain, n_k, paired, n_rep, &L);
    MET_TRY(met_gate("eval_rank_ci", workspace, workspace_bytes, &L.r.g.m, [&] { return gauc_temp(n, "eval_rank_ci", &L.r.g.m); }));
    const MetWs ws{(char*)workspace};
    char* base = ws.base;
    const uint64_t* keys = ws.ptr<const uint64_t>(L.r.g.m.keys_out);
    const GaucScan* sc = ws.ptr<const GaucScan>(L.r.g.scan);
    const GaucScan* sc_b = ws.ptr<const GaucScan>(L.scan_b);
    const int64_t* start = ws.ptr<const int64_t>(L.r.g.m.start);
    double* part = ws.ptr<double>(L.r.part);
    int64_t* part_cnt = ws.ptr<int64_t>(L.r.part_cnt);
    double* part_b = ws.ptr<double>(L.part_b);
    int64_t* part_cnt_b = ws.ptr<int64_t>(L.part_cnt_b);
    int64_t* counts_b = ws.ptr<int64_t>(L.counts_b);
    double* part_sq = ws.ptr<double>(L.part_sq);
    double* part_rep = ws.ptr<double>(L.part_rep);
    int64_t* part_rep_cnt = ws.ptr<int64_t>(L.part_rep_cnt);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = 2 * n;
    const int seg = n_domain + 1, nval = RANK_FIGS * n_k, n_sl = rank_ci_slices(n_domain), n_sl_all = rank_ci_slices_all(n_domain);
    const int ntiles = n_rep > 0 ? (n_rep + RANK_CI_REP_TILE - 1) / RANK_CI_REP_TILE : 1;
    if (paired) {                                                   // the second vector first: of its order only the scan stays
        GaucLayout Lb = L.r.g;
        Lb.scan = L.scan_b;
        MET_TRY(gauc_order(pred_b, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, base, Lb, nullptr, "eval_rank_ci", st));
    }
    MET_TRY(gauc_order(pred_a, label, user, ld_user, n_user, domain, ld_domain, n_domain, n, err_flag, base, L.r.g, nullptr, "eval_rank_ci", st));
    for (int v = 0; v <= paired; ++v) {                             // the counts follow from the labels alone: the second set is dropped
        switch (n_k) {
#define RANK_CASE(NK) case NK: rank_sum_launch<NK>(seg, st, keys, v ? sc_b : sc, start, user_weight, ks, discounts, n_user, n2, \
                                                   v ? part_b : part, v ? part_cnt_b : part_cnt); break;
            RANK_CASE(1) RANK_CASE(2) RANK_CASE(3) RANK_CASE(4) RANK_CASE(5) RANK_CASE(6) RANK_CASE(7) RANK_CASE(8)
#undef RANK_CASE
        }
        CDC_LAUNCH_CHECK("eval_rank_ci(sum)");
        hipLaunchKernelGGL(k_rank_final, dim3(seg), dim3(RANK_SLICES), 0, st, (const double*)(v ? part_b : part),
                           (const int64_t*)(v ? part_cnt_b : part_cnt), n_k, seg, out + (int64_t)v * 2 * nval * seg, v ? counts_b : counts);
        CDC_LAUNCH_CHECK("eval_rank_ci(final)");
    }
    const dim3 grid(n_domain * n_sl + n_sl_all, ntiles);
    switch (n_k) {
#define RANK_CASE(NK) case NK: rank_ci_pass_launch<NK>(paired, grid, st, keys, sc, sc_b, start, user_weight, ks, discounts, n_user, n2, seg, \
                                                       n_sl, n_sl_all, n_rep, seed, (const double*)out, part_sq, part_rep, part_rep_cnt); break;
        RANK_CASE(1) RANK_CASE(2) RANK_CASE(3) RANK_CASE(4) RANK_CASE(5) RANK_CASE(6) RANK_CASE(7) RANK_CASE(8)
#undef RANK_CASE
    }
    CDC_LAUNCH_CHECK("eval_rank_ci(pass)");
    hipLaunchKernelGGL(k_rank_ci_final, dim3(seg), dim3(RANK_SLICES), 0, st, (const double*)part, (const int64_t*)counts,
                       (const double*)part_sq, n_k, seg, n_sl, n_sl_all, paired, out);
    CDC_LAUNCH_CHECK("eval_rank_ci(variances)");
    if (n_rep > 0) {
        const int64_t items = (int64_t)seg * (paired ? 2 : 1) * nval * n_rep;
        hipLaunchKernelGGL(k_rank_ci_rep_final, dim3((unsigned)cdc_ceil_div(items, GAUC_THREADS)), dim3(GAUC_THREADS), 0, st,
                           (const double*)part_rep, (const int64_t*)part_rep_cnt, n_k, paired ? 2 : 1, seg, n_sl, n_sl_all, n_rep, reps, rep_counts);
        CDC_LAUNCH_CHECK("eval_rank_ci(replicates)");
    }
    return 0;
}
