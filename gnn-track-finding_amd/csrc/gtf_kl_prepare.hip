// gtf_kl_prepare.hip -- the graph gtf_parabolic_kl reads, built on the GPU (include/gtf.h:
// gtf_kl_prepare, gtf_kl_coords, gtf_kl_pair_rows).
//
// gtf/parabolic.py ParabolicKL.__init__ with tile = 0 is the definition; every array written here
// is equal to the one it uploads, element for element. The steps, each a fixed number of launches:
//
//   cut       with is_edge: the flags' exclusive sum places every kept slot and, read at the
//             caller's slot_ptr, is the in-edge CSR (in_edge_csr). One launch checks the
//             caller's slot_ptr (starts at 0, does not decrease, ends at n_slots)
//   order     a node's key is its degree rank 0..9 (layout 1) or its bucket 0..4 (layout 0);
//             ONE stable 4-bit hipCUB radix pass over (key, node) is the stable argsort of the
//             rank, and in layout 0 leaves the four bucket lists, each ascending, one after
//             another. The ten run starts are lower bounds in the sorted keys
//   tables    degrees in the new order; two exclusive sums give slot_ptr (int32) and pair_ptr
//             (int64); one thread per node copies its slots (slot_of, slot_src through the
//             inverse order), checking each kept source against [0, N)
//   coords    one gather per node: x, y as [N, 2], the truth id, and for compact the fixed-point
//             pair. The scale comes from a two-launch maximum (per-block partials, then one
//             block that also applies quantise_xy's e += 1 step) and stays on the device: the
//             quantising launch reads it there and the host gets it with the counts
//   truth32   the 64-bit radix sort with the sign flipped ALWAYS runs; the kernel that writes the
//             ids reads a device flag (some id outside int32) and stores either the id or its
//             rank among the distinct ids (head flags, exclusive sum). One synchronisation.
//
// No atomic but the error word's, touched only on a violation. Vector stores only. Nothing is
// allocated. Every index read from device memory is checked against its array before it is used.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_search.h"

namespace {

using gtf::bad;
using gtf::bound;
using gtf::clampi;
using gtf::fail;
using gtf::flip;
using gtf::grid;
using gtf::unflip;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int32_t MAX_N = int32_t(1) << 30;
constexpr int MAX_PART = 1024;                    // blocks of the maximum's first launch
constexpr double Q_LIMIT = 1073741824.0;          // 2^30
enum { S_ERR = 0, S_WIDE, S_KEPT, S_WORDS = 4 };  // the words beside the counts

struct Ws {
    gtf_kl_counts* cnt;               // the counts record, as the host gets it
    int32_t* scal;                    // [S_WORDS] error word, "an id outside int32", kept slots
    int32_t *ef, *es;                 // [S + 1] is_edge as 0 / 1; its exclusive sum
    int32_t* kp;                      // [N + 1] the in-edge CSR's slot_ptr
    int32_t* ksrc;                    // [S] its slot_src
    uint32_t *key, *skey;             // [N] rank or bucket; sorted
    int32_t *val, *order;             // [N] node; sorted (layout 0: buf.list instead)
    int32_t* inv;                     // [N] the inverse order
    int32_t* dn;                      // [N + 1] degrees in the new order
    int64_t* pn;                      // [N + 1] pairs in the new order
    double* part;                     // [MAX_PART] partial maxima
    uint64_t *tk, *tks;               // [N] truth ids, sign flipped; sorted
    int32_t *tv, *tvs;                // [N] their nodes; sorted
    int32_t *th, *te;                 // [N + 1] head flags; their exclusive sum
    gtf::Scratch cub;
    size_t total;
};

Ws carve(void* base, int64_t N, int64_t S) {
    Ws w = {};
    gtf::Arena a(base);
    const size_t n = (size_t)N, n1 = n + 1, s = (size_t)S, s1 = s + 1;
    w.cnt = a.take<gtf_kl_counts>(1);
    w.scal = a.take<int32_t>(S_WORDS);
    w.ef = a.take<int32_t>(s1);
    w.es = a.take<int32_t>(s1);
    w.kp = a.take<int32_t>(n1);
    w.ksrc = a.take<int32_t>(s);
    w.key = a.take<uint32_t>(n);
    w.skey = a.take<uint32_t>(n);
    w.val = a.take<int32_t>(n);
    w.order = a.take<int32_t>(n);
    w.inv = a.take<int32_t>(n);
    w.dn = a.take<int32_t>(n1);
    w.pn = a.take<int64_t>(n1);
    w.part = a.take<double>(MAX_PART);
    w.tk = a.take<uint64_t>(n);
    w.tks = a.take<uint64_t>(n);
    w.tv = a.take<int32_t>(n);
    w.tvs = a.take<int32_t>(n);
    w.th = a.take<int32_t>(n1);
    w.te = a.take<int32_t>(n1);
    const int big = (int)(N > S ? N : S) + 1;
    w.cub = gtf::CubNeed().scan<int32_t>(big).scan<int64_t>((int)N + 1).sort_pairs<uint32_t, int32_t>((int)N)
                .sort_pairs<uint64_t, int32_t>((int)N).take(a);
    w.total = a.used();
    return w;
}

struct Prep {
    int32_t N, S;
    int32_t layout, with_single, compact, stride, has_edge, has_truth;
    const int32_t* ptr;       // the caller's
    const int32_t* src;
    const uint8_t* ise;
    const double* gnn;
    const int64_t* truth;
    const int32_t* kp;        // the in-edge CSR: the caller's, or the workspace's after the cut
    const int32_t* ksrc;
    int32_t* order;           // the sorted nodes: w.order, or buf.list
    gtf_kl_prepare_buf o;
    Ws w;
};

__device__ __forceinline__ void flag(int32_t* scal, uint32_t bit) { atomicOr((uint32_t*)scal + S_ERR, bit); }

// the first true key of [d == 1 if with_single] + [d == q for q in 2..8] + [d > 8]; 9: unlisted
__device__ __forceinline__ uint32_t rank_of(int d, int with_single) {
    if (d <= 0) return 9;
    if (d == 1) return with_single ? 0 : 9;
    return d > 8 ? 8 : (uint32_t)(d - 1);
}
// the list of BUCKETS = (1, 2), (3, 4), (5, 8), (9, ..) with lo = 1 if with_single else 2; 4: none
__device__ __forceinline__ uint32_t bucket_of(int d, int with_single) {
    if (d <= 0) return 4;
    if (d == 1) return with_single ? 0 : 4;
    return d <= 2 ? 0 : d <= 4 ? 1 : d <= 8 ? 2 : 3;
}
__device__ __forceinline__ int degree(const int32_t* kp, int v) {
    const int d = kp[v + 1] - kp[v];
    return d > 0 ? d : 0;
}
__device__ __forceinline__ int64_t pairs_of(int d) { return d >= 2 ? (int64_t)d * (d - 1) / 2 : 0; }

// ---- cut ----
__global__ __launch_bounds__(BLOCK) void k_edge_flags(Prep a) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s > a.S) return;
    a.w.ef[s] = s < a.S && a.ise[s] != 0;
}

// the caller's slot_ptr checked; with is_edge the kept slots before each node
__global__ __launch_bounds__(BLOCK) void k_cut_ptr(Prep a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v > a.N) return;
    const int p = a.ptr[v];
    bool ok = p >= 0 && p <= a.S;
    if (v == 0) ok = ok && p == 0;
    if (v < a.N) ok = ok && a.ptr[v + 1] >= p;
    else ok = ok && p == a.S;
    if (!ok) flag(a.w.scal, GTF_KL_ERR_SLOT_PTR);
    if (a.has_edge) a.w.kp[v] = a.w.es[clampi(p, 0, a.S)];
    if (v == a.N) a.w.scal[S_KEPT] = a.has_edge ? a.w.es[a.S] : a.S;
}

__global__ __launch_bounds__(BLOCK) void k_cut_src(Prep a) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= a.S || !a.w.ef[s]) return;
    a.w.ksrc[a.w.es[s]] = a.src[s];   // (es[s] < S: a sum of s flags)
}

// ---- order ----
__global__ __launch_bounds__(BLOCK) void k_keys(Prep a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= a.N) return;
    const int d = degree(a.kp, v);
    a.w.key[v] = a.layout ? rank_of(d, a.with_single) : bucket_of(d, a.with_single);
    a.w.val[v] = v;
}

// degrees and pairs in the new order; layout 1: node_of and the inverse order
__global__ __launch_bounds__(BLOCK) void k_order(Prep a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > a.N) return;
    int d = 0;
    if (i < a.N) {
        int o = i;
        if (a.layout) {
            o = a.order[i];   // (a permutation of [0, N): the sorted values)
            a.o.node_of[i] = o;
            a.w.inv[o] = i;
        }
        d = degree(a.kp, o);
    }
    a.w.dn[i] = d;
    a.w.pn[i] = pairs_of(d);
}

// ---- tables: one thread per node copies its slots ----
__global__ __launch_bounds__(BLOCK) void k_slots(Prep a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int o = a.layout ? a.order[i] : i;
    const int b = a.o.slot_ptr[i], b0 = a.kp[o], d = a.w.dn[i];
    for (int k = 0; k < d; k++) {
        const int s = b + k, s0 = b0 + k;
        if (s < 0 || s >= a.S || s0 < 0 || s0 >= a.S) break;   // (a broken slot_ptr: flagged by k_cut_ptr)
        const int x = a.ksrc[s0];
        const bool ok = x >= 0 && x < a.N;
        if (!ok) flag(a.w.scal, GTF_KL_ERR_SOURCE);
        a.o.slot_src[s] = !ok ? -1 : a.layout ? a.w.inv[x] : x;
        if (a.layout) a.o.slot_of[s] = s0;
    }
}

// ---- coords ----
// per-block maxima of |x|, |y| over the finite coordinates; a non-finite one is flagged
__global__ __launch_bounds__(BLOCK) void k_absmax(const double* gnn, int stride, int N, double* part, int32_t* scal) {
    __shared__ double red[BLOCK];
    double m = 0.0;
    bool nonfinite = false;
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < N; v += (int64_t)gridDim.x * BLOCK) {
        const double x = fabs(gnn[v * stride]), y = fabs(gnn[v * stride + 1]);
        if (isfinite(x) && isfinite(y)) m = fmax(m, fmax(x, y));
        else nonfinite = true;
    }
    if (nonfinite) flag(scal, GTF_KL_ERR_NONFINITE);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// the maximum and quantise_xy's scale (parabolic.py:51-59); one block
__global__ __launch_bounds__(BLOCK) void k_scale(const double* part, int n_part, double scale_in, gtf_kl_counts* cnt,
                                                 int32_t* scal) {
    __shared__ double red[BLOCK];
    double m = 0.0;
    for (int b = threadIdx.x; b < n_part; b += BLOCK) m = fmax(m, part[b]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    m = red[0];
    double scale = scale_in;
    if (scale_in == 0.0) {
        int e = 0;
        if (m > 0.0) {
            (void)frexp(m, &e);   // m = f * 2^e with 0.5 <= f < 1
            if (rint(ldexp(m, 30 - e)) >= Q_LIMIT) e += 1;   // (within half a step of 2^e)
        }
        scale = ldexp(1.0, e - 30);
    }
    if (!(isfinite(scale) && scale > 0.0)) flag(scal, GTF_KL_ERR_SCALE);
    cnt->scale = scale;
    cnt->max_abs = m;
}

// One node per thread: x, y as a compact row, the truth id, the fixed-point pair. o = node_of[i]
// or i. scale_dev, where given, is the scale to use (gtf_kl_prepare's derived one).
__global__ __launch_bounds__(BLOCK) void k_coords(const double* gnn, int stride, int N, const int64_t* node_of, double* xy,
                                                  int32_t* q, const double* scale_dev, double scale_val,
                                                  const int64_t* truth, int64_t* truth_out, uint32_t* err) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    int64_t o = node_of ? node_of[i] : i;
    if (o < 0 || o >= N) {
        atomicOr(err, GTF_KL_ERR_NODE_OF);
        o = 0;
    }
    const double x = gnn[o * stride], y = gnn[o * stride + 1];
    if (xy) *(double2*)(xy + 2 * (size_t)i) = make_double2(x, y);
    if (truth_out) truth_out[i] = truth[o];
    if (!q) return;
    const double scale = scale_dev ? *scale_dev : scale_val;
    int2 r = make_int2(0, 0);
    if (!(isfinite(x) && isfinite(y))) atomicOr(err, GTF_KL_ERR_NONFINITE);
    else if (scale > 0.0) {   // (no scale: flagged by k_scale or refused by the host)
        const double qx = rint(x / scale), qy = rint(y / scale);
        if (fabs(qx) >= Q_LIMIT || fabs(qy) >= Q_LIMIT) atomicOr(err, GTF_KL_ERR_FIT);
        else r = make_int2((int)qx, (int)qy);
    }
    *(int2*)(q + 2 * (size_t)i) = r;
}

// ---- truth32 ----
__global__ __launch_bounds__(BLOCK) void k_truth_keys(Prep a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int64_t id = a.truth[a.layout ? a.order[i] : i];
    a.w.tk[i] = flip(id);
    a.w.tv[i] = i;
    if (id < -(int64_t(1) << 31) || id >= (int64_t(1) << 31)) a.w.scal[S_WIDE] = 1;   // (every writer stores 1)
}

__global__ __launch_bounds__(BLOCK) void k_truth_heads(Prep a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p > a.N) return;
    a.w.th[p] = p < a.N && (p == 0 || a.w.tks[p] != a.w.tks[p - 1]);
}

// the id itself, or np.unique's inverse: the run of equal ids the element lies in
__global__ __launch_bounds__(BLOCK) void k_truth_write(Prep a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.N) return;
    const int32_t lab = a.w.te[p] + a.w.th[p] - 1;
    a.o.truth32[a.w.tvs[p]] = a.w.scal[S_WIDE] ? lab : (int32_t)unflip(a.w.tks[p]);   // (tvs: a permutation of [0, N))
}

// ---- counts: the run starts of the ten (five) keys; one block ----
__global__ __launch_bounds__(64) void k_counts(Prep a) {
    __shared__ int32_t start[11];
    if (threadIdx.x < 11) start[threadIdx.x] = bound<false>(a.w.skey, a.N, (uint32_t)threadIdx.x);
    __syncthreads();
    if (threadIdx.x != 0) return;
    gtf_kl_counts* c = a.w.cnt;
    c->n_kept = a.w.scal[S_KEPT];
    c->n_pairs = a.o.pair_ptr[a.N];
    int32_t r[10];
    for (int q = 0; q < 10; q++) r[q] = start[q + 1] - start[q];
    if (a.layout) {
        c->n_listed = start[9];
        c->n_d1 = r[0];
        c->count[0] = r[0] + r[1];
        c->count[1] = r[2] + r[3];
        c->count[2] = r[4] + r[5] + r[6] + r[7];
        c->count[3] = r[8];
        int32_t f = 0;
        for (int q = 0; q < 4; q++) {
            c->first[q] = f;
            f += c->count[q];
        }
        for (int q = 0; q < 6; q++) c->n_deg[q] = r[2 + q];
    } else {
        c->n_listed = start[4];
        for (int q = 0; q < 4; q++) c->count[q] = r[q];
    }
}

// ---- pair rows ----
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_pair_rows(const int64_t* pair_ptr, int N, int64_t P, const int64_t* node_of,
                                                     const T* emp, int64_t* node, int64_t* pi, int64_t* pj, T* emp_row) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const int v = gtf::segment_of(pair_ptr, N, p);
    int64_t t = p - pair_ptr[v];
    if (t < 0) t = 0;   // (a pair_ptr that does not cover p)
    // the triangular root: the i with i (i - 1) / 2 <= t < (i + 1) i / 2, from the fp64 estimate
    int64_t i = (int64_t)floor((1.0 + sqrt(1.0 + 8.0 * (double)t)) / 2.0);
    while (i > 1 && i * (i - 1) / 2 > t) i--;
    while ((i + 1) * i / 2 <= t) i++;
    node[p] = node_of ? node_of[v] : v;
    pi[p] = i;
    pj[p] = t - i * (i - 1) / 2;
    if (emp_row) emp_row[p] = emp[v];
}

const char* error_text(uint32_t err) {
    if (err & GTF_KL_ERR_SLOT_PTR) return "slot_ptr does not start at 0, decreases or does not end at n_slots";
    if (err & GTF_KL_ERR_SOURCE) return "a kept slot's source outside [0, n_nodes)";
    if (err & GTF_KL_ERR_NODE_OF) return "a node_of entry outside [0, n_nodes)";
    if (err & GTF_KL_ERR_NONFINITE) return "non-finite coordinate";
    if (err & GTF_KL_ERR_SCALE) return "scale must be finite and > 0";
    if (err & GTF_KL_ERR_FIT) return "max |x|, |y| does not fit scale (|q| < 2^30)";
    return "unknown error bit";
}

}  // namespace

extern "C" {

size_t gtf_kl_prepare_workspace_bytes(int32_t n_nodes, int32_t n_slots) {
    const int64_t N = n_nodes > 0 ? (n_nodes < MAX_N ? n_nodes : MAX_N) : 0;
    const int64_t S = n_slots > 0 ? (n_slots < MAX_N ? n_slots : MAX_N) : 0;
    return carve(nullptr, N, S).total;
}

int gtf_kl_prepare(const gtf_kl_prepare_in* in, const gtf_kl_prepare_buf* buf, gtf_kl_graph* out, gtf_kl_q32* q32,
                   gtf_kl_counts* counts, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_kl_prepare";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_kl_prepare_in", "gtf_kl_prepare_in")) return rc;
    if (!buf || !out || !counts) return bad("gtf_kl_prepare: null buf, out or counts");
    const int32_t N = in->n_nodes, S = in->n_slots;
    if (N < 0 || S < 0) return bad("gtf_kl_prepare: negative sizes");
    if (N > MAX_N || S > MAX_N) return bad("gtf_kl_prepare: more than 2^30 nodes or slots");
    if (in->gnn_stride != 2 && in->gnn_stride != 4) return bad("gtf_kl_prepare: gnn_stride must be 2 or 4");
    if (in->layout != 0 && in->layout != 1) return bad("gtf_kl_prepare: layout must be 0 (natural) or 1 (ordered)");
    if (in->compact && !(isfinite(in->scale) && in->scale >= 0.0))
        return bad("gtf_kl_prepare: scale must be finite and > 0 (0: derived)");
    if (in->compact && !q32) return bad("gtf_kl_prepare: compact needs a gtf_kl_q32");
    const bool has_truth = in->truth != nullptr;
    const char* miss = !in->slot_ptr                                                ? "in.slot_ptr"
                       : S > 0 && !in->slot_src                                     ? "in.slot_src"
                       : N > 0 && !in->gnn                                          ? "in.gnn"
                       : !buf->slot_ptr || !buf->pair_ptr                           ? "buf.slot_ptr / pair_ptr"
                       : S > 0 && !buf->slot_src                                    ? "buf.slot_src"
                       : N > 0 && !buf->xy                                          ? "buf.xy"
                       : N > 0 && has_truth && !buf->truth                          ? "buf.truth"
                       : N > 0 && !in->layout && !buf->list                         ? "buf.list"
                       : N > 0 && in->layout && !buf->node_of                       ? "buf.node_of"
                       : S > 0 && in->layout && !buf->slot_of                       ? "buf.slot_of"
                       : N > 0 && in->compact && !buf->q                            ? "buf.q"
                       : N > 0 && in->compact && has_truth && !buf->truth32         ? "buf.truth32"
                                                                                    : nullptr;
    if (miss) {
        snprintf(m, sizeof(m), "gtf_kl_prepare: missing array: %s", miss);
        return bad(m);
    }
    if (N > 0 && (!workspace || workspace_bytes < gtf_kl_prepare_workspace_bytes(N, S)))
        return bad("gtf_kl_prepare: workspace smaller than gtf_kl_prepare_workspace_bytes");
    *counts = gtf_kl_counts{};
    *out = gtf_kl_graph{};
    out->n_nodes = N;
    out->slot_ptr = buf->slot_ptr; out->slot_src = buf->slot_src; out->gnn = buf->xy;
    out->truth = has_truth ? buf->truth : nullptr;
    out->pair_ptr = buf->pair_ptr;
    out->gnn_stride = 2;
    out->deg_runs = in->layout;
    if (q32) *q32 = gtf_kl_q32{};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (N == 0) {   // (two stream-ordered fills; nothing to bring back)
        if (S != 0) return bad("gtf_kl_prepare: slots without nodes");
        if ((e = hipMemsetAsync(buf->slot_ptr, 0, 4, st)) != hipSuccess ||
            (e = hipMemsetAsync(buf->pair_ptr, 0, 8, st)) != hipSuccess)
            return fail(who, "memset", e);
        if (in->compact) {
            counts->scale = in->scale > 0.0 ? in->scale : ldexp(1.0, -30);
            q32->xy = buf->q; q32->scale = counts->scale; q32->truth32 = has_truth ? buf->truth32 : nullptr;
        }
        return 0;
    }
    Prep a = {};
    a.N = N; a.S = S;
    a.layout = in->layout; a.with_single = in->with_single != 0; a.compact = in->compact != 0;
    a.stride = in->gnn_stride; a.has_edge = in->is_edge != nullptr && S > 0; a.has_truth = has_truth;
    a.ptr = in->slot_ptr; a.src = in->slot_src; a.ise = in->is_edge; a.gnn = in->gnn; a.truth = in->truth;
    a.o = *buf;
    a.w = carve(workspace, N, S);
    const Ws& w = a.w;
    a.kp = a.has_edge ? w.kp : in->slot_ptr;
    a.ksrc = a.has_edge ? w.ksrc : in->slot_src;
    a.order = in->layout ? w.order : buf->list;
    const gtf::Cub cub{w.cub, st};
    const dim3 gn(grid(N)), gn1(grid((int64_t)N + 1)), bl(BLOCK);
    static_assert(sizeof(gtf_kl_counts) % 4 == 0, "cleared as words");
    if ((e = hipMemsetAsync(w.cnt, 0, sizeof(gtf_kl_counts), st)) != hipSuccess ||
        (e = hipMemsetAsync(w.scal, 0, 4 * S_WORDS, st)) != hipSuccess)
        return fail(who, "memset", e);
    // cut
    if (a.has_edge) {
        hipLaunchKernelGGL(k_edge_flags, dim3(grid((int64_t)S + 1)), bl, 0, st, a);
        if ((e = cub.scan(w.ef, w.es, S + 1)) != hipSuccess) return fail(who, "scan is_edge", e);
    }
    hipLaunchKernelGGL(k_cut_ptr, gn1, bl, 0, st, a);
    if (a.has_edge) hipLaunchKernelGGL(k_cut_src, dim3(grid(S)), bl, 0, st, a);
    // order
    hipLaunchKernelGGL(k_keys, gn, bl, 0, st, a);
    if ((e = cub.sort_pairs(w.key, w.skey, w.val, a.order, N, 4)) != hipSuccess) return fail(who, "sort ranks", e);
    hipLaunchKernelGGL(k_order, gn1, bl, 0, st, a);
    // tables
    if ((e = cub.scan(w.dn, buf->slot_ptr, N + 1)) != hipSuccess) return fail(who, "scan degrees", e);
    if ((e = cub.scan(w.pn, buf->pair_ptr, N + 1)) != hipSuccess) return fail(who, "scan pairs", e);
    if (S > 0) hipLaunchKernelGGL(k_slots, gn, bl, 0, st, a);
    // coords
    if (a.compact) {
        const int n_part = grid(N) < MAX_PART ? grid(N) : MAX_PART;
        hipLaunchKernelGGL(k_absmax, dim3(n_part), bl, 0, st, in->gnn, a.stride, N, w.part, w.scal);
        hipLaunchKernelGGL(k_scale, dim3(1), bl, 0, st, w.part, n_part, in->scale, w.cnt, w.scal);
    }
    hipLaunchKernelGGL(k_coords, gn, bl, 0, st, in->gnn, a.stride, N, in->layout ? buf->node_of : nullptr, buf->xy,
                       a.compact ? buf->q : nullptr, &w.cnt->scale, 0.0, in->truth, has_truth ? buf->truth : nullptr,
                       (uint32_t*)w.scal + S_ERR);
    // truth32
    if (a.compact && has_truth) {
        hipLaunchKernelGGL(k_truth_keys, gn, bl, 0, st, a);
        if ((e = cub.sort_pairs(w.tk, w.tks, w.tv, w.tvs, N)) != hipSuccess) return fail(who, "sort truth", e);
        hipLaunchKernelGGL(k_truth_heads, gn1, bl, 0, st, a);
        if ((e = cub.scan(w.th, w.te, N + 1)) != hipSuccess) return fail(who, "scan truth", e);
        hipLaunchKernelGGL(k_truth_write, gn, bl, 0, st, a);
    }
    hipLaunchKernelGGL(k_counts, dim3(1), dim3(64), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t scal[S_WORDS] = {0, 0, 0, 0};
    if ((e = hipMemcpyAsync(counts, w.cnt, sizeof(gtf_kl_counts), hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(scal, w.scal, sizeof(scal), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    counts->error = (uint32_t)scal[S_ERR];
    if (counts->error) {
        snprintf(m, sizeof(m), "gtf_kl_prepare: %s", error_text(counts->error));
        return bad(m);
    }
    if (counts->n_kept < 0 || counts->n_kept > S || counts->n_listed < 0 || counts->n_listed > N || counts->n_pairs < 0)
        return bad("gtf_kl_prepare: inconsistent counts");
    out->n_slots = counts->n_kept;
    int32_t at = 0;
    for (int q = 0; q < 4; q++) {
        out->count[q] = counts->count[q];
        out->first[q] = counts->first[q];
        if (!in->layout) {   // the four lists lie one after another in buf.list
            out->list[q] = counts->count[q] > 0 ? buf->list + at : nullptr;
            at += counts->count[q];
        }
    }
    out->n_d1 = counts->n_d1;
    for (int q = 0; q < 6; q++) out->n_deg[q] = counts->n_deg[q];
    if (in->compact) {
        q32->xy = buf->q;
        q32->scale = counts->scale;
        q32->truth32 = has_truth ? buf->truth32 : nullptr;
    }
    return 0;
}

int gtf_kl_coords(int32_t n_nodes, const double* gnn, int32_t gnn_stride, const int64_t* node_of, double* xy, int32_t* q,
                  double scale, uint32_t* err, gtf_stream_t stream) {
    if (n_nodes < 0) return bad("gtf_kl_coords: negative sizes");
    if (gnn_stride != 2 && gnn_stride != 4) return bad("gtf_kl_coords: gnn_stride must be 2 or 4");
    if (!xy && !q) return bad("gtf_kl_coords: neither xy nor q");
    if (!err) return bad("gtf_kl_coords: null err");
    if (q && !(isfinite(scale) && scale > 0.0)) return bad("gtf_kl_coords: scale must be finite and > 0");
    if (n_nodes == 0) return 0;
    if (!gnn) return bad("gtf_kl_coords: null gnn");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_coords, dim3(grid(n_nodes)), dim3(BLOCK), 0, st, gnn, gnn_stride, n_nodes, node_of, xy, q,
                       (const double*)nullptr, scale, (const int64_t*)nullptr, (int64_t*)nullptr, err);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("gtf_kl_coords", "launch", e);
    return 0;
}

int gtf_kl_pair_rows(const gtf_kl_graph* g, int64_t n_pairs, const int64_t* node_of, const void* emp_var, int32_t dtype,
                     int64_t* node, int64_t* i, int64_t* j, void* emp_row, gtf_stream_t stream) {
    if (!g) return bad("gtf_kl_pair_rows: null graph");
    if (g->n_nodes < 0 || n_pairs < 0) return bad("gtf_kl_pair_rows: negative sizes");
    if (dtype != GTF_F64 && dtype != GTF_F32) return bad("gtf_kl_pair_rows: dtype must be GTF_F64 or GTF_F32");
    if ((emp_var == nullptr) != (emp_row == nullptr)) return bad("gtf_kl_pair_rows: emp_var and emp_row go together");
    if (n_pairs == 0) return 0;
    if (g->n_nodes == 0) return bad("gtf_kl_pair_rows: pairs without nodes");
    if (!g->pair_ptr || !g->slot_ptr || !node || !i || !j) return bad("gtf_kl_pair_rows: null pair_ptr, slot_ptr, node, i or j");
    hipStream_t st = (hipStream_t)stream;
    const dim3 gr((unsigned)((n_pairs + BLOCK - 1) / BLOCK)), bl(BLOCK);
    if (dtype == GTF_F64)
        hipLaunchKernelGGL(k_pair_rows<double>, gr, bl, 0, st, g->pair_ptr, g->n_nodes, n_pairs, node_of,
                           (const double*)emp_var, node, i, j, (double*)emp_row);
    else
        hipLaunchKernelGGL(k_pair_rows<float>, gr, bl, 0, st, g->pair_ptr, g->n_nodes, n_pairs, node_of,
                           (const float*)emp_var, node, i, j, (float*)emp_row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("gtf_kl_pair_rows", "launch", e);
    return 0;
}

}  // extern "C"
