// gtf_truth.hip -- the scorer's static truth tables on the GPU (include/gtf.h: gtf_truth_build):
// gtf/metrics.py truth_tables (src/extract/reconstruction_efficiency.py:41-91 the reference
// tracks, utilities/helper.py:466-479 hit_dissociation) from the parsed columns of the hit
// mapping, the truth file and the particles file, as device arrays; the six arrays it writes
// are array_equal to the host function's.
//
// Every id (node, hit, particle) is an arbitrary int64: it is sorted as its bits with the sign
// flipped (an unsigned order that is the signed one), by hipCUB radix sorts, which are stable.
//
//   high pT   1. particles sorted by id with the flag sqrt(px*px + py*py) >= pt_cut as value;
//                the exclusive sum of the sorted flags: "is this id one of the high-pT ones"
//                (np.isin) = a lower and an upper bound and a difference of two sums, whatever
//                the table repeats
//             2. per truth row that test on its particle; truth rows sorted by hit id, the row
//                index as value (stable: a hit's rows in row order); the sum of the flags again
//   rows      3. per mapping row: the run of its hit among the sorted truth rows. Empty: the
//                host's ValueError (GTF_TRUTH_ERR_MISSING). Its first element is the truth row
//                helper.py looks up (row_part); a flagged row anywhere in the run selects the
//                hit (isin over hits, not over rows), with the volume window: sel
//   region    4. rows sorted by ((not sel) << 63 | volume << 42 | layer << 21 | module) and then,
//                stably, by particle: a particle's selected rows come first in its run, in
//                (volume, layer, module) order, so a selected row's predecessor in the same run is
//                selected too. One launch marks particle heads, (volume, layer) heads and repeated
//                full keys; two exclusive sums of the packed marks place R and give each particle
//                its row count, its distinct (volume, layer) and its repeats as differences
//                between its head and the next one (particles without a selected row in between
//                add nothing)
//   CSR       5. rows sorted by node (row order inside a node), then that order sorted stably by
//                hit: (hit, node, row). The first of each (hit, node) run is the pair's first
//                row; the flag goes back to the node order, where an exclusive sum of (kept |
//                node head << 32) places P and T. A node's first row is always kept, so node
//                heads are kept rows
//
// No atomic but the error word's, which is touched only when the input is broken. Vector stores
// only. One synchronisation, for the four counts and the error word.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_host.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int32_t MAX_ROWS = 1 << 30;
constexpr uint64_t SIGN = uint64_t(1) << 63;
constexpr int ID_BITS = 21;                       // volume, layer, module: [0, 2^21)
constexpr int64_t ID_LIMIT = int64_t(1) << ID_BITS;
enum { S_T = 0, S_P, S_R, S_REF, S_ERR, S_WORDS };

struct Ws {
    int32_t* scal;                    // [S_WORDS]
    uint64_t *ka, *kb, *kc;           // [M + 1] sort keys
    int32_t *va, *vb, *vc;            // [M + 1] sort values
    uint64_t* pk;                     // [NP + 1] particle ids, sorted
    int32_t *pf, *ps;                 // [NP + 1] their high-pT flags; the exclusive sum
    uint64_t* tk;                     // [NT + 1] truth hit ids, sorted
    int32_t *tidx, *tflag, *tfs, *ts; // [NT + 1] the truth row; its flag by row; sorted; summed
    int64_t* row_part;                // [N] the particle of the row's hit (its first truth row)
    uint8_t* sel;                     // [N] region row
    int64_t *in_a, *in_b, *sum_a, *sum_b;   // [N + 1] packed marks and their exclusive sums
    int32_t *pos, *ref;               // [N + 1] position of particle r's head; its reference flag
    gtf::Scratch cub;
    size_t total;
};

Ws carve(void* base, int64_t N, int64_t NT, int64_t NP) {
    Ws w;
    gtf::Arena a(base);
    const size_t m = (size_t)(N > NT ? (N > NP ? N : NP) : (NT > NP ? NT : NP)) + 1;
    const size_t n = (size_t)N, n1 = n + 1, t1 = (size_t)NT + 1, p1 = (size_t)NP + 1;
    w.scal = a.take<int32_t>(16);
    w.ka = a.take<uint64_t>(m);
    w.kb = a.take<uint64_t>(m);
    w.kc = a.take<uint64_t>(m);
    w.va = a.take<int32_t>(m);
    w.vb = a.take<int32_t>(m);
    w.vc = a.take<int32_t>(m);
    w.pk = a.take<uint64_t>(p1);
    w.pf = a.take<int32_t>(p1);
    w.ps = a.take<int32_t>(p1);
    w.tk = a.take<uint64_t>(t1);
    w.tidx = a.take<int32_t>(t1);
    w.tflag = a.take<int32_t>(t1);
    w.tfs = a.take<int32_t>(t1);
    w.ts = a.take<int32_t>(t1);
    w.row_part = a.take<int64_t>(n);
    w.sel = a.take<uint8_t>(n);
    w.in_a = a.take<int64_t>(n1);
    w.in_b = a.take<int64_t>(n1);
    w.sum_a = a.take<int64_t>(n1);
    w.sum_b = a.take<int64_t>(n1);
    w.pos = a.take<int32_t>(n1);
    w.ref = a.take<int32_t>(n1);
    const int mi = (int)m;
    w.cub = gtf::CubNeed().sort_pairs<uint64_t, int32_t>(mi).scan<int64_t>(mi).scan<int32_t>(mi).sum<int32_t>(mi).take(a);
    w.total = a.used();
    return w;
}

struct Build {
    int32_t N, NT, NP, num_layers, min_volume, max_volume;
    double pt_cut;
    const int64_t *node, *hit, *pid, *vol, *lay, *mod;
    const int64_t *th, *tp;           // the truth columns (the mapping's own hit / pid when none are given)
    const int64_t* part_id;
    const double *px, *py;
    gtf_truth_buf o;
    Ws w;
};

__device__ __forceinline__ uint64_t flip(int64_t x) { return (uint64_t)x ^ SIGN; }
__device__ __forceinline__ int32_t lo32(int64_t x) { return (int32_t)(uint32_t)x; }
__device__ __forceinline__ int32_t hi32(int64_t x) { return (int32_t)((uint64_t)x >> 32); }

// first index in [0, n) with k[i] >= key (upper = false) or k[i] > key (upper = true)
template <bool upper>
__device__ __forceinline__ int bound(const uint64_t* k, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (upper ? k[mid] <= key : k[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- 1. the particles: id and high-pT flag (reconstruction_efficiency.py:44-47) ----
__global__ __launch_bounds__(BLOCK) void k_particles(Build a) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= a.NP) return;
    const double x = a.px[j], y = a.py[j];
    // np.sqrt(px ** 2 + py ** 2): two rounded products, a rounded sum (-ffp-contract=off), the
    // correctly rounded root
    const double pt = __dsqrt_rn(x * x + y * y);
    a.w.ka[j] = flip(a.part_id[j]);
    a.w.va[j] = pt >= a.pt_cut ? 1 : 0;
}

// ---- 2. the truth rows: is the row's particle a high-pT one; the keys of the sort by hit ----
__global__ __launch_bounds__(BLOCK) void k_truth_rows(Build a) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= a.NT) return;
    const uint64_t id = flip(a.tp[j]);
    const int lb = bound<false>(a.w.pk, a.NP, id), ub = bound<true>(a.w.pk, a.NP, id);
    a.w.tflag[j] = ub > lb && a.w.ps[ub] - a.w.ps[lb] > 0;
    a.w.ka[j] = flip(a.th[j]);
    a.w.va[j] = j;
}

__global__ __launch_bounds__(BLOCK) void k_truth_sorted(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.NT) return;
    const int j = a.w.tidx[i];
    a.w.tfs[i] = j >= 0 && j < a.NT ? a.w.tflag[j] : 0;
}

__device__ __forceinline__ uint64_t pack(int64_t v, int64_t l, int64_t m) {
    const uint64_t mask = (uint64_t)ID_LIMIT - 1;
    return (((uint64_t)v & mask) << (2 * ID_BITS)) | (((uint64_t)l & mask) << ID_BITS) | ((uint64_t)m & mask);
}

// ---- 3. the mapping rows ----
__global__ __launch_bounds__(BLOCK) void k_rows(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const uint64_t h = flip(a.hit[i]);
    const int lb = bound<false>(a.w.tk, a.NT, h), ub = bound<true>(a.w.tk, a.NT, h);
    const bool found = ub > lb;
    int64_t part = 0;
    if (found) {
        const int j = a.w.tidx[lb];
        if (j >= 0 && j < a.NT) part = a.tp[j];
    } else {
        atomicOr((uint32_t*)&a.w.scal[S_ERR], GTF_TRUTH_ERR_MISSING);   // (only on a violation)
    }
    const int64_t v = a.vol[i], l = a.lay[i], m = a.mod[i];
    const bool in_range = v >= 0 && v < ID_LIMIT && l >= 0 && l < ID_LIMIT && m >= 0 && m < ID_LIMIT;
    if (!in_range) atomicOr((uint32_t*)&a.w.scal[S_ERR], GTF_TRUTH_ERR_RANGE);
    const bool sel = found && in_range && a.w.ts[ub] - a.w.ts[lb] > 0 && v >= a.min_volume && v <= a.max_volume;
    a.w.row_part[i] = part;
    a.w.sel[i] = sel;
    a.w.ka[i] = (sel ? 0 : SIGN) | pack(v, l, m);
    a.w.va[i] = i;
}

// ---- 4. the region particles ----
__global__ __launch_bounds__(BLOCK) void k_pid_keys(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int r = a.w.vb[i];
    a.w.ka[i] = flip(a.pid[r >= 0 && r < a.N ? r : 0]);
}

// kb: the particle keys in (particle, not sel, volume, layer, module) order; va: the rows
__global__ __launch_bounds__(BLOCK) void k_mark(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    int r = a.w.va[i];
    if (r < 0 || r >= a.N) r = 0;
    const bool s = a.w.sel[r];
    bool head = false, vl = false, dup = false;
    if (s) {
        head = i == 0 || a.w.kb[i - 1] != a.w.kb[i];
        vl = head;
        if (!head) {   // the predecessor is a selected row of the same particle
            int q = a.w.va[i - 1];
            if (q < 0 || q >= a.N) q = 0;
            vl = a.vol[q] != a.vol[r] || a.lay[q] != a.lay[r];
            dup = !vl && a.mod[q] == a.mod[r];
        }
    }
    a.w.in_a[i] = (int64_t)head | ((int64_t)dup << 32);
    a.w.in_b[i] = (int64_t)s | ((int64_t)vl << 32);
}

__global__ __launch_bounds__(BLOCK) void k_heads(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int r = lo32(a.w.sum_a[i]);
    if (lo32(a.w.sum_a[i + 1]) != r && r >= 0 && r < a.N) a.w.pos[r] = i;
}

__global__ __launch_bounds__(BLOCK) void k_region(Build a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= a.N) return;
    const int R = lo32(a.w.sum_a[a.N]);
    int ref = 0;
    if (r < R) {
        int i = a.w.pos[r], e = r + 1 < R ? a.w.pos[r + 1] : a.N;
        if (i < 0 || i >= a.N) i = 0;
        if (e < i || e > a.N) e = i;
        const int hits = lo32(a.w.sum_b[e]) - lo32(a.w.sum_b[i]);
        const int layers = hi32(a.w.sum_b[e]) - hi32(a.w.sum_b[i]);
        const int dups = hi32(a.w.sum_a[e]) - hi32(a.w.sum_a[i]);
        ref = layers >= a.num_layers && dups == 0;
        a.o.part_id[r] = (int64_t)(a.w.kb[i] ^ SIGN);
        a.o.part_hits[r] = hits;
        a.o.part_ref[r] = (uint8_t)ref;
    }
    a.w.ref[r] = ref;
    if (r == 0) a.w.scal[S_R] = R;
}

// ---- 5. hit_dissociation ----
__global__ __launch_bounds__(BLOCK) void k_node_keys(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    a.w.ka[i] = flip(a.node[i]);
    a.w.va[i] = i;
}

// kb / vb: the nodes and rows in (node, row) order
__global__ __launch_bounds__(BLOCK) void k_hit_keys(Build a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.N) return;
    const int r = a.w.vb[p];
    a.w.ka[p] = flip(a.hit[r >= 0 && r < a.N ? r : 0]);
    a.w.va[p] = p;
}

// kc / vc: the hits and positions in (hit, node, row) order -> per position: kept | node head << 32
__global__ __launch_bounds__(BLOCK) void k_first(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    int p = a.w.vc[i];
    if (p < 0 || p >= a.N) return;
    bool first = i == 0 || a.w.kc[i - 1] != a.w.kc[i];
    if (!first) {
        int q = a.w.vc[i - 1];
        if (q < 0 || q >= a.N) q = 0;
        first = a.w.kb[q] != a.w.kb[p];
    }
    const bool head = p == 0 || a.w.kb[p - 1] != a.w.kb[p];
    a.w.in_a[p] = (int64_t)first | ((int64_t)head << 32);
}

__global__ __launch_bounds__(BLOCK) void k_csr(Build a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.N) return;
    const int64_t s = a.w.sum_a[p], n = a.w.sum_a[p + 1];
    const int e = lo32(s), t = hi32(s);
    if (lo32(n) != e && e >= 0 && e < a.N) {
        const int r = a.w.vb[p];
        a.o.node_part[e] = a.w.row_part[r >= 0 && r < a.N ? r : 0];
    }
    if (hi32(n) != t && t >= 0 && t < a.N) {
        a.o.node_id[t] = (int64_t)(a.w.kb[p] ^ SIGN);
        a.o.node_ptr[t] = e;
    }
    if (p == a.N - 1) {
        const int T = hi32(n), P = lo32(n);
        if (T >= 0 && T <= a.N) a.o.node_ptr[T] = P;
        a.w.scal[S_T] = T;
        a.w.scal[S_P] = P;
    }
}

}  // namespace

extern "C" {

size_t gtf_truth_build_workspace_bytes(int32_t n_rows, int32_t n_truth, int32_t n_particles) {
    const int64_t N = n_rows > 0 ? n_rows : 0;
    return carve(nullptr, N, n_truth > 0 ? n_truth : N, n_particles > 0 ? n_particles : 0).total;
}

int gtf_truth_build(const gtf_truth_in* in, const gtf_truth_buf* buf, gtf_truth* out, gtf_truth_counts* counts,
                    void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_truth_build";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_truth_in", "gtf_truth_in")) return rc;
    if (!buf || !out || !counts) return bad("gtf_truth_build: null buf, out or counts");
    if (in->n_rows < 0 || in->n_truth < 0 || in->n_particles < 0) return bad("gtf_truth_build: negative sizes");
    if (in->n_rows > MAX_ROWS || in->n_truth > MAX_ROWS || in->n_particles > MAX_ROWS)
        return bad("gtf_truth_build: more than 2^30 rows");
    if (in->min_volume > in->max_volume) return bad("gtf_truth_build: min_volume > max_volume");
    const int32_t N = in->n_rows, NP = in->n_particles;
    const char* miss = nullptr;
    if (!buf->node_ptr) miss = "buf.node_ptr";
    else if (N > 0 && (!in->node_idx || !in->hit_id || !in->particle_id || !in->volume_id || !in->layer_id ||
                       !in->module_id))
        miss = "a mapping column";
    else if (in->n_truth > 0 && (!in->truth_hit || !in->truth_part)) miss = "truth_hit / truth_part";
    else if (NP > 0 && (!in->part_id || !in->px || !in->py)) miss = "part_id / px / py";
    else if (N > 0 && (!buf->node_id || !buf->node_part || !buf->part_id || !buf->part_hits || !buf->part_ref))
        miss = "an output array of gtf_truth_buf";
    if (miss) {
        snprintf(m, sizeof(m), "gtf_truth_build: missing array: %s", miss);
        return bad(m);
    }
    if (N > 0 && (!workspace || workspace_bytes < gtf_truth_build_workspace_bytes(N, in->n_truth, NP)))
        return bad("gtf_truth_build: workspace smaller than gtf_truth_build_workspace_bytes");
    out->struct_size = (uint32_t)sizeof(gtf_truth);
    out->abi_version = GTF_ABI_VERSION;
    out->n_nodes = out->n_entries = out->n_particles = 0;
    out->pad_ = 0;
    out->node_id = buf->node_id; out->node_ptr = buf->node_ptr; out->node_part = buf->node_part;
    out->part_id = buf->part_id; out->part_hits = buf->part_hits; out->part_ref = buf->part_ref;
    counts->n_nodes = counts->n_entries = counts->n_particles = counts->n_reference = 0;
    counts->error = 0;
    counts->pad_ = 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (N == 0) {   // (one stream-ordered fill; nothing to bring back)
        if ((e = hipMemsetAsync(buf->node_ptr, 0, 4, st)) != hipSuccess) return fail(who, "memset", e);
        return 0;
    }
    Build a;
    a.N = N; a.NT = in->n_truth > 0 ? in->n_truth : N; a.NP = NP;
    a.num_layers = in->num_layers; a.min_volume = in->min_volume; a.max_volume = in->max_volume;
    a.pt_cut = in->pt_cut;
    a.node = in->node_idx; a.hit = in->hit_id; a.pid = in->particle_id;
    a.vol = in->volume_id; a.lay = in->layer_id; a.mod = in->module_id;
    a.th = in->n_truth > 0 ? in->truth_hit : in->hit_id;
    a.tp = in->n_truth > 0 ? in->truth_part : in->particle_id;
    a.part_id = in->part_id; a.px = in->px; a.py = in->py;
    a.o = *buf;
    a.w = carve(workspace, N, a.NT, NP);
    const Ws& w = a.w;
    const gtf::Cub cub{w.cub, st};
    if ((e = hipMemsetAsync(w.scal, 0, 4 * S_WORDS, st)) != hipSuccess) return fail(who, "memset", e);
    // 1. the high-pT ids
    if (NP > 0) {
        hipLaunchKernelGGL(k_particles, dim3(grid(NP)), dim3(BLOCK), 0, st, a);
        if ((e = cub.sort_pairs(w.ka, w.pk, w.va, w.pf, NP)) != hipSuccess) return fail(who, "sort particles", e);
        if ((e = cub.scan(w.pf, w.ps, NP + 1)) != hipSuccess) return fail(who, "scan particles", e);
    }
    // 2. the truth rows by hit
    hipLaunchKernelGGL(k_truth_rows, dim3(grid(a.NT)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.tk, w.va, w.tidx, a.NT)) != hipSuccess) return fail(who, "sort truth", e);
    hipLaunchKernelGGL(k_truth_sorted, dim3(grid(a.NT)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.tfs, w.ts, a.NT + 1)) != hipSuccess) return fail(who, "scan truth", e);
    // 3. the rows; 4. the region particles
    hipLaunchKernelGGL(k_rows, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.kb, w.va, w.vb, N)) != hipSuccess) return fail(who, "sort modules", e);
    hipLaunchKernelGGL(k_pid_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.kb, w.vb, w.va, N)) != hipSuccess) return fail(who, "sort region", e);
    hipLaunchKernelGGL(k_mark, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.in_a, w.sum_a, N + 1)) != hipSuccess) return fail(who, "scan heads", e);
    if ((e = cub.scan(w.in_b, w.sum_b, N + 1)) != hipSuccess) return fail(who, "scan rows", e);
    hipLaunchKernelGGL(k_heads, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_region, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sum(w.ref, w.scal + S_REF, N)) != hipSuccess) return fail(who, "sum", e);
    // 5. the CSR
    hipLaunchKernelGGL(k_node_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.kb, w.va, w.vb, N)) != hipSuccess) return fail(who, "sort nodes", e);
    hipLaunchKernelGGL(k_hit_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.kc, w.va, w.vc, N)) != hipSuccess) return fail(who, "sort pairs", e);
    hipLaunchKernelGGL(k_first, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.in_a, w.sum_a, N + 1)) != hipSuccess) return fail(who, "scan pairs", e);
    hipLaunchKernelGGL(k_csr, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t c[S_WORDS] = {0, 0, 0, 0, 0};
    if ((e = hipMemcpyAsync(c, w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    counts->error = (uint32_t)c[S_ERR];
    if (counts->error & GTF_TRUTH_ERR_RANGE)
        return bad("gtf_truth_build: a volume_id, layer_id or module_id outside [0, 2^21)");
    if (counts->error & GTF_TRUTH_ERR_MISSING) return bad("gtf_truth_build: a mapped hit has no truth row");
    if (c[S_T] < 0 || c[S_T] > N || c[S_P] < c[S_T] || c[S_P] > N || c[S_R] < 0 || c[S_R] > N || c[S_REF] < 0 ||
        c[S_REF] > c[S_R])
        return bad("gtf_truth_build: inconsistent counts");
    counts->n_nodes = out->n_nodes = c[S_T];
    counts->n_entries = out->n_entries = c[S_P];
    counts->n_particles = out->n_particles = c[S_R];
    counts->n_reference = c[S_REF];
    return 0;
}

}  // extern "C"
