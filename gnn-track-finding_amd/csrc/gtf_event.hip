// gtf_event.hip -- the packed event on the GPU (include/gtf.h: gtf_event_pack,
// gtf_fill_columns): what gtf/io.py build_event_csr assembles with NumPy after the CSR build
// -- the node columns of construct_graph (helper.py:465-545) in packed order and the empty
// state arrays event conversion starts from (event_conversion.py:53-101) -- so an event whose
// CSR gtf_build_event_csr_device left in HBM becomes a ready gtf_graph / gtf_nodes /
// gtf_states / gtf_edges without a round trip through the host.
//
//   pack  one launch, three grid-stride loops: the 4N words of gnn and xyzr (word f = column
//         f & 3 of CSV row order[f >> 2]), the 2N words of vivl, and per node layer, node_id
//         and solo (sub_id is non-decreasing in packed order: a node is alone when both
//         neighbouring entries differ)
//   fill  up to MAXC columns per launch (the column table in the kernel arguments,
//         blockIdx.y = column): every 1-, 4- or 8-byte word of the column gets the pattern
//
//   window  (gtf_event_window) the parsed node columns of gtf_csv_parse -> the kept rows of
//         io.read_nodes: lo <= layer_id <= hi, compacted in file order by one exclusive sum of
//         (kept | ambiguous << 32), with r = sqrt(x*x + y*y) and the list of the nodes whose x*x
//         or y*y lies so close to a rounding midpoint that the C library's pow(x, 2), which
//         defines r (io.edge_length_xy), may round the other way; gtf_event_radius_patch
//         scatters the caller's r of those nodes. One synchronisation, for the two counts.
//         A batch (gtf_event_window_ev) is the same two launches on the batch's rows and one
//         gather of the sum at the events' K + 1 row offsets: the kept rows per event.
//
// Plain loads, vector stores, consecutive lanes on consecutive destination words; no atomics,
// no allocation; pack and fill do not synchronise.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/gtf.h"
#include "gtf_host.h"

namespace {

using gtf::bad;
using gtf::fail;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int MAXC = GTF_FILL_MAX_COLUMNS;
constexpr int MAX_BLOCKS = 2048;   // of one loop's grid (8 a CU); longer arrays stride

inline int blocks(int64_t words, int cap) {
    const int64_t b = (words + BLOCK - 1) / BLOCK;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

struct Pack {
    int32_t N;
    const int32_t *order, *sub_id;
    const int64_t *ids, *layer_id;
    const double *x, *y, *z, *r;
    gtf_event_out o;
};

__global__ __launch_bounds__(BLOCK) void k_pack(Pack a) {
    const int64_t t0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x, step = (int64_t)gridDim.x * BLOCK;
    const int64_t N = a.N;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (a.o.gnn || a.o.xyzr) {
        for (int64_t f = t0; f < 4 * N; f += step) {
            const int c = (int)(f & 3);
            const int32_t row = a.order[f >> 2];
            const double* col = c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.r;
            const double v = row >= 0 && row < N ? col[row] : nan;   // (not a CSV row: nothing read)
            if (a.o.gnn) a.o.gnn[f] = v;
            if (a.o.xyzr) a.o.xyzr[f] = v;
        }
    }
    if (a.o.vivl) {
        for (int64_t f = t0; f < 2 * N; f += step) {
            const int32_t row = a.order[f >> 1];
            double v = nan;
            if (row >= 0 && row < N) {
                const int64_t lid = a.layer_id[row];
                v = (double)((f & 1) ? lid % 100 : lid / 1000);
            }
            a.o.vivl[f] = v;
        }
    }
    if (a.o.layer || a.o.node_id || a.o.solo) {
        for (int64_t i = t0; i < N; i += step) {
            if (a.o.layer || a.o.node_id) {   // solo reads sub_id alone: order may be NULL then
                const int32_t row = a.order[i];
                const bool ok = row >= 0 && row < N;
                if (a.o.layer) a.o.layer[i] = ok ? (double)(a.layer_id[row] % 100) : nan;
                if (a.o.node_id) a.o.node_id[i] = ok ? a.ids[row] : -1;
            }
            if (a.o.solo) {
                const int32_t s = a.sub_id[i];
                const bool before = i > 0 && a.sub_id[i - 1] == s, after = i + 1 < N && a.sub_id[i + 1] == s;
                a.o.solo[i] = !before && !after;
            }
        }
    }
}

struct Col {
    void* dst;
    uint64_t pattern;
    int64_t words;
    int32_t lg;      // log2(word bytes): 0, 2 or 3
    int32_t pad_;
};
struct ColTab {
    Col c[MAXC];
};

template <typename T>
__device__ __forceinline__ void fill_words(const Col& c) {
    T* dst = (T*)c.dst;
    const T v = (T)c.pattern;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < c.words; f += (int64_t)gridDim.x * BLOCK) dst[f] = v;
}

__global__ __launch_bounds__(BLOCK) void k_fill(ColTab tab) {
    const Col c = tab.c[blockIdx.y];
    if (c.lg == 3) fill_words<uint64_t>(c);
    else if (c.lg == 2) fill_words<uint32_t>(c);
    else fill_words<uint8_t>(c);
}

// ---- window ----
struct WinWs {
    int64_t *in, *sum;   // [n + 1] kept | ambiguous << 32; the exclusive sum
    int32_t* off;        // ev [K + 1] the caller's row offsets
    int64_t* at;         // ev [K + 1] the sum at the offsets
    gtf::Scratch cub;
    size_t total;
};

// K: the events of a batch; -1: one event, no offsets
WinWs win_carve(void* base, int64_t n, int64_t K) {
    WinWs w = {};
    gtf::Arena a(base);
    const size_t n1 = (size_t)(n > 0 ? n : 0) + 1;
    w.in = a.take<int64_t>(n1);
    w.sum = a.take<int64_t>(n1);
    if (K >= 0) {
        w.off = a.take<int32_t>((size_t)K + 1);
        w.at = a.take<int64_t>((size_t)K + 1);
    }
    w.cub = gtf::CubNeed().scan<int64_t>((int)n1).take(a);
    w.total = a.used();
    return w;
}

struct Win {
    int32_t n;
    int64_t lo, hi;
    const int64_t *ids, *layer_id;
    const double *x, *y, *z;
    gtf_window_out o;
    WinWs w;
};

// May a pow(v, 2) with a final error of at most 0.5625 ulp differ from the rounded v * v: the exact
// square p + e (e = fma(v, v, -p), exact) lies within ulp(p) / 16 of the midpoint between p and a
// neighbour. |e| <= ulp(p) / 2, so that is |e| > 7 / 16 ulp(p); ulp from the exponent bits, so every
// product below is exact. A square that is not a normal number (0 * 0 aside) is left to the caller.
__device__ __forceinline__ bool ambiguous_square(double v) {
    if (v == 0.0) return false;
    const double p = v * v;
    const int ex = (int)((uint64_t)__double_as_longlong(p) >> 52) & 0x7ff;
    if (ex == 0x7ff || ex < 64) return true;   // inf, nan; a square near or below the subnormals
    const double e = fma(v, v, -p);
    const double ulp = __longlong_as_double((int64_t)(ex - 52) << 52);
    return fabs(e) > 0.4375 * ulp;
}

__global__ __launch_bounds__(BLOCK) void k_window_flags(Win a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > a.n) return;
    int64_t f = 0;
    if (i < a.n) {
        const int64_t l = a.layer_id[i];
        if (l >= a.lo && l <= a.hi) f = 1 | ((int64_t)(ambiguous_square(a.x[i]) || ambiguous_square(a.y[i])) << 32);
    }
    a.w.in[i] = f;
}

__global__ __launch_bounds__(BLOCK) void k_window_scatter(Win a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int64_t f = a.w.in[i], s = a.w.sum[i];
    if (!(f & 1)) return;
    const int d = (int)(uint32_t)s, k = (int)((uint64_t)s >> 32);
    if (d < 0 || d >= a.n || k < 0 || k >= a.n) return;
    const double x = a.x[i], y = a.y[i];
    a.o.node_idx[d] = a.ids[i];
    a.o.layer_id[d] = a.layer_id[i];
    a.o.x[d] = x;
    a.o.y[d] = y;
    a.o.z[d] = a.z[i];
    a.o.r[d] = __dsqrt_rn(x * x + y * y);   // two rounded products, a rounded sum (-ffp-contract=off)
    if (f >> 32) {
        a.o.amb_index[k] = d;
        a.o.amb_x[k] = x;
        a.o.amb_y[k] = y;
    }
}

// a batch: the sum at the events' offsets
__global__ __launch_bounds__(BLOCK) void k_window_events(Win a, int K) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e > K) return;
    const int32_t r = a.w.off[e];
    a.w.at[e] = a.w.sum[r < 0 ? 0 : r > a.n ? a.n : r];
}

__global__ __launch_bounds__(BLOCK) void k_radius_patch(double* r, int32_t n_nodes, const int32_t* index, const double* value,
                                                        int32_t n) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const int32_t d = index[k];
    if (d >= 0 && d < n_nodes) r[d] = value[k];
}

}  // namespace

extern "C" {

size_t gtf_event_window_workspace_bytes(int32_t n_rows) { return win_carve(nullptr, n_rows, -1).total; }

size_t gtf_event_window_ev_workspace_bytes(int32_t n_rows, int32_t n_events) {
    return win_carve(nullptr, n_rows, n_events > 0 ? n_events : 0).total;
}

}  // extern "C"

namespace {

// Both entry points: row_off null is one event (K is not read), else the K events of a batch with
// their kept rows in n_kept.
int window(const char* who, const gtf_window_in* in, const int32_t* row_off, int32_t K, const gtf_window_out* out,
           int32_t* n_kept, gtf_window_counts* counts, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    char m[200];
    auto no = [&](const char* what) {
        snprintf(m, sizeof(m), "%s: %s", who, what);
        return bad(m);
    };
    if (int rc = gtf::check_abi(in, who, "gtf_window_in", "gtf_window_in")) return rc;
    if (!out || !counts) return no("null out or counts");
    if (in->n_rows < 0) return no("negative n_rows");
    if (in->n_rows > INT32_MAX / 4) return no("event too large for int32 indices");
    const int32_t n = in->n_rows;
    const bool ev = row_off != nullptr;
    if (ev) {
        if (K > 0 && !n_kept) return no("null n_kept with n_events > 0");
        if (row_off[0] != 0 || row_off[K] != n) return no("row_off does not run from 0 to n_rows");
        for (int e = 0; e < K; e++)
            if (row_off[e + 1] < row_off[e]) return no("row_off decreases");
        for (int e = 0; e < K; e++) n_kept[e] = 0;
    }
    counts->n_kept = counts->n_ambiguous = 0;
    if (n == 0) return 0;
    if (!in->node_idx || !in->layer_id || !in->x || !in->y || !in->z) return no("missing input column (node_idx, layer_id, x, y, z)");
    if (!out->node_idx || !out->layer_id || !out->x || !out->y || !out->z || !out->r || !out->amb_index || !out->amb_x ||
        !out->amb_y)
        return no("missing array of gtf_window_out");
    if (!workspace || workspace_bytes < win_carve(nullptr, n, ev ? K : -1).total)
        return no(ev ? "workspace smaller than gtf_event_window_ev_workspace_bytes"
                     : "workspace smaller than gtf_event_window_workspace_bytes");
    Win a;
    a.n = n; a.lo = in->lo; a.hi = in->hi;
    a.ids = in->node_idx; a.layer_id = in->layer_id; a.x = in->x; a.y = in->y; a.z = in->z;
    a.o = *out;
    a.w = win_carve(workspace, n, ev ? K : -1);
    hipStream_t st = (hipStream_t)stream;
    const gtf::Cub cub{a.w.cub, st};
    hipError_t e;
    if (ev && (e = hipMemcpyAsync(a.w.off, row_off, 4 * ((size_t)K + 1), hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(who, "offsets", e);
    hipLaunchKernelGGL(k_window_flags, dim3(gtf::grid((int64_t)n + 1)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(a.w.in, a.w.sum, n + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_window_scatter, dim3(gtf::grid(n)), dim3(BLOCK), 0, st, a);
    if (ev) hipLaunchKernelGGL(k_window_events, dim3(gtf::grid((int64_t)K + 1)), dim3(BLOCK), 0, st, a, K);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int64_t total = 0;
    std::vector<int64_t> at(ev ? (size_t)K + 1 : 0);
    if (ev) e = hipMemcpyAsync(at.data(), a.w.at, 8 * at.size(), hipMemcpyDeviceToHost, st);
    else e = hipMemcpyAsync(&total, a.w.sum + n, 8, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    if (ev) total = at[K];
    const int64_t kept = (int64_t)(uint32_t)total, amb = (int64_t)((uint64_t)total >> 32);
    if (kept > n || amb > kept) return no("inconsistent counts");
    for (int f = 0; ev && f < K; f++) {
        const int64_t k = (int64_t)(uint32_t)at[f + 1] - (int64_t)(uint32_t)at[f];
        if (k < 0 || k > row_off[f + 1] - row_off[f]) return no("inconsistent counts");
        n_kept[f] = (int32_t)k;
    }
    counts->n_kept = (int32_t)kept;
    counts->n_ambiguous = (int32_t)amb;
    return 0;
}

}  // namespace

extern "C" {

int gtf_event_window(const gtf_window_in* in, const gtf_window_out* out, gtf_window_counts* counts, void* workspace,
                     size_t workspace_bytes, gtf_stream_t stream) {
    return window("gtf_event_window", in, nullptr, 1, out, nullptr, counts, workspace, workspace_bytes, stream);
}

int gtf_event_window_ev(const gtf_window_in* in, const int32_t* row_off, int32_t n_events, const gtf_window_out* out,
                        int32_t* n_kept, gtf_window_counts* counts, void* workspace, size_t workspace_bytes,
                        gtf_stream_t stream) {
    const char* who = "gtf_event_window_ev";
    if (n_events < 0) return bad("gtf_event_window_ev: negative n_events");
    static const int32_t none[1] = {0};
    if (n_events > 0 && !row_off) return bad("gtf_event_window_ev: null row_off with n_events > 0");
    return window(who, in, row_off ? row_off : none, n_events, out, n_kept, counts, workspace, workspace_bytes, stream);
}

int gtf_event_radius_patch(double* r, int32_t n_nodes, const int32_t* index, const double* value, int32_t n,
                           gtf_stream_t stream) {
    if (n_nodes < 0 || n < 0) return bad("gtf_event_radius_patch: negative sizes");
    if (n == 0) return 0;
    if (!r || !index || !value) return bad("gtf_event_radius_patch: null r, index or value with n > 0");
    hipLaunchKernelGGL(k_radius_patch, dim3(gtf::grid(n)), dim3(BLOCK), 0, (hipStream_t)stream, r, n_nodes, index, value, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("gtf_event_radius_patch", "launch", e);
    return 0;
}

int gtf_event_pack(const gtf_event_csr* ev, const gtf_event_cols* in, const gtf_event_out* out, gtf_stream_t stream) {
    const char* who = "gtf_event_pack";
    if (!ev) return bad("gtf_event_pack: null gtf_event_csr");
    if (!out) return bad("gtf_event_pack: null gtf_event_out");
    if (ev->n_nodes < 0 || ev->n_rows < 0 || ev->n_edges < 0 || ev->n_subgraphs < 0)
        return bad("gtf_event_pack: negative sizes");
    if (ev->n_nodes > INT32_MAX / 4) return bad("gtf_event_pack: event too large for int32 indices");
    const int32_t N = (int32_t)ev->n_nodes;
    if (N == 0) return 0;
    const bool coords = out->gnn || out->xyzr, lids = out->layer || out->vivl;
    if (!(coords || lids || out->node_id || out->solo)) return 0;
    if ((coords || lids || out->node_id) && !ev->order) return bad("gtf_event_pack: missing event array order");
    if (out->node_id && !ev->node_id) return bad("gtf_event_pack: missing event array node_id");
    if (out->solo && !ev->sub_id) return bad("gtf_event_pack: missing event array sub_id");
    if ((coords || lids) && !in) return bad("gtf_event_pack: null gtf_event_cols");
    if (coords && (!in->x || !in->y || !in->z || !in->r)) return bad("gtf_event_pack: missing input column (x, y, z, r)");
    if (lids && !in->layer_id) return bad("gtf_event_pack: missing input column layer_id");
    Pack a;
    a.N = N;
    a.order = ev->order; a.sub_id = ev->sub_id; a.ids = ev->node_id;
    a.x = in ? in->x : nullptr; a.y = in ? in->y : nullptr; a.z = in ? in->z : nullptr; a.r = in ? in->r : nullptr;
    a.layer_id = in ? in->layer_id : nullptr;
    a.o = *out;
    hipLaunchKernelGGL(k_pack, dim3(blocks(4 * (int64_t)N, MAX_BLOCKS)), dim3(BLOCK), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_fill_columns(const gtf_fill_column* cols, int32_t n_cols, gtf_stream_t stream) {
    const char* who = "gtf_fill_columns";
    if (n_cols < 0 || n_cols > MAXC) return bad("gtf_fill_columns: n_cols must be in [0, 32]");
    if (n_cols == 0) return 0;
    if (!cols) return bad("gtf_fill_columns: null column table");
    ColTab tab;
    int n = 0;
    int64_t longest = 0;
    for (int i = 0; i < n_cols; i++) {
        const gtf_fill_column& c = cols[i];
        if (c.rows < 0) return bad("gtf_fill_columns: negative rows");
        const int32_t rb = c.row_bytes;
        if (rb != 1 && rb != 4 && (rb <= 0 || rb % 8)) return bad("gtf_fill_columns: row_bytes must be 1, 4 or a multiple of 8");
        if (c.rows > 0 && !c.dst) return bad("gtf_fill_columns: null destination with rows > 0");
        const int lg = rb == 1 ? 0 : rb == 4 ? 2 : 3;
        if ((uintptr_t)c.dst % ((uintptr_t)1 << lg)) return bad("gtf_fill_columns: destination not aligned to its row words");
        if (c.rows > INT64_MAX / rb) return bad("gtf_fill_columns: column too large");
        if (c.rows == 0) continue;
        Col& t = tab.c[n++];
        t.dst = c.dst;
        t.pattern = c.pattern;
        t.words = c.rows * (int64_t)(rb >> lg);
        t.lg = lg;
        t.pad_ = 0;
        if (t.words > longest) longest = t.words;
    }
    if (n == 0) return 0;
    for (int i = n; i < MAXC; i++) tab.c[i] = tab.c[0];
    int cap = 2 * MAX_BLOCKS / n;
    cap = cap < 64 ? 64 : cap;
    hipLaunchKernelGGL(k_fill, dim3(blocks(longest, cap), n), dim3(BLOCK), 0, (hipStream_t)stream, tab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

}  // extern "C"
