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
// Plain loads, vector stores, consecutive lanes on consecutive destination words; no atomics,
// no synchronisation, no allocation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

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

}  // namespace

extern "C" {

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
