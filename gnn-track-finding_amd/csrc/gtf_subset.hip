// gtf_subset.hip -- node removal between two iterations on the GPU (include/gtf.h:
// gtf_graph_subset_plan / _apply, gtf_subset_gather, gtf_refresh_send_mw): the packed form of
// the reference's subGraph.remove_nodes_from(extracted) (extract_track_candidates.py:459-467)
// plus dropping the emptied subgraphs, array for array gtf/graph.py's subset() and
// refresh_send_mw(), so the extraction's verdict becomes the next iteration's graph without a
// round trip through the host.
//
//   plan   1. per node: keep flag; per wavefront one integer atomic on the counter of each
//             subgraph it holds kept nodes of
//          2. per slot: receiver (binary search in slot_ptr) and a 64-bit code -- dropped,
//             inside (receiver and sender kept; an edge or a dict key), or an orphan's order
//             key (tse_rank, else 2^31 + uts_rank: pack() discovers the track_state_estimates
//             keys first)
//          3. per node: surviving slots and out-edges; hipCUB exclusive sums of the keep flags
//             (old -> new node), the two counts (the new slot_ptr / out_ptr) and the subgraphs
//             that keep a node (the dense sub_id)
//          4. per slot: its new position = the segment's new start + the inside slots before it,
//             or + every inside slot + the orphans of the segment that order before it (by
//             key, then old index): a count over the segment's codes, any segment length
//          5. per node: new -> old map, new sub_id and solo; the four sizes to the host (the
//             call's one synchronisation)
//   apply  per kept node its rows of the structure arrays and its out-list; per surviving slot
//          slot_map and the renumbered slot_src
//   gather the payload: up to MAXC columns per launch (the column table in the kernel
//          arguments, blockIdx.y = column), rows through the new -> old map, 8-byte words where
//          the rows allow, consecutive lanes on consecutive destination words
//
// No same-address atomic (the subgraph counters are n_sub different words), vector stores only.
// The sizes of the result live in a header at the start of the workspace, so apply and gather
// need nothing from the host but the workspace pointer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/gtf.h"
#include "gtf_host.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int MAXC = 32;              // columns per gather launch
constexpr int GATHER_BLOCKS = 4096;   // blocks of a gather launch, over its columns (16 a CU)
constexpr uint32_t MAGIC = 0x67735562u;
constexpr int64_t DROPPED = -2, INSIDE = -1;   // slot codes; >= 0: an orphan's order key

// the plan's header, at offset 0 of the workspace
struct Hdr {
    uint32_t magic;
    int32_t N, S, E, n_sub;        // of the planned graph
    int32_t N2, S2, E2, n_sub2;    // of the result
    int32_t pad_;
    int64_t off_node_map, off_slot_map;   // byte offsets of the new -> old maps
};

struct Ws {
    Hdr* hdr;
    int32_t *scal, *flag, *new_idx, *scnt, *sptr, *ocnt, *optr, *node_sub, *node_map, *slot_dst, *slot_new, *slot_map;
    uint8_t* node_solo;
    int64_t* code;
    // n_sub-dependent part, after everything apply and gather read
    int32_t *sub_cnt, *sub_flag, *sub_new;
    gtf::Scratch cub;
    size_t total;
};

Ws carve(const void* base, int64_t N, int64_t S, int64_t nsub) {
    Ws w;
    gtf::Arena a(base);
    const size_t n = (size_t)N, n1 = n + 1, s = (size_t)S, b1 = (size_t)nsub + 1;
    w.hdr = a.take<Hdr>(1);
    w.scal = a.take<int32_t>(16);
    w.flag = a.take<int32_t>(n1);
    w.new_idx = a.take<int32_t>(n1);
    w.scnt = a.take<int32_t>(n1);
    w.sptr = a.take<int32_t>(n1);
    w.ocnt = a.take<int32_t>(n1);
    w.optr = a.take<int32_t>(n1);
    w.node_sub = a.take<int32_t>(n);
    w.node_map = a.take<int32_t>(n);
    w.node_solo = a.take<uint8_t>(n);
    w.slot_dst = a.take<int32_t>(s);
    w.slot_new = a.take<int32_t>(s);
    w.slot_map = a.take<int32_t>(s);
    w.code = a.take<int64_t>(s);
    w.sub_cnt = a.take<int32_t>(b1);
    w.sub_flag = a.take<int32_t>(b1);
    w.sub_new = a.take<int32_t>(b1);
    w.cub = gtf::CubNeed().scan<int32_t>((int)n1).scan<int32_t>((int)b1).take(a);
    w.total = a.used();
    return w;
}

struct Plan {
    int32_t N, S, E, n_sub;
    const int32_t *slot_ptr, *slot_src, *out_ptr, *out_slot, *tse_rank, *uts_rank, *sub_id;
    const uint8_t *is_edge, *keep;
    Ws w;
};

// ---- plan ----
__global__ __launch_bounds__(BLOCK) void k_nodes(Plan a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (v == 0) a.w.flag[a.N] = 0;
    int s = -1;
    if (v < a.N) {
        const int f = a.keep[v] != 0;
        a.w.flag[v] = f;
        if (f) s = a.sub_id[v];
        if (s >= a.n_sub) s = -1;
    }
    // one atomic per distinct subgraph of the wavefront: consecutive nodes mostly share theirs, and an
    // event that is one giant subgraph would otherwise put every kept node on the same word
    unsigned long long todo = __ballot(s >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int s0 = __shfl(s, leader);
        const unsigned long long m = __ballot(s == s0);
        if (lane == leader) atomicAdd(&a.w.sub_cnt[s0], __popcll(m));
        todo &= ~m;
    }
}

// the slot's segment, clamped to the slot arrays (a malformed slot_ptr reads nothing outside)
__device__ __forceinline__ void segment(const Plan& a, int v, int& lo, int& hi) {
    lo = a.slot_ptr[v];
    hi = a.slot_ptr[v + 1];
    if (lo < 0) lo = 0;
    if (hi > a.S) hi = a.S;
}

__global__ __launch_bounds__(BLOCK) void k_classify(Plan a) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= a.S) return;
    int lo = 0, hi = a.N - 1;   // receiver: slot_ptr[v] <= k < slot_ptr[v + 1]
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a.slot_ptr[mid + 1] <= k) lo = mid + 1;
        else hi = mid;
    }
    const int v = lo;
    a.w.slot_dst[k] = v;
    int64_t c = DROPPED;
    if (a.keep[v]) {
        const int src = a.slot_src[k];
        const int tr = a.tse_rank[k], ur = a.uts_rank[k];
        const bool key = tr >= 0 || ur >= 0;
        const bool inside = src >= 0 && src < a.N && a.keep[src];
        if (inside) c = (a.is_edge[k] || key) ? INSIDE : DROPPED;
        else if (key) c = tr >= 0 ? (int64_t)tr : ((int64_t)1 << 31) + ur;
    }
    a.w.code[k] = c;
}

__device__ __forceinline__ bool out_edge_survives(const Plan& a, int o) {
    const int k = a.out_slot[o];
    return k >= 0 && k < a.S && a.w.code[k] == INSIDE && a.is_edge[k];
}

__global__ __launch_bounds__(BLOCK) void k_count(Plan a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v == 0) a.w.scnt[a.N] = a.w.ocnt[a.N] = 0;
    if (v >= a.N) return;
    int c = 0, oc = 0;
    if (a.keep[v]) {
        int lo, hi;
        segment(a, v, lo, hi);
        for (int k = lo; k < hi; k++) c += a.w.code[k] != DROPPED;
        int ob = a.out_ptr[v], oe = a.out_ptr[v + 1];
        if (ob < 0) ob = 0;
        if (oe > a.E) oe = a.E;
        for (int o = ob; o < oe; o++) oc += out_edge_survives(a, o);
    }
    a.w.scnt[v] = c;
    a.w.ocnt[v] = oc;
}

__global__ __launch_bounds__(BLOCK) void k_subflag(Plan a) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s <= a.n_sub) a.w.sub_flag[s] = s < a.n_sub && a.w.sub_cnt[s] > 0;
}

__global__ __launch_bounds__(BLOCK) void k_pos(Plan a) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= a.S) return;
    const int64_t c = a.w.code[k];
    int nw = -1;
    if (c != DROPPED) {
        const int v = a.w.slot_dst[k];
        int lo, hi;
        segment(a, v, lo, hi);
        int pos = 0;
        if (c == INSIDE) {
            for (int j = lo; j < k; j++) pos += a.w.code[j] == INSIDE;
        } else {
            for (int j = lo; j < hi; j++) {
                const int64_t cj = a.w.code[j];
                pos += cj == INSIDE || (cj >= 0 && (cj < c || (cj == c && j < k)));
            }
        }
        const int64_t q = (int64_t)a.w.sptr[v] + pos;
        if (q >= 0 && q < a.S) {
            nw = (int)q;
            a.w.slot_map[nw] = c == INSIDE ? k : ~k;   // (an orphan: the old index complemented)
        }
    }
    a.w.slot_new[k] = nw;
}

__global__ __launch_bounds__(BLOCK) void k_finish(Plan a, int64_t off_node_map, int64_t off_slot_map) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v == 0) {
        Hdr h;
        h.magic = MAGIC;
        h.N = a.N; h.S = a.S; h.E = a.E; h.n_sub = a.n_sub;
        h.N2 = a.w.new_idx[a.N];
        h.S2 = a.w.sptr[a.N];
        h.E2 = a.w.optr[a.N];
        h.n_sub2 = a.w.sub_new[a.n_sub];
        h.pad_ = 0;
        h.off_node_map = off_node_map;
        h.off_slot_map = off_slot_map;
        *a.w.hdr = h;
        a.w.scal[0] = h.N2; a.w.scal[1] = h.S2; a.w.scal[2] = h.E2; a.w.scal[3] = h.n_sub2;
    }
    if (v >= a.N || !a.w.flag[v]) return;
    const int nv = a.w.new_idx[v];
    if (nv >= 0 && nv < a.N) a.w.node_map[nv] = v;
    const int s = a.sub_id[v];
    const bool ok = s >= 0 && s < a.n_sub;
    a.w.node_sub[v] = ok ? a.w.sub_new[s] : -1;
    a.w.node_solo[v] = ok && a.w.sub_cnt[s] == 1;
}

// ---- apply ----
struct Apply {
    int32_t N, S, E;
    const int32_t *slot_src, *out_ptr, *out_slot;
    const uint8_t* is_edge;
    gtf_subset_out o;
    Ws w;
};

__global__ __launch_bounds__(BLOCK) void k_apply_nodes(Apply a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    const Hdr h = *a.w.hdr;
    if (h.magic != MAGIC || h.N != a.N || h.S != a.S || h.E != a.E) return;   // not this graph's plan
    if (v == 0) {
        if (a.o.slot_ptr) a.o.slot_ptr[h.N2] = h.S2;
        if (a.o.out_ptr) a.o.out_ptr[h.N2] = h.E2;
    }
    if (v >= a.N || !a.w.flag[v]) return;
    const int nv = a.w.new_idx[v];
    if (nv < 0 || nv >= h.N2) return;
    if (a.o.node_map) a.o.node_map[nv] = v;
    if (a.o.slot_ptr) a.o.slot_ptr[nv] = a.w.sptr[v];
    if (a.o.out_ptr) a.o.out_ptr[nv] = a.w.optr[v];
    if (a.o.sub_id) a.o.sub_id[nv] = a.w.node_sub[v];
    if (a.o.solo) a.o.solo[nv] = a.w.node_solo[v];
    if (a.o.out_slot) {   // the surviving out-edges, successor order kept
        int ob = a.out_ptr[v], oe = a.out_ptr[v + 1];
        if (ob < 0) ob = 0;
        if (oe > a.E) oe = a.E;
        int64_t j = a.w.optr[v];
        for (int o = ob; o < oe; o++) {
            const int k = a.out_slot[o];
            if (k >= 0 && k < a.S && a.w.code[k] == INSIDE && a.is_edge[k]) {
                if (j >= 0 && j < h.E2) a.o.out_slot[j] = a.w.slot_new[k];
                j++;
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_apply_slots(Apply a) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    const Hdr h = *a.w.hdr;
    if (h.magic != MAGIC || h.N != a.N || h.S != a.S || h.E != a.E) return;
    if (k >= a.S) return;
    const int nw = a.w.slot_new[k];
    if (nw < 0 || nw >= h.S2) return;
    if (a.o.slot_map) a.o.slot_map[nw] = k;
    if (a.o.slot_src) {
        int s = -1;
        if (a.w.code[k] == INSIDE) {
            const int src = a.slot_src[k];
            if (src >= 0 && src < a.N) s = a.w.new_idx[src];
        }
        a.o.slot_src[nw] = s;
    }
}

// ---- gather ----
struct Col {
    const void* src;
    void* dst;
    int32_t words;   // per row
    int32_t mode;    // fill | log2(word bytes) << 8
};
struct ColTab {
    Col c[MAXC];
};

// rows r0 .. r0 + BLOCK of one column: lane t stores destination words t, t + BLOCK, ... of the
// tile's W * BLOCK consecutive words
template <typename T, int WC>
__device__ __forceinline__ void gather_tiles(const Col& c, const int32_t* map, int64_t rows, int limit, int fill) {
    const int W = WC > 0 ? WC : c.words;
    const T* src = (const T*)c.src;
    T* dst = (T*)c.dst;
    const T nanw = sizeof(T) == 8 ? (T)0x7ff8000000000000ull : (T)0;
    for (int64_t r0 = (int64_t)blockIdx.x * BLOCK; r0 < rows; r0 += (int64_t)gridDim.x * BLOCK) {
        const int n = rows - r0 < BLOCK ? (int)(rows - r0) : BLOCK;
        // (a constant width keeps the index arithmetic in 32 bits; any other row may be long)
        using I = typename std::conditional<(WC > 0), int, int64_t>::type;
        for (I f = threadIdx.x; f < (I)n * W; f += BLOCK) {
            const I row = f / W, w = f - row * W;
            T val = 0;
            if (fill != GTF_COL_ZERO_ALL) {
                const int m = map[r0 + row], old = m >= 0 ? m : ~m;
                if (old >= limit) val = 0;   // (not a row of the planned graph: nothing read)
                else if (m >= 0 || fill == GTF_COL_COPY) val = src[(int64_t)old * W + w];
                else if (fill == GTF_COL_NAN_ORPHAN) val = nanw;
            }
            dst[r0 * W + f] = val;
        }
    }
}

template <typename T>
__device__ __forceinline__ void gather_words(const Col& c, const int32_t* map, int64_t rows, int limit, int fill) {
    switch (c.words) {   // (block-uniform: the usual row widths get a constant divisor)
    case 1: gather_tiles<T, 1>(c, map, rows, limit, fill); break;
    case 3: gather_tiles<T, 3>(c, map, rows, limit, fill); break;
    case 4: gather_tiles<T, 4>(c, map, rows, limit, fill); break;
    case 5: gather_tiles<T, 5>(c, map, rows, limit, fill); break;
    default: gather_tiles<T, 0>(c, map, rows, limit, fill);
    }
}

__global__ __launch_bounds__(BLOCK) void k_gather(const void* ws, int axis, ColTab tab) {
    const Hdr h = *(const Hdr*)ws;
    if (h.magic != MAGIC) return;
    const Col c = tab.c[blockIdx.y];
    const int64_t rows = axis == 0 ? h.N2 : h.S2;
    const int32_t* map = (const int32_t*)((const char*)ws + (axis == 0 ? h.off_node_map : h.off_slot_map));
    const int fill = c.mode & 0xff, lg = c.mode >> 8;
    const int limit = axis == 0 ? h.N : h.S;
    if (lg == 3) gather_words<uint64_t>(c, map, rows, limit, fill);
    else if (lg == 2) gather_words<uint32_t>(c, map, rows, limit, fill);
    else gather_words<uint8_t>(c, map, rows, limit, fill);
}

// ---- send weights ----
struct Send {
    int32_t N, S;
    const int32_t *slot_ptr, *slot_src, *slot_dst, *tse_rank;
    const uint8_t* is_edge;
    const double* tse_mw;
    double* send_mw;
};

__global__ __launch_bounds__(BLOCK) void k_send_mw(Send a) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= a.S) return;
    double mw = __longlong_as_double(0x7ff8000000000000ll);
    const int u = a.slot_src[k];
    if (a.is_edge[k] && u >= 0 && u < a.N) {
        int v;
        if (a.slot_dst) v = a.slot_dst[k];
        else {
            int lo = 0, hi = a.N - 1;
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (a.slot_ptr[mid + 1] <= k) lo = mid + 1;
                else hi = mid;
            }
            v = lo;
        }
        // the slot (receiver u, sender v): u's non-orphan slots ascend by slot_src, orphans (-1) last
        int lo = a.slot_ptr[u], hi = a.slot_ptr[u + 1];
        if (lo < 0) lo = 0;
        if (hi > a.S) hi = a.S;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const int s = a.slot_src[mid];
            if (s >= 0 && s < v) lo = mid + 1;
            else hi = mid;
        }
        if (lo < a.S && lo < a.slot_ptr[u + 1] && a.slot_src[lo] == v && a.tse_rank[lo] >= 0) mw = a.tse_mw[lo];
    }
    a.send_mw[k] = mw;
}

}  // namespace

extern "C" {

size_t gtf_graph_subset_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_edges, int32_t n_sub) {
    (void)n_edges;   // (no per-edge scratch: the out view is walked per sender)
    return carve(nullptr, n_nodes > 0 ? n_nodes : 0, n_slots > 0 ? n_slots : 0, n_sub > 0 ? n_sub : 0).total;
}

int gtf_graph_subset_plan(const gtf_graph* g, const int32_t* tse_rank, const int32_t* uts_rank,
                          const int32_t* sub_id, int32_t n_sub, const uint8_t* keep, void* workspace,
                          size_t workspace_bytes, gtf_subset_counts* counts, gtf_stream_t stream) {
    const char* who = "gtf_graph_subset_plan";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (g->n_nodes < 0 || g->n_slots < 0 || g->n_edges < 0 || n_sub < 0)
        return bad("gtf_graph_subset_plan: negative sizes");
    const int32_t N = g->n_nodes, S = g->n_slots, E = g->n_edges;
    if (!counts) return bad("gtf_graph_subset_plan: null counts");
    if (N > 0 && !g->slot_ptr) return bad("gtf_graph_subset_plan: missing graph array slot_ptr");
    if (N > 0 && !g->out_ptr) return bad("gtf_graph_subset_plan: missing graph array out_ptr");
    if (N > 0 && !keep) return bad("gtf_graph_subset_plan: missing array keep");
    if (N > 0 && !sub_id) return bad("gtf_graph_subset_plan: missing array sub_id");
    if (S > 0 && !g->slot_src) return bad("gtf_graph_subset_plan: missing graph array slot_src");
    if (S > 0 && !g->is_edge) return bad("gtf_graph_subset_plan: missing graph array is_edge");
    if (S > 0 && !tse_rank) return bad("gtf_graph_subset_plan: missing array tse_rank");
    if (S > 0 && !uts_rank) return bad("gtf_graph_subset_plan: missing array uts_rank");
    if (E > 0 && !g->out_slot) return bad("gtf_graph_subset_plan: missing graph array out_slot");
    if ((S > 0 || E > 0) && N == 0) return bad("gtf_graph_subset_plan: slots or edges without nodes");
    if (!workspace || workspace_bytes < gtf_graph_subset_workspace_bytes(N, S, E, n_sub))
        return bad("gtf_graph_subset_plan: workspace smaller than gtf_graph_subset_workspace_bytes");
    counts->n_nodes = counts->n_slots = counts->n_edges = counts->n_sub = 0;
    if (N == 0) return 0;

    Plan a;
    a.N = N; a.S = S; a.E = E; a.n_sub = n_sub;
    a.slot_ptr = g->slot_ptr; a.slot_src = g->slot_src; a.out_ptr = g->out_ptr; a.out_slot = g->out_slot;
    a.is_edge = g->is_edge; a.tse_rank = tse_rank; a.uts_rank = uts_rank; a.sub_id = sub_id; a.keep = keep;
    a.w = carve(workspace, N, S, n_sub);
    const Ws& w = a.w;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(w.sub_cnt, 0, 4 * (size_t)(n_sub + 1), st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_nodes, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if (S > 0) hipLaunchKernelGGL(k_classify, dim3(grid(S)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_count, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_subflag, dim3(grid((int64_t)n_sub + 1)), dim3(BLOCK), 0, st, a);
    const gtf::Cub cub{w.cub, st};
    if ((e = cub.scan(w.flag, w.new_idx, N + 1)) != hipSuccess) return fail(who, "scan", e);
    if ((e = cub.scan(w.scnt, w.sptr, N + 1)) != hipSuccess) return fail(who, "scan", e);
    if ((e = cub.scan(w.ocnt, w.optr, N + 1)) != hipSuccess) return fail(who, "scan", e);
    if ((e = cub.scan(w.sub_flag, w.sub_new, n_sub + 1)) != hipSuccess) return fail(who, "scan", e);
    if (S > 0) hipLaunchKernelGGL(k_pos, dim3(grid(S)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_finish, dim3(grid(N)), dim3(BLOCK), 0, st, a, (int64_t)((char*)w.node_map - (char*)workspace),
                       (int64_t)((char*)w.slot_map - (char*)workspace));
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t c[4] = {0, 0, 0, 0};
    if ((e = hipMemcpyAsync(c, w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    if (c[0] < 0 || c[0] > N || c[1] < 0 || c[1] > S || c[2] < 0 || c[2] > E || c[3] < 0 || c[3] > n_sub)
        return bad("gtf_graph_subset_plan: inconsistent slot_ptr / out_ptr");
    counts->n_nodes = c[0]; counts->n_slots = c[1]; counts->n_edges = c[2]; counts->n_sub = c[3];
    return 0;
}

int gtf_graph_subset_apply(const gtf_graph* g, const void* workspace, const gtf_subset_out* out,
                           gtf_stream_t stream) {
    const char* who = "gtf_graph_subset_apply";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (g->n_nodes < 0 || g->n_slots < 0 || g->n_edges < 0) return bad("gtf_graph_subset_apply: negative sizes");
    const int32_t N = g->n_nodes, S = g->n_slots, E = g->n_edges;
    if (!out) return bad("gtf_graph_subset_apply: null gtf_subset_out");
    if (!workspace) return bad("gtf_graph_subset_apply: null workspace");
    if (N == 0) return bad("gtf_graph_subset_apply: an empty graph has no plan to apply");
    if (!g->out_ptr) return bad("gtf_graph_subset_apply: missing graph array out_ptr");
    if (S > 0 && !g->slot_src) return bad("gtf_graph_subset_apply: missing graph array slot_src");
    if (S > 0 && !g->is_edge) return bad("gtf_graph_subset_apply: missing graph array is_edge");
    if (E > 0 && !g->out_slot) return bad("gtf_graph_subset_apply: missing graph array out_slot");
    Apply a;
    a.N = N; a.S = S; a.E = E;
    a.slot_src = g->slot_src; a.out_ptr = g->out_ptr; a.out_slot = g->out_slot; a.is_edge = g->is_edge;
    a.o = *out;
    a.w = carve(workspace, N, S, 0);   // (the n_sub-dependent part is not read here)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_apply_nodes, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if (S > 0 && (a.o.slot_map || a.o.slot_src)) hipLaunchKernelGGL(k_apply_slots, dim3(grid(S)), dim3(BLOCK), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_subset_gather(const void* workspace, int32_t axis, const gtf_column* cols, int32_t n_cols,
                      gtf_stream_t stream) {
    const char* who = "gtf_subset_gather";
    if (n_cols < 0) return bad("gtf_subset_gather: negative n_cols");
    if (axis != 0 && axis != 1) return bad("gtf_subset_gather: axis must be 0 (nodes) or 1 (slots)");
    if (n_cols == 0) return 0;
    if (!workspace) return bad("gtf_subset_gather: null workspace");
    if (!cols) return bad("gtf_subset_gather: null column table");
    for (int i = 0; i < n_cols; i++) {
        const gtf_column& c = cols[i];
        if (c.row_bytes <= 0) return bad("gtf_subset_gather: row_bytes must be at least 1");
        if (c.fill < GTF_COL_COPY || c.fill > GTF_COL_ZERO_ALL) return bad("gtf_subset_gather: unknown fill");
        if (!c.dst || (!c.src && c.fill != GTF_COL_ZERO_ALL)) return bad("gtf_subset_gather: null column pointer");
        if (c.fill == GTF_COL_NAN_ORPHAN && (c.row_bytes % 8 || ((uintptr_t)c.dst | (uintptr_t)c.src) % 8))
            return bad("gtf_subset_gather: GTF_COL_NAN_ORPHAN needs 8-byte aligned rows of a multiple of 8 bytes");
    }
    hipStream_t st = (hipStream_t)stream;
    for (int at = 0; at < n_cols; at += MAXC) {
        const int n = n_cols - at < MAXC ? n_cols - at : MAXC;
        ColTab tab;
        for (int i = 0; i < n; i++) {
            const gtf_column& c = cols[at + i];
            const uintptr_t bits = (uintptr_t)c.dst | (uintptr_t)c.src | (uintptr_t)c.row_bytes;
            const int lg = bits % 8 == 0 ? 3 : bits % 4 == 0 ? 2 : 0;
            tab.c[i].src = c.src;
            tab.c[i].dst = c.dst;
            tab.c[i].words = c.row_bytes >> lg;
            tab.c[i].mode = c.fill | (lg << 8);
        }
        for (int i = n; i < MAXC; i++) tab.c[i] = tab.c[0];
        // the row count is on the device: a fixed grid of about GATHER_BLOCKS blocks strides over the row tiles
        int gx = GATHER_BLOCKS / n;
        gx = gx < 64 ? 64 : gx > 1024 ? 1024 : gx;
        hipLaunchKernelGGL(k_gather, dim3(gx, n), dim3(BLOCK), 0, st, workspace, (int)axis, tab);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_refresh_send_mw(const gtf_graph* g, const int32_t* tse_rank, const double* tse_mw, double* send_mw,
                        gtf_stream_t stream) {
    const char* who = "gtf_refresh_send_mw";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (g->n_nodes < 0 || g->n_slots < 0) return bad("gtf_refresh_send_mw: negative sizes");
    const int32_t N = g->n_nodes, S = g->n_slots;
    if (S == 0) return 0;
    if (N == 0) return bad("gtf_refresh_send_mw: slots without nodes");
    if (!g->slot_ptr) return bad("gtf_refresh_send_mw: missing graph array slot_ptr");
    if (!g->slot_src) return bad("gtf_refresh_send_mw: missing graph array slot_src");
    if (!g->is_edge) return bad("gtf_refresh_send_mw: missing graph array is_edge");
    if (!tse_rank || !tse_mw || !send_mw) return bad("gtf_refresh_send_mw: missing array (tse_rank, tse_mw, send_mw)");
    if ((const void*)tse_mw == (const void*)send_mw) return bad("gtf_refresh_send_mw: send_mw aliases tse_mw");
    Send a;
    a.N = N; a.S = S;
    a.slot_ptr = g->slot_ptr; a.slot_src = g->slot_src; a.slot_dst = g->slot_dst; a.tse_rank = tse_rank;
    a.is_edge = g->is_edge; a.tse_mw = tse_mw; a.send_mw = send_mw;
    hipLaunchKernelGGL(k_send_mw, dim3(grid(S)), dim3(BLOCK), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

}  // extern "C"
