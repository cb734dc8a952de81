// gtf_prepare.hip -- the graph-static schedules and slot tables of gtf_graph on the GPU
// (gtf_graph_prepare, include/gtf.h): everything between the packed CSR and the kernels
// that gtf/device.py builds with NumPy (node_schedule, sched_segments, sender_schedule,
// sender_lanes, slot_classes, slot_static_words, slot_sender_xzr and the inline tables of
// DeviceGraph.__init__), array for array the same values, so a C caller reaches the
// lane-group kernels from the base fields alone.
//
//   1. schedules: every node gets a node class (slot count <= 2, 3..4, 5..6, 7..8, 9..12,
//      13..16, 17..32, 33..64, more) and, with an out-edge, a sender class (1..4, 5..8,
//      more out-edges). The schedules are the stable 9-way / 3-way partitions by class:
//      per-block class histograms (wave ballots), one hipCUB exclusive scan over the
//      class-major [12][blocks] histogram, then each node's position = its block's scanned
//      offset + the matching lanes below it in the block. The scan's class boundaries are
//      the counts n_g2 ... n_o16, copied to the host (the call's one synchronisation).
//   2. slot tables: one lane per slot in lane groups of 2/4/8/16/32/64 taken from the
//      schedule just written (a wavefront per node beyond 64 slots). A lane loads its
//      sender's layer and GNN x, z, r once; the class masks come from cross-lane
//      operations only -- position j's value is broadcast over the group and the equal
//      lanes balloted, the group's slice of the ballot is position j's class (== is
//      symmetric, so it is also the set of positions equal to j) -- Sum d^2 comparisons per
//      receiver without a d x d matrix in memory. slot_sxzr rows are exchanged by shuffle so
//      that each of the three store instructions writes one contiguous run per group.
//   3. out-edge tables: one thread per out-edge (its sender by binary search in out_ptr)
//      for out_dst / slot_outpos / slot_outidx, one thread per lane of the 4- and 8-lane
//      sender buckets for out_lanes.
//
// Integer work, comparisons and copies only (no arithmetic on the doubles). Once per graph,
// not on the timed path.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_host.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;   // 4 wavefronts
constexpr int WAVES = BLOCK / 64;
constexpr int NCLS = 9, SCLS = 3, CLS = NCLS + SCLS;   // node classes, then sender classes

struct Prep {
    int32_t N, S, E;
    const int32_t *slot_ptr, *slot_src, *out_ptr, *out_slot;
    const uint8_t *is_edge, *rev_edge;
    const double *gnn, *layer;
    // outputs (NULL = not written); sched / seg / slot_dst always point somewhere (the
    // caller's table or the workspace: the later kernels read them)
    int32_t *sched, *seg, *slot_dst, *out_sched, *out_lanes, *out_dst, *slot_outpos, *slot_outidx;
    double *slot_layer, *slot_sxzr;
    uint64_t *slot_class, *slot_xclass;
    uint8_t* slot_sflags;
    uint32_t* slot_static;
    // workspace
    int32_t *hist, *scan, *scal;
    int32_t nb;   // blocks of the per-node kernels
};

__device__ __forceinline__ int node_class(int d) {
    return d <= 2 ? 0 : d <= 4 ? 1 : d <= 6 ? 2 : d <= 8 ? 3 : d <= 12 ? 4 : d <= 16 ? 5 : d <= 32 ? 6 : d <= 64 ? 7 : 8;
}
__device__ __forceinline__ int sender_class(int od) { return od < 1 ? -1 : od <= 4 ? NCLS : od <= 8 ? NCLS + 1 : NCLS + 2; }

// the two classes of node v (sender class -1: no out-edge; both -1 past the last node)
__device__ __forceinline__ void classify(const Prep& a, int v, int& cn, int& cs) {
    cn = cs = -1;
    if (v < a.N) {
        cn = node_class(a.slot_ptr[v + 1] - a.slot_ptr[v]);
        cs = sender_class(a.out_ptr[v + 1] - a.out_ptr[v]);
    }
}

// 1a. class-major block histogram: hist[c * nb + b] = nodes of class c in block b
__global__ __launch_bounds__(BLOCK) void k_hist(Prep a) {
    __shared__ int32_t cnt[CLS][WAVES];
    const int v = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cn, cs;
    classify(a, v, cn, cs);
    for (int c = 0; c < CLS; c++) {
        const unsigned long long m = __ballot(c < NCLS ? cn == c : cs == c);
        if (lane == 0) cnt[c][w] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < CLS) {
        int s = 0;
        for (int q = 0; q < WAVES; q++) s += cnt[threadIdx.x][q];
        a.hist[threadIdx.x * a.nb + blockIdx.x] = s;
    }
    if (v == 0) a.hist[CLS * a.nb] = 0;   // the scan's last entry is then the total
}

// 1b. scatter: node v to the node schedule at (scanned offset of its class and block) + (the
// class's nodes below v in the block), the same for the sender schedule, whose positions
// start after the NCLS node classes (every node has one, so those hold exactly N)
__global__ __launch_bounds__(BLOCK) void k_scatter(Prep a) {
    __shared__ int32_t cnt[CLS][WAVES];
    const int v = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cn, cs;
    classify(a, v, cn, cs);
    const unsigned long long below = (1ull << lane) - 1;
    int rn = 0, rs = 0;
    for (int c = 0; c < CLS; c++) {
        const unsigned long long m = __ballot(c < NCLS ? cn == c : cs == c);
        if (lane == 0) cnt[c][w] = __popcll(m);
        if (c == cn) rn = __popcll(m & below);
        if (c == cs) rs = __popcll(m & below);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < CLS)   // the twelve class sizes, for the host
        a.scal[threadIdx.x] = a.scan[(threadIdx.x + 1) * a.nb] - a.scan[threadIdx.x * a.nb];
    if (v >= a.N) return;
    for (int q = 0; q < w; q++) rn += cnt[cn][q];
    const int pos = a.scan[cn * a.nb + blockIdx.x] + rn;
    if (pos >= 0 && pos < a.N) {
        a.sched[pos] = v;
        a.seg[2 * pos] = a.slot_ptr[v];
        a.seg[2 * pos + 1] = a.slot_ptr[v + 1];
    }
    if (cs >= 0 && a.out_sched) {
        for (int q = 0; q < w; q++) rs += cnt[cs][q];
        const int sp = a.scan[cs * a.nb + blockIdx.x] - a.scan[NCLS * a.nb] + rs;
        if (sp >= 0 && sp < a.N) {
            int32_t* q = a.out_sched + 4 * (int64_t)sp;
            q[0] = v;
            q[1] = a.out_ptr[v];
            q[2] = a.out_ptr[v + 1];
            q[3] = 0;
        }
    }
}

struct SlotVals {
    double lay, x, z, r;
};

// a slot's sender values: layer[src] and gnn[src][0, 2, 3]; NaN for an orphan key
__device__ __forceinline__ SlotVals load_slot(const Prep& a, bool on, int64_t k) {
    SlotVals s = {NAN, NAN, NAN, NAN};
    if (on) {
        const int src = a.slot_src[k];
        if (src >= 0 && src < a.N) {
            s.lay = a.layer[src];
            s.x = a.gnn[4 * (int64_t)src];
            s.z = a.gnn[4 * (int64_t)src + 2];
            s.r = a.gnn[4 * (int64_t)src + 3];
        }
    }
    return s;
}

// slot_sxzr rows of the d slots from `lo`, held one per lane from lane gbase: the 3 d doubles
// are one contiguous run, so lane i stores elements i, i + G, i + 2 G of it (fetched from the
// lane that holds the row) and each store instruction writes whole consecutive rows
template <int G>
__device__ __forceinline__ void store_xzr(double* out, int64_t lo, int d, int i, int gbase, const SlotVals& s) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int f = i + q * G, row = f / 3, c = f - 3 * row;
        const double vx = __shfl(s.x, gbase + row), vz = __shfl(s.z, gbase + row), vr = __shfl(s.r, gbase + row);
        if (f < 3 * d) out[3 * lo + f] = c == 0 ? vx : c == 1 ? vz : vr;
    }
}

// the per-slot tables that need no neighbour: receiver, sender layer, "no edge" defaults of
// the out-edge indices (k_edges overwrites the slots that have one)
__device__ __forceinline__ void store_plain(const Prep& a, int64_t k, int v, const SlotVals& s) {
    a.slot_dst[k] = v;
    if (a.slot_layer) a.slot_layer[k] = s.lay;
    if (a.slot_outpos) a.slot_outpos[k] = -1;
    if (a.slot_outidx) a.slot_outidx[k] = -1;
}

// 2a. `count` schedule entries from `first`, G lanes each (segments of <= G slots)
template <int G>
__global__ __launch_bounds__(BLOCK) void k_slots(Prep a, int first, int count) {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int ent = (int)(t / G), i = (int)(t % G);
    const int lane = threadIdx.x & 63, gbase = lane & ~(G - 1);
    int v = 0, lo = 0, d = 0;
    if (ent < count) {
        v = a.sched[first + ent];
        lo = a.seg[2 * (int64_t)(first + ent)];
        d = a.seg[2 * (int64_t)(first + ent) + 1] - lo;
        if (v < 0 || v >= a.N || lo < 0 || d < 0 || d > G || (int64_t)lo + d > a.S) d = 0;   // malformed CSR: nothing written
    }
    const bool on = i < d;
    const int64_t k = (int64_t)lo + i;
    const SlotVals s = load_slot(a, on, k);
    const bool sfl = on && s.x < a.gnn[4 * (int64_t)v];   // false for an orphan (NaN)
    if (on) store_plain(a, k, v, s);
    if (a.slot_sxzr) store_xzr<G>(a.slot_sxzr, lo, d, i, gbase, s);
    if (!a.slot_class) return;   // (wave-uniform: the three class tables come together)
    // classes: broadcast position j's values, ballot the equal lanes; lane j keeps its group's
    // slice. A lane always equals itself (a NaN: only itself); -0.0 == 0.0.
    constexpr unsigned long long GM = G == 64 ? ~0ull : (1ull << (G & 63)) - 1;
    unsigned long long lm = 0, xm = 0;
    for (int j = 0; j < G; j++) {
        const double lj = __shfl(s.lay, gbase + j), xj = __shfl(s.x, gbase + j);
        const unsigned long long bl = __ballot(on && (s.lay == lj || i == j));
        const unsigned long long bx = __ballot(on && (s.x == xj || i == j));
        if (i == j) {
            lm = (bl >> gbase) & GM;
            xm = (bx >> gbase) & GM;
        }
    }
    if (!on) return;
    const unsigned long long cls = d <= 32 ? (lm | (xm << 32)) : lm;
    a.slot_class[k] = cls;
    a.slot_xclass[k] = d <= 32 ? 0ull : xm;
    a.slot_sflags[k] = sfl ? 1 : 0;
    if (a.slot_static) {
        uint32_t w = 0;
        if (d <= 8)
            w = (uint32_t)(cls & 0xff) | ((uint32_t)((cls >> 32) & 0xff) << 8) | ((uint32_t)(a.is_edge[k] & 1) << 16) |
                ((uint32_t)(a.rev_edge[k] & 1) << 17) | ((uint32_t)sfl << 18);
        a.slot_static[k] = w;
    }
}

// 2b. the nodes beyond 64 slots: one wavefront per node, 64 slots a step; their classes are 0
// (the node kernel builds them)
__global__ __launch_bounds__(BLOCK) void k_slots_big(Prep a, int first, int count) {
    const int ent = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ent >= count) return;   // (whole wavefronts)
    const int v = a.sched[first + ent];
    const int lo = a.seg[2 * (int64_t)(first + ent)], hi = a.seg[2 * (int64_t)(first + ent) + 1];
    if (v < 0 || v >= a.N || lo < 0 || hi < lo || hi > a.S) return;
    const double rx = a.gnn[4 * (int64_t)v];
    for (int base = lo; base < hi; base += 64) {
        const int d = hi - base < 64 ? hi - base : 64;
        const bool on = lane < d;
        const int64_t k = (int64_t)base + lane;
        const SlotVals s = load_slot(a, on, k);
        if (on) store_plain(a, k, v, s);
        if (a.slot_sxzr) store_xzr<64>(a.slot_sxzr, base, d, lane, 0, s);
        if (on && a.slot_class) {
            a.slot_class[k] = 0;
            a.slot_xclass[k] = 0;
            a.slot_sflags[k] = s.x < rx ? 1 : 0;
            if (a.slot_static) a.slot_static[k] = 0;
        }
    }
}

// 3a. out-edge o of sender u (out_ptr[u] <= o < out_ptr[u + 1], binary search): its receiver,
// and its slot's position in u's out-list / global out-edge index
__global__ __launch_bounds__(BLOCK) void k_edges(Prep a) {
    const int o = blockIdx.x * BLOCK + threadIdx.x;
    if (o >= a.E) return;
    const int k = a.out_slot[o];
    if (k < 0 || k >= a.S) return;
    if (a.out_dst) a.out_dst[o] = a.slot_dst[k];
    if (a.slot_outidx) a.slot_outidx[k] = o;
    if (a.slot_outpos) {
        int lo = 0, hi = a.N - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (a.out_ptr[mid + 1] <= o) lo = mid + 1;
            else hi = mid;
        }
        a.slot_outpos[k] = o - a.out_ptr[lo];
    }
}

// 3b. lane l of entry e of the sender schedule's 4- and 8-lane buckets: (slot, receiver) of
// out-edge out_ptr[sender] + l, (-1, 0) past the sender's last one
__global__ __launch_bounds__(BLOCK) void k_lanes(Prep a, int n_o4, int n_o8) {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= 4 * (int64_t)n_o4 + 8 * (int64_t)n_o8) return;
    int e, l;
    if (t < 4 * (int64_t)n_o4) {
        e = (int)(t >> 2);
        l = (int)(t & 3);
    } else {
        const int64_t r = t - 4 * (int64_t)n_o4;
        e = n_o4 + (int)(r >> 3);
        l = (int)(r & 7);
    }
    const int32_t begin = a.out_sched[4 * (int64_t)e + 1], end = a.out_sched[4 * (int64_t)e + 2];
    int32_t slot = -1, dst = 0;
    const int64_t o = (int64_t)begin + l;
    if (begin >= 0 && o < end && o < a.E) {
        const int k = a.out_slot[o];
        if (k >= 0 && k < a.S) {
            slot = k;
            dst = a.slot_dst[k];
        }
    }
    a.out_lanes[2 * t] = slot;
    a.out_lanes[2 * t + 1] = dst;
}

struct PrepWs {
    int32_t *hist, *scan, *scal, *sched, *seg, *slot_dst;
    gtf::Scratch cub;
    size_t total;
    int32_t nb;
};

PrepWs carve(void* base, int64_t N, int64_t S) {
    PrepWs w;
    gtf::Arena a(base);
    w.nb = (int32_t)((N + BLOCK - 1) / BLOCK);
    const size_t m = (size_t)CLS * (size_t)w.nb + 1;
    w.hist = a.take<int32_t>(m);
    w.scan = a.take<int32_t>(m);
    w.scal = a.take<int32_t>(16);
    w.sched = a.take<int32_t>((size_t)N);       // used when the caller asks for no sched / sched_seg /
    w.seg = a.take<int32_t>(2 * (size_t)N);     // slot_dst: the slot and out-edge kernels read them
    w.slot_dst = a.take<int32_t>((size_t)S);
    w.cub = gtf::CubNeed().scan<int32_t>((int)m).take(a);
    w.total = a.used();
    return w;
}

template <int G>
void launch_slots(const Prep& a, int first, int count, hipStream_t st) {
    if (count > 0)
        hipLaunchKernelGGL(k_slots<G>, dim3(grid((int64_t)count * G)), dim3(BLOCK), 0, st, a, first, count);
}

}  // namespace

extern "C" {

size_t gtf_graph_prepare_workspace_bytes(int32_t n_nodes, int32_t n_slots, int32_t n_edges) {
    (void)n_edges;   // (no per-edge scratch; kept in the signature for later layouts)
    return carve(nullptr, n_nodes > 0 ? n_nodes : 0, n_slots > 0 ? n_slots : 0).total;
}

int gtf_graph_prepare(gtf_graph* g, const gtf_graph_tables* t, void* workspace, size_t workspace_bytes,
                      gtf_stream_t stream) {
    const char* who = "gtf_graph_prepare";
    if (int rc = gtf::check_abi(g, who)) return rc;
    if (g->n_nodes < 0 || g->n_slots < 0 || g->n_edges < 0) return bad("gtf_graph_prepare: negative sizes");
    const int32_t N = g->n_nodes, S = g->n_slots, E = g->n_edges;
    if (!t) return bad("gtf_graph_prepare: null gtf_graph_tables");
    if ((N > 0 && (!g->slot_ptr || !g->out_ptr)) ||
        (S > 0 && (!g->slot_src || !g->is_edge || !g->rev_edge || !g->gnn || !g->layer)) || (E > 0 && !g->out_slot))
        return bad("gtf_graph_prepare: missing graph arrays (slot_ptr, slot_src, out_ptr, out_slot, is_edge, "
                   "rev_edge, gnn, layer)");
    if ((S > 0 || E > 0) && N == 0) return bad("gtf_graph_prepare: slots or edges without nodes");
    if (!workspace || workspace_bytes < gtf_graph_prepare_workspace_bytes(N, S, E))
        return bad("gtf_graph_prepare: workspace smaller than gtf_graph_prepare_workspace_bytes");

    // which tables come out (include/gtf.h: the dependent ones follow)
    const bool cls = t->slot_class && t->slot_sflags && t->slot_xclass;
    const bool empty = N == 0 || (S == 0 && E == 0);
    Prep a;
    a.N = N; a.S = S; a.E = E;
    a.slot_ptr = g->slot_ptr; a.slot_src = g->slot_src; a.out_ptr = g->out_ptr; a.out_slot = g->out_slot;
    a.is_edge = g->is_edge; a.rev_edge = g->rev_edge; a.gnn = g->gnn; a.layer = g->layer;
    const PrepWs w = carve(workspace, N, S);
    a.hist = w.hist; a.scan = w.scan; a.scal = w.scal; a.nb = w.nb;
    int32_t* const sched = empty ? nullptr : t->sched;
    int32_t* const seg = sched ? t->sched_seg : nullptr;
    int32_t* const osched = empty ? nullptr : t->out_sched;
    a.sched = sched ? sched : w.sched;
    a.seg = seg ? seg : w.seg;
    a.slot_dst = t->slot_dst ? t->slot_dst : w.slot_dst;
    a.out_sched = osched;
    a.out_lanes = osched ? t->out_lanes : nullptr;
    a.out_dst = empty ? nullptr : t->out_dst;
    a.slot_outpos = empty ? nullptr : t->slot_outpos;
    a.slot_outidx = empty ? nullptr : t->slot_outidx;
    a.slot_layer = empty ? nullptr : t->slot_layer;
    a.slot_sxzr = empty ? nullptr : t->slot_sxzr;
    a.slot_class = cls && !empty ? t->slot_class : nullptr;
    a.slot_sflags = a.slot_class ? t->slot_sflags : nullptr;
    a.slot_xclass = a.slot_class ? t->slot_xclass : nullptr;
    a.slot_static = a.slot_class ? t->slot_static : nullptr;

    int32_t c[CLS] = {0};
    if (!empty) {
        hipStream_t st = (hipStream_t)stream;
        const gtf::Cub cub{w.cub, st};
        hipError_t e;
        // 1. the schedules, and their class sizes to the host
        hipLaunchKernelGGL(k_hist, dim3(a.nb), dim3(BLOCK), 0, st, a);
        if ((e = cub.scan(a.hist, a.scan, CLS * a.nb + 1)) != hipSuccess) return fail(who, "scan", e);
        hipLaunchKernelGGL(k_scatter, dim3(a.nb), dim3(BLOCK), 0, st, a);
        if ((e = hipMemcpyAsync(c, a.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return fail(who, "counts", e);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
        int64_t nodes = 0;
        for (int q = 0; q < CLS; q++) {
            if (c[q] < 0 || c[q] > N) return bad("gtf_graph_prepare: inconsistent slot_ptr / out_ptr");
            if (q < NCLS) nodes += c[q];
        }
        if (nodes != N) return bad("gtf_graph_prepare: inconsistent slot_ptr / out_ptr");
        // 2. the slot tables, one launch per lane-group width over its schedule range
        if (S > 0) {
            int at = 0;
            launch_slots<2>(a, at, c[0], st); at += c[0];
            launch_slots<4>(a, at, c[1], st); at += c[1];
            launch_slots<8>(a, at, c[2] + c[3], st); at += c[2] + c[3];
            launch_slots<16>(a, at, c[4] + c[5], st); at += c[4] + c[5];
            launch_slots<32>(a, at, c[6], st); at += c[6];
            launch_slots<64>(a, at, c[7], st); at += c[7];
            if (c[8] > 0)
                hipLaunchKernelGGL(k_slots_big, dim3((c[8] + WAVES - 1) / WAVES), dim3(BLOCK), 0, st, a, at, c[8]);
        }
        // 3. the out-edge tables (after the slot kernels: they read slot_dst and overwrite the -1s)
        if (E > 0 && (a.out_dst || a.slot_outpos || a.slot_outidx))
            hipLaunchKernelGGL(k_edges, dim3(grid(E)), dim3(BLOCK), 0, st, a);
        const int64_t lanes = 4 * (int64_t)c[NCLS] + 8 * (int64_t)c[NCLS + 1];
        if (a.out_lanes && lanes > 0)
            hipLaunchKernelGGL(k_lanes, dim3(grid(lanes)), dim3(BLOCK), 0, st, a, c[NCLS], c[NCLS + 1]);
        if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    }

    // the written tables and the counts into *g; a table not asked for leaves its optional field NULL
    // (slot_dst and slot_outpos, which gtf_pass requires, stay the caller's when not asked for)
    if (!empty && t->slot_dst) g->slot_dst = t->slot_dst;
    if (a.slot_outpos) g->slot_outpos = a.slot_outpos;
    g->out_dst = a.out_dst;
    g->slot_layer = a.slot_layer;
    g->slot_outidx = a.slot_outidx;
    g->slot_class = a.slot_class;
    g->slot_sflags = a.slot_sflags;
    g->slot_xclass = a.slot_xclass;
    g->slot_sxzr = a.slot_sxzr;
    g->slot_static = a.slot_static;
    g->sched = sched;
    g->sched_seg = seg;
    g->out_sched = osched;
    g->out_lanes = a.out_lanes;
    const bool ns = sched != nullptr, os = osched != nullptr;
    g->n_g2 = ns ? c[0] : 0;
    g->n_g4 = ns ? c[0] + c[1] : 0;
    g->n_g6 = ns ? c[2] : 0;
    g->n_g8 = ns ? c[2] + c[3] : 0;
    g->n_g12 = ns ? c[4] : 0;
    g->n_g16 = ns ? c[4] + c[5] : 0;
    g->n_g32 = ns ? c[6] : 0;
    g->n_g64 = ns ? c[7] : 0;
    g->n_big = ns ? c[8] : 0;
    g->n_o4 = os ? c[NCLS] : 0;
    g->n_o8 = os ? c[NCLS + 1] : 0;
    g->n_o16 = os ? c[NCLS + 2] : 0;
    return 0;
}

}  // extern "C"
