// gtf_build_dev.hip -- event conversion's graph build on the GPU ("CSV ->
// CSR directly" on the device): the same packed CSR, in the same networkx orders, as the
// host builder gtf_build_event_csr (gtf_build.cpp), from device arrays of the CSV columns.
//
// The reference (helper.construct_graph, helper.py:465-521; event_conversion.py:63-84)
// adds both directions of every edges.csv row to a networkx DiGraph, splits it into
// weakly connected components and copies each one; the orders that come out of that are
// what every later stage depends on. Here, as sorts, scans and per-segment threads:
//
//   1. node ids -> CSV index: radix sort of (id, index), binary search per row end;
//   2. G's successor lists in insertion order: both directions of row r at times 2r and
//      2r + 1, a stable radix sort by (u, v) keeps each pair's first time (networkx keeps
//      a repeated edge's first position), a second one by (u, time) gives succ[u] in
//      insertion order;
//   3. weakly connected components by hook + pointer jumping to the minimum CSV index
//      (= the node networkx's component loop starts from, so components come out in
//      root order);
//   4. node order of each component's copy: CSV-index order when 2|c| >= |G| (FilterAtlas
//      iterates G), else CPython 3.10 set order -- one thread per such component runs the
//      BFS (successors in insertion order; the graph is symmetric, so the predecessor
//      loop adds nothing) into a set table and copies it into a second one
//      (show_nodes(set(c))), exactly as gtf_build.cpp's PySet does, in global scratch;
//   5. slots: (packed receiver, packed sender) sorted, so each receiver's predecessors
//      come in copy node order; out-lists keep G's successor order; the
//      track_state_estimates key order reversed(set(chain(pred, succ))) (helper.py:277,
//      350-351) from one set table per node.
//
// Integer and byte work only: sorts and scans are hipCUB, the rest one thread per row /
// edge / node / component. Not on the timed path (once per event).
//
// A batch of events (gtf_build_events_csr_device) is the same build on the events' columns
// laid end to end: a graph whose components never cross an event boundary. Its sorts, scans,
// hook rounds, slot keys and out-lists run on global indices as they are and leave the arrays
// gtf/graph.py concat defines. There is one build: every kernel exists once, and the steps
// that know the event of what they handle -- the id -> CSV index map, sorted by (event, id)
// and searched inside the event's segment; the 2|c| >= |G| rule, with |G| the node count of
// the component's own event -- ask an Events value for it. One event is the Events without
// offset tables: event 0, the nodes [0, N), nothing read. What only a batch has is on the
// host side of build_csr: the offset upload, the second sort of the id map by event (from
// two events on), the event column and the event in the duplicate-id message.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_pyset.h"

namespace {

using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;

constexpr uint64_t NONE = ~uint64_t(0);
constexpr int32_t ERR_DUP = 1, ERR_RANGE = 2, ERR_ASYM = 4, ERR_OVER = 8;

// set_capacity, DevSet (CPython 3.10 set) and find_id_in (node id -> CSV index): gtf_pyset.h

// first position in [b, e) of slot_src holding >= x
__device__ inline int32_t lower(const int32_t* s, int32_t b, int32_t e, int32_t x) {
    return b + gtf::bound<false>(s + b, e - b, x);
}

__global__ void k_iota(int32_t* a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) a[i] = (int32_t)i;
}

// The events a kernel works on, by value. One event: K == 0 and no tables -- event 0, the nodes
// [0, n), nothing read (a branch every thread of a launch takes the same way). A batch: the K
// events' offsets on the node and the row axis, [K + 1] each, in the workspace.
struct Events {
    const int32_t* noff;
    const int32_t* roff;
    int32_t K;
    int32_t n;   // nodes of all events

    __device__ int32_t of_node(int32_t i) const { return K ? gtf::segment_of(noff, K, i) : 0; }
    __device__ int32_t of_row(int32_t r) const { return K ? gtf::segment_of(roff, K, r) : 0; }
    // the nodes [lo, hi) of event e: its segment of the id map, and its |G|
    __device__ void nodes(int32_t e, int32_t& lo, int32_t& hi) const {
        lo = K ? noff[e] : 0;
        hi = K ? noff[e + 1] : n;
    }
};

// ids in (event, id) order: event e's are positions [lo, hi) of ev.nodes(e). A repeated id is
// an error inside one event only; err[3] keeps the first such event.
__global__ void k_check_ids(const uint64_t* ids, int64_t n, Events ev, int32_t* err) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (ids[i] >= ((uint64_t)1 << 61) - 1) atomicOr(err, ERR_RANGE);   // also catches negatives
    if (i > 0 && ids[i] == ids[i - 1]) {
        const int32_t e = ev.of_node((int32_t)i);
        int32_t lo, hi;
        ev.nodes(e, lo, hi);
        if (i > lo) {
            atomicOr(err, ERR_DUP);
            atomicMin(err + 3, e);
        }
    }
}

// both directions of row r at times 2r (a -> b) and 2r + 1 (b -> a), both ends looked up among
// the nodes of the row's own event; rows naming a node outside the window are dropped
// (helper.py:512-518 adds edges between kept nodes only)
__global__ void k_rows(const int64_t* ra, const int64_t* rb, int64_t R, const uint64_t* ids, const int32_t* idx,
                       Events ev, uint64_t* key, int32_t* t) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= R) return;
    int32_t lo, hi;
    ev.nodes(ev.of_row((int32_t)r), lo, hi);
    const int32_t ia = find_id_in(ids, idx, lo, hi, ra[r]), ib = find_id_in(ids, idx, lo, hi, rb[r]);
    const bool ok = ia >= 0 && ib >= 0;
    key[2 * r] = ok ? ((uint64_t)ia << 32) | (uint32_t)ib : NONE;
    key[2 * r + 1] = ok ? ((uint64_t)ib << 32) | (uint32_t)ia : NONE;
    t[2 * r] = (int32_t)(2 * r);
    t[2 * r + 1] = (int32_t)(2 * r + 1);
}

// sorted by (u, v) with times ascending inside a pair: keep each pair's first insertion,
// re-keyed by (u, time) with v as the value
__global__ void k_first(const uint64_t* key, const int32_t* t, int64_t n, uint64_t* k2, int32_t* v2) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i];
    const bool keep = k != NONE && (i == 0 || key[i - 1] != k);
    k2[i] = keep ? ((k >> 32) << 33) | (uint32_t)t[i] : NONE;
    v2[i] = (int32_t)(k & 0xffffffffu);
}

__global__ void k_count_valid(const uint64_t* k, int64_t n, int32_t* m) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    // sorted: the valid keys form a prefix; its end is where NONE starts
    if (k[i] != NONE && (i + 1 == n || k[i + 1] == NONE)) *m = (int32_t)(i + 1);
}

__global__ void k_gdeg(const uint64_t* k, int32_t m, int32_t* deg) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < m) atomicAdd(&deg[k[i] >> 33], 1);
}

__global__ void k_lab_init(int32_t* lab, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) lab[i] = (int32_t)i;
}

// hook the larger root under the smaller one (labels only decrease, so every component
// ends labelled by its minimum CSV index)
__global__ void k_hook(const uint64_t* k, const int32_t* v, int32_t m, int32_t* lab, int32_t* changed) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int32_t a = lab[(int32_t)(k[i] >> 33)], b = lab[v[i]];
    if (a == b) return;
    atomicMin(&lab[a > b ? a : b], a < b ? a : b);
    *changed = 1;
}

__global__ void k_compress(int32_t* lab, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t l = lab[i];
    while (lab[l] != l) l = lab[l];
    lab[i] = l;
}

__global__ void k_isroot(const int32_t* lab, int64_t n, int32_t* isroot) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i <= n) isroot[i] = (i < n && lab[i] == i) ? 1 : 0;
}

__global__ void k_comp_of(const int32_t* lab, const int32_t* rank, int64_t n, int32_t* comp, int32_t* size,
                          uint64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t c = rank[lab[i]];
    comp[i] = c;
    key[i] = (uint64_t)c;
    atomicAdd(&size[c], 1);
}

// members of every component in CSV-index order (the stable sort by component): the copy's
// node order when 2|c| >= |G|. Written everywhere (k_comp_order then overwrites the components
// under half of their event), so `order` is a permutation whatever comes after.
__global__ void k_order_sorted(const int32_t* memb, int64_t n, int32_t* order) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < n) order[p] = memb[p];
}

// true when the component of `sz` nodes holding `member` keeps CSV order: at least half of its
// own event's nodes. `e`: that event.
__device__ inline bool csv_order(const Events& ev, int32_t member, int32_t sz, int32_t& e) {
    int32_t lo, hi;
    e = ev.of_node(member);
    ev.nodes(e, lo, hi);
    return 2 * (int64_t)sz >= (int64_t)(hi - lo);
}

__global__ void k_comp_words(const int32_t* size, const int32_t* coff, const int32_t* memb, int32_t n_sub, Events ev,
                             int64_t* words) {
    const int32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c > n_sub) return;
    int32_t e;
    words[c] = (c < n_sub && !csv_order(ev, memb[coff[c]], size[c], e)) ? 3 * set_capacity(size[c]) : 0;
}

// one thread per component smaller than half of its event: BFS from its root in successor
// order into set(...) (nx.weakly_connected_components: set(_plain_bfs(G, root))), then the
// copy's node order = the order of a second set filled from the first (show_nodes); the
// set's ids go back to CSV indices inside the event's segment of the map. The queue and the
// written order stay inside the component's `sz` entries whatever the arrays hold.
__global__ void k_comp_order(const int32_t* memb, const int32_t* coff, const int32_t* size, int32_t n_sub, Events ev,
                             const int32_t* gptr, const int32_t* gdst, const int64_t* node_id, const uint64_t* ids,
                             const int32_t* idx, const int64_t* toff, int64_t* tbl, int32_t* queue, uint8_t* seen,
                             int32_t* order, int32_t* err) {
    const int32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n_sub) return;
    const int32_t lo = coff[c], sz = size[c], root = memb[lo];
    int32_t e, elo, ehi;
    if (csv_order(ev, root, sz, e)) return;
    ev.nodes(e, elo, ehi);
    const int64_t cap = set_capacity(sz);
    int64_t* t = tbl + toff[c];
    DevSet s;
    s.init(t, t + cap, cap);
    int32_t head = lo, tail = lo;
    seen[root] = 1;
    s.add(node_id[root]);
    queue[tail++] = root;
    while (head < tail) {
        const int32_t v = queue[head++];
        for (int32_t j = gptr[v]; j < gptr[v + 1]; j++) {
            const int32_t w = gdst[j];
            if (!seen[w] && tail < lo + sz) {
                seen[w] = 1;
                s.add(node_id[w]);
                queue[tail++] = w;
            }
        }
    }
    DevSet shown;
    int64_t* spare = (s.a == t) ? t + cap : t;   // the first set's spare table
    shown.init(spare, t + 2 * cap, cap);
    for (int64_t i = 0; i <= s.mask; i++)
        if (s.a[i] >= 0) shown.add(s.a[i]);
    if (s.over || shown.over) { atomicOr(err, ERR_OVER); return; }
    int32_t r = lo;
    for (int64_t i = 0; i <= shown.mask; i++) {
        if (shown.a[i] < 0) continue;
        const int32_t g = find_id_in(ids, idx, elo, ehi, shown.a[i]);
        if (g >= 0 && r < lo + sz) order[r++] = g;
    }
}

__global__ void k_pos(const int32_t* order, const int32_t* comp, int64_t n, int32_t* pos, int32_t* sub_id) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    pos[order[p]] = (int32_t)p;
    sub_id[p] = comp[order[p]];
}

// every kept edge u -> v as (packed receiver, packed sender): sorted, each receiver's
// predecessors come in copy node order (the copy adds edges in its node order)
__global__ void k_slot_keys(const uint64_t* gkey, const int32_t* gdst, int32_t m, const int32_t* pos, uint64_t* sk,
                            int32_t* rdeg) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int32_t q = pos[gdst[i]], p = pos[(int32_t)(gkey[i] >> 33)];
    sk[i] = ((uint64_t)q << 32) | (uint32_t)p;
    atomicAdd(&rdeg[q], 1);
}

__global__ void k_slot_src(const uint64_t* sk, int32_t m, int32_t* slot_src) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < m) slot_src[i] = (int32_t)(sk[i] & 0xffffffffu);
}

__global__ void k_outdeg(const int32_t* order, const int32_t* gdeg, int64_t n, int32_t* od) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p <= n) od[p] = p < n ? gdeg[order[p]] : 0;
}

// out-list of packed sender p in G's successor order: the slot of p in each receiver; the
// write stays inside the `cap` entries of out_slot
__global__ void k_out_slot(const uint64_t* gkey, const int32_t* gdst, const int32_t* gptr, int32_t m,
                           const int32_t* pos, const int32_t* slot_ptr, const int32_t* slot_src,
                           const int32_t* out_ptr, int32_t* out_slot, int64_t cap) {
    const int32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int32_t u = (int32_t)(gkey[i] >> 33), p = pos[u], q = pos[gdst[i]];
    const int64_t at = (int64_t)out_ptr[p] + (i - gptr[u]);
    if (at >= 0 && at < cap) out_slot[at] = lower(slot_src, slot_ptr[q], slot_ptr[q + 1], p);
}

__global__ void k_tse_words(const int32_t* slot_ptr, int64_t n, int64_t* words) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p <= n) words[p] = p < n ? 2 * set_capacity(slot_ptr[p + 1] - slot_ptr[p]) : 0;
}

// track_state_estimates key order of packed node p: reversed(set(chain(pred, succ)))
// with the copy's predecessors (slot order) then G's successors, the keys looked up inside the
// node's own event. Slots outside the `cap_out` entries of tse_rank, or a key that is no node
// of the event, are ERR_ASYM.
__global__ void k_tse_rank(const int32_t* order, int64_t n, Events ev, const int32_t* slot_ptr,
                           const int32_t* slot_src, const int32_t* gptr, const int32_t* gdst, const int32_t* pos,
                           const int64_t* node_id, const uint64_t* ids, const int32_t* idx, const int64_t* toff,
                           int64_t* tbl, int32_t* tse_rank, int64_t cap_out, int32_t* err) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t b = slot_ptr[p], e = slot_ptr[p + 1], u = order[p];
    if (b < 0 || e < b || e > cap_out) { atomicOr(err, ERR_ASYM); return; }
    int32_t lo, hi;
    ev.nodes(ev.of_node(u), lo, hi);
    const int64_t cap = set_capacity(e - b);
    DevSet s;
    s.init(tbl + toff[p], tbl + toff[p] + cap, cap);
    for (int32_t k = b; k < e; k++) {
        s.add(node_id[order[slot_src[k]]]);
        tse_rank[k] = -1;
    }
    for (int32_t j = gptr[u]; j < gptr[u + 1]; j++) s.add(node_id[gdst[j]]);
    if (s.over) { atomicOr(err, ERR_OVER); return; }
    int32_t r = 0;
    for (int64_t i = s.mask; i >= 0; i--) {   // reversed iteration order
        if (s.a[i] < 0) continue;
        const int32_t g = find_id_in(ids, idx, lo, hi, s.a[i]);
        if (g < 0) { atomicOr(err, ERR_ASYM); return; }
        const int32_t q = pos[g];
        const int32_t f = lower(slot_src, b, e, q);
        if (f == e || slot_src[f] != q) { atomicOr(err, ERR_ASYM); return; }
        tse_rank[f] = r++;
    }
}

// ---- a batch of two events or more: the id map from id order to (event, id) order ----

// the ids come sorted by id with the CSV index each came from: the event of every entry, the
// key of the stable sort that makes it (event, id) order
__global__ void k_event_keys(const int32_t* idx, int64_t n, const int32_t* noff, int32_t K, uint64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) key[i] = (uint64_t)gtf::segment_of(noff, K, idx[i]);
}

__global__ void k_gather_ids(const int64_t* node_id, const int32_t* idx, int64_t n, uint64_t* ids) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) ids[i] = (uint64_t)node_id[idx[i]];
}

// components are ranked by their minimum global CSV index, so event e's packed nodes are the
// positions [noff[e], noff[e + 1]): the event column is a function of the position
__global__ void k_event_column(const int32_t* noff, int32_t K, int64_t n, int32_t* event) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < n) event[p] = gtf::segment_of(noff, K, (int32_t)p);
}

struct BuildWs {
    uint64_t *ids, *ka, *kb, *gk;
    int32_t *idx, *iota, *va, *vb, *gv;
    int32_t *gdeg, *gptr, *lab, *isroot, *rank, *comp, *size, *coff, *memb, *pos, *queue, *rdeg, *od;
    uint8_t* seen;
    int64_t *words, *toff, *tbl;
    int32_t* scal;   // [0] error bits, [1] changed, [2] valid edges, [3] the first event with a repeated id
    int32_t *noff, *roff;   // a batch: the events' node and row offsets, [K + 1] each
    gtf::Scratch cub;
    size_t tbl_words, total;
};

// capacity bound: a set of k distinct keys has a table of <= 8 max(k, 1) entries, so the
// component tables (3 per component) take <= 24 N words and the key-order tables (2 per
// node) <= 16 (S + N)
// K: the events of a batch, whose two offset tables follow the single event's layout (-1: none)
BuildWs carve(void* base, int64_t N, int64_t R, int64_t K = -1) {
    const int64_t E2 = 2 * R, M = N > E2 ? N : E2;
    const size_t n = (size_t)N, n1 = n + 1, m = (size_t)M, e2 = (size_t)(E2 > 0 ? E2 : 1);
    gtf::Arena a(base);
    BuildWs w;
    w.ids = a.take<uint64_t>(n);
    w.ka = a.take<uint64_t>(m);
    w.kb = a.take<uint64_t>(m);
    w.idx = a.take<int32_t>(n);
    w.iota = a.take<int32_t>(m);
    w.va = a.take<int32_t>(m);
    w.vb = a.take<int32_t>(m);
    w.gk = a.take<uint64_t>(e2);
    w.gv = a.take<int32_t>(e2);
    w.gdeg = a.take<int32_t>(n1);
    w.gptr = a.take<int32_t>(n1);
    w.lab = a.take<int32_t>(n1);
    w.isroot = a.take<int32_t>(n1);
    w.rank = a.take<int32_t>(n1);
    w.comp = a.take<int32_t>(n1);
    w.size = a.take<int32_t>(n1);
    w.coff = a.take<int32_t>(n1);
    w.memb = a.take<int32_t>(n1);
    w.pos = a.take<int32_t>(n1);
    w.queue = a.take<int32_t>(n1);
    w.rdeg = a.take<int32_t>(n1);
    w.od = a.take<int32_t>(n1);
    w.seen = a.take<uint8_t>(n1);
    w.words = a.take<int64_t>(n1);
    w.toff = a.take<int64_t>(n1);
    w.scal = a.take<int32_t>(16);
    const int c = (int)(m > n1 ? m : n1);
    gtf::CubNeed need;
    need.sort_pairs<uint64_t, int32_t>(c).sort_keys<uint64_t>(c).scan<int32_t>(c + 1).scan<int64_t>(c + 1);
    w.cub = need.take(a);
    const int64_t t1 = 24 * (N > 0 ? N : 1), t2 = 16 * (E2 + N + 1);
    w.tbl_words = (size_t)(t1 > t2 ? t1 : t2);
    w.tbl = a.take<int64_t>(w.tbl_words);
    w.noff = w.roff = nullptr;
    if (K >= 0) {
        w.noff = a.take<int32_t>((size_t)K + 1);
        w.roff = a.take<int32_t>((size_t)K + 1);
    }
    w.total = a.used() + 256;
    return w;
}

size_t carve_bytes(int64_t N, int64_t R, int64_t K = -1) { return carve(nullptr, N, R, K).total; }

// "who: what" as the error text, `rc` as the status
int say(int rc, const char* who, const char* what) {
    char m[256];
    snprintf(m, sizeof(m), "%s: %s", who, what);
    gtf::set_error(m);
    return rc;
}

// The build behind both entry points, their arguments checked. K == 0: one event, no offset
// tables. K > 0: a batch of K events whose offsets noff / roff (host arrays) go into the
// workspace first. Every launch, sort, scan and synchronisation after the id map is the same.
int build_csr(gtf_event_csr* ev, int32_t K, const int32_t* noff, const int32_t* roff, int32_t* event, const char* who,
              const BuildWs& w, hipStream_t st) {
    const int64_t N = ev->n_nodes, R = ev->n_rows, E2 = 2 * R;
    const gtf::Cub cub{w.cub, st};
    const Events evs{w.noff, w.roff, K, (int32_t)N};
    // a failure that is not a HIP call's: -1 with its own text
    auto broken = [who](const char* what) { return say(-1, who, what); };
    hipError_t e;
    const int32_t zero4[4] = {0, 0, 0, INT32_MAX};
    if ((e = hipMemcpyAsync(w.scal, zero4, sizeof(zero4), hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(who, "scalars", e);
    if (N == 0) {
        if ((e = hipMemsetAsync(ev->slot_ptr, 0, 4, st)) != hipSuccess) return fail(who, "memset", e);
        if ((e = hipMemsetAsync(ev->out_ptr, 0, 4, st)) != hipSuccess) return fail(who, "memset", e);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
        ev->n_edges = 0;
        ev->n_subgraphs = 0;
        return 0;
    }
    const int64_t M2 = N > E2 ? N : E2;
    // 1. ids -> CSV index
    hipLaunchKernelGGL(k_iota, dim3(grid(M2)), dim3(BLOCK), 0, st, w.iota, M2);
    if (K > 0 &&
        ((e = hipMemcpyAsync(w.noff, noff, 4 * ((size_t)K + 1), hipMemcpyHostToDevice, st)) != hipSuccess ||
         (e = hipMemcpyAsync(w.roff, roff, 4 * ((size_t)K + 1), hipMemcpyHostToDevice, st)) != hipSuccess))
        return fail(who, "offsets", e);
    // ids of different events collide and cannot be shifted apart (both set orders hash the id
    // itself): from two events on the id sort, then a stable sort by the event over the bits K
    // needs, leaves event e's ids ascending at [noff[e], noff[e + 1])
    const bool by_event = K > 1;
    if ((e = cub.sort_pairs((const uint64_t*)ev->node_id, by_event ? w.kb : w.ids, w.iota, by_event ? w.va : w.idx,
                            (int)N)) != hipSuccess)
        return fail(who, "sort ids", e);
    if (by_event) {
        int bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < K) bits++;
        hipLaunchKernelGGL(k_event_keys, dim3(grid(N)), dim3(BLOCK), 0, st, w.va, N, w.noff, K, w.ka);
        if ((e = cub.sort_pairs(w.ka, w.kb, w.va, w.idx, (int)N, bits)) != hipSuccess) return fail(who, "sort events", e);
        hipLaunchKernelGGL(k_gather_ids, dim3(grid(N)), dim3(BLOCK), 0, st, ev->node_id, w.idx, N, w.ids);
    }
    hipLaunchKernelGGL(k_check_ids, dim3(grid(N)), dim3(BLOCK), 0, st, w.ids, N, evs, w.scal);
    if (K > 0 && event) hipLaunchKernelGGL(k_event_column, dim3(grid(N)), dim3(BLOCK), 0, st, w.noff, K, N, event);
    // 2. G's successor lists in insertion order
    int32_t m = 0;
    if (R > 0) {
        hipLaunchKernelGGL(k_rows, dim3(grid(R)), dim3(BLOCK), 0, st, ev->row_a, ev->row_b, R, w.ids, w.idx, evs, w.ka,
                           w.va);
        if ((e = cub.sort_pairs(w.ka, w.kb, w.va, w.vb, (int)E2)) != hipSuccess) return fail(who, "sort pairs", e);
        hipLaunchKernelGGL(k_first, dim3(grid(E2)), dim3(BLOCK), 0, st, w.kb, w.vb, E2, w.ka, w.va);
        if ((e = cub.sort_pairs(w.ka, w.gk, w.va, w.gv, (int)E2)) != hipSuccess) return fail(who, "sort succ", e);
        hipLaunchKernelGGL(k_count_valid, dim3(grid(E2)), dim3(BLOCK), 0, st, w.gk, E2, w.scal + 2);
    }
    int32_t scal[4];
    if ((e = hipMemcpyAsync(scal, w.scal, sizeof(scal), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
    if (scal[0] & ERR_RANGE) return say(-2, who, "node ids must be in [0, 2^61 - 1)");
    if (scal[0] & ERR_DUP) {
        if (K == 0) return say(-2, who, "duplicate node id");
        char what[64];
        snprintf(what, sizeof(what), "duplicate node id in event %d", scal[3]);
        return say(-2, who, what);
    }
    m = scal[2];
    const uint64_t* gkey = w.gk;   // kept edges by (u, insertion time); value: v
    const int32_t* gdst = w.gv;
    if ((e = hipMemsetAsync(w.gdeg, 0, 4 * (N + 1), st)) != hipSuccess) return fail(who, "memset", e);
    if (m > 0) hipLaunchKernelGGL(k_gdeg, dim3(grid(m)), dim3(BLOCK), 0, st, gkey, m, w.gdeg);
    if ((e = cub.scan(w.gdeg, w.gptr, (int)N + 1)) != hipSuccess) return fail(who, "scan", e);
    // 3. weakly connected components, labelled by their minimum CSV index
    hipLaunchKernelGGL(k_lab_init, dim3(grid(N)), dim3(BLOCK), 0, st, w.lab, N);
    for (int round = 0; m > 0; round++) {
        if (round > 200) return broken("components did not converge");
        int32_t z = 0, changed = 0;
        if ((e = hipMemcpyAsync(w.scal + 1, &z, 4, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(who, "flag", e);
        hipLaunchKernelGGL(k_hook, dim3(grid(m)), dim3(BLOCK), 0, st, gkey, gdst, m, w.lab, w.scal + 1);
        hipLaunchKernelGGL(k_compress, dim3(grid(N)), dim3(BLOCK), 0, st, w.lab, N);
        if ((e = hipMemcpyAsync(&changed, w.scal + 1, 4, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return fail(who, "flag", e);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
        if (!changed) break;
    }
    hipLaunchKernelGGL(k_isroot, dim3(grid(N + 1)), dim3(BLOCK), 0, st, w.lab, N, w.isroot);
    if ((e = cub.scan(w.isroot, w.rank, (int)N + 1)) != hipSuccess) return fail(who, "scan", e);
    int32_t n_sub = 0;
    if ((e = hipMemcpyAsync(&n_sub, w.rank + N, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "read", e);
    if ((e = hipMemsetAsync(w.size, 0, 4 * (N + 1), st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_comp_of, dim3(grid(N)), dim3(BLOCK), 0, st, w.lab, w.rank, N, w.comp, w.size, w.ka);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
    if ((e = cub.scan(w.size, w.coff, n_sub + 1)) != hipSuccess) return fail(who, "scan", e);
    // 4. node order of every component's copy: CSV-index order (the stable sort by
    // component), replaced by the set order for components under half of their event (|G| of
    // the 2|c| >= |G| rule: the node count of the component's own event)
    if ((e = cub.sort_pairs(w.ka, w.kb, w.iota, w.memb, (int)N, 32)) != hipSuccess) return fail(who, "sort members", e);
    hipLaunchKernelGGL(k_order_sorted, dim3(grid(N)), dim3(BLOCK), 0, st, w.memb, N, ev->order);
    hipLaunchKernelGGL(k_comp_words, dim3(grid(n_sub + 1)), dim3(BLOCK), 0, st, w.size, w.coff, w.memb, n_sub, evs,
                       w.words);
    if ((e = cub.scan(w.words, w.toff, n_sub + 1)) != hipSuccess) return fail(who, "scan", e);
    int64_t words = 0;
    if ((e = hipMemcpyAsync(&words, w.toff + n_sub, 8, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
    if ((size_t)words > w.tbl_words) return broken("set tables exceed the workspace bound");
    if ((e = hipMemsetAsync(w.seen, 0, N, st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_comp_order, dim3(grid(n_sub)), dim3(BLOCK), 0, st, w.memb, w.coff, w.size, n_sub, evs, w.gptr,
                       gdst, ev->node_id, w.ids, w.idx, w.toff, w.tbl, w.queue, w.seen, ev->order, w.scal);
    hipLaunchKernelGGL(k_pos, dim3(grid(N)), dim3(BLOCK), 0, st, ev->order, w.comp, N, w.pos, ev->sub_id);
    // 5. slots: (packed receiver, packed sender) in order; the out-lists; the key orders
    if ((e = hipMemsetAsync(w.rdeg, 0, 4 * (N + 1), st)) != hipSuccess) return fail(who, "memset", e);
    if (m > 0) {
        hipLaunchKernelGGL(k_slot_keys, dim3(grid(m)), dim3(BLOCK), 0, st, gkey, gdst, m, w.pos, w.ka, w.rdeg);
        if ((e = cub.sort_keys(w.ka, w.kb, m)) != hipSuccess) return fail(who, "sort slots", e);
        hipLaunchKernelGGL(k_slot_src, dim3(grid(m)), dim3(BLOCK), 0, st, w.kb, m, ev->slot_src);
    }
    if ((e = cub.scan(w.rdeg, ev->slot_ptr, (int)N + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_outdeg, dim3(grid(N + 1)), dim3(BLOCK), 0, st, ev->order, w.gdeg, N, w.od);
    if ((e = cub.scan(w.od, ev->out_ptr, (int)N + 1)) != hipSuccess) return fail(who, "scan", e);
    if (m > 0)
        hipLaunchKernelGGL(k_out_slot, dim3(grid(m)), dim3(BLOCK), 0, st, gkey, gdst, w.gptr, m, w.pos, ev->slot_ptr,
                           ev->slot_src, ev->out_ptr, ev->out_slot, E2);
    hipLaunchKernelGGL(k_tse_words, dim3(grid(N + 1)), dim3(BLOCK), 0, st, ev->slot_ptr, N, w.words);
    if ((e = cub.scan(w.words, w.toff, (int)N + 1)) != hipSuccess) return fail(who, "scan", e);
    if ((e = hipMemcpyAsync(&words, w.toff + N, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
    if ((size_t)words > w.tbl_words) return broken("set tables exceed the workspace bound");
    hipLaunchKernelGGL(k_tse_rank, dim3(grid(N)), dim3(BLOCK), 0, st, ev->order, N, evs, ev->slot_ptr, ev->slot_src,
                       w.gptr, gdst, w.pos, ev->node_id, w.ids, w.idx, w.toff, w.tbl, ev->tse_rank, E2, w.scal);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    if ((e = hipMemcpyAsync(scal, w.scal, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "sync", e);
    if (scal[0] & ERR_OVER) return broken("a set held more keys than its table was sized for");
    if (scal[0] & ERR_ASYM) return broken("neighbour without an in-edge (graph not symmetric)");
    ev->n_edges = m;
    ev->n_subgraphs = n_sub;
    return 0;
}

}  // namespace

extern "C" {

size_t gtf_build_event_device_workspace_bytes(int64_t n_nodes, int64_t n_rows) {
    return carve_bytes(n_nodes > 0 ? n_nodes : 0, n_rows > 0 ? n_rows : 0);
}

int gtf_build_event_csr_device(gtf_event_csr* ev, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_build_event_csr_device";
    if (gtf::bad_event_csr(ev) || !workspace) return say(-2, who, "bad arguments");
    const int64_t N = ev->n_nodes, R = ev->n_rows;
    if (N > INT32_MAX / 2 || 2 * R > INT32_MAX / 2) return say(-2, who, "graph too large for int32 indices");
    if (workspace_bytes < carve_bytes(N, R))
        return say(-2, who, "workspace smaller than gtf_build_event_device_workspace_bytes");
    return build_csr(ev, 0, nullptr, nullptr, nullptr, who, carve(workspace, N, R), (hipStream_t)stream);
}

size_t gtf_build_events_device_workspace_bytes(int64_t n_nodes, int64_t n_rows, int32_t n_events) {
    return carve_bytes(n_nodes > 0 ? n_nodes : 0, n_rows > 0 ? n_rows : 0, n_events > 0 ? n_events : 0);
}

int gtf_build_events_csr_device(gtf_event_csr* ev, const gtf_event_batch* b, void* workspace, size_t workspace_bytes,
                                gtf_stream_t stream) {
    const char* who = "gtf_build_events_csr_device";
    if (const int rc = gtf::check_abi(b, who, "gtf_event_batch", "batch")) return rc;
    if (gtf::bad_event_csr(ev) || !workspace || b->n_events < 0 || !b->node_off || !b->row_off)
        return say(-2, who, "bad arguments");
    const int64_t N = ev->n_nodes, R = ev->n_rows;
    const int32_t K = b->n_events;
    if (N > INT32_MAX / 2 || 2 * R > INT32_MAX / 2) return say(-2, who, "batch too large for int32 indices");
    for (const int32_t* off : {b->node_off, b->row_off}) {
        if (off[0] != 0) return say(-2, who, "node_off and row_off start at 0");
        for (int32_t e = 0; e < K; e++)
            if (off[e + 1] < off[e]) return say(-2, who, "node_off and row_off may not decrease");
    }
    if (b->node_off[K] != N || b->row_off[K] != R)
        return say(-2, who, "node_off and row_off end at n_nodes and n_rows");
    if (workspace_bytes < carve_bytes(N, R, K))
        return say(-2, who, "workspace smaller than gtf_build_events_device_workspace_bytes");
    return build_csr(ev, K, b->node_off, b->row_off, b->event, who, carve(workspace, N, R, K), (hipStream_t)stream);
}

}  // extern "C"
