// gtf_truth.hip -- the scorer's static truth tables on the GPU, for one event (include/gtf.h:
// gtf_truth_build) and for a batch of K events in one call (gtf_truth_build_ev).
//
// One event: gtf/metrics.py truth_tables (src/extract/reconstruction_efficiency.py:41-91 the
// reference tracks, utilities/helper.py:466-479 hit_dissociation) from the parsed columns of the
// hit mapping, the truth file and the particles file, as device arrays; the six arrays it writes
// are array_equal to the host function's. A batch: gtf/metrics.py truth_tables_batch, which is
// concat_tables of the K truth_tables; what it leaves is what gtf_truth_concat of K
// gtf_truth_build results leaves, word for word, in a number of launches that does not depend on
// K. Every kernel exists once: where the batch differs, the kernel takes the compile-time flag EV
// and the one-event instantiation pays nothing for events.
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
// The batch runs these steps on global indices over the K events' columns laid end to end. What
// learns about events:
//
//   events    0. one int32 event column per axis (particles, truth rows, mapping rows): a search
//                over the K + 1 offsets, which are uploaded once in stream order. The "truth
//                rows" are the effective ones: an event without truth columns of its own
//                contributes its mapping's hit_id / particle_id, so their offsets are an
//                exclusive sum made on the device
//   sorts        ids of different events collide (the same event twice is the plain case) and
//                cannot be shifted (arbitrary int64), so every sorted table is ordered by
//                (event, key): the 64-bit key sort, then one stable radix pass over the bits K
//                needs on the event word of each element, and a gather. The input is event-major
//                and both passes are stable, so event e's elements occupy [off[e], off[e + 1])
//                of every sorted order. At K == 1 the second pass is skipped
//   lookups      a truth row's particle is searched in its event's segment of the sorted
//                particles, a mapping row's hit in its event's segment of the sorted truth rows;
//                the prefix sums stay global and only differences inside a segment are taken
//   heads        a particle head, a node head and a (hit, node) head also break where the event
//                column changes
//   offsets      part_off[e], node_off[e] and entry_off[e] are the exclusive sums of the packed
//                marks read at row_off[e]; node_ptr[t] is the global entry index;
//                n_reference[e] is a difference of the exclusive sum of part_ref at part_off
//
// No atomic but the error words' (one for the event, one per event of a batch), which are
// touched only when the input is broken. Vector stores only. One synchronisation, for the counts
// and the error words.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_search.h"

namespace {

using gtf::bad;
using gtf::bound;
using gtf::fail;
using gtf::flip;
using gtf::grid;
using gtf::hi32;
using gtf::index_or0;
using gtf::lo32;
using gtf::unflip;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int64_t MAX_ROWS = int64_t(1) << 30;
constexpr uint64_t SIGN = uint64_t(1) << 63;
constexpr int ID_BITS = 21;                       // volume, layer, module: [0, 2^21)
constexpr int64_t ID_LIMIT = int64_t(1) << ID_BITS;
enum { S_T = 0, S_P, S_R, S_REF, S_ERR, S_WORDS };   // one event: the words brought back
constexpr int CNT_WORDS = sizeof(gtf_truth_counts) / 4;
static_assert(sizeof(gtf_truth_counts) == 24, "k_counts writes gtf_truth_counts as six words");

// ev: carved by carve<true> alone. In the one-event instantiation these pointers are null and
// only code under `if constexpr (EV)` (and the batch-only kernels) may read them.
struct Ws {
    int32_t* scal;                    // [S_WORDS] one event's counts
    int32_t *roff, *toff, *poff;      // ev [K + 1] the caller's offsets
    int32_t *tsz, *eoff;              // ev [K + 1] effective truth rows per event; their exclusive sum
    uint32_t* err;                    // GTF_TRUTH_ERR_*: ev [K] per event; one event: scal[S_ERR]
    int32_t* cnt;                     // ev [K] gtf_truth_counts
    int32_t *evp, *evt, *evr;         // ev [NP], [NT], [N] the event of a particle, truth row, mapping row
    uint64_t *ka, *kb, *kc;           // [M + 1] sort keys
    int32_t *va, *vb, *vc;            // [M + 1] sort values
    uint64_t* tmpk;                   // ev [M + 1] the (event, key) sort: the key-sorted keys,
    int32_t* tmpv;                    //            values,
    uint32_t *ek, *ek2;               //            event words, in and out,
    int32_t *epos, *eperm;            //            positions, in and out
    uint64_t* pk;                     // [NP + 1] particle ids, sorted by (event, id)
    int32_t *pidx, *pflag;            // ev [NP + 1] the particle; its high-pT flag by row
    int32_t *pf, *ps;                 // [NP + 1] the flag, sorted; summed
    uint64_t* tk;                     // [NT + 1] truth hit ids, sorted by (event, hit)
    int32_t *tidx, *tflag, *tfs, *ts; // [NT + 1] the truth row; its flag by row; sorted; summed
    int64_t* tpart;                   // ev [NT] the truth row's particle
    int64_t* row_part;                // [N] the particle of the row's hit (its first truth row)
    uint8_t* sel;                     // [N] region row
    int64_t *in_a, *in_b, *sum_a, *sum_b;   // [N + 1] packed marks and their exclusive sums
    int32_t *pos, *ref;               // [N + 1] position of particle r's head; its reference flag
    int32_t* refsum;                  // ev [N + 1] the reference flags summed
    gtf::Scratch cub;
    size_t total;
};

// NT: the bound of the effective truth rows
template <bool EV>
Ws carve(void* base, int64_t N, int64_t NT, int64_t NP, int64_t K) {
    Ws w = {};
    gtf::Arena a(base);
    const size_t m = (size_t)(N > NT ? (N > NP ? N : NP) : (NT > NP ? NT : NP)) + 1;
    const size_t n = (size_t)N, n1 = n + 1, t1 = (size_t)NT + 1, p1 = (size_t)NP + 1, k1 = (size_t)K + 1;
    if constexpr (EV) {
        w.roff = a.take<int32_t>(k1);
        w.toff = a.take<int32_t>(k1);
        w.poff = a.take<int32_t>(k1);
        w.tsz = a.take<int32_t>(k1);
        w.eoff = a.take<int32_t>(k1);
        w.err = a.take<uint32_t>(k1);
        w.cnt = a.take<int32_t>(k1 * CNT_WORDS);
        w.evp = a.take<int32_t>(p1);
        w.evt = a.take<int32_t>(t1);
        w.evr = a.take<int32_t>(n1);
    } else {
        w.scal = a.take<int32_t>(16);
        w.err = (uint32_t*)w.scal + S_ERR;
    }
    w.ka = a.take<uint64_t>(m);
    w.kb = a.take<uint64_t>(m);
    w.kc = a.take<uint64_t>(m);
    w.va = a.take<int32_t>(m);
    w.vb = a.take<int32_t>(m);
    w.vc = a.take<int32_t>(m);
    if constexpr (EV) {
        w.tmpk = a.take<uint64_t>(m);
        w.tmpv = a.take<int32_t>(m);
        w.ek = a.take<uint32_t>(m);
        w.ek2 = a.take<uint32_t>(m);
        w.epos = a.take<int32_t>(m);
        w.eperm = a.take<int32_t>(m);
    }
    w.pk = a.take<uint64_t>(p1);
    if constexpr (EV) {
        w.pidx = a.take<int32_t>(p1);
        w.pflag = a.take<int32_t>(p1);
    }
    w.pf = a.take<int32_t>(p1);
    w.ps = a.take<int32_t>(p1);
    w.tk = a.take<uint64_t>(t1);
    w.tidx = a.take<int32_t>(t1);
    w.tflag = a.take<int32_t>(t1);
    w.tfs = a.take<int32_t>(t1);
    w.ts = a.take<int32_t>(t1);
    if constexpr (EV) w.tpart = a.take<int64_t>(t1);
    w.row_part = a.take<int64_t>(n);
    w.sel = a.take<uint8_t>(n);
    w.in_a = a.take<int64_t>(n1);
    w.in_b = a.take<int64_t>(n1);
    w.sum_a = a.take<int64_t>(n1);
    w.sum_b = a.take<int64_t>(n1);
    w.pos = a.take<int32_t>(n1);
    w.ref = a.take<int32_t>(n1);
    if constexpr (EV) {
        w.refsum = a.take<int32_t>(n1);
        const size_t big = m > k1 ? m : k1;
        const int mi = big > (size_t)INT32_MAX ? INT32_MAX : (int)big;
        w.cub = gtf::CubNeed().sort_pairs<uint64_t, int32_t>(mi).sort_pairs<uint32_t, int32_t>(mi).scan<int64_t>(mi)
                    .scan<int32_t>(mi).take(a);
    } else {
        const int mi = (int)m;
        w.cub = gtf::CubNeed().sort_pairs<uint64_t, int32_t>(mi).scan<int64_t>(mi).scan<int32_t>(mi).sum<int32_t>(mi).take(a);
    }
    w.total = a.used();
    return w;
}

// One event: K is 1 and unused, o has no offset arrays (null), w has no ev pieces (null).
struct Build {
    int32_t K, N, NT, NP, num_layers, min_volume, max_volume;
    double pt_cut;
    const int64_t *node, *hit, *pid, *vol, *lay, *mod;
    // the truth columns: of one event, the mapping's own hit / pid when none are given; of a
    // batch, the separate ones at the caller's truth_off
    const int64_t *th, *tp;
    const int64_t* part_id;
    const double *px, *py;
    gtf_truth_batch_buf o;            // (one event: no offsets)
    Ws w;
};

// ---- 0. the events ----
// the effective truth rows of every event: its own, or its mapping rows where it brings none
__global__ __launch_bounds__(BLOCK) void k_truth_sizes(Build a) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e > a.K) return;
    int n = 0;
    if (e < a.K) {
        n = a.w.toff[e + 1] - a.w.toff[e];
        if (n <= 0) n = a.w.roff[e + 1] - a.w.roff[e];
    }
    a.w.tsz[e] = n;
}

__global__ __launch_bounds__(BLOCK) void k_events(Build a) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j < a.NP) a.w.evp[j] = gtf::segment_of(a.w.poff, a.K, j);
    if (j < a.NT) a.w.evt[j] = gtf::segment_of(a.w.eoff, a.K, j);
    if (j < a.N) a.w.evr[j] = gtf::segment_of(a.w.roff, a.K, j);
}

// the (event, key) sort's second pass: the event word of each key-sorted element, and its position
__global__ __launch_bounds__(BLOCK) void k_event_keys(const int32_t* v, int n, const int32_t* ev, uint32_t* ek,
                                                      int32_t* epos) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ek[i] = (uint32_t)ev[index_or0(v[i], n)];
    epos[i] = i;
}

__global__ __launch_bounds__(BLOCK) void k_permute(const uint64_t* k, const int32_t* v, const int32_t* perm, int n,
                                                   uint64_t* kout, int32_t* vout) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int p = index_or0(perm[i], n);
    kout[i] = k[p];
    vout[i] = v[p];
}

// ---- 1. the particles: id and high-pT flag (reconstruction_efficiency.py:44-47) ----
// One event: the flag is the sort's value. A batch: the particle is, and k_particles_sorted
// gathers the flags (the second sort pass moves values, not flags).
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_particles(Build a) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= a.NP) return;
    const double x = a.px[j], y = a.py[j];
    // np.sqrt(px ** 2 + py ** 2): two rounded products, a rounded sum (-ffp-contract=off), the
    // correctly rounded root
    const double pt = __dsqrt_rn(x * x + y * y);
    const int flag = pt >= a.pt_cut ? 1 : 0;
    a.w.ka[j] = flip(a.part_id[j]);
    if constexpr (EV) {
        a.w.va[j] = j;
        a.w.pflag[j] = flag;
    } else {
        a.w.va[j] = flag;
    }
}

__global__ __launch_bounds__(BLOCK) void k_particles_sorted(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.NP) return;
    a.w.pf[i] = a.w.pflag[index_or0(a.w.pidx[i], a.NP)];
}

// ---- 2. the truth rows: is the row's particle a high-pT one of its event; the keys of the sort by hit ----
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_truth_rows(Build a) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= a.NT) return;
    int64_t hit, part;
    int b = 0, end = a.NP;                                  // its event's segment of the sorted particles
    if constexpr (EV) {
        const int e = a.w.evt[j];
        const int k = j - a.w.eoff[e];                      // the row inside its event
        const int t0 = a.w.toff[e], own = a.w.toff[e + 1] - t0;
        if (own > 0) {                                      // truth columns of its own
            const int s = t0 + index_or0(k, own);
            hit = a.th[s];
            part = a.tp[s];
        } else {                                            // the mapping's hit_id / particle_id
            const int s = index_or0(a.w.roff[e] + k, a.N);
            hit = a.hit[s];
            part = a.pid[s];
        }
        gtf::segment(a.w.poff, e, a.NP, b, end);
        a.w.tpart[j] = part;
    } else {
        hit = a.th[j];
        part = a.tp[j];
    }
    const uint64_t id = flip(part);
    const int lb = b + bound<false>(a.w.pk + b, end - b, id), ub = b + bound<true>(a.w.pk + b, end - b, id);
    a.w.tflag[j] = ub > lb && a.w.ps[ub] - a.w.ps[lb] > 0;
    a.w.ka[j] = flip(hit);
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
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_rows(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    int e = 0, b = 0, end = a.NT;                           // its event; the event's segment of the sorted truth rows
    if constexpr (EV) {
        e = a.w.evr[i];
        gtf::segment(a.w.eoff, e, a.NT, b, end);
    }
    const uint64_t h = flip(a.hit[i]);
    const int lb = b + bound<false>(a.w.tk + b, end - b, h), ub = b + bound<true>(a.w.tk + b, end - b, h);
    const bool found = ub > lb;
    int64_t part = 0;
    if (found) {
        const int j = a.w.tidx[lb];
        if (j >= 0 && j < a.NT) part = EV ? a.w.tpart[j] : a.tp[j];
    } else {
        atomicOr(&a.w.err[e], GTF_TRUTH_ERR_MISSING);   // (only on a violation)
    }
    const int64_t v = a.vol[i], l = a.lay[i], m = a.mod[i];
    const bool in_range = v >= 0 && v < ID_LIMIT && l >= 0 && l < ID_LIMIT && m >= 0 && m < ID_LIMIT;
    if (!in_range) atomicOr(&a.w.err[e], GTF_TRUTH_ERR_RANGE);
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
    a.w.ka[i] = flip(a.pid[index_or0(a.w.vb[i], a.N)]);
}

// kb: the particle keys in ((event,) particle, not sel, volume, layer, module) order; va: the rows.
// Position i of that order belongs to the event evr[i].
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_mark(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int r = index_or0(a.w.va[i], a.N);
    const bool s = a.w.sel[r];
    bool head = false, vl = false, dup = false;
    if (s) {
        head = i == 0 || a.w.kb[i - 1] != a.w.kb[i];
        if constexpr (EV) head = head || a.w.evr[i - 1] != a.w.evr[i];
        vl = head;
        if (!head) {   // the predecessor is a selected row of the same particle (of the same event)
            const int q = index_or0(a.w.va[i - 1], a.N);
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

template <bool EV>
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
        a.o.part_id[r] = unflip(a.w.kb[i]);
        a.o.part_hits[r] = hits;
        a.o.part_ref[r] = (uint8_t)ref;
    }
    a.w.ref[r] = ref;
    if constexpr (EV) {
        if (r == a.N - 1) a.w.ref[a.N] = 0;
    } else {
        if (r == 0) a.w.scal[S_R] = R;
    }
}

// ---- 5. hit_dissociation ----
__global__ __launch_bounds__(BLOCK) void k_node_keys(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    a.w.ka[i] = flip(a.node[i]);
    a.w.va[i] = i;
}

// kb / vb: the nodes and rows in ((event,) node, row) order: position p belongs to the event evr[p]
__global__ __launch_bounds__(BLOCK) void k_hit_keys(Build a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.N) return;
    a.w.ka[p] = flip(a.hit[index_or0(a.w.vb[p], a.N)]);
    a.w.va[p] = p;
}

// kc / vc: the hits and positions in ((event,) hit, node, row) order -> per position: kept | node head << 32
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_first(Build a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    const int p = a.w.vc[i];
    if (p < 0 || p >= a.N) return;
    bool first = i == 0 || a.w.kc[i - 1] != a.w.kc[i];
    if constexpr (EV) first = first || a.w.evr[i - 1] != a.w.evr[i];
    if (!first) first = a.w.kb[index_or0(a.w.vc[i - 1], a.N)] != a.w.kb[p];
    bool head = p == 0 || a.w.kb[p - 1] != a.w.kb[p];
    if constexpr (EV) head = head || a.w.evr[p - 1] != a.w.evr[p];
    a.w.in_a[p] = (int64_t)first | ((int64_t)head << 32);
}

// sum: the exclusive sum of (kept | node head << 32) over the ((event,) node, row) order. One
// event: sum_a; a batch: sum_b, since sum_a keeps the region heads for the offsets
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_csr(Build a) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.N) return;
    const int64_t* sum = EV ? a.w.sum_b : a.w.sum_a;
    const int64_t s = sum[p], n = sum[p + 1];
    const int e = lo32(s), t = hi32(s);
    if (lo32(n) != e && e >= 0 && e < a.N) a.o.node_part[e] = a.w.row_part[index_or0(a.w.vb[p], a.N)];
    if (hi32(n) != t && t >= 0 && t < a.N) {
        a.o.node_id[t] = unflip(a.w.kb[p]);
        a.o.node_ptr[t] = e;
    }
    if (p == a.N - 1) {
        const int T = hi32(n), P = lo32(n);
        if (T >= 0 && T <= a.N) a.o.node_ptr[T] = P;
        if constexpr (!EV) {
            a.w.scal[S_T] = T;
            a.w.scal[S_P] = P;
        }
    }
}

// ---- a batch's offsets and counts: the sums read at row_off ----
__global__ __launch_bounds__(BLOCK) void k_counts(Build a) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e > a.K) return;
    const int r0 = gtf::clampi(a.w.roff[e], 0, a.N);
    const int64_t reg = a.w.sum_a[r0], csr = a.w.sum_b[r0];
    a.o.part_off[e] = lo32(reg);
    a.o.node_off[e] = hi32(csr);
    a.o.entry_off[e] = lo32(csr);
    if (e == a.K) return;
    const int r1 = gtf::clampi(a.w.roff[e + 1], r0, a.N);
    const int64_t reg1 = a.w.sum_a[r1], csr1 = a.w.sum_b[r1];
    const int p0 = gtf::clampi(lo32(reg), 0, a.N), p1 = gtf::clampi(lo32(reg1), p0, a.N);
    int32_t* c = a.w.cnt + (size_t)e * CNT_WORDS;
    c[0] = hi32(csr1) - hi32(csr);
    c[1] = lo32(csr1) - lo32(csr);
    c[2] = lo32(reg1) - lo32(reg);
    c[3] = a.w.refsum[p1] - a.w.refsum[p0];
    c[4] = (int32_t)a.w.err[e];
    c[5] = 0;
}

// offsets [K + 1] on the host: start at 0 and do not decrease (so none is negative)
const char* check_offsets(const int32_t* off, int K) {
    if (off[0] != 0) return "does not start at 0";
    for (int e = 0; e < K; e++)
        if (off[e + 1] < off[e]) return "is negative or decreases";
    return nullptr;
}

// Every launch of a build, up to the words the entry point brings back. off: a batch's row_off,
// truth_off and particle_off on the host. 0, or fail()'s status.
template <bool EV>
int launch(const Build& a, const int32_t* const* off, hipStream_t st, const char* who) {
    const Ws& w = a.w;
    const int32_t K = a.K, N = a.N, NT = a.NT, NP = a.NP;
    const gtf::Cub cub{w.cub, st};
    hipError_t e;
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < K) bits++;
    // stable by key, then (a batch of K > 1) stable by the event of the element's value: (event, key, input order)
    auto sort = [&](const uint64_t* kin, uint64_t* kout, const int32_t* vin, int32_t* vout, int n,
                    const int32_t* ev) -> hipError_t {
        if (!EV || K == 1) return cub.sort_pairs(kin, kout, vin, vout, n);
        hipError_t r = cub.sort_pairs(kin, w.tmpk, vin, w.tmpv, n);
        if (r != hipSuccess) return r;
        hipLaunchKernelGGL(k_event_keys, dim3(grid(n)), dim3(BLOCK), 0, st, w.tmpv, n, ev, w.ek, w.epos);
        if ((r = cub.sort_pairs(w.ek, w.ek2, w.epos, w.eperm, n, bits)) != hipSuccess) return r;
        hipLaunchKernelGGL(k_permute, dim3(grid(n)), dim3(BLOCK), 0, st, w.tmpk, w.tmpv, w.eperm, n, kout, vout);
        return hipSuccess;
    };
    if constexpr (EV) {   // 0. the offsets, the error words, the event columns
        const size_t kb = 4 * ((size_t)K + 1);
        if ((e = hipMemcpyAsync(w.roff, off[0], kb, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(w.toff, off[1], kb, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(w.poff, off[2], kb, hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(who, "offsets", e);
        if ((e = hipMemsetAsync(w.err, 0, kb, st)) != hipSuccess) return fail(who, "memset", e);
        hipLaunchKernelGGL(k_truth_sizes, dim3(grid(K + 1)), dim3(BLOCK), 0, st, a);
        if ((e = cub.scan(w.tsz, w.eoff, K + 1)) != hipSuccess) return fail(who, "scan events", e);
        const int32_t longest = N > NT ? (N > NP ? N : NP) : (NT > NP ? NT : NP);
        hipLaunchKernelGGL(k_events, dim3(grid(longest)), dim3(BLOCK), 0, st, a);
    } else {
        if ((e = hipMemsetAsync(w.scal, 0, 4 * S_WORDS, st)) != hipSuccess) return fail(who, "memset", e);
    }
    // 1. the high-pT ids
    if (NP > 0) {
        hipLaunchKernelGGL(k_particles<EV>, dim3(grid(NP)), dim3(BLOCK), 0, st, a);
        if ((e = sort(w.ka, w.pk, w.va, EV ? w.pidx : w.pf, NP, w.evp)) != hipSuccess) return fail(who, "sort particles", e);
        if constexpr (EV) hipLaunchKernelGGL(k_particles_sorted, dim3(grid(NP)), dim3(BLOCK), 0, st, a);
        if ((e = cub.scan(w.pf, w.ps, NP + 1)) != hipSuccess) return fail(who, "scan particles", e);
    }
    // 2. the truth rows by hit
    hipLaunchKernelGGL(k_truth_rows<EV>, dim3(grid(NT)), dim3(BLOCK), 0, st, a);
    if ((e = sort(w.ka, w.tk, w.va, w.tidx, NT, w.evt)) != hipSuccess) return fail(who, "sort truth", e);
    hipLaunchKernelGGL(k_truth_sorted, dim3(grid(NT)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.tfs, w.ts, NT + 1)) != hipSuccess) return fail(who, "scan truth", e);
    // 3. the rows; 4. the region particles: by module key, stably by particle (, stably by event)
    hipLaunchKernelGGL(k_rows<EV>, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.sort_pairs(w.ka, w.kb, w.va, w.vb, N)) != hipSuccess) return fail(who, "sort modules", e);
    hipLaunchKernelGGL(k_pid_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = sort(w.ka, w.kb, w.vb, w.va, N, w.evr)) != hipSuccess) return fail(who, "sort region", e);
    hipLaunchKernelGGL(k_mark<EV>, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.in_a, w.sum_a, N + 1)) != hipSuccess) return fail(who, "scan heads", e);
    if ((e = cub.scan(w.in_b, w.sum_b, N + 1)) != hipSuccess) return fail(who, "scan rows", e);
    hipLaunchKernelGGL(k_heads, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_region<EV>, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if constexpr (EV) {
        if ((e = cub.scan(w.ref, w.refsum, N + 1)) != hipSuccess) return fail(who, "scan reference", e);
    } else {
        if ((e = cub.sum(w.ref, w.scal + S_REF, N)) != hipSuccess) return fail(who, "sum", e);
    }
    // 5. the CSR
    hipLaunchKernelGGL(k_node_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = sort(w.ka, w.kb, w.va, w.vb, N, w.evr)) != hipSuccess) return fail(who, "sort nodes", e);
    hipLaunchKernelGGL(k_hit_keys, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = sort(w.ka, w.kc, w.va, w.vc, N, w.evr)) != hipSuccess) return fail(who, "sort pairs", e);
    hipLaunchKernelGGL(k_first<EV>, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if ((e = cub.scan(w.in_a, EV ? w.sum_b : w.sum_a, N + 1)) != hipSuccess) return fail(who, "scan pairs", e);
    hipLaunchKernelGGL(k_csr<EV>, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    if constexpr (EV) hipLaunchKernelGGL(k_counts, dim3(grid(K + 1)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    return 0;
}

// the argument checks both entry points make alike: the first missing array, or null
template <typename In>
const char* missing_columns(const In* in, int32_t N, bool truth, bool particles) {
    if (N > 0 && (!in->node_idx || !in->hit_id || !in->particle_id || !in->volume_id || !in->layer_id || !in->module_id))
        return "a mapping column";
    if (truth && (!in->truth_hit || !in->truth_part)) return "truth_hit / truth_part";
    if (particles && (!in->part_id || !in->px || !in->py)) return "part_id / px / py";
    return nullptr;
}

template <typename In>
void fill(Build& a, const In* in) {
    a.num_layers = in->num_layers; a.min_volume = in->min_volume; a.max_volume = in->max_volume;
    a.pt_cut = in->pt_cut;
    a.node = in->node_idx; a.hit = in->hit_id; a.pid = in->particle_id;
    a.vol = in->volume_id; a.lay = in->layer_id; a.mod = in->module_id;
    a.th = in->truth_hit; a.tp = in->truth_part;
    a.part_id = in->part_id; a.px = in->px; a.py = in->py;
}

}  // namespace

extern "C" {

size_t gtf_truth_build_workspace_bytes(int32_t n_rows, int32_t n_truth, int32_t n_particles) {
    const int64_t N = n_rows > 0 ? n_rows : 0;
    return carve<false>(nullptr, N, n_truth > 0 ? n_truth : N, n_particles > 0 ? n_particles : 0, 0).total;
}

size_t gtf_truth_build_ev_workspace_bytes(int32_t n_rows, int32_t n_truth, int32_t n_particles, int32_t n_events) {
    const int64_t N = n_rows > 0 ? n_rows : 0, NT = n_truth > 0 ? n_truth : 0;
    return carve<true>(nullptr, N, N + NT, n_particles > 0 ? n_particles : 0, n_events > 0 ? n_events : 0).total;
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
    const char* miss = !buf->node_ptr ? "buf.node_ptr" : missing_columns(in, N, in->n_truth > 0, NP > 0);
    if (!miss && N > 0 && (!buf->node_id || !buf->node_part || !buf->part_id || !buf->part_hits || !buf->part_ref))
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
    fill(a, in);
    a.K = 1; a.N = N; a.NT = in->n_truth > 0 ? in->n_truth : N; a.NP = NP;
    if (in->n_truth <= 0) {
        a.th = in->hit_id;
        a.tp = in->particle_id;
    }
    a.o = gtf_truth_batch_buf{nullptr, nullptr, nullptr, buf->node_id, buf->node_ptr, buf->node_part,
                              buf->part_id, buf->part_hits, buf->part_ref};
    a.w = carve<false>(workspace, N, a.NT, NP, 0);
    if (int rc = launch<false>(a, nullptr, st, who)) return rc;
    int32_t c[S_WORDS] = {0, 0, 0, 0, 0};
    if ((e = hipMemcpyAsync(c, a.w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
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

int gtf_truth_build_ev(const gtf_truth_in_ev* in, const gtf_truth_batch_buf* buf, gtf_truth_batch* out,
                       gtf_truth_counts* counts, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_truth_build_ev";
    char m[260];
    if (int rc = gtf::check_abi(in, who, "gtf_truth_in_ev", "gtf_truth_in_ev")) return rc;
    if (int rc = gtf::check_abi(out, who, "gtf_truth_batch", "gtf_truth_batch")) return rc;
    if (!buf) return bad("gtf_truth_build_ev: null buf, out or counts");
    const int32_t K = in->n_events;
    if (K < 0) return bad("gtf_truth_build_ev: negative sizes");
    if (K > 0 && !counts) return bad("gtf_truth_build_ev: null buf, out or counts");
    if (!in->row_off || !in->truth_off || !in->particle_off)
        return bad("gtf_truth_build_ev: missing array: row_off / truth_off / particle_off");
    const int32_t* offs[3] = {in->row_off, in->truth_off, in->particle_off};
    const char* names[3] = {"row_off", "truth_off", "particle_off"};
    for (int x = 0; x < 3; x++)
        if (const char* what = check_offsets(offs[x], K)) {
            snprintf(m, sizeof(m), "gtf_truth_build_ev: %s %s", names[x], what);
            return bad(m);
        }
    int64_t nt_eff = 0;   // the truth rows with the own-column events' mapping rows in their place
    for (int e = 0; e < K; e++) {
        const int64_t t = (int64_t)in->truth_off[e + 1] - in->truth_off[e];
        nt_eff += t > 0 ? t : (int64_t)in->row_off[e + 1] - in->row_off[e];
    }
    if (in->row_off[K] > MAX_ROWS || in->truth_off[K] > MAX_ROWS || in->particle_off[K] > MAX_ROWS || nt_eff > MAX_ROWS)
        return bad("gtf_truth_build_ev: more than 2^30 rows");
    if (in->min_volume > in->max_volume) return bad("gtf_truth_build_ev: min_volume > max_volume");
    const int32_t N = in->row_off[K], NTc = in->truth_off[K], NP = in->particle_off[K];
    const char* miss = !buf->node_ptr ? "buf.node_ptr"
                       : !buf->node_off || !buf->entry_off || !buf->part_off ? "buf.node_off / entry_off / part_off"
                       : missing_columns(in, N, N > 0 && NTc > 0, N > 0 && NP > 0);
    if (!miss && N > 0 && (!buf->node_id || !buf->node_part || !buf->part_id || !buf->part_hits || !buf->part_ref))
        miss = "an output array of gtf_truth_batch_buf";
    if (miss) {
        snprintf(m, sizeof(m), "gtf_truth_build_ev: missing array: %s", miss);
        return bad(m);
    }
    if (N > 0 && (!workspace || workspace_bytes < gtf_truth_build_ev_workspace_bytes(N, NTc, NP, K)))
        return bad("gtf_truth_build_ev: workspace smaller than gtf_truth_build_ev_workspace_bytes");
    out->n_events = K;
    out->n_nodes = out->n_entries = out->n_particles = 0;
    out->node_off = buf->node_off; out->entry_off = buf->entry_off; out->part_off = buf->part_off;
    out->node_id = buf->node_id; out->node_ptr = buf->node_ptr; out->node_part = buf->node_part;
    out->part_id = buf->part_id; out->part_hits = buf->part_hits; out->part_ref = buf->part_ref;
    for (int e = 0; e < K; e++) {
        counts[e].n_nodes = counts[e].n_entries = counts[e].n_particles = counts[e].n_reference = 0;
        counts[e].error = 0;
        counts[e].pad_ = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (N == 0) {   // (four stream-ordered fills; nothing to bring back)
        const size_t kb = 4 * ((size_t)K + 1);
        if ((e = hipMemsetAsync(buf->node_off, 0, kb, st)) != hipSuccess ||
            (e = hipMemsetAsync(buf->entry_off, 0, kb, st)) != hipSuccess ||
            (e = hipMemsetAsync(buf->part_off, 0, kb, st)) != hipSuccess ||
            (e = hipMemsetAsync(buf->node_ptr, 0, 4, st)) != hipSuccess)
            return fail(who, "memset", e);
        return 0;
    }
    Build a;
    fill(a, in);
    a.K = K; a.N = N; a.NT = (int32_t)nt_eff; a.NP = NP;
    a.o = *buf;
    a.w = carve<true>(workspace, N, (int64_t)N + NTc, NP, K);
    if (int rc = launch<true>(a, offs, st, who)) return rc;
    if ((e = hipMemcpyAsync(counts, a.w.cnt, sizeof(gtf_truth_counts) * (size_t)K, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    for (int ev = 0; ev < K; ev++) {
        if (!counts[ev].error) continue;
        snprintf(m, sizeof(m), "gtf_truth_build_ev: event %d: %s", ev,
                 counts[ev].error & GTF_TRUTH_ERR_RANGE ? "a volume_id, layer_id or module_id outside [0, 2^21)"
                                                        : "a mapped hit has no truth row");
        return bad(m);
    }
    int64_t T = 0, P = 0, R = 0;
    for (int ev = 0; ev < K; ev++) {
        const gtf_truth_counts& c = counts[ev];
        const int32_t n = in->row_off[ev + 1] - in->row_off[ev];
        if (c.n_nodes < 0 || c.n_nodes > n || c.n_entries < c.n_nodes || c.n_entries > n || c.n_particles < 0 ||
            c.n_particles > n || c.n_reference < 0 || c.n_reference > c.n_particles)
            return bad("gtf_truth_build_ev: inconsistent counts");
        T += c.n_nodes; P += c.n_entries; R += c.n_particles;
    }
    out->n_nodes = (int32_t)T; out->n_entries = (int32_t)P; out->n_particles = (int32_t)R;
    return 0;
}

}  // extern "C"
