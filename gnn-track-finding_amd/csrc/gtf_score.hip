// gtf_score.hip -- candidate scoring on the GPU, for one event (include/gtf.h: gtf_score_reset,
// gtf_score_candidates, gtf_score_finish) and for the K events of a fused graph in one call
// (gtf_truth_concat, gtf_score_reset_ev, gtf_score_candidates_ev, gtf_score_finish_ev):
// src/extract/reconstruction_efficiency.py:118-183 (gtf/metrics.py candidate_particles, majority,
// reconstruction_efficiency) on the device arrays gtf_extract_outputs leaves, accumulated over
// the iterations of the loop. The batch computes what K one-event calls compute, in launch
// sequences whose length does not depend on K: the K truth tables lie end to end (ids of
// different events collide) and every lookup stays inside its own event's segment. Members, vote
// and winners exist once: the kernels take the compile-time flag EV, and the one-event
// instantiation searches [0, T) and [0, R) and pays nothing for events.
//
//   candidates 0. (batch) per candidate its event (a search over cand_first, staged in LDS when
//                 it fits; -1 for an unscored event or a broken cand_first), per event the
//                 checks of cand_first
//              1. per member: binary search of its id in truth.node_id (as find_id in
//                 gtf_pyset.h), of a batch inside its event's segment; the start of its
//                 node_part row and the row's length. hipCUB exclusive sum of the lengths:
//                 candidate c's entries are off[cand_ptr[c]] .. off[cand_ptr[c + 1]], never
//                 materialised
//              2. the vote. A wavefront takes 4 consecutive candidates, one per 16 lanes.
//                 One entry per lane: entry e's member by a binary search in the candidate's
//                 own slice of `off`. For position j = 0, 1, ...: broadcast j's id, ballot
//                 the equal lanes, count = popcount. j ascends and only a larger count
//                 replaces the best, so the winner is the id of the highest count whose first
//                 occurrence (the lowest set bit of its ballot) comes first: max over
//                 (count, -first), Counter + max(key=get). Candidates of 17..64 entries then
//                 take the whole wavefront one after the other, the same loop in registers;
//                 longer ones the chunked loop (every position against every 64-entry chunk:
//                 O(n^2 / 64) searches, any length). The group's first lane looks the particle
//                 up (in its event's segment), applies the thresholds and claims part r with a
//                 64-bit atomicMin on best_key[r]; the key holds the candidate's index inside
//                 its event
//              3. per passing candidate: the one whose key is the stored one writes
//                 best_good / best_total
//   finish     one event: radix sort of the R (key, particle) pairs, unmatched keys (all-ones)
//              last; one launch writes the records and the count; one synchronisation.
//              A batch: one segmented radix sort of the keys over part_off (unmatched keys last
//              in their segment); per event the number of matched keys; their exclusive sum;
//              one launch writes the records compacted; one synchronisation
//   concat     1. one block: the exclusive sums of the parts' nodes, entries and particles
//              2. one launch over nodes (+ the closing pointer), entries and particles
//                 (blockIdx.y): a thread finds its part by a binary search over the offsets of
//                 its axis -- staged in LDS when they fit -- and copies its row, node_ptr
//                 shifted by the part's entry offset
//   reset      (batch) one launch: every key, or the keys of the marked events
//
// No same-address atomic except on a violation: the claims land on R different words, the error
// words are touched only when the input is broken. Every read is clamped to the sums the host
// passed. Vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_search.h"

namespace {

using gtf::bad;
using gtf::bound;
using gtf::fail;
using gtf::grid;
using gtf::segment;
using gtf::segment_of;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int G = 16;                  // lanes of a small candidate's group
constexpr int PER_WAVE = 64 / G;       // candidates of a wavefront
constexpr int PER_BLOCK = PER_WAVE * (BLOCK / 64);
constexpr uint64_t NONE = ~uint64_t(0);
constexpr int32_t MAX_MEMBERS = 1 << 30;
constexpr int COPY_BLOCKS = 1024;      // blocks per axis of the concat's copy launch
constexpr int64_t LIMIT = (int64_t)1 << 31;

// "who: " and the pieces of what it refuses: -2
int refuse(const char* who, const char* a, const char* b = "", const char* c = "", const char* d = "") {
    char m[320];
    snprintf(m, sizeof(m), "%s: %s%s%s%s", who, a, b, c, d);
    return bad(m);
}

// ---- concat ----
enum { AX_NODE = 0, AX_ENTRY = 1, AX_PART = 2, AXES = 3 };

__device__ __forceinline__ int32_t part_size(const gtf_truth_part& p, int axis) {
    const int32_t n = axis == AX_NODE ? p.n_nodes : axis == AX_ENTRY ? p.n_entries : p.n_particles;
    return n > 0 ? n : 0;
}

struct Concat {
    int32_t K, T, P, R;   // the host's sums: no write beyond them
    const gtf_truth_part* parts;
    gtf_truth_batch_buf o;
    int32_t* mismatch;
};

// one block: chunks of BLOCK parts, an inclusive scan in LDS per axis and a running carry
__global__ __launch_bounds__(BLOCK) void k_toffsets(Concat a) {
    __shared__ int64_t s[AXES][BLOCK];
    const int t = threadIdx.x, K = a.K;
    int32_t* const off[AXES] = {a.o.node_off, a.o.entry_off, a.o.part_off};
    int64_t carry[AXES] = {0, 0, 0};
    if (t == 0) *a.mismatch = 0;
    for (int base = 0; base < K; base += BLOCK) {
        const int i = base + t;
        int64_t v[AXES];
        for (int x = 0; x < AXES; x++) s[x][t] = v[x] = i < K ? part_size(a.parts[i], x) : 0;
        __syncthreads();
        for (int d = 1; d < BLOCK; d <<= 1) {
            int64_t add[AXES];
            for (int x = 0; x < AXES; x++) add[x] = t >= d ? s[x][t - d] : 0;
            __syncthreads();
            for (int x = 0; x < AXES; x++) s[x][t] += add[x];
            __syncthreads();
        }
        for (int x = 0; x < AXES; x++) {
            const int64_t o = carry[x] + s[x][t] - v[x];
            if (i < K) off[x][i] = o < LIMIT ? (int32_t)o : INT32_MAX;
            carry[x] += s[x][BLOCK - 1];
        }
        __syncthreads();
    }
    if (t < AXES) off[t][K] = carry[t] < LIMIT ? (int32_t)carry[t] : INT32_MAX;
}

__global__ __launch_bounds__(BLOCK) void k_tcopy(Concat a) {
    __shared__ int32_t lds[gtf::LDS_OFFS];
    const int axis = blockIdx.y;
    const int32_t* goff = axis == AX_NODE ? a.o.node_off : axis == AX_ENTRY ? a.o.entry_off : a.o.part_off;
    const int64_t rows = axis == AX_NODE ? (int64_t)a.T + 1 : axis == AX_ENTRY ? a.P : a.R;
    if (a.K == 0) {   // no part: the closing pointer alone
        if (axis == AX_NODE && blockIdx.x == 0 && threadIdx.x == 0) a.o.node_ptr[0] = 0;
        return;
    }
    const int32_t* off = gtf::stage_offsets<BLOCK>(goff, a.K, lds);
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * BLOCK) {
        if (axis == AX_NODE && r == a.T) {
            a.o.node_ptr[a.T] = a.P;
            continue;
        }
        const int p = segment_of(off, a.K, (int)r);
        const int l = (int)r - off[p];
        const gtf_truth_part q = a.parts[p];
        if (l < 0 || l >= part_size(q, axis)) {   // (the device table disagrees with the host's sums)
            atomicOr(a.mismatch, 1);
            continue;
        }
        if (axis == AX_NODE) {
            a.o.node_id[r] = q.node_id[l];
            a.o.node_ptr[r] = q.node_ptr[l] + a.o.entry_off[p];
        } else if (axis == AX_ENTRY) {
            a.o.node_part[r] = q.node_part[l];
        } else {
            a.o.part_id[r] = q.part_id[l];
            a.o.part_hits[r] = q.part_hits[l];
            a.o.part_ref[r] = q.part_ref[l];
        }
    }
}

// ---- candidates ----
// (batch): carved by carve<true> alone, null in the one-event instantiation
struct Ws {
    int32_t* c_event;                    // (batch) [n_cand] the candidate's event; -1: not scored
    int32_t *c_row, *c_good, *c_total;   // [n_cand] the passing candidate's particle row (-1: none), its counts
    int32_t* mrow;                       // [M + 1] start of the member's node_part row
    int64_t *mlen, *off;                 // [M + 1] its length; the exclusive sum
    gtf::Scratch cub;
    size_t total;
};

template <bool EV>
Ws carve(void* base, int64_t C, int64_t M) {
    Ws w = {};
    gtf::Arena a(base);
    const size_t c = (size_t)C, m1 = (size_t)M + 1;
    if constexpr (EV) w.c_event = a.take<int32_t>(c);
    w.c_row = a.take<int32_t>(c);
    w.c_good = a.take<int32_t>(c);
    w.c_total = a.take<int32_t>(c);
    w.mrow = a.take<int32_t>(m1);
    w.mlen = a.take<int64_t>(m1);
    w.off = a.take<int64_t>(m1);
    w.cub = gtf::CubNeed().scan<int64_t>((int)m1).take(a);
    w.total = a.used();
    return w;
}

// The fields marked (batch) are set for gtf_score_candidates_ev alone: in the one-event
// instantiation they are zero / null and only code under `if constexpr (EV)` may read them.
struct Score {
    int32_t K, T, P, R;      // (batch) events; the sums of the tables
    const int32_t *node_off, *part_off;   // (batch)
    const int64_t *node_id, *node_part, *part_id;
    const int32_t *node_ptr, *part_hits;
    const uint8_t *part_ref, *scored;     // scored: (batch)
    const int32_t *cand_ptr, *cand_first; // cand_first: (batch)
    const int64_t* cand_ids;
    int32_t C, M;            // candidates; member capacity of the workspace
    uint32_t group;
    gtf_score_out o;
    uint64_t* best_key;
    int32_t *best_good, *best_total;
    uint32_t* error;         // [1]; (batch) [2]: the bits, the first event of a violation
    Ws w;
};

// a violation; of a batch, met in event e (e < 0: in no event)
template <bool EV>
__device__ __forceinline__ void violation(const Score& a, uint32_t bit, int e) {
    atomicOr(&a.error[0], bit);
    if constexpr (EV)
        if (e >= 0) atomicMin((int32_t*)&a.error[1], e);
}

// the claim of candidate c (of event e): the group, then its index inside its event
template <bool EV>
__device__ __forceinline__ unsigned long long claim(const Score& a, int c, int e) {
    if constexpr (EV) c -= a.cand_first[e];
    return ((unsigned long long)a.group << 32) | (uint32_t)c;
}

// the members in use: cand_ptr[C] clamped to the workspace's capacity
__device__ __forceinline__ int members(const Score& a) {
    const int m = a.cand_ptr[a.C];
    return m < 0 ? 0 : m > a.M ? a.M : m;
}

// ---- 0. the candidates' events ----
__global__ __launch_bounds__(BLOCK) void k_events(Score a) {
    __shared__ int32_t lds[gtf::LDS_OFFS];
    const int32_t* cf = gtf::stage_offsets<BLOCK>(a.cand_first, a.K, lds);
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i <= a.K) {
        bool wrong = (i == 0 && cf[0] != 0) || (i == a.K && cf[a.K] != a.C);
        if (i < a.K) wrong |= cf[i] > cf[i + 1];
        if (wrong) violation<true>(a, GTF_SCORE_ERR_RANGE, -1);
    }
    if (i >= a.C) return;
    int e = -1;
    if (a.K > 0) {
        e = segment_of(cf, a.K, i);
        if (cf[e] > i || cf[e + 1] <= i) e = -1;   // (a broken cand_first, reported above: the candidate is skipped)
        else if (a.scored && !a.scored[e]) e = -1;
    }
    a.w.c_event[i] = e;
}

// ---- 1. members ----
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_members(Score a) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m > a.M) return;
    const int nm = a.cand_ptr[a.C];
    if (m == 0 && (nm < 0 || nm > a.M)) violation<EV>(a, nm < 0 ? GTF_SCORE_ERR_RANGE : GTF_SCORE_ERR_WORKSPACE, -1);
    int row = 0, len = 0;
    if (m < nm) {
        int e = 0, s0 = 0, s1 = a.T;   // its event; the event's nodes
        if constexpr (EV) {
            e = a.w.c_event[segment_of(a.cand_ptr, a.C, m)];   // its candidate's (empty ones are passed over)
            if (e >= 0) segment(a.node_off, e, a.T, s0, s1);
        }
        if (e >= 0) {
            const int64_t key = a.cand_ids[m];
            const int lo = s0 + bound<false>(a.node_id + s0, s1 - s0, key);
            if (lo < s1 && a.node_id[lo] == key) {
                int b = a.node_ptr[lo], n = a.node_ptr[lo + 1];   // clamped: a malformed node_ptr reads nothing outside
                if (b < 0) b = 0;
                if (n > a.P) n = a.P;
                row = b;
                len = n > b ? n - b : 0;
            } else {
                violation<EV>(a, GTF_SCORE_ERR_MISSING, e);   // (only on a violation)
            }
        }
    }
    a.w.mrow[m] = row;
    a.w.mlen[m] = len;
}

// ---- 2. the vote ----
struct Cand {
    int lo, hi;       // its members
    int64_t base, n;  // off[lo]; its entries
};

// entry e (0 <= e < c.n) of the candidate: the member m with off[m] - base <= e < off[m + 1] - base
__device__ __forceinline__ int64_t entry(const Score& a, const Cand& c, int64_t e) {
    const int l = segment_of(a.w.off, c.hi - c.lo, e + c.base, c.lo);
    const int64_t i = (int64_t)a.w.mrow[l] + (e - (a.w.off[l] - c.base));
    return i >= 0 && i < a.P ? a.node_part[i] : 0;
}

// One entry per lane of a W-lane group at lane gbase (W = 64: the wavefront). Every lane of the
// wavefront calls it; nmax bounds the positions of every group (wave-uniform).
template <int W>
__device__ __forceinline__ void vote(bool on, int64_t id, int n, int nmax, int gbase, int& best_cnt, int64_t& best_id) {
    const unsigned long long mask = W == 64 ? ~0ull : ((1ull << W) - 1);
    for (int j = 0; j < nmax; j++) {
        const int64_t idj = __shfl((long long)id, gbase + j);
        const unsigned long long eq = (__ballot(on && id == idj) >> gbase) & mask;
        const int cnt = j < n ? __popcll(eq) : 0;
        // j ascends: a count is first met at its id's first occurrence, so "larger only" keeps,
        // among the ids of the highest count, the one seen first (Counter + max(key=get))
        if (cnt > best_cnt) {
            best_cnt = cnt;
            best_id = idj;
        }
    }
}

template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_vote(Score a) {
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane - gl;
    const int wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const int c = wave * PER_WAVE + (lane / G);
    const int nm = members(a);
    const bool valid = c < a.C;
    Cand cd = {0, 0, 0, 0};
    bool broken = false;
    if (valid) {
        int lo = a.cand_ptr[c], hi = a.cand_ptr[c + 1];
        broken = lo < 0 || hi < lo;
        if (lo < 0) lo = 0;
        if (lo > nm) lo = nm;
        if (hi > nm) hi = nm;   // (past the capacity: GTF_SCORE_ERR_WORKSPACE is set, nothing is read there)
        if (hi < lo) hi = lo;
        cd.lo = lo;
        cd.hi = hi;
        cd.base = a.w.off[lo];
        cd.n = a.w.off[hi] - cd.base;
        if (cd.n > INT32_MAX) {   // (the counts are int32; such a candidate would not finish its loop either)
            broken = true;
            cd.n = 0;
        }
    }
    int best_cnt = 0;
    int64_t best_id = 0;
    // up to G entries: the four groups at once
    {
        const bool small = valid && cd.n <= G;
        const int n = small ? (int)cd.n : 0;
        int nmax = n;
        for (int s = G; s < 64; s <<= 1) nmax = max(nmax, __shfl_xor(nmax, s));
        const bool on = gl < n;
        const int64_t id = on ? entry(a, cd, gl) : 0;
        vote<G>(on, id, n, nmax, gbase, best_cnt, best_id);
    }
    // longer ones: the wavefront, one candidate after the other
    for (int g = 0; g < PER_WAVE; g++) {
        Cand w;
        w.lo = __shfl(cd.lo, g * G);
        w.hi = __shfl(cd.hi, g * G);
        w.base = __shfl((long long)cd.base, g * G);
        w.n = __shfl((long long)cd.n, g * G);
        if (w.n <= G) continue;   // (wave-uniform)
        int cnt = 0;
        int64_t bid = 0;
        if (w.n <= 64) {
            const bool on = lane < w.n;
            const int64_t id = on ? entry(a, w, lane) : 0;
            vote<64>(on, id, (int)w.n, (int)w.n, 0, cnt, bid);
        } else {
            for (int64_t j = 0; j < w.n; j++) {
                const int64_t idj = entry(a, w, j);
                int k = 0;
                for (int64_t e0 = 0; e0 < w.n; e0 += 64) {
                    const int64_t e = e0 + lane;
                    k += __popcll(__ballot(e < w.n && entry(a, w, e) == idj));
                }
                if (k > cnt) {
                    cnt = k;
                    bid = idj;
                }
            }
        }
        if (lane / G == g) {
            best_cnt = cnt;
            best_id = bid;
        }
    }
    if (!valid || gl != 0) return;
    int e = 0, s0 = 0, s1 = a.R;   // its event; the event's particles
    if constexpr (EV) e = a.w.c_event[c];
    if (broken) violation<EV>(a, GTF_SCORE_ERR_RANGE, e);
    const int total = (int)cd.n;   // (0 for a candidate that is not scored: its members have no rows)
    int row = -1;
    if (total > 0 && e >= 0) {
        if constexpr (EV) segment(a.part_off, e, a.R, s0, s1);
        const int lo = s0 + bound<false>(a.part_id + s0, s1 - s0, best_id);
        if (lo < s1 && a.part_id[lo] == best_id && a.part_ref[lo] && 2 * (int64_t)best_cnt >= a.part_hits[lo] &&
            2 * (int64_t)best_cnt >= total)
            row = lo;
    }
    if (row >= 0) atomicMin((unsigned long long*)&a.best_key[row], claim<EV>(a, c, e));
    a.w.c_row[c] = row;
    a.w.c_good[c] = best_cnt;
    a.w.c_total[c] = total;
    if (a.o.pid) a.o.pid[c] = best_id;
    if (a.o.n_good) a.o.n_good[c] = best_cnt;
    if (a.o.total) a.o.total[c] = total;
    if (a.o.passes) a.o.passes[c] = row >= 0;
}

// ---- 3. the winners ----
template <bool EV>
__global__ __launch_bounds__(BLOCK) void k_winners(Score a) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.C) return;
    const int row = a.w.c_row[c];
    if (row < 0 || row >= a.R) return;
    int e = 0;
    if constexpr (EV) {
        e = a.w.c_event[c];
        if (e < 0 || e >= a.K) return;
    }
    if (a.best_key[row] != claim<EV>(a, c, e)) return;
    a.best_good[row] = a.w.c_good[c];
    a.best_total[row] = a.w.c_total[c];
}

// ---- reset ----
__global__ __launch_bounds__(BLOCK) void k_reset_ev(uint64_t* best_key, uint32_t* error, int R, int K,
                                                    const int32_t* part_off, const uint8_t* events) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (!events) {
        if (r == 0) {
            error[0] = 0;
            error[1] = (uint32_t)INT32_MAX;
        }
        if (r < R) best_key[r] = NONE;
        return;
    }
    if (r >= R || K <= 0) return;
    const int e = segment_of(part_off, K, r);
    if (part_off[e] <= r && r < part_off[e + 1] && events[e]) best_key[r] = NONE;
}

// ---- finish ----
// (batch): set by the batch finish alone, null / zero in the one-event one (FinWs and Fin)
struct FinWs {
    uint64_t* keys;          // [R] sorted (a batch: inside every event's segment)
    int32_t *vin, *vout;     // [R] particle rows
    int32_t* cnt;            // (batch) [K + 1] matched keys per event, a closing 0
    int32_t* scal;           // [2] n_reconstructed, error; (batch) the error words
    gtf::Scratch cub;
    size_t total;
};

template <bool EV>
FinWs carve_fin(void* base, int64_t R, int64_t K) {
    FinWs w = {};
    gtf::Arena a(base);
    w.scal = a.take<int32_t>(16);
    if constexpr (EV) w.cnt = a.take<int32_t>((size_t)K + 1);
    w.keys = a.take<uint64_t>((size_t)R);
    w.vin = a.take<int32_t>((size_t)R);
    w.vout = a.take<int32_t>((size_t)R);
    if constexpr (EV) {   // (one piece serves the segmented sort and the scan: the larger of the two)
        size_t bytes = 0, scan = 0;
        (void)hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                                          (int32_t*)nullptr, (int32_t*)nullptr, (int)R, (int)K,
                                                          (const int32_t*)nullptr, (const int32_t*)nullptr);
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int32_t*)nullptr, (int32_t*)nullptr, (int)K + 1);
        if (scan > bytes) bytes = scan;
        w.cub = gtf::Scratch{a.take<char>(bytes), bytes};
    } else {
        w.cub = gtf::CubNeed().sort_pairs<uint64_t, int32_t>((int)R).take(a);
    }
    w.total = a.used();
    return w;
}

struct Fin {
    int32_t R, K;            // K, part_off, rec_first: (batch)
    const int32_t* part_off;
    const int64_t* part_id;
    const int32_t *part_hits, *best_good, *best_total;
    const uint64_t* best_key;
    const uint32_t* error;
    uint64_t* out_key;
    int64_t* out_pid;
    int32_t *out_good, *out_total, *out_hits, *rec_first;
    FinWs w;
};

__global__ __launch_bounds__(BLOCK) void k_iota(Fin a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r < a.R) a.w.vin[r] = r;
}

// sorted position i, the record of particle vout[i], to out[at]
__device__ __forceinline__ void record(const Fin& a, int i, int64_t at) {
    const int r = a.w.vout[i];
    if (r < 0 || r >= a.R) return;
    if (a.out_key) a.out_key[at] = a.w.keys[i];
    if (a.out_pid) a.out_pid[at] = a.part_id[r];
    if (a.out_good) a.out_good[at] = a.best_good[r];
    if (a.out_total) a.out_total[at] = a.best_total[r];
    if (a.out_hits) a.out_hits[at] = a.part_hits[r];
}

__global__ __launch_bounds__(BLOCK) void k_records(Fin a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) {
        a.w.scal[1] = (int32_t)*a.error;
        if (a.R == 0 || a.w.keys[0] == NONE) a.w.scal[0] = 0;
    }
    if (i >= a.R) return;
    if (a.w.keys[i] == NONE) return;
    if (i == a.R - 1 || a.w.keys[i + 1] == NONE) a.w.scal[0] = i + 1;   // (the last matched one: the only writer)
    record(a, i, i);
}

// per event the number of matched keys: the first all-ones key of its sorted segment
__global__ __launch_bounds__(BLOCK) void k_count_ev(Fin a) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e == 0) {
        a.w.scal[0] = (int32_t)a.error[0];
        a.w.scal[1] = (int32_t)a.error[1];
    }
    if (e > a.K) return;
    int n = 0;
    if (e < a.K) {
        int s0, s1;
        segment(a.part_off, e, a.R, s0, s1);
        n = bound<false>(a.w.keys + s0, s1 - s0, NONE);
    }
    a.w.cnt[e] = n;
}

__global__ __launch_bounds__(BLOCK) void k_records_ev(Fin a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.R || a.K <= 0) return;
    const int e = segment_of(a.part_off, a.K, i);
    const int j = i - a.part_off[e];
    if (j < 0 || j >= a.w.cnt[e]) return;
    const int64_t at = (int64_t)a.rec_first[e] + j;
    if (at < 0 || at >= a.R) return;
    record(a, i, at);
}

// ---- the argument checks ----
// The tables of another layout of include/gtf.h: -3; null or inconsistent ones: -2.
template <typename T>
int check_tables(const T* t, const char* who) {
    constexpr bool EV = std::is_same<T, gtf_truth_batch>::value;
    const char* type = EV ? "gtf_truth_batch" : "gtf_truth";
    if (int rc = gtf::check_abi(t, who, type, type)) return rc;
    bool negative = t->n_nodes < 0 || t->n_entries < 0 || t->n_particles < 0;
    const char* miss = nullptr;
    if constexpr (EV) {
        negative |= t->n_events < 0;
        if (!t->node_off || !t->entry_off || !t->part_off) miss = "node_off, entry_off or part_off";
    }
    if (negative) return refuse(who, "negative sizes in ", type);
    if (miss) {}
    else if (t->n_nodes > 0 && !t->node_id) miss = "node_id";
    else if (!t->node_ptr) miss = "node_ptr";
    else if (t->n_entries > 0 && !t->node_part) miss = "node_part";
    else if (t->n_particles > 0 && !t->part_id) miss = "part_id";
    else if (t->n_particles > 0 && !t->part_hits) miss = "part_hits";
    else if (t->n_particles > 0 && !t->part_ref) miss = "part_ref";
    return miss ? refuse(who, "missing ", type, " array ", miss) : 0;
}

// the state of the tables t (null: of any)
template <typename S, typename T>
int check_state(const S* s, const T* t, const char* who) {
    constexpr bool EV = std::is_same<S, gtf_score_state_ev>::value;
    const char* type = EV ? "gtf_score_state_ev" : "gtf_score_state";
    if constexpr (EV) {
        if (int rc = gtf::check_abi(s, who, type, type)) return rc;
    } else if (!s) {
        return refuse(who, "null ", type);
    }
    if (s->n_particles < 0) return refuse(who, "negative n_particles in ", type);
    if (!s->error) return refuse(who, "missing ", type, " array error");
    if (s->n_particles > 0 && (!s->best_key || !s->best_good || !s->best_total))
        return refuse(who, "missing ", type, " array (best_key, best_good, best_total)");
    if (t && s->n_particles != t->n_particles)
        return refuse(who, type, ".n_particles differs from ", EV ? "gtf_truth_batch" : "gtf_truth", ".n_particles");
    return 0;
}

template <bool EV>
size_t score_bytes(int32_t n_cand, int32_t n_members) {
    return carve<EV>(nullptr, n_cand > 0 ? n_cand : 0, n_members > 0 ? n_members : 0).total;
}

// gtf_score_candidates (cand_first: none) and gtf_score_candidates_ev
template <bool EV, typename T, typename S>
int score(const char* who, const char* sizer, const T* t, const int32_t* cand_ptr, const int64_t* cand_ids,
          const int32_t* cand_first, int32_t n_cand, int32_t group, const gtf_score_out* out, const S* state,
          void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    if (int rc = check_tables(t, who)) return rc;
    if (int rc = check_state(state, t, who)) return rc;
    if (n_cand < 0) return refuse(who, "negative n_cand");
    if (group < 0) return refuse(who, "negative group");
    if (n_cand == 0) return 0;
    if (n_cand > INT32_MAX - PER_BLOCK) return refuse(who, "too many candidates");
    if (!cand_ptr) return refuse(who, "missing array cand_ptr");
    if (!cand_ids) return refuse(who, "missing array cand_ids");
    if (EV && !cand_first) return refuse(who, "missing array cand_first");
    if (!workspace || workspace_bytes < score_bytes<EV>(n_cand, 0)) return refuse(who, "workspace smaller than ", sizer);
    // the member capacity of this workspace: the largest M that fits (the size is non-decreasing in M)
    int32_t lo = 0, hi = MAX_MEMBERS;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (score_bytes<EV>(n_cand, mid) <= workspace_bytes) lo = mid;
        else hi = mid - 1;
    }
    Score a = {};
    a.T = t->n_nodes; a.P = t->n_entries; a.R = t->n_particles;
    a.node_id = t->node_id; a.node_part = t->node_part; a.part_id = t->part_id;
    a.node_ptr = t->node_ptr; a.part_hits = t->part_hits; a.part_ref = t->part_ref;
    if constexpr (EV) {
        a.K = t->n_events;
        a.node_off = t->node_off; a.part_off = t->part_off;
        a.scored = t->scored;
    }
    a.cand_ptr = cand_ptr; a.cand_ids = cand_ids; a.cand_first = cand_first;
    a.C = n_cand; a.M = lo; a.group = (uint32_t)group;
    a.o = out ? *out : gtf_score_out{nullptr, nullptr, nullptr, nullptr};
    a.best_key = state->best_key; a.best_good = state->best_good; a.best_total = state->best_total;
    a.error = state->error;
    a.w = carve<EV>(workspace, n_cand, a.M);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if constexpr (EV) {
        const int64_t first = (int64_t)a.K + 1 > n_cand ? (int64_t)a.K + 1 : n_cand;
        hipLaunchKernelGGL(k_events, dim3(grid(first)), dim3(BLOCK), 0, st, a);
    }
    hipLaunchKernelGGL(k_members<EV>, dim3(grid((int64_t)a.M + 1)), dim3(BLOCK), 0, st, a);
    if ((e = gtf::Cub{a.w.cub, st}.scan(a.w.mlen, a.w.off, a.M + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_vote<EV>, dim3((n_cand + PER_BLOCK - 1) / PER_BLOCK), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_winners<EV>, dim3(grid(n_cand)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    return 0;
}

template <typename T, typename S>
Fin fin(const T* t, const S* state, uint64_t* out_key, int64_t* out_pid, int32_t* out_good, int32_t* out_total,
        int32_t* out_hits) {
    Fin a = {};
    a.R = t->n_particles;
    a.part_id = t->part_id; a.part_hits = t->part_hits;
    a.best_good = state->best_good; a.best_total = state->best_total; a.best_key = state->best_key;
    a.error = state->error;
    a.out_key = out_key; a.out_pid = out_pid; a.out_good = out_good; a.out_total = out_total; a.out_hits = out_hits;
    return a;
}

}  // namespace

extern "C" {

size_t gtf_truth_concat_workspace_bytes(int32_t n_parts) {
    (void)n_parts;   // (the mismatch word alone: the offsets go to the caller's arrays)
    gtf::Arena a(nullptr);
    a.take<int32_t>(16);
    return a.used();
}

int gtf_truth_concat(const gtf_truth_sizes* sizes, const gtf_truth_part* parts, int32_t n_parts,
                     const gtf_truth_batch_buf* buf, gtf_truth_batch* out, void* workspace,
                     size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_truth_concat";
    if (int rc = gtf::check_abi(out, who, "gtf_truth_batch", "gtf_truth_batch")) return rc;
    if (n_parts < 0) return bad("gtf_truth_concat: negative n_parts");
    if (!buf) return bad("gtf_truth_concat: null gtf_truth_batch_buf");
    if (n_parts > 0 && !sizes) return bad("gtf_truth_concat: null sizes");
    if (n_parts > 0 && !parts) return bad("gtf_truth_concat: null part table");
    int64_t sum[AXES] = {0, 0, 0};
    for (int i = 0; i < n_parts; i++) {
        const gtf_truth_sizes& z = sizes[i];
        if (z.n_nodes < 0 || z.n_entries < 0 || z.n_particles < 0) return bad("gtf_truth_concat: negative sizes");
        sum[AX_NODE] += z.n_nodes; sum[AX_ENTRY] += z.n_entries; sum[AX_PART] += z.n_particles;
    }
    for (int x = 0; x < AXES; x++)
        if (sum[x] >= LIMIT) return bad("gtf_truth_concat: the parts sum to 2^31 or more nodes, entries or particles");
    if (!buf->node_off || !buf->entry_off || !buf->part_off || !buf->node_ptr || (sum[AX_NODE] > 0 && !buf->node_id) ||
        (sum[AX_ENTRY] > 0 && !buf->node_part) ||
        (sum[AX_PART] > 0 && (!buf->part_id || !buf->part_hits || !buf->part_ref)))
        return bad("gtf_truth_concat: missing gtf_truth_batch_buf array");
    if (!workspace || workspace_bytes < gtf_truth_concat_workspace_bytes(n_parts))
        return bad("gtf_truth_concat: workspace smaller than gtf_truth_concat_workspace_bytes");
    Concat a;
    a.K = n_parts; a.T = (int32_t)sum[AX_NODE]; a.P = (int32_t)sum[AX_ENTRY]; a.R = (int32_t)sum[AX_PART];
    a.parts = parts; a.o = *buf; a.mismatch = (int32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_toffsets, dim3(1), dim3(BLOCK), 0, st, a);
    int64_t longest = (int64_t)a.T + 1;
    if (a.P > longest) longest = a.P;
    if (a.R > longest) longest = a.R;
    const int gx = grid(longest) < COPY_BLOCKS ? grid(longest) : COPY_BLOCKS;
    hipLaunchKernelGGL(k_tcopy, dim3(gx, AXES), dim3(BLOCK), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    out->n_events = n_parts; out->n_nodes = a.T; out->n_entries = a.P; out->n_particles = a.R;
    out->node_off = buf->node_off; out->entry_off = buf->entry_off; out->part_off = buf->part_off;
    out->node_id = buf->node_id; out->node_ptr = buf->node_ptr; out->node_part = buf->node_part;
    out->part_id = buf->part_id; out->part_hits = buf->part_hits; out->part_ref = buf->part_ref;
    return 0;
}

int gtf_score_reset(const gtf_score_state* state, gtf_stream_t stream) {
    const char* who = "gtf_score_reset";
    if (int rc = check_state(state, (const gtf_truth*)nullptr, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (state->n_particles > 0 &&
        (e = hipMemsetAsync(state->best_key, 0xff, 8 * (size_t)state->n_particles, st)) != hipSuccess)
        return fail(who, "memset", e);
    if ((e = hipMemsetAsync(state->error, 0, 4, st)) != hipSuccess) return fail(who, "memset", e);
    return 0;
}

int gtf_score_reset_ev(const gtf_score_state_ev* state, const gtf_truth_batch* batch, const uint8_t* events,
                       gtf_stream_t stream) {
    const char* who = "gtf_score_reset_ev";
    if (int rc = check_tables(batch, who)) return rc;
    if (int rc = check_state(state, batch, who)) return rc;
    const int32_t R = state->n_particles;
    if (events && R == 0) return 0;
    hipLaunchKernelGGL(k_reset_ev, dim3(grid(R > 0 ? R : 1)), dim3(BLOCK), 0, (hipStream_t)stream, state->best_key,
                       state->error, (int)R, (int)batch->n_events, batch->part_off, events);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

size_t gtf_score_workspace_bytes(int32_t n_cand, int32_t n_members) { return score_bytes<false>(n_cand, n_members); }

size_t gtf_score_ev_workspace_bytes(int32_t n_cand, int32_t n_members, int32_t n_events) {
    (void)n_events;   // (cand_first is read where it lies)
    return score_bytes<true>(n_cand, n_members);
}

size_t gtf_score_finish_workspace_bytes(int32_t n_particles) {
    return carve_fin<false>(nullptr, n_particles > 0 ? n_particles : 0, 0).total;
}

size_t gtf_score_finish_ev_workspace_bytes(int32_t n_particles, int32_t n_events) {
    return carve_fin<true>(nullptr, n_particles > 0 ? n_particles : 0, n_events > 0 ? n_events : 0).total;
}

int gtf_score_candidates(const gtf_truth* truth, const int32_t* cand_ptr, const int64_t* cand_ids,
                         int32_t n_cand, int32_t group, const gtf_score_out* out,
                         const gtf_score_state* state, void* workspace, size_t workspace_bytes,
                         gtf_stream_t stream) {
    return score<false>("gtf_score_candidates", "gtf_score_workspace_bytes", truth, cand_ptr, cand_ids, nullptr, n_cand,
                        group, out, state, workspace, workspace_bytes, stream);
}

int gtf_score_candidates_ev(const gtf_truth_batch* batch, const int32_t* cand_ptr, const int64_t* cand_ids,
                            const int32_t* cand_first, int32_t n_cand, int32_t group, const gtf_score_out* out,
                            const gtf_score_state_ev* state, void* workspace, size_t workspace_bytes,
                            gtf_stream_t stream) {
    return score<true>("gtf_score_candidates_ev", "gtf_score_ev_workspace_bytes", batch, cand_ptr, cand_ids, cand_first,
                       n_cand, group, out, state, workspace, workspace_bytes, stream);
}

int gtf_score_finish(const gtf_truth* truth, const gtf_score_state* state, uint64_t* out_key,
                     int64_t* out_pid, int32_t* out_good, int32_t* out_total, int32_t* out_hits,
                     gtf_score_counts* counts, void* workspace, size_t workspace_bytes,
                     gtf_stream_t stream) {
    const char* who = "gtf_score_finish";
    if (int rc = check_tables(truth, who)) return rc;
    if (int rc = check_state(state, truth, who)) return rc;
    if (!counts) return bad("gtf_score_finish: null counts");
    const int32_t R = truth->n_particles;
    if (!workspace || workspace_bytes < gtf_score_finish_workspace_bytes(R))
        return bad("gtf_score_finish: workspace smaller than gtf_score_finish_workspace_bytes");
    counts->n_reconstructed = 0;
    counts->error = 0;
    Fin a = fin(truth, state, out_key, out_pid, out_good, out_total, out_hits);
    a.w = carve_fin<false>(workspace, R, 0);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (R > 0) {
        hipLaunchKernelGGL(k_iota, dim3(grid(R)), dim3(BLOCK), 0, st, a);
        if ((e = gtf::Cub{a.w.cub, st}.sort_pairs(a.best_key, a.w.keys, a.w.vin, a.w.vout, R)) != hipSuccess)
            return fail(who, "sort", e);
    }
    hipLaunchKernelGGL(k_records, dim3(grid(R > 0 ? R : 1)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t c[2] = {0, 0};
    if ((e = hipMemcpyAsync(c, a.w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    counts->error = (uint32_t)c[1];
    if (counts->error & GTF_SCORE_ERR_MISSING) return bad("gtf_score_finish: a candidate node has no hit_dissociation");
    if (counts->error & GTF_SCORE_ERR_WORKSPACE)
        return bad("gtf_score_finish: a gtf_score_candidates call had more members than its workspace holds");
    if (counts->error & GTF_SCORE_ERR_RANGE)
        return bad("gtf_score_finish: a candidate of 2^31 or more particle entries, or a malformed cand_ptr");
    if (c[0] < 0 || c[0] > R) return bad("gtf_score_finish: inconsistent keys");
    counts->n_reconstructed = c[0];
    return 0;
}

int gtf_score_finish_ev(const gtf_truth_batch* batch, const gtf_score_state_ev* state, uint64_t* out_key,
                        int64_t* out_pid, int32_t* out_good, int32_t* out_total, int32_t* out_hits,
                        int32_t* rec_first, int32_t* n_reconstructed, uint32_t* error, void* workspace,
                        size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_score_finish_ev";
    if (int rc = check_tables(batch, who)) return rc;
    if (int rc = check_state(state, batch, who)) return rc;
    const int32_t R = batch->n_particles, K = batch->n_events;
    if (!rec_first) return bad("gtf_score_finish_ev: null rec_first");
    if (!error || (K > 0 && !n_reconstructed)) return bad("gtf_score_finish_ev: null counts");
    if (!workspace || workspace_bytes < gtf_score_finish_ev_workspace_bytes(R, K))
        return bad("gtf_score_finish_ev: workspace smaller than gtf_score_finish_ev_workspace_bytes");
    for (int i = 0; i < K; i++) n_reconstructed[i] = 0;
    error[0] = 0;
    error[1] = (uint32_t)INT32_MAX;
    Fin a = fin(batch, state, out_key, out_pid, out_good, out_total, out_hits);
    a.K = K;
    a.part_off = batch->part_off;
    a.rec_first = rec_first;
    a.w = carve_fin<true>(workspace, R, K);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (R > 0 && K > 0) {
        hipLaunchKernelGGL(k_iota, dim3(grid(R)), dim3(BLOCK), 0, st, a);
        size_t b = a.w.cub.bytes;
        if ((e = hipcub::DeviceSegmentedRadixSort::SortPairs(a.w.cub.ptr, b, a.best_key, a.w.keys, a.w.vin, a.w.vout, R, K,
                                                             batch->part_off, batch->part_off + 1, 0, 64, st)) != hipSuccess)
            return fail(who, "sort", e);
    }
    hipLaunchKernelGGL(k_count_ev, dim3(grid((int64_t)K + 1)), dim3(BLOCK), 0, st, a);
    if ((e = gtf::Cub{a.w.cub, st}.scan(a.w.cnt, rec_first, K + 1)) != hipSuccess) return fail(who, "scan", e);
    if (R > 0 && K > 0) hipLaunchKernelGGL(k_records_ev, dim3(grid(R)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t c[2] = {0, INT32_MAX};
    if ((e = hipMemcpyAsync(c, a.w.scal, sizeof(c), hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "counts", e);
    if (K > 0 && (e = hipMemcpyAsync(n_reconstructed, a.w.cnt, 4 * (size_t)K, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "counts", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    error[0] = (uint32_t)c[0];
    error[1] = (uint32_t)c[1];
    const char* what = nullptr;
    if (error[0] & GTF_SCORE_ERR_MISSING) what = "a candidate node has no hit_dissociation";
    else if (error[0] & GTF_SCORE_ERR_WORKSPACE) what = "a gtf_score_candidates_ev call had more members than its workspace holds";
    else if (error[0] & GTF_SCORE_ERR_RANGE)
        what = "a candidate of 2^31 or more particle entries, or a malformed cand_ptr or cand_first";
    if (what) {
        char m[240];
        if (c[1] >= 0 && c[1] < K) snprintf(m, sizeof(m), "gtf_score_finish_ev: event %d: %s", c[1], what);
        else snprintf(m, sizeof(m), "gtf_score_finish_ev: %s", what);
        for (int i = 0; i < K; i++) n_reconstructed[i] = 0;
        return bad(m);
    }
    int64_t sum = 0;
    for (int i = 0; i < K; i++) {
        if (n_reconstructed[i] < 0) return bad("gtf_score_finish_ev: inconsistent keys");
        sum += n_reconstructed[i];
    }
    if (sum > R) return bad("gtf_score_finish_ev: inconsistent keys");
    return 0;
}

}  // extern "C"
