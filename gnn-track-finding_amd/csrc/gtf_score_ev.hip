// gtf_score_ev.hip -- candidate scoring for a batch of events in one call (include/gtf.h:
// gtf_truth_concat, gtf_score_reset_ev, gtf_score_candidates_ev, gtf_score_finish_ev): what K
// calls of gtf_score.hip compute for the K events of a fused graph, in launch sequences whose
// length does not depend on K. The K truth tables lie end to end (ids of different events
// collide) and every lookup stays inside its own event's segment.
//
//   concat     1. one block: the exclusive sums of the parts' nodes, entries and particles
//              2. one launch over nodes (+ the closing pointer), entries and particles
//                 (blockIdx.y): a thread finds its part by a binary search over the offsets of
//                 its axis -- staged in LDS when they fit -- and copies its row, node_ptr
//                 shifted by the part's entry offset
//   reset      one launch: every key, or the keys of the marked events
//   candidates 0. per candidate its event (an upper bound over cand_first, staged in LDS when
//                 it fits; -1 for an unscored event or a broken cand_first), per event the
//                 checks of cand_first
//              1.-3. the launches of gtf_score.hip (members, exclusive sum, vote, winners) as
//                 sibling kernels: the member's and the particle's binary searches run inside
//                 the event's segment and the key holds the candidate's index inside its event.
//                 The vote itself is the code of gtf_score.hip, which stays as it is
//   finish     one segmented radix sort of the keys over part_off (unmatched keys, all-ones, last
//              in their segment); per event the number of matched keys; their exclusive sum;
//              one launch writes the records compacted; one synchronisation
//
// No same-address atomic except on a violation: the claims land on different words, the error
// words are touched only when the input is broken. Every read is clamped to the sums the host
// passed. Vector stores only.
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
constexpr int G = 16;                  // lanes of a small candidate's group
constexpr int PER_WAVE = 64 / G;       // candidates of a wavefront
constexpr int PER_BLOCK = PER_WAVE * (BLOCK / 64);
constexpr uint64_t NONE = ~uint64_t(0);
constexpr int32_t MAX_MEMBERS = 1 << 30;
constexpr int LDS_OFFS = 2048;         // offsets staged in LDS when K + 1 <= this (8 KiB)
constexpr int COPY_BLOCKS = 1024;      // blocks per axis of the concat's copy launch
constexpr int64_t LIMIT = (int64_t)1 << 31;

// the segment of row r: the largest p in [0, K) with off[p] <= r (empty segments share their
// successor's offset and are passed over); K >= 1
__device__ __forceinline__ int find_part(const int32_t* off, int K, int r) {
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// K + 1 offsets for this block: in LDS when they fit, else where they lie
__device__ __forceinline__ const int32_t* stage_offsets(const int32_t* off, int K, int32_t* lds) {
    if (K + 1 > LDS_OFFS) return off;
    for (int i = threadIdx.x; i <= K; i += BLOCK) lds[i] = off[i];
    __syncthreads();
    return lds;
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

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
    __shared__ int32_t lds[LDS_OFFS];
    const int axis = blockIdx.y;
    const int32_t* goff = axis == AX_NODE ? a.o.node_off : axis == AX_ENTRY ? a.o.entry_off : a.o.part_off;
    const int64_t rows = axis == AX_NODE ? (int64_t)a.T + 1 : axis == AX_ENTRY ? a.P : a.R;
    if (a.K == 0) {   // no part: the closing pointer alone
        if (axis == AX_NODE && blockIdx.x == 0 && threadIdx.x == 0) a.o.node_ptr[0] = 0;
        return;
    }
    const int32_t* off = stage_offsets(goff, a.K, lds);
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * BLOCK) {
        if (axis == AX_NODE && r == a.T) {
            a.o.node_ptr[a.T] = a.P;
            continue;
        }
        const int p = find_part(off, a.K, (int)r);
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
struct Ws {
    int32_t* c_event;                    // [n_cand] the candidate's event; -1: not scored
    int32_t *c_row, *c_good, *c_total;   // [n_cand] the passing candidate's particle row in the batch (-1: none), its counts
    int32_t* mrow;                       // [M + 1] start of the member's node_part row
    int64_t *mlen, *off;                 // [M + 1] its length; the exclusive sum
    gtf::Scratch cub;
    size_t total;
};

Ws carve(void* base, int64_t C, int64_t M) {
    Ws w;
    gtf::Arena a(base);
    const size_t c = (size_t)C, m1 = (size_t)M + 1;
    w.c_event = a.take<int32_t>(c);
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

struct Score {
    int32_t K, T, P, R;      // events; the batch's sums
    const int32_t *node_off, *part_off;
    const int64_t *node_id, *node_part, *part_id;
    const int32_t *node_ptr, *part_hits;
    const uint8_t *part_ref, *scored;
    const int32_t *cand_ptr, *cand_first;
    const int64_t* cand_ids;
    int32_t C, M;            // candidates; member capacity of the workspace
    uint32_t group;
    gtf_score_out o;
    uint64_t* best_key;
    int32_t *best_good, *best_total;
    uint32_t* error;         // [2]
    Ws w;
};

// a violation met in event e (e < 0: in no event)
__device__ __forceinline__ void violation(const Score& a, uint32_t bit, int e) {
    atomicOr(&a.error[0], bit);
    if (e >= 0) atomicMin((int32_t*)&a.error[1], e);
}

// the members in use: cand_ptr[C] clamped to the workspace's capacity
__device__ __forceinline__ int members(const Score& a) {
    const int m = a.cand_ptr[a.C];
    return m < 0 ? 0 : m > a.M ? a.M : m;
}

// ---- 0. the candidates' events ----
__global__ __launch_bounds__(BLOCK) void k_events(Score a) {
    __shared__ int32_t lds[LDS_OFFS];
    const int32_t* cf = stage_offsets(a.cand_first, a.K, lds);
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i <= a.K) {
        bool wrong = (i == 0 && cf[0] != 0) || (i == a.K && cf[a.K] != a.C);
        if (i < a.K) wrong |= cf[i] > cf[i + 1];
        if (wrong) violation(a, GTF_SCORE_ERR_RANGE, -1);
    }
    if (i >= a.C) return;
    int e = -1;
    if (a.K > 0) {
        e = find_part(cf, a.K, i);
        if (cf[e] > i || cf[e + 1] <= i) e = -1;   // (a broken cand_first, reported above: the candidate is skipped)
        else if (a.scored && !a.scored[e]) e = -1;
    }
    a.w.c_event[i] = e;
}

// ---- 1. members ----
__global__ __launch_bounds__(BLOCK) void k_members_ev(Score a) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m > a.M) return;
    const int nm = a.cand_ptr[a.C];
    if (m == 0 && (nm < 0 || nm > a.M)) violation(a, nm < 0 ? GTF_SCORE_ERR_RANGE : GTF_SCORE_ERR_WORKSPACE, -1);
    int row = 0, len = 0;
    if (m < nm) {
        const int c = find_part(a.cand_ptr, a.C, m);   // its candidate (empty ones are passed over)
        const int e = a.w.c_event[c];
        if (e >= 0) {
            const int64_t key = a.cand_ids[m];
            const int s0 = clampi(a.node_off[e], 0, a.T), s1 = clampi(a.node_off[e + 1], s0, a.T);
            int lo = s0, hi = s1;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (a.node_id[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            if (lo < s1 && a.node_id[lo] == key) {
                int b = a.node_ptr[lo], n = a.node_ptr[lo + 1];   // clamped: a malformed node_ptr reads nothing outside
                if (b < 0) b = 0;
                if (n > a.P) n = a.P;
                row = b;
                len = n > b ? n - b : 0;
            } else {
                violation(a, GTF_SCORE_ERR_MISSING, e);   // (only on a violation)
            }
        }
    }
    a.w.mrow[m] = row;
    a.w.mlen[m] = len;
}

// ---- 2. the vote (gtf_score.hip's, on the batch's node_part) ----
struct Cand {
    int lo, hi;       // its members
    int64_t base, n;  // off[lo]; its entries
};

// entry e (0 <= e < c.n) of the candidate: the member m with off[m] - base <= e < off[m + 1] - base
__device__ __forceinline__ int64_t entry(const Score& a, const Cand& c, int64_t e) {
    int l = c.lo, h = c.hi - 1;
    while (l < h) {
        const int mid = l + ((h - l + 1) >> 1);
        if (a.w.off[mid] - c.base <= e) l = mid;
        else h = mid - 1;
    }
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

__global__ __launch_bounds__(BLOCK) void k_vote_ev(Score a) {
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
    const int e = a.w.c_event[c];
    if (broken) violation(a, GTF_SCORE_ERR_RANGE, e);
    const int total = (int)cd.n;   // (0 for a candidate that is not scored: its members have no rows)
    int row = -1;
    if (total > 0 && e >= 0) {
        const int s0 = clampi(a.part_off[e], 0, a.R), s1 = clampi(a.part_off[e + 1], s0, a.R);
        int lo = s0, hi = s1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.part_id[mid] < best_id) lo = mid + 1;
            else hi = mid;
        }
        if (lo < s1 && a.part_id[lo] == best_id && a.part_ref[lo] && 2 * (int64_t)best_cnt >= a.part_hits[lo] &&
            2 * (int64_t)best_cnt >= total)
            row = lo;
    }
    if (row >= 0)
        atomicMin((unsigned long long*)&a.best_key[row],
                  ((unsigned long long)a.group << 32) | (uint32_t)(c - a.cand_first[e]));
    a.w.c_row[c] = row;
    a.w.c_good[c] = best_cnt;
    a.w.c_total[c] = total;
    if (a.o.pid) a.o.pid[c] = best_id;
    if (a.o.n_good) a.o.n_good[c] = best_cnt;
    if (a.o.total) a.o.total[c] = total;
    if (a.o.passes) a.o.passes[c] = row >= 0;
}

// ---- 3. the winners ----
__global__ __launch_bounds__(BLOCK) void k_winners_ev(Score a) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.C) return;
    const int row = a.w.c_row[c], e = a.w.c_event[c];
    if (row < 0 || row >= a.R || e < 0 || e >= a.K) return;
    if (a.best_key[row] != (((uint64_t)a.group << 32) | (uint32_t)(c - a.cand_first[e]))) return;
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
    const int e = find_part(part_off, K, r);
    if (part_off[e] <= r && r < part_off[e + 1] && events[e]) best_key[r] = NONE;
}

// ---- finish ----
struct FinWs {
    uint64_t* keys;          // [R] sorted inside every event's segment
    int32_t *vin, *vout;     // [R] particle rows
    int32_t *cnt, *scal;     // [K + 1] matched keys per event, a closing 0; [2] the error words
    gtf::Scratch cub;
    size_t total;
};

size_t segmented_sort_bytes(int R, int K) {
    size_t b = 0;
    (void)hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr,
                                                      (int32_t*)nullptr, R, K, (const int32_t*)nullptr,
                                                      (const int32_t*)nullptr);
    return b;
}

FinWs carve_fin(void* base, int64_t R, int64_t K) {
    FinWs w;
    gtf::Arena a(base);
    w.scal = a.take<int32_t>(16);
    w.cnt = a.take<int32_t>((size_t)K + 1);
    w.keys = a.take<uint64_t>((size_t)R);
    w.vin = a.take<int32_t>((size_t)R);
    w.vout = a.take<int32_t>((size_t)R);
    // (one piece serves the sort and the scan: the larger of the two)
    size_t bytes = segmented_sort_bytes((int)R, (int)K), scan = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int32_t*)nullptr, (int32_t*)nullptr, (int)K + 1);
    if (scan > bytes) bytes = scan;
    w.cub = gtf::Scratch{a.take<char>(bytes), bytes};
    w.total = a.used();
    return w;
}

struct Fin {
    int32_t R, K;
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

__global__ __launch_bounds__(BLOCK) void k_iota_ev(Fin a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r < a.R) a.w.vin[r] = r;
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
        const int s0 = clampi(a.part_off[e], 0, a.R), s1 = clampi(a.part_off[e + 1], s0, a.R);
        int lo = s0, hi = s1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.w.keys[mid] != NONE) lo = mid + 1;
            else hi = mid;
        }
        n = lo - s0;
    }
    a.w.cnt[e] = n;
}

__global__ __launch_bounds__(BLOCK) void k_records_ev(Fin a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.R || a.K <= 0) return;
    const int e = find_part(a.part_off, a.K, i);
    const int j = i - a.part_off[e];
    if (j < 0 || j >= a.w.cnt[e]) return;
    const int64_t at = (int64_t)a.rec_first[e] + j;
    if (at < 0 || at >= a.R) return;
    const int r = a.w.vout[i];
    if (r < 0 || r >= a.R) return;
    if (a.out_key) a.out_key[at] = a.w.keys[i];
    if (a.out_pid) a.out_pid[at] = a.part_id[r];
    if (a.out_good) a.out_good[at] = a.best_good[r];
    if (a.out_total) a.out_total[at] = a.best_total[r];
    if (a.out_hits) a.out_hits[at] = a.part_hits[r];
}

// the gtf_truth_batch of another layout of include/gtf.h: -3; a null or inconsistent one: -2
int check_batch(const gtf_truth_batch* t, const char* who) {
    char m[220];
    if (int rc = gtf::check_abi(t, who, "gtf_truth_batch", "gtf_truth_batch")) return rc;
    if (t->n_events < 0 || t->n_nodes < 0 || t->n_entries < 0 || t->n_particles < 0) {
        snprintf(m, sizeof(m), "%s: negative sizes in gtf_truth_batch", who);
        return bad(m);
    }
    const char* miss = nullptr;
    if (!t->node_off || !t->entry_off || !t->part_off) miss = "node_off, entry_off or part_off";
    else if (t->n_nodes > 0 && !t->node_id) miss = "node_id";
    else if (!t->node_ptr) miss = "node_ptr";
    else if (t->n_entries > 0 && !t->node_part) miss = "node_part";
    else if (t->n_particles > 0 && !t->part_id) miss = "part_id";
    else if (t->n_particles > 0 && !t->part_hits) miss = "part_hits";
    else if (t->n_particles > 0 && !t->part_ref) miss = "part_ref";
    if (miss) {
        snprintf(m, sizeof(m), "%s: missing gtf_truth_batch array %s", who, miss);
        return bad(m);
    }
    return 0;
}

int check_state(const gtf_score_state_ev* s, const gtf_truth_batch* t, const char* who) {
    char m[200];
    if (int rc = gtf::check_abi(s, who, "gtf_score_state_ev", "gtf_score_state_ev")) return rc;
    const char* what = nullptr;
    if (s->n_particles < 0) what = "negative n_particles in gtf_score_state_ev";
    else if (!s->error) what = "missing gtf_score_state_ev array error";
    else if (s->n_particles > 0 && (!s->best_key || !s->best_good || !s->best_total))
        what = "missing gtf_score_state_ev array (best_key, best_good, best_total)";
    else if (s->n_particles != t->n_particles) what = "gtf_score_state_ev.n_particles differs from gtf_truth_batch.n_particles";
    if (!what) return 0;
    snprintf(m, sizeof(m), "%s: %s", who, what);
    return bad(m);
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

int gtf_score_reset_ev(const gtf_score_state_ev* state, const gtf_truth_batch* batch, const uint8_t* events,
                       gtf_stream_t stream) {
    const char* who = "gtf_score_reset_ev";
    if (int rc = check_batch(batch, who)) return rc;
    if (int rc = check_state(state, batch, who)) return rc;
    const int32_t R = state->n_particles;
    if (events && R == 0) return 0;
    hipLaunchKernelGGL(k_reset_ev, dim3(grid(R > 0 ? R : 1)), dim3(BLOCK), 0, (hipStream_t)stream, state->best_key,
                       state->error, (int)R, (int)batch->n_events, batch->part_off, events);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

size_t gtf_score_ev_workspace_bytes(int32_t n_cand, int32_t n_members, int32_t n_events) {
    (void)n_events;   // (cand_first is read where it lies)
    return carve(nullptr, n_cand > 0 ? n_cand : 0, n_members > 0 ? n_members : 0).total;
}

size_t gtf_score_finish_ev_workspace_bytes(int32_t n_particles, int32_t n_events) {
    return carve_fin(nullptr, n_particles > 0 ? n_particles : 0, n_events > 0 ? n_events : 0).total;
}

int gtf_score_candidates_ev(const gtf_truth_batch* batch, const int32_t* cand_ptr, const int64_t* cand_ids,
                            const int32_t* cand_first, int32_t n_cand, int32_t group, const gtf_score_out* out,
                            const gtf_score_state_ev* state, void* workspace, size_t workspace_bytes,
                            gtf_stream_t stream) {
    const char* who = "gtf_score_candidates_ev";
    if (int rc = check_batch(batch, who)) return rc;
    if (int rc = check_state(state, batch, who)) return rc;
    if (n_cand < 0) return bad("gtf_score_candidates_ev: negative n_cand");
    if (group < 0) return bad("gtf_score_candidates_ev: negative group");
    if (n_cand == 0) return 0;
    if (n_cand > INT32_MAX - PER_BLOCK) return bad("gtf_score_candidates_ev: too many candidates");
    if (!cand_ptr) return bad("gtf_score_candidates_ev: missing array cand_ptr");
    if (!cand_ids) return bad("gtf_score_candidates_ev: missing array cand_ids");
    if (!cand_first) return bad("gtf_score_candidates_ev: missing array cand_first");
    const int32_t K = batch->n_events;
    if (!workspace || workspace_bytes < gtf_score_ev_workspace_bytes(n_cand, 0, K))
        return bad("gtf_score_candidates_ev: workspace smaller than gtf_score_ev_workspace_bytes");
    // the member capacity of this workspace: the largest M that fits (the size is non-decreasing in M)
    int32_t lo = 0, hi = MAX_MEMBERS;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (gtf_score_ev_workspace_bytes(n_cand, mid, K) <= workspace_bytes) lo = mid;
        else hi = mid - 1;
    }
    Score a;
    a.K = K; a.T = batch->n_nodes; a.P = batch->n_entries; a.R = batch->n_particles;
    a.node_off = batch->node_off; a.part_off = batch->part_off;
    a.node_id = batch->node_id; a.node_part = batch->node_part; a.part_id = batch->part_id;
    a.node_ptr = batch->node_ptr; a.part_hits = batch->part_hits; a.part_ref = batch->part_ref;
    a.scored = batch->scored;
    a.cand_ptr = cand_ptr; a.cand_ids = cand_ids; a.cand_first = cand_first;
    a.C = n_cand; a.M = lo; a.group = (uint32_t)group;
    a.o = out ? *out : gtf_score_out{nullptr, nullptr, nullptr, nullptr};
    a.best_key = state->best_key; a.best_good = state->best_good; a.best_total = state->best_total;
    a.error = state->error;
    a.w = carve(workspace, n_cand, a.M);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const int64_t first = (int64_t)K + 1 > n_cand ? (int64_t)K + 1 : n_cand;
    hipLaunchKernelGGL(k_events, dim3(grid(first)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_members_ev, dim3(grid((int64_t)a.M + 1)), dim3(BLOCK), 0, st, a);
    if ((e = gtf::Cub{a.w.cub, st}.scan(a.w.mlen, a.w.off, a.M + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_vote_ev, dim3((n_cand + PER_BLOCK - 1) / PER_BLOCK), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_winners_ev, dim3(grid(n_cand)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_score_finish_ev(const gtf_truth_batch* batch, const gtf_score_state_ev* state, uint64_t* out_key,
                        int64_t* out_pid, int32_t* out_good, int32_t* out_total, int32_t* out_hits,
                        int32_t* rec_first, int32_t* n_reconstructed, uint32_t* error, void* workspace,
                        size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_score_finish_ev";
    if (int rc = check_batch(batch, who)) return rc;
    if (int rc = check_state(state, batch, who)) return rc;
    const int32_t R = batch->n_particles, K = batch->n_events;
    if (!rec_first) return bad("gtf_score_finish_ev: null rec_first");
    if (!error || (K > 0 && !n_reconstructed)) return bad("gtf_score_finish_ev: null counts");
    if (!workspace || workspace_bytes < gtf_score_finish_ev_workspace_bytes(R, K))
        return bad("gtf_score_finish_ev: workspace smaller than gtf_score_finish_ev_workspace_bytes");
    for (int i = 0; i < K; i++) n_reconstructed[i] = 0;
    error[0] = 0;
    error[1] = (uint32_t)INT32_MAX;
    Fin a;
    a.R = R; a.K = K;
    a.part_off = batch->part_off; a.part_id = batch->part_id; a.part_hits = batch->part_hits;
    a.best_good = state->best_good; a.best_total = state->best_total; a.best_key = state->best_key;
    a.error = state->error;
    a.out_key = out_key; a.out_pid = out_pid; a.out_good = out_good; a.out_total = out_total; a.out_hits = out_hits;
    a.rec_first = rec_first;
    a.w = carve_fin(workspace, R, K);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (R > 0 && K > 0) {
        hipLaunchKernelGGL(k_iota_ev, dim3(grid(R)), dim3(BLOCK), 0, st, a);
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
