// gtf_score.hip -- candidate scoring on the GPU (include/gtf.h: gtf_score_reset,
// gtf_score_candidates, gtf_score_finish): src/extract/reconstruction_efficiency.py:118-183
// (gtf/metrics.py candidate_particles, majority, reconstruction_efficiency) on the device
// arrays gtf_extract_outputs leaves, accumulated over the iterations of the loop.
//
//   candidates 1. per member: binary search of its id in truth.node_id (as find_id in
//                 gtf_pyset.h); the start of its node_part row and the row's length. hipCUB
//                 exclusive sum of the lengths: candidate c's entries are
//                 off[cand_ptr[c]] .. off[cand_ptr[c + 1]], never materialised
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
//                 up, applies the thresholds and claims part r with a 64-bit atomicMin on
//                 best_key[r]
//              3. per passing candidate: the one whose key is the stored one writes
//                 best_good / best_total
//   finish     radix sort of the R (key, particle) pairs, unmatched keys (all-ones) last; one
//              launch writes the records and the count; one synchronisation
//
// No same-address atomic: the claims land on R different words and the error word is touched
// only when the input is broken. Vector stores only.
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

struct Ws {
    int32_t *c_row, *c_good, *c_total;   // [n_cand] the passing candidate's particle row (-1: none), its counts
    int32_t* mrow;                       // [M + 1] start of the member's node_part row
    int64_t *mlen, *off;                 // [M + 1] its length; the exclusive sum
    gtf::Scratch cub;
    size_t total;
};

Ws carve(void* base, int64_t C, int64_t M) {
    Ws w;
    gtf::Arena a(base);
    const size_t c = (size_t)C, m1 = (size_t)M + 1;
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

struct FinWs {
    uint64_t* keys;          // [R] sorted
    int32_t *vin, *vout;     // [R] particle rows
    int32_t* scal;           // [2] n_reconstructed, error
    gtf::Scratch cub;
    size_t total;
};

FinWs carve_fin(void* base, int64_t R) {
    FinWs w;
    gtf::Arena a(base);
    w.scal = a.take<int32_t>(16);
    w.keys = a.take<uint64_t>((size_t)R);
    w.vin = a.take<int32_t>((size_t)R);
    w.vout = a.take<int32_t>((size_t)R);
    w.cub = gtf::CubNeed().sort_pairs<uint64_t, int32_t>((int)R).take(a);
    w.total = a.used();
    return w;
}

struct Score {
    int32_t T, P, R;
    const int64_t *node_id, *node_part, *part_id;
    const int32_t *node_ptr, *part_hits;
    const uint8_t* part_ref;
    const int32_t* cand_ptr;
    const int64_t* cand_ids;
    int32_t C, M;            // candidates; member capacity of the workspace
    uint32_t group;
    gtf_score_out o;
    uint64_t* best_key;
    int32_t *best_good, *best_total;
    uint32_t* error;
    Ws w;
};

// the members in use: cand_ptr[C] clamped to the workspace's capacity
__device__ __forceinline__ int members(const Score& a) {
    const int m = a.cand_ptr[a.C];
    return m < 0 ? 0 : m > a.M ? a.M : m;
}

// ---- 1. members ----
__global__ __launch_bounds__(BLOCK) void k_members(Score a) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m > a.M) return;
    const int nm = a.cand_ptr[a.C];
    if (m == 0 && (nm < 0 || nm > a.M)) atomicOr(a.error, nm < 0 ? GTF_SCORE_ERR_RANGE : GTF_SCORE_ERR_WORKSPACE);
    int row = 0, len = 0;
    if (m < nm) {
        const int64_t key = a.cand_ids[m];
        int lo = 0, hi = a.T;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.node_id[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        if (lo < a.T && a.node_id[lo] == key) {
            int b = a.node_ptr[lo], e = a.node_ptr[lo + 1];   // clamped: a malformed node_ptr reads nothing outside
            if (b < 0) b = 0;
            if (e > a.P) e = a.P;
            row = b;
            len = e > b ? e - b : 0;
        } else {
            atomicOr(a.error, GTF_SCORE_ERR_MISSING);   // (only on a violation)
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
    if (broken) atomicOr(a.error, GTF_SCORE_ERR_RANGE);
    const int total = (int)cd.n;
    int row = -1;
    if (total > 0) {
        int lo = 0, hi = a.R;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (a.part_id[mid] < best_id) lo = mid + 1;
            else hi = mid;
        }
        if (lo < a.R && a.part_id[lo] == best_id && a.part_ref[lo] && 2 * (int64_t)best_cnt >= a.part_hits[lo] &&
            2 * (int64_t)best_cnt >= total)
            row = lo;
    }
    if (row >= 0) atomicMin((unsigned long long*)&a.best_key[row], ((unsigned long long)a.group << 32) | (uint32_t)c);
    a.w.c_row[c] = row;
    a.w.c_good[c] = best_cnt;
    a.w.c_total[c] = total;
    if (a.o.pid) a.o.pid[c] = best_id;
    if (a.o.n_good) a.o.n_good[c] = best_cnt;
    if (a.o.total) a.o.total[c] = total;
    if (a.o.passes) a.o.passes[c] = row >= 0;
}

// ---- 3. the winners ----
__global__ __launch_bounds__(BLOCK) void k_winners(Score a) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= a.C) return;
    const int row = a.w.c_row[c];
    if (row < 0 || row >= a.R) return;
    if (a.best_key[row] != (((uint64_t)a.group << 32) | (uint32_t)c)) return;
    a.best_good[row] = a.w.c_good[c];
    a.best_total[row] = a.w.c_total[c];
}

// ---- finish ----
struct Fin {
    int32_t R;
    const int64_t* part_id;
    const int32_t *part_hits, *best_good, *best_total;
    const uint64_t* best_key;
    const uint32_t* error;
    uint64_t* out_key;
    int64_t* out_pid;
    int32_t *out_good, *out_total, *out_hits;
    FinWs w;
};

__global__ __launch_bounds__(BLOCK) void k_iota(Fin a) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r < a.R) a.w.vin[r] = r;
}

__global__ __launch_bounds__(BLOCK) void k_records(Fin a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) {
        a.w.scal[1] = (int32_t)*a.error;
        if (a.R == 0 || a.w.keys[0] == NONE) a.w.scal[0] = 0;
    }
    if (i >= a.R) return;
    const uint64_t key = a.w.keys[i];
    if (key == NONE) return;
    if (i == a.R - 1 || a.w.keys[i + 1] == NONE) a.w.scal[0] = i + 1;   // (the last matched one: the only writer)
    const int r = a.w.vout[i];
    if (r < 0 || r >= a.R) return;
    if (a.out_key) a.out_key[i] = key;
    if (a.out_pid) a.out_pid[i] = a.part_id[r];
    if (a.out_good) a.out_good[i] = a.best_good[r];
    if (a.out_total) a.out_total[i] = a.best_total[r];
    if (a.out_hits) a.out_hits[i] = a.part_hits[r];
}

// the gtf_truth of another layout of include/gtf.h: -3; a null or inconsistent one: -2
int check_truth(const gtf_truth* t, const char* who) {
    char m[220];
    if (int rc = gtf::check_abi(t, who, "gtf_truth", "gtf_truth")) return rc;
    if (t->n_nodes < 0 || t->n_entries < 0 || t->n_particles < 0) {
        snprintf(m, sizeof(m), "%s: negative sizes in gtf_truth", who);
        return bad(m);
    }
    const char* miss = nullptr;
    if (t->n_nodes > 0 && !t->node_id) miss = "node_id";
    else if (!t->node_ptr) miss = "node_ptr";
    else if (t->n_entries > 0 && !t->node_part) miss = "node_part";
    else if (t->n_particles > 0 && !t->part_id) miss = "part_id";
    else if (t->n_particles > 0 && !t->part_hits) miss = "part_hits";
    else if (t->n_particles > 0 && !t->part_ref) miss = "part_ref";
    if (miss) {
        snprintf(m, sizeof(m), "%s: missing gtf_truth array %s", who, miss);
        return bad(m);
    }
    return 0;
}

int check_state(const gtf_score_state* s, const char* who) {
    char m[160];
    const char* what = nullptr;
    if (!s) what = "null gtf_score_state";
    else if (s->n_particles < 0) what = "negative n_particles in gtf_score_state";
    else if (!s->error) what = "missing gtf_score_state array error";
    else if (s->n_particles > 0 && (!s->best_key || !s->best_good || !s->best_total))
        what = "missing gtf_score_state array (best_key, best_good, best_total)";
    if (!what) return 0;
    snprintf(m, sizeof(m), "%s: %s", who, what);
    return bad(m);
}

}  // namespace

extern "C" {

int gtf_score_reset(const gtf_score_state* state, gtf_stream_t stream) {
    const char* who = "gtf_score_reset";
    if (int rc = check_state(state, who)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (state->n_particles > 0 &&
        (e = hipMemsetAsync(state->best_key, 0xff, 8 * (size_t)state->n_particles, st)) != hipSuccess)
        return fail(who, "memset", e);
    if ((e = hipMemsetAsync(state->error, 0, 4, st)) != hipSuccess) return fail(who, "memset", e);
    return 0;
}

size_t gtf_score_workspace_bytes(int32_t n_cand, int32_t n_members) {
    return carve(nullptr, n_cand > 0 ? n_cand : 0, n_members > 0 ? n_members : 0).total;
}

size_t gtf_score_finish_workspace_bytes(int32_t n_particles) {
    return carve_fin(nullptr, n_particles > 0 ? n_particles : 0).total;
}

int gtf_score_candidates(const gtf_truth* truth, const int32_t* cand_ptr, const int64_t* cand_ids,
                         int32_t n_cand, int32_t group, const gtf_score_out* out,
                         const gtf_score_state* state, void* workspace, size_t workspace_bytes,
                         gtf_stream_t stream) {
    const char* who = "gtf_score_candidates";
    if (int rc = check_truth(truth, who)) return rc;
    if (int rc = check_state(state, who)) return rc;
    if (state->n_particles != truth->n_particles)
        return bad("gtf_score_candidates: gtf_score_state.n_particles differs from gtf_truth.n_particles");
    if (n_cand < 0) return bad("gtf_score_candidates: negative n_cand");
    if (group < 0) return bad("gtf_score_candidates: negative group");
    if (n_cand == 0) return 0;
    if (n_cand > INT32_MAX - PER_BLOCK) return bad("gtf_score_candidates: too many candidates");
    if (!cand_ptr) return bad("gtf_score_candidates: missing array cand_ptr");
    if (!cand_ids) return bad("gtf_score_candidates: missing array cand_ids");
    if (!workspace || workspace_bytes < gtf_score_workspace_bytes(n_cand, 0))
        return bad("gtf_score_candidates: workspace smaller than gtf_score_workspace_bytes");
    // the member capacity of this workspace: the largest M that fits (the size is non-decreasing in M)
    int32_t lo = 0, hi = MAX_MEMBERS;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (gtf_score_workspace_bytes(n_cand, mid) <= workspace_bytes) lo = mid;
        else hi = mid - 1;
    }
    Score a;
    a.T = truth->n_nodes; a.P = truth->n_entries; a.R = truth->n_particles;
    a.node_id = truth->node_id; a.node_part = truth->node_part; a.part_id = truth->part_id;
    a.node_ptr = truth->node_ptr; a.part_hits = truth->part_hits; a.part_ref = truth->part_ref;
    a.cand_ptr = cand_ptr; a.cand_ids = cand_ids;
    a.C = n_cand; a.M = lo; a.group = (uint32_t)group;
    a.o = out ? *out : gtf_score_out{nullptr, nullptr, nullptr, nullptr};
    a.best_key = state->best_key; a.best_good = state->best_good; a.best_total = state->best_total;
    a.error = state->error;
    a.w = carve(workspace, n_cand, a.M);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    hipLaunchKernelGGL(k_members, dim3(grid((int64_t)a.M + 1)), dim3(BLOCK), 0, st, a);
    if ((e = gtf::Cub{a.w.cub, st}.scan(a.w.mlen, a.w.off, a.M + 1)) != hipSuccess) return fail(who, "scan", e);
    hipLaunchKernelGGL(k_vote, dim3((n_cand + PER_BLOCK - 1) / PER_BLOCK), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_winners, dim3(grid(n_cand)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_score_finish(const gtf_truth* truth, const gtf_score_state* state, uint64_t* out_key,
                     int64_t* out_pid, int32_t* out_good, int32_t* out_total, int32_t* out_hits,
                     gtf_score_counts* counts, void* workspace, size_t workspace_bytes,
                     gtf_stream_t stream) {
    const char* who = "gtf_score_finish";
    if (int rc = check_truth(truth, who)) return rc;
    if (int rc = check_state(state, who)) return rc;
    if (state->n_particles != truth->n_particles)
        return bad("gtf_score_finish: gtf_score_state.n_particles differs from gtf_truth.n_particles");
    if (!counts) return bad("gtf_score_finish: null counts");
    const int32_t R = truth->n_particles;
    if (!workspace || workspace_bytes < gtf_score_finish_workspace_bytes(R))
        return bad("gtf_score_finish: workspace smaller than gtf_score_finish_workspace_bytes");
    counts->n_reconstructed = 0;
    counts->error = 0;
    Fin a;
    a.R = R;
    a.part_id = truth->part_id; a.part_hits = truth->part_hits;
    a.best_good = state->best_good; a.best_total = state->best_total; a.best_key = state->best_key;
    a.error = state->error;
    a.out_key = out_key; a.out_pid = out_pid; a.out_good = out_good; a.out_total = out_total; a.out_hits = out_hits;
    a.w = carve_fin(workspace, R);
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

}  // extern "C"
