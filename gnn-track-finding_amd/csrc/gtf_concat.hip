// gtf_concat.hip -- a batch of resident events as one graph, and one extraction's outputs per
// event again (include/gtf.h: gtf_graph_concat, gtf_concat_columns, gtf_event_split): the device
// form of gtf/graph.py concat. Subgraphs of different events share no edge, so the stages of
// run_gnn_trackml_mod.sh compute on the fused graph what they compute on every event, and the
// per-iteration synchronisations of the resident loop are paid once for the batch.
//
//   concat   1. one block: the exclusive sums of the parts' nodes, slots, out-edges and
//               subgraphs, [4][K + 1] in the workspace
//            2. one launch over nodes, slots and out-edges (blockIdx.y): a thread finds its
//               part by a binary search over the K + 1 offsets of its axis -- staged in LDS
//               when they fit -- and writes its entry of the structure arrays shifted by the
//               part's offsets; event[v] = the part
//   columns  up to MAXC payload columns per launch (the column table in the kernel
//            arguments, blockIdx.y = column, the per-part source pointers in a device table):
//            per tile of BLOCK rows the part and the row inside it once per row, then
//            consecutive lanes on consecutive destination words, 8-byte words where the rows
//            allow
//   split    per list the first group of every event (a lower bound over the events of the
//            groups' first members), the checks of what that rule relies on, then the counts
//            and the rebased candidate pointers of every event
//
// Every read of a part is guarded by the part's own size and every write by the summed sizes
// the host passed, so a device table that disagrees with the host's sizes, or a list that is
// not of the expected form, writes nothing outside the outputs. Vector stores only; the one
// atomic is the split's error word, touched only on a violation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/gtf.h"
#include "gtf_host.h"
#include "gtf_search.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int MAXC = GTF_CONCAT_MAX_COLUMNS;
constexpr int COPY_BLOCKS = 4096;     // blocks of a column launch, over its columns (16 a CU)
constexpr int STRUCT_BLOCKS = 1024;   // blocks per axis of the structure launch
constexpr int64_t LIMIT = (int64_t)1 << 31;

enum { AX_NODE = 0, AX_SLOT = 1, AX_EDGE = 2, AX_SUB = 3, AXES = 4 };

struct Ws {
    int32_t* off;   // [AXES][K + 1]
    size_t total;
};

Ws carve(const void* base, int64_t K) {
    Ws w;
    gtf::Arena a(base);
    w.off = a.take<int32_t>((size_t)AXES * ((size_t)K + 1));
    w.total = a.used();
    return w;
}

// ---- offsets ----
__device__ __forceinline__ int32_t part_size(const gtf_concat_part& p, int axis) {
    const int32_t n = axis == AX_NODE ? p.n_nodes : axis == AX_SLOT ? p.n_slots : axis == AX_EDGE ? p.n_edges : p.n_sub;
    return n > 0 ? n : 0;
}

// one block: chunks of BLOCK parts, an inclusive scan in LDS per axis and a running carry
__global__ __launch_bounds__(BLOCK) void k_offsets(const gtf_concat_part* parts, int K, int32_t* off) {
    __shared__ int64_t s[AXES][BLOCK];
    const int t = threadIdx.x;
    int64_t carry[AXES] = {0, 0, 0, 0};
    for (int base = 0; base < K; base += BLOCK) {
        const int i = base + t;
        int64_t v[AXES];
        for (int a = 0; a < AXES; a++) s[a][t] = v[a] = i < K ? part_size(parts[i], a) : 0;
        __syncthreads();
        for (int d = 1; d < BLOCK; d <<= 1) {
            int64_t add[AXES];
            for (int a = 0; a < AXES; a++) add[a] = t >= d ? s[a][t - d] : 0;
            __syncthreads();
            for (int a = 0; a < AXES; a++) s[a][t] += add[a];
            __syncthreads();
        }
        for (int a = 0; a < AXES; a++) {
            const int64_t o = carry[a] + s[a][t] - v[a];
            if (i < K) off[(size_t)a * (K + 1) + i] = o < LIMIT ? (int32_t)o : INT32_MAX;
            carry[a] += s[a][BLOCK - 1];
        }
        __syncthreads();
    }
    if (t < AXES) off[(size_t)t * (K + 1) + K] = carry[t] < LIMIT ? (int32_t)carry[t] : INT32_MAX;
}

// ---- structure arrays ----
struct Struct {
    int32_t K, N, S, E;   // the host's sums: no write beyond them
    const gtf_concat_part* parts;
    const int32_t* off;
    gtf_concat_out o;
};

__global__ __launch_bounds__(BLOCK) void k_struct(Struct a) {
    __shared__ int32_t lds[gtf::LDS_OFFS];
    const int axis = blockIdx.y, K1 = a.K + 1;
    const int32_t* noff = a.off + (size_t)AX_NODE * K1;
    const int32_t* soff = a.off + (size_t)AX_SLOT * K1;
    const int32_t* eoff = a.off + (size_t)AX_EDGE * K1;
    const int32_t* boff = a.off + (size_t)AX_SUB * K1;
    const int32_t* off = gtf::stage_offsets<BLOCK>(a.off + (size_t)axis * K1, a.K, lds);
    const int64_t rows = axis == AX_NODE ? (int64_t)a.N + 1 : axis == AX_SLOT ? a.S : a.E;
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * BLOCK) {
        if (axis == AX_NODE && r == a.N) {   // the closing pointers
            if (a.o.slot_ptr) a.o.slot_ptr[a.N] = a.S;
            if (a.o.out_ptr) a.o.out_ptr[a.N] = a.E;
            continue;
        }
        const int p = gtf::segment_of(off, a.K, (int)r);
        const int l = (int)r - off[p];
        const gtf_concat_part q = a.parts[p];
        if (l < 0 || l >= part_size(q, axis)) continue;   // (the device table disagrees with the host's sums)
        if (axis == AX_NODE) {
            // (graph.concat starts every part at the sum before it, whatever the part's slot_ptr[0])
            if (a.o.slot_ptr) a.o.slot_ptr[r] = l == 0 ? soff[p] : q.slot_ptr[l] + soff[p];
            if (a.o.out_ptr) a.o.out_ptr[r] = l == 0 ? eoff[p] : q.out_ptr[l] + eoff[p];
            if (a.o.sub_id) a.o.sub_id[r] = q.sub_id[l] + boff[p];
            if (a.o.event) a.o.event[r] = p;
        } else if (axis == AX_SLOT) {
            if (a.o.slot_src) {
                const int32_t s = q.slot_src[l];
                a.o.slot_src[r] = s >= 0 ? s + noff[p] : -1;   // (an orphan key stays one)
            }
        } else if (a.o.out_slot) {
            a.o.out_slot[r] = q.out_slot[l] + soff[p];
        }
    }
}

// ---- payload columns ----
struct Col {
    const void* const* src;   // device: [K] pointers
    void* dst;
    int32_t words;            // per row
    int32_t mode;             // axis | log2(word bytes) << 8
};
struct ColTab {
    Col c[MAXC];
};

// rows r0 .. r0 + BLOCK of one column: the part and the row inside it once per row, then lane t on
// destination words t, t + BLOCK, ... of the tile's W * BLOCK consecutive words
template <typename T, int WC>
__device__ __forceinline__ void copy_tiles(const Col& c, const int32_t* off, int K, int64_t rows, int32_t* s_part,
                                           int32_t* s_row) {
    const int W = WC > 0 ? WC : c.words;
    T* dst = (T*)c.dst;
    for (int64_t r0 = (int64_t)blockIdx.x * BLOCK; r0 < rows; r0 += (int64_t)gridDim.x * BLOCK) {
        const int n = rows - r0 < BLOCK ? (int)(rows - r0) : BLOCK;
        if ((int)threadIdx.x < n) {
            const int r = (int)r0 + threadIdx.x;
            const int p = gtf::segment_of(off, K, r);
            const int l = r - off[p];
            s_part[threadIdx.x] = l >= 0 && l < off[p + 1] - off[p] ? p : -1;
            s_row[threadIdx.x] = l;
        }
        __syncthreads();
        // (a constant width keeps the index arithmetic in 32 bits; any other row may be long)
        using I = typename std::conditional<(WC > 0), int, int64_t>::type;
        for (I f = threadIdx.x; f < (I)n * W; f += BLOCK) {
            const I row = f / W, w = f - row * W;
            const int p = s_part[row];
            if (p < 0) continue;
            const T* src = (const T*)c.src[p];
            dst[r0 * W + f] = src[(int64_t)s_row[row] * W + w];
        }
        __syncthreads();
    }
}

template <typename T>
__device__ __forceinline__ void copy_words(const Col& c, const int32_t* off, int K, int64_t rows, int32_t* s_part,
                                           int32_t* s_row) {
    switch (c.words) {   // (block-uniform: the usual row widths get a constant divisor)
    case 1: copy_tiles<T, 1>(c, off, K, rows, s_part, s_row); break;
    case 2: copy_tiles<T, 2>(c, off, K, rows, s_part, s_row); break;
    case 3: copy_tiles<T, 3>(c, off, K, rows, s_part, s_row); break;
    case 4: copy_tiles<T, 4>(c, off, K, rows, s_part, s_row); break;
    case 5: copy_tiles<T, 5>(c, off, K, rows, s_part, s_row); break;
    default: copy_tiles<T, 0>(c, off, K, rows, s_part, s_row);
    }
}

__global__ __launch_bounds__(BLOCK) void k_columns(const int32_t* offs, int K, int N, int S, ColTab tab) {
    __shared__ int32_t lds[gtf::LDS_OFFS];
    __shared__ int32_t s_part[BLOCK], s_row[BLOCK];
    const Col c = tab.c[blockIdx.y];
    const int axis = c.mode & 0xff, lg = c.mode >> 8;
    const int64_t rows = axis == 0 ? N : S;
    const int32_t* off = gtf::stage_offsets<BLOCK>(offs + (size_t)(axis == 0 ? AX_NODE : AX_SLOT) * (K + 1), K, lds);
    if (lg == 3) copy_words<uint64_t>(c, off, K, rows, s_part, s_row);
    else if (lg == 2) copy_words<uint32_t>(c, off, K, rows, s_part, s_row);
    else copy_words<uint8_t>(c, off, K, rows, s_part, s_row);
}

// ---- split ----
constexpr int LISTS = 3;

struct List {
    const int32_t *ptr, *mem;
    int32_t n_groups, n_members;
    int32_t* first;   // [K + 1]
};

struct Split {
    int32_t N, K;
    const int32_t* event;
    List l[LISTS];
    int32_t *counts, *cand_ptr_ev, *err;
};

// the event of group g's first member; INT32_MAX where the list gives none (k_split_check reports it)
__device__ __forceinline__ int32_t group_event(const Split& a, const List& l, int g) {
    const int32_t m = l.ptr[g];
    if (m < 0 || m >= l.n_members) return INT32_MAX;
    const int32_t v = l.mem[m];
    return v >= 0 && v < a.N ? a.event[v] : INT32_MAX;
}

__global__ __launch_bounds__(BLOCK) void k_split_first(Split a) {
    const List l = a.l[blockIdx.y];
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e > a.K) return;
    int lo = 0, hi = l.n_groups;   // the first group whose event is at least e
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (group_event(a, l, mid) < e) lo = mid + 1;
        else hi = mid;
    }
    l.first[e] = lo;
}

// what the lower bounds rely on, per group and per member
__global__ __launch_bounds__(BLOCK) void k_split_check(Split a) {
    const List l = a.l[blockIdx.y];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    bool wrong = false;
    if (i < l.n_groups) {
        const int32_t b = l.ptr[i], e = l.ptr[i + 1];
        wrong |= b < 0 || e > l.n_members || b >= e;                         // in the counts, with a member
        wrong |= (i == 0 && b != 0) || (i == l.n_groups - 1 && e != l.n_members);
        if (i > 0) {
            const int32_t ev = group_event(a, l, i), before = group_event(a, l, i - 1);
            wrong |= ev == INT32_MAX || before == INT32_MAX || ev < before;   // events ascend
        }
    }
    if (i < l.n_members) {
        const int32_t v = l.mem[i];
        if (v < 0 || v >= a.N) wrong = true;
        else {
            const int32_t ev = a.event[v];
            wrong |= ev < 0 || ev >= a.K;
            const int lo = gtf::segment_of(l.ptr, l.n_groups, i);   // the member's group
            wrong |= l.n_groups <= 0 || group_event(a, l, lo) != ev;          // one event per group
        }
    }
    if (wrong) atomicOr(a.err, 1);
}

// members before group g (g clamped into the list; 0 for an empty list)
__device__ __forceinline__ int32_t members_before(const List& l, int g) {
    if (l.n_groups <= 0) return 0;
    return l.ptr[g < 0 ? 0 : g > l.n_groups ? l.n_groups : g];
}

__global__ __launch_bounds__(BLOCK) void k_split_finish(Split a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < a.K) {
        for (int j = 0; j < LISTS; j++) {
            const List& l = a.l[j];
            const int32_t f0 = l.first[i], f1 = l.first[i + 1];
            a.counts[6 * i + 2 * j] = f1 - f0;
            a.counts[6 * i + 2 * j + 1] = members_before(l, f1) - members_before(l, f0);
        }
    }
    const List& c = a.l[0];
    const int n_cand = c.n_groups > 0 ? c.n_groups : 0;
    if (i < n_cand + a.K) {
        int lo = 0, hi = a.K - 1;   // the event of entry i: the last e with first[e] + e <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int64_t)c.first[mid] + mid <= i) lo = mid;
            else hi = mid - 1;
        }
        a.cand_ptr_ev[i] = members_before(c, i - lo) - members_before(c, c.first[lo]);
    }
}

}  // namespace

extern "C" {

size_t gtf_graph_concat_workspace_bytes(int32_t n_parts) { return carve(nullptr, n_parts > 0 ? n_parts : 0).total; }

int gtf_graph_concat(const gtf_concat_sizes* sizes, const gtf_concat_part* parts, int32_t n_parts,
                     const gtf_concat_out* out, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_graph_concat";
    if (int rc = gtf::check_abi(out, who, "gtf_concat_out", "gtf_concat_out")) return rc;
    if (n_parts < 0) return bad("gtf_graph_concat: negative n_parts");
    if (n_parts > 0 && !sizes) return bad("gtf_graph_concat: null sizes");
    if (n_parts > 0 && !parts) return bad("gtf_graph_concat: null part table");
    int64_t sum[AXES] = {0, 0, 0, 0};
    for (int i = 0; i < n_parts; i++) {
        const gtf_concat_sizes& z = sizes[i];
        if (z.n_nodes < 0 || z.n_slots < 0 || z.n_edges < 0 || z.n_sub < 0) return bad("gtf_graph_concat: negative sizes");
        if (z.n_nodes == 0 && (z.n_slots > 0 || z.n_edges > 0)) return bad("gtf_graph_concat: slots or edges without nodes");
        sum[AX_NODE] += z.n_nodes; sum[AX_SLOT] += z.n_slots; sum[AX_EDGE] += z.n_edges; sum[AX_SUB] += z.n_sub;
    }
    for (int a = 0; a < AXES; a++)
        if (sum[a] >= LIMIT) return bad("gtf_graph_concat: the parts sum to 2^31 or more nodes, slots, edges or subgraphs");
    if (!workspace || workspace_bytes < gtf_graph_concat_workspace_bytes(n_parts))
        return bad("gtf_graph_concat: workspace smaller than gtf_graph_concat_workspace_bytes");
    const Ws w = carve(workspace, n_parts);
    hipStream_t st = (hipStream_t)stream;
    Struct a;
    a.K = n_parts; a.N = (int32_t)sum[AX_NODE]; a.S = (int32_t)sum[AX_SLOT]; a.E = (int32_t)sum[AX_EDGE];
    a.parts = parts; a.off = w.off; a.o = *out;
    hipLaunchKernelGGL(k_offsets, dim3(1), dim3(BLOCK), 0, st, parts, (int)n_parts, w.off);
    if (a.N == 0 || n_parts == 0) {   // no row to search a part for: the two closing pointers alone
        a.K = 0; a.S = a.E = 0;
        hipLaunchKernelGGL(k_struct, dim3(1, 1), dim3(BLOCK), 0, st, a);
    } else {
        int64_t longest = (int64_t)a.N + 1;
        if (a.S > longest) longest = a.S;
        if (a.E > longest) longest = a.E;
        const int gx = grid(longest) < STRUCT_BLOCKS ? grid(longest) : STRUCT_BLOCKS;
        hipLaunchKernelGGL(k_struct, dim3(gx, 3), dim3(BLOCK), 0, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

int gtf_concat_columns(const void* workspace, int32_t n_parts, int32_t n_nodes, int32_t n_slots,
                       const gtf_concat_column* cols, int32_t n_cols, gtf_stream_t stream) {
    const char* who = "gtf_concat_columns";
    if (n_cols < 0 || n_parts < 0 || n_nodes < 0 || n_slots < 0) return bad("gtf_concat_columns: negative sizes");
    if (n_cols == 0) return 0;
    if (!workspace) return bad("gtf_concat_columns: null workspace");
    if (!cols) return bad("gtf_concat_columns: null column table");
    for (int i = 0; i < n_cols; i++) {
        const gtf_concat_column& c = cols[i];
        if (c.row_bytes <= 0) return bad("gtf_concat_columns: row_bytes must be at least 1");
        if (c.axis != 0 && c.axis != 1) return bad("gtf_concat_columns: axis must be 0 (nodes) or 1 (slots)");
        const int64_t rows = c.axis == 0 ? n_nodes : n_slots;
        if (rows == 0) continue;
        if (!c.dst || !c.src) return bad("gtf_concat_columns: null column pointer");
        const int wb = c.row_bytes % 8 == 0 ? 8 : c.row_bytes % 4 == 0 ? 4 : 1;
        if ((uintptr_t)c.dst % wb) return bad("gtf_concat_columns: destination not aligned to its row words");
        if (rows > INT64_MAX / c.row_bytes) return bad("gtf_concat_columns: column too large");
    }
    if (n_parts == 0) return 0;
    const Ws w = carve(workspace, n_parts);
    hipStream_t st = (hipStream_t)stream;
    for (int at = 0; at < n_cols;) {
        ColTab tab;
        int n = 0;
        int64_t longest = 0;
        for (; at < n_cols && n < MAXC; at++) {
            const gtf_concat_column& c = cols[at];
            const int64_t rows = c.axis == 0 ? n_nodes : n_slots;
            if (rows == 0) continue;
            const int lg = c.row_bytes % 8 == 0 ? 3 : c.row_bytes % 4 == 0 ? 2 : 0;
            tab.c[n].src = c.src;
            tab.c[n].dst = c.dst;
            tab.c[n].words = c.row_bytes >> lg;
            tab.c[n].mode = c.axis | (lg << 8);
            if (rows > longest) longest = rows;
            n++;
        }
        if (n == 0) break;
        for (int i = n; i < MAXC; i++) tab.c[i] = tab.c[0];
        int gx = COPY_BLOCKS / n;
        gx = gx < 64 ? 64 : gx > 1024 ? 1024 : gx;
        if (gx > grid(longest)) gx = grid(longest);
        hipLaunchKernelGGL(k_columns, dim3(gx, n), dim3(BLOCK), 0, st, (const int32_t*)w.off, (int)n_parts, (int)n_nodes,
                           (int)n_slots, tab);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    return 0;
}

size_t gtf_event_split_workspace_bytes(int32_t n_events) {
    (void)n_events;   // (the error word alone: every result goes to the caller's arrays)
    gtf::Arena a(nullptr);
    a.take<int32_t>(16);
    return a.used();
}

int gtf_event_split(const int32_t* event, int32_t n_nodes, int32_t n_events,
                    const gtf_extract_out_counts* counts, const gtf_split_in* in, const gtf_split_out* out,
                    void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_event_split";
    if (int rc = gtf::check_abi(in, who, "gtf_split_in", "gtf_split_in")) return rc;
    if (!counts || !out) return bad("gtf_event_split: null argument");
    if (n_nodes < 0 || n_events < 0 || counts->n_extracted < 0 || counts->n_extracted_nodes < 0 ||
        counts->n_remaining < 0 || counts->n_remaining_nodes < 0 || counts->n_fragments < 0 ||
        counts->n_fragment_nodes < 0)
        return bad("gtf_event_split: negative sizes");
    if (n_events == 0) return 0;
    if (!out->cand_first || !out->rem_first || !out->frag_first || !out->counts || !out->cand_ptr_ev)
        return bad("gtf_event_split: missing output array");
    Split a;
    a.N = n_nodes; a.K = n_events; a.event = event;
    a.l[0] = List{in->cand_ptr, in->cand_members, counts->n_extracted, counts->n_extracted_nodes, out->cand_first};
    a.l[1] = List{in->rem_ptr, in->rem_nodes, counts->n_remaining, counts->n_remaining_nodes, out->rem_first};
    a.l[2] = List{in->frag_ptr, in->frag_nodes, counts->n_fragments, counts->n_fragment_nodes, out->frag_first};
    int64_t longest = (int64_t)n_events + 1;
    for (int j = 0; j < LISTS; j++) {
        const List& l = a.l[j];
        if ((l.n_groups > 0 || l.n_members > 0) && (!l.ptr || !l.mem || !event))
            return bad("gtf_event_split: missing array of a list that is not empty (pointers, members, event)");
        if (l.n_groups > longest) longest = l.n_groups;
        if (l.n_members > longest) longest = l.n_members;
    }
    if (!workspace || workspace_bytes < gtf_event_split_workspace_bytes(n_events))
        return bad("gtf_event_split: workspace smaller than gtf_event_split_workspace_bytes");
    a.counts = out->counts; a.cand_ptr_ev = out->cand_ptr_ev; a.err = (int32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(a.err, 0, 64, st)) != hipSuccess) return fail(who, "memset", e);
    hipLaunchKernelGGL(k_split_first, dim3(grid((int64_t)n_events + 1), LISTS), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_split_check, dim3(grid(longest), LISTS), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_split_finish, dim3(grid((int64_t)counts->n_extracted + n_events)), dim3(BLOCK), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(who, "launch", e);
    int32_t err = 0;
    if ((e = hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    if (err) return bad("gtf_event_split: a group spans two events, events decrease, or a list is malformed");
    return 0;
}

}  // extern "C"
