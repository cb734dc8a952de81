// gtf_event_errors.hip -- which event of a batch raised (include/gtf.h: gtf_event_errors): the
// per-node GTF_ERR_* bits that raise_node() (gtf_pass.hip) leaves in gtf_diag.node_err, reduced
// over the fused graph's event column, and the keep mask that cuts the raising events out. The
// device form of gtf/graph.py event_errors.
//
//   init    one thread per event: err 0, count 0, first INT32_MAX; the violation word INT32_MAX
//   reduce  one thread per node: its event checked (in [0, K), not below its predecessor's), its
//           masked bits read; only a node that carries one ORs them into its event's word, counts
//           itself and lowers the event's first index -- three atomics per raising node, none for
//           the others (raising nodes are a handful among tens of thousands)
//   out     one thread per event writes the caller's per-event arrays (first INT32_MAX -> -1,
//           first_id through node_id) and the staging copy the host reads; one thread per node
//           writes keep from its event's word
//
// The results live in one piece of the workspace, so the host half is ONE copy after ONE
// synchronisation. Every read of node_err, event and node_id is guarded by n_nodes and every
// per-event access by n_events: an event column that breaks the contract is reported, and writes
// nothing outside the outputs. Vector stores only; the violation word is the one atomic outside
// a raising node's three, touched only on a violation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/gtf.h"
#include "gtf_host.h"

namespace {

using gtf::bad;
using gtf::fail;
using gtf::grid;

constexpr int BLOCK = gtf::BLOCK256;
constexpr int32_t NONE = INT32_MAX;
constexpr size_t HEAD = 64;   // bytes before the per-event arrays: the violation word

// the one piece of the workspace: [HEAD][first_id K x 8][err K x 4][n_raising K x 4][first K x 4]
struct Ws {
    int32_t* bad_node;
    int64_t* first_id;
    uint32_t* err;
    int32_t* n_raising;
    int32_t* first;
    size_t piece, total;
};

Ws carve(const void* base, int64_t K) {
    Ws w;
    gtf::Arena a(base);
    w.piece = HEAD + 20 * (size_t)K;
    char* p = a.take<char>(w.piece);
    w.bad_node = (int32_t*)p;
    w.first_id = (int64_t*)(p + HEAD);
    w.err = (uint32_t*)(p + HEAD + 8 * (size_t)K);
    w.n_raising = (int32_t*)(p + HEAD + 12 * (size_t)K);
    w.first = (int32_t*)(p + HEAD + 16 * (size_t)K);
    w.total = a.used();
    return w;
}

struct Args {
    gtf_event_errors_io io;
    Ws w;
};

__global__ void __launch_bounds__(BLOCK) k_init(Args a) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) a.w.bad_node[0] = NONE;
    if (i >= a.io.n_events) return;
    a.w.err[i] = 0u;
    a.w.n_raising[i] = 0;
    a.w.first[i] = NONE;
}

__global__ void __launch_bounds__(BLOCK) k_reduce(Args a) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= a.io.n_nodes) return;
    int32_t e = 0;
    if (a.io.event) {
        e = a.io.event[v];
        const bool in_range = e >= 0 && e < a.io.n_events;
        if (!in_range || (v > 0 && a.io.event[v - 1] > e)) atomicMin(a.w.bad_node, (int32_t)v);   // (a violation only)
        if (!in_range) return;
    }
    const uint32_t bits = a.io.node_err[v] & a.io.mask;
    if (bits == 0u) return;
    atomicOr(a.w.err + e, bits);
    atomicAdd(a.w.n_raising + e, 1);
    atomicMin(a.w.first + e, (int32_t)v);
}

__global__ void __launch_bounds__(BLOCK) k_out(Args a) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < a.io.n_events) {
        const int32_t f = a.w.first[i];
        const int32_t fn = f == NONE ? -1 : f;
        const int64_t id = (a.io.node_id && fn >= 0 && fn < a.io.n_nodes) ? a.io.node_id[fn] : (int64_t)-1;
        a.w.first[i] = fn;
        a.w.first_id[i] = id;
        if (a.io.err_ev) a.io.err_ev[i] = a.w.err[i];
        if (a.io.n_raising) a.io.n_raising[i] = a.w.n_raising[i];
        if (a.io.first_node) a.io.first_node[i] = fn;
        if (a.io.first_id && a.io.node_id) a.io.first_id[i] = id;
    }
    if (i < a.io.n_nodes && a.io.keep) {
        const int32_t e = a.io.event ? a.io.event[i] : 0;
        const bool in_range = e >= 0 && e < a.io.n_events;
        a.io.keep[i] = (in_range && a.w.err[e] == 0u) ? 1 : 0;
    }
}

}  // namespace

extern "C" {

size_t gtf_event_errors_workspace_bytes(int32_t n_events) { return carve(nullptr, n_events > 0 ? n_events : 0).total; }

int gtf_event_errors(const gtf_event_errors_io* io, void* workspace, size_t workspace_bytes, gtf_stream_t stream) {
    const char* who = "gtf_event_errors";
    if (int rc = gtf::check_abi(io, who, "gtf_event_errors_io", "gtf_event_errors_io")) return rc;
    if (io->n_nodes < 0 || io->n_events < 0) return bad("gtf_event_errors: negative sizes");
    if (io->n_nodes == 0 || io->n_events == 0) return 0;
    if (!io->node_err) return bad("gtf_event_errors: null node_err");
    if (!io->event && io->n_events != 1) return bad("gtf_event_errors: a null event column means one event (n_events == 1)");
    if (!workspace || workspace_bytes < gtf_event_errors_workspace_bytes(io->n_events))
        return bad("gtf_event_errors: workspace smaller than gtf_event_errors_workspace_bytes");
    Args a;
    a.io = *io;
    a.w = carve(workspace, io->n_events);
    const int64_t K = io->n_events, N = io->n_nodes;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_init, dim3(grid(K)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_reduce, dim3(grid(N)), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_out, dim3(grid(N > K ? N : K)), dim3(BLOCK), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(who, "launch", e);
    std::vector<char> h(a.w.piece);
    if ((e = hipMemcpyAsync(h.data(), a.w.bad_node, a.w.piece, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(who, "read", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(who, "synchronize", e);
    int32_t bad_node;
    memcpy(&bad_node, h.data(), 4);
    if (bad_node != NONE) {
        char m[160];
        snprintf(m, sizeof(m), "gtf_event_errors: event[%d] is outside [0, %d) or below event[%d]: the column must be "
                 "non-decreasing", bad_node, io->n_events, bad_node - 1);
        return bad(m);
    }
    const char* p = h.data() + HEAD;
    if (io->host_first_id && io->node_id) memcpy(io->host_first_id, p, 8 * (size_t)K);
    if (io->host_err_ev) memcpy(io->host_err_ev, p + 8 * (size_t)K, 4 * (size_t)K);
    if (io->host_n_raising) memcpy(io->host_n_raising, p + 12 * (size_t)K, 4 * (size_t)K);
    if (io->host_first_node) memcpy(io->host_first_node, p + 16 * (size_t)K, 4 * (size_t)K);
    return 0;
}

}  // extern "C"
