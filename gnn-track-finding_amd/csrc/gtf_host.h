// gtf_host.h -- the host half every entry point of libgtf shares: the error text and the
// return codes, the ABI check of the versioned structs, launch-grid arithmetic, the workspace
// arena (gtf_arena.h) and the hipcub scratch carved from it. Host code only: no kernel and no
// device function lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gtf.h"
#include "gtf_arena.h"

namespace gtf {

// ---- errors: the text of gtf_last_error() (kept in gtf_pass.hip) and the status ----
void set_error(const char* msg);

// a refused argument: -2
inline int bad(const char* msg) {
    set_error(msg);
    return -2;
}

// a failed HIP call: -1, "who: what: <the runtime's text>"
inline int fail(const char* who, const char* what, hipError_t e) {
    char m[256];
    snprintf(m, sizeof(m), "%s: %s: %s", who, what, hipGetErrorString(e));
    set_error(m);
    return -1;
}

// A versioned struct (struct_size, abi_version first) built against another layout of
// include/gtf.h: refused with status -3 instead of read with shifted fields; a null one: -2.
template <typename T>
int check_abi(const T* s, const char* who, const char* type, const char* null_what) {
    char m[260];
    if (!s) {
        snprintf(m, sizeof(m), "%s: null %s", who, null_what);
        return bad(m);
    }
    if (s->struct_size != (uint32_t)sizeof(T) || s->abi_version != GTF_ABI_VERSION) {
        snprintf(m, sizeof(m), "%s: %s ABI mismatch (caller struct_size %u, abi_version %u; library %u, %u)", who, type,
                 s->struct_size, s->abi_version, (unsigned)sizeof(T), (unsigned)GTF_ABI_VERSION);
        set_error(m);
        return -3;
    }
    return 0;
}
// every entry point taking a gtf_graph
inline int check_abi(const gtf_graph* g, const char* who) { return check_abi(g, who, "gtf_graph", "graph"); }

// a gtf_event_csr neither event builder (gtf_build.cpp, gtf_build_dev.hip) can work on: null,
// a negative size, or without a column or an output that its sizes call for
inline bool bad_event_csr(const gtf_event_csr* ev) {
    return !ev || ev->n_nodes < 0 || ev->n_rows < 0 || (ev->n_nodes && !ev->node_id) ||
           (ev->n_rows && (!ev->row_a || !ev->row_b)) || !ev->order || !ev->sub_id || !ev->slot_ptr || !ev->out_ptr ||
           (ev->n_rows && (!ev->slot_src || !ev->tse_rank || !ev->out_slot));
}

// ---- launches of 256 threads, one per item ----
constexpr int BLOCK256 = 256;
inline int grid(int64_t n) { return (int)((n + BLOCK256 - 1) / BLOCK256); }

// ---- hipcub scratch ----
// hipcub is slow to parse, so only a file that sorts or scans pays for it: it includes
// <hipcub/hipcub.hpp> before this header and gets the rest.
#ifdef HIPCUB_VERSION
// The piece of a workspace hipcub works in. A layout sizes it with CubNeed and takes it from
// its arena; an entry point calls hipcub through Cub.
struct Scratch {
    void* ptr;
    size_t bytes;
};

// The largest of the size queries of the calls a layout will make: need.scan<int32_t>(n)
// .sort_pairs<uint64_t, int32_t>(n).take(arena). A query that fails adds nothing (without a
// device every size is 0 and the arena part of a layout still adds up).
class CubNeed {
public:
    template <typename K, typename V>
    CubNeed& sort_pairs(int n) {
        size_t b = 0;
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, n);
        return add(b);
    }
    template <typename K>
    CubNeed& sort_keys(int n) {
        size_t b = 0;
        (void)hipcub::DeviceRadixSort::SortKeys(nullptr, b, (K*)nullptr, (K*)nullptr, n);
        return add(b);
    }
    template <typename T>
    CubNeed& scan(int n) {
        size_t b = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (T*)nullptr, (T*)nullptr, n);
        return add(b);
    }
    template <typename T>
    CubNeed& sum(int n) {
        size_t b = 0;
        (void)hipcub::DeviceReduce::Sum(nullptr, b, (T*)nullptr, (T*)nullptr, n);
        return add(b);
    }
    template <typename T>
    CubNeed& max(int n) {
        size_t b = 0;
        (void)hipcub::DeviceReduce::Max(nullptr, b, (T*)nullptr, (T*)nullptr, n);
        return add(b);
    }
    Scratch take(Arena& a) const { return Scratch{a.take<char>(bytes_), bytes_}; }

private:
    CubNeed& add(size_t b) {
        if (b > bytes_) bytes_ = b;
        return *this;
    }
    size_t bytes_ = 0;
};

// hipcub on one scratch and stream. hipcub overwrites the size it is given, so every call gets
// a copy of its own. scan is the exclusive sum; the sorts are stable, ascending, over key bits
// [0, end_bit).
struct Cub {
    Scratch s;
    hipStream_t st;

    template <typename K, typename V>
    hipError_t sort_pairs(const K* kin, K* kout, const V* vin, V* vout, int n, int end_bit = (int)(8 * sizeof(K))) const {
        size_t b = s.bytes;
        return hipcub::DeviceRadixSort::SortPairs(s.ptr, b, kin, kout, vin, vout, n, 0, end_bit, st);
    }
    template <typename K>
    hipError_t sort_keys(const K* kin, K* kout, int n) const {
        size_t b = s.bytes;
        return hipcub::DeviceRadixSort::SortKeys(s.ptr, b, kin, kout, n, 0, 8 * sizeof(K), st);
    }
    template <typename In, typename Out>
    hipError_t scan(In in, Out out, int n) const {
        size_t b = s.bytes;
        return hipcub::DeviceScan::ExclusiveSum(s.ptr, b, in, out, n, st);
    }
    template <typename In, typename Out>
    hipError_t sum(In in, Out out, int n) const {
        size_t b = s.bytes;
        return hipcub::DeviceReduce::Sum(s.ptr, b, in, out, n, st);
    }
    template <typename In, typename Out>
    hipError_t max(In in, Out out, int n) const {
        size_t b = s.bytes;
        return hipcub::DeviceReduce::Max(s.ptr, b, in, out, n, st);
    }
};
#endif  // HIPCUB_VERSION

}  // namespace gtf
