// gtf_search.h -- the device half the table-building and scoring kernels share: the searches in
// sorted arrays and offset tables, the clamps that keep a broken index inside its array and the
// bit helpers of the packed sort keys. Device code only (gtf_host.h is the host half).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gtf {

// an int64 id as its bits with the sign flipped: the unsigned order of the result is the signed one
__device__ __forceinline__ uint64_t flip(int64_t x) { return (uint64_t)x ^ (uint64_t(1) << 63); }
__device__ __forceinline__ int64_t unflip(uint64_t k) { return (int64_t)(k ^ (uint64_t(1) << 63)); }
// the halves of two int32 counts packed into one int64 sum
__device__ __forceinline__ int32_t lo32(int64_t x) { return (int32_t)(uint32_t)x; }
__device__ __forceinline__ int32_t hi32(int64_t x) { return (int32_t)((uint64_t)x >> 32); }

// x as an index into an array of n: itself, or 0 where it is none
__device__ __forceinline__ int index_or0(int x, int n) { return x >= 0 && x < n ? x : 0; }
// x inside [lo, hi]
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

// event e's segment [b, end) of an axis of `total` rows, from the axis' K + 1 offsets, clamped
// to the axis: broken offsets read nothing outside
__device__ __forceinline__ void segment(const int32_t* off, int e, int total, int& b, int& end) {
    b = clampi(off[e], 0, total);
    end = clampi(off[e + 1], b, total);
}

// first index in [0, n) of the ascending k with k[i] >= key (upper = false) or k[i] > key
// (upper = true); n where there is none
template <bool upper, typename T>
__device__ __forceinline__ int bound(const T* k, int n, T key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (upper ? k[mid] <= key : k[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The segment of r in a table of K + 1 non-decreasing offsets (only off[0 .. K - 1] are read):
// the largest p in [0, K) with off[p] <= r. Empty segments share their successor's offset and
// are passed over, so for off[0] <= r < off[K] it is the p with off[p] <= r < off[p + 1]. An r
// before off[0] gives 0 and one from off[K] on gives the last segment: a caller that may meet
// either checks r against off[p] and off[p + 1] itself. K <= 0 gives 0 and reads nothing.
// With `first`, the table is the K + 1 offsets from off[first] on and p lies in [first, first + K).
template <typename T>
__device__ __forceinline__ int segment_of(const T* off, int K, T r, int first = 0) {
    int lo = first, hi = first + K - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// K + 1 offsets for a block of BLOCK threads: in the caller's LDS when they fit, else where
// they lie. Every thread of the block calls it.
constexpr int LDS_OFFS = 2048;   // offsets staged in LDS when K + 1 <= this (8 KiB)
template <int BLOCK>
__device__ __forceinline__ const int32_t* stage_offsets(const int32_t* off, int K, int32_t* lds) {
    if (K + 1 > LDS_OFFS) return off;
    for (int i = threadIdx.x; i <= K; i += BLOCK) lds[i] = off[i];
    __syncthreads();
    return lds;
}

}  // namespace gtf
