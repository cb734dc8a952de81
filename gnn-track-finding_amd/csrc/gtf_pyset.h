// gtf_pyset.h -- CPython 3.10's set of non-negative ints on the device, shared by the
// event build (gtf_build_dev.hip) and the candidate order (gtf_extract.hip): both reproduce
// networkx orders that are set iteration orders (Objects/setobject.c: linear probes of 9,
// then perturbed probing, resize at 3/5 fill). Node ids hash to themselves (Python ints
// below 2^61 - 1). gtf_build.cpp's PySet is the host form.
#ifndef GTF_PYSET_H
#define GTF_PYSET_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gtf_search.h"

namespace {

// final table size of a CPython 3.10 set after n distinct insertions (start 8, resize when
// fill * 5 >= mask * 3 to the next power of two above 4 * fill, 2 * fill past 50000)
__host__ __device__ inline int64_t set_capacity(int64_t n) {
    int64_t mask = 7;
    for (int64_t fill = 1; fill <= n; fill++) {
        if (fill * 5 >= mask * 3) {
            const int64_t minused = fill > 50000 ? fill * 2 : fill * 4;
            int64_t ns = 8;
            while (ns <= minused) ns <<= 1;
            mask = ns - 1;
        }
    }
    return mask + 1;
}

// CPython 3.10 set of non-negative ints in caller memory: `a` the live table, `b` a spare
// of the same capacity (set_capacity of the distinct keys to come), swapped on resize
struct DevSet {
    int64_t* a;
    int64_t* b;
    int64_t mask;
    int64_t fill;
    int64_t cap;        // entries of each table (a resize beyond it sets `over` and stops)
    bool over;

    __device__ void init(int64_t* t0, int64_t* t1, int64_t capacity) {
        a = t0;
        b = t1;
        mask = 7;
        fill = 0;
        cap = capacity;
        over = capacity < 8;
        if (!over)
            for (int i = 0; i < 8; i++) a[i] = -1;
    }
    __device__ void insert_clean(int64_t key) {
        uint64_t perturb = (uint64_t)key;
        int64_t i = key & mask;
        for (;;) {
            if (a[i] < 0) { a[i] = key; return; }
            if (i + 9 <= mask)
                for (int64_t j = 1; j <= 9; j++)
                    if (a[i + j] < 0) { a[i + j] = key; return; }
            perturb >>= 5;
            i = (int64_t)(((uint64_t)i * 5 + 1 + perturb) & (uint64_t)mask);
        }
    }
    __device__ void resize(int64_t minused) {
        int64_t ns = 8;
        while (ns <= minused) ns <<= 1;
        if (ns > cap) { over = true; return; }   // more distinct keys than the table was sized for
        int64_t* old = a;
        const int64_t om = mask;
        a = b;
        b = old;
        mask = ns - 1;
        for (int64_t i = 0; i <= mask; i++) a[i] = -1;
        for (int64_t i = 0; i <= om; i++)
            if (old[i] >= 0) insert_clean(old[i]);
    }
    __device__ void add(int64_t key) {
        if (over) return;
        uint64_t perturb = (uint64_t)key;
        int64_t i = key & mask;
        for (;;) {
            int64_t probes = (i + 9 <= mask) ? 9 : 0;
            int64_t j = i;
            for (;;) {
                if (a[j] < 0) {
                    a[j] = key;
                    fill++;
                    if (fill * 5 >= mask * 3) resize(fill > 50000 ? fill * 2 : fill * 4);
                    return;
                }
                if (a[j] == key) return;
                if (probes-- == 0) break;
                j++;
            }
            perturb >>= 5;
            i = (int64_t)(((uint64_t)i * 5 + 1 + perturb) & (uint64_t)mask);
        }
    }
};

// find_id inside the segment [lo, hi) of a map sorted by (event, id): the index of `key`
// among one event's nodes, -1 if that event does not hold it (another one may)
__device__ inline int32_t find_id_in(const uint64_t* ids, const int32_t* idx, int32_t lo, int32_t hi, int64_t key) {
    const int32_t at = lo + gtf::bound<false>(ids + lo, hi - lo, (uint64_t)key);
    return (at < hi && ids[at] == (uint64_t)key) ? idx[at] : -1;
}

// index of node id `key` (ids sorted ascending, idx the index each came from), -1 if absent
__device__ inline int32_t find_id(const uint64_t* ids, const int32_t* idx, int32_t n, int64_t key) {
    return find_id_in(ids, idx, 0, n, key);
}

}  // namespace

#endif
