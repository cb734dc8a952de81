// gtf_arena.h -- the bump arena every workspace layout of libgtf is carved from. Plain C++, no
// HIP include, so tests/host_arena_check.cpp checks it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gtf {

inline size_t al(size_t x) { return (x + 255) & ~size_t(255); }

// Consecutive 256-byte aligned pieces of one allocation, in the order they are taken. A piece
// of zero bytes still advances 256, so no two pieces share an address. On a null base it is a
// dry run: the pointers are the offsets (never dereferenced) and used() is the size to
// allocate. A layout is one function that takes its pieces from an Arena; run dry it is the
// *_workspace_bytes of its entry point, so the two cannot drift apart.
class Arena {
public:
    explicit Arena(const void* base) : base_((uintptr_t)base) {}
    template <typename T>
    T* take(size_t count) {
        T* const p = (T*)(base_ + off_);
        off_ += al(count ? count * sizeof(T) : 1);
        return p;
    }
    size_t used() const { return off_; }

private:
    uintptr_t base_;
    size_t off_ = 0;
};

}  // namespace gtf
