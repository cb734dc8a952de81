"""Device buffers between guard bytes, for the tests that call the builders' C-ABI on raw memory
(tests/test_gpu_build.py, tests/test_gpu_build_batch.py): an entry point that writes outside what it was
given, or into an output it refuses, shows as a changed guard."""
import ctypes

import numpy as np

GUARD = 256   # (a multiple of the arena's alignment: the workspace between its guards stays aligned)
FILL = 0xA5


class Mem:
    """device buffers of one allocator: "torch" tensors or "hip" (gtf.devmem) arrays"""

    def __init__(self, mem):
        self.mem = mem
        if mem == "torch":
            import torch
            self.torch = torch
            self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        else:
            self.stream = ctypes.c_void_p(0)

    def up(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        if self.mem == "torch":
            return self.torch.from_numpy(a).cuda()
        from gtf.devmem import HipArray
        return HipArray.from_numpy(a)

    def host(self, t):
        return t.cpu().numpy() if self.mem == "torch" else t.numpy()

    def guarded(self, nbytes):
        return self.up(np.full(GUARD + nbytes + GUARD, FILL, np.uint8))

    def payload(self, t, nbytes, dtype=np.int32):
        h = self.host(t)
        assert bool((h[:GUARD] == FILL).all()) and bool((h[GUARD + nbytes:] == FILL).all()), "guard bytes"
        return h[GUARD:GUARD + nbytes].view(dtype)


def at(t):
    """the address of a guarded buffer's payload"""
    return ctypes.c_void_p(t.data_ptr() + GUARD)


def untouched(got):
    """every payload of the dict still holds the fill pattern"""
    return all(bool((v.view(np.uint8) == FILL).all()) for v in got.values())
