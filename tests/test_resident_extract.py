"""The resident loop's C entry points without a GPU (gtf_subgraph_ptr_device,
gtf_candidate_order_device, gtf_extract_outputs and their workspace sizes): exported, mirrored
field for field, and every argument error decided on the host before any device work."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from gtf import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NEW = ["gtf_subgraph_ptr_device", "gtf_candidate_order_workspace_bytes", "gtf_candidate_order_device",
       "gtf_extract_outputs_workspace_bytes", "gtf_extract_outputs"]

pytestmark = pytest.mark.skipif(not os.path.exists(nat.LIB_PATH), reason="libgtf.so not built")


def test_new_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gtf_\w+)", out))
    src = open(HDR).read()
    for s in NEW:
        assert s in exported and s in nat.SYMBOLS and re.search(r"\b%s\s*\(" % s, src), s
    ver = re.search(r"#define GTF_ABI_VERSION (\d+)u", src)
    assert int(ver.group(1)) == nat.ABI_VERSION == 8      # no existing struct changed layout


def test_struct_mirrors_match_header():
    py = {"gtf_order_counts": nat.GtfOrderCounts, "gtf_extract_out": nat.GtfExtractOut,
          "gtf_extract_out_counts": nat.GtfExtractOutCounts}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values())
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k


def _order(L, g, e=None, counts=True, ws=1, n_sub=0):
    cnt = nat.GtfOrderCounts()
    z = ctypes.c_void_p(0)
    return L.gtf_candidate_order_device(ctypes.byref(g) if g is not None else None,
                                        ctypes.byref(e) if e is not None else None, z, z, n_sub, z, z,
                                        ctypes.c_void_p(ws), ctypes.c_size_t(1 << 40),
                                        ctypes.byref(cnt) if counts else None, z)


def _outputs(L, g, io=None, out=None, counts=True, fragment=4, ws=1, xws=1, nbytes=1 << 40):
    cnt = nat.GtfExtractOutCounts()
    return L.gtf_extract_outputs(ctypes.byref(g) if g is not None else None,
                                 ctypes.byref(io) if io is not None else None, fragment, ctypes.c_void_p(xws),
                                 ctypes.byref(out) if out is not None else None, ctypes.c_void_p(ws),
                                 ctypes.c_size_t(nbytes), ctypes.byref(cnt) if counts else None, ctypes.c_void_p(0))


def test_null_arguments_are_refused_on_the_host():
    """-2 with a message, and nothing launched (the pointers given are not device memory)"""
    L = nat.lib()
    g, e = nat.GtfGraph(n_nodes=5, n_slots=3, n_edges=3), nat.GtfEdges()
    assert _order(L, None, e) == -2
    assert _order(L, g, None) == -2 and b"gtf_candidate_order_device" in L.gtf_last_error()
    assert _order(L, g, e, counts=False) == -2
    assert _order(L, g, e, ws=0) == -2
    assert _order(L, g, e) == -2 and b"missing array" in L.gtf_last_error()      # no sub_id, node_id, ...
    assert _order(L, nat.GtfGraph(n_nodes=-1), e) == -2
    io, out = nat.GtfExtractIO(), nat.GtfExtractOut()
    assert _outputs(L, None, io, out) == -2
    assert _outputs(L, g, None, out) == -2 and b"gtf_extract_outputs" in L.gtf_last_error()
    assert _outputs(L, g, io, None) == -2
    assert _outputs(L, g, io, out, counts=False) == -2
    assert _outputs(L, g, io, out, ws=0) == -2
    assert _outputs(L, g, io, out, xws=0) == -2
    assert _outputs(L, g, io, out, fragment=0) == -2
    assert _outputs(L, g, io, out) == -2 and b"missing arrays" in L.gtf_last_error()
    z = ctypes.c_void_p(0)
    assert L.gtf_subgraph_ptr_device(z, 0, 0, z, z) == -2
    assert L.gtf_subgraph_ptr_device(z, 5, 1, ctypes.c_void_p(1), z) == -2
    assert L.gtf_subgraph_ptr_device(ctypes.c_void_p(1), 5, 0, ctypes.c_void_p(1), z) == -2
    assert L.gtf_subgraph_ptr_device(ctypes.c_void_p(1), -1, 1, ctypes.c_void_p(1), z) == -2


def test_small_workspace_is_refused_on_the_host():
    L = nat.lib()
    one = ctypes.c_void_p(1)
    g = nat.GtfGraph(n_nodes=5, n_slots=0, n_edges=0, slot_ptr=one, out_ptr=one)
    cnt = nat.GtfOrderCounts()
    nb = L.gtf_candidate_order_workspace_bytes(5, 0, 1)
    rc = L.gtf_candidate_order_device(ctypes.byref(g), ctypes.byref(nat.GtfEdges()), one, one, 1, one, one, one,
                                      ctypes.c_size_t(nb - 1), ctypes.byref(cnt), None)
    assert rc == -2 and b"workspace" in L.gtf_last_error()
    io = nat.GtfExtractIO(one, one, one, one, 1, 0, None, one, one, one, one, one, one, one)
    out = nat.GtfExtractOut(left=one, keep=one)
    nb = L.gtf_extract_outputs_workspace_bytes(5, 1)
    assert _outputs(L, g, io, out, nbytes=nb - 1) == -2 and b"workspace" in L.gtf_last_error()
    out = nat.GtfExtractOut(left=one, keep=one, cand_ids=one)          # id lists without node_id
    assert _outputs(L, g, io, out) == -2 and b"node_id" in L.gtf_last_error()


def test_abi_mismatch_is_refused_without_device_work():
    L = nat.lib()
    g = nat.GtfGraph(n_nodes=5)
    g.abi_version = nat.ABI_VERSION + 1
    assert _order(L, g, nat.GtfEdges()) == -3 and b"ABI mismatch" in L.gtf_last_error()
    assert _outputs(L, g, nat.GtfExtractIO(), nat.GtfExtractOut()) == -3 and b"ABI mismatch" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=5)
    g.struct_size -= 8
    assert _order(L, g, nat.GtfEdges()) == -3
    assert _outputs(L, g, nat.GtfExtractIO(), nat.GtfExtractOut()) == -3


def test_empty_graph_returns_zero_counts_without_a_launch():
    L = nat.lib()
    g = nat.GtfGraph(n_nodes=0)
    cnt = nat.GtfOrderCounts(7, 7, 7, 7)
    one = ctypes.c_void_p(1)
    assert L.gtf_candidate_order_device(ctypes.byref(g), ctypes.byref(nat.GtfEdges()), None, None, 0, None, None,
                                        one, ctypes.c_size_t(0), ctypes.byref(cnt), None) == 0
    assert (cnt.n_components, cnt.n_set_ordered, cnt.max_set_ordered) == (0, 0, 0)
    oc = nat.GtfExtractOutCounts(7, 7, 7, 7, 7, 7)
    assert L.gtf_extract_outputs(ctypes.byref(g), ctypes.byref(nat.GtfExtractIO()), 4, one,
                                 ctypes.byref(nat.GtfExtractOut()), one, ctypes.c_size_t(0), ctypes.byref(oc), None) == 0
    assert [getattr(oc, f) for f, _ in oc._fields_] == [0] * 6


def test_workspace_sizes_are_positive_and_monotone():
    L = nat.lib()
    f = L.gtf_candidate_order_workspace_bytes
    assert f(0, 0, 0) > 0 and f(-5, -5, -5) == f(0, 0, 0)
    base = f(1000, 5000, 40)
    assert f(1001, 5000, 40) >= base and f(1000, 5001, 40) >= base and f(1000, 5000, 41) >= base
    assert f(2000, 5000, 40) > base and f(1000, 5000, 100000) > base
    assert base >= 8 * 24 * 1000          # three set tables of <= 8 k entries per component
    sizes = [f(n, 4 * n, n // 7) for n in (0, 1, 2, 255, 256, 257, 1000, 4096, 100000, 1 << 20)]
    assert sizes == sorted(sizes)
    h = L.gtf_extract_outputs_workspace_bytes
    assert h(0, 0) > 0 and h(-1, -1) == h(0, 0)
    base = h(1000, 40)
    assert h(1001, 40) >= base and h(1000, 41) >= base and h(2000, 40) > base and h(1000, 100000) > base
    sizes = [h(n, n // 7) for n in (0, 1, 2, 255, 256, 257, 1000, 4096, 100000, 1 << 20)]
    assert sizes == sorted(sizes)
