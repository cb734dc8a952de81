"""The batch cases on the CPU (tests/batch_cases.py): every part list fuses under gtf.graph.concat into a
graph that passes check_layout, holds what the case claims and comes apart again under
gtf.graph.split_events; the NumPy statement of gtf_event_split's rule equals per-event slicing; libgtf
exports the batch entry points and the ctypes structs match include/gtf.h."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import batch_cases as bc
from gtf import graph
from gtf.graph import NODE_FIELDS, SLOT_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NEW_SYMBOLS = ("gtf_graph_concat_workspace_bytes", "gtf_graph_concat", "gtf_concat_columns",
               "gtf_candidate_order_device_ev", "gtf_event_split_workspace_bytes", "gtf_event_split")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def _graphs_equal(got, exp, what):
    assert (got.n_nodes, got.n_slots, got.n_edges, got.n_subgraphs) == \
        (exp.n_nodes, exp.n_slots, exp.n_edges, exp.n_subgraphs), what
    for k in ("slot_ptr", "out_ptr", "out_slot"):
        assert _same(getattr(got, k), getattr(exp, k)), (what, k)
    for k in NODE_FIELDS:
        assert _same(got.node[k], exp.node[k]), (what, k)
    for k in SLOT_FIELDS:
        assert _same(got.slot[k], exp.slot[k]), (what, k)


# ---------------------------------------------------------------- concat cases
@pytest.mark.parametrize("name", list(bc.CONCAT))
def test_concat_case_fuses_and_splits(name):
    parts, g, event = bc.host_concat(name)
    graph.check_layout(g)
    assert g.n_nodes == sum(p.n_nodes for p in parts) == event.size
    assert g.n_subgraphs == sum(p.n_subgraphs for p in parts)
    if name != "orphans":   # (scattered sub_id: split_events renumbers dense, grouped ids only)
        for i, (got, exp) in enumerate(zip(graph.split_events(g, event, len(parts)), parts)):
            _graphs_equal(got, exp, (name, i))
    if g.n_nodes:
        with pytest.raises(ValueError, match="non-decreasing"):
            graph.split_events(g, event[::-1] if np.unique(event).size > 1 else event + len(parts), len(parts))


def test_concat_cases_hold_what_they_claim():
    sizes = {n: [p.n_nodes for p in bc.host_concat(n)[0]] for n in bc.CONCAT}
    assert sizes["hand4"] == [1, 2, 65, 257]
    assert sizes["empty_first"][0] == 0 and sizes["empty_last"][-1] == 0 and sizes["empty_middle"][1:3] == [0, 0]
    assert sum(sizes["all_empty"]) == 0 and len(sizes["k1"]) == 1
    assert len(sizes["k65"]) == 65 and len(sizes["k257"]) == 257 and set(sizes["k257"]) == {1, 2}
    # a part boundary inside a 64-thread run of nodes, of slots and of out-edges
    parts = bc.host_concat("midwave")[0]
    for cut in (np.cumsum([p.n_nodes for p in parts])[:-1], np.cumsum([p.n_slots for p in parts])[:-1],
                np.cumsum([p.n_edges for p in parts])[:-1]):
        assert any(c % 64 for c in cut), cut
    # the same event twice: every id collides, inside an event none does
    parts, g, event = bc.host_concat("vol7_twice")
    ids = g.node["node_id"]
    assert parts[0].n_nodes == 8748 and np.unique(ids).size == parts[0].n_nodes == ids.size // 2
    # the subset() children keep orphan keys, and one has scattered subgraph ids
    parts, g, _ = bc.host_concat("orphans")
    assert all((p.slot["slot_src"] < 0).sum() > 100 for p in parts)
    assert (g.slot["slot_src"] < 0).sum() == sum((p.slot["slot_src"] < 0).sum() for p in parts)
    assert np.any(np.diff(parts[1].node["sub_id"]) < 0)
    # tiny parts: ids differ between the parts
    parts, g, _ = bc.host_concat("k257")
    assert np.unique(g.node["node_id"]).size == g.n_nodes == 257 + 128


# ---------------------------------------------------------------- split rule
@pytest.mark.parametrize("name", list(bc.SPLIT) + ["k257"])
def test_split_rule_equals_per_event_slicing(name):
    c = bc.split_case(name)
    K, per = c["K"], c["per_event"]
    first, counts, pev = bc.split_rule(c["event"], K, c["lists"])
    for j, k in enumerate(("cand", "rem", "frag")):
        ptr, mem = c["lists"][k]
        assert first[k][0] == 0 and first[k][K] == ptr.size - 1
        for e in range(K):
            got = [mem[ptr[i]:ptr[i + 1]] for i in range(first[k][e], first[k][e + 1])]
            assert len(got) == len(per[e][k]) and all(np.array_equal(a, b) for a, b in zip(got, per[e][k])), (k, e)
            assert counts[e, 2 * j] == len(per[e][k]) and counts[e, 2 * j + 1] == sum(len(g) for g in per[e][k])
    assert counts.sum(axis=0).tolist() == bc.counts_of(c["lists"])
    fc = first["cand"]
    for e in range(K):   # event e's slice is the pointer array of its own candidates
        own = bc._csr(per[e]["cand"])[0]
        assert np.array_equal(pev[fc[e] + e:fc[e + 1] + e + 1], own), e
    assert pev.size == fc[K] + K


def test_split_cases_hold_what_they_claim():
    n = lambda name, k: [len(e[k]) for e in bc.split_case(name)["per_event"]]  # noqa: E731
    assert n("no_candidate", "cand")[1] == 0 and n("no_candidate", "rem")[1] > 0
    assert (n("only_fragments", "cand")[1], n("only_fragments", "rem")[1]) == (0, 0) and n("only_fragments", "frag")[1] > 0
    c = bc.split_case("last_empty")
    assert int(c["event"].max()) == c["K"] - 2            # no node of the last event
    assert bc.split_case("k257")["K"] == 257 and sum(n("k257", "cand")) > 50
    assert 0 in n("k257", "cand") and 0 in n("k257", "frag")
    # the refused lists break the rule's premises, and only those
    ok = bc.split_case("no_candidate")
    ev = ok["event"]
    p, m = bc.bad_split_case("spanning")["lists"]["rem"]
    assert np.unique(ev[m[p[0]:p[1]]]).size == 2
    p, m = bc.bad_split_case("decreasing")["lists"]["cand"]
    assert np.any(np.diff(ev[m[p[:-1]]]) < 0)
    p, m = bc.bad_split_case("empty_group")["lists"]["frag"]
    assert p[0] == p[1]
    assert bc.bad_split_case("member_range")["lists"]["cand"][1][0] == ok["N"]


# ---------------------------------------------------------------- the library and its bindings
def test_library_exports_the_batch_entry_points():
    from gtf import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libgtf.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gtf_\w+)", out))
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", open(HDR).read(), re.M))
    for s in NEW_SYMBOLS:
        assert s in exported and s in declared and s in _native.SYMBOLS, s
    L = _native.lib(lean=True)
    assert L.gtf_graph_concat_workspace_bytes(0) > 0 and L.gtf_event_split_workspace_bytes(0) > 0
    assert L.gtf_graph_concat_workspace_bytes(257) >= 4 * 4 * 258 >= L.gtf_graph_concat_workspace_bytes(-3)


def test_batch_struct_layout_matches_header():
    from gtf import _native as nat
    py = {"gtf_concat_sizes": nat.GtfConcatSizes, "gtf_concat_part": nat.GtfConcatPart,
          "gtf_concat_out": nat.GtfConcatOut, "gtf_concat_column": nat.GtfConcatColumn,
          "gtf_split_in": nat.GtfSplitIn, "gtf_split_out": nat.GtfSplitOut,
          "gtf_extract_out_counts": nat.GtfExtractOutCounts, "gtf_order_counts": nat.GtfOrderCounts}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    lines.append('  printf("macro.GTF_CONCAT_MAX_COLUMNS %d\\n", GTF_CONCAT_MAX_COLUMNS);')
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values()) + 1
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        elif t == "macro":
            assert nat.CONCAT_MAX_COLUMNS == int(v)
        else:
            assert getattr(py[t], f).offset == int(v), k


def test_concat_refuses_oversize_sums_on_the_host():
    """sizes alone decide: no device memory is touched (the pointers are never read)"""
    from gtf import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib(lean=True)
    out = nat.GtfConcatOut()
    fake = ctypes.c_void_p(256)
    for axis in range(4):
        z = [[1, 0, 0, 0], [1, 0, 0, 0]]
        z[0][axis] = z[1][axis] = 1 << 30
        sizes = (nat.GtfConcatSizes * 2)(*[nat.GtfConcatSizes(*r) for r in z])
        assert L.gtf_graph_concat(sizes, fake, 2, ctypes.byref(out), fake, 1 << 20, None) == -2
        assert b"2^31" in L.gtf_last_error()
    sizes = (nat.GtfConcatSizes * 1)(nat.GtfConcatSizes(0, 3, 0, 0))
    assert L.gtf_graph_concat(sizes, fake, 1, ctypes.byref(out), fake, 1 << 20, None) == -2
    assert b"without nodes" in L.gtf_last_error()
    assert L.gtf_graph_concat(None, fake, 1, ctypes.byref(out), fake, 1 << 20, None) == -2
    sizes = (nat.GtfConcatSizes * 1)(nat.GtfConcatSizes(1, 0, 0, 1))
    assert L.gtf_graph_concat(sizes, fake, 1, ctypes.byref(out), fake, 8, None) == -2 and b"workspace" in L.gtf_last_error()
    assert L.gtf_graph_concat(sizes, fake, 1, None, fake, 1 << 20, None) == -2
    other = nat.GtfConcatOut()      # built against another layout of the header
    other.struct_size += 8
    assert L.gtf_graph_concat(sizes, fake, 1, ctypes.byref(other), fake, 1 << 20, None) == -3
    assert b"gtf_concat_out ABI mismatch" in L.gtf_last_error()
    other = nat.GtfSplitIn()
    other.abi_version = nat.ABI_VERSION + 1
    cnt, so = nat.GtfExtractOutCounts(), nat.GtfSplitOut(fake, fake, fake, fake, fake)
    assert L.gtf_event_split(None, 0, 2, ctypes.byref(cnt), ctypes.byref(other), ctypes.byref(so), fake, 256, None) == -3
