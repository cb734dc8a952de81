"""gtf.graph.event_errors (the definition of gtf_event_errors) against a plain Python loop on the hand-made
cases of tests/event_error_cases.py, the ctypes mirror of gtf_event_errors_io against the header, and the
refusals of the on_error argument. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import event_error_cases as ec
from gtf import graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ec.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_definition_equals_the_loop(name):
    err, ev, K, mask, ids = CASES[name]
    got = graph.event_errors(err, ev, K, mask, node_id=ids)
    exp = ec.by_loop(err, ev, K, mask, ids)
    for g, x, what in zip(got, exp, ("err_ev", "n_raising", "first_node", "first_id", "keep")):
        assert g.dtype == x.dtype and np.array_equal(g, x), (name, what)
    assert graph.event_errors(err, ev, K, mask)[3] is None      # (no node_id: no first_id)


def test_the_cases_hold_what_they_claim():
    """the hand-made cases exercise what their names say (so a definition that ignored them would show)"""
    r = {n: graph.event_errors(*c[:4], node_id=c[4]) for n, c in CASES.items()}
    assert r["first_node"][2].tolist() == [-1, 5, -1] and r["last_node"][2].tolist() == [-1, 74, -1]
    assert r["or_together"][0].tolist() == [0, ec.TIE | ec.NAN_KL] and r["or_together"][1].tolist() == [0, 2]
    assert r["masked_out"][0].tolist() == [0, 0, ec.TIE] and r["masked_out"][4][:20].all()
    assert (r["every_event"][0] != 0).all() and not r["every_event"][4].any()
    assert r["every_event"][2].tolist() == [2, 66, 67, 68]
    assert r["one_event_null"][0].tolist() == [ec.TIE | ec.NAN_KL] and not r["one_event_null"][4].any()
    assert r["clean"][4].all() and r["n0"][0].tolist() == [0, 0, 0] and r["n0_k0"][0].size == 0
    assert r["k2049"][2].tolist().count(-1) == 2046 and r["k2049"][3][2048] == CASES["k2049"][4][2048]
    assert sum(int((x[0] != 0).any()) for n, x in r.items() if n.startswith("random")) >= 4


@pytest.mark.parametrize("name", sorted(ec.bad_cases()))
def test_definition_refuses_a_bad_event_column(name):
    err, ev, K, mask, ids, node = ec.bad_cases()[name]
    with pytest.raises(ValueError, match=r"event\[%d\]" % node):
        graph.event_errors(err, ev, K, mask, node_id=ids)


def test_struct_layout_matches_header(tmp_path):
    """offsetof / sizeof of gtf_event_errors_io from a C probe against the ctypes mirror"""
    from gtf import _native as nat
    cls, t = nat.GtfEventErrorsIo, "gtf_event_errors_io"
    lines = ['  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, t, f) for f, _ in cls._fields_]
    lines.append('  printf("sizeof %%zu\\n", sizeof(%s));' % t)
    c = tmp_path / "p.c"
    c.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n"
                 % "\n".join(lines))
    exe = str(tmp_path / "p")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == len(cls._fields_) + 1 and int(got.pop("sizeof")) == ctypes.sizeof(cls)
    for f, v in got.items():
        assert getattr(cls, f).offset == int(v), f
    io = cls(n_nodes=3)
    assert io.struct_size == ctypes.sizeof(cls) and io.abi_version == nat.ABI_VERSION and io.n_nodes == 3
    assert "gtf_event_errors" in nat.SYMBOLS and "gtf_event_errors_workspace_bytes" in nat.SYMBOLS


def test_on_error_refusals():
    """an unknown policy is refused before anything touches a device"""
    from gtf import pipeline
    for bad in ("skip", None, True, "Isolate"):
        with pytest.raises(ValueError, match="on_error"):
            pipeline.run_batch([], on_error=bad)
        with pytest.raises(ValueError, match="on_error"):
            pipeline.build_events_dev([], 7, 7, on_error=bad)
    out = pipeline.run_batch([], on_error="isolate")       # (no event: nothing to load or launch)
    assert out == [] and out.errors == {}
    assert pipeline.run_batch([], on_error="raise") == []
    e = pipeline.BatchError("x", {1: 8})
    assert isinstance(e, ValueError) and e.events == {1: 8}
