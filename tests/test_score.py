"""The device scoring (gtf_score_reset / _candidates / _finish) without a GPU: the header
declares the entry points and the library exports them, the ctypes mirrors of the new structs
match the header, the workspace sizes behave, every refusal the header promises on the host
comes back before any launch, and gtf.metrics.truth_tables restates reference_tracks /
node_particles on the golden event."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from fixtures import GOLDEN
from gtf import _native as nat
from gtf import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NAMES = ("gtf_score_reset", "gtf_score_workspace_bytes", "gtf_score_candidates", "gtf_score_finish_workspace_bytes",
         "gtf_score_finish")
SIZES = (0, 1, 3, 4, 5, 255, 256, 257, 1000, 4097, 100000, 1 << 20)
STRUCTS = {"gtf_truth": "GtfTruth", "gtf_score_state": "GtfScoreState", "gtf_score_out": "GtfScoreOut",
           "gtf_score_counts": "GtfScoreCounts"}


def _lib():
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built (run __graft_entry__.build())")
    return nat.lib()


def test_header_declares_and_library_exports():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", src, re.M))
    assert set(NAMES) <= declared
    assert set(NAMES) <= set(nat.SYMBOLS)
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gtf_\w+)", out))
    for name in NAMES:   # every declaration cites the reference lines it replaces
        at = src.index(" %s(" % name)
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"reconstruction_efficiency\.py:\d+-\d+", comment), name
    assert "#define GTF_ABI_VERSION 8u" in src and nat.ABI_VERSION == 8


def test_structs_match_header():
    """offsetof() / sizeof() of the four new structs from a C probe against the ctypes mirrors"""
    py = {t: getattr(nat, c) for t, c in STRUCTS.items()}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    for k in ("MISSING", "WORKSPACE", "RANGE"):
        lines.append('  printf("err.%s %%u\\n", GTF_SCORE_ERR_%s);' % (k, k))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == 12 + 6 + 4 + 2 + 4 + 3
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        elif t == "err":
            assert getattr(nat, "SCORE_ERR_" + f) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    assert nat.GtfTruth().struct_size == ctypes.sizeof(nat.GtfTruth) and nat.GtfTruth().abi_version == 8


def test_workspace_sizes():
    L = _lib()
    ws, fin = L.gtf_score_workspace_bytes, L.gtf_score_finish_workspace_bytes
    assert ws(0, 0) > 0 and fin(0) > 0 and ws(-5, -5) == ws(0, 0) and fin(-1) == fin(0)
    for other in (0, 1000):
        last_c = last_m = last_f = 0
        for n in SIZES:
            assert ws(n, other) >= last_c and ws(other, n) >= last_m and fin(n) >= last_f, n
            last_c, last_m, last_f = ws(n, other), ws(other, n), fin(n)
    # three words per candidate; a row, a length and an offset per member
    assert ws(1000, 6000) >= 12 * 1000 + 20 * 6000
    assert fin(1000) >= 16 * 1000


def _args(L, truth=None, state=None, n_cand=4, group=0, ws_bytes=None, ptr=True, ids=True):
    """gtf_score_candidates with host buffers and a NULL stream: only for calls the library must
    refuse, or finish, on the host (nothing may be launched, so nothing reads the buffers)"""
    arr = ctypes.create_string_buffer(256)
    a = ctypes.cast(arr, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    if truth is None:
        truth = nat.GtfTruth(n_nodes=2, n_entries=2, n_particles=2, node_id=a, node_ptr=a, node_part=a, part_id=a,
                             part_hits=a, part_ref=a)
    if state is None:
        state = nat.GtfScoreState(2, 0, a, a, a, a)
    need = L.gtf_score_workspace_bytes(max(n_cand, 0), 16)
    n = need if ws_bytes is None else ws_bytes
    buf = ctypes.create_string_buffer(max(n, 1))
    rc = L.gtf_score_candidates(ctypes.byref(truth), a if ptr else null, a if ids else null, n_cand, group, None,
                                ctypes.byref(state), ctypes.cast(buf, ctypes.c_void_p), ctypes.c_size_t(n), null)
    return rc, (arr, buf, truth, state)


def test_abi_mismatch_is_refused_on_the_host():
    L = _lib()
    arr = ctypes.create_string_buffer(256)
    a = ctypes.cast(arr, ctypes.c_void_p)
    for mutate in ("abi", "size"):
        t = nat.GtfTruth(n_nodes=2, n_entries=2, n_particles=2, node_id=a, node_ptr=a, node_part=a, part_id=a,
                         part_hits=a, part_ref=a)
        if mutate == "abi":
            t.abi_version = nat.ABI_VERSION + 1
        else:
            t.struct_size -= 8
        assert _args(L, truth=t)[0] == -3 and b"ABI mismatch" in L.gtf_last_error()
        st = nat.GtfScoreState(2, 0, a, a, a, a)
        cnt = nat.GtfScoreCounts(7, 7)
        assert L.gtf_score_finish(ctypes.byref(t), ctypes.byref(st), a, a, a, a, a, ctypes.byref(cnt), a,
                                  ctypes.c_size_t(1 << 20), None) == -3
        assert (cnt.n_reconstructed, cnt.error) == (7, 7)


def test_null_and_inconsistent_arguments_are_refused_on_the_host():
    L = _lib()
    arr = ctypes.create_string_buffer(256)
    a = ctypes.cast(arr, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    st = nat.GtfScoreState(2, 0, a, a, a, a)
    assert L.gtf_score_candidates(None, a, a, 4, 0, None, ctypes.byref(st), a, ctypes.c_size_t(1 << 20), None) == -2
    assert b"null gtf_truth" in L.gtf_last_error()
    t = nat.GtfTruth(n_nodes=2, n_entries=2, n_particles=2, node_id=a, node_ptr=a, node_part=a, part_id=a,
                     part_hits=a, part_ref=a)
    assert L.gtf_score_candidates(ctypes.byref(t), a, a, 4, 0, None, None, a, ctypes.c_size_t(1 << 20), None) == -2
    assert b"null gtf_score_state" in L.gtf_last_error()
    for f in ("node_id", "node_ptr", "node_part", "part_id", "part_hits", "part_ref"):
        kw = {k: a for k in ("node_id", "node_ptr", "node_part", "part_id", "part_hits", "part_ref") if k != f}
        bad = nat.GtfTruth(n_nodes=2, n_entries=2, n_particles=2, **kw)
        assert _args(L, truth=bad)[0] == -2 and f.encode() in L.gtf_last_error(), f
    assert _args(L, truth=nat.GtfTruth(n_nodes=-1, node_ptr=a))[0] == -2 and b"negative" in L.gtf_last_error()
    assert _args(L, state=nat.GtfScoreState(3, 0, a, a, a, a))[0] == -2 and b"differs" in L.gtf_last_error()
    assert _args(L, state=nat.GtfScoreState(2, 0, null, a, a, a))[0] == -2
    assert _args(L, state=nat.GtfScoreState(2, 0, a, a, a, null))[0] == -2
    assert _args(L, n_cand=-1)[0] == -2 and b"n_cand" in L.gtf_last_error()
    assert _args(L, group=-1)[0] == -2 and b"group" in L.gtf_last_error()
    assert _args(L, ptr=False)[0] == -2 and b"cand_ptr" in L.gtf_last_error()
    assert _args(L, ids=False)[0] == -2 and b"cand_ids" in L.gtf_last_error()
    assert _args(L, ws_bytes=L.gtf_score_workspace_bytes(4, 0) - 1)[0] == -2 and b"workspace" in L.gtf_last_error()
    # no candidates: nothing to launch, whatever else is missing
    assert _args(L, n_cand=0, ptr=False, ids=False, ws_bytes=0)[0] == 0
    # reset and finish
    assert L.gtf_score_reset(None, None) == -2
    assert L.gtf_score_reset(ctypes.byref(nat.GtfScoreState(2, 0, null, a, a, a)), None) == -2
    cnt = nat.GtfScoreCounts()
    assert L.gtf_score_finish(ctypes.byref(t), ctypes.byref(st), a, a, a, a, a, None, a, ctypes.c_size_t(1 << 20), None) == -2
    assert L.gtf_score_finish(ctypes.byref(t), ctypes.byref(st), a, a, a, a, a, ctypes.byref(cnt), a,
                              ctypes.c_size_t(L.gtf_score_finish_workspace_bytes(2) - 1), None) == -2
    assert L.gtf_score_finish(ctypes.byref(t), ctypes.byref(nat.GtfScoreState(3, 0, a, a, a, a)), a, a, a, a, a,
                              ctypes.byref(cnt), a, ctypes.c_size_t(1 << 20), None) == -2


def test_truth_tables_on_the_golden_event():
    z = np.load(os.path.join(GOLDEN, "metrics_vol7.npz"), allow_pickle=False)
    m = metrics.HitMapping(*(z["map__" + c] for c in ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id",
                                                       "module_id")))
    pid, px, py = z["particles__particle_id"], z["particles__px"], z["particles__py"]
    t = metrics.truth_tables(m, pid, px, py, 7, 7)
    rows = metrics.region_hits(m, m.hit_id, m.particle_id, metrics.high_pt_particles(pid, px, py), 7, 7)
    ref_ids, ref_hits, (reg_ids, reg_hits) = metrics.reference_tracks(m, rows)
    nid, nptr, npart = metrics.node_particles(m)
    assert (t.n_reference, t.part_id.size, t.node_id.size, t.node_part.size) == (163, 246, 8748, 13129)
    assert np.array_equal(t.part_id, reg_ids) and np.array_equal(t.part_hits, reg_hits)
    assert np.array_equal(t.part_id[t.part_ref == 1], ref_ids) and np.array_equal(t.part_hits[t.part_ref == 1], ref_hits)
    assert np.array_equal(t.node_id, nid) and np.array_equal(t.node_ptr, nptr) and np.array_equal(t.node_part, npart)
    assert [a.dtype for a in (t.node_id, t.node_ptr, t.node_part, t.part_id, t.part_hits, t.part_ref)] == \
        [np.int64, np.int32, np.int64, np.int64, np.int32, np.uint8]
    assert np.all(np.diff(t.node_id) > 0) and np.all(np.diff(t.part_id) > 0)
    assert t.part_id.max() >= 1 << 58 and 0 in t.node_part   # 60-bit ids, and the noise id occurs
    assert 1 <= np.diff(t.node_ptr).min() and np.diff(t.node_ptr).max() <= 6
