"""tests/kl_prepare_cases.py on the CPU: every case through ParabolicKL(device="cpu"), asserting what
the case is there to exercise, so that the GPU test's definition really reaches each rule; the host
refusals of the device path's entry points; the ctypes mirrors of the new structs."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kl_prepare_cases as kc
from gtf import parabolic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rank(d, with_single):
    r = np.full(d.size, 9)
    r[d > 8] = 8
    for q in range(2, 9):
        r[d == q] = q - 1
    if with_single:
        r[d == 1] = 0
    return r


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_holds_its_claim(name):
    c = kc.case(name)
    claim = c["claim"][0] if isinstance(c["claim"], tuple) else c["claim"]
    arg = c["claim"][1] if isinstance(c["claim"], tuple) else None
    n = c["ptr"].size - 1
    assert c["gnn"].shape == (n, 4) and (c["truth"] is None or c["truth"].shape == (n,))
    assert c["is_edge"] is None or c["is_edge"].shape == c["src"].shape
    if c["error"] is None:
        assert c["ptr"][0] == 0 and (np.diff(c["ptr"]) >= 0).all() and c["ptr"][-1] == c["src"].size
        ptr, src = kc.cut(c)
        assert src.size == 0 or (src.min() >= 0 and src.max() < n)
        d0 = np.diff(ptr).astype(np.int64)
        for mode in c["modes"]:
            ordered, with_single, compact = mode
            k = kc.host(c, mode)
            assert k.n_nodes == n and k.n_slots == src.size
            if ordered:   # the stable argsort of the rank, the rank-9 nodes last
                r = _rank(d0, with_single)
                assert np.array_equal(k.node_of, np.argsort(r, kind="stable"))
                assert (np.diff(r[k.node_of]) >= 0).all()
                unlisted = int((r == 9).sum())
                assert (r[k.node_of][n - unlisted:] == 9).all() and k.n_listed == n - unlisted
                assert (k._g.n_d1 > 0) == (with_single and bool((d0 == 1).any()))   # the one-edge run
            else:
                lo = 1 if with_single else 2
                assert k.n_listed == int((d0 >= lo).sum())
            if compact:
                assert k.q is not None and (c["truth"] is None) == (k.truth32 is None)
    else:
        assert claim in ("source_n", "ptr_decreases", "nonfinite", "given")
    # ---- what the case is there for
    if claim == "empty":
        assert n == 0 and c["src"].size == 0
    elif claim == "no_slots":
        assert n == 1 and c["src"].size == 0
    elif claim == "every_degree":
        d = np.diff(c["ptr"])
        assert set(range(11)) | {65} <= set(d.tolist())
        assert kc.host(c, (False, False, False)).n_pairs >= 65 * 64 // 2 == 2080
    elif claim == "deg8_9":
        assert np.diff(c["ptr"])[:4].tolist() == [8, 9, 9, 8]
        k = kc.host(c, (True, False, False))
        assert k._g.n_deg[5] == 2 and k._g.count[3] == 2
    elif claim == "single_only":
        assert (np.diff(c["ptr"]) == 1).all()
        assert kc.host(c, (True, True, False)).n_listed == n and kc.host(c, (True, False, False)).n_listed == 0
        assert kc.host(c, (False, True, False)).lists[0].numel() == n and kc.host(c, (False, False, False)).n_listed == 0
    elif claim == "seeded":
        d = np.diff(c["ptr"])
        assert d.min() == 0 and d.max() == 10
        if n > 256:   # equal ranks on both sides of a block boundary
            r = _rank(d.astype(np.int64), True)
            past = set(r[256:].tolist())
            assert past <= set(r[:256].tolist()) and (n < 1025 or past == set(range(10)))
    elif claim == "interleaved":
        e = c["is_edge"]
        assert 0 < e.sum() < e.size and (np.diff(e.astype(int)) != 0).sum() > e.size // 4 and (c["src"] >= 0).all()
    elif claim == "minus1":
        e = c["is_edge"].astype(bool)
        assert (c["src"][~e] == -1).all() and (~e).sum() > 10 and (c["src"][e] >= 0).all()
    elif claim == "node_dropped":
        v = arg
        assert c["ptr"][v + 1] - c["ptr"][v] >= 3 and not c["is_edge"][c["ptr"][v]:c["ptr"][v + 1]].any()
        assert np.diff(kc.cut(c)[0])[v] == 0
    elif claim == "source_n":
        e = c["is_edge"].astype(bool)
        assert (c["src"][e] == n).sum() == 1 and (c["src"][e] <= n).all() and (c["src"][~e] == -1).all()
    elif claim == "ptr_decreases":
        assert (np.diff(c["ptr"]) < 0).sum() == 1
    elif claim in ("truth_plain", "truth_relabel", "truth_signed", "truth_absent"):
        for mode in c["modes"]:
            k = kc.host(c, mode)
            if claim == "truth_absent":
                assert k.truth32 is None and k._q.truth32 is None
                continue
            t64 = k.truth.numpy()
            t32 = k.truth32.numpy()
            if claim == "truth_plain":
                assert t64.min() == -(1 << 31) and t64.max() == (1 << 31) - 1 and np.array_equal(t32, t64)
            else:   # the relabel branch: dense ranks in signed order
                assert t64.min() < -(1 << 31) or t64.max() >= (1 << 31)
                u = np.unique(t64)
                assert t32.max() == u.size - 1 and np.array_equal(u[t32], t64) and u.size < t64.size
            if claim == "truth_signed":
                assert t64.min() < -(1 << 31) and t64.max() >= (1 << 31)
                assert t32[np.argmin(t64)] == 0   # (unsigned order would put a negative id last)
    elif claim in ("scale", "bump"):
        m = float(np.abs(c["gnn"][:, :2]).max())
        k = kc.host(c, c["modes"][0])
        assert k.scale == 2.0 ** (arg - 30)
        e = int(np.frexp(m)[1]) if m > 0 else 0
        assert (e == arg - 1) == (claim == "bump")   # e += 1 really fires
        if claim == "scale" and m > 0:
            assert m == 2.0 ** (arg - 1) and int(np.abs(k.q.numpy()).max()) == 1 << 29
        if claim == "bump":
            assert int(np.abs(k.q.numpy()).max()) == 1 << 29
    elif claim == "ties":
        k = kc.host(c, c["modes"][0])
        assert k.scale == arg
        x = c["gnn"][:, :2].reshape(-1) / arg
        half = x[np.abs(x - np.trunc(x)) == 0.5]
        assert half.size == 12 and (half > 0).sum() == 6
        q = k.q.numpy().reshape(-1)[np.abs(x - np.trunc(x)) == 0.5]
        assert (q % 2 == 0).all() and set(np.abs(q).tolist()) == {0, 2, 4, 6}
    elif claim == "nonfinite":
        assert not np.isfinite(c["gnn"][:, :2]).all()
        with pytest.raises(ValueError, match="non-finite coordinate"):
            kc.host(c, c["modes"][0])
    elif claim == "given":
        if arg:
            k = kc.host(c, c["modes"][0])
            assert k.scale == c["scale"] != parabolic.quantise_xy(c["gnn"])[1]
        else:
            assert parabolic.quantise_xy(c["gnn"])[1] == 2 * c["scale"]   # one step too small
            with pytest.raises(ValueError, match="does not fit scale"):
                kc.host(c, c["modes"][0])
    elif claim == "vol7x3":
        assert n == 3 * 8748 and c["src"].size == 3 * 14766
    else:
        assert claim == "random"


def test_every_rule_has_a_case():
    claims = {c["claim"][0] if isinstance(c["claim"], tuple) else c["claim"] for c in kc.CASES.values()}
    assert {"empty", "no_slots", "every_degree", "deg8_9", "single_only", "seeded", "interleaved", "minus1",
            "node_dropped", "source_n", "ptr_decreases", "truth_plain", "truth_relabel", "truth_signed", "truth_absent",
            "scale", "bump", "ties", "nonfinite", "given", "random"} <= claims
    assert sum(1 for n in kc.CASES if n.startswith("rand")) == 20
    kinds = {(kc.CASES[n]["truth"] is None, kc.CASES[n]["is_edge"] is None) for n in kc.CASES if n.startswith("rand")}
    assert len(kinds) == 4


def test_lazy_host_copies_do_not_change_the_host_object():
    """node_of, slot_of, degree, slot_ptr_host and pair_ptr_host are plain attributes of a host-built object"""
    c = kc.case("n257")
    k = kc.host(c, (True, True, True))
    assert k.node_of.dtype == np.int64 and k.slot_of.dtype == np.int64 and k.degree.dtype == np.int64
    assert np.array_equal(k.degree, np.diff(k.slot_ptr_host)) and k.pair_ptr_host[-1] == k.n_pairs
    k0 = kc.host(c, (False, False, False))
    assert k0.node_of is None and k0.slot_of is None
    node, i, j = k.pair_index()
    assert node.size == k.n_pairs and (i > j).all() and (j >= 0).all()


def test_host_refusals():
    c = kc.case("n255")
    with pytest.raises(ValueError, match="prepare must be"):
        parabolic.ParabolicKL(c["ptr"], c["src"], c["gnn"], device="cpu", prepare="gpu")
    with pytest.raises(ValueError, match="tiled layout"):
        parabolic.ParabolicKL(c["ptr"], c["src"], c["gnn"], device="cpu", tile=64, prepare="device")


def test_entry_points_refuse_on_the_host():
    """the checks made before any launch: wrong ABI -3; null arguments, negative sizes, a small workspace -2"""
    from gtf import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib()
    one = ctypes.c_void_p(256)   # (never dereferenced: every call is refused first)

    def call(pin, buf=None, ws=one, nb=1 << 30, g=None, q=None, counts=None):
        buf = buf or nat.GtfKlPrepareBuf(one, one, one, one, one, one, one, one, one, one)
        g, q, counts = g or nat.GtfKlGraph(), q or nat.GtfKlQ32(), counts or nat.GtfKlCounts()
        rc = L.gtf_kl_prepare(ctypes.byref(pin), ctypes.byref(buf), ctypes.byref(g), ctypes.byref(q),
                              ctypes.byref(counts), ws, nb, None)
        return rc, L.gtf_last_error().decode()

    ok = dict(n_nodes=4, n_slots=3, slot_ptr=one, slot_src=one, gnn=one, gnn_stride=4)
    pin = nat.GtfKlPrepareIn(**ok)
    pin.struct_size += 8
    assert call(pin)[0] == -3
    pin = nat.GtfKlPrepareIn(**ok)
    pin.abi_version += 1
    rc, msg = call(pin)
    assert rc == -3 and "ABI mismatch" in msg
    for bad, word in ((dict(n_nodes=-1), "negative"), (dict(n_slots=-2), "negative"), (dict(gnn_stride=3), "gnn_stride"),
                      (dict(layout=2), "layout"), (dict(slot_ptr=None), "slot_ptr"), (dict(slot_src=None), "slot_src"),
                      (dict(gnn=None), "gnn"), (dict(compact=1, scale=-1.0), "scale"),
                      (dict(compact=1, scale=float("nan")), "scale")):
        rc, msg = call(nat.GtfKlPrepareIn(**dict(ok, **bad)))
        assert rc == -2 and word in msg, (bad, msg)
    for field in ("slot_ptr", "slot_src", "xy", "pair_ptr", "list"):
        buf = nat.GtfKlPrepareBuf(one, one, one, one, one, one, one, one, one, one)
        setattr(buf, field, None)
        rc, msg = call(nat.GtfKlPrepareIn(**ok), buf)
        assert rc == -2 and "missing array" in msg, field
    for extra, field in ((dict(layout=1), "node_of"), (dict(layout=1), "slot_of"), (dict(compact=1), "q"),
                         (dict(truth=one), "truth"), (dict(truth=one, compact=1), "truth32")):
        buf = nat.GtfKlPrepareBuf(one, one, one, one, one, one, one, one, one, one)
        setattr(buf, field, None)
        rc, msg = call(nat.GtfKlPrepareIn(**dict(ok, **extra)), buf)
        assert rc == -2 and field in msg, field
    need = L.gtf_kl_prepare_workspace_bytes(4, 3)
    assert need > 0 and L.gtf_kl_prepare_workspace_bytes(0, 0) > 0 and L.gtf_kl_prepare_workspace_bytes(-5, -5) > 0
    assert L.gtf_kl_prepare_workspace_bytes(1000, 3) > need and L.gtf_kl_prepare_workspace_bytes(4, 1000) > need
    rc, msg = call(nat.GtfKlPrepareIn(**ok), nb=need - 1)
    assert rc == -2 and "workspace" in msg
    assert call(nat.GtfKlPrepareIn(**ok), ws=None)[0] == -2
    # gtf_kl_coords, gtf_kl_pair_rows
    assert L.gtf_kl_coords(-1, one, 4, None, one, None, 0.0, one, None) == -2
    assert L.gtf_kl_coords(4, one, 3, None, one, None, 0.0, one, None) == -2
    assert L.gtf_kl_coords(4, one, 4, None, None, None, 0.0, one, None) == -2
    assert L.gtf_kl_coords(4, one, 4, None, one, one, 0.0, one, None) == -2       # q without a scale
    assert L.gtf_kl_coords(4, one, 4, None, one, None, 0.0, None, None) == -2     # no error word
    assert L.gtf_kl_coords(4, None, 4, None, one, None, 0.0, one, None) == -2
    assert L.gtf_kl_coords(0, None, 4, None, one, None, 0.0, one, None) == 0
    g = nat.GtfKlGraph(n_nodes=4, slot_ptr=one, pair_ptr=one)
    assert L.gtf_kl_pair_rows(None, 1, None, None, 0, one, one, one, None, None) == -2
    assert L.gtf_kl_pair_rows(ctypes.byref(g), -1, None, None, 0, one, one, one, None, None) == -2
    assert L.gtf_kl_pair_rows(ctypes.byref(g), 1, None, None, 2, one, one, one, None, None) == -2
    assert L.gtf_kl_pair_rows(ctypes.byref(g), 1, None, one, 0, one, one, one, None, None) == -2
    assert L.gtf_kl_pair_rows(ctypes.byref(g), 1, None, None, 0, None, one, one, None, None) == -2
    assert L.gtf_kl_pair_rows(ctypes.byref(g), 0, None, None, 0, None, None, None, None, None) == 0


def test_struct_layout_matches_header():
    """offsetof() / sizeof() of the structs gtf_kl_prepare adds against their ctypes mirrors"""
    from gtf import _native as nat
    py = {"gtf_kl_prepare_in": nat.GtfKlPrepareIn, "gtf_kl_prepare_buf": nat.GtfKlPrepareBuf,
          "gtf_kl_counts": nat.GtfKlCounts, "gtf_kl_q32": nat.GtfKlQ32, "gtf_kl_out32": nat.GtfKlOut32}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "p.c")
        open(src, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values())
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    assert nat.GtfKlPrepareIn().struct_size == ctypes.sizeof(nat.GtfKlPrepareIn)
    assert (nat.KL_ERR_SLOT_PTR, nat.KL_ERR_SOURCE, nat.KL_ERR_NONFINITE, nat.KL_ERR_FIT, nat.KL_ERR_SCALE,
            nat.KL_ERR_NODE_OF) == (1, 2, 4, 8, 16, 32)
