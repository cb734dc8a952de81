"""tests/truth_cases.py on the host: every case reaches the branch it is named for on
gtf.metrics.truth_tables, the host function agrees with oracle/metrics_oracle.py's
reference_tracks and hit_dissociation wherever pandas can express the case, the 20 seeded random
events that the device runs are not vacuous, and the ctypes mirrors of the gtf_truth_build
structs match include/gtf.h. The device runs the same cases in tests/test_gpu_truth.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pandas as pd
import pytest

import metrics_oracle as MO
import truth_cases as TC
from gtf import metrics

COLS = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(case, t):
    """what the case is named for, on a TruthTables"""
    e = case["expect"]
    assert t.node_id.dtype == t.node_part.dtype == t.part_id.dtype == np.int64
    assert t.node_ptr.dtype == t.part_hits.dtype == np.int32 and t.part_ref.dtype == np.uint8
    assert (t.node_id.size, t.node_part.size, t.part_id.size, t.n_reference) == e["counts"]
    assert t.node_ptr.size == t.node_id.size + 1 and t.part_hits.size == t.part_ref.size == t.part_id.size
    assert t.n_reference == int(t.part_ref.sum())
    assert np.all(np.diff(t.node_id) > 0) and np.all(np.diff(t.part_id) > 0)       # ascending as signed int64
    assert t.node_ptr[0] == 0 and t.node_ptr[-1] == t.node_part.size and np.all(np.diff(t.node_ptr) > 0)
    for node, parts in e.get("node_part", {}).items():
        k = int(np.searchsorted(t.node_id, node))
        assert t.node_id[k] == node and list(t.node_part[t.node_ptr[k]:t.node_ptr[k + 1]]) == parts, node
    for node, n in e.get("node_len", {}).items():
        k = int(np.searchsorted(t.node_id, node))
        assert t.node_id[k] == node and t.node_ptr[k + 1] - t.node_ptr[k] == n, node
    for pid, (hits, ref) in e.get("part", {}).items():
        k = int(np.searchsorted(t.part_id, pid))
        assert t.part_id[k] == pid and (t.part_hits[k], t.part_ref[k]) == (hits, ref), pid
    if "part" in e:
        assert sorted(e["part"]) == list(t.part_id)
    for pid in e.get("absent", ()):
        assert pid not in t.part_id
    if "order" in e:
        assert list(t.part_id) == e["order"] and e["order"][0] < 0 < e["order"][-1]


def _frames(case):
    m = case["m"]
    hits = pd.DataFrame({c: getattr(m, c) for c in COLS})
    pid, px, py = case["particles"]
    parts = pd.DataFrame({"particle_id": pid, "px": px, "py": py})
    if case["truth"] is None:
        truth = hits[["hit_id", "particle_id"]]
    else:
        truth = pd.DataFrame({"hit_id": case["truth"][0], "particle_id": case["truth"][1]})
    return parts, truth, hits


def check_against_oracle(case, t):
    """reference_tracks on every case; hit_dissociation where pandas can express it: the oracle
    looks a hit up in the mapping itself and takes .item(), so every hit id on one row only and
    no truth columns of their own"""
    parts, truth, hits = _frames(case)
    ref, pixel = MO.reference_tracks(parts, truth, hits, *case["window"])
    assert sorted(int(p) for p in ref) == list(t.part_id[t.part_ref == 1])
    ids, n = np.unique(pixel.particle_id.to_numpy(np.int64), return_counts=True)
    assert np.array_equal(ids, t.part_id) and np.array_equal(n, t.part_hits)
    for p, h in ref.items():
        assert len(h) == t.part_hits[np.searchsorted(t.part_id, p)]
    m = case["m"]
    if case["truth"] is None and np.unique(m.hit_id).size == m.hit_id.size and m.hit_id.size:
        hd = MO.hit_dissociation(hits)
        assert sorted(hd) == list(t.node_id)
        for k, node in enumerate(t.node_id):
            assert hd[int(node)] == list(t.node_part[t.node_ptr[k]:t.node_ptr[k + 1]])
        return True
    return False


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_case_reaches_its_branch_on_host_and_oracle(name):
    case = TC.CASES[name]()
    if case["expect"].get("raises"):
        with pytest.raises(ValueError, match="no truth row"):
            TC.host_tables(case)
        return
    t = TC.host_tables(case)
    check(case, t)
    with_hd = check_against_oracle(case, t)
    m = case["m"]
    if name == "dup_pairs":
        pairs = np.stack([m.node_idx, m.hit_id], 1)
        same = np.flatnonzero(np.all(pairs == pairs[0], 1))
        assert list(same[:2]) == [0, 1] and same[2] > 3 and not with_hd      # next to it, and far from it
    if name == "interleaved_descending":
        own = np.flatnonzero(m.node_idx == 20)
        assert np.all(np.diff(own) > 1) and np.all(np.diff(m.hit_id[own]) < 0) and with_hd
    if name == "truth_two_rows":
        th, tp = case["truth"]
        assert list(tp[th == 100]) == [8, 9]
    if name in ("window_one", "window_several"):
        lo, hi = case["window"]
        assert {lo - 1, lo, hi, hi + 1} <= set(m.volume_id) and (lo == hi) == (name == "window_one")
    if name.startswith("pt_cut"):
        pid, px, py = case["particles"]
        pt = np.sqrt(px ** 2 + py ** 2)
        assert pt[pid == 1][0] == 1.0 and pt[pid == 2][0] < 1.0
        assert px[pid == 2][0] == np.nextafter(px[pid == 1][0], 0.0) and px[pid == 1][0] != 0.6
        assert 3 not in pid and 77 not in m.particle_id and (0 in pid) == (name == "pt_cut_zero_present")
    if name == "ids":
        assert m.node_idx.max() > 1 << 32 and m.hit_id.max() > 1 << 32 and m.node_idx.min() < 0
    if name == "runs":
        assert sorted(t.part_hits)[:5] == list(TC.RUNS[:5]) and m.node_idx[-1] == t.node_id[-1]
        assert m.particle_id[-1] == t.part_id[-1] and t.part_hits[-1] == 1025 + 70
    if name.startswith("range_"):
        bad = np.concatenate([m.volume_id, m.layer_id, m.module_id])
        assert ((bad < 0) | (bad >= 1 << 21)).sum() == 1


def test_the_table_of_cases_is_complete():
    assert len(TC.CASES) == 20
    assert sum(bool(TC.CASES[n]()["expect"].get("dev_raises")) for n in TC.CASES) == 2
    assert sum(TC.CASES[n]()["truth"] is not None for n in TC.CASES) == 3


def _not_vacuous(case):
    """-> what the event holds of: a reference track, a particle disqualified by a repeated
    (volume, layer, module) alone, a particle below num_layers, a repeated (node, hit) pair, a hit
    with two truth rows"""
    m = case["m"]
    t = TC.host_tables(case)
    th = m.hit_id if case["truth"] is None else case["truth"][0]
    tp = m.particle_id if case["truth"] is None else case["truth"][1]
    rows = metrics.region_hits(m, th, tp, metrics.high_pt_particles(*case["particles"]), *case["window"])
    by_dup = below = 0
    for p, ref in zip(t.part_id, t.part_ref):
        r = rows & (m.particle_id == p)
        n_layers = len(set(zip(m.volume_id[r], m.layer_id[r])))
        keys = list(zip(m.volume_id[r], m.layer_id[r], m.module_id[r]))
        by_dup += n_layers >= metrics.NUM_DISTINCT_LAYERS and len(set(keys)) < len(keys) and not ref
        below += n_layers < metrics.NUM_DISTINCT_LAYERS and not ref
    pairs = np.stack([m.node_idx, m.hit_id], 1)
    return (t.n_reference, by_dup, below, len(pairs) - len(np.unique(pairs, axis=0)), th.size - np.unique(th).size)


@pytest.mark.parametrize("separate", [False, True])
def test_random_events_are_not_vacuous(separate):
    for seed in range(TC.N_RANDOM):
        case = TC.random_event(seed, separate)
        assert case["m"].node_idx.size <= 2000 and (case["truth"] is not None) == separate
        held = _not_vacuous(case)
        assert all(x >= 1 for x in held), (seed, held)
        check_against_oracle(case, TC.host_tables(case))


def test_truth_struct_layout_matches_header():
    """offsetof() / sizeof() of every field of the gtf_truth_build structs, from a C probe compiled
    against the header, equal the ctypes mirrors'"""
    from gtf import _native as nat
    py = {"gtf_truth_in": nat.GtfTruthIn, "gtf_truth_buf": nat.GtfTruthBuf, "gtf_truth_counts": nat.GtfTruthCounts,
          "gtf_truth": nat.GtfTruth}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(c, "w") as f:
            f.write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).split("\n") if line)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values())
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    assert (nat.TRUTH_ERR_MISSING, nat.TRUTH_ERR_RANGE, nat.TRUTH_ID_LIMIT) == (1, 2, 1 << 21)


def test_truth_build_refuses_bad_arguments_without_a_gpu():
    """null arrays, negative sizes, a small workspace, an inverted window (-2) and another ABI (-3)
    are decided on the host before any device work"""
    from gtf import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib()
    assert L.gtf_truth_build_workspace_bytes(0, 0, 0) > 0
    sizes = [L.gtf_truth_build_workspace_bytes(*a) for a in ((-5, -5, -5), (0, 0, 0), (10, 0, 0), (10, 10, 0), (10, 11, 0),
                                                             (10, 11, 7), (1000, 11, 7), (1000, 2000, 7), (1000, 2000, 3000))]
    assert sizes[0] == sizes[1] and sizes[2] == sizes[3] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > sizes[1]
    fake = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused first)
    cols = {k: fake for k in ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")}
    buf = nat.GtfTruthBuf(*([fake] * 6))
    out, cnt = nat.GtfTruth(), nat.GtfTruthCounts()

    def call(tin, b=buf, ws=fake, nb=1 << 40):
        return L.gtf_truth_build(ctypes.byref(tin), ctypes.byref(b), ctypes.byref(out), ctypes.byref(cnt), ws,
                                 ctypes.c_size_t(nb), None)

    ok = dict(n_rows=4, n_truth=0, n_particles=0, num_layers=4, min_volume=7, max_volume=7, pt_cut=1.0, **cols)
    other = nat.GtfTruthIn(**ok)
    other.abi_version += 1
    assert call(other) == -3 and b"ABI mismatch" in L.gtf_last_error()
    other = nat.GtfTruthIn(**ok)
    other.struct_size -= 8
    assert call(other) == -3
    for change, text in (({"n_rows": -1}, b"negative"), ({"n_truth": -1}, b"negative"), ({"n_particles": -2}, b"negative"),
                         ({"min_volume": 8}, b"min_volume > max_volume"), ({"hit_id": None}, b"mapping column"),
                         ({"module_id": None}, b"mapping column"), ({"n_truth": 3}, b"truth_hit"),
                         ({"n_particles": 3}, b"part_id / px / py"), ({"n_rows": (1 << 30) + 1}, b"2^30")):
        assert call(nat.GtfTruthIn(**dict(ok, **change))) == -2, change
        assert text in L.gtf_last_error(), (change, L.gtf_last_error())
    for k in range(6):
        ptrs = [fake] * 6
        ptrs[k] = None
        assert call(nat.GtfTruthIn(**ok), b=nat.GtfTruthBuf(*ptrs)) == -2 and b"missing array" in L.gtf_last_error()
    need = L.gtf_truth_build_workspace_bytes(4, 0, 0)
    assert call(nat.GtfTruthIn(**ok), nb=need - 1) == -2 and b"workspace" in L.gtf_last_error()
    assert call(nat.GtfTruthIn(**ok), ws=None) == -2 and b"workspace" in L.gtf_last_error()
    assert L.gtf_truth_build(None, ctypes.byref(buf), ctypes.byref(out), ctypes.byref(cnt), fake, ctypes.c_size_t(1), None) == -2
