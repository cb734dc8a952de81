"""tests/score_cases.py on the host: every case reaches the branch it is named for on
gtf.metrics.reconstruction_efficiency AND on oracle/metrics_oracle.py (the reference script
restated loop for loop), and the two agree. The device runs the same cases in
tests/test_gpu_score.py."""
import numpy as np
import pandas as pd
import pytest

import metrics_oracle as MO
import score_cases as SC
from gtf import metrics

COLS = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")


def _oracle(case, cands):
    m = case["m"]
    hits = pd.DataFrame({c: getattr(m, c) for c in COLS})
    pid, px, py = case["particles"]
    parts = pd.DataFrame({"particle_id": pid, "px": px, "py": py})
    ref, pixel = MO.reference_tracks(parts, hits[["hit_id", "particle_id"]], hits, 7, 7)
    return MO.efficiency(cands, MO.hit_dissociation(hits), ref, pixel), ref, pixel


def check(case, r):
    """what the case is named for, on a Result of its flattened candidates"""
    e = case["expect"]
    for k, got in (("pid", r.reconstructed_pid), ("n_good", r.n_good), ("matched", r.matched)):
        if k in e:
            assert np.array_equal(got, np.array(e[k], got.dtype)), k
    if "purities" in e:
        assert np.array_equal(r.track_purities, e["purities"][0]) and np.array_equal(r.particle_purities, e["purities"][1])


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_reaches_its_branch_on_host_and_oracle(name):
    case = SC.CASES[name]()
    e = case["expect"]
    ptr, ids, cands = SC.flatten(case)
    if e.get("raises"):
        with pytest.raises(ValueError, match="no hit_dissociation"):
            SC.host_result(case)
        with pytest.raises(KeyError):
            _oracle(case, cands)
        return
    r = SC.host_result(case)
    check(case, r)
    t = SC.tables(case)
    assert r.n_reference == t.n_reference == int(t.part_ref.sum())
    # the reference script raises on an empty candidate (max() of an empty Counter); it never
    # writes one, so the oracle scores the others -- which the empty ones cannot change
    (n_reco, n_ref, tp, pp, eff), ref, pixel = _oracle(case, [c for c in cands if len(c)])
    assert (n_reco, n_ref) == (r.n_reconstructed, r.n_reference)
    assert n_ref == 0 or eff == r.efficiency_str
    assert np.array_equal(tp, r.track_purities) and np.array_equal(pp, r.particle_purities)
    # the per-candidate totals, and the details some cases name
    cand_of, part = metrics.candidate_particles(ptr, ids, t.node_id, t.node_ptr.astype(np.int64), t.node_part)
    pid, good, total = metrics.majority(len(cands), cand_of, part)
    assert np.array_equal(pid, r.reconstructed_pid) and np.array_equal(good, r.n_good)
    if "total" in e:
        assert list(total) == e["total"]
    if e.get("tie"):
        for c in range(len(cands)):
            ids_c = part[cand_of == c]
            assert sorted(np.unique(ids_c, return_counts=True)[1])[-2:] == [good[c], good[c]]   # a real tie
            assert ids_c[0] == pid[c]
    if "first_at" in e:
        assert int(np.flatnonzero(part == pid[0])[0]) == e["first_at"] and total[0] == 65
    if "hits" in e:
        for p, h in zip(e["pid"], e["hits"]):
            assert t.part_hits[np.searchsorted(t.part_id, p)] == h
        # 2n == hits, one short of it, 2n == total, one short of it
        assert [(2 * g - h, 2 * g - n) for g, h, n in zip(e["n_good"], e["hits"], e["total"])] == \
            [(0, 3), (-1, 3), (0, 0), (0, -1)]
    for p in e.get("absent", ()):
        assert p not in t.part_id
    for p in e.get("non_reference", ()):
        assert t.part_ref[np.searchsorted(t.part_id, p)] == 0 and t.part_id[np.searchsorted(t.part_id, p)] == p
    if "ends" in e:
        assert e["ends"] == (t.node_id[0], t.node_id[-1])
    if name == "sizes":
        assert sorted(set(total)) == list(SC.SIZES) and max(np.diff(t.node_ptr)) == 6
    if name == "ids_60bit":
        assert (pid[0] & 0xffffffff) == (part[cand_of == 0][0] & 0xffffffff) and pid[0] != part[cand_of == 0][0]
    if name == "pid_zero_noise":
        assert 0 not in t.part_id and total[0] > 0
    if name == "pid_zero_particle":
        assert t.part_id[0] == 0 and t.part_ref[0] == 1
    if name == "repeated_member":
        assert len(set(cands[0])) < len(cands[0])


def test_the_table_of_cases_is_complete():
    assert len(SC.CASES) == 17
    both = [SC.CASES[n]() for n in ("dup_across_short_first", "dup_across_full_first")]
    assert all(len(c["calls"]) == 2 for c in both)
