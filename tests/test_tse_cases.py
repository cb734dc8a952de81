"""The directed a2 cases (tse_cases.py) on the CPU, before test_gpu_tse_cases.py holds the HIP
kernel to them.

  * every case reaches the branch it claims (its predicate on the oracle's output), and the nodes
    at which the oracle finds a singular H are the declared ones;
  * the oracle equals the record of the reference's own helper.compute_track_state_estimates
    (tests/golden/tse_cases.npz) at rtol 1e-12, non-finite entries equal in kind (NaN, +inf, -inf);
    the dict order (tse_rank) is the record's exactly;
  * where the reference raised, the oracle raises the same type and names the same source line;
  * every value that is compared as a finite number moves by less than 1e-9 relative in the oracle
    when the coordinates are perturbed by +-2^-46 relative, each coordinate of each node on its
    own. Only the coordinate that sits on the comparison under test is kept (Case.hold): a |z| equal
    to endcap_boundary is frozen, two coordinates that must stay equal move by one common factor.
    No case and no node is exempt;
  * the schedule of everything(): every bucket ends in a partial block, both edges of every bucket
    are there.

oracle/cpu_ref.cpp does not implement a2 (it restates the fused pass and the clustering), so there
is nothing of it to hold to the record here.
"""
import os
import re

import numpy as np
import pytest

import gtf_oracle as O
import tse_cases as TC
from fixtures import GOLDEN

NAMES = [c.name for c in TC.CASES]


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(GOLDEN, "tse_cases.npz"), allow_pickle=False)


def same_kind(a, b):
    """non-finite entries equal in kind; returns the mask of the entries finite in both"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN where the other is none"
    inf = np.isinf(a) | np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), "infinities differ"
    return np.isfinite(a) & np.isfinite(b)


def close(a, b, rtol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = same_kind(a, b)
    a, b = np.where(fin, a, 0.0), np.where(fin, b, 0.0)
    bad = ~(np.abs(a - b) <= rtol * np.abs(b))
    assert not bad.any(), (what, np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])


def recorded(record, case):
    """({slot field: array}, {node field: array}) of the record, or the 'Type file:line' it raised"""
    g, _ = TC.packed(case)
    assert np.array_equal(record[case.name + "__node_id"], g.node["node_id"])
    assert np.array_equal(record[case.name + "__slot_key"], g.slot["slot_key"])
    if case.name + "__raised" in record.files:
        return str(record[case.name + "__raised"])
    pre = case.name + "__"
    return ({k[len(pre) + 6:]: record[k] for k in record.files if k.startswith(pre + "slot__")},
            {k[len(pre) + 6:]: record[k] for k in record.files if k.startswith(pre + "node__")})


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch(name):
    case = TC.BY_NAME[name]
    info = TC.info_of(case)
    assert case.check is not None, "a case without a predicate proves nothing"
    case.check(info)
    assert sorted(set(n for n, _ in info["singular"])) == sorted(info["ix"][k] for k in case.raises)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference_record(record, name):
    case = TC.BY_NAME[name]
    if case.ref is not None:
        assert not any(k.startswith(name + "__") for k in record.files) and len(case.ref) > 20
        return
    rec = recorded(record, case)
    g, _ = TC.packed(case)
    if isinstance(rec, str):
        assert case.raises, "the reference raised where the case declares nothing"
        typ, where = rec.split()
        with np.errstate(all="ignore"), pytest.raises(getattr(np.linalg, typ, Exception)) as ei:
            O.compute_track_state_estimates(g, TC.P)
        assert type(ei.value).__name__ == typ
        f, line = re.search(r"\((\w+\.py):(\d+)\)", str(ei.value)).groups()
        assert "%s:%s" % (f, line) == where
        return
    assert not case.raises
    slot, node = rec
    out, onode, sing = TC.run_oracle(g)
    assert sing == []
    assert np.array_equal(slot["tse_rank"], g.slot["tse_rank"]), "dict order"
    for f in TC.FIELDS:
        close(out.slot[f], slot[f], 1e-12, (name, f))
    for f in TC.NODE_FIELDS:
        close(onode[f], node[f], 1e-12, (name, f))
    for f in ("xy_mean_var", "zr_mean_var"):   # the same numpy sums: bit for bit
        assert np.array_equal(onode[f], node[f], equal_nan=True), (name, f)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_well_conditioned(name):
    case = TC.BY_NAME[name]
    g, names = TC.packed(case)
    out, node, sing = TC.run_oracle(g)
    for seed in range(4):
        o2, n2, _ = TC.run_oracle(TC.perturbed(g, case.hold, names, seed))
        # a singular key's outputs are unspecified. (LAPACK's x * (1 / x) need not round to 1, so
        # whether np.linalg.inv notices x_B == x_0 depends on the last bit of x_0.)
        for _, k in sing:
            for f in TC.FIELDS:
                o2.slot[f][k] = np.nan
        for f in TC.FIELDS:
            close(o2.slot[f], out.slot[f], 1e-9, (name, f, seed))
        for f in TC.NODE_FIELDS:
            close(n2[f], node[f], 1e-9, (name, f, seed))


def test_schedule_of_everything():
    g, comps = TC.everything()
    deg = np.diff(g.slot_ptr)
    for b, gpb in TC.GROUPS_PER_BLOCK.items():
        n = int(sum(1 for d in deg if TC.bucket(d) == b))
        assert n > gpb and n % gpb == 1, (b, n)          # whole blocks and one group more
    for edge in (4, 5, 8, 9, 16, 17, 32, 33, 64, 65):   # both edges of every bucket
        assert (deg == edge).any(), edge
    # every case whose node has at most 8 slots stands in every bucket
    for case in TC.CASES:
        if TC.v_slots(case) <= 8:
            got = set(int(deg[c["ix"]["v"]]) for c in comps if c["case"] is case and c["slots"] is not None)
            assert got == set(TC.PAD_SLOTS), (case.name, got)
    # the padding holds no key
    for c in comps:
        for v in range(c["nodes"][0] + c["own"], c["nodes"][1]):
            assert deg[v] == 0
    assert len(set(g.node["node_id"].tolist())) == g.n_nodes
