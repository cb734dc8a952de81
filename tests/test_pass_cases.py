"""The directed fused-pass cases (pass_cases.py) on the CPU: every case is pinned to the record of
the reference's own stage functions (tests/golden/pass_cases.npz, make_golden_pass_cases.py), the
oracle and the C++ restatement to that, before test_gpu_pass_cases.py holds the HIP path to the
oracle on the same components.

  * the oracle reproduces the recorded reference output of every case, in every padded variant:
    masks, ranks and flags exactly, clustering outputs bit for bit, other floats within 1e-6;
  * where the reference raised, the oracle raises on that component alone, names the same source
    line, and the node it raises at is the declared one;
  * every case reaches what it declares (its predicate on the oracle's output);
  * cpu_ref.full_pass / cpu_ref.cluster on all the components of a (stage, Params) group return
    exactly the OR of the declared bits, and equal the oracle on the clean components;
  * the clean cases are well conditioned: ulp-level perturbations of the inputs flip no mask and
    move no float by more than 1e-6 of its value (compare.noise_envelope). A case whose input sits
    on a decision boundary on purpose (Case.exact: |z| equal to the endcap boundary, a stored x equal
    to the node's or to another key's live x) is exempt, since perturbing that input is perturbing the decision under test;
  * in the running-covariance cases the last extrapolated edge's chi2 differs by more than 1e-3
    with and without the var_ms accumulated in the sender's merged_cov[1, 1].
"""
import os
import warnings

import numpy as np
import pytest

import cpu_ref
import gtf_oracle as O
import pass_cases as PC
from compare import compare, noise_envelope
from fixtures import GOLDEN
from gtf import graph

RTOL = 1e-6
NAMES = [c.name for c in PC.CASES]


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(GOLDEN, "pass_cases.npz"), allow_pickle=False)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (NaN inputs are cases here)
        yield


def _is_cluster(case):
    return case.stage in ("cluster_uts", "cluster_tse")


def expected(record, case):
    """the unpadded case with the reference's recorded outputs swapped in"""
    g, names, _ = PC.packed(case)
    assert np.array_equal(record[case.name + "__node_id"], g.node["node_id"])
    assert np.array_equal(record[case.name + "__slot_key"], g.slot["slot_key"])
    e = g.copy()
    pre = case.name + "__"
    for k in record.files:
        if k.startswith(pre + "node__"):
            e.node[k[len(pre) + 6:]] = record[k].copy()
        elif k.startswith(pre + "slot__"):
            e.slot[k[len(pre) + 6:]] = record[k].copy()
    return e


def raising_node(exc):
    """the node the oracle was at when it raised: local `v` of its innermost frame that has one"""
    tb, v = exc.__traceback__, None
    while tb is not None:
        if tb.tb_frame.f_code.co_filename == O.__file__ and "v" in tb.tb_frame.f_locals:
            v = tb.tb_frame.f_locals["v"]
        tb = tb.tb_next
    return int(v)


def unpadded(g, pads):
    return graph.subset(g, ~np.isin(g.node["node_id"], list(pads))) if pads else g


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference_record(record, name):
    case = PC.BY_NAME[name]
    p = PC.params_of(name)
    raised = str(record[name + "__raised"]) if name + "__raised" in record.files else None
    assert case.ref is not None or raised is not None or name + "__node__degree" in record.files, "case not recorded"
    assert (raised is not None) == (case.err is not None) or case.ref is not None
    for i, slots in enumerate(PC.variants(case)):
        g, names, pads = PC.packed(case, 1000 * i, slots)
        ix = lambda nm: int(np.nonzero(g.node["node_id"] == names[nm])[0][0])   # noqa: E731
        if case.err is not None:
            with pytest.raises(O.ReferenceError_) as ei:
                PC.run_oracle(g, case, p, "raise")
            assert raising_node(ei.value) == ix(case.err[1]), (name, slots)
            typ, where = raised.split()
            f, line = PC.line_of(str(ei.value))
            assert str(ei.value).startswith(typ + ":") and line == int(where.split(":")[1]), (str(ei.value), raised)
            assert f is None or f == where.split(":")[0]
            if not case.tie_stop:
                continue
        out, info = PC.run_oracle(g, case, p, "stop")
        if case.check:
            case.check(out, g, ix, info)
        if case.ref is None and raised is None:
            exp = expected(record, case)
            rtol = 0.0 if _is_cluster(case) else RTOL
            errs = compare(unpadded(out, pads), exp, rtol=rtol, atol=0.0 if rtol == 0.0 else 1e-12)
            assert errs == [], (name, slots, "\n".join(errs))


def test_every_size_is_reached():
    """the padded variants put a receiver of every lane-group width, and of the tail above 64 slots,
    behind every node-kernel case"""
    g, comps = PC.everything()
    deg = np.diff(g.slot_ptr)
    for c in comps:
        if c["case"].pad and c["slots"] is not None:
            assert deg[c["ix"]["v"]] == c["slots"], (c["case"].name, c["slots"])
    for case in PC.CASES:
        if case.pad:
            assert PC.variants(case)[-3:] == [32, 64, 65], case.name
    # receivers of 17..64 slots, and of more, that hold 3..15 keys: the clustering code of the 32- and
    # 64-lane groups and of the thread-per-node tail
    for key in ("uts", "tse"):
        dd = np.bincount(g.slot_dst()[g.slot[key + "_rank"] >= 0], minlength=g.n_nodes)
        for lo, hi in ((17, 32), (33, 64), (65, 1 << 30)):
            assert int(((deg >= lo) & (deg <= hi) & (dd >= 3) & (dd <= 15)).sum()) >= 10, (key, lo)


def _group_graph(g, cs):
    m = PC.node_mask(g, cs)
    return graph.subset(g, m), m


@pytest.mark.parametrize("stage", ["full_pass", "cluster_uts", "cluster_tse"])
def test_cpu_ref_flags_and_outputs(stage):
    g, comps = PC.everything()
    seen = 0
    for (st, _), cs in PC.groups(comps).items():
        if st != stage:
            continue
        case0 = cs[0]["case"]
        p = PC.params_of(case0.name)
        gg, _ = _group_graph(g, cs)
        want = 0
        for c in cs:
            want |= c["case"].err[0] if c["case"].err else 0
        got = gg.copy()
        flags = cpu_ref.full_pass(got, p, 2) if stage == "full_pass" else cpu_ref.cluster(
            got, stage[-3:], p.cluster_chi2, p.cluster_kl, p, 2)
        assert flags == want, (stage, case0.name, flags, want)
        clean = [c for c in cs if PC.is_clean(c["case"])]
        gc, m = _group_graph(g, clean)
        exp, _ = PC.run_oracle(gc, case0, p, "stop")
        keep = m[PC.node_mask(g, cs)]
        rtol = 0.0 if stage != "full_pass" else RTOL
        errs = compare(graph.subset(got, keep), exp, rtol=rtol, atol=0.0 if rtol == 0.0 else 1e-12)
        assert errs == [], (case0.name, "\n".join(errs))
        seen += 1
    assert seen >= 1


def test_clean_cases_are_well_conditioned():
    g, comps = PC.everything()
    eps = 2.0 ** -52
    for (st, _), cs in PC.groups(comps).items():
        cs = [c for c in cs if PC.is_clean(c["case"]) and not c["case"].exact and c["slots"] is None]
        if not cs:
            continue
        case0 = cs[0]["case"]
        p = PC.params_of(case0.name)
        gg, _ = _group_graph(g, cs)
        ref, noise, flips = noise_envelope(lambda x: PC.run_oracle(x, case0, p, "stop")[0], gg)
        for key, fl in flips.items():
            assert not fl.any(), (case0.name, key, np.nonzero(fl)[0][:5])
        for (kind, f), nz in noise.items():
            val = np.abs(getattr(ref, kind)[f])
            tol = RTOL * np.where(np.isfinite(val), val, np.inf)
            if f == "uts_sv":   # the receiver-frame offset c cancels to ~0: the rounding scale of the predicted state
                tol[:, 2] += 8 * eps * ref.slot["xp_scale"] if "xp_scale" in ref.slot else 0.0
            bad = np.nonzero(~(nz <= tol))
            assert bad[0].size == 0, (case0.name, kind, f, bad[0][:5], nz[bad][:5], val[bad][:5])


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if c.running])
def test_running_covariance_is_visible(name):
    """the chi2 of the last extrapolated out-edge, with the sender's merged_cov[1, 1] as the out-edges
    before it left it and with the value the sender started from"""
    case = PC.BY_NAME[name]
    p = PC.params_of(name)
    g, names, _ = PC.packed(case)
    out, info = PC.run_oracle(g, case, p)
    u = int(np.nonzero(g.node["node_id"] == names["u"])[0][0])
    ks = [int(k) for k in g.out_slot[g.out_ptr[u]:g.out_ptr[u + 1]] if not np.isnan(info["chi2"][k])]
    k = ks[-1]
    v = int(g.slot_dst()[k])
    args = (p.chi2_cut, p.sigma0xy, p.sigma0rz, p.sigma0rz2, p.endcap_boundary)
    cov = O.mat_from_cov5(g.node["merged_cov"][u])
    own = cov.copy()
    O.extrapolate_validate(g.node["gnn"][u], g.node["gnn"][v], g.node["merged_state"][u], own, *args)
    cov[1, 1] -= own[1, 1] - cov[1, 1]     # (the call adds the edge's own var_ms: none at all is left)
    without = float(np.ravel(O.extrapolate_validate(g.node["gnn"][u], g.node["gnn"][v], g.node["merged_state"][u],
                                                    cov, *args)[2])[0])
    with_ = float(info["chi2"][k])
    assert abs(with_ - without) > 1e-3 * abs(with_), (with_, without)
    assert out.node["merged_cov"][u][3] > g.node["merged_cov"][u][3]
