"""The directed fused-pass cases (pass_cases.py, pinned to the reference by test_pass_cases.py) on the
GPU, in every configuration of the node kernel.

All cases with their padded variants form one graph (one component each). A configuration uploads
it once; the components that share a stage and Params (a group) are then run together: the uploaded
state is restored, the group's stage runs over the whole graph with the group's Params, and only
the group's components are looked at. Per configuration and group:

  * every clean component equals the oracle's run of it (compare() at rtol 1e-6, atol 1e-12; rtol 0
    for the clustering-only stages), with no noise envelope: test_pass_cases.py shows the inputs
    need none;
  * gtf_diag.node_err is nonzero at exactly the declared raising nodes of the group, with exactly
    the declared bits, and errors() is the OR of node_err over the graph;
  * every extrapolated edge's chi2 (gtf_diag.edge_chi2) is within 1e-6 of the oracle's;
  * a raising component is compared on its error alone, except the tie that empties the state
    list: include/gtf.h promises the merged state formed so far, the oracle's tie_policy="stop";
  * every configuration is bit-equal to the first one on the group's components, array for array.
"""
import functools
import warnings

import numpy as np
import pytest

import pass_cases as PC
from compare import compare
from gtf import graph
from test_gpu_lane_groups import _bit_equal

pytestmark = pytest.mark.gpu

TILE = 256
CONFIGS = {
    "lane_groups_kernel_classes": dict(classes=False),
    "lane_groups_static_classes": dict(classes=True),
    "thread_per_node": dict(schedule=False, classes=False),
    "packed_segments": dict(pack=True),
    "tiled": dict(layout="tiled", tile=TILE),
    "padded": dict(layout="padded", tile=TILE),
    "device_tables": dict(tables="device"),
    "device_tables_tiled": dict(tables="device", layout="tiled", tile=TILE),
    "power_of_two_groups": dict(classes=False, no_g6_g12=True),
}
FIRST = next(iter(CONFIGS))


@functools.lru_cache(maxsize=1)
def world():
    """the graph, and per group: its stage and Params, the node masks of its components and of the
    clean ones, the oracle's output and chi2 on the clean ones, and the declared node_err"""
    g, comps = PC.everything()
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (NaN inputs are cases here)
        for cs in PC.groups(comps).values():
            case0 = cs[0]["case"]
            p = PC.params_of(case0.name)
            clean = PC.node_mask(g, [c for c in cs if PC.is_clean(c["case"])])
            exp, info = PC.run_oracle(graph.subset(g, clean), case0, p, "stop")
            err = np.zeros(g.n_nodes, np.uint32)
            for c in cs:
                if c["case"].err:
                    err[c["ix"][c["case"].err[1]]] = c["case"].err[0]
            out.append(dict(case=case0, params=p, nodes=PC.node_mask(g, cs), clean=clean, exp=exp, comps=cs,
                            chi2=info.get("chi2"), err=err, names=sorted(set(c["case"].name for c in cs))))
    return g, out


def run_stage(d, case, p):
    st = case.stage
    if st == "extrapolate":
        d.extrapolate(p)
    elif st == "update":
        d.update(p)
    elif st in ("cluster_uts", "cluster_tse"):
        d.cluster(st[-3:], p.cluster_chi2, p.cluster_kl, p)
    elif st == "full_pass":
        d.full_pass(p)
    else:
        d.node_ops(list(st), p)


@functools.lru_cache(maxsize=None)
def results(config):
    """per group: the downloaded graph cut to the group's components, the flags, node_err and edge_chi2"""
    from gtf.device import DeviceGraph
    g, groups = world()
    kw = dict(CONFIGS[config])
    no612 = kw.pop("no_g6_g12", False)
    d = DeviceGraph(g, **kw)
    if no612:   # every node on its power-of-two lane group
        d.cg.n_g6 = 0
        d.cg.n_g12 = 0
    snap = d.snapshot()
    d.set_diagnostics(node_err=True, edge_chi2=True)
    out = []
    for grp in groups:
        d.restore(snap)
        d.clear_errors()
        d.clear_diagnostics()
        run_stage(d, grp["case"], grp["params"])
        flags = d.errors()
        diag = d.diagnostics()
        got = d.download(g.copy())
        got.slot["edge_chi2"] = diag["edge_chi2"].copy()   # (rides along through subset())
        out.append(dict(flags=flags, node_err=diag["node_err"].copy(), got=graph.subset(got, grp["nodes"]),
                        clean=graph.subset(got, grp["clean"])))
    return out


def _variant(c):
    return c["case"].name + ("" if c["slots"] is None else "@%d" % c["slots"])


def blame(grp, got, exp, rtol, node_err):
    """the variants of a failing group whose own component differs (failure path only)"""
    orig = np.nonzero(grp["clean"])[0]
    bad = []
    for c in grp["comps"]:
        nodes = c["nodes"]
        if not np.array_equal(node_err[nodes], grp["err"][nodes]):
            bad.append(_variant(c) + ":err")
        if not PC.is_clean(c["case"]):
            continue
        m = (orig >= nodes[0]) & (orig <= nodes[-1])
        a, b = graph.subset(got, m), graph.subset(exp, m)
        ok = compare(a, b, rtol=rtol, atol=0.0 if rtol == 0.0 else 1e-12) == []
        if ok and "edge_chi2" in a.slot and grp["chi2"] is not None:
            e = graph.subset(_with(exp, "edge_chi2", grp["chi2"]), m).slot["edge_chi2"]
            with np.errstate(invalid="ignore"):
                ok = bool(np.all((np.abs(a.slot["edge_chi2"] - e) <= 1e-6 * np.abs(e)) | (np.isnan(e) & np.isnan(a.slot["edge_chi2"]))))
        if not ok:
            bad.append(_variant(c))
    return bad


def _with(g, name, arr):
    g = g.copy()
    g.slot[name] = np.asarray(arr).copy()
    return g


@pytest.mark.parametrize("config", list(CONFIGS))
def test_cases_match_the_oracle(config):
    g, groups = world()
    for grp, res in zip(groups, results(config)):
        what = (config, grp["case"].stage)
        mine = grp["nodes"]
        rtol = 0.0 if grp["case"].stage in ("cluster_uts", "cluster_tse") else 1e-6
        who = lambda: blame(grp, res["clean"], grp["exp"], rtol, res["node_err"])   # noqa: E731
        assert np.array_equal(res["node_err"][mine], grp["err"][mine]), (what, "FAILING", who())
        assert res["flags"] == int(np.bitwise_or.reduce(res["node_err"])), what
        errs = compare(res["clean"], grp["exp"], rtol=rtol, atol=0.0 if rtol == 0.0 else 1e-12)
        assert errs == [], (what, "FAILING", who(), "\n".join(errs))
        if grp["chi2"] is not None:
            a, b = res["clean"].slot["edge_chi2"], grp["chi2"]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "FAILING", who())
            m = ~np.isnan(b)
            assert m.any() and np.all(np.abs(a[m] - b[m]) <= 1e-6 * np.abs(b[m])), (what, "FAILING", who())


@pytest.mark.parametrize("config", [c for c in CONFIGS if c != FIRST])
def test_configurations_are_bit_equal(config):
    _, groups = world()
    for grp, a, b in zip(groups, results(config), results(FIRST)):
        what = (config, grp["case"].stage, grp["names"][:3])
        assert a["flags"] == b["flags"] and np.array_equal(a["node_err"], b["node_err"]), what
        _bit_equal(a["got"], b["got"], what)
