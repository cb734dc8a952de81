"""A raising event of a batch is named and cut out, the others finish (gtf_event_errors,
DeviceGraph.track_node_errors / event_errors, pipeline.run_batch(on_error=), build_events_dev(on_error=),
run_pipeline.py --batch-on-error): the C-ABI against gtf.graph.event_errors on the hand-made cases between
guard bytes, and the loop against pipeline.run(d, None, resident="device") event by event -- the failing
event raises what run() on it alone raises, every other event gets run()'s records, bit for bit.

The failing events: the real 800' event (tests/golden/kat800, volumes 7-14), which raises GTF_ERR_TIE_EMPTIED
in iteration 1 (tests/test_gpu_real800.py pins that to the reference), and vol-7 copies with one column entry
changed before the loop starts (section d says which and why they raise where they do)."""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import batch_cases as bc
import event_error_cases as ec
import real800 as R
from gtf import _native as nat
from gtf import graph
from guard_mem import FILL, GUARD, Mem, at
from test_gpu_batch import _alone, _records_equal, _with_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ec.cases()
MSG = {f: re.escape(nat.ERR_FLAGS[f]) for f in (1, 8, 64)}
STAGE1, STAGE2 = "clustering(track_state_estimates)", "extrapolation"


# ---------------------------------------------------------------- (a) the C-ABI between guard bytes
def _buffer(M, nbytes):
    """a guarded device buffer whose payload holds 0xFF (the call must overwrite it)"""
    h = np.full(GUARD + nbytes + GUARD, FILL, np.uint8)
    h[GUARD:GUARD + nbytes] = 0xFF
    return M.up(h)


def _call(M, err, ev, K, mask, ids, outputs=("err_ev", "n_raising", "first_node", "first_id", "keep")):
    """gtf_event_errors on raw buffers: (rc, {name: device payload}, {name: host array})"""
    L = nat.lib()
    N = int(err.size)
    dev_in = [M.up(a) if a is not None and N else None for a in (err, ev, ids)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
    sizes = {"err_ev": (4 * K, np.uint32), "n_raising": (4 * K, np.int32), "first_node": (4 * K, np.int32),
             "first_id": (8 * K, np.int64), "keep": (N, np.uint8)}
    bufs = {k: _buffer(M, sizes[k][0]) for k in outputs}
    host = {k: np.full(sizes[k][0], 0xFF, np.uint8).view(sizes[k][1])      # (all bits set: -1, or 2^32 - 1)
            for k in ("err_ev", "n_raising", "first_node", "first_id")}
    nb = int(L.gtf_event_errors_workspace_bytes(K))
    ws = _buffer(M, nb)
    io = nat.GtfEventErrorsIo(node_err=vp(dev_in[0]), event=vp(dev_in[1]), node_id=vp(dev_in[2]), n_nodes=N, n_events=K,
                              mask=mask, **{k: at(t) for k, t in bufs.items()},
                              **{"host_" + k: ctypes.c_void_p(a.ctypes.data) for k, a in host.items()})
    rc = L.gtf_event_errors(ctypes.byref(io), at(ws), nb, M.stream)
    M.payload(ws, nb, np.uint8)     # (the workspace's guards)
    return rc, {k: M.payload(bufs[k], sizes[k][0], sizes[k][1]) for k in outputs}, host


@pytest.mark.parametrize("mem", ["torch", "hip"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_abi_equals_the_definition(name, mem):
    err, ev, K, mask, ids = CASES[name]
    exp = dict(zip(("err_ev", "n_raising", "first_node", "first_id", "keep"), graph.event_errors(err, ev, K, mask, ids)))
    rc, dev, host = _call(Mem(mem), err, ev, K, mask, ids)
    assert rc == 0, nat.lib().gtf_last_error()
    if err.size == 0 or K == 0:      # nothing launched, nothing written
        assert all(bool((v.view(np.uint8) == 0xFF).all()) for v in dev.values())
        assert all(bool((v.view(np.uint8) == 0xFF).all()) for v in host.values())
        return
    for k, x in exp.items():
        assert np.array_equal(dev[k], x), (name, k)
        if k != "keep":
            assert np.array_equal(host[k], x), (name, "host_" + k)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_abi_optional_arguments(mem):
    """without node_id no first_id is written; with only keep given the others are not needed"""
    err, ev, K, mask, ids = CASES["block_bounds"]
    exp = graph.event_errors(err, ev, K, mask)
    rc, dev, host = _call(Mem(mem), err, ev, K, mask, None)
    assert rc == 0 and np.array_equal(dev["err_ev"], exp[0]) and np.array_equal(dev["first_node"], exp[2])
    assert bool((dev["first_id"].view(np.uint8) == 0xFF).all()) and bool((host["first_id"] == -1).all())
    rc, dev, _ = _call(Mem(mem), err, ev, K, mask, ids, outputs=("keep",))
    assert rc == 0 and np.array_equal(dev["keep"], exp[4])


@pytest.mark.parametrize("mem", ["torch", "hip"])
@pytest.mark.parametrize("name", sorted(ec.bad_cases()))
def test_abi_refuses_a_bad_event_column(name, mem):
    err, ev, K, mask, ids, node = ec.bad_cases()[name]
    rc, _, _ = _call(Mem(mem), err, ev, K, mask, ids)       # (the guard bytes are checked whatever the status)
    assert rc == -2 and ("event[%d]" % node).encode() in nat.lib().gtf_last_error()


def test_abi_host_refusals():
    L = nat.lib()
    fake = ctypes.c_void_p(256)
    io = nat.GtfEventErrorsIo(n_nodes=0, n_events=4)
    assert L.gtf_event_errors(ctypes.byref(io), None, 0, None) == 0          # no node: nothing to do
    io = nat.GtfEventErrorsIo(n_nodes=5, n_events=0)
    assert L.gtf_event_errors(ctypes.byref(io), None, 0, None) == 0
    io = nat.GtfEventErrorsIo(n_nodes=-1, n_events=1)
    assert L.gtf_event_errors(ctypes.byref(io), fake, 4096, None) == -2
    io = nat.GtfEventErrorsIo(n_nodes=5, n_events=2, node_err=fake)
    assert L.gtf_event_errors(ctypes.byref(io), fake, 4096, None) == -2 and b"one event" in L.gtf_last_error()
    io = nat.GtfEventErrorsIo(n_nodes=5, n_events=1)
    assert L.gtf_event_errors(ctypes.byref(io), fake, 4096, None) == -2 and b"node_err" in L.gtf_last_error()
    io = nat.GtfEventErrorsIo(n_nodes=5, n_events=2, node_err=fake, event=fake)
    assert L.gtf_event_errors(ctypes.byref(io), fake, 8, None) == -2 and b"workspace" in L.gtf_last_error()
    io.abi_version = nat.ABI_VERSION - 1
    assert L.gtf_event_errors(ctypes.byref(io), fake, 4096, None) == -3
    assert b"gtf_event_errors_io ABI mismatch" in L.gtf_last_error()
    assert L.gtf_event_errors(None, fake, 4096, None) == -2


# ---------------------------------------------------------------- the events
@functools.lru_cache(maxsize=None)
def _kat800():
    """the real 800' event, resident: treat as read-only (run_batch does not modify a list's parts)"""
    from gtf import pipeline
    return pipeline.build_event_dev(R.PREFIX, *R.VOLS)


def _vol7():
    from gtf import pipeline
    return pipeline.build_event_dev(bc.PREFIX, 7, 7)


def _hand(name="perm257"):
    from gtf.device import DeviceGraph
    return _with_states(DeviceGraph.from_event(*bc.columns(("hand", name))))


def _empty():
    from gtf.device import DeviceGraph
    return DeviceGraph.from_event(*bc.columns(("empty",)))


def _run(d, iterations=3, first=1):
    from gtf import pipeline
    return pipeline.run(d, None, iterations=iterations, first=first, resident="device")


# ---------------------------------------------------------------- (b) the self-check
def test_kat800_raises_alone_and_vol7_does_not():
    from gtf import pipeline
    with pytest.raises(ValueError, match=MSG[8]):
        _run(pipeline.build_event_dev(R.PREFIX, *R.VOLS))      # (a build of its own: run() works on its input)
    assert [len(r.candidates) for r in _alone(("vol7",))] == [1055, 110, 2]


# ---------------------------------------------------------------- (c) the golden batch
GOLDEN_SPECS = [("vol7",), None, ("hand", "perm257"), ("empty",), ("vol7",)]      # (None: kat800)


def _golden_list():
    return [_vol7(), _kat800(), _hand(), _empty(), _vol7()]


def _raising_ids():
    """the node ids of the two subgraphs the reference raises in (c2_800_cluster_tse.npz)"""
    h = _kat800().host_graph()[0]
    raised = R.fixture("cluster_tse")["raised"].astype(bool)
    assert raised.size == h.n_subgraphs and raised.sum() == 2
    return set(h.node["node_id"][raised[h.node["sub_id"]]].tolist())


def _check_golden(out, scorers=None, batch_scorer=None):
    assert isinstance(out, list) and len(out) == 5 and set(out.errors) == {1} and out[1] == []
    err = out.errors[1]
    assert (err.iteration, err.stage, err.flags, err.messages) == (1, STAGE1, 8, [nat.ERR_FLAGS[8]])
    assert err.first_node_id in _raising_ids() and err.n_raising >= 2
    for e, s in enumerate(GOLDEN_SPECS):
        if s is not None:
            _records_equal(out[e], _alone(s), (e, s))
    res = batch_scorer.results() if batch_scorer is not None else [s and s.result() for s in scorers]
    for e in (0, 4):
        assert [len(r.candidates) for r in out[e]] == [1055, 110, 2]
        assert (res[e].n_reconstructed, res[e].n_reference, res[e].efficiency_str) == (133, 163, "81.595")


def test_golden_batch_raise_and_name():
    from gtf import pipeline
    ds = _golden_list()
    with pytest.raises(ValueError, match="^reference exception reproduced on device: " + MSG[8] + "$") as ei:
        pipeline.run_batch(ds)
    assert type(ei.value) is ValueError
    with pytest.raises(pipeline.BatchError, match="^reference exception reproduced on device: " + MSG[8]) as ei:
        pipeline.run_batch(ds, on_error="name")
    assert ei.value.events == {1: 8}
    named = re.findall(r"event (\d+): (.*?); node id (\d+)", str(ei.value))
    assert [(int(e), m) for e, m, _ in named] == [(1, nat.ERR_FLAGS[8])] and int(named[0][2]) in _raising_ids()


@pytest.mark.parametrize("scoring", ["per_event", "batch"])
def test_golden_batch_isolate(scoring):
    from gtf import metrics, pipeline
    from test_gpu_score import golden
    tables = [golden()[3] if s == ("vol7",) else None for s in GOLDEN_SPECS]
    ds = _golden_list()
    if scoring == "batch":
        one = metrics.BatchScorer(tables)
        _check_golden(pipeline.run_batch(ds, scorers=one, on_error="isolate"), batch_scorer=one)
    else:
        per = [metrics.DeviceScorer(t) if t is not None else None for t in tables]
        _check_golden(pipeline.run_batch(ds, scorers=per, on_error="isolate"), scorers=per)


def test_golden_batch_isolate_on_the_fused_graph(event_dirs):
    from gtf import metrics, pipeline
    from test_gpu_score import golden
    d = pipeline.build_events_dev(event_dirs, *R.VOLS, on_error="isolate")
    assert d.event_error_records == {} and d.event_nodes == [8748, 29590, 257, 0, 8748]     # (a clean build)
    one = metrics.BatchScorer([golden()[3] if s == ("vol7",) else None for s in GOLDEN_SPECS])
    _check_golden(pipeline.run_batch(d, scorers=one, on_error="isolate", lists=True), batch_scorer=one)
    d = pipeline.build_events_dev(event_dirs, *R.VOLS, on_error="name")     # (iteration 1 ran on the first one)
    with pytest.raises(pipeline.BatchError) as ei:
        pipeline.run_batch(d, on_error="name")
    assert ei.value.events == {1: 8}


@pytest.fixture(scope="module")
def event_dirs(tmp_path_factory):
    """the golden batch as --eventNetwork prefixes: the hand-made events written as CSVs"""
    out = []
    for i, spec in enumerate(GOLDEN_SPECS):
        if spec is None or spec == ("vol7",):
            out.append(R.PREFIX if spec is None else bc.PREFIX)
            continue
        d = str(tmp_path_factory.mktemp("ev%d" % i))
        ids, x, y, z, r, layer, a, b = bc.columns(spec)
        with open(os.path.join(d, "event_1_filtered_graph_nodes.csv"), "w") as f:
            f.write("node_idx,layer_id,x,y,z\n")
            for k in range(ids.size):
                f.write("%d,%d,%r,%r,%r\n" % (ids[k], layer[k], float(x[k]), float(y[k]), float(z[k])))
        with open(os.path.join(d, "event_1_filtered_graph_edges.csv"), "w") as f:
            f.write("%d %d\nnode2,node1,weight\n" % (ids.size, a.size))
            for k in range(a.size):
                f.write("%d,%d,1.0\n" % (b[k], a[k]))
        out.append(os.path.join(d, "event_1_filtered_graph_"))
    return out


# ---------------------------------------------------------------- (d) later iterations
# Two ways to make a resident vol-7 event raise after iteration 1, each by ONE changed column entry:
#
# "update" (from iteration 1 on): has_tse = 0 on a node that iteration 1 does not cluster, that no accepted
#   extrapolation of iteration 2 reaches (has_uts stays 0) and that the extraction of iteration 2 leaves in the
#   remaining graph. Nothing reads the flag of such a node before remove_state_metadata's pruning, which finds a
#   node without a state dict: GTF_ERR_NO_STATE_DICT in the update() after iteration 2. The records of
#   iterations 1 and 2 are the clean event's.
# "extrapolation" (a loop started with first=2): the event carries the full load of tests/real800.py (every
#   node's merged state = its first track-state estimate), so iteration 2's extrapolation has merged senders; the
#   send_mw of one edge that the clean extrapolation accepts is NaN: GTF_ERR_SEND_MW_MISSING at that edge.
def _set(d, column, index, value):
    d.t[column][index] = value


@functools.lru_cache(maxsize=None)
def _update_victim():
    """the id of a vol-7 node as the "update" case needs it, from the clean run's graph after iteration 2"""
    from gtf import pipeline
    its = pipeline.run(_vol7(), None, iterations=2, resident="device", keep_graphs=True)
    g = its[1].remaining_graph
    ok = (g.node["has_uts"] == 0) & (g.node["has_tse"] == 1) & (g.node["has_merged"] == 0)
    assert ok.any()
    return int(g.node["node_id"][np.flatnonzero(ok)[0]])


def _vol7_failing_update():
    d = _vol7()
    v = int(np.flatnonzero(d._np(d.t["node_id"]) == _update_victim())[0])
    _set(d, "has_tse", v, 0)
    return d


def _vol7_full_load(poison=False):
    import torch
    d = _vol7()
    f = R.full_load(d.host_graph()[0])
    for k in ("has_merged", "merged_state", "merged_cov", "merged_prior"):
        d.t[k].copy_(torch.from_numpy(np.ascontiguousarray(f.node[k]).reshape(-1)).to(d.t[k].device))
    if poison:
        _set(d, "send_mw", _accepted_slot(), float("nan"))
    return d


@functools.lru_cache(maxsize=None)
def _accepted_slot():
    """a slot whose edge the clean extrapolation of the full-load event accepts"""
    from gtf.params import Params
    d = _vol7_full_load()
    d.clear_errors()
    d.extrapolate(Params())
    d.raise_errors()
    acc = np.flatnonzero(d._np(d.t["uts_fresh"]) & 1)
    assert acc.size > 100
    return int(acc[acc.size // 2])


@functools.lru_cache(maxsize=None)
def _alone_full_load():
    """run() from iteration 2 on the clean full-load event and on the hand event: read-only"""
    return _run(_vol7_full_load(), 2, first=2), _run(_hand(), 2, first=2)


def test_extrapolation_failure_in_iteration_2():
    from gtf import pipeline
    with pytest.raises(ValueError, match=MSG[1]):
        _run(_vol7_full_load(poison=True), 2, first=2)
    clean, hand = _alone_full_load()
    assert len(clean) == 2 and clean[0].stage == STAGE2 and clean[0].counts["n_extracted"] > 0
    out = pipeline.run_batch([_vol7_full_load(), _vol7_full_load(poison=True), _hand()], iterations=2, first=2,
                             on_error="isolate")
    assert set(out.errors) == {1} and out[1] == []
    err = out.errors[1]
    assert (err.iteration, err.stage, err.flags, err.n_raising) == (2, STAGE2, 1, 1)
    _records_equal(out[0], clean, "full load")
    _records_equal(out[2], hand, "hand")


def test_update_failure_after_iteration_2():
    from gtf import pipeline
    with pytest.raises(ValueError, match=MSG[64]):
        _run(_vol7_failing_update())
    with pytest.raises(ValueError, match=MSG[64]):
        _run(_vol7_failing_update(), 2)                 # (it is the update after iteration 2 ...)
    assert len(_run(_vol7_failing_update(), 1)) == 1    # (... not iteration 1)
    out = pipeline.run_batch([_hand("chain65"), _vol7_failing_update(), _vol7()], on_error="isolate")
    assert set(out.errors) == {1}
    err = out.errors[1]
    assert (err.iteration, err.stage, err.flags, err.first_node_id, err.n_raising) == (2, "update", 64, _update_victim(), 1)
    _records_equal(out[1], _alone(("vol7",))[:2], "the records before the update")     # iteration 2's record stays
    _records_equal(out[0], _alone(("hand", "chain65")), "hand")
    _records_equal(out[2], _alone(("vol7",)), "vol7")


# ---------------------------------------------------------------- (e) other placements
def test_failing_event_first_and_last():
    from gtf import pipeline
    out = pipeline.run_batch([_kat800(), _hand(), _vol7()], on_error="isolate")
    assert set(out.errors) == {0} and out[0] == [] and out.errors[0].iteration == 1
    _records_equal(out[1], _alone(("hand", "perm257")), "hand")
    _records_equal(out[2], _alone(("vol7",)), "vol7")
    out = pipeline.run_batch([_vol7(), _empty(), _vol7_failing_update()], on_error="isolate", lists=False)
    assert set(out.errors) == {2} and out[1] == [] and out.errors[2].stage == "update"
    _records_equal(out[0], _alone(("vol7",)), "vol7", lists=False)
    _records_equal(out[2], _alone(("vol7",))[:2], "before the update", lists=False)


def test_two_events_fail_in_different_iterations():
    from gtf import pipeline
    out = pipeline.run_batch([_vol7_failing_update(), _vol7(), _kat800()], on_error="isolate")
    assert {e: (r.iteration, r.stage, r.flags) for e, r in out.errors.items()} == {2: (1, STAGE1, 8), 0: (2, "update", 64)}
    assert out[2] == []
    _records_equal(out[0], _alone(("vol7",))[:2], "before the update")
    _records_equal(out[1], _alone(("vol7",)), "vol7")
    with pytest.raises(pipeline.BatchError) as ei:
        pipeline.run_batch([_vol7_failing_update(), _vol7()], on_error="name")
    assert ei.value.events == {0: 64} and "event 0: " in str(ei.value) and "node id %d" % _update_victim() in str(ei.value)


def test_every_event_fails():
    from gtf import pipeline
    out = pipeline.run_batch([_kat800(), _kat800()], on_error="isolate")
    assert out == [[], []] and set(out.errors) == {0, 1}
    assert out.errors[0].first_node_id == out.errors[1].first_node_id and out.errors[0].flags == 8


def test_track_node_errors_without_torch_arrays():
    """mem="hip" (what the CLIs use): the registration and the reduction through gtf.devmem arrays"""
    from gtf import pipeline
    from gtf.device import DeviceGraph
    from gtf.params import Params
    parts = [pipeline.build_event_dev(p, 7, 7, mem="hip") for p in (bc.PREFIX, bc.PREFIX)]
    v = int(np.flatnonzero(parts[1]._np(parts[1].t["node_id"]) == _update_victim())[0])
    d = DeviceGraph.concat(parts)
    assert d.mem == "hip" and d.torch is None
    d.track_node_errors()
    d.clear_errors()
    d.cluster("tse", *pipeline.CLUSTER_FIRST, Params())
    assert d.errors() == 0
    r = d.event_errors()
    assert r["err_ev"].tolist() == [0, 0] and r["first_id"].tolist() == [-1, -1] and bool(r["keep"].numpy().all())
    from gtf.devmem import HipArray
    bits = np.zeros(d.n_nodes, np.int32)
    bits[parts[0].n_nodes + v] = 64
    d.node_err_t = HipArray.from_numpy(bits)           # (as a kernel would have left it)
    r = d.event_errors()
    assert r["err_ev"].tolist() == [0, 64] and r["first_node"].tolist() == [-1, parts[0].n_nodes + v]
    assert r["first_id"].tolist() == [-1, _update_victim()] and r["n_raising"].tolist() == [0, 1]
    c = d.subset(r["keep"], carry={"vivl": d.carried["vivl"], "event": d.carried["event"]})
    assert c.n_nodes == parts[0].n_nodes and not c._np(c.carried["event"]).any()
    assert d.event_errors(mask=8)["err_ev"].tolist() == [0, 0]


# ---------------------------------------------------------------- (f) the CLI
def test_cli_batch_on_error_isolate(tmp_path):
    """--batch vol-7 kat800 vol-7 --batch-on-error isolate: error.json under 1/, and 0/ and 2/ hold the files of
    --batch vol-7 vol-7. Compared as the other CLI tests compare: .npz array by array (the archive holds
    timestamps), text files byte for byte, timings.json (wall times) by its keys."""
    import pandas as pd
    from test_gpu_score import golden
    z = golden()[0]
    tdir = str(tmp_path / "truth")
    os.makedirs(tdir)
    cols = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")
    pd.DataFrame({c: z["map__" + c] for c in cols}).to_csv(
        os.path.join(tdir, "event000001000-full-mapping-minCurv-0.3-134.csv"), index=False)
    pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")}).to_csv(
        os.path.join(tdir, "event000001000-particles.csv"), index=False)
    cli = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
    v7, k800 = os.path.join(bc.GOLDEN, "kat134"), R.KAT800
    common = ["-a", "7", "-z", "14", "--truth", tdir, "--mapping", "full-mapping-minCurv-0.3-134.csv", "--batch-build",
              "--batch-metrics"]
    a, b = str(tmp_path / "three"), str(tmp_path / "two")
    run = subprocess.run([sys.executable, cli, "--batch", v7, k800, v7, "-o", a, "--batch-on-error", "isolate"] + common,
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert len(re.findall(r"^event 1 failed in iteration 1 .*node id \d+$", run.stdout, re.M)) == 1
    subprocess.check_call([sys.executable, cli, "--batch", v7, v7, "-o", b] + common)
    err = json.load(open(os.path.join(a, "1", "error.json")))
    assert (err["iteration"], err["stage"], err["flags"], err["messages"]) == (1, STAGE1, 8, [nat.ERR_FLAGS[8]])
    assert err["node_id"] in _raising_ids()
    assert not os.path.exists(os.path.join(a, "1", "metrics.json")) and not os.path.exists(os.path.join(a, "1", "iteration_1"))
    for got, exp in (("0", "0"), ("2", "1")):
        one, two = os.path.join(a, got), os.path.join(b, exp)
        files = sorted(os.path.relpath(os.path.join(r, f), two) for r, _, fs in os.walk(two) for f in fs)
        assert files == sorted(os.path.relpath(os.path.join(r, f), one) for r, _, fs in os.walk(one) for f in fs)
        assert "metrics.json" in files and sum(f.endswith(".npz") for f in files) >= 1 + 4 * 3
        for f in files:
            p, q = os.path.join(one, f), os.path.join(two, f)
            if f.endswith(".npz"):
                with np.load(p) as zp, np.load(q) as zq:
                    assert sorted(zp.files) == sorted(zq.files), f
                    for k in zp.files:
                        assert zp[k].dtype == zq[k].dtype and zp[k].shape == zq[k].shape and \
                            np.array_equal(zp[k], zq[k], equal_nan=zp[k].dtype.kind == "f"), (got, f, k)
            elif f == "timings.json":
                assert sorted(json.load(open(p))) == sorted(json.load(open(q)))
            else:
                assert open(p, "rb").read() == open(q, "rb").read(), (got, f)
    bad = subprocess.run([sys.executable, cli, "-n", v7, "-o", str(tmp_path / "x"), "--batch-on-error", "isolate"],
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "--batch" in bad.stderr
