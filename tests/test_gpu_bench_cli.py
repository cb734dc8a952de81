"""bench.py's plain run and --dump-outputs.

* A plain run (no --full) prints one JSON line with the headline fields and none of the
  sections that moved behind --full; --steps sets the number of timed steps.
* --dump-outputs writes float32 / float64 .npy files of at most 64 MB in all, every number
  finite; with the NaN of absent entries put back from the <name>_nonfinite maps they equal,
  bit for bit, the host-order arrays of one pass on a freshly uploaded copy of the same seeded
  event (every timed step runs on the same input, so the last step's result is that pass's).
* When the per-slot arrays do not fit the budget, a fixed seeded sample of rows is written
  (checked in process with a small budget: the C2 event fits whole)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh_pass():
    """(event, its host-order state after one pass on a fresh upload), natural layout"""
    import torch
    from gtf import synth
    from gtf.device import DeviceGraph
    from gtf.params import Params
    g = synth.workload("c2", seed=0)
    d = DeviceGraph(g, "cuda:0", layout="natural")
    d.clear_errors()
    d.full_pass(Params())
    torch.cuda.synchronize()
    assert d.errors() == 0
    return g, d.download(g.copy())


def _check_against(outdir, gh):
    files = sorted(glob.glob(os.path.join(outdir, "*.npy")))
    assert files
    assert sum(os.path.getsize(f) for f in files) <= 64 * 1000 * 1000
    rows = np.load(os.path.join(outdir, "slot_sample_index.npy")).astype(np.int64)
    assert np.all(np.diff(rows) > 0)
    compared = 0
    loaded = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    for name, a in loaded.items():
        assert a.dtype in (np.float32, np.float64), name
        assert np.isfinite(a).all(), name
        if name.endswith("_nonfinite"):
            assert name[:-len("_nonfinite")] in loaded, name
            continue
        kind = loaded.get(name + "_nonfinite")
        if kind is not None:   # a float field: put back what the map says stood there
            assert kind.shape == a.shape and np.all(a[kind != 0] == 0), name
            a = a.copy()
            for code, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
                a[kind == code] = v
        if name.startswith("node_"):
            ref = gh.node[name[5:]]
        elif name.startswith("slot_") and name != "slot_sample_index":
            ref = gh.slot[name[5:]][rows]
        else:
            continue
        assert np.array_equal(a, ref.astype(a.dtype), equal_nan=True), name
        compared += 1
    assert compared >= 25   # every mutable per-node and per-slot array
    return rows


def test_plain_run_line_and_dump(tmp_path, fresh_pass):
    g, gh = fresh_pass
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "c2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(g.n_edges / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["device_error_flags"] == 0
    for moved in ("kernel_ms", "roofline", "cpu_baseline", "cpu_baseline_cpp", "dropin_stage", "c5_parabolic_kl",
                  "c3_fused_batch", "other_path_stages", "instrumented_ms_per_step", "ms_per_step_inline_restore"):
        assert moved not in line, moved
    rows = _check_against(str(out), gh)
    assert rows.size == g.n_slots   # C2 fits whole


def test_dump_samples_slots_when_over_budget(tmp_path, fresh_pass, monkeypatch):
    import bench
    from gtf.device import DeviceGraph
    from gtf.params import Params
    g, gh = fresh_pass
    d = DeviceGraph(g, "cuda:0", layout="tiled", tile=4096)
    snap = d.snapshot(DeviceGraph.PASS_INPUTS)
    d.stage_inputs(2)
    d.fill_inputs(snap)
    d.clear_errors()
    for i in range(2):
        d.use_inputs(i)
        d.full_pass(Params())
    d.use_inputs(None)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 * 1000 * 1000)
    monkeypatch.setattr(bench, "DUMP_SLOT_SAMPLE", 5000)
    info = [bench.dump_outputs(d, g, 1, str(tmp_path / n)) for n in ("a", "b")]
    assert info[0]["slots_sampled"] == 5000 < g.n_slots and info[0]["bytes"] <= 8 * 1000 * 1000
    rows = [_check_against(str(tmp_path / n), gh) for n in ("a", "b")]
    assert np.array_equal(rows[0], rows[1])   # the same sample every time
