"""tests/truth_batch_cases.py on the host: gtf.metrics.truth_tables_batch is concat_tables of the
per-event tables and BatchTables.event gives each event's tables back; a NumPy restatement of the rule
gtf_truth_build_ev follows -- sorts by (event, key), searches clamped to the event's segment, offsets
read from the prefix sums at row_off -- gives the same nine arrays (this pins the design, not the
library); the expectations tests/truth_cases.py attaches to a case hold per event inside a batch; the
ctypes mirror of gtf_truth_in_ev matches include/gtf.h; the workspace size and the refusals on the host
need no device. The device runs the same batches in tests/test_gpu_truth_batch.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import truth_batch_cases as BC
import truth_cases as TC
from gtf import _native as nat
from gtf import metrics
from test_truth_cases import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = (("node_id", np.int64), ("node_ptr", np.int32), ("node_part", np.int64), ("part_id", np.int64),
          ("part_hits", np.int32), ("part_ref", np.uint8), ("node_off", np.int32), ("entry_off", np.int32),
          ("part_off", np.int32))


def batches_equal(a, b):
    for name, dt in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == dt and np.array_equal(x, y), name
    assert np.array_equal(a.scored, b.scored) and list(a.n_reference) == list(b.n_reference)


def host_batch(batch):
    return metrics.truth_tables_batch(BC.parts(batch), *batch["window"])


def tables_equal(a, b):
    for name, dt in ARRAYS[:6]:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == dt and np.array_equal(x, y), name
    assert a.n_reference == b.n_reference


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", BC.NON_RAISING)
def test_batch_is_the_concatenation_of_its_events(name):
    batch = BC.BATCHES[name]()
    got = host_batch(batch)
    per_event = [None if c is None else TC.host_tables(dict(c, window=batch["window"])) for c in batch["events"]]
    batches_equal(got, metrics.concat_tables(per_event))
    K = len(batch["events"])
    assert got.scored.size == K and got.node_off.size == got.entry_off.size == got.part_off.size == K + 1
    assert got.node_ptr.size == got.node_id.size + 1 and got.node_ptr[-1] == got.node_part.size
    for e, (c, t) in enumerate(zip(batch["events"], per_event)):
        back = got.event(e)
        if c is None:
            assert back is None and not got.scored[e]
            continue
        tables_equal(back, t)
        if c["expect"].get("counts"):
            check(c, back)          # what the case is named for, inside the batch


def test_raising_batches_raise_on_the_host_where_the_host_can():
    for name in BC.RAISING:
        batch = BC.BATCHES[name]()
        e, kind = batch["raises"]
        assert 0 <= e < len(batch["events"]) and kind in ("missing", "range")
        if kind == "missing":
            with pytest.raises(ValueError, match="no truth row"):
                host_batch(batch)
            for k, c in enumerate(batch["events"]):     # ... and that event alone is the broken one
                if k != e:
                    TC.host_tables(c)
        else:
            host_batch(batch)                             # the host function has no packed key


def test_the_table_of_batches_is_complete():
    names = set(BC.BATCHES)
    for n in BC.PLAIN:
        assert {"alone_" + n, "twice_" + n, "thrice_" + n} <= names
    assert {"singleton_" + n for n in TC.CASES} <= names
    singles = [n for n in BC.RAISING if n.startswith("singleton_")]
    assert sorted(singles) == ["singleton_range_module", "singleton_range_volume", "singleton_truth_missing"]
    assert all(BC.BATCHES[n]()["raises"][0] == 0 for n in singles)
    assert len(BC.PLAIN) == 17 and len(BC.RAISING) == 4 + len(singles)
    for n in ("empty_first", "empty_middle", "empty_last", "only_empty", "none_between", "truth_beside_own",
              "no_particles_beside", "pt_differs", "hit_in_neighbours_only", "node_with_other_hits",
              "reference_here_repeat_there", "range_module_in_event_2", "range_volume_in_event_2", "runs_beside_one_row",
              "one_row_x65", "one_row_x257", "one_row_x2049") + tuple("random_%d" % s for s in range(5)) + \
            tuple("%s_boundary_%d" % (a, n) for a in ("row", "truth") for n in (100, 255, 256, 257)):
        assert n in names, n
    # the boundaries lie where they are named
    for n in (100, 255, 256, 257):
        ev = BC.BATCHES["row_boundary_%d" % n]()["events"]
        assert ev[0]["m"].node_idx.size == n
        ev = BC.BATCHES["truth_boundary_%d" % n]()["events"]
        assert ev[0]["truth"][0].size == n and ev[2]["truth"] is None
    b = BC.BATCHES["truth_beside_own"]()["events"]
    assert [c["truth"] is not None for c in b] == [True, False, True, False]
    b = BC.BATCHES["no_particles_beside"]()["events"]
    assert [c["particles"][0].size for c in b] == [0, 1, 0]
    for s in range(5):
        ev = BC.BATCHES["random_%d" % s]()["events"]
        assert 2 <= len(ev) <= 6
    assert any(len({c["m"].node_idx.size for c in BC.BATCHES["random_%d" % s]()["events"]}) <
               len(BC.BATCHES["random_%d" % s]()["events"]) for s in range(5))     # an event repeats


def test_collisions_are_collisions():
    """the ids the collision batches are about really occur in both events"""
    a, b, _ = BC.BATCHES["pt_differs"]()["events"]
    assert 5 in a["particles"][0] and 5 in b["particles"][0] and a["particles"][1][0] != b["particles"][1][0]
    got = host_batch(BC.BATCHES["pt_differs"]())
    assert list(np.diff(got.part_off)) == [1, 0, 1] and list(got.n_reference) == [1, 0, 1]
    a, b, c = BC.BATCHES["hit_in_neighbours_only"]()["events"]
    assert 100 in a["truth"][0] and 100 in c["truth"][0] and 100 not in b["truth"][0] and 100 in b["m"].hit_id
    a, b = BC.BATCHES["node_with_other_hits"]()["events"]
    assert 10 in a["m"].node_idx and 10 in b["m"].node_idx
    assert set(a["m"].hit_id[a["m"].node_idx == 10]) != set(b["m"].hit_id[b["m"].node_idx == 10])
    got = host_batch(BC.BATCHES["reference_here_repeat_there"]())
    assert list(got.part_id) == [6, 6, 6] and list(got.part_ref) == [1, 0, 1] and list(got.part_hits) == [4, 5, 4]


# ------------------------------------------------------------------ the rule of the device build, in NumPy
def _cum0(x):
    return np.concatenate([[0], np.cumsum(np.asarray(x, np.int64), dtype=np.int64)]).astype(np.int64)


def _breaks(key, ev):
    """True where a run of equal (event, key) starts"""
    b = np.ones(key.size, bool)
    b[1:] = (key[1:] != key[:-1]) | (ev[1:] != ev[:-1])
    return b


def _segment_bounds(sorted_keys, off, ev, keys):
    """per key: lower and upper bound inside its event's segment of sorted_keys, as global indices"""
    lb, ub = np.zeros(keys.size, np.int64), np.zeros(keys.size, np.int64)
    for e in np.unique(ev):
        seg, at = sorted_keys[off[e]:off[e + 1]], ev == e
        lb[at] = off[e] + np.searchsorted(seg, keys[at], "left")
        ub[at] = off[e] + np.searchsorted(seg, keys[at], "right")
    return lb, ub


def batch_rule(batch):
    """gtf_truth.hip's steps on global indices -> the nine arrays, n_reference per event"""
    lo, hi = batch["window"]
    live = [c for c in batch["events"]]
    K = len(live)
    i64 = lambda xs: np.concatenate([np.asarray(x, np.int64) for x in xs]) if xs else np.zeros(0, np.int64)  # noqa: E731
    cols = {c: i64([getattr(ev["m"], c) for ev in live if ev is not None]) for c in metrics.MAPPING_COLUMNS}
    n_rows = [0 if ev is None else ev["m"].node_idx.size for ev in live]
    own = [ev is not None and ev["truth"] is not None for ev in live]
    th = i64([(ev["truth"][0] if t else ev["m"].hit_id) for ev, t in zip(live, own) if ev is not None])
    tp = i64([(ev["truth"][1] if t else ev["m"].particle_id) for ev, t in zip(live, own) if ev is not None])
    n_truth = [0 if ev is None else (ev["truth"][0].size if t else ev["m"].hit_id.size) for ev, t in zip(live, own)]
    pid = i64([ev["particles"][0] for ev in live if ev is not None])
    px = np.concatenate([ev["particles"][1] for ev in live if ev is not None] or [np.zeros(0)])
    py = np.concatenate([ev["particles"][2] for ev in live if ev is not None] or [np.zeros(0)])
    n_part = [0 if ev is None else ev["particles"][0].size for ev in live]
    row_off, eoff, poff = _cum0(n_rows), _cum0(n_truth), _cum0(n_part)
    evr, evt, evp = (np.repeat(np.arange(K), np.asarray(n, np.int64)) for n in (n_rows, n_truth, n_part))
    N = int(row_off[-1])
    # 1. the particles by (event, id)
    o = np.lexsort((pid, evp))
    pk, ps = pid[o], _cum0((np.sqrt(px ** 2 + py ** 2) >= metrics.PT_CUT)[o])
    # 2. the truth rows: their flag, then by (event, hit)
    lb, ub = _segment_bounds(pk, poff, evt, tp)
    tflag = (ub > lb) & (ps[ub] - ps[lb] > 0)
    tidx = np.lexsort((th, evt))
    tk, ts = th[tidx], _cum0(tflag[tidx])
    # 3. the rows
    node, hit, vol, lay, mod = (cols[c] for c in ("node_idx", "hit_id", "volume_id", "layer_id", "module_id"))
    lb, ub = _segment_bounds(tk, eoff, evr, hit)
    if np.any(ub == lb):
        raise ValueError("event %d: a mapped hit has no truth row" % evr[ub == lb].min())
    row_part = tp[tidx[np.minimum(lb, max(tk.size - 1, 0))]] if N else np.zeros(0, np.int64)
    sel = (ts[ub] - ts[lb] > 0) & (vol >= lo) & (vol <= hi)
    # 4. the region: (event, particle, not selected, volume, layer, module); position i belongs to evr[i]
    order = np.lexsort((mod, lay, vol, ~sel, cols["particle_id"], evr))
    kb, s = cols["particle_id"][order], sel[order]
    head = s & _breaks(kb, evr)
    q = np.concatenate([[0], order[:-1]]) if N else order
    vl = head | (s & ~head & ((vol[q] != vol[order]) | (lay[q] != lay[order])))
    dup = s & ~head & ~vl & (mod[q] == mod[order])
    sum_head, sum_dup, sum_s, sum_vl = _cum0(head), _cum0(dup), _cum0(s), _cum0(vl)
    pos = np.flatnonzero(head)
    end = np.append(pos[1:], N)
    part_id = kb[pos]
    part_hits = sum_s[end] - sum_s[pos]
    part_ref = ((sum_vl[end] - sum_vl[pos] >= metrics.NUM_DISTINCT_LAYERS) & (sum_dup[end] - sum_dup[pos] == 0))
    part_off = sum_head[row_off]
    refsum = _cum0(part_ref)
    n_ref = refsum[part_off[1:]] - refsum[part_off[:-1]]
    # 5. the CSR: (event, node, row), then its positions by (event, hit)
    vb = np.lexsort((node, evr))
    kbn = node[vb]
    vc = np.lexsort((hit[vb], evr))
    kc = hit[vb][vc]
    first = _breaks(kc, evr)
    first[1:] |= kbn[vc[1:]] != kbn[vc[:-1]]
    kept = np.zeros(N, bool)
    kept[vc] = first
    headn = _breaks(kbn, evr)
    sum_kept, sum_headn = _cum0(kept), _cum0(headn)
    node_ptr = np.append(sum_kept[:-1][headn], sum_kept[-1])
    return metrics.BatchTables(kbn[headn], node_ptr.astype(np.int32), row_part[vb[kept]], part_id, part_hits.astype(np.int32),
                               part_ref.astype(np.uint8), sum_headn[row_off].astype(np.int32),
                               sum_kept[row_off].astype(np.int32), part_off.astype(np.int32),
                               np.array([ev is not None for ev in live], np.uint8),
                               [None if ev is None else int(n) for ev, n in zip(live, n_ref)])


@pytest.mark.parametrize("name", BC.NON_RAISING)
def test_the_rule_of_the_device_build_gives_the_same_arrays(name):
    batch = BC.BATCHES[name]()
    batches_equal(batch_rule(batch), host_batch(batch))


def test_the_rule_names_the_event_of_a_missing_truth_row():
    for name in BC.RAISING:
        batch = BC.BATCHES[name]()
        e, kind = batch["raises"]
        if kind == "missing":
            with pytest.raises(ValueError, match="event %d: a mapped hit has no truth row" % e):
                batch_rule(batch)


# ------------------------------------------------------------------ the C-ABI without a device
def test_truth_in_ev_layout_matches_header():
    """offsetof() / sizeof() of every field of gtf_truth_in_ev, from a C probe compiled against the
    header, equal the ctypes mirror's"""
    t, cls = "gtf_truth_in_ev", nat.GtfTruthInEv
    lines = ['  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, t, f) for f, _ in cls._fields_]
    lines.append('  printf("sizeof %%zu\\n", sizeof(%s));' % t)
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(c, "w") as f:
            f.write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).split("\n") if line)
    assert len(got) == len(cls._fields_) + 1
    for k, v in got.items():
        assert (ctypes.sizeof(cls) if k == "sizeof" else getattr(cls, k).offset) == int(v), k
    assert {"gtf_truth_build_ev", "gtf_truth_build_ev_workspace_bytes"} <= set(nat.SYMBOLS)


def _lib():
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    return nat.lib()


def test_workspace_bytes_positive_and_monotonic():
    L = _lib()
    f = L.gtf_truth_build_ev_workspace_bytes
    assert f(0, 0, 0, 0) > 0 and f(-5, -5, -5, -5) == f(0, 0, 0, 0)
    steps = [(0, 0, 0, 0), (0, 0, 0, 1), (10, 0, 0, 1), (10, 10, 0, 1), (10, 11, 0, 1), (10, 11, 7, 1), (10, 11, 7, 64),
             (1000, 11, 7, 64), (1000, 2000, 7, 64), (1000, 2000, 3000, 64), (1000, 2000, 3000, 5000)]
    sizes = [f(*a) for a in steps]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    for base in ((100, 50, 20, 8), (2049, 0, 2049, 2049)):
        for k in range(4):
            more = list(base)
            more[k] += 1000
            assert f(*more) >= f(*base), (base, k)


def test_truth_build_ev_refuses_bad_arguments_without_a_gpu():
    """another ABI (-3); null arrays, offsets that do not start at 0 or decrease, a sum above 2^30, an
    inverted window and a small workspace (-2): all decided on the host before any device work"""
    L = _lib()
    fake = ctypes.c_void_p(4096)        # (never dereferenced: every call below is refused first)
    cols = {k: fake for k in metrics.MAPPING_COLUMNS + ("truth_hit", "truth_part", "part_id", "px", "py")}
    buf = nat.GtfTruthBatchBuf(*([fake] * 9))
    cnt = (nat.GtfTruthCounts * 4)()
    off = lambda *v: np.array(v, np.int32)  # noqa: E731
    arrays = {"row_off": off(0, 4, 4, 9), "truth_off": off(0, 0, 0, 3), "particle_off": off(0, 2, 2, 2)}

    def call(change=None, b=buf, ws=fake, nb=1 << 40, out=None, **offs):
        a = dict(arrays, **offs)
        keep = {k: np.ascontiguousarray(v) for k, v in a.items() if v is not None}
        fields = dict(n_events=3, num_layers=4, min_volume=7, max_volume=7, pt_cut=1.0, **cols)
        fields.update({k: (keep[k].ctypes.data if v is not None else None) for k, v in a.items()})
        fields.update(change or {})
        tin = nat.GtfTruthInEv(**fields)
        if change and "abi_version" in change:
            tin.abi_version = change["abi_version"]
        out = nat.GtfTruthBatch() if out is None else out
        return L.gtf_truth_build_ev(ctypes.byref(tin), ctypes.byref(b) if b is not None else None, ctypes.byref(out), cnt,
                                    ws, ctypes.c_size_t(nb), None)

    assert call({"abi_version": nat.ABI_VERSION + 1}) == -3 and b"ABI mismatch" in L.gtf_last_error()
    other = nat.GtfTruthBatch()
    other.struct_size -= 8
    assert call(out=other) == -3 and b"gtf_truth_batch" in L.gtf_last_error()
    for change, text in (({"min_volume": 8}, b"min_volume > max_volume"), ({"hit_id": None}, b"mapping column"),
                         ({"module_id": None}, b"mapping column"), ({"truth_part": None}, b"truth_hit"),
                         ({"px": None}, b"part_id / px / py"), ({"n_events": -1}, b"negative")):
        assert call(change) == -2, change
        assert text in L.gtf_last_error(), (change, L.gtf_last_error())
    for offs, text in (({"row_off": off(1, 4, 4, 9)}, b"row_off does not start at 0"),
                       ({"truth_off": off(0, 2, 1, 3)}, b"truth_off is negative or decreases"),
                       ({"particle_off": off(0, -1, 2, 2)}, b"particle_off is negative or decreases"),
                       ({"row_off": None}, b"row_off"), ({"particle_off": None}, b"particle_off"),
                       ({"row_off": off(0, 1 << 29, 1 << 30, (1 << 30) + 1)}, b"2^30"),
                       ({"truth_off": off(0, 0, 0, (1 << 30) + 1)}, b"2^30")):
        assert call(**offs) == -2, offs
        assert text in L.gtf_last_error(), (offs, L.gtf_last_error())
    for k in range(9):
        ptrs = [fake] * 9
        ptrs[k] = None
        assert call(b=nat.GtfTruthBatchBuf(*ptrs)) == -2 and b"missing array" in L.gtf_last_error(), k
    assert call(b=None) == -2
    need = L.gtf_truth_build_ev_workspace_bytes(9, 3, 2, 3)
    assert call(nb=need - 1) == -2 and b"workspace" in L.gtf_last_error()
    assert call(ws=None) == -2 and b"workspace" in L.gtf_last_error()
    assert all(c.error == 0 for c in cnt)
    assert L.gtf_truth_build_ev(None, ctypes.byref(buf), ctypes.byref(nat.GtfTruthBatch()), cnt, fake, ctypes.c_size_t(1),
                                None) == -2
