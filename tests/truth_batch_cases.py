"""Batches of events for the batched truth tables (gtf.metrics.truth_tables_batch on the host,
gtf_truth_build_ev / gtf.metrics.truth_tables_batch_dev on the device), made from tests/truth_cases.py.
A batch has one volume window, so the cases are grouped by theirs: the (7, 7) cases, the (7, 8) ones
(`reference` and the random events), and each `window_*` variant alone; every case is also a batch
of its own (`singleton_*`), so the batch entry point runs each single-event case.

A batch: "events" (truth_cases cases, or None for an event without truth), "window", and where the
device path must refuse it "raises": (the event the error names, "missing" | "range").
tests/test_truth_batch_cases.py checks them on the host, tests/test_gpu_truth_batch.py on the device."""
import numpy as np

import truth_cases as TC
from truth_cases import HI, LO, Rows, build


def part(case):
    """a case as a part of truth_tables_batch / truth_tables_batch_dev"""
    if case is None:
        return None
    return (case["m"],) + tuple(case["particles"]) + (tuple(case["truth"]) if case["truth"] is not None else ())


def parts(batch):
    return [part(c) for c in batch["events"]]


def _raising(name):
    e = TC.CASES[name]()["expect"]
    return bool(e.get("raises") or e.get("dev_raises"))


def _singleton_raises(name):
    """what a batch of this case alone raises: the host's ValueError is the missing truth row, the
    device-only refusal the packed key's range"""
    e = TC.CASES[name]()["expect"]
    return (0, "missing") if e.get("raises") else (0, "range") if e.get("dev_raises") else None


PLAIN = sorted(n for n in TC.CASES if not _raising(n))
GROUP_77 = [n for n in PLAIN if TC.CASES[n]()["window"] == (7, 7)]


def _batch(events, window=None, raises=None):
    windows = {c["window"] for c in events if c is not None}
    assert window is not None or len(windows) == 1, windows
    return {"events": list(events), "window": window if window is not None else windows.pop(), "raises": raises}


def _named(*names):
    return [None if n is None else TC.CASES[n]() for n in names]


def chain(n, pid0=1, n_pids=7, extra_truth=0, window=(7, 7)):
    """n rows, each a node and a hit of its own, over n_pids particles (high pT every second one) on
    layers 2, 4, ...; extra_truth >= 0: truth columns of their own, n + extra_truth rows (the extra ones
    second rows of the first hits, of another particle); None: the mapping's own"""
    r = Rows()
    for k in range(n):
        r.add(pid0 + k % n_pids, lay=2 * (k // n_pids % 9) + 2)
    truth = None
    if extra_truth is not None:
        hits = [x[1] for x in r.rows]
        truth = [(h, x[2]) for h, x in zip(hits, r.rows)] + [(hits[k % max(n, 1)], pid0 + 1) for k in range(extra_truth)]
    return build(r.rows, [(pid0 + k, HI if k % 2 == 0 else LO, 0) for k in range(n_pids)], truth=truth, window=window)


def one_row(k=0):
    """one row on node 10, hit 100: every such event collides with every other"""
    return build([(10, 100, 1 + k % 3, 7, 2, 1)], [(1, HI, 0), (2, LO, 0)])


# ---- colliding ids that must not leak across events
def _pt_differs():
    """particle 5 is high-pT in event 0 and low-pT in event 1: a region particle in event 0 only"""
    def ev(px):
        r = Rows()
        r.track(5, (2, 4, 6, 8))
        return build(r.rows, [(5, px, 0)], counts=(4, 4, int(px == HI), int(px == HI)),
                     **({"part": {5: (4, 1)}} if px == HI else {"absent": [5]}))
    return _batch([ev(HI), ev(LO), ev(HI)])


def _hit_in_neighbours_only():
    """hit 100 has a truth row in events 0 and 2 and none in event 1, which maps it: MISSING, event 1"""
    def ev(with_row):
        r = Rows()
        r.add(1, node=10, hit=100)
        r.add(1, lay=4, node=11, hit=101)
        return build(r.rows, [(1, HI, 0)], truth=[(101, 1)] + ([(100, 1)] if with_row else []))
    return _batch([ev(True), ev(False), ev(True)], raises=(1, "missing"))


def _node_with_other_hits():
    """node 10 holds hits 100, 101 in event 0 and hits 200, 100 in event 1, of other particles"""
    a, b = Rows(), Rows()
    a.add(1, node=10, hit=100), a.add(2, lay=4, node=10, hit=101)
    b.add(3, node=10, hit=200), b.add(4, lay=4, node=10, hit=100), b.add(3, lay=6, node=9, hit=101)
    return _batch([build(a.rows, [(1, HI, 0)], node_part={10: [1, 2]}, counts=(1, 2, 1, 0)),
                   build(b.rows, [(3, HI, 0)], node_part={10: [3, 4], 9: [3]}, counts=(2, 3, 1, 0))])


def _reference_here_repeat_there():
    """particle 6 is a reference track in event 0 and has a (volume, layer, module) twice in event 1"""
    a, b = Rows(), Rows()
    for lay, mod in ((2, 1), (4, 2), (6, 3), (8, 4)):
        a.add(6, lay=lay, mod=mod)
    for lay, mod in ((2, 1), (4, 2), (6, 3), (8, 4), (8, 4)):
        b.add(6, lay=lay, mod=mod)
    return _batch([build(a.rows, [(6, HI, 0)], part={6: (4, 1)}, counts=(4, 4, 1, 1)),
                   build(b.rows, [(6, HI, 0)], part={6: (5, 0)}, counts=(5, 5, 1, 0)),
                   build(a.rows, [(6, HI, 0)], part={6: (4, 1)}, counts=(4, 4, 1, 1))])


def _random(seed):
    """2-6 random events whose seeds come from a pool of three, so that whole events repeat (and every id
    collides); with and without truth columns of their own"""
    rng = np.random.default_rng(500 + seed)
    k = int(rng.integers(2, 7))
    pool = rng.integers(0, TC.N_RANDOM, 3)
    return _batch([TC.random_event(int(pool[rng.integers(0, 3)]), bool(rng.integers(0, 2))) for _ in range(k)])


def _make():
    b = {}
    for n in TC.CASES:       # every case of truth_cases.py as a batch of one event; a raising case names event 0
        b["singleton_" + n] = lambda n=n: _batch(_named(n), raises=_singleton_raises(n))
    for n in PLAIN:
        b["alone_" + n] = lambda n=n: _batch(_named(n))
        b["twice_" + n] = lambda n=n: _batch(_named(n, n))
        b["thrice_" + n] = lambda n=n: _batch(_named(n, n, n))
    b["empty_first"] = lambda: _batch(_named("no_rows", "dup_pairs", "shared_hit"))
    b["empty_middle"] = lambda: _batch(_named("dup_pairs", "no_rows", "no_rows", "shared_hit"))
    b["empty_last"] = lambda: _batch(_named("dup_pairs", "shared_hit", "no_rows"))
    b["only_empty"] = lambda: _batch(_named("no_rows", "no_rows", "no_rows"))
    b["no_events"] = lambda: _batch([], window=(7, 7))
    b["none_between"] = lambda: _batch(_named("dup_pairs", None, "own_shared_hit"))
    b["none_only"] = lambda: _batch([None, None], window=(7, 7))
    b["truth_beside_own"] = lambda: _batch(_named("truth_two_rows", "dup_pairs", "truth_selects", "own_shared_hit"))
    b["own_beside_truth"] = lambda: _batch(_named("ids", "truth_selects", "ids"))
    b["no_particles_beside"] = lambda: _batch(_named("no_particles", "shared_hit", "no_particles"))
    b["all_of_7_7"] = lambda: _batch(_named(*GROUP_77))
    b["pt_differs"] = _pt_differs
    b["hit_in_neighbours_only"] = _hit_in_neighbours_only
    b["truth_missing_last"] = lambda: _batch(_named("dup_pairs", "truth_missing"), raises=(1, "missing"))
    b["node_with_other_hits"] = _node_with_other_hits
    b["reference_here_repeat_there"] = _reference_here_repeat_there
    for f in ("module", "volume"):
        b["range_%s_in_event_2" % f] = lambda f=f: _batch(_named("dup_pairs", "shared_hit", "range_" + f, "own_shared_hit"),
                                                          raises=(2, "range"))
    for n in (100, 255, 256, 257):
        b["row_boundary_%d" % n] = lambda n=n: _batch([chain(n, extra_truth=None), chain(300, pid0=3, extra_truth=None)])
        # n truth rows in the first event (n - 40 rows and 40 second rows), the mapping's own in the second
        b["truth_boundary_%d" % n] = lambda n=n: _batch([chain(n - 40, extra_truth=40), chain(300, pid0=3, extra_truth=9),
                                                         chain(5, extra_truth=None)])
    b["runs_beside_one_row"] = lambda: _batch([one_row(0), TC.CASES["runs"](), one_row(1), one_row(2)])
    for k in (65, 257, 2049):
        b["one_row_x%d" % k] = lambda k=k: _batch([one_row(j) for j in range(k)])
    for s in range(5):
        b["random_%d" % s] = lambda s=s: _random(s)
    return b


BATCHES = _make()
RAISING = sorted(n for n in BATCHES if BATCHES[n]()["raises"])
NON_RAISING = sorted(n for n in BATCHES if not BATCHES[n]()["raises"])
