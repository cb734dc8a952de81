"""Hand-made hit mappings for the scorer's truth tables (gtf.metrics.truth_tables on the host,
gtf_truth_build / gtf.metrics.truth_tables_dev on the device), one per branch of
reconstruction_efficiency.py:41-91 and helper.py:466-479. tests/test_truth_cases.py checks that
every case reaches the branch it is named for, on gtf.metrics and (where pandas can express it) on
oracle/metrics_oracle.py; tests/test_gpu_truth.py runs them on the device.

A case: "m" (HitMapping), "particles" (id, px, py), "truth" (None, or the separate (hit_id,
particle_id) columns), "window" (min_volume, max_volume) and "expect": what the case is about
(checked by test_truth_cases.check):
  "node_part": {node: its particle list}, "part": {particle: (region hits, reference flag)},
  "absent": particles that are no region particle, "counts": (T, P, R, reference tracks),
  "raises": both paths raise ValueError, "dev_raises": only the device path does."""
import numpy as np

from gtf import metrics

B59 = 1 << 59
HI, LO = 2.0, 0.5          # px of a high-pT and of a low-pT particle (py = 0)


def build(rows, particles, truth=None, window=(7, 7), **expect):
    """rows: (node, hit, particle, volume, layer, module); particles: (id, px, py)"""
    a = np.array(rows, np.int64).reshape(-1, 6).T
    p = np.array([x[0] for x in particles], np.int64)
    px = np.array([x[1] for x in particles], np.float64)
    py = np.array([x[2] for x in particles], np.float64)
    if truth is not None:
        truth = (np.array([t[0] for t in truth], np.int64), np.array([t[1] for t in truth], np.int64))
    return {"m": metrics.HitMapping(*a), "particles": (p, px, py), "truth": truth, "window": window, "expect": expect}


class Rows:
    """rows under construction: fresh node and hit ids count up, a fresh module per hit unless given"""

    def __init__(self, node0=10, hit0=100):
        self.rows, self._node, self._hit = [], node0, hit0

    def add(self, pid, vol=7, lay=2, mod=None, node=None, hit=None):
        if node is None:
            node, self._node = self._node, self._node + 1
        if hit is None:
            hit, self._hit = self._hit, self._hit + 1
        self.rows.append((node, hit, pid, vol, lay, len(self.rows) + 1 if mod is None else mod))
        return node, hit

    def track(self, pid, layers, vol=7, node=None):
        """one hit per layer, each on a fresh node (or all on `node`)"""
        return [self.add(pid, vol, lay, node=node) for lay in layers]


def host_tables(case):
    th, tp = case["truth"] if case["truth"] is not None else (None, None)
    return metrics.truth_tables(case["m"], *case["particles"], *case["window"], th, tp)


# ---- 1-3: hit_dissociation
def _dup_pairs():
    """a repeat next to its original and one far from it: the first is kept, the order is the rows'"""
    r = Rows(node0=11, hit0=200)
    r.add(5, lay=2, node=10, hit=100)
    r.add(5, lay=2, node=10, hit=100)          # next to its original
    r.add(6, lay=4, node=10, hit=101)
    r.track(7, (2, 4, 6, 8))
    r.add(5, lay=2, node=10, hit=100)          # far from it
    r.add(8, lay=6, node=10, hit=102)
    r.add(6, lay=4, node=10, hit=101)
    return build(r.rows, [(5, HI, 0), (6, HI, 0), (7, HI, 0), (8, LO, 0)], node_part={10: [5, 6, 8]},
                 part={5: (3, 0), 6: (2, 0), 7: (4, 1)}, counts=(5, 7, 3, 1))


def _interleaved_descending():
    """node 20's rows lie between other nodes' rows and its hit ids descend: row order, not hit order"""
    r = Rows()
    for k, (hit, pid) in enumerate(((900, 1), (800, 2), (700, 3), (600, 4))):
        r.add(50 + k, node=21 + 2 * k, hit=300 + k)
        r.add(pid, lay=2 * k + 2, node=20, hit=hit)
        r.add(60 + k, node=19 - 2 * k, hit=310 + k)
    return build(r.rows, [(p, HI, 0) for p in (1, 2, 3, 4)], node_part={20: [1, 2, 3, 4]}, counts=(9, 12, 4, 0))


def _shared_hit():
    """one hit on two nodes: both hold its particle"""
    r = Rows()
    r.add(1, node=30, hit=500)
    r.add(2, node=30, hit=501)
    r.add(1, node=31, hit=500)
    r.add(3, node=31, hit=502)
    return build(r.rows, [(1, HI, 0)], node_part={30: [1, 2], 31: [1, 3]}, part={1: (2, 0)}, absent=[2, 3],
                 counts=(2, 4, 1, 0))


# ---- 4: separate truth columns
def _truth_two_rows():
    """hit 100 has two truth rows, of the low-pT 8 and then of the high-pT 9: the first one is the
    node's particle, either one selects the hit; the mapping's own particle 4 is the region particle"""
    r = Rows()
    r.add(4, node=10, hit=100)
    r.add(4, lay=4, node=11, hit=101)
    return build(r.rows, [(8, LO, 0), (9, HI, 0), (4, LO, 0)], truth=[(101, 8), (100, 8), (100, 9)],
                 node_part={10: [8], 11: [8]}, part={4: (1, 0)}, counts=(2, 2, 1, 0))


def _truth_selects():
    """rows selected only through the truth particle: the mapping's own particle 4 is low-pT and is
    a reference track all the same; its own high-pT id on an unselected hit changes nothing"""
    r = Rows()
    hits = [h for _, h in r.track(4, (2, 4, 6, 8))]
    _, other = r.add(9, lay=10)                 # the mapping says 9 (high pT), the truth says 8 (low pT)
    return build(r.rows, [(4, LO, 0), (9, HI, 0), (8, LO, 0)], truth=[(h, 9) for h in hits] + [(other, 8)],
                 node_part={10: [9], 14: [8]}, part={4: (4, 1)}, absent=[9, 8], counts=(5, 5, 1, 1))


def _truth_missing():
    r = Rows()
    r.track(1, (2, 4, 6, 8))
    hits = [x[1] for x in r.rows]
    return build(r.rows, [(1, HI, 0)], truth=[(h, 1) for h in hits[:-1]], raises=True)


# ---- 5: the mapping's own columns, one hit on rows of different particles
def _own_shared_hit():
    """hit 600 on a row of the low-pT 3 and on a row of the high-pT 1: both rows are selected"""
    r = Rows()
    r.add(3, node=10, hit=600)
    r.add(1, lay=4, node=11, hit=600)
    r.add(3, lay=6, node=12, hit=601)           # 3's own hit: not selected
    return build(r.rows, [(1, HI, 0), (3, LO, 0)], node_part={10: [3], 11: [3], 12: [3]}, part={3: (1, 0), 1: (1, 0)},
                 counts=(3, 3, 2, 0))


# ---- 6: the volume window
def _window(lo, hi):
    r = Rows()
    for vol in (5, 6, 7, 8, 9, 10, 11):
        r.track(100 + vol, (2, 4, 6, 8), vol=vol)
    inside = [v for v in (5, 6, 7, 8, 9, 10, 11) if lo <= v <= hi]
    return build(r.rows, [(100 + v, HI, 0) for v in (5, 6, 7, 8, 9, 10, 11)], window=(lo, hi),
                 part={100 + v: (4, 1) for v in inside}, absent=[100 + lo - 1, 100 + hi + 1],
                 counts=(28, 28, len(inside), len(inside)))


# ---- 7: pT at the cut
def at_the_cut():
    """-> ((px, py) with sqrt(px**2 + py**2) == 1.0, the pair one step of px below it for which
    NumPy's test is False). nextafter(0.6, 0) with 0.8 still rounds to 1.0, so the search walks."""
    def pt(x, y):
        return float(np.sqrt(np.array([x], np.float64) ** 2 + np.array([y], np.float64) ** 2)[0])   # (as high_pt_particles)
    px, py = np.float64(0.6), np.float64(0.8)
    while pt(px, py) < 1.0:
        px = np.nextafter(px, 1.0)
    while pt(np.nextafter(px, 0.0), py) >= 1.0:
        px = np.nextafter(px, 0.0)
    below = np.nextafter(px, 0.0)
    assert pt(px, py) == 1.0 and pt(px, py) >= metrics.PT_CUT and not pt(below, py) >= metrics.PT_CUT
    return (float(px), float(py)), (float(below), float(py))


def _pt_cut(zero_present):
    """a particle exactly at the cut, its neighbour below it, a particle missing from the table,
    id 0 (absent: noise; present with high pT: a particle), a high-pT particle without hits"""
    on, under = at_the_cut()
    r = Rows()
    for pid in (1, 2, 3, 0):
        r.track(pid, (2, 4, 6, 8))
    parts = [(1,) + on, (2,) + under, (77, HI, 0)] + ([(0, 0.0, 1.5)] if zero_present else [])
    part = {1: (4, 1)}
    if zero_present:
        part[0] = (4, 1)
    return build(r.rows, parts, part=part, absent=[2, 3, 77] + ([] if zero_present else [0]),
                 counts=(16, 16, len(part), len(part)))


# ---- 8: the reference-track tests
def _reference():
    r = Rows()
    r.track(1, (2, 4, 6, 8))                                   # exactly num_layers
    r.track(2, (2, 4, 6))                                      # one fewer
    r.track(3, (2, 4, 6, 6, 6))                                # five hits on three layers
    r.track(4, (2, 4), vol=7), r.track(4, (4, 6), vol=8)       # layer 4 in two volumes counts twice (and they are
                                                               # neighbours in (volume, layer) order)
    for lay, mod in ((2, 1), (4, 2), (6, 3), (8, 4), (8, 4)):  # a (volume, layer, module) twice
        r.add(5, lay=lay, mod=mod)
    for lay, mod in ((2, 1), (4, 2), (6, 3), (8, 4), (8, 4), (10, 5), (8, 4)):   # three times
        r.add(6, lay=lay, mod=mod)
    for lay in (2, 4, 6, 8):                                   # the same module on different layers
        r.add(7, lay=lay, mod=9)
    r.add(8, vol=7, lay=2, mod=3), r.add(8, vol=8, lay=2, mod=3)   # ... and in different volumes
    r.track(8, (4, 6))
    return build(r.rows, [(p, HI, 0) for p in range(1, 9)], window=(7, 8),
                 part={1: (4, 1), 2: (3, 0), 3: (5, 0), 4: (4, 1), 5: (5, 0), 6: (7, 0), 7: (4, 1), 8: (4, 1)},
                 counts=(36, 36, 8, 4))


# ---- 9: ids
def _ids():
    """negative, zero and 2^59-scale particle ids (the signed order), node and hit ids above 2^32,
    a negative node id"""
    r = Rows(node0=(1 << 32) + 5, hit0=(1 << 40) + 1)
    pids = (B59 + 7, -5, 0, 3, -B59 - 1, B59 + (1 << 32) + 7)
    for pid in pids:
        r.track(pid, (2, 4, 6, 8))
    r.add(3, lay=10, node=-4, hit=(1 << 33))
    r.add(-5, lay=10, node=-4, hit=-9)
    order = sorted(pids)
    return build(r.rows, [(p, HI, 0) for p in pids], part={p: (5 if p in (3, -5) else 4, 1) for p in pids},
                 node_part={-4: [3, -5], (1 << 32) + 5: [B59 + 7]}, order=order, counts=(25, 26, 6, 6))


# ---- 10: run lengths across wave and block boundaries
RUNS = (1, 63, 64, 65, 257, 1025)


def _runs():
    """particles of 1 .. 1,025 region hits, a node of 300 hits, and every run (the last particle's,
    the last node's) ending exactly at the last row"""
    r = Rows()
    for k, n in enumerate(RUNS):
        r.track(10 + k, range(1, n + 1))         # n distinct layers: the largest id has the longest run
    for j in range(300):
        r.add(2, lay=j + 1, node=5)
    big = r._node + 50                           # the largest node id, on the last rows
    for j in range(70):
        r.add(10 + len(RUNS) - 1, lay=2000 + j, node=big)
    part = {10 + k: (n, int(n >= 4)) for k, n in enumerate(RUNS)}
    part[10 + len(RUNS) - 1] = (1025 + 70, 1)
    part[2] = (300, 1)
    n_nodes = sum(RUNS) + 2
    return build(r.rows, [(p, HI, 0) for p in part], part=part, node_len={5: 300, big: 70},
                 counts=(n_nodes, sum(RUNS) + 370, len(part), len(part) - 1))


# ---- 11: empty shapes
def _nothing_in_window():
    r = Rows()
    r.track(1, (2, 4, 6, 8), vol=8)
    return build(r.rows, [(1, HI, 0)], counts=(4, 4, 0, 0))


def _no_high_pt():
    r = Rows()
    r.track(1, (2, 4, 6, 8))
    return build(r.rows, [(1, LO, 0)], counts=(4, 4, 0, 0))


def _no_particles():
    r = Rows()
    r.track(1, (2, 4, 6, 8))
    return build(r.rows, [], counts=(4, 4, 0, 0))


def _no_rows():
    return build([], [(1, HI, 0)], counts=(0, 0, 0, 0))


# ---- 12: the packed key's range (the device path only)
def _range(field):
    r = Rows()
    r.track(1, (2, 4, 6, 8))
    row = list(r.rows[-1])
    if field == "module":
        row[5] = 1 << 21
    else:
        row[3] = -1
    r.rows.append(tuple(row[:1] + [999] + row[2:]))
    return build(r.rows, [(1, HI, 0)], dev_raises=True, counts=(4, 5, 1, 1))


CASES = {
    "dup_pairs": _dup_pairs,
    "interleaved_descending": _interleaved_descending,
    "shared_hit": _shared_hit,
    "truth_two_rows": _truth_two_rows,
    "truth_selects": _truth_selects,
    "truth_missing": _truth_missing,
    "own_shared_hit": _own_shared_hit,
    "window_one": lambda: _window(8, 8),
    "window_several": lambda: _window(7, 9),
    "pt_cut_zero_absent": lambda: _pt_cut(False),
    "pt_cut_zero_present": lambda: _pt_cut(True),
    "reference": _reference,
    "ids": _ids,
    "runs": _runs,
    "nothing_in_window": _nothing_in_window,
    "no_high_pt": _no_high_pt,
    "no_particles": _no_particles,
    "no_rows": _no_rows,
    "range_module": lambda: _range("module"),
    "range_volume": lambda: _range("volume"),
}


# ---- seeded random events
N_RANDOM = 20


def random_event(seed, separate):
    """<= 2,000 rows over id ranges small enough to collide: about 60 particles (0 and negative ids
    among them) of 1-40 rows, hits shared between rows, repeated rows, volumes 6-9 with the window
    (7, 8). separate: truth columns of their own, some hits with two rows of different particles."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(600, 1900))
    pids = np.unique(np.concatenate([[0, -3, -B59], rng.integers(1, 400, 60), B59 + rng.integers(0, 50, 10)]))
    weight = rng.integers(1, 41, pids.size).astype(np.float64)
    pid = rng.choice(pids, n, p=weight / weight.sum())
    node = rng.integers(-5, n // 3, n)
    hit = rng.integers(0, n, n) + (1 << 32) * rng.integers(0, 2, n)
    vol = rng.choice([6, 7, 7, 7, 8, 8, 9], n)
    lay = rng.choice([2, 4, 6, 8, 10, 12, 14], n)
    mod = rng.integers(0, 40, n)
    rows = np.stack([node, hit, pid, vol, lay, mod], 1)
    rep = rng.integers(0, n, max(n // 20, 2))          # repeated rows: (node, hit) pairs twice
    rows = np.concatenate([rows, rows[rep]])[rng.permutation(n + rep.size)]
    known = pids[rng.random(pids.size) < 0.9]
    px = np.where(rng.random(known.size) < 0.7, 1.5, 0.3)
    truth = None
    if separate:
        hits = np.unique(rows[:, 1])
        th = np.concatenate([hits, rng.choice(hits, hits.size // 4)])
        tp = rng.choice(pids, th.size)
        o = rng.permutation(th.size)
        truth = list(zip(th[o], tp[o]))
    return build(rows, list(zip(known, px, np.zeros(known.size))), truth=truth, window=(7, 8))
