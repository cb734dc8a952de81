"""Hand-made events for the candidate scoring (gtf.metrics.reconstruction_efficiency on the host,
gtf_score_* on the device): small hit mappings and candidate lists, one per branch of
reconstruction_efficiency.py:118-183. tests/test_score_cases.py checks that every case reaches
the branch it is named for, on gtf.metrics and on oracle/metrics_oracle.py alike;
tests/test_gpu_score.py runs them on the device.

A case: "m" (HitMapping), "particles" (id, px, py), "calls": a list of (group, candidates), each
candidate a list of node ids -- the host scores the candidates of all calls concatenated by
ascending group, the device takes one gtf_score_candidates call each, in any order -- and
"expect": what the case is about (checked by test_score_cases.check)."""
import numpy as np

from gtf import metrics

B60 = 1 << 59   # particle ids of the fixture's size


class World:
    """an event under construction: every hit is one mapping row (node, hit, particle, volume 7,
    layer, module); hit ids count up, modules are the hit ids unless given (no shared module)"""

    def __init__(self, node0=10, stride=3):
        self.rows, self.pt, self._node, self._stride = [], {}, node0, stride

    def nodes(self, n):
        out = [self._node + self._stride * i for i in range(n)]
        self._node += self._stride * n
        return out

    def hit(self, node, pid, layer, module=None, pt=2.0):
        h = 100 + len(self.rows)
        self.rows.append((node, h, pid, 7, layer, h if module is None else module))
        self.pt.setdefault(pid, pt)

    def track(self, pid, n, pt=2.0, layers=None):
        """a particle with one hit on each of n fresh nodes, on n distinct layers -> the nodes"""
        ns = self.nodes(n)
        for i, v in enumerate(ns):
            self.hit(v, pid, 2 * i + 2 if layers is None else layers[i], pt=pt)
        return ns

    def singles(self, n, pid0):
        """n fresh nodes, each the one hit of a particle of its own (pid0, pid0 + 1, ...)"""
        ns = self.nodes(n)
        for i, v in enumerate(ns):
            self.hit(v, pid0 + i, 2)
        return ns

    def build(self, calls, expect, drop=()):
        a = np.array(self.rows, np.int64).T
        pids = [p for p in self.pt if p not in drop]
        return {"m": metrics.HitMapping(*a), "particles": (np.array(pids, np.int64),
                                                            np.array([self.pt[p] for p in pids], np.float64),
                                                            np.zeros(len(pids))),
                "calls": [(g, [list(c) for c in cs]) for g, cs in calls], "expect": expect}


def _ties():
    w = World()
    a, b = w.track(9, 4), w.track(5, 4)
    return w.build([(0, [a[:2] + b[:2], b[:2] + a[:2]])], {"pid": [9, 5], "n_good": [2, 2], "total": [4, 4], "tie": True})


def _dense(w, pid, n, filler0):
    """a candidate of n entries over nodes of up to 6 hits: hit 0 of every node is pid's, the
    others cycle through 7 filler particles -> (nodes, pid's count)"""
    ns = w.nodes((n + 5) // 6)
    e = 0
    for k, v in enumerate(ns):
        for j in range(min(6, n - 6 * k)):
            w.hit(v, pid if j == 0 else filler0 + e % 7, 2 * k + 2)
            e += 1
    return ns, len(ns)


SIZES = (1, 2, 63, 64, 65, 200)


def _sizes():
    w = World()
    cands, pid, good, total = [], [], [], []
    for i, n in enumerate(SIZES):
        ns, cnt = _dense(w, 1000 + i, n, 2000 + 10 * i)
        cands.append(ns)
        # (the fillers: 5 of 6 entries over 7 ids stay below one per node once there are 2 nodes)
        total.append(n)
        pid.append(1000 + i)
        good.append(cnt)
        cands.append(w.track(3000 + i, n))      # n members of one hit each
        total.append(n)
        pid.append(3000 + i)
        good.append(n)
    return w.build([(0, cands)], {"pid": pid, "n_good": good, "total": total})


def _late_winner():
    w = World()
    c = w.singles(63, 5000) + w.track(4999, 2)
    a = w.track(1, 4)
    return w.build([(0, [c, a])], {"pid": [4999, 1], "n_good": [2, 4], "total": [65, 4], "first_at": 63})


def _empty_between():
    w = World()
    a, b = w.track(1, 4), w.track(2, 5)
    return w.build([(0, [a, [], b])], {"pid": [1, 0, 2], "n_good": [4, 0, 5], "total": [4, 0, 5], "matched": [1, 0, 1]})


def _no_candidates():
    w = World()
    w.track(1, 4)
    return w.build([(0, [])], {"pid": [], "n_good": [], "total": [], "matched": []})


def _dup_in_call():
    w = World()
    a = w.track(1, 6)
    return w.build([(0, [a[:3], a])], {"pid": [1, 1], "n_good": [3, 6], "total": [3, 6], "matched": [1, 0],
                                       "purities": ([1.0], [0.5])})


def _dup_across(first_short):
    w = World()
    a = w.track(1, 6)
    calls = [(0, [a[:3]]), (1, [a])] if first_short else [(0, [a]), (1, [a[:3]])]
    pur = ([1.0], [0.5]) if first_short else ([1.0], [1.0])
    return w.build(calls, {"matched": [1, 0], "purities": pur})


def _thresholds():
    w = World()
    a, b, c, d = w.track(1, 6), w.track(2, 7), w.track(3, 4), w.track(4, 4)
    n1, n2 = w.singles(2, 700), w.singles(3, 710)
    return w.build([(0, [a[:3], b[:3], c[:2] + n1, d[:2] + n2])],
                   {"pid": [1, 2, 3, 4], "n_good": [3, 3, 2, 2], "total": [3, 3, 4, 5], "hits": [6, 7, 4, 4],
                    "matched": [1, 0, 1, 0]})


def _not_in_region():
    w = World()
    e, a = w.track(8, 4, pt=0.5), w.track(1, 4)
    return w.build([(0, [e, a])], {"pid": [8, 1], "matched": [0, 1], "absent": [8]})


def _not_reference():
    w = World()
    f = w.track(6, 3)                                  # three layers
    g = w.nodes(5)                                     # four layers, two hits on one module
    for v, (lay, mod) in zip(g, ((2, 1), (4, 2), (6, 3), (8, 4), (8, 4))):
        w.hit(v, 7, lay, mod)
    a = w.track(1, 4)
    return w.build([(0, [f, g, a])], {"pid": [6, 7, 1], "matched": [0, 0, 1], "non_reference": [6, 7]})


def _pid_zero(noise):
    w = World()
    z, a = w.track(0, 5), w.track(1, 4)
    return w.build([(0, [z + a[:2], a])], {"pid": [0, 1], "n_good": [5, 4], "total": [7, 4], "matched": [0 if noise else 1, 1]},
                   drop=(0,) if noise else ())


def _ids60():
    w = World()
    a, b = w.track(B60 + 5, 4), w.track((1 << 58) + 5, 4)     # the same low 32 bits
    c = w.track(B60 + (1 << 40) + 7, 6)
    return w.build([(0, [a[:1] + b[:2], c, b])],
                   {"pid": [(1 << 58) + 5, B60 + (1 << 40) + 7, (1 << 58) + 5], "n_good": [2, 6, 4], "total": [3, 6, 4],
                    "matched": [1, 1, 0]})


def _table_ends():
    w = World(node0=0)
    a = w.track(1, 4)
    mid = w.track(2, 4)
    z = w.track(3, 4)
    return w.build([(0, [[a[0], z[-1], a[1], a[2]], [z[-1], z[0], z[1], a[0]], mid])],
                   {"pid": [1, 3, 2], "n_good": [3, 3, 4], "matched": [1, 1, 1], "ends": (a[0], z[-1])})


def _missing():
    w = World()
    a = w.track(1, 4)
    return w.build([(0, [a, a[:2] + [a[-1] + 1]])], {"raises": True})


def _repeated_member():
    w = World()
    a = w.track(1, 6)
    n = w.singles(1, 50)
    return w.build([(0, [[a[0], a[0], a[0], n[0], a[1]]])], {"pid": [1], "n_good": [4], "total": [5], "matched": [1]})


CASES = {
    "tie_first_seen": _ties,
    "sizes": _sizes,
    "late_winner": _late_winner,
    "empty_between": _empty_between,
    "no_candidates": _no_candidates,
    "dup_in_call": _dup_in_call,
    "dup_across_short_first": lambda: _dup_across(True),
    "dup_across_full_first": lambda: _dup_across(False),
    "thresholds": _thresholds,
    "not_in_region": _not_in_region,
    "not_reference": _not_reference,
    "pid_zero_noise": lambda: _pid_zero(True),
    "pid_zero_particle": lambda: _pid_zero(False),
    "ids_60bit": _ids60,
    "table_ends": _table_ends,
    "missing_id": _missing,
    "repeated_member": _repeated_member,
}


def flatten(case):
    """the candidates of every call by ascending group -> (cand_ptr, cand_ids) as the host function takes them"""
    cands = [c for _, cs in sorted(case["calls"], key=lambda x: x[0]) for c in cs]
    ptr = np.zeros(len(cands) + 1, np.int64)
    ptr[1:] = np.cumsum([len(c) for c in cands])
    ids = np.array([v for c in cands for v in c], np.int64)
    return ptr, ids, cands


def host_result(case):
    ptr, ids, _ = flatten(case)
    pid, px, py = case["particles"]
    return metrics.reconstruction_efficiency(ptr, ids, case["m"], pid, px, py, 7, 7)


def tables(case):
    pid, px, py = case["particles"]
    return metrics.truth_tables(case["m"], pid, px, py, 7, 7)
