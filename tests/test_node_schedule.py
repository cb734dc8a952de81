"""The node schedule's sub-buckets (gtf.device.node_schedule, no GPU): inside the <= 4-, <= 8-
and <= 16-slot buckets the nodes of the narrower lane group (<= 2, <= 6, <= 12 slots) come
first, in node order, and n_g2 / n_g6 / n_g12 count them -- the fused node kernel runs
those entries on 2, 6 and 12 lanes (include/gtf.h, ABI v8)."""
import numpy as np

from gtf import synth
from gtf.device import node_schedule
from gtf.graph import BUCKETS


def _check(slot_ptr):
    deg = np.diff(np.asarray(slot_ptr, dtype=np.int64))
    sched, n_g, n_big, (n_g2, n_g6, n_g12) = node_schedule(slot_ptr)
    assert sorted(sched.tolist()) == list(range(deg.size))
    assert sum(n_g) + n_big == deg.size
    lo = 0
    for (dlo, dhi), n, (narrow, first) in zip(BUCKETS, n_g, ((2, n_g2), (6, n_g6), (12, n_g12), (None, 0), (None, 0))):
        part = sched[lo:lo + n]
        d = deg[part]
        assert n == int(((deg >= dlo) & (deg <= dhi)).sum())
        assert ((d >= dlo) & (d <= dhi)).all()
        if narrow is None:
            assert (np.diff(part) > 0).all()
        else:   # the narrow group's nodes first, node order inside either part
            assert first == int(((deg >= dlo) & (deg <= narrow)).sum())
            assert (d[:first] <= narrow).all() and (d[first:] > narrow).all()
            assert (np.diff(part[:first]) > 0).all() and (np.diff(part[first:]) > 0).all()
        lo += n
    assert (deg[sched[lo:]] > 64).all() and n_big == int((deg > 64).sum())
    return n_g, (n_g2, n_g6, n_g12)


def test_sub_buckets_first_and_counted():
    g = synth.event(seed=7, n_tracks=1000, fake_mean=synth.C4_FAKE)
    deg = np.diff(g.slot_ptr)
    n_g, (n_g2, n_g6, n_g12) = _check(g.slot_ptr)
    # the histogram of this event: every class is populated
    assert n_g6 == int(((deg >= 5) & (deg <= 6)).sum()) == 842
    assert n_g[1] - n_g6 == int(((deg >= 7) & (deg <= 8)).sum()) == 284
    assert n_g12 == int(((deg >= 9) & (deg <= 12)).sum()) == 182
    assert n_g[2] - n_g12 == int(((deg >= 13) & (deg <= 16)).sum()) == 68


def test_sub_buckets_degenerate():
    # every slot count 0..70 once, then graphs with none of a class, then no node at all
    _check(np.concatenate([[0], np.cumsum(np.arange(71))]))
    n_g, sub = _check(np.concatenate([[0], np.cumsum([7, 8, 13, 16, 3, 4] * 3)]))
    assert sub == (0, 0, 0) and n_g[:3] == [6, 6, 6]
    n_g, sub = _check(np.concatenate([[0], np.cumsum([5, 6, 9, 12, 1, 2] * 3)]))
    assert sub == (6, 6, 6) and n_g[:3] == [6, 6, 6]
    n_g, sub = _check(np.zeros(1, np.int64))
    assert sub == (0, 0, 0) and sum(n_g) == 0
