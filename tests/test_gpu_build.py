"""gtf_build_event_csr_device -- event conversion's graph build on the GPU (SURVEY §8f
#2) -- against the host builder gtf_build_event_csr, which tests/test_build.py pins to
the reference's networkx construction and tests/test_real800.py to the reference's own
packed 800' network (structure digest). The device build must give the same arrays bit
for bit: node order (CPython set order for components under half the graph), subgraph
ids, slots, successor order and the track_state_estimates key order.

Inputs: the committed vol-7 134 event, the 800' all-volume event, the synthetic CSV
events of test_build.py (duplicates, self loops, unknown ends, a component over half the
graph, a dense id space) and a C4-sized edge list (1M directed edges) from the synthetic
generator's graph; and, on raw buffers between guard bytes as tests/test_gpu_build_batch.py
does for the batch, the small hand-made events of tests/build_batch_cases.py one at a time,
the same events as a batch of one, and every refusal of the single-event entry point."""
import ctypes
import os

import numpy as np
import pytest

import build_batch_cases as bb
import real800 as R
from fixtures import GOLDEN
from guard_mem import FILL, Mem, at, untouched
from gtf import _native as nat
from gtf import io, synth
from test_build import _equal, _write_event

gpu = pytest.mark.gpu   # every test but the workspace sizes at the end

KEYS = ("order", "sub_id", "slot_ptr", "slot_src", "tse_rank", "out_ptr", "out_slot")


def _both_builders(prefix, lo, hi):
    return io.build_event_csr(prefix, lo, hi) + io.build_event_csr(prefix, lo, hi, device="cuda")


@gpu
def test_device_build_vol7():
    _equal(*_both_builders(os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_"), 7, 7))


@gpu
def test_device_build_800_all_volumes():
    g, v = io.build_event_csr(R.PREFIX, *R.VOLS, device="cuda")
    assert g.n_nodes == 29590 and g.n_edges == 89028
    assert R.structure_digest(g) == str(R.fixture("pass")["structure_sha"])
    _equal(g, v, *io.build_event_csr(R.PREFIX, *R.VOLS))


@gpu
@pytest.mark.parametrize("seed,n,rows,space,chain", [(0, 400, 300, 10 ** 6, 0.0), (1, 3000, 4000, 5000, 0.0),
                                                     (2, 2000, 1500, 10 ** 6, 0.7), (3, 5000, 9000, 2 ** 40, 0.3)])
def test_device_build_synthetic(tmp_path, seed, n, rows, space, chain):
    _equal(*_both_builders(_write_event(str(tmp_path), seed, n, rows, space, chain), 7, 8))


def _rows_of(g, seed):
    """the undirected edges of a packed graph as shuffled CSV rows, random node ids"""
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(g.n_nodes), np.diff(g.slot_ptr))
    src = g.slot["slot_src"]
    keep = (src >= 0) & (src < dst)
    a, b = src[keep], dst[keep]
    perm = rng.permutation(a.size)
    flip = rng.random(a.size) < 0.5
    a, b = np.where(flip, b, a)[perm], np.where(flip, a, b)[perm]
    ids = rng.choice(2 ** 40, size=g.n_nodes, replace=False).astype(np.int64)
    return ids, ids[a], ids[b]


@gpu
@pytest.mark.parametrize("workload", ["c2", "c4"])
def test_device_build_generator_sized(workload):
    g = synth.workload(workload, seed=3)
    ids, a, b = _rows_of(g, 5)
    oh, eh, sh = io.csr_from_rows(ids, a, b)
    od, ed, sd = io.csr_from_rows(ids, a, b, device="cuda")
    assert (eh, sh) == (ed, sd) and eh == 2 * a.size
    for k in KEYS:
        n = {"slot_src": eh, "tse_rank": eh, "out_slot": eh}.get(k, oh[k].size)
        assert np.array_equal(oh[k][:n], od[k][:n]), k


@gpu
def test_device_build_rejects_duplicate_ids():
    ids = np.array([5, 7, 5], np.int64)
    with pytest.raises(RuntimeError, match="duplicate"):
        io.csr_from_rows(ids, np.array([5], np.int64), np.array([7], np.int64), device="cuda")


@gpu
def test_device_build_no_edges():
    ids = np.array([9, 3, 4], np.int64)
    o, e, s = io.csr_from_rows(ids, np.zeros(0, np.int64), np.zeros(0, np.int64), device="cuda")
    oh, eh, sh = io.csr_from_rows(ids, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert (e, s) == (eh, sh) == (0, 3)
    for k in ("order", "sub_id", "slot_ptr", "out_ptr"):
        assert np.array_equal(o[k], oh[k]), k


# ---------------------------------------------------------------- the C-ABI between guard bytes
def _merged(*parts):
    """parts with disjoint ids as one event"""
    return tuple(np.concatenate(c) for c in zip(*parts))


# every distinct part of build_batch_cases.CASES with at most a few hundred nodes, as an event of its own, and
# BIG + HALF + THIRD as one event: the half-size rule is then taken against 216 nodes, and HALF's component of
# four goes from CSV order to set order
EVENTS = {
    "half": bb.HALF, "third": bb.THIRD, "big": bb.BIG, "a60": bb.A60, "a60_other_rows": bb.A60_OTHER_ROWS,
    "empty": bb.EMPTY, "rows_only": bb.ROWS_ONLY, "tiny0": bb.tiny(0), "tiny1": bb.tiny(1), "tiny2": bb.tiny(2),
    "sized255": bb.CASES["block_boundary"][0], "sized1": bb.CASES["block_boundary"][1],
    "sized257": bb.CASES["block_boundary"][2], "loops_repeats": bb.CASES["loops_repeats"][1],
    "deep_chain": bb.CASES["deep_chain"][1], "dense_ids0": bb.CASES["dense_ids"][0],
    "dense_ids1": bb.CASES["dense_ids"][1], "big_half_third": _merged(bb.BIG, bb.HALF, bb.THIRD),
}
_HOST = {}


def _host(name):
    """io.csr_from_rows of EVENTS[name] on the host, once: read-only"""
    if name not in _HOST:
        _HOST[name] = io.csr_from_rows(*EVENTS[name])
    return _HOST[name]


def _abi(part, mem, batch_of_one=False, tamper=None, ws_short=0):
    """gtf_build_event_csr_device -- or gtf_build_events_csr_device with the event as a batch of one -- on raw
    buffers: every output (the batch's event column too) and the workspace lie between guard bytes. Returns
    (status, outputs as host arrays at their allocated sizes, n_edges, n_sub)."""
    L = nat.lib()
    m = Mem(mem)
    N, Rr = int(part[0].size), int(part[1].size)
    ids, a, b = (m.up(np.concatenate([c, np.zeros(1, np.int64)])) for c in part)   # (never empty)
    size = {"order": N, "sub_id": N, "slot_ptr": N + 1, "out_ptr": N + 1, "slot_src": 2 * Rr, "tse_rank": 2 * Rr,
            "out_slot": 2 * Rr}
    if batch_of_one:
        size["event"] = N
    out = {k: m.guarded(4 * n) for k, n in size.items()}
    nb = int(L.gtf_build_events_device_workspace_bytes(N, Rr, 1) if batch_of_one else
             L.gtf_build_event_device_workspace_bytes(N, Rr))
    ws = m.guarded(nb)
    ev = nat.GtfEventCsr(N, Rr, ids.data_ptr(), a.data_ptr(), b.data_ptr(), *[at(out[k]) for k in KEYS], 0, 0, 0)
    if tamper:
        tamper(ev)
    if batch_of_one:
        node_off, row_off = np.array([0, N], np.int32), np.array([0, Rr], np.int32)
        bt = nat.GtfEventBatch(n_events=1, node_off=node_off.ctypes.data, row_off=row_off.ctypes.data,
                               event=at(out["event"]))
        rc = L.gtf_build_events_csr_device(ctypes.byref(ev), ctypes.byref(bt), at(ws), ctypes.c_size_t(nb), m.stream)
    else:
        rc = L.gtf_build_event_csr_device(ctypes.byref(ev), at(ws), ctypes.c_size_t(nb - ws_short), m.stream)
    got = {k: m.payload(out[k], 4 * n) for k, n in size.items()}
    m.payload(ws, nb, np.uint8)
    return rc, got, int(ev.n_edges), int(ev.n_subgraphs)


@gpu
@pytest.mark.parametrize("mem", ["torch", "hip"])
@pytest.mark.parametrize("name", list(EVENTS))
def test_single_event_abi_equals_the_host_builder(name, mem):
    exp, E, B = _host(name)
    N = int(EVENTS[name][0].size)
    rc, got, e, b = _abi(EVENTS[name], mem)
    assert rc == 0, nat.lib().gtf_last_error()
    assert (e, b) == (E, B)
    for k in KEYS:
        n = {"order": N, "sub_id": N, "slot_ptr": N + 1, "out_ptr": N + 1}.get(k, E)
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k][:n], exp[k][:n]), k
    for k in ("slot_src", "tse_rank", "out_slot"):      # beyond the kept edges nothing is written
        assert bool((got[k][E:].view(np.uint8) == FILL).all()), k


@gpu
@pytest.mark.parametrize("name", list(EVENTS))
def test_batch_of_one_equals_the_single_event_call(name):
    rc, one, e, b = _abi(EVENTS[name], "torch")
    assert rc == 0, nat.lib().gtf_last_error()
    rc, got, e1, b1 = _abi(EVENTS[name], "torch", batch_of_one=True)
    assert rc == 0, nat.lib().gtf_last_error()
    assert (e1, b1) == (e, b) == _host(name)[1:]
    for k in KEYS:
        assert got[k].dtype == one[k].dtype and got[k].tobytes() == one[k].tobytes(), k
    assert got["event"].dtype == np.int32 and not got["event"].any()


@gpu
def test_single_event_refusals_leave_the_outputs_untouched():
    L = nat.lib()
    who = b"gtf_build_event_csr_device: "

    def refused(text, part=bb.HALF, exact=False, **kw):
        rc, got, _, _ = _abi(part, "torch", **kw)
        msg = L.gtf_last_error()
        assert rc == -2 and msg.startswith(who) and (msg == who + text if exact else text in msg), (rc, msg)
        assert untouched(got), text

    refused(b"workspace smaller than gtf_build_event_device_workspace_bytes", exact=True, ws_short=1)

    def too_large(ev):
        ev.n_nodes = (2 ** 31 - 1) // 2 + 1
    refused(b"graph too large for int32 indices", exact=True, tamper=too_large)

    def rows_too_large(ev):
        ev.n_rows = (2 ** 31 - 1) // 4 + 1
    refused(b"graph too large for int32 indices", exact=True, tamper=rows_too_large)

    def null_output(ev):
        ev.sub_id = None
    refused(b"bad arguments", exact=True, tamper=null_output)
    assert L.gtf_build_event_csr_device(None, ctypes.c_void_p(256), 256, None) == -2
    assert L.gtf_last_error() == who + b"bad arguments"
    refused(b"2^61", part=bb.part([1, 2, bb.TOP + 1], [(1, 2)]))
    refused(b"2^61", part=bb.part([3, -4], [(3, -4)]))
    refused(b"duplicate node id", exact=True, part=bb.part([4, 5, 4], [(4, 5)]))   # (no "in event")


# ---------------------------------------------------------------- the workspace sizes (CPU: no device is asked)
SIZE_POINTS = [(0, 0), (1, 0), (1, 1), (255, 255), (256, 256), (257, 257), (4096, 8192), (100000, 300000)]
SIZE_EVENTS = (0, 1, 64, 4096)
# (single [point], batch [point][events]) recorded from the library before the fold
WITHOUT_DEVICE = ([7424, 7424, 7680, 140032, 144640, 147200, 3613696, 121703424],
                  [[7936, 7936, 8448, 40704], [7936, 7936, 8448, 40704], [8192, 8192, 8704, 40960],
                   [140544, 140544, 141056, 173312], [145152, 145152, 145664, 177920],
                   [147712, 147712, 148224, 180480], [3614208, 3614208, 3614720, 3646976],
                   [121703936, 121703936, 121704448, 121736704]])
WITH_DEVICE = ([8448, 8448, 8704, 141056, 145664, 148224, 3810048, 128908032],           # (an MI355X)
               [[8960, 8960, 9472, 41728], [8960, 8960, 9472, 41728], [9216, 9216, 9728, 41984],
                [141568, 141568, 142080, 174336], [146176, 146176, 146688, 178944],
                [148736, 148736, 149248, 181504], [3810560, 3810560, 3811072, 3843328],
                [128908544, 128908544, 128909056, 128941312]])


def test_workspace_sizes_are_the_recorded_ones():
    """gtf_build_event_device_workspace_bytes and gtf_build_events_device_workspace_bytes at SIZE_POINTS (and
    SIZE_EVENTS events) against the values the library gave before the two builds were folded into one: the
    layout of the workspace is part of neither build's change. The hipcub scratch in the middle of the layout is
    sized by hipcub itself, which answers 0 without a device (gtf_host.h CubNeed), so there is one table per
    case; the batch's two offset tables come last in both."""
    L = nat.lib()
    single = [int(L.gtf_build_event_device_workspace_bytes(n, r)) for n, r in SIZE_POINTS]
    batch = [[int(L.gtf_build_events_device_workspace_bytes(n, r, k)) for k in SIZE_EVENTS] for n, r in SIZE_POINTS]
    import torch
    exp_single, exp_batch = WITH_DEVICE if torch.cuda.is_available() else WITHOUT_DEVICE
    assert single == exp_single
    assert batch == exp_batch
    for s, row in zip(single, batch):       # one event's layout, then 2 (K + 1) int32 in 256-byte pieces
        assert [b - s for b in row] == [2 * ((4 * (k + 1) + 255) // 256 * 256) for k in SIZE_EVENTS]
