"""Parabolic-model edge states and pairwise KL distances on the GPU.

Host side of ``gtf_parabolic_kl`` (include/gtf.h). It mirrors the reference's
training-data generator in learn_KL_parabolic_model/src/generate_training_data:

* ``compute_track_state_estimates`` (utils.py:221-289): per in-edge parabolic
  state ``edge_state_vector`` (3,) / ``edge_covariance`` (3, 3) and the node's
  ``xy_edge_gradient_mean_var``;
* ``calc_pairwise_distances`` + the row loop of
  extract_metadata_trackml_parabolic_model.py:15-99: one ``(kl_dist, emp_var,
  truth)`` row per pair i > j of the in-edges of every node with >= 2 in-edges.

Pairs are laid out node by node (node order), row-major lower triangle over the
node's in-slots (slot order = sender index order); ``ParabolicKL.pair_index``
gives each row's node and slot positions. The reference orders its rows by glob()
file order and dict order, which carry no meaning; the row
multiset is what parity is checked on.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _native as nat
from .graph import TrackGraph

BUCKETS = ((1, 2), (3, 4), (5, 8), (9, 1 << 30))   # in-degree ranges of the 1/4/8/64-lane groups
TILE_MAX = 256   # bucket-0 nodes per tile of the tiled layout (one per thread of a gtf_kl.hip WBLOCK)
WIN_NODES = 1024   # LDS window of a tile (gtf_kl.hip WWIN)
WIN_MARGIN = 128   # window nodes either side of a tile (99 % of the vol-7 neighbours lie within 73)


def _ptr(t):
    if t is None:
        return ctypes.c_void_p(0)
    if t.numel() == 0 and t._base is not None:   # an empty view of a one-element buffer (an empty event's
        t = t._base                               # arrays): its own data_ptr() is null, the buffer's is not
    return ctypes.c_void_p(t.data_ptr())


def quantise_xy(gnn, scale=None):
    """(q [N, 2] int32, scale): the x, y columns of ``gnn`` as 32-bit fixed point, the
    compact input of gtf_parabolic_kl_q32 (include/gtf.h). scale = 2^(e - 30) with e the
    smallest integer such that every |x|, |y| < 2^e, and q = rint(xy / scale): every
    |q| < 2^30 (the difference of two coordinates is then an exact int32), q * scale is
    exact in fp64 and within scale / 2 of the input. A given ``scale`` (a replica keeps its
    parent's) is used as it is; coordinates that do not fit it raise ValueError."""
    xy = np.asarray(gnn, np.float64)
    xy = xy.reshape(-1, xy.shape[-1] if xy.ndim > 1 else 2)[:, :2]   # ([N, 2], [N, 4] or flat x, y pairs)
    if not np.isfinite(xy).all():
        raise ValueError("quantise_xy: non-finite coordinate")
    m = float(np.abs(xy).max()) if xy.size else 0.0
    if scale is None:
        e = int(np.frexp(m)[1]) if m > 0.0 else 0   # m = f * 2^e with 0.5 <= f < 1: 2^(e - 1) <= m < 2^e
        if np.rint(np.ldexp(m, 30 - e)) >= 2.0 ** 30:   # (within half a step of 2^e: it would round to 2^30)
            e += 1
        scale = float(np.ldexp(1.0, e - 30))
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError("quantise_xy: scale must be finite and > 0")
    q = np.rint(xy / scale)
    if q.size and np.abs(q).max() >= 2.0 ** 30:
        raise ValueError("quantise_xy: max |x|, |y| = %g does not fit scale %g (|q| < 2^30)" % (m, scale))
    return np.ascontiguousarray(q.astype(np.int32)), scale


def in_edge_csr(g: TrackGraph):
    """(slot_ptr, slot_src) of the graph's in-edges (slots that are edges)."""
    ise = g.slot["is_edge"].astype(bool)
    if ise.all():
        return g.slot_ptr.astype(np.int32), g.slot["slot_src"].astype(np.int32)
    dst = g.slot_dst()
    cnt = np.bincount(dst[ise], minlength=g.n_nodes)
    ptr = np.zeros(g.n_nodes + 1, np.int32)
    np.cumsum(cnt, out=ptr[1:])
    return ptr, g.slot["slot_src"][ise].astype(np.int32)


def _down(t):
    return t.cpu().numpy() if t is not None else None


def _lazy(name, fetch):
    """an attribute that is either assigned or, on its first read, fetched and kept"""
    key = "_lazy_" + name

    def fget(self):
        if key not in self.__dict__:
            self.__dict__[key] = fetch(self)
        return self.__dict__[key]

    def fset(self, v):
        self.__dict__[key] = v
    return property(fget, fset)


def _raise_prepare_error(c):
    """the ValueError of a gtf_kl_prepare / gtf_kl_coords error word (quantise_xy's wording for its rules)"""
    e = int(c.error) if hasattr(c, "error") else int(c)
    if e & (nat.KL_ERR_SLOT_PTR | nat.KL_ERR_SOURCE | nat.KL_ERR_NODE_OF):
        raise ValueError("ParabolicKL: " + ("slot_ptr does not start at 0, decreases or does not end at n_slots"
                                            if e & nat.KL_ERR_SLOT_PTR else
                                            "a kept slot's source outside [0, n_nodes)" if e & nat.KL_ERR_SOURCE
                                            else "a node_of entry outside [0, n_nodes)"))
    if e & nat.KL_ERR_NONFINITE:
        raise ValueError("quantise_xy: non-finite coordinate")
    if e & nat.KL_ERR_SCALE:
        raise ValueError("quantise_xy: scale must be finite and > 0")
    if e & nat.KL_ERR_FIT:
        if hasattr(c, "max_abs"):
            raise ValueError("quantise_xy: max |x|, |y| = %g does not fit scale %g (|q| < 2^30)" % (c.max_abs, c.scale))
        raise ValueError("quantise_xy: the coordinates do not fit the scale (|q| < 2^30)")
    raise ValueError("ParabolicKL: device error word %d" % e)


class ParabolicKL:
    """Device-resident KL graph of one or many events (events concatenated into one CSR).

    ordered: the nodes are renumbered on upload so that each in-degree bucket is one node
    range -- one-edge nodes, two-edge nodes, then the 3..4, 5..8 and > 8 buckets, then the
    unlisted nodes -- with slots and pairs following node order (gtf_kl_graph's ordered
    layout: the kernel reaches the two-edge bucket by arithmetic). Device outputs are then
    in that order: ``node_of`` maps a device node to the caller's, pair_index() returns the
    caller's node ids, and ``host_nodes`` / ``host_slots`` reorder per-node / per-slot
    outputs; pairs keep the caller's (node, i, j) rows through pair_index().

    tile = T > 0 (T <= 256): the nodes azimuth-sorted inside sort windows (an event of a
    batch), then cut into tiles of T one- / two-edge (bucket-0) nodes and whatever lies
    between them, each tile with its bucket-0 nodes first: one 256-thread block per tile
    record (gtf_kl_graph.blk) loads its nodes' sender lists and the coordinates of a window
    of consecutive nodes around the tile -- where a hit's neighbours lie -- in one round,
    and reads the neighbours from LDS. The 3..4, 5..8 and > 8 buckets go by node list.

    compact: additionally upload the coordinates as 32-bit fixed point (quantise_xy) with
    their scale, and the truth ids as int32 (ids beyond int32 relabelled densely: only their
    equality matters), for run(out, "q32") -- gtf_parabolic_kl_q32, 12
    bytes per node instead of 24, fp32 arithmetic. The structure arrays are shared with the
    fp64 path; without compact the object and its device footprint are unchanged.

    prepare "host" (default): everything above is built in NumPy and uploaded; this is the
    definition. prepare "device": the caller's raw arrays are uploaded and gtf_kl_prepare
    (include/gtf.h) builds the same arrays in HBM, element for element; from_device and
    from_device_graph do so on arrays that are resident already. node_of, slot_of, degree,
    slot_ptr_host and pair_ptr_host are then downloaded on first use, and in the ordered layout
    ``lists`` is empty (the kernel reads ranges, no list). Not with tile > 0."""

    # host copies of the structure: set by the host constructor; after prepare="device" each is
    # downloaded on its first use (pair_index, host_nodes and host_slots read them)
    node_of = _lazy("node_of", lambda k: _down(k._node_of_dev))
    slot_of = _lazy("slot_of", lambda k: _down(k._slot_of_dev))
    slot_ptr_host = _lazy("slot_ptr_host", lambda k: k.slot_ptr.cpu().numpy().astype(np.int64))
    pair_ptr_host = _lazy("pair_ptr_host", lambda k: k.pair_ptr.cpu().numpy())
    degree = _lazy("degree", lambda k: np.diff(k.slot_ptr_host))

    def __init__(self, slot_ptr, slot_src, gnn, truth=None, device="cuda", with_single=False, ordered=False,
                 tile=0, sort_window=8192, tile_b1=True, compact=False, prepare="host"):
        if prepare not in ("host", "device"):
            raise ValueError("prepare must be 'host' or 'device'")
        if prepare == "device":   # the caller's raw arrays go up; gtf_kl_prepare builds the rest
            if int(tile) > 0:
                raise ValueError("prepare='device' does not build the tiled layout (its node order sorts by "
                                 "np.arctan2, which a device atan2 does not reproduce bit for bit): use prepare='host'")
            dev = torch.device(device)
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
            g = np.asarray(gnn, np.float64)
            g = g.reshape(-1, g.shape[-1] if g.ndim > 1 else 4)
            self._prepare_device(t(slot_ptr, np.int32).reshape(-1), t(slot_src, np.int32).reshape(-1), t(g, np.float64),
                                 t(truth, np.int64).reshape(-1) if truth is not None else None, None, with_single,
                                 ordered, compact, None)
            return
        slot_ptr = np.ascontiguousarray(slot_ptr, np.int32)
        self.n_nodes = int(slot_ptr.shape[0] - 1)
        self.n_slots = int(slot_ptr[-1])
        d = np.diff(slot_ptr).astype(np.int64)
        lo = 1 if with_single else 2
        self.node_of = self.slot_of = None
        self.tile = int(tile)
        ordered = ordered or self.tile > 0
        if ordered:
            sp = slot_ptr.astype(np.int64)
            # buckets 1 and 2 as runs of one in-degree each (3, 4 | 5, 6, 7, 8), then the > 8 bucket
            keys = [d == 1 if lo == 1 else np.zeros(d.size, bool)] + [d == q for q in range(2, 9)] + [d > 8]
            rank = np.full(d.size, len(keys), np.int64)
            for q in reversed(range(len(keys))):
                rank[keys[q]] = q
            if self.tile > 0:   # azimuth order in sort windows, cut into tiles of T bucket-0 nodes
                if not 0 < self.tile <= TILE_MAX:
                    raise ValueError("tile must be in 1..%d" % TILE_MAX)
                xy = np.asarray(gnn, np.float64).reshape(-1, 4)
                phi = np.arctan2(xy[:, 1], xy[:, 0])
                idx = np.arange(d.size, dtype=np.int64)
                o1 = np.lexsort((idx, phi, idx // sort_window))
                self.tile_b1 = bool(tile_b1)
                b0 = rank[o1] < (4 if self.tile_b1 else 2)          # the nodes a tile's threads take
                tid = np.empty(d.size, np.int64)
                tid[o1] = (np.cumsum(b0) - b0) // self.tile         # a tile: T such nodes and the rest between
                order = np.lexsort((np.argsort(o1), rank, tid))
                self._tiles = (tid[order], rank[order])
            else:
                order = np.argsort(rank, kind="stable")
            nd = d[order]
            new_ptr = np.zeros(self.n_nodes + 1, np.int64)
            np.cumsum(nd, out=new_ptr[1:])
            owner = np.repeat(np.arange(self.n_nodes), nd)
            slot_of = sp[order][owner] + (np.arange(self.n_slots) - new_ptr[owner])
            inv = np.empty(self.n_nodes, np.int64)
            inv[order] = np.arange(self.n_nodes)
            slot_src = inv[np.asarray(slot_src, np.int64)[slot_of]]
            gnn = np.asarray(gnn, np.float64).reshape(-1, 4)[order]
            truth = np.asarray(truth, np.int64)[order] if truth is not None else None
            slot_ptr = new_ptr.astype(np.int32)
            d = nd
            self.node_of, self.slot_of = order, slot_of
            self._ranges = [int(k.sum()) for k in keys]
        self.slot_ptr_host = np.asarray(slot_ptr, np.int64)
        npair = np.where(d >= 2, d * (d - 1) // 2, 0)
        pair_ptr = np.zeros(self.n_nodes + 1, np.int64)
        np.cumsum(npair, out=pair_ptr[1:])
        self.n_pairs = int(pair_ptr[-1])
        lists = [np.nonzero((d >= max(a, lo)) & (d <= b))[0].astype(np.int32) for a, b in BUCKETS]
        self.n_listed = int(sum(x.size for x in lists))
        self.degree = d
        self.pair_ptr_host = pair_ptr
        dev = torch.device(device)

        def t(a):
            # an empty array (no node, no slot) as an empty view of a one-element buffer: _ptr passes
            # the buffer's address, since the C-ABI takes a null pointer for a missing array
            a = np.ascontiguousarray(a)
            if a.size:
                return torch.from_numpy(a).to(dev)
            return torch.empty(1, dtype=torch.from_numpy(a).dtype, device=dev)[:0].reshape(a.shape)
        self.slot_ptr = t(slot_ptr)
        self.slot_src = t(np.asarray(slot_src, np.int32))
        # the kernel reads GNN_Measurement x and y only: a compact [N, 2] copy (gnn_stride 2)
        # halves the bytes of the node and neighbour coordinate gathers
        self.gnn = t(np.asarray(gnn, np.float64).reshape(-1, 4)[:, :2])
        self.truth = t(np.asarray(truth, np.int64)) if truth is not None else None
        self.pair_ptr = t(pair_ptr)
        self.lists = [t(x) for x in lists]
        self.device = dev
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.q = self.truth32 = self.scale = self._q = None
        if compact:
            self._set_compact(np.asarray(gnn, np.float64).reshape(-1, 4), truth)
        if self.tile > 0:   # one block record per tile (gtf_kl_graph.blk); buckets 1..3 by list
            blk = self._block_table(d, pair_ptr)
            self.blk = t(blk)
            self.n_blk = int(blk.size // 12)
            by_list = [q >= (2 if self.tile_b1 else 1) and self.lists[q].numel() > 0 for q in range(4)]
            self._g = nat.GtfKlGraph(self.n_nodes, self.n_slots, _ptr(self.slot_ptr), _ptr(self.slot_src),
                                     _ptr(self.gnn), _ptr(self.truth), _ptr(self.pair_ptr),
                                     (ctypes.c_void_p * 4)(*[x.data_ptr() if b else None
                                                             for x, b in zip(self.lists, by_list)]),
                                     (ctypes.c_int32 * 4)(*[x.numel() if b else 0 for x, b in zip(self.lists, by_list)]),
                                     (ctypes.c_int32 * 4)(), 0, 2, 0, 0, _ptr(self.blk), self.n_blk)
        elif ordered:   # bucket ranges, no lists
            n1, n2 = self._ranges[0], self._ranges[1]
            counts = [n1 + n2] + [int(x.size) for x in lists[1:]]
            first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
            self._g = nat.GtfKlGraph(self.n_nodes, self.n_slots, _ptr(self.slot_ptr), _ptr(self.slot_src),
                                     _ptr(self.gnn), _ptr(self.truth), _ptr(self.pair_ptr),
                                     (ctypes.c_void_p * 4)(), (ctypes.c_int32 * 4)(*counts),
                                     (ctypes.c_int32 * 4)(*first.tolist()), n1, 2, 0, 0)
            if os.environ.get("GTF_KL_DEG_RUNS", "1") != "0":   # degree runs (0: the round-3 ordered form)
                self._g.deg_runs = 1
                for q in range(6):
                    self._g.n_deg[q] = self._ranges[2 + q]
        else:
            self._g = nat.GtfKlGraph(self.n_nodes, self.n_slots, _ptr(self.slot_ptr), _ptr(self.slot_src),
                                     _ptr(self.gnn), _ptr(self.truth), _ptr(self.pair_ptr),
                                     (ctypes.c_void_p * 4)(*[x.data_ptr() if x.numel() else None for x in self.lists]),
                                     (ctypes.c_int32 * 4)(*[x.numel() for x in self.lists]), gnn_stride=2)

    def _set_compact(self, gnn, truth, scale=None):
        """upload the fixed-point coordinates (device node order) and int32 truth ids"""
        q, self.scale = quantise_xy(np.asarray(gnn, np.float64)[:, :2], scale)
        self.q = torch.from_numpy(q).to(self.device) if q.size else torch.empty(2, dtype=torch.int32, device=self.device)[:0].reshape(0, 2)
        if truth is not None and self.truth32 is None:
            # the kernel only compares ids: those that fit int32 go as they are, others (TrackML
            # particle ids are 60-bit numbers) as dense labels, equal exactly where the ids are
            t64 = np.asarray(truth, np.int64)
            if t64.size and (t64.min() < -2**31 or t64.max() >= 2**31):
                t64 = np.unique(t64, return_inverse=True)[1].reshape(-1)
            self.truth32 = (torch.from_numpy(np.ascontiguousarray(t64.astype(np.int32))).to(self.device) if t64.size
                            else torch.empty(1, dtype=torch.int32, device=self.device)[:0])
        self._q = nat.GtfKlQ32(_ptr(self.q), self.scale, _ptr(self.truth32))

    def _prepare_device(self, slot_ptr, slot_src, gnn, truth, is_edge, with_single, ordered, compact, scale):
        """gtf_kl_prepare (include/gtf.h) on device tensors in the caller's order: slot_ptr int32
        [N + 1], slot_src int32 [S], gnn float64 [N, 2] or [N, 4], truth int64 [N] or None, is_edge
        uint8 [S] or None. Leaves the object the host constructor leaves, its host copies lazy."""
        dev = slot_ptr.device
        want = ((slot_ptr, torch.int32, "slot_ptr"), (slot_src, torch.int32, "slot_src"), (gnn, torch.float64, "gnn"),
                (truth, torch.int64, "truth"), (is_edge, torch.uint8, "is_edge"))
        for a, dt, name in want:
            if a is not None and (a.dtype != dt or a.device != dev or not a.is_contiguous()):
                raise ValueError("ParabolicKL: %s must be a contiguous %s tensor on %s" % (name, dt, dev))
        N, S = int(slot_ptr.numel()) - 1, int(slot_src.numel())
        if N < 0 or gnn.dim() != 2 or gnn.shape[0] != N or gnn.shape[1] not in (2, 4):
            raise ValueError("ParabolicKL: slot_ptr holds N + 1 offsets and gnn is [N, 2] or [N, 4]")
        if (truth is not None and truth.numel() != N) or (is_edge is not None and is_edge.numel() != S):
            raise ValueError("ParabolicKL: one truth id per node, one is_edge byte per slot")
        if scale is not None and not (np.isfinite(scale) and scale > 0.0):
            raise ValueError("quantise_xy: scale must be finite and > 0")
        z = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=dev)  # noqa: E731
        o_ptr, o_src, o_xy, o_pair = z(N + 1, torch.int32), z(S, torch.int32), z(2 * N, torch.float64), z(N + 1, torch.int64)
        o_truth = z(N, torch.int64) if truth is not None else None
        o_list = z(N, torch.int32) if not ordered else None
        o_node = z(N, torch.int64) if ordered else None
        o_slot = z(S, torch.int64) if ordered else None
        o_q = z(2 * N, torch.int32) if compact else None
        o_t32 = z(N, torch.int32) if compact and truth is not None else None
        L = nat.lib()
        nb = int(L.gtf_kl_prepare_workspace_bytes(N, S))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        pin = nat.GtfKlPrepareIn(n_nodes=N, n_slots=S, slot_ptr=_ptr(slot_ptr), slot_src=_ptr(slot_src),
                                 is_edge=_ptr(is_edge), gnn=_ptr(gnn), truth=_ptr(truth), gnn_stride=int(gnn.shape[1]),
                                 with_single=int(bool(with_single)), layout=int(bool(ordered)), compact=int(bool(compact)),
                                 scale=float(scale) if scale is not None else 0.0)
        buf = nat.GtfKlPrepareBuf(_ptr(o_ptr), _ptr(o_src), _ptr(o_xy), _ptr(o_truth), _ptr(o_pair), _ptr(o_list),
                                  _ptr(o_node), _ptr(o_slot), _ptr(o_q), _ptr(o_t32))
        g, q, c = nat.GtfKlGraph(), nat.GtfKlQ32(), nat.GtfKlCounts()
        s = torch.cuda.current_stream(dev)
        rc = L.gtf_kl_prepare(ctypes.byref(pin), ctypes.byref(buf), ctypes.byref(g), ctypes.byref(q), ctypes.byref(c),
                              _ptr(ws), nb, ctypes.c_void_p(s.cuda_stream))
        if rc == -2 and c.error:
            _raise_prepare_error(c)
        nat.check(rc)
        self.n_nodes, self.n_slots, self.n_pairs, self.n_listed = N, int(c.n_kept), int(c.n_pairs), int(c.n_listed)
        self.tile = 0
        self.device = dev
        self.slot_ptr, self.slot_src, self.pair_ptr = o_ptr[:N + 1], o_src[:self.n_slots], o_pair[:N + 1]
        self.gnn = o_xy[:2 * N].reshape(N, 2)
        self.truth = o_truth[:N] if truth is not None else None
        self._node_of_dev = o_node[:N] if ordered else None
        self._slot_of_dev = o_slot[:self.n_slots] if ordered else None
        if ordered:
            self.lists = [torch.empty(0, dtype=torch.int32, device=dev) for _ in range(4)]   # (ranges, no lists)
            self._ranges = [int(c.n_d1), int(c.count[0] - c.n_d1)] + [int(x) for x in c.n_deg] + [int(c.count[3])]
            if os.environ.get("GTF_KL_DEG_RUNS", "1") == "0":   # (the round-3 ordered form, as the host constructor)
                g.deg_runs = 0
                for k in range(6):
                    g.n_deg[k] = 0
        else:
            at = np.concatenate([[0], np.cumsum([int(x) for x in c.count])])
            self.lists = [o_list[int(at[k]):int(at[k + 1])] for k in range(4)]
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.q = self.truth32 = self.scale = self._q = None
        if compact:
            self.q, self.scale = o_q[:2 * N].reshape(N, 2), float(c.scale)
            self.truth32 = o_t32[:N] if truth is not None else None
            self._q = q
        self._g = g
        self._keep = (o_ptr, o_src, o_xy, o_pair, o_truth, o_list, o_node, o_slot, o_q, o_t32)   # (the structs' targets)

    @classmethod
    def from_device(cls, slot_ptr, slot_src, gnn, truth=None, is_edge=None, with_single=False, ordered=False,
                    compact=False, scale=None):
        """The KL graph of arrays that are resident already (torch device tensors: slot_ptr int32
        [N + 1], slot_src int32 [S], gnn float64 [N, 2] or [N, 4], truth int64 [N], is_edge uint8 [S]
        marking the slots that are in-edges): gtf_kl_prepare on them, nothing is uploaded. What
        ParabolicKL(*in_edge_csr, ..., prepare="host") builds from their downloads, array for array."""
        k = cls.__new__(cls)
        k._prepare_device(slot_ptr, slot_src, gnn, truth, is_edge, with_single, ordered, compact, scale)
        return k

    @classmethod
    def from_device_graph(cls, d, truth=None, with_single=False, ordered=False, compact=False, scale=None):
        """from_device on a natural-layout gtf.device.DeviceGraph's own slot_ptr, slot_src, is_edge and
        gnn: one resident event (DeviceGraph.from_event) or the fused graph of a batch (from_events;
        events share no edge, so no pair spans two). What from_graph(d.host_graph()[0]) computes.
        truth: int64 [N], a host array (uploaded) or a device tensor."""
        if getattr(d, "mem", None) != "torch" or d.layout != "natural":
            raise ValueError("from_device_graph: a natural-layout DeviceGraph of torch tensors (mem='torch')")
        N, S = int(d.n_nodes), int(d.n_slots)
        if truth is not None and not torch.is_tensor(truth):
            truth = torch.from_numpy(np.ascontiguousarray(truth, np.int64).reshape(-1)).to(d.device)
        return cls.from_device(d.t["slot_ptr"].reshape(-1)[:N + 1], d.t["slot_src"].reshape(-1)[:S],
                               d.t["gnn"].reshape(-1)[:4 * N].reshape(N, 4), truth, d.t["is_edge"].reshape(-1)[:S],
                               with_single, ordered, compact, scale)

    def _node_of_device(self):
        """node_of as a device tensor (None: natural layout); a host-prepared object uploads it once"""
        if "_node_of_dev" not in self.__dict__:
            self._node_of_dev = (torch.from_numpy(np.ascontiguousarray(self.node_of, np.int64)).to(self.device)
                                 if self.node_of is not None else None)
        return self._node_of_dev

    def rows_dev(self, out):
        """The (node, i, j, emp_var) columns of the training rows as device tensors (gtf_kl_pair_rows):
        pair_index() and the emp_var[node] gather of training_rows_csr, from the buffers ``out`` of a
        run(); node in the caller's numbering. Stream-ordered."""
        P = self.n_pairs
        z = lambda dt: torch.empty(max(P, 1), dtype=dt, device=self.device)  # noqa: E731
        node, i, j = z(torch.int64), z(torch.int64), z(torch.int64)
        ev = out.get("emp_var")
        er = z(ev.dtype) if ev is not None else None
        s = torch.cuda.current_stream(self.device)
        nat.check(nat.lib().gtf_kl_pair_rows(ctypes.byref(self._g), P, _ptr(self._node_of_device()), _ptr(ev),
                                             nat.GTF_F64 if ev is None or ev.dtype == torch.float64 else nat.GTF_F32,
                                             _ptr(node), _ptr(i), _ptr(j), _ptr(er), ctypes.c_void_p(s.cuda_stream)))
        rows = {"node": node[:P], "i": i[:P], "j": j[:P]}
        if er is not None:
            rows["emp_var"] = er[:P]
        return rows

    def _block_table(self, d, pair_ptr, margin=WIN_MARGIN):   # (rank < 16: 10 keys)
        """gtf_kl_graph.blk of the tiled layout: one record of 12 int32 per tile (first node,
        bucket-0 count, its one-edge count, the three- and four-edge counts that follow (0 and
        0 unless tile_b1), 0, bucket 0's first slot, its first pair lo / hi, the window
        [lo, hi) -- the tile's nodes and `margin` nodes either side, at most WIN_NODES -- 0)"""
        tid, rank = self._tiles
        sp = self.slot_ptr_host
        n = tid.size
        nt = int(tid.max()) + 1 if n else 0
        bounds = np.searchsorted(tid, np.arange(nt + 1))
        a, b = bounds[:-1], bounds[1:]
        n1 = np.searchsorted(tid * 16 + rank, tid[a] * 16 + 1) - a if nt else a   # rank-0 run at the tile head
        n0 = np.searchsorted(tid * 16 + rank, tid[a] * 16 + 2) - a if nt else a
        z = np.zeros(nt, np.int64)
        n3 = n4 = z
        if self.tile_b1 and nt:
            n3 = np.searchsorted(tid * 16 + rank, tid[a] * 16 + 3) - a - n0
            n4 = np.searchsorted(tid * 16 + rank, tid[a] * 16 + 4) - a - n0 - n3
        pr = pair_ptr[a]   # (one-edge nodes have no pairs: the first two-edge node's, then the 3- / 4-edge nodes')
        span = b - a
        m = np.clip((WIN_NODES - span) // 2, 0, margin)
        wlo = np.maximum(a - m, 0)
        whi = np.minimum(np.minimum(b + m, n), wlo + WIN_NODES)
        # one thread per node of the tile's bucket 0 and its in-tile 3- / 4-edge nodes: a
        # 256-thread block (gtf_kl.hip) would skip any beyond 256 without an error
        if nt and int((n0 + n3 + n4).max()) > 256:
            raise ValueError("KL tile with %d one- to four-edge nodes (the block handles at most 256)"
                             % int((n0 + n3 + n4).max()))
        recs = np.stack([a, n0, n1, n3, n4, z, sp[a], pr & 0xFFFFFFFF, pr >> 32, wlo, whi, z], 1)
        recs = np.where(recs >= 2**31, recs - 2**32, recs)   # low words as int32 bits
        return recs.astype(np.int32).reshape(-1)

    def replica(self, gnn=None):
        """An independent copy of this batch in its own device buffers (same structure):
        ``gnn`` (caller's node order, [N, 4] or [N, 2]) replaces the coordinates, e.g. a
        batch jittered with another seed. Used to rotate launches over several resident
        batches so that no launch finds its inputs in the caches (bench.py, config 5)."""
        import copy
        r = copy.copy(self)
        cl = lambda t: t.clone() if t is not None else None  # noqa: E731
        r.slot_ptr, r.slot_src, r.pair_ptr = cl(self.slot_ptr), cl(self.slot_src), cl(self.pair_ptr)
        r.truth = cl(self.truth)
        r.lists = [cl(x) for x in self.lists]
        if getattr(self, "blk", None) is not None:
            r.blk = cl(self.blk)
        r.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        if gnn is None:
            r.gnn = cl(self.gnn)
        elif torch.is_tensor(gnn):   # resident coordinates: gtf_kl_coords permutes and quantises them there
            if (gnn.dtype != torch.float64 or gnn.device != self.gnn.device or not gnn.is_contiguous() or gnn.dim() != 2
                    or gnn.shape[0] != self.n_nodes or gnn.shape[1] not in (2, 4)):
                raise ValueError("replica: gnn as a tensor is a contiguous float64 [N, 2] or [N, 4] on %s" % self.device)
            N = self.n_nodes
            r.gnn = torch.empty(max(2 * N, 1), dtype=torch.float64, device=self.device)[:2 * N].reshape(N, 2)
            if self.q is not None:
                r.truth32 = cl(self.truth32)
                r.q = torch.empty(max(2 * N, 1), dtype=torch.int32, device=self.device)[:2 * N].reshape(N, 2)
            s = torch.cuda.current_stream(self.device)
            nat.check(nat.lib().gtf_kl_coords(N, _ptr(gnn), int(gnn.shape[1]), _ptr(self._node_of_device()), _ptr(r.gnn),
                                              _ptr(r.q) if self.q is not None else None,
                                              self.scale if self.q is not None else 0.0, _ptr(r.err),
                                              ctypes.c_void_p(s.cuda_stream)))
            e = int(r.err.item())
            if e:
                r.err.zero_()
                _raise_prepare_error(e)
            if self.q is not None:
                r._q = nat.GtfKlQ32(_ptr(r.q), r.scale, _ptr(r.truth32))
        else:
            gh = np.asarray(gnn, np.float64)[:, :2]
            if self.node_of is not None:
                gh = gh[self.node_of]
            r.gnn = torch.from_numpy(np.ascontiguousarray(gh)).to(self.device)
        if self.q is not None and not torch.is_tensor(gnn):   # the compact copy: re-quantised with the parent's scale
            r.truth32 = cl(self.truth32)
            if gnn is None:
                r.q = cl(self.q)
                r._q = nat.GtfKlQ32(_ptr(r.q), r.scale, _ptr(r.truth32))
            else:
                r._set_compact(gh, None, self.scale)
        g = nat.GtfKlGraph.from_buffer_copy(self._g)
        g.slot_ptr, g.slot_src, g.gnn = _ptr(r.slot_ptr), _ptr(r.slot_src), _ptr(r.gnn)
        g.truth, g.pair_ptr = _ptr(r.truth), _ptr(r.pair_ptr)
        if getattr(r, "blk", None) is not None:
            g.blk = _ptr(r.blk)
        for q in range(4):
            if g.list[q]:
                g.list[q] = r.lists[q].data_ptr() if r.lists[q].numel() else None
        r._g = g
        return r

    def footprint_bytes(self, out, dtype=None) -> int:
        """device bytes of this batch's inputs and the outputs in ``out``: of the coordinate
        and truth arrays, those the path of ``dtype`` touches ("q32": the fixed-point copy and
        the int32 ids; default: the fp64 rows and int64 ids)"""
        coords = [self.q, self.truth32] if dtype == "q32" else [self.gnn, self.truth]
        ts = [self.slot_ptr, self.slot_src, self.pair_ptr] + coords + list(self.lists)
        ts += [v for k, v in out.items() if k not in ("kl", "truth")]   # (views of _kl / _truth)
        seen, tot = set(), 0
        for t in ts:
            if t is None or t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            tot += t.numel() * t.element_size()
        return tot

    @classmethod
    def from_graph(cls, g: TrackGraph, truth=None, device="cuda", with_single=False):
        ptr, src = in_edge_csr(g)
        return cls(ptr, src, g.node["gnn"], truth, device, with_single)

    def alloc(self, dtype="f64", truth=True, emp=True, states=False):
        if dtype not in ("f64", "f32", "q32"):
            raise ValueError("dtype must be 'f64', 'f32' or 'q32'")
        if dtype == "q32" and states:
            raise ValueError("the q32 path has no sv / cov outputs (full states are fp64: dtype='f64')")
        f = torch.float64 if dtype == "f64" else torch.float32
        fm = torch.float32 if dtype == "q32" else torch.float64   # the gradient moments
        # pair buffers hold >= 1 element so their pointers are never null, even with no
        # pairs (the C-ABI rejects null outputs); "kl"/"truth" are views of the pair count
        z = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=self.device)  # noqa: E731
        out = {"_kl": z(self.n_pairs, f)}
        out["kl"] = out["_kl"][:self.n_pairs]
        if truth and self.truth is not None:
            out["_truth"] = z(self.n_pairs, torch.int8)
            out["truth"] = out["_truth"][:self.n_pairs]
        if emp:     # True: gradient mean and variance; "var": variance only (the training rows)
            out["emp_var"] = torch.full((self.n_nodes,), float("nan"), dtype=fm, device=self.device)
            if emp is True:
                out["emp_mean"] = torch.full((self.n_nodes,), float("nan"), dtype=fm, device=self.device)
        if states:
            out["sv"] = torch.full((self.n_slots, 3), float("nan"), dtype=torch.float64, device=self.device)
            out["cov"] = torch.full((self.n_slots, 3, 3), float("nan"), dtype=torch.float64, device=self.device)
        return out

    def run(self, out, dtype="f64", stream=None):
        """launch gtf_parabolic_kl -- dtype "q32": gtf_parabolic_kl_q32 -- into the buffers of
        ``alloc`` for the same dtype (stream-ordered)."""
        if dtype == "q32":
            if self._q is None:
                raise ValueError("run(out, 'q32') needs ParabolicKL(..., compact=True)")
            if out["_kl"].dtype != torch.float32 or "sv" in out or any(
                    k in out and out[k].dtype != torch.float32 for k in ("emp_var", "emp_mean")):
                raise ValueError("run(out, 'q32') needs the buffers of alloc('q32')")
            o = nat.GtfKlOut32(_ptr(out["_kl"]), _ptr(out.get("_truth")), _ptr(out.get("emp_var")),
                               _ptr(out.get("emp_mean")), _ptr(self.err))
            s = stream if stream is not None else torch.cuda.current_stream(self.device)
            nat.check(nat.lib().gtf_parabolic_kl_q32(ctypes.byref(self._g), ctypes.byref(self._q), ctypes.byref(o),
                                                     ctypes.c_void_p(s.cuda_stream)))
            return out
        o = nat.GtfKlOut(_ptr(out["_kl"]), _ptr(out.get("_truth")), _ptr(out.get("emp_var")),
                         _ptr(out.get("emp_mean")), _ptr(out.get("sv")), _ptr(out.get("cov")), _ptr(self.err))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        nat.check(nat.lib().gtf_parabolic_kl(ctypes.byref(self._g), nat.GTF_F64 if dtype == "f64" else nat.GTF_F32,
                                             ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)))
        return out

    def errors(self):
        return int(self.err.item())

    def pair_index(self, device_nodes=False):
        """(node, i, j) of every pair row (host); node in the caller's numbering unless
        device_nodes (the ordered layout's own)."""
        d = self.degree
        nodes = np.nonzero(d >= 2)[0]
        node = np.repeat(nodes, (d[nodes] * (d[nodes] - 1) // 2))
        t = np.arange(self.n_pairs, dtype=np.int64) - self.pair_ptr_host[node]
        i = np.floor((1 + np.sqrt(1 + 8 * t.astype(np.float64))) / 2).astype(np.int64)
        i -= (i * (i - 1) // 2 > t)
        i += ((i + 1) * i // 2 <= t)
        if self.node_of is not None and not device_nodes:
            node = self.node_of[node]
        return node, i, t - i * (i - 1) // 2

    def host_nodes(self, a):
        """a per-node device output (array, first axis = node) in the caller's node order"""
        a = np.asarray(a)
        if self.node_of is None:
            return a
        out = np.empty_like(a)
        out[self.node_of] = a
        return out

    def host_slots(self, a):
        """a per-slot device output in the caller's slot order"""
        a = np.asarray(a)
        if self.slot_of is None:
            return a
        out = np.empty_like(a)
        out[self.slot_of] = a
        return out


def training_rows(g: TrackGraph, truth=None, dtype="f64", device="cuda", prepare="host"):
    """(node, i, j, kl_dist, emp_var, truth) rows of extract_metadata_trackml_parabolic_model.py
    for one event graph, computed on the GPU (dtype "f64", "f32" or the compact "q32").
    prepare "device": as training_rows_csr."""
    ptr, src = in_edge_csr(g)
    return training_rows_csr(ptr, src, g.node["gnn"], truth, dtype, device, prepare)


def training_rows_csr(slot_ptr, slot_src, gnn, truth=None, dtype="f64", device="cuda", prepare="host"):
    """prepare "device": the graph is built by gtf_kl_prepare and the node, i, j and emp_var columns by
    gtf_kl_pair_rows (ParabolicKL.rows_dev); the same six host arrays."""
    k = ParabolicKL(slot_ptr, slot_src, gnn, truth, device, compact=dtype == "q32", prepare=prepare)
    out = k.run(k.alloc(dtype, truth=truth is not None, emp="var"), dtype)
    if prepare == "device":
        rows = k.rows_dev(out)
        node, i, j, ev = (rows[c].cpu().numpy() for c in ("node", "i", "j", "emp_var"))
    else:
        node, i, j = k.pair_index()
        ev = out["emp_var"].cpu().numpy()[node]
    tr = out["truth"].cpu().numpy() if "truth" in out else np.zeros(k.n_pairs, np.int8)
    flags = k.errors()
    if flags:
        raise np.linalg.LinAlgError(nat.ERR_FLAGS[128])
    return node, i, j, out["kl"].cpu().numpy(), ev, tr


def compute_track_state_estimates(g: TrackGraph, device="cuda"):
    """Per in-edge parabolic states and per-node gradient (mean, var) of one graph
    (utils.py:221-289): returns (sv [S,3], cov [S,3,3], grad_mean [N], grad_var [N]),
    slots in the graph's in-edge order."""
    k = ParabolicKL.from_graph(g, None, device, with_single=True)
    out = k.run(k.alloc("f64", truth=False, emp=True, states=True), "f64")
    if k.errors():
        raise np.linalg.LinAlgError(nat.ERR_FLAGS[128])
    return (out["sv"].cpu().numpy(), out["cov"].cpu().numpy(), out["emp_mean"].cpu().numpy(),
            out["emp_var"].cpu().numpy())


def batch(slot_ptr, slot_src, gnn, truth, n_events, jitter=1e-3, seed=0):
    """n_events copies of one event concatenated into one CSR (the config-5 batch):
    copy e > 0 has every hit moved by a seeded N(0, jitter) mm in x and y, so the
    events differ. Truth ids repeat per copy (pairs never span copies)."""
    rng = np.random.default_rng(seed)
    n, s = gnn.shape[0], slot_src.shape[0]
    ptrs = [np.asarray(slot_ptr[:-1], np.int64) + e * s for e in range(n_events)] + [np.array([n_events * s])]
    src = np.concatenate([np.asarray(slot_src, np.int64) + e * n for e in range(n_events)])
    g = np.tile(np.asarray(gnn, np.float64), (n_events, 1))
    g[n:, :2] += rng.normal(0.0, jitter, (g.shape[0] - n, 2))
    tr = np.tile(np.asarray(truth, np.int64), n_events) if truth is not None else None
    return np.concatenate(ptrs).astype(np.int32), src.astype(np.int32), g, tr
