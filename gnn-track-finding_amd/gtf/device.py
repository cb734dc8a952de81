"""Device-resident TrackGraph and the stage entry points (host side of the C-ABI).

``DeviceGraph`` uploads a :class:`gtf.graph.TrackGraph` into HBM once (torch
tensors are used only as device allocations; every computation runs in
libgtf.so's HIP kernels), then the stage methods call the C-ABI on the current
HIP stream. ``download`` copies the mutable arrays back for unpacking.

Stage methods mirror the reference's stage bodies:
  extrapolate() -> src/extrapolate/extrapolate_merged_states.py:552-566
  update()      -> src/update/remove_state_metadata.py:29-53
  cluster()     -> src/clustering/clustering.py:181-373
  full_pass()   -> the three in run_gnn_trackml_mod.sh order (extrapolate,
                   update, cluster on updated_track_states), fused
  tag_propagation() -> tag_propagation/tag_propagation.py:97-164
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat
from .graph import BUCKETS, TrackGraph, NODE_FIELDS, SLOT_FIELDS, padded, renumber
from .params import Params

STATIC_SLOT = ("slot_src", "is_edge", "rev_edge", "send_mw")
MUTABLE_NODE = ("has_merged", "merged_state", "merged_cov", "merged_prior", "has_tse", "has_uts", "degree")
STATE_FIELDS = ("rank", "sv", "tau", "cov", "xyzr", "lik", "mw", "prior", "lr", "side", "fresh")


def sched_segments(slot_ptr, sched):
    """gtf_graph.sched_seg: (slot_ptr[v], slot_ptr[v + 1]) of every schedule entry v"""
    sp = np.asarray(slot_ptr, dtype=np.int64)
    v = np.asarray(sched, dtype=np.int64)
    return np.stack([sp[v], sp[v + 1]], axis=1).astype(np.int32).reshape(-1)


def sender_schedule(out_ptr, nodes=None):
    """gtf_graph.out_sched: (sender, out begin, out end, 0) of every node with an
    out-edge (or of the given nodes: a shard's senders), bucketed by out-degree 1..4 /
    5..8 / more; returns (array, counts)"""
    op = np.asarray(out_ptr, dtype=np.int64)
    idx = np.arange(op.size - 1, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
    od = op[idx + 1] - op[idx]
    parts = [idx[(od >= 1) & (od <= 4)], idx[(od >= 5) & (od <= 8)], idx[od > 8]]
    u = np.concatenate(parts).astype(np.int64)
    q = np.stack([u, op[u], op[u + 1], np.zeros_like(u)], axis=1).astype(np.int32).reshape(-1)
    return q, [int(x.size) for x in parts]


def sender_lanes(out_slot, out_dst, q, counts):
    """gtf_graph.out_lanes: for every lane of the 4- and 8-lane entries of the sender
    schedule `q` (sender_schedule), (slot, receiver) of the lane's out-edge or (-1, 0)"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 4)
    os_ = np.asarray(out_slot, dtype=np.int64)
    od = np.asarray(out_dst, dtype=np.int64)
    parts, at = [], 0
    for G, n in ((4, counts[0]), (8, counts[1])):
        e = q[at:at + n]
        at += n
        idx = e[:, 1:2] + np.arange(G)[None, :]
        ok = idx < e[:, 2:3]
        safe = np.minimum(idx, max(os_.size - 1, 0))
        k = np.where(ok, os_[safe] if os_.size else -1, -1)
        v = np.where(ok, od[safe] if od.size else 0, 0)
        parts.append(np.stack([k, v], axis=2).reshape(-1))
    return np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)


def pack_schedule(slot_ptr):
    """gtf_graph.pack_ent / pack_wave: the nodes with <= 64 slots, largest first, packed
    greedily into wavefronts of 64 lanes (one lane per slot, one for a slot-free node);
    returns (entries [4*n] int32 (v, lo, hi, first lane), wave_ptr [W+1] int32)"""
    sp = np.asarray(slot_ptr, dtype=np.int64)
    deg = np.diff(sp)
    idx = np.nonzero(deg <= 64)[0]
    order = idx[np.argsort(-deg[idx], kind="stable")]
    size = np.maximum(deg[order], 1)
    off = np.empty(order.size, np.int64)
    starts = [0]
    used = 0
    for i, z in enumerate(size.tolist()):
        if used + z > 64:
            starts.append(i)
            used = 0
        off[i] = used
        used += z
    starts.append(order.size)
    ent = np.stack([order, sp[order], sp[order + 1], off], axis=1).astype(np.int32).reshape(-1)
    wave = np.asarray(starts if order.size else [0], dtype=np.int32)
    return ent, wave


CLASS_MAX = 32   # segments of up to this many slots get graph-static classes (gtf_graph.slot_class)
XCLASS_MAX = 64  # 33..64-slot segments: the layer classes in slot_class, the x ones in slot_xclass (ABI v7)
CLASS_MIN_SLOTS = 1 << 16   # graphs this large get them by default (the host pass: ~4 ms on 15k slots)


def slot_classes(g: TrackGraph):
    """gtf_graph.slot_class / slot_sflags (ABI v5) / slot_xclass (v7): for every slot of a receiver segment of
    d <= 32 slots, bits 0..31 = the segment positions whose sender has this slot's sender
    layer (compute_prior_probabilities' groups, helper.py:30-63), bits 32..63 = the positions
    whose sender's GNN x equals this slot's sender's (the side norm's distinct-x classes,
    helper.py:111-139, for entries holding their sender's live coordinates); a NaN (orphan
    key) equals only itself. sflags bit 0 = sender GNN x < receiver GNN x (the side,
    helper.py:116-121). Segments of 33..64 slots (v7): all 64 bits of slot_class are the
    layer positions and slot_xclass holds the x positions. Larger segments get 0 (the kernel
    builds their classes)."""
    S = g.n_slots
    cls = np.zeros(S, np.uint64)
    src = g.slot["slot_src"].astype(np.int64)
    ok = src >= 0
    layer = np.full(S, np.nan)
    sx = np.full(S, np.nan)
    if g.n_nodes:
        layer[ok] = g.node["layer"][src[ok]]
        sx[ok] = g.node["gnn"][src[ok], 0]
    rx = g.node["gnn"][g.slot_dst(), 0] if S else np.zeros(0)
    with np.errstate(invalid="ignore"):
        sfl = (sx < rx).astype(np.uint8)
    sp = g.slot_ptr.astype(np.int64)
    deg = np.diff(sp)
    xcls = np.zeros(S, np.uint64)
    for d in range(1, XCLASS_MAX + 1):
        v = np.nonzero(deg == d)[0]
        if v.size == 0:
            continue
        idx = sp[v][:, None] + np.arange(d)[None, :]                 # [n, d] slots
        own = np.eye(d, dtype=bool)[None, :, :]
        bits = (np.uint64(1) << np.arange(d, dtype=np.uint64))[None, None, :]
        masks = []
        for val in (layer, sx):
            a = val[idx]
            eq = (a[:, :, None] == a[:, None, :]) | own              # [n, i, j]
            masks.append(np.bitwise_or.reduce(np.where(eq, bits, np.uint64(0)), axis=2))
        if d <= CLASS_MAX:   # both in one word
            cls[idx.reshape(-1)] = (masks[0] | (masks[1] << np.uint64(32))).reshape(-1)
        else:                # 33..64 slots: the layer positions in slot_class, the x ones in slot_xclass
            cls[idx.reshape(-1)] = masks[0].reshape(-1)
            xcls[idx.reshape(-1)] = masks[1].reshape(-1)
    return cls, sfl, xcls


STATIC_MAX = 8   # segments of up to this many slots get gtf_graph.slot_static words


def slot_static_words(g: TrackGraph, cls: np.ndarray, sfl: np.ndarray) -> np.ndarray:
    """gtf_graph.slot_static (ABI v7): for a slot of a segment of d <= 8 slots, its class bits
    (same layer: bits 0..7, same x: bits 8..15), is_edge (16), rev_edge (17) and side flag
    (18) in one uint32; 0 for larger segments"""
    deg = np.diff(g.slot_ptr.astype(np.int64))
    small = np.repeat(deg <= STATIC_MAX, deg)
    c = cls.astype(np.uint64)
    w = (c & np.uint64(0xff)) | (((c >> np.uint64(32)) & np.uint64(0xff)) << np.uint64(8))
    w = w.astype(np.uint32)
    w |= (g.slot["is_edge"].astype(np.uint32) & 1) << 16
    w |= (g.slot["rev_edge"].astype(np.uint32) & 1) << 17
    w |= (sfl.astype(np.uint32) & 1) << 18
    return np.where(small, w, np.uint32(0)).astype(np.uint32)


def slot_sender_xzr(g: TrackGraph) -> np.ndarray:
    """gtf_graph.slot_sxzr (ABI v7): per slot its sender's GNN_Measurement x, z, r
    (gnn[slot_src][0, 2, 3]), NaN rows for orphan keys; [S, 3] float64"""
    src = g.slot["slot_src"].astype(np.int64)
    out = np.full((g.n_slots, 3), np.nan)
    ok = src >= 0
    if g.n_nodes and ok.any():
        out[ok] = g.node["gnn"][src[ok]][:, [0, 2, 3]]
    return out


def live_coordinates(g: TrackGraph) -> np.ndarray:
    """gtf_states.fresh bit 1 for an uploaded graph: the updated_track_states entries whose
    stored 'xyzr' is bit for bit their sender's current GNN_Measurement coordinates (what
    extrapolate_merged_states.py:377 stores; a close-proximity merge of the sender since,
    extract_track_candidates.py:111-118, breaks it). Those entries' xyzr is read from gnn."""
    src = g.slot["slot_src"].astype(np.int64)
    ok = (src >= 0) & (g.slot["uts_rank"] >= 0)
    live = np.zeros(g.n_slots, bool)
    if ok.any():
        a = np.ascontiguousarray(g.slot["uts_xyzr"][ok]).view(np.int64)
        b = np.ascontiguousarray(g.node["gnn"][src[ok]]).view(np.int64)
        live[ok] = (a == b).all(axis=1)
    return live


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("gtf needs a HIP device (MI355X); torch.cuda.is_available() is False")
    return torch


def schedule_order(slot_ptr, tile=0):
    """node indices bucketed by slot count as the node-kernel schedule takes them
    (BUCKETS, then the nodes beyond 64 slots), node order inside a bucket. tile > 0:
    the same inside every run of `tile` consecutive nodes, tile after tile, so a bucket's
    nodes stay contiguous within a tile and spatially close nodes stay close"""
    deg = np.diff(np.asarray(slot_ptr, dtype=np.int64))
    idx = np.arange(deg.size, dtype=np.int64)
    bucket = np.full(deg.size, len(BUCKETS), np.int64)
    for q, (lo, hi) in reversed(list(enumerate(BUCKETS))):
        bucket[(deg >= lo) & (deg <= hi)] = q
    t = idx // tile if tile > 0 else np.zeros_like(idx)
    return np.lexsort((idx, bucket, t))


def node_schedule(slot_ptr):
    """(sched, bucket sizes [n_g4, n_g8, n_g16, n_g32, n_g64], n_big, (n_g2, n_g6, n_g12)): the
    slot-count-bucketed node schedule of the node-local kernels (gtf_graph.sched: G lanes per
    node), node order inside a bucket except that the nodes of a narrower lane group come
    first -- the <= 2-slot nodes in the <= 4-slot bucket (2 lanes, n_g2), the <= 6-slot ones
    in the <= 8-slot bucket (6 lanes, n_g6) and the <= 12-slot ones in the <= 16-slot bucket
    (12 lanes, n_g12); then the nodes beyond 64 slots (one thread each)"""
    deg = np.diff(np.asarray(slot_ptr, dtype=np.int64))
    idx = np.arange(deg.size, dtype=np.int32)
    buckets = [idx[(deg >= lo) & (deg <= hi)] for lo, hi in BUCKETS]
    sub = []
    for q, narrow in ((0, 2), (1, 6), (2, 12)):
        first = deg[buckets[q]] <= narrow
        buckets[q] = np.concatenate([buckets[q][first], buckets[q][~first]])
        sub.append(int(first.sum()))
    rest = idx[deg > 64]
    sched = np.concatenate(buckets + [rest]).astype(np.int32)
    return sched, [int(b.size) for b in buckets], int(rest.size), tuple(sub)


TILE = 4096   # nodes per tile of the "tiled" layout


class DeviceGraph:
    """pack: the fused pass's node kernel on packed variable-size lane segments
    (gtf_graph.pack_ent) instead of power-of-two lane groups -- same results, same speed
    on C4, kept as an option.
    layout "natural": the host graph's node and slot order. layout "schedule": nodes
    renumbered into schedule order (graph.renumber), so the lane groups of one
    wavefront take adjacent slot segments and every slot load of the node kernel is
    one contiguous run; download() maps the results back to the host order. The
    stage methods are layout-independent (the pass is equivariant under renumber)."""

    def __init__(self, g: TrackGraph, device: str = "cuda", schedule: bool = True, layout: str = "natural",
                 pack: bool = False, tile: int = TILE, mem: str = "torch", classes=None, tables: str = "host"):
        """mem "torch": the arrays are torch tensors (every method). mem "hip": plain
        allocations from libgtf (gtf.devmem, no torch in the process): the stage methods,
        clear_errors / errors and download only -- the drop-in CLIs' path. classes: upload
        the graph-static slot classes (gtf_graph.slot_class); None = on graphs of at least
        CLASS_MIN_SLOTS slots. tables "host": the schedules and slot tables are built by the NumPy
        builders of this module and uploaded. tables "device": only the base arrays are uploaded
        and gtf_graph_prepare (include/gtf.h) builds the same tables on the GPU, from the
        (possibly renumbered) graph; classes=None then means on (the host cost behind
        CLASS_MIN_SLOTS is gone). Not with layout "padded" or pack=True."""
        if mem not in ("torch", "hip"):
            raise ValueError("mem must be 'torch' or 'hip'")
        if tables not in ("host", "device"):
            raise ValueError("tables must be 'host' or 'device'")
        if tables == "device" and (layout == "padded" or pack):
            raise ValueError("tables='device' builds neither the padded layout nor the packed schedule: "
                             "use tables='host' with layout='padded' or pack=True")
        self.mem = mem
        torch = _torch() if mem == "torch" else None
        self.layout = layout
        self.order = self.slot_perm = None
        self.pad_plan = None
        if layout in ("schedule", "tiled"):
            self.order = schedule_order(g.slot_ptr, tile if layout == "tiled" else 0)
            g, self.slot_perm = renumber(g, self.order)
        elif layout == "padded":   # padded tiles (graph.padded): dummy nodes / padding slots map to -1
            g, self.order, self.slot_perm, self.pad_plan = padded(g, tile)
        elif layout != "natural":
            raise ValueError("layout must be 'natural', 'schedule', 'tiled' or 'padded'")
        self.slot_ptr_host = g.slot_ptr
        self._node_id_host = g.node["node_id"]   # uploaded on first need (node_id_dev)
        self.torch = torch
        if torch is not None:
            self.device = torch.device(device)
            self.lib = nat.lib()
        else:
            self.device = device
            self.lib = nat.lib(lean=True)
            nat.check(self.lib.gtf_device_init(int(device.split(":")[1]) if ":" in device else 0))
        self.n_nodes, self.n_slots, self.n_edges = g.n_nodes, g.n_slots, g.n_edges
        self.t = {}
        up = self._up
        up("slot_ptr", g.slot_ptr.astype(np.int32))
        up("out_ptr", g.out_ptr.astype(np.int32))
        up("out_slot", g.out_slot.astype(np.int32))
        # tables "device": gtf_graph_prepare builds them (a graph without nodes, or without
        # slots and edges, has nothing to build there: its few tables come from the host)
        self.tables = tables
        dev_tables = tables == "device" and g.n_nodes > 0 and (g.n_slots > 0 or g.n_edges > 0)
        if dev_tables:
            self._upload_rest(g, pack)
            self._device_tables(g, classes, schedule)
            self._finish(g, pack)
            return
        self._host_tables(g, classes, schedule, pack)
        self._upload_rest(g, pack)
        self._finish(g, pack)

    def _host_tables(self, g: TrackGraph, classes, schedule, pack):
        """tables "host": the schedules and slot tables from the NumPy builders of this module"""
        up = self._up
        up("slot_dst", g.slot_dst().astype(np.int32))
        out_dst = g.slot_dst()[g.out_slot].astype(np.int32) if g.n_edges else np.zeros(0, np.int32)
        up("out_dst", out_dst)
        src = g.slot["slot_src"].astype(np.int64)
        up("slot_layer", np.where(src >= 0, g.node["layer"][np.maximum(src, 0)] if g.n_nodes else np.nan,
                                  np.nan).astype(np.float64))
        outpos = np.full(g.n_slots, -1, np.int32)
        if g.n_edges:
            owner = np.repeat(np.arange(g.n_nodes, dtype=np.int64), np.diff(g.out_ptr.astype(np.int64)))
            outpos[g.out_slot] = (np.arange(g.n_edges) - g.out_ptr[owner]).astype(np.int32)
        up("slot_outpos", outpos)
        # global out-edge index of every slot's edge (gtf_graph.slot_outidx): the sender scan
        # stores its running values in out-edge order (GTF_NO_OUTIDX=1: by slot, for A/B)
        import os
        self.use_outidx = os.environ.get("GTF_NO_OUTIDX", "0") != "1"
        # graph-static slot classes for the node kernel on graphs of >= CLASS_MIN_SLOTS slots
        # (smaller ones -- a drop-in stage's directory -- have the kernel build them: the host
        # pass would cost more than it saves); classes=True / False forces either way,
        # GTF_NO_CLASSES=1 turns them off (A/B)
        self.use_classes = (classes if classes is not None else g.n_slots >= CLASS_MIN_SLOTS) and \
            os.environ.get("GTF_NO_CLASSES", "0") != "1"
        oidx = np.full(g.n_slots, -1, np.int32)
        if g.n_edges:
            oidx[g.out_slot] = np.arange(g.n_edges, dtype=np.int32)
        up("slot_outidx", oidx)
        if self.use_classes:
            cls, sfl, xcls = slot_classes(g)
            up("slot_class", cls.view(np.int64))
            up("slot_sflags", sfl)
            up("slot_xclass", xcls.view(np.int64))
        # the senders' GNN x, z, r per slot (gtf_graph.slot_sxzr): a live UTS entry's stored
        # coordinates, read contiguously by the clustering instead of gathered per state
        # (GTF_NO_SXZR=1: gathered, for A/B)
        self.use_sxzr = self.use_classes and os.environ.get("GTF_NO_SXZR", "0") != "1"
        if self.use_sxzr:
            up("slot_sxzr", slot_sender_xzr(g))
        # the static slot fields of <= 8-slot segments in one word (gtf_graph.slot_static;
        # GTF_NO_STATIC32=1: the separate arrays, for A/B)
        self.use_static32 = self.use_classes and os.environ.get("GTF_NO_STATIC32", "0") != "1"
        if self.use_static32:
            up("slot_static", slot_static_words(g, cls, sfl).view(np.int32))
        sub = g.node["sub_id"].astype(np.int64)
        if g.n_nodes:
            sizes = np.bincount(sub - sub.min())
            solo = (sizes[sub - sub.min()] == 1).astype(np.uint8)
        else:
            solo = np.zeros(0, np.uint8)
        up("solo", solo)
        # slot-count-bucketed node schedule for the node-local kernels (G lanes per node)
        sched, self.n_g_all, self.n_big, sub = node_schedule(g.slot_ptr)
        self.n_g2, self.n_g6, self.n_g12 = sub
        up("sched", sched)
        up("sched_seg", sched_segments(g.slot_ptr, sched))
        osched, self.n_o = sender_schedule(g.out_ptr)
        up("out_sched", osched)
        up("out_lanes", sender_lanes(g.out_slot, out_dst, osched, self.n_o))
        self.n_pack_waves = 0
        if pack:   # the packed lane segments are built only when asked for
            pent, pwave = pack_schedule(g.slot_ptr)
            up("pack_ent", pent)
            up("pack_wave", pwave)
            self.n_pack_waves = int(pwave.size - 1)
        self.n_g = self.n_g_all if schedule else [0] * len(BUCKETS)
        self.use_sched = schedule

    def _upload_rest(self, g: TrackGraph, pack):
        """solo and the node and slot arrays of the graph (no schedule, no slot table)"""
        up = self._up
        if "solo" not in self.t:
            sub = g.node["sub_id"].astype(np.int64)
            if g.n_nodes:
                sizes = np.bincount(sub - sub.min())
                solo = (sizes[sub - sub.min()] == 1).astype(np.uint8)
            else:
                solo = np.zeros(0, np.uint8)
            up("solo", solo)
        # the subgraph ids, for subset(): every value in [0, n_sub)
        sub = g.node["sub_id"].astype(np.int32)
        self.n_sub = max(int(g.n_subgraphs), int(sub.max()) + 1 if sub.size else 0, 0)
        self._sub_ok = not sub.size or int(sub.min()) >= 0
        up("sub_id", sub)
        for f in ("gnn", "xyzr", "layer") + MUTABLE_NODE:
            up(f, g.node[f])
        for f in SLOT_FIELDS:
            if f in ("slot_key",):
                continue
            if f == "uts_fresh":   # bit 0: fresh; bit 1: the entry's xyzr is its sender's live gnn
                up(f, ((g.slot[f] != 0).astype(np.uint8) | (live_coordinates(g).astype(np.uint8) << 1)))
                continue
            up(f, g.slot[f])

    def _finish(self, g: TrackGraph, pack):
        """the arena, the workspace and the C structs"""
        torch = self.torch
        self._staged, self._resident = [], None   # stage_inputs() copies
        ws_bytes = int(self.lib.gtf_workspace_bytes(g.n_nodes, g.n_slots))
        if torch is not None:
            self._make_arena(self.PASS_INPUTS)
            self.t["ws"] = torch.zeros(ws_bytes, dtype=torch.uint8, device=self.device)
        else:   # (no arena: snapshots and staged inputs are benchmark tools, torch only)
            from .devmem import HipArray
            self.arena = None
            self.t["ws"] = HipArray.zeros(ws_bytes, np.uint8)
            nat.check(self.lib.gtf_stream_synchronize(None))   # the uploads' host buffers may go
            for t in self.t.values():
                t._pending = None
        self._build_structs(pack)

    def _device_tables(self, g: TrackGraph, classes, schedule):
        """tables "device": allocate the schedules and slot tables, have gtf_graph_prepare fill
        them from the uploaded base arrays, and take the bucket counts from the struct it filled"""
        import os
        N, S, E = g.n_nodes, g.n_slots, g.n_edges
        self.use_outidx = os.environ.get("GTF_NO_OUTIDX", "0") != "1"
        self.use_classes = (classes if classes is not None else True) and os.environ.get("GTF_NO_CLASSES", "0") != "1"
        self.use_sxzr = self.use_classes and os.environ.get("GTF_NO_SXZR", "0") != "1"
        self.use_static32 = self.use_classes and os.environ.get("GTF_NO_STATIC32", "0") != "1"
        want = [("slot_dst", S, np.int32), ("out_dst", E, np.int32), ("slot_layer", S, np.float64),
                ("slot_outpos", S, np.int32), ("slot_outidx", S, np.int32), ("sched", N, np.int32),
                ("sched_seg", 2 * N, np.int32), ("out_sched", 4 * N, np.int32), ("out_lanes", 16 * N, np.int32)]
        if self.use_classes:
            want += [("slot_class", S, np.int64), ("slot_sflags", S, np.uint8), ("slot_xclass", S, np.int64)]
        if self.use_sxzr:
            want.append(("slot_sxzr", 3 * S, np.float64))
        if self.use_static32:
            want.append(("slot_static", S, np.int32))
        for name, n, dt in want:
            self.t[name] = self._dev_empty(n, dt)
        ws = self._dev_empty(int(self.lib.gtf_graph_prepare_workspace_bytes(N, S, E)), np.uint8)
        p = self.ptr
        cg = nat.GtfGraph(n_nodes=N, n_slots=S, n_edges=E, slot_ptr=p("slot_ptr"), slot_src=p("slot_src"),
                          out_ptr=p("out_ptr"), out_slot=p("out_slot"), is_edge=p("is_edge"), rev_edge=p("rev_edge"),
                          gnn=p("gnn"), layer=p("layer"))
        tb = nat.GtfGraphTables(**{name: p(name) for name, _, _ in want})
        nat.check(self.lib.gtf_graph_prepare(ctypes.byref(cg), ctypes.byref(tb), ctypes.c_void_p(ws.data_ptr()),
                                             ctypes.c_size_t(ws.numel()), self.stream))
        # the slot and out-edge kernels are still in flight and the workspace goes out of scope
        # here: a torch allocation is reused in stream order, a plain one is freed at once
        if self.torch is None:
            nat.check(self.lib.gtf_stream_synchronize(None))
        self.n_g_all = [cg.n_g4, cg.n_g8, cg.n_g16, cg.n_g32, cg.n_g64]
        self.n_big = cg.n_big
        self.n_g2, self.n_g6, self.n_g12 = cg.n_g2, cg.n_g6, cg.n_g12
        self.n_o = [cg.n_o4, cg.n_o8, cg.n_o16]
        self.n_pack_waves = 0
        self.n_g = self.n_g_all if schedule else [0] * len(BUCKETS)
        self.use_sched = schedule

    def _dev_empty(self, n, dtype):
        """an uninitialised device array of this graph's allocator"""
        if self.torch is None:
            from .devmem import HipArray
            return HipArray(n, dtype)
        return self.torch.empty(n, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)

    # ---------------------------------------------------------------- memory
    def _make_arena(self, names):
        """place the arrays a pass mutates in one contiguous allocation, so a
        benchmark restore of the pass input is a single device copy"""
        torch = self.torch
        offs, total = {}, 0
        for k in names:
            nb = self.t[k].numel() * self.t[k].element_size()
            offs[k] = total
            total += (nb + 255) // 256 * 256
        arena = torch.zeros(max(total, 256), dtype=torch.uint8, device=self.device)
        for k in names:
            t = self.t[k]
            nb = t.numel() * t.element_size()
            view = arena[offs[k]:offs[k] + nb].view(t.dtype)
            view.copy_(t)
            self.t[k] = view
        self.arena = arena


    def _up(self, name, arr):
        arr = np.ascontiguousarray(arr)
        if self.torch is None:
            from .devmem import HipArray
            self.t[name] = HipArray.from_numpy(arr)
            return
        t = self.torch.from_numpy(arr.reshape(-1) if arr.size else arr.reshape(0)).to(self.device)
        self.t[name] = t

    def _np(self, t):
        """host copy of a device array (synchronises)"""
        return t.numpy() if self.torch is None else t.cpu().numpy()

    def _need_torch(self, what):
        if self.torch is None:
            raise NotImplementedError("%s needs DeviceGraph(mem='torch'); mem='hip' carries the stage methods, "
                                      "errors and download only" % what)

    def ptr(self, name):
        t = self.t[name]
        return ctypes.c_void_p(t.data_ptr() if t.numel() else 0)

    def _build_structs(self, pack=True):
        p = self.ptr
        base = dict(n_nodes=self.n_nodes, n_slots=self.n_slots, n_edges=self.n_edges,
                    slot_ptr=p("slot_ptr"), slot_src=p("slot_src"), slot_dst=p("slot_dst"), out_ptr=p("out_ptr"),
                    out_slot=p("out_slot"), slot_outpos=p("slot_outpos"), is_edge=p("is_edge"),
                    rev_edge=p("rev_edge"), solo=p("solo"), gnn=p("gnn"), xyzr=p("xyzr"), layer=p("layer"),
                    out_dst=p("out_dst"), slot_layer=p("slot_layer"),
                    slot_outidx=p("slot_outidx") if self.use_outidx else ctypes.c_void_p(0),
                    slot_class=p("slot_class") if self.use_classes else ctypes.c_void_p(0),
                    slot_sflags=p("slot_sflags") if self.use_classes else ctypes.c_void_p(0),
                    slot_sxzr=p("slot_sxzr") if self.use_sxzr else ctypes.c_void_p(0),
                    slot_static=p("slot_static") if self.use_static32 else ctypes.c_void_p(0),
                    slot_xclass=p("slot_xclass") if self.use_classes else ctypes.c_void_p(0))
        # with the node schedule (lane groups) and the sender schedule
        sched = dict(n_big=self.n_big, sched=p("sched"), n_g4=self.n_g_all[0], n_g8=self.n_g_all[1],
                     n_g16=self.n_g_all[2], n_g32=self.n_g_all[3], n_g64=self.n_g_all[4], sched_seg=p("sched_seg"),
                     out_sched=p("out_sched"), n_o4=self.n_o[0], n_o8=self.n_o[1], n_o16=self.n_o[2],
                     n_g2=self.n_g2, out_lanes=p("out_lanes"), n_g6=self.n_g6, n_g12=self.n_g12)
        if self.pad_plan is not None and self.pad_plan["tile_nodes"] > 0:   # (an empty graph has no tiles)
            pl = self.pad_plan
            sched.update(pad_tiles=pl["tiles"], pad_tile_nodes=pl["tile_nodes"], pad_tile_slots=pl["tile_slots"],
                         pad_count=(ctypes.c_int32 * 6)(*pl["count"]))
        if not self.use_sched:   # thread per node, 8-lane sender scan
            self.cg = nat.GtfGraph(**base)
        elif pack and self.n_pack_waves:
            self.cg = nat.GtfGraph(**base, **sched, pack_ent=p("pack_ent"), pack_wave=p("pack_wave"),
                                   n_pack_waves=self.n_pack_waves)
        else:
            self.cg = nat.GtfGraph(**base, **sched)
        self.cg_sched = nat.GtfGraph(**base, **sched)
        self.cn = nat.GtfNodes(*[p(f) for f in MUTABLE_NODE])
        self.cuts = nat.GtfStates(p("uts_rank"), p("uts_sv"), p("uts_tau"), p("uts_cov"), p("uts_xyzr"),
                                  p("uts_lik"), p("uts_mw"), p("uts_prior"), p("uts_lr"), p("uts_side"),
                                  p("uts_fresh"))
        self.ctse = nat.GtfStates(p("tse_rank"), p("tse_sv"), p("tse_tau"), p("tse_cov"), p("tse_xyzr"),
                                  ctypes.c_void_p(0), p("tse_mw"), p("tse_prior"), ctypes.c_void_p(0),
                                  ctypes.c_void_p(0), ctypes.c_void_p(0))
        self.ce = nat.GtfEdges(p("act"), p("edge_mw"), p("send_mw"))

    @property
    def stream(self):
        if self.torch is None:
            return ctypes.c_void_p(0)   # mem "hip": the default stream
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def cparams(p: Params) -> nat.GtfParams:
        return nat.GtfParams(p.sigma0xy, p.sigma0rz, p.sigma0rz2, p.endcap_boundary, p.chi2_cut,
                             p.reweight_threshold, p.cluster_chi2, p.cluster_kl)

    # ---------------------------------------------------------------- stages
    def clear_errors(self):
        nat.check(self.lib.gtf_clear_errors(self.ptr("ws"), self.stream))

    def errors(self) -> int:
        f = ctypes.c_uint32(0)
        nat.check(self.lib.gtf_read_errors(self.ptr("ws"), ctypes.byref(f), self.stream))
        return int(f.value)

    def raise_errors(self, ignore=0):
        f = self.errors() & ~ignore
        if f:
            msgs = [m for b, m in nat.ERR_FLAGS.items() if f & b]
            raise ValueError("reference exception reproduced on device: " + "; ".join(msgs))

    def extrapolate(self, p: Params):
        cp = self.cparams(p)
        nat.check(self.lib.gtf_extrapolate(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(self.cuts),
                                           ctypes.byref(self.ce), ctypes.byref(cp), self.ptr("ws"), self.stream))

    def message_passing(self, p: Params):
        cp = self.cparams(p)
        nat.check(self.lib.gtf_message_passing(ctypes.byref(self.cg), ctypes.byref(self.cn),
                                               ctypes.byref(self.cuts), ctypes.byref(self.ce), ctypes.byref(cp),
                                               self.ptr("ws"), self.stream))

    def node_ops(self, ops, p: Params, chi2=0.0, kl=0.0):
        """run named node-local ops (gtf._native.OPS) in order, one launch"""
        codes = [nat.OPS[o] for o in ops]
        arr = (ctypes.c_int8 * len(codes))(*codes)
        cp = self.cparams(p)
        nat.check(self.lib.gtf_node_ops(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(self.ctse),
                                        ctypes.byref(self.cuts), ctypes.byref(self.ce), ctypes.byref(cp), arr,
                                        len(codes), float(chi2), float(kl), self.ptr("ws"), self.stream))

    def update(self, p: Params):
        cp = self.cparams(p)
        nat.check(self.lib.gtf_update(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(self.ctse),
                                      ctypes.byref(self.cuts), ctypes.byref(self.ce), ctypes.byref(cp),
                                      self.ptr("ws"), self.stream))

    def cluster(self, key: str, chi2: float, kl: float, p: Params):
        cp = self.cparams(p)
        st = self.cuts if key in ("uts", "updated_track_states") else self.ctse
        k = 1 if st is self.cuts else 0
        nat.check(self.lib.gtf_cluster(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(st),
                                       ctypes.byref(self.ce), k, float(chi2), float(kl), ctypes.byref(cp),
                                       self.ptr("ws"), self.stream))

    def full_pass(self, p: Params, events=None):
        """events: optional 5 raw hipEvent_t handles (per-kernel timing)"""
        cp = self.cparams(p)
        if events is None:
            nat.check(self.lib.gtf_pass(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(self.ctse),
                                        ctypes.byref(self.cuts), ctypes.byref(self.ce), ctypes.byref(cp),
                                        self.ptr("ws"), self.stream))
        else:
            arr = (ctypes.c_void_p * 5)(*events)
            nat.check(self.lib.gtf_pass_ev(ctypes.byref(self.cg), ctypes.byref(self.cn), ctypes.byref(self.ctse),
                                           ctypes.byref(self.cuts), ctypes.byref(self.ce), ctypes.byref(cp),
                                           self.ptr("ws"), self.stream, arr))

    def track_state_estimates(self, p: Params, host_order: bool = True):
        """helper.compute_track_state_estimates (helper.py:238-452) for every key of the
        nodes' track_state_estimates dicts (tse_rank >= 0, dict order as given): writes
        tse_sv / tse_cov / tse_tau / tse_xyzr / tse_theta / tse_var_ms on the device and
        returns the per-node attributes (xy/zr_edge_gradient_mean_var,
        angle_of_rotation, translation) as device tensors -- in host node order, or with
        host_order=False in the device layout's order (no gathers: what a caller that keeps
        the event on the device consumes). A key whose parabola matrix is singular
        (np.linalg.inv raises, helper.py:384) sets GTF_ERR_SINGULAR_H in errors() and in the
        node's entry of the node_err diagnostics; raise_errors() raises for it."""
        self._natural_only("track_state_estimates")
        if self.torch is None:
            return self._track_state_estimates_hip(p, host_order)
        torch = self.torch
        N = self.n_nodes
        nan = float("nan")
        x = {"xy_mean_var": torch.full((N, 2), nan, dtype=torch.float64, device=self.device),
             "zr_mean_var": torch.full((N, 2), nan, dtype=torch.float64, device=self.device),
             "angle_of_rotation": torch.full((N,), nan, dtype=torch.float64, device=self.device),
             "translation": torch.full((N, 2), nan, dtype=torch.float64, device=self.device)}
        vp = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)  # noqa: E731
        ex = nat.GtfTseExtra(self.ptr("tse_theta"), self.ptr("tse_var_ms"), vp(x["xy_mean_var"]),
                             vp(x["zr_mean_var"]), vp(x["angle_of_rotation"]), vp(x["translation"]))
        cp = self.cparams(p)
        nat.check(self.lib.gtf_track_state_estimates_ws(ctypes.byref(self.cg_sched), ctypes.byref(self.ctse),
                                                        ctypes.byref(ex), ctypes.byref(cp), self.ptr("ws"),
                                                        self.stream))
        if self.order is not None and host_order:   # per-node outputs in host node order
            inv = self._inv_order()
            x = {k: v[inv] for k, v in x.items()}
        return x

    def _track_state_estimates_hip(self, p: Params, host_order: bool):
        """mem "hip": the same call on gtf.devmem arrays; the per-node attributes come back
        as host arrays"""
        from .devmem import HipArray
        N = self.n_nodes
        shapes = {"xy_mean_var": (N, 2), "zr_mean_var": (N, 2), "angle_of_rotation": (N,), "translation": (N, 2)}
        x = {k: HipArray.from_numpy(np.full(int(np.prod(sh)), np.nan)) for k, sh in shapes.items()}
        vp = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)  # noqa: E731
        ex = nat.GtfTseExtra(self.ptr("tse_theta"), self.ptr("tse_var_ms"), vp(x["xy_mean_var"]),
                             vp(x["zr_mean_var"]), vp(x["angle_of_rotation"]), vp(x["translation"]))
        cp = self.cparams(p)
        nat.check(self.lib.gtf_track_state_estimates_ws(ctypes.byref(self.cg_sched), ctypes.byref(self.ctse),
                                                        ctypes.byref(ex), ctypes.byref(cp), self.ptr("ws"),
                                                        self.stream))
        out = {k: v.numpy().reshape(shapes[k]) for k, v in x.items()}
        if self.order is not None and host_order:
            inv = np.empty(self.order.size, np.int64)
            inv[self.order] = np.arange(self.order.size)
            out = {k: v[inv] for k, v in out.items()}
        return out

    # ------------------------------------------ a15: distances between updated states
    def updated_state_distances(self, truth=None, host_order: bool = True):
        """calculate_distance_between_updated_track_states.py (:27-104 over the pair loop
        :134-195) on the current updated_track_states: every pair i > j of the dict entries
        of each node with the dict and more than one active in-edge. Returns (pair_ptr [N+1]
        int64, {"chi2", "avg_tau", "avg_theta", "delta_theta"[, "truth"]}) as device
        tensors, pairs of node v at [pair_ptr[v], pair_ptr[v+1]) in the reference's loop
        order. truth: [N] truth_particle per node (host or device), or None. host_order=False:
        the node segments in the device layout's node order (no reordering gathers)."""
        self._natural_only("updated_state_distances")
        self._need_torch("updated_state_distances")
        torch = self.torch
        dev = self.device
        N = self.n_nodes
        vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)  # noqa: E731
        counts = torch.zeros(max(N, 1), dtype=torch.int64, device=dev)
        nat.check(self.lib.gtf_updated_state_pair_counts(ctypes.byref(self.cg_sched), ctypes.byref(self.cn),
                                                         ctypes.byref(self.cuts), ctypes.byref(self.ce), vp(counts),
                                                         self.stream))
        pair_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        if N:
            torch.cumsum(counts[:N], 0, out=pair_ptr[1:])
        P = int(pair_ptr[-1].item())
        out = {k: torch.empty(max(P, 1), dtype=torch.float64, device=dev)
               for k in ("chi2", "avg_tau", "avg_theta", "delta_theta")}
        tr = None
        if truth is not None:
            tr = torch.as_tensor(np.asarray(truth, dtype=np.int64) if not torch.is_tensor(truth) else truth,
                                 device=dev).to(torch.int64).contiguous()
            out["truth"] = torch.empty(max(P, 1), dtype=torch.int8, device=dev)
        if tr is not None and self.order is not None:
            tr = tr[torch.from_numpy(self.order).to(dev)].contiguous()   # device node order
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        po = nat.GtfPairOut(vp(out["chi2"]), vp(out["avg_tau"]), vp(out["avg_theta"]), vp(out["delta_theta"]),
                            vp(out.get("truth")), vp(err))
        nat.check(self.lib.gtf_updated_state_distances(ctypes.byref(self.cg_sched), ctypes.byref(self.cn),
                                                       ctypes.byref(self.cuts), ctypes.byref(self.ce), vp(tr),
                                                       vp(pair_ptr), ctypes.byref(po), self.stream))
        f = int(err.item())
        if f:
            raise ValueError("updated-state distances: " +
                             "; ".join(m for b, m in nat.ERR_FLAGS.items() if f & b))
        cols = {k: v[:P] for k, v in out.items()}
        if self.order is not None and N and host_order:   # node segments of pairs in host node order
            inv = self._inv_order()
            cnt = counts[:N][inv]
            hptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            torch.cumsum(cnt, 0, out=hptr[1:])
            first = torch.repeat_interleave(pair_ptr[:N][inv], cnt, output_size=P)
            idx = first + (torch.arange(P, device=dev) - torch.repeat_interleave(hptr[:N], cnt, output_size=P))
            cols = {k: v[idx] for k, v in cols.items()}
            pair_ptr = hptr
        return pair_ptr, cols

    # ------------------------------------------------------- tag propagation
    def tag_propagation(self, tags, radius, threshold=0.1, max_sweeps=100000):
        """Jacobi sweeps until flips / processed <= threshold (tag_propagation.py:97-164), the
        whole stage in one gtf_tag_propagate call (stop rule on the device, one host read per
        batch of sweeps). tags / radius in host node order; returns (tags, flips per sweep)."""
        self._natural_only("tag_propagation")
        r = self._dev_from(np.ascontiguousarray(self._to_dev_nodes(radius), dtype=np.float64))
        ta = self._dev_from(np.ascontiguousarray(self._to_dev_nodes(tags), dtype=np.int64))
        flips = self.tag_propagation_dev(ta, r, threshold, max_sweeps)
        out = self._np(ta)[:self.n_nodes]
        if self.order is not None:
            h = np.empty_like(out)
            h[self.order] = out
            out = h
        return out, flips

    def tag_propagation_dev(self, tags, radius, threshold=0.1, max_sweeps=100000):
        """gtf_tag_propagate on device arrays in this graph's node order: `tags` (int64 [N]) is
        replaced by the final tags; returns the flip count of every sweep"""
        nb = int(self.lib.gtf_tag_workspace_bytes(self.n_nodes, self.n_edges))
        ws = getattr(self, "_tag_ws", None)
        if ws is None or ws.numel() < nb:
            ws = self._tag_ws = self._dev_zeros(nb, np.uint8)
        hf = getattr(self, "_tag_flips", None)
        if hf is None or hf.size < max(max_sweeps, 1):
            hf = self._tag_flips = np.zeros(max(max_sweeps, 1), np.int32)
        n = ctypes.c_int32(0)
        vp = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)  # noqa: E731
        nat.check(self.lib.gtf_tag_propagate(ctypes.byref(self.cg), vp(radius), vp(tags), float(threshold),
                                             int(max_sweeps), ctypes.c_void_p(hf.ctypes.data), ctypes.byref(n),
                                             vp(ws), ctypes.c_size_t(nb), self.stream))
        return [int(x) for x in hf[:n.value]]

    def _dev_zeros(self, n, dtype):
        """a zeroed device array of this graph's allocator"""
        if self.torch is None:
            from .devmem import HipArray
            return HipArray.zeros(n, dtype)
        return self.torch.zeros(n, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)

    def _dev_from(self, a):
        """a host array on the device (this graph's allocator)"""
        a = np.ascontiguousarray(a).reshape(-1)
        if self.torch is None:
            from .devmem import HipArray
            return HipArray.from_numpy(a)
        return self.torch.from_numpy(a).to(self.device)

    # ------------------------------------------------------------ diagnostics
    def set_diagnostics(self, node_err: bool = True, edge_chi2: bool = True, slot_cluster: bool = False):
        """SURVEY §5's optional diagnostic outputs (gtf_set_diagnostics), written by the stage
        kernels from now on: the GTF_ERR_* bits of every reference exception per node (which
        node, so which subgraph, would make the reference raise) and the chi2 of every
        extrapolated edge (the values extrapolate_merged_states.py:134-172 prints to CSV).
        Off by default and never on the benchmark's path; set_diagnostics(False, False)
        unregisters them."""
        self._need_torch("set_diagnostics")
        torch = self.torch
        self.diag_t = {}
        if node_err:
            self.diag_t["node_err"] = torch.zeros(max(self.n_nodes, 1), dtype=torch.int32, device=self.device)
        if edge_chi2:
            self.diag_t["edge_chi2"] = torch.full((max(self.n_slots, 1),), float("nan"), dtype=torch.float64,
                                                  device=self.device)
        if slot_cluster:
            self.diag_t["slot_cluster"] = torch.zeros(max(self.n_slots, 1), dtype=torch.uint8, device=self.device)
        vp = lambda k: ctypes.c_void_p(self.diag_t[k].data_ptr()) if k in self.diag_t else ctypes.c_void_p(0)  # noqa: E731
        d = nat.GtfDiag(vp("node_err"), vp("edge_chi2"), vp("slot_cluster"))
        nat.check(self.lib.gtf_set_diagnostics(self.ptr("ws"), ctypes.byref(d), self.stream))

    def diagnostics(self) -> dict:
        """the registered diagnostics in host order: node_err [N] uint32, edge_chi2 [S]
        (NaN where no extrapolation ran), slot_cluster [S] uint8"""
        out = {}
        for k, v in getattr(self, "diag_t", {}).items():
            if k == "node_err":
                a = v.cpu().numpy()[:self.n_nodes].astype(np.uint32)
                out[k] = a if self.order is None else self._host_nodes(a)
            else:
                a = v.cpu().numpy()[:self.n_slots]
                out[k] = a if self.slot_perm is None else self._host_slots(a, np.nan if a.dtype.kind == "f" else 0)
        return out

    def clear_diagnostics(self):
        """zero node_err / slot_cluster and NaN-fill edge_chi2 (stream-ordered)"""
        for k, v in getattr(self, "diag_t", {}).items():
            v.fill_(float("nan") if k == "edge_chi2" else 0)

    def track_node_errors(self, on: bool = True):
        """Register a zeroed per-node error array (gtf_diag.node_err, uint32 [N]) ALONE through
        gtf_set_diagnostics: from now on every reference exception the stage kernels reproduce also ORs its
        GTF_ERR_* bits into the raising node's entry, which event_errors() reduces per event. The array
        comes from this graph's own allocator (mem "torch" or "hip": the CLIs never import torch); its zero
        fill is the whole cost while nothing raises. It replaces whatever set_diagnostics() registered;
        on=False unregisters it. The registration lives in this graph's workspace: a subset() child starts
        without one. Natural layout only (the entries are in device node order)."""
        if on and self.layout != "natural":
            raise NotImplementedError("track_node_errors: only layout='natural'")
        self.diag_t = {}
        self.node_err_t = self._dev_zeros(max(self.n_nodes, 1), np.int32) if on else None
        d = nat.GtfDiag(ctypes.c_void_p(self.node_err_t.data_ptr() if on else 0), ctypes.c_void_p(0), ctypes.c_void_p(0))
        nat.check(self.lib.gtf_set_diagnostics(self.ptr("ws"), ctypes.byref(d), self.stream))
        return self

    def event_errors(self, mask: int = 0xFFFFFFFF, n_events: int = None) -> dict:
        """gtf_event_errors on the array of track_node_errors() and ``carried["event"]`` (one event without
        that column): which events raised. Returns the host arrays err_ev [K] uint32, n_raising [K] int32,
        first_node [K] int32 (-1: none), first_id [K] int64 (the resident node_id column; None without it),
        and ``keep``, a device uint8 [N] of this graph's allocator: 1 on the nodes of the events that did
        not raise, what subset() takes. One synchronisation. n_events: this graph's ``n_events`` (1 when it
        is not a batch)."""
        if getattr(self, "node_err_t", None) is None:
            raise ValueError("event_errors needs track_node_errors() before the stage")
        event = getattr(self, "carried", {}).get("event")
        K = int(n_events if n_events is not None else (getattr(self, "n_events", 1) if event is not None else 1))
        N = self.n_nodes
        out = {"err_ev": np.zeros(K, np.uint32), "n_raising": np.zeros(K, np.int32),
               "first_node": np.full(K, -1, np.int32), "first_id": None}
        nid = self.t.get("node_id")
        if nid is not None:
            out["first_id"] = np.full(K, -1, np.int64)
        keep = self._dev_empty(N, np.uint8)
        if N and K:
            vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)  # noqa: E731
            hp = lambda a: ctypes.c_void_p(a.ctypes.data if a is not None else 0)  # noqa: E731
            io = nat.GtfEventErrorsIo(node_err=vp(self.node_err_t), event=vp(event), node_id=vp(nid), n_nodes=N,
                                      n_events=K, mask=int(mask) & 0xFFFFFFFF, keep=vp(keep),
                                      host_err_ev=hp(out["err_ev"]), host_n_raising=hp(out["n_raising"]),
                                      host_first_node=hp(out["first_node"]), host_first_id=hp(out["first_id"]))
            nb = int(self.lib.gtf_event_errors_workspace_bytes(K))
            ws = self._dev_empty(nb, np.uint8)
            nat.check(self.lib.gtf_event_errors(ctypes.byref(io), vp(ws), ctypes.c_size_t(nb), self.stream))
        out["keep"] = keep
        return out

    def _host_nodes(self, a, fill=0):
        nm = self.order >= 0
        h = np.full(int(nm.sum()), fill, a.dtype)
        h[self.order[nm]] = a[nm]
        return h

    def _host_slots(self, a, fill=0):
        sm = self.slot_perm >= 0
        h = np.full(int(sm.sum()), fill, a.dtype)
        h[self.slot_perm[sm]] = a[sm]
        return h

    # ---------------------------------------------------------------- results
    def materialize(self):
        """write the live updated_track_states coordinates (gtf_states.fresh bit 1) into
        uts_xyzr on the device (gtf_uts_materialize): before reading them back"""
        nat.check(self.lib.gtf_uts_materialize(ctypes.byref(self.cg_sched), ctypes.byref(self.cuts), self.stream))

    def download(self, g: TrackGraph) -> TrackGraph:
        """copy the mutable arrays back into the host TrackGraph (in place, host order)"""
        self.materialize()
        nm = None if self.order is None else self.order >= 0          # (padded: not a dummy node)
        sm = None if self.slot_perm is None else self.slot_perm >= 0  # (padded: not a padding slot)
        for f in MUTABLE_NODE:
            a = self._np(self.t[f]).reshape((-1,) + g.node[f].shape[1:])
            if self.order is None:
                g.node[f][...] = a
            else:
                g.node[f][self.order[nm]] = a[nm]
        for f in SLOT_FIELDS:
            if f in STATIC_SLOT or f == "slot_key":
                continue
            a = self._np(self.t[f]).reshape((-1,) + g.slot[f].shape[1:])
            if f == "uts_fresh":
                a = a & 1   # (bit 1 is cleared by materialize())
            if self.slot_perm is None:
                g.slot[f][...] = a
            else:
                g.slot[f][self.slot_perm[sm]] = a[sm]
        return g

    # ------------------------------------------------ node removal between iterations
    SUBSET_FILL = {"is_edge": nat.COL_ZERO_ORPHAN, "rev_edge": nat.COL_ZERO_ORPHAN, "act": nat.COL_ZERO_ORPHAN,
                   "edge_mw": nat.COL_NAN_ORPHAN, "send_mw": nat.COL_NAN_ORPHAN, "uts_fresh": nat.COL_ZERO_ALL}

    def _base_graph(self):
        """a gtf_graph of the base fields alone (what plan, apply and prepare read)"""
        p = self.ptr
        return nat.GtfGraph(n_nodes=self.n_nodes, n_slots=self.n_slots, n_edges=self.n_edges, slot_ptr=p("slot_ptr"),
                            slot_src=p("slot_src"), out_ptr=p("out_ptr"), out_slot=p("out_slot"),
                            is_edge=p("is_edge"), rev_edge=p("rev_edge"), gnn=p("gnn"), layer=p("layer"))

    def _as_dev(self, a, dtype, n, what):
        """`a` (a host array, or a device array of this graph's allocator) as a flat device array
        of n elements of dtype"""
        dtype = np.dtype(dtype)
        if self.torch is not None and self.torch.is_tensor(a):
            t = a.to(device=self.device, dtype=getattr(self.torch, dtype.name)).contiguous().reshape(-1)
        elif hasattr(a, "data_ptr"):   # a gtf.devmem array
            if a.dtype != dtype:
                raise ValueError("%s: a device array must be %s" % (what, dtype.name))
            t = a
        else:
            t = self._dev_from(np.ascontiguousarray(np.asarray(a), dtype=dtype))
        if t.numel() != n:
            raise ValueError("%s must have %d elements" % (what, n))
        return t

    def node_id_dev(self):
        """the node ids (int64 [N]) as a resident node column: uploaded on first need; a subset()
        child of a graph that holds the column gets it through the gather"""
        if "node_id" not in self.t:
            if getattr(self, "_node_id_host", None) is None:
                raise ValueError("this DeviceGraph holds no node ids (a subset() child of a parent without the "
                                 "resident column: call node_id_dev() on the parent first)")
            if self.layout != "natural":
                raise NotImplementedError("node_id_dev: only layout='natural'")
            self.t["node_id"] = self._dev_from(np.ascontiguousarray(self._node_id_host, np.int64))
        return self.t["node_id"]

    def subset(self, keep, gnn=None, carry=None, keep_fresh: bool = False) -> "DeviceGraph":
        """The graph after removing the nodes whose `keep` is false, built on the device:
        gtf.graph.subset (extract_track_candidates.py:459-467), array for array, by
        gtf_graph_subset_plan / _apply and gtf_subset_gather, with the child's schedules and
        slot tables by gtf_graph_prepare (tables == "device" whatever this graph had).
        keep: host bool [N] or device uint8 [N] in this graph's node order; gnn: optional
        [N, 4] replacement of the GNN coordinates (host or device) -- the extraction's
        close-proximity merge. The child's uts_fresh is 0 in both bits: its entries read
        their stored xyzr until the next message passing rewrites them. Natural layout only.
        carry: {name: [N, ...] array} of the caller's own node-axis columns (host, or device of
        this graph's allocator), gathered with the payload; the child holds them as device arrays
        in ``carried``. The resident node_id column (node_id_dev) travels the same way.
        keep_fresh: the child's uts_fresh keeps bit 0 of the parent's instead of 0 -- a cut in the middle of
        an iteration (run_batch's on_error="isolate"), where the stage's output is still to be saved."""
        if self.layout != "natural" or self.n_pack_waves:
            raise NotImplementedError("DeviceGraph.subset: only layout='natural' without pack=True (the renumbered, "
                                      "padded and packed layouts are not carried over); this graph has layout=%r, "
                                      "pack=%r" % (self.layout, bool(self.n_pack_waves)))
        if not self._sub_ok:
            raise ValueError("DeviceGraph.subset needs sub_id >= 0 on every node")
        N, S, E = self.n_nodes, self.n_slots, self.n_edges
        if not (self.torch is not None and self.torch.is_tensor(keep)) and not hasattr(keep, "data_ptr"):
            keep = np.asarray(keep)
            if keep.shape != (N,):
                raise ValueError("keep must be a mask over the %d nodes" % N)
            keep = (keep != 0).astype(np.uint8)
        keep_t = self._as_dev(keep, np.uint8, N, "keep")
        gnn_t = self._as_dev(gnn, np.float64, 4 * N, "gnn") if gnn is not None else self.t["gnn"]
        self.materialize()
        L, vp = self.lib, (lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0))
        cg = self._base_graph()
        nb = int(L.gtf_graph_subset_workspace_bytes(N, S, E, self.n_sub))
        ws = self._dev_empty(nb, np.uint8)
        cnt = nat.GtfSubsetCounts()
        nat.check(L.gtf_graph_subset_plan(ctypes.byref(cg), self.ptr("tse_rank"), self.ptr("uts_rank"),
                                          self.ptr("sub_id"), self.n_sub, vp(keep_t), vp(ws), ctypes.c_size_t(nb),
                                          ctypes.byref(cnt), self.stream))
        N2, S2, E2 = cnt.n_nodes, cnt.n_slots, cnt.n_edges
        c = DeviceGraph.__new__(DeviceGraph)
        c.mem, c.torch, c.lib, c.device = self.mem, self.torch, self.lib, self.device
        c.layout, c.order, c.slot_perm, c.pad_plan = "natural", None, None, None
        c.slot_ptr_host = None
        c.n_nodes, c.n_slots, c.n_edges, c.n_sub, c._sub_ok = N2, S2, E2, cnt.n_sub, True
        c.tables = "device"
        c.t = {}
        c._node_id_host, c.carried = None, {}
        extra = []   # (source, destination, row bytes) of the node-axis columns beyond the graph's own
        if "node_id" in self.t:
            c.t["node_id"] = c._dev_empty(N2, np.int64)
            extra.append((self.t["node_id"], c.t["node_id"], 8))
        for name, a in (carry or {}).items():
            if not hasattr(a, "data_ptr"):
                a = np.ascontiguousarray(a)
                dt = a.dtype
                a = self._dev_from(a)
            else:
                dt = a.dtype if isinstance(a.dtype, np.dtype) else np.dtype(str(a.dtype).split(".")[-1])
                a = a if self.torch is None else a.contiguous().reshape(-1)
            if N and a.numel() % N:
                raise ValueError("carry[%r] must have one row per node" % name)
            width = a.numel() // N if N else 1
            c.carried[name] = c._dev_empty(N2 * width, dt)
            extra.append((a, c.carried[name], width * np.dtype(dt).itemsize))
        struct = [("node_map", N2, np.int32), ("slot_map", S2, np.int32), ("slot_ptr", N2 + 1, np.int32),
                  ("slot_src", S2, np.int32), ("out_ptr", N2 + 1, np.int32), ("out_slot", E2, np.int32),
                  ("sub_id", N2, np.int32), ("solo", N2, np.uint8)]
        for name, n, dt in struct:
            c.t[name] = c._dev_empty(n, dt) if N else c._dev_zeros(n, dt)
        if N:
            so = nat.GtfSubsetOut(**{name: c.ptr(name) for name, _, _ in struct})
            nat.check(L.gtf_graph_subset_apply(ctypes.byref(cg), vp(ws), ctypes.byref(so), self.stream))
        # the payload: every device-resident node and slot array through the maps
        for axis, rows, names in ((0, N2, ("gnn", "xyzr", "layer") + MUTABLE_NODE),
                                  (1, S2, tuple(f for f in SLOT_FIELDS if f not in ("slot_key", "slot_src")))):
            cols = []
            for f in names:
                src = gnn_t if f == "gnn" else self.t[f]
                dt, shape, _ = (NODE_FIELDS if axis == 0 else SLOT_FIELDS)[f]
                width = int(np.prod(shape, dtype=np.int64))
                c.t[f] = c._dev_empty(rows * width, dt)
                if rows:
                    cols.append(nat.GtfColumn(vp(src), c.ptr(f), width * np.dtype(dt).itemsize,
                                              self.SUBSET_FILL.get(f, nat.COL_COPY)
                                              if axis and not (keep_fresh and f == "uts_fresh") else nat.COL_COPY))
            if axis == 0 and rows:
                cols += [nat.GtfColumn(vp(a), vp(b), rb, nat.COL_COPY) for a, b, rb in extra if rb]
            if cols:
                arr = (nat.GtfColumn * len(cols))(*cols)
                nat.check(L.gtf_subset_gather(vp(ws), axis, arr, len(cols), self.stream))
        # the plan's workspace and a converted keep / gnn go out of scope with kernels in flight: a
        # torch allocation is reused in stream order, a plain one is freed at once
        if self.torch is None:
            nat.check(L.gtf_stream_synchronize(None))
        shape = TrackGraph(N2, S2, None, None, np.zeros(E2, np.int32), {}, {}, cnt.n_sub)   # (sizes only)
        if N2 > 0 and (S2 > 0 or E2 > 0):
            c._device_tables(shape, None, True)
        else:   # nothing for gtf_graph_prepare to build: the few tables of a slot-free graph from the host
            from .graph import empty_arrays
            z = np.zeros(N2 + 1, np.int32)
            solo = c.t["solo"]
            c._host_tables(TrackGraph(N2, 0, z, z, np.zeros(0, np.int32), empty_arrays(NODE_FIELDS, N2),
                                      empty_arrays(SLOT_FIELDS, 0), cnt.n_sub), None, True, False)
            c.t["solo"] = solo
        c._finish(shape, False)
        if hasattr(self, "n_events"):   # (a batch: the child's carried event column names as many events)
            c.n_events = self.n_events
        return c

    # ------------------------------------------------ a batch of resident events as one graph
    @classmethod
    def concat(cls, parts, mem=None, device=None) -> "DeviceGraph":
        """gtf.graph.concat on the device (gtf_graph_concat, gtf_concat_columns): the resident graphs
        `parts` -- natural layout, one allocator and device, as from_event, build_event_dev or subset
        leave them -- fused into one DeviceGraph with tables == "device" (gtf_graph_prepare), part after
        part, indices shifted, orphan keys kept. ``carried["event"]`` (int32 [N]) names the part of
        every node and ``n_events`` their number; the resident node_id column and the parts' carried
        columns (vivl) are fused with the payload when every part holds them. Parts without nodes are
        legal anywhere. The number of launches does not depend on len(parts); nothing synchronises
        (mem "hip": once, before the tables' scratch is freed). host_graph() downloads the result when
        no part has orphan keys. mem / device: those of the parts (given, they must agree); they decide
        alone for an empty list."""
        parts = list(parts)
        K = len(parts)
        for d in parts:
            if not isinstance(d, cls):
                raise TypeError("DeviceGraph.concat takes DeviceGraphs")
            if d.layout != "natural" or d.n_pack_waves:
                raise NotImplementedError("DeviceGraph.concat: only layout='natural' without pack=True (the "
                                          "renumbered, padded and packed layouts are not carried over); a part has "
                                          "layout=%r, pack=%r" % (d.layout, bool(d.n_pack_waves)))
            if not d._sub_ok:
                raise ValueError("DeviceGraph.concat needs sub_id >= 0 on every node")
            if d.mem != parts[0].mem or str(d.device) != str(parts[0].device):
                raise ValueError("DeviceGraph.concat: the parts must share one allocator and device")
        if parts and mem is not None and mem != parts[0].mem:
            raise ValueError("DeviceGraph.concat: mem=%r, but the parts were allocated with mem=%r" % (mem, parts[0].mem))
        mem = parts[0].mem if parts else (mem or "torch")
        if mem not in ("torch", "hip"):
            raise ValueError("mem must be 'torch' or 'hip'")
        c = cls.__new__(cls)
        c.mem = mem
        c.torch = torch = _torch() if mem == "torch" else None
        if parts:
            c.device, c.lib = parts[0].device, parts[0].lib
        elif torch is not None:
            c.device, c.lib = torch.device(device or "cuda"), nat.lib()
        else:
            c.device, c.lib = device or "cuda", nat.lib(lean=True)
            nat.check(c.lib.gtf_device_init(int(c.device.split(":")[1]) if ":" in c.device else 0))
        c.layout, c.order, c.slot_perm, c.pad_plan = "natural", None, None, None
        c.slot_ptr_host, c._node_id_host = None, None
        c.tables = "device"
        c.t, c.carried = {}, {}
        c.n_events = K
        sizes = [(d.n_nodes, d.n_slots, d.n_edges, d.n_sub) for d in parts]
        N, S, E, B = (sum(z[i] for z in sizes) for i in range(4))
        if max(N, S, E, B) >= 1 << 31:
            raise ValueError("DeviceGraph.concat: the parts sum to 2^31 or more nodes, slots, edges or subgraphs")
        c.n_nodes, c.n_slots, c.n_edges, c.n_sub, c._sub_ok = N, S, E, B, True
        L, vp = c.lib, (lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0))
        adr = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
        # the columns: (axis, sources, destination, row bytes)
        cols = []

        def column(axis, name, srcs, dt, width, store):
            rows = N if axis == 0 else S
            rb = width * np.dtype(dt).itemsize
            wb = 8 if rb % 8 == 0 else 4 if rb % 4 == 0 else 1
            for d, a in zip(parts, srcs):
                if a.numel() != (d.n_nodes if axis == 0 else d.n_slots) * width:
                    raise ValueError("DeviceGraph.concat: %r of a part has not one row of %d per %s"
                                     % (name, width, "node" if axis == 0 else "slot"))
                if a.numel() and a.data_ptr() % wb:
                    raise ValueError("DeviceGraph.concat: %r of a part is not aligned to %d bytes" % (name, wb))
            store[name] = c._dev_empty(rows * width, dt)
            cols.append((axis, [adr(a) for a in srcs], store[name], rb))

        for f in ("gnn", "xyzr", "layer") + MUTABLE_NODE:
            dt, shape, _ = NODE_FIELDS[f]
            column(0, f, [d.t[f] for d in parts], dt, int(np.prod(shape, dtype=np.int64)), c.t)
        column(0, "solo", [d.t["solo"] for d in parts], np.uint8, 1, c.t)
        if all("node_id" in d.t or getattr(d, "_node_id_host", None) is not None for d in parts):
            column(0, "node_id", [d.node_id_dev() for d in parts], np.int64, 1, c.t)
        names = [set(getattr(d, "carried", {})) for d in parts]
        for name in sorted(set.intersection(*names) if names else ()):
            if name == "event":   # (a fused graph as a part: its events become one)
                continue
            srcs = [d.carried[name] for d in parts]
            a0 = srcs[0]
            dt = a0.dtype if isinstance(a0.dtype, np.dtype) else np.dtype(str(a0.dtype).split(".")[-1])
            width = next((a.numel() // d.n_nodes for d, a in zip(parts, srcs) if d.n_nodes), 2 if name == "vivl" else 1)
            column(0, name, srcs, dt, width, c.carried)
        for f, (dt, shape, _) in SLOT_FIELDS.items():
            if f not in ("slot_key", "slot_src"):
                column(1, f, [d.t[f] for d in parts], dt, int(np.prod(shape, dtype=np.int64)), c.t)
        struct = [("slot_ptr", N + 1), ("slot_src", S), ("out_ptr", N + 1), ("out_slot", E), ("sub_id", N)]
        for name, n in struct:
            c.t[name] = c._dev_empty(n, np.int32)
        c.carried["event"] = c._dev_empty(N, np.int32)
        # one upload: the part table, then every column's K source pointers
        ptab = (nat.GtfConcatPart * max(K, 1))(*[
            nat.GtfConcatPart(d.n_nodes, d.n_slots, d.n_edges, d.n_sub, *[adr(d.t[k]) for k in
                                                                          ("slot_ptr", "slot_src", "out_ptr", "out_slot",
                                                                           "sub_id")]) for d in parts])
        pwords = ctypes.sizeof(nat.GtfConcatPart) // 8
        host = np.zeros(max(K, 1) * (pwords + len(cols)), np.int64)
        host[:max(K, 1) * pwords] = np.frombuffer(ptab, np.int64)
        for i, (_, srcs, _, _) in enumerate(cols):
            at = max(K, 1) * pwords + i * K
            host[at:at + K] = srcs
        tab = c._dev_from(host)
        nb = int(L.gtf_graph_concat_workspace_bytes(K))
        ws = c._dev_empty(nb, np.uint8)
        hs = (nat.GtfConcatSizes * max(K, 1))(*[nat.GtfConcatSizes(*z) for z in sizes])
        co = nat.GtfConcatOut(event=vp(c.carried["event"]), **{name: c.ptr(name) for name, _ in struct})
        nat.check(L.gtf_graph_concat(hs, ctypes.c_void_p(tab.data_ptr()), K, ctypes.byref(co), vp(ws),
                                     ctypes.c_size_t(nb), c.stream))
        if cols:
            cc = (nat.GtfConcatColumn * len(cols))(*[
                nat.GtfConcatColumn(tab.data_ptr() + 8 * (max(K, 1) * pwords + i * K), vp(dst), rb, axis)
                for i, (axis, _, dst, rb) in enumerate(cols)])
            nat.check(L.gtf_concat_columns(vp(ws), K, N, S, cc, len(cols), c.stream))
        # the tables and the workspace go out of scope with kernels in flight: a torch allocation is reused
        # in stream order, a plain one is freed at once
        if torch is None:
            nat.check(L.gtf_stream_synchronize(None))
        c._event = "node_id" in c.t and "vivl" in c.carried   # (host_graph: the ids and vivl are resident)
        shape = TrackGraph(N, S, None, None, np.zeros(E, np.int32), {}, {}, B)   # (sizes only)
        if N > 0 and (S > 0 or E > 0):
            c._device_tables(shape, None, True)
        else:   # nothing for gtf_graph_prepare to build: the few tables of a slot-free graph from the host
            from .graph import empty_arrays
            zp = np.zeros(N + 1, np.int32)
            solo = c.t["solo"]
            c._host_tables(TrackGraph(N, 0, zp, zp, np.zeros(0, np.int32), empty_arrays(NODE_FIELDS, N),
                                      empty_arrays(SLOT_FIELDS, 0), B), None, True, False)
            c.t["solo"] = solo
        c._finish(shape, False)
        return c

    # ------------------------------------------------ event conversion into a resident graph
    EVENT_FILL = {"has_tse": 1, "is_edge": 1, "rev_edge": 1, "act": 1}   # (else: the field's empty value)

    @classmethod
    def from_event(cls, ids, x, y, z, r, layer_id, row_a, row_b, device: str = "cuda", mem: str = "torch"):
        """The packed event of gtf.io.build_event_csr (event_conversion.py:53-101, helper.py:465-545),
        made in HBM: host columns of the nodes kept by the volume window, in CSV order (io.read_nodes),
        and the edge rows as io.csr_from_rows takes them (add_edge(row_a, row_b) first). The eight
        columns go up once -- or are device arrays of this allocator already (gtf.io.read_nodes_dev /
        read_edges_dev: int64 ids, layer_id >= 0 and rows, float64 coordinates; nothing is uploaded and
        N and R are their lengths) --; gtf_build_event_csr_device builds the CSR, gtf_event_pack the node columns,
        gtf_fill_columns the empty states (every edge active, has_tse set) and gtf_graph_prepare the
        schedules and slot tables. Natural layout, tables == "device"; the node ids are the resident
        node_id column (node_id_dev, subset) and vivl is ``carried["vivl"]``. host_graph() downloads it."""
        return cls._from_event(ids, x, y, z, r, layer_id, row_a, row_b, device, mem, lambda part: None)

    @classmethod
    def _event_shell(cls, device, mem):
        """an empty DeviceGraph of from_event's kind: the allocator, the library, natural layout"""
        if mem not in ("torch", "hip"):
            raise ValueError("mem must be 'torch' or 'hip'")
        c = cls.__new__(cls)
        c.mem = mem
        c.torch = torch = _torch() if mem == "torch" else None
        if torch is not None:
            c.device = torch.device(device)
            c.lib = nat.lib()
        else:
            c.device = device
            c.lib = nat.lib(lean=True)
            nat.check(c.lib.gtf_device_init(int(device.split(":")[1]) if ":" in device else 0))
        c.layout, c.order, c.slot_perm, c.pad_plan = "natural", None, None, None
        c.slot_ptr_host, c._node_id_host = None, None
        c.tables = "device"
        c.t, c.carried = {}, {}
        c._event = True   # (host_graph: a whole event, its ids resident -- not a subset() child)
        return c

    @classmethod
    def from_events(cls, parts, device: str = "cuda", mem: str = "torch"):
        """DeviceGraph.concat([from_event(*p) for p in parts]) in ONE build: ``parts`` is a list of
        from_event's eight columns (ids, x, y, z, r, layer_id, row_a, row_b), all host or all device
        arrays. Host columns are concatenated and go up once per column; device columns are gathered by
        gtf_graph_concat's offsets and gtf_concat_columns (the node and the row axis; no launch per
        part). Then, each once on the batch: gtf_build_events_csr_device, gtf_event_pack,
        gtf_fill_columns and gtf_graph_prepare. The same arrays, carried columns (vivl, event) and
        sizes as the concat, bit for bit; ``n_events`` = len(parts) and ``event_nodes`` the host list of
        the events' node counts (known from the inputs, nothing is read back). Node ids belong to their
        event: the same event twice is legal. Events without nodes or without rows are legal anywhere;
        the synchronisations do not grow with len(parts)."""
        return cls._from_events(parts, device, mem, lambda part: None)

    @classmethod
    def _from_events(cls, parts, device, mem, mark):
        """from_events; mark as _from_event's (tools/batch_build.py)"""
        parts = [tuple(p) for p in parts]
        if any(len(p) != 8 for p in parts):
            raise ValueError("from_events: every part holds from_event's eight columns")
        K = len(parts)
        on_dev = [hasattr(a, "data_ptr") for p in parts for a in p]
        if any(on_dev) and not all(on_dev):
            raise ValueError("from_events: the columns are all host arrays or all device arrays")
        c = cls._event_shell(device, mem)
        INT, FLT = (0, 5, 6, 7), (1, 2, 3, 4)   # (ids, layer_id, row_a, row_b: int64; x, y, z, r: float64)
        if K and on_dev[0]:
            size = lambda a: int(a.numel())  # noqa: E731
        else:
            parts = [tuple(np.ascontiguousarray(a, np.int64 if i in INT else np.float64).reshape(-1)
                           for i, a in enumerate(p)) for p in parts]
            size = lambda a: int(a.size)  # noqa: E731
        for p in parts:
            if any(size(p[i]) != size(p[0]) for i in (1, 2, 3, 4, 5)) or size(p[6]) != size(p[7]):
                raise ValueError("from_events: one x, y, z, r and layer_id per node id, one row_b per row_a")
        # (the rows of an event without nodes name no node of it: every one would be dropped)
        nn = [size(p[0]) for p in parts]
        nr = [size(p[6]) if size(p[0]) else 0 for p in parts]
        node_off = np.concatenate([[0], np.cumsum(nn, dtype=np.int64)]).astype(np.int64)
        row_off = np.concatenate([[0], np.cumsum(nr, dtype=np.int64)]).astype(np.int64)
        N, R = int(node_off[-1]), int(row_off[-1])
        if max(N, 2 * R) > (2 ** 31 - 1) // 2:
            raise ValueError("from_events: the batch is too large for int32 indices")
        if K and on_dev[0]:
            cols = cls._gather_columns(c, parts, nn, nr, N, R) if N else [c._dev_empty(0, np.int64)] * 8
        else:
            cols = [np.concatenate([p[i][:(nr[e] if i > 5 else nn[e])] for e, p in enumerate(parts)])
                    if K else np.zeros(0, np.int64 if i in INT else np.float64) for i in range(8)]
        d = cls._from_event(*cols, device, mem, mark, shell=c,
                            batch=(node_off.astype(np.int32), row_off.astype(np.int32)))
        d.n_events, d.event_nodes = K, nn
        return d

    @classmethod
    def from_fused(cls, cols, node_off, row_off, device: str = "cuda", mem: str = "torch"):
        """from_events for columns that are fused already: ``cols`` holds from_event's eight columns
        (ids, x, y, z, r, layer_id, row_a, row_b) of K events end to end as device arrays, ``node_off``
        and ``row_off`` (host, [K + 1], from 0, not decreasing) say where each event's nodes and rows
        lie -- what io.read_nodes_batch_dev and io.read_edges_batch_dev return. No gather, no copy.
        The rows of an event that keeps no node stay in the row columns (from_events drops them): they
        name no node of their event, so gtf_build_events_csr_device drops every one of them and the
        graph is from_events' graph, bit for bit."""
        cols = tuple(cols)
        if len(cols) != 8 or not all(hasattr(a, "data_ptr") for a in cols):
            raise ValueError("from_fused: from_event's eight columns as device arrays")
        node_off, row_off = (np.ascontiguousarray(o, np.int64).reshape(-1) for o in (node_off, row_off))
        if node_off.size != row_off.size or node_off.size < 1:
            raise ValueError("from_fused: node_off and row_off hold one entry per event and one more")
        for o, a, what in ((node_off, cols[0], "node"), (row_off, cols[6], "row")):
            if o[0] != 0 or (np.diff(o) < 0).any() or int(o[-1]) != int(a.numel()):
                raise ValueError("from_fused: %s_off does not run from 0 to the %s count without decreasing" % (what, what))
        N, R = int(node_off[-1]), int(row_off[-1])
        if max(N, 2 * R) > (2 ** 31 - 1) // 2:
            raise ValueError("from_fused: the batch is too large for int32 indices")
        d = cls._from_event(*cols, device, mem, lambda part: None, shell=cls._event_shell(device, mem),
                            batch=(node_off.astype(np.int32), row_off.astype(np.int32)))
        d.n_events, d.event_nodes = node_off.size - 1, [int(n) for n in np.diff(node_off)]
        return d

    @staticmethod
    def _gather_columns(c, parts, nn, nr, N, R):
        """the eight device columns of every part end to end: gtf_graph_concat with no structure output
        (its offsets: the nodes, and the rows on the slot axis) and gtf_concat_columns"""
        K = len(parts)
        L, vp = c.lib, (lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0))
        adr = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
        for p in parts:
            if any(adr(a) % 8 for a in p):
                raise ValueError("from_events: a device column is not aligned to 8 bytes")
        dst = [c._dev_empty(R if i > 5 else N, np.int64 if i in (0, 5, 6, 7) else np.float64) for i in range(8)]
        ptab = (nat.GtfConcatPart * K)(*[nat.GtfConcatPart(nn[e], nr[e], 0, 0, 0, 0, 0, 0, 0) for e in range(K)])
        pwords = ctypes.sizeof(nat.GtfConcatPart) // 8
        host = np.zeros(K * (pwords + 8), np.int64)
        host[:K * pwords] = np.frombuffer(ptab, np.int64)
        for i in range(8):
            host[K * (pwords + i):K * (pwords + i + 1)] = [adr(p[i]) if (nr[e] if i > 5 else nn[e]) else 0
                                                           for e, p in enumerate(parts)]
        tab = c._dev_from(host)
        nb = int(L.gtf_graph_concat_workspace_bytes(K))
        ws = c._dev_empty(nb, np.uint8)
        hs = (nat.GtfConcatSizes * K)(*[nat.GtfConcatSizes(nn[e], nr[e], 0, 0) for e in range(K)])
        nat.check(L.gtf_graph_concat(hs, ctypes.c_void_p(tab.data_ptr()), K, ctypes.byref(nat.GtfConcatOut()),
                                     vp(ws), ctypes.c_size_t(nb), c.stream))
        cc = (nat.GtfConcatColumn * 8)(*[nat.GtfConcatColumn(tab.data_ptr() + 8 * K * (pwords + i), vp(dst[i]), 8,
                                                             1 if i > 5 else 0) for i in range(8)])
        nat.check(L.gtf_concat_columns(vp(ws), K, N, R, cc, 8, c.stream))
        # the tables and the workspace go out of scope with kernels in flight: a torch allocation is reused
        # in stream order, a plain one is freed at once
        if c.torch is None:
            nat.check(L.gtf_stream_synchronize(None))
        return dst

    @classmethod
    def _from_event(cls, ids, x, y, z, r, layer_id, row_a, row_b, device, mem, mark, shell=None, batch=None):
        """from_event; mark is called with "upload", "csr", "pack_fill" and "prepare" as each part has
        been issued (tools/resident_event.py synchronises and reads the clock there). batch: the
        (node_off, row_off) of from_events, whose columns these are -- the CSR is then
        gtf_build_events_csr_device's and carried["event"] its event column; shell: its _event_shell."""
        if mem not in ("torch", "hip"):
            raise ValueError("mem must be 'torch' or 'hip'")
        on_dev = hasattr(ids, "data_ptr")   # device columns (gtf.io.read_nodes_dev / read_edges_dev)
        if on_dev:
            given = (ids, row_a, row_b, x, y, z, r, layer_id)
            if not all(hasattr(a, "data_ptr") for a in given):
                raise ValueError("from_event: the eight columns are all host arrays or all device arrays")
            N, R = int(ids.numel()), int(row_a.numel())
            if any(int(a.numel()) != N for a in (x, y, z, r, layer_id)) or int(row_b.numel()) != R:
                raise ValueError("from_event: one x, y, z, r and layer_id per node id, one row_b per row_a")
        else:
            ids, layer_id, row_a, row_b = (np.ascontiguousarray(a, np.int64).reshape(-1)
                                           for a in (ids, layer_id, row_a, row_b))
            x, y, z, r = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (x, y, z, r))
            N, R = int(ids.size), int(row_a.size)
            if any(a.size != N for a in (x, y, z, r, layer_id)) or row_b.size != R:
                raise ValueError("from_event: one x, y, z, r and layer_id per node id, one row_b per row_a")
            if N and int(layer_id.min()) < 0:
                raise ValueError("from_event: negative layer_id")
        c = shell if shell is not None else cls._event_shell(device, mem)
        torch = c.torch
        L, vp = c.lib, (lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0))
        E = n_sub = 0
        if batch is not None:
            c.carried["event"] = c._dev_empty(N, np.int32)
        if N:
            up = {k: a if on_dev else c._dev_from(a) for k, a in (("ids", ids), ("a", row_a), ("b", row_b), ("x", x),
                                                                  ("y", y), ("z", z), ("r", r), ("layer_id", layer_id))}
            mark("upload")
            csr = {k: c._dev_empty(n, np.int32) for k, n in (("order", N), ("sub_id", N), ("slot_ptr", N + 1),
                                                              ("slot_src", 2 * R), ("tse_rank", 2 * R),
                                                              ("out_ptr", N + 1), ("out_slot", 2 * R))}
            ev = nat.GtfEventCsr(N, R, vp(up["ids"]), vp(up["a"]), vp(up["b"]),
                                 *[vp(csr[k]) for k in ("order", "sub_id", "slot_ptr", "slot_src", "tse_rank",
                                                        "out_ptr", "out_slot")], 0, 0, 0)
            if batch is None:
                nb = int(L.gtf_build_event_device_workspace_bytes(N, R))
                ws = c._dev_empty(nb, np.uint8)
                nat.check(L.gtf_build_event_csr_device(ctypes.byref(ev), vp(ws), ctypes.c_size_t(nb), c.stream))
            else:
                node_off, row_off = batch
                nb = int(L.gtf_build_events_device_workspace_bytes(N, R, node_off.size - 1))
                ws = c._dev_empty(nb, np.uint8)
                bt = nat.GtfEventBatch(n_events=node_off.size - 1, node_off=node_off.ctypes.data,
                                       row_off=row_off.ctypes.data, event=vp(c.carried["event"]))
                nat.check(L.gtf_build_events_csr_device(ctypes.byref(ev), ctypes.byref(bt), vp(ws),
                                                        ctypes.c_size_t(nb), c.stream))
            E, n_sub = int(ev.n_edges), int(ev.n_subgraphs)
            for k in ("sub_id", "slot_ptr", "out_ptr"):
                c.t[k] = csr[k]
            for k in ("slot_src", "tse_rank", "out_slot"):   # trimmed to the edges the builder kept
                c.t[k] = csr[k][:E] if torch is not None else csr[k].view(0, E, np.int32)
        else:   # no node in the window: nothing to build
            for k, n in (("sub_id", 0), ("slot_ptr", 1), ("out_ptr", 1), ("slot_src", 0), ("tse_rank", 0),
                         ("out_slot", 0)):
                c.t[k] = c._dev_zeros(n, np.int32)
        mark("csr")
        c.n_nodes, c.n_slots, c.n_edges, c.n_sub, c._sub_ok = N, E, E, n_sub, True
        for f in ("gnn", "xyzr", "layer") + MUTABLE_NODE:
            dt, shape, _ = NODE_FIELDS[f]
            c.t[f] = c._dev_empty(N * int(np.prod(shape, dtype=np.int64)), dt)
        for f, (dt, shape, _) in SLOT_FIELDS.items():
            if f not in c.t and f != "slot_key":
                c.t[f] = c._dev_empty(E * int(np.prod(shape, dtype=np.int64)), dt)
        c.t["node_id"] = c._dev_empty(N, np.int64)
        c.t["solo"] = c._dev_empty(N, np.uint8)
        c.carried["vivl"] = c._dev_empty(2 * N, np.float64)
        if N:
            cols = nat.GtfEventCols(vp(up["x"]), vp(up["y"]), vp(up["z"]), vp(up["r"]), vp(up["layer_id"]))
            out = nat.GtfEventOut(c.ptr("gnn"), c.ptr("xyzr"), c.ptr("layer"), c.ptr("node_id"),
                                  vp(c.carried["vivl"]), c.ptr("solo"))
            nat.check(L.gtf_event_pack(ctypes.byref(ev), ctypes.byref(cols), ctypes.byref(out), c.stream))
            for fields, rows, names in ((NODE_FIELDS, N, MUTABLE_NODE),
                                        (SLOT_FIELDS, E, tuple(f for f in SLOT_FIELDS
                                                               if f not in ("slot_key", "slot_src", "tse_rank")))):
                fc = []
                for f in names:
                    dt, shape, fill = fields[f]
                    word = np.full(8 // np.dtype(dt).itemsize, cls.EVENT_FILL.get(f, fill), dtype=dt)
                    fc.append(nat.GtfFillColumn(c.ptr(f), rows, int(np.prod(shape, dtype=np.int64)) * word.itemsize, 0,
                                                int(word.view(np.uint64)[0])))
                if rows:
                    nat.check(L.gtf_fill_columns((nat.GtfFillColumn * len(fc))(*fc), len(fc), c.stream))
            # the uploaded columns, the untrimmed CSR arrays and the builder's workspace go out of scope
            # with kernels in flight: a torch allocation is reused in stream order, a plain one is freed at once
            if torch is None:
                nat.check(L.gtf_stream_synchronize(None))
        mark("pack_fill")
        shape = TrackGraph(N, E, None, None, np.zeros(E, np.int32), {}, {}, n_sub)   # (sizes only)
        if N > 0 and E > 0:
            c._device_tables(shape, None, True)
        else:   # nothing for gtf_graph_prepare to build: the few tables of a slot-free graph from the host
            from .graph import empty_arrays
            zp = np.zeros(N + 1, np.int32)
            solo = c.t["solo"]
            c._host_tables(TrackGraph(N, 0, zp, zp, np.zeros(0, np.int32), empty_arrays(NODE_FIELDS, N),
                                      empty_arrays(SLOT_FIELDS, 0), n_sub), None, True, False)
            c.t["solo"] = solo
        c._finish(shape, False)
        mark("prepare")
        return c

    def host_graph(self):
        """A from_event() graph (or, with the states build_event_dev computes, the event network) as a
        host TrackGraph without a parent: every resident field downloaded, tag = node_id and
        slot_key = node_id[slot_src] (a fresh event has no orphan keys). Returns (graph, vivl [N, 2]).
        to_host(parent) stays the way back for a subset() child."""
        if not getattr(self, "_event", False):
            raise ValueError("host_graph: this DeviceGraph holds no node_id column (only a graph made by "
                             "DeviceGraph.from_event() carries its ids and vivl; a subset() child has to_host(parent))")
        self.materialize()
        N, S = self.n_nodes, self.n_slots
        nid = self._np(self.t["node_id"]).astype(np.int64, copy=False)
        node, slot = {"tag": nid.copy(), "node_id": nid}, {}
        for f, (dt, shape, _) in NODE_FIELDS.items():
            if f not in node:
                node[f] = self._np(self.t[f]).reshape((N,) + shape).astype(dt, copy=False)
        for f, (dt, shape, _) in SLOT_FIELDS.items():
            if f != "slot_key":
                slot[f] = self._np(self.t[f]).reshape((S,) + shape).astype(dt, copy=False)
        src = slot["slot_src"].astype(np.int64)
        if (src < 0).any():
            raise ValueError("host_graph: orphan keys (a subset() child): their ids come from to_host(parent)")
        slot["slot_key"] = nid[src] if S else np.zeros(0, np.int64)
        slot["uts_fresh"] = slot["uts_fresh"] & 1   # (bit 1 is cleared by materialize())
        from .graph import check_layout
        h = TrackGraph(N, S, self._np(self.t["slot_ptr"]), self._np(self.t["out_ptr"]), self._np(self.t["out_slot"]),
                       node, slot, self.n_sub)
        check_layout(h)
        return h, self._np(self.carried["vivl"]).reshape(N, 2)

    def refresh_send_mw(self):
        """gtf.graph.refresh_send_mw on the device (gtf_refresh_send_mw): send_mw of every edge
        from the sender's current tse_mw, NaN where the sender holds no such entry"""
        self._natural_only("refresh_send_mw")
        nat.check(self.lib.gtf_refresh_send_mw(ctypes.byref(self.cg_sched), self.ptr("tse_rank"), self.ptr("tse_mw"),
                                               self.ptr("send_mw"), self.stream))

    def to_host(self, parent: TrackGraph) -> TrackGraph:
        """A subset() child as a host graph: the structure and every device-resident field
        downloaded, the host-only fields (slot_key, node_id, tag) taken from `parent` -- the host
        graph of the DeviceGraph that subset() was called on -- through node_map / slot_map."""
        if "node_map" not in self.t:
            raise ValueError("to_host: only a graph made by DeviceGraph.subset() has the maps to its parent")
        self.materialize()
        N, S = self.n_nodes, self.n_slots
        nm = self._np(self.t["node_map"]).astype(np.int64)
        sm = self._np(self.t["slot_map"]).astype(np.int64)
        if (N and nm.max() >= parent.n_nodes) or (S and sm.max() >= parent.n_slots):
            raise ValueError("to_host: `parent` is not the graph this one was cut from")
        node, slot = {}, {}
        for f, (dt, shape, _) in NODE_FIELDS.items():
            if f in self.t:
                node[f] = self._np(self.t[f]).reshape((N,) + shape).astype(dt, copy=False)
            else:
                node[f] = parent.node[f][nm].copy()
        for f, (dt, shape, _) in SLOT_FIELDS.items():
            if f in self.t:
                slot[f] = self._np(self.t[f]).reshape((S,) + shape).astype(dt, copy=False)
            else:
                slot[f] = parent.slot[f][sm].copy()
        slot["uts_fresh"] = slot["uts_fresh"] & 1   # (bit 1 is cleared by materialize())
        from .graph import check_layout
        h = TrackGraph(N, S, self._np(self.t["slot_ptr"]), self._np(self.t["out_ptr"]), self._np(self.t["out_slot"]),
                       node, slot, self.n_sub)
        check_layout(h)
        return h

    def _natural_only(self, what):
        """node-indexed arrays cross these methods in host order: every layout whose node order
        is a permutation of the host's maps them (the padded layout's dummy nodes do not)"""
        if self.layout == "padded":
            raise NotImplementedError("%s takes node-indexed host arrays: not with layout='padded'" % what)

    def _to_dev_nodes(self, a):
        """a host-order per-node array (numpy) in device node order"""
        a = np.asarray(a)
        return a if self.order is None else a[self.order]

    def _inv_order(self):
        """device tensor: host node h -> device node"""
        if getattr(self, "_inv_t", None) is None:
            inv = np.empty(self.order.size, np.int64)
            inv[self.order] = np.arange(self.order.size)
            self._inv_t = self.torch.from_numpy(inv).to(self.device)
        return self._inv_t

    # arrays whose values decide how much work the next pass does: restoring
    # them makes every benchmark step process the same input
    PASS_INPUTS = ("act", "uts_rank", "has_uts", "has_merged", "merged_state", "merged_cov", "merged_prior")

    def snapshot(self, names=None):
        """device-side copy of mutable arrays (default: every one). The pass inputs
        (PASS_INPUTS) live in one arena and snapshot as a single buffer."""
        self._need_torch("snapshot")
        if names is not None and tuple(names) == tuple(self.PASS_INPUTS):
            return {"__arena__": self.arena.clone()}
        names = names or [k for k in self.t if k in MUTABLE_NODE or
                          (k in SLOT_FIELDS and k not in STATIC_SLOT and k != "slot_key")]
        return {k: self.t[k].clone() for k in names}

    def restore(self, snap):
        """copy a snapshot back (the pass-input arena is one device copy)"""
        if "__arena__" in snap:
            self.arena.copy_(snap["__arena__"], non_blocking=True)
            return
        for k, v in snap.items():
            self.t[k].copy_(v, non_blocking=True)

    # ------------------------------------------------ staged copies of the pass input
    def stage_inputs(self, k: int):
        """k device copies of the pass-input arena (PASS_INPUTS), each with its own C structs,
        for a benchmark whose steps each run one pass over a resident, identical input without
        a restore copy between them: use_inputs(i) points every stage method at copy i
        (None: the arrays of this graph). The arrays outside the arena (state values,
        degree) are shared: a pass overwrites every value it reads back."""
        self._need_torch("stage_inputs")
        if self._resident is None:
            self._resident = (self.cn, self.cuts, self.ctse, self.ce)
        self.use_inputs(None)
        lo = self.arena.data_ptr()
        hi = lo + self.arena.numel()

        def rebase(st, off):
            vals = []
            for name, typ in st._fields_:
                v = getattr(st, name)
                if typ is ctypes.c_void_p and v is not None and lo <= v < hi:
                    v = v + off
                vals.append(v)
            return type(st)(*vals)

        self._staged = []   # (a second call replaces the copies)
        for _ in range(k):
            a = self.torch.empty_like(self.arena)
            off = a.data_ptr() - lo
            self._staged.append((a, tuple(rebase(s, off) for s in self._resident)))

    def fill_inputs(self, snap):
        """copy the pass-input snapshot (snapshot(PASS_INPUTS)) into every staged copy"""
        if "__arena__" not in snap:
            raise ValueError("fill_inputs takes snapshot(DeviceGraph.PASS_INPUTS)")
        for a, _ in self._staged:
            a.copy_(snap["__arena__"], non_blocking=True)

    def use_inputs(self, i):
        """point the stage methods at staged copy i, or back at this graph's arrays (None)"""
        if i is None:
            if self._resident is not None:
                self.cn, self.cuts, self.ctse, self.ce = self._resident
            return
        self.cn, self.cuts, self.ctse, self.ce = self._staged[i][1]
