"""The track-finding loop of run_gnn_trackml_mod.sh (:61-146) on the device.

Reference flow (one process per stage, gpickle directories in between):

    event_conversion  ->  it 1: clustering(track_state_estimates, -c 1.0 -k 2.0) -> extract
                          it 2: extrapolate(-c 2.0) -> extract -> remove_state_metadata(remaining)
                          it 3: clustering(updated_track_states, -c 1000 -k 100) -> extract
                          ... (even: as 2, odd: as 3); each iteration starts from the
                          previous iteration's remaining subgraphs (:140)

Here every stage runs in HBM through the C-ABI on one packed graph per iteration:
the stage and the extraction share one DeviceGraph (the extraction reads the stage's
activation mask in place), and the host only builds the next iteration's graph from
the extraction's verdict (:func:`gtf.graph.subset`, the packed form of
``remove_nodes_from`` + dropping fragments) with the extraction's GNN_Measurement
coordinate mutation (close-proximity merging, extract_track_candidates.py:91-118)
carried over -- or, with ``run(..., resident=True)``, the device does
(:meth:`gtf.device.DeviceGraph.subset`) and the graph stays in HBM from one iteration
to the next.

Event conversion (:func:`build_event`, event_conversion.py:53-101): the packed graph
and its orders come from gtf_build_event_csr (csrc/gtf_build.cpp: the reference's
node, successor and weakly-connected-component orders and the set order of the
track_state_estimates keys, helper.py:277,350-351, without networkx); the states,
priors, mixture weights and degrees are computed on the device
(gtf_track_state_estimates + gtf_node_ops). :func:`build_event_dev` does the same without
leaving HBM (gtf_event_pack, gtf_fill_columns) and returns the DeviceGraph that
``run(d, None, resident="device")`` starts iteration 1 on.
"""
from __future__ import annotations

import dataclasses
import time
from typing import List, Optional

import numpy as np

from . import extract
from .graph import TrackGraph, concat, pack, refresh_send_mw, split_events, subset
from .params import Params

CLUSTER_FIRST = (1.0, 2.0)        # run_gnn_trackml_mod.sh:89  -d track_state_estimates -c 1.0 -k 2.0
CLUSTER_LATER = (1000.0, 100.0)   # run_gnn_trackml_mod.sh:112 -d updated_track_states -c 1000 -k 100


@dataclasses.dataclass
class Iteration:
    """One iteration's outputs as node ids (the reference's candidates/, remaining/,
    fragments/ directories and candidates/pvals.csv)."""
    index: int
    stage: str
    candidates: Optional[List[np.ndarray]]      # (the three lists: None from run(lists=False))
    pval_xy: np.ndarray
    pval_zr: np.ndarray
    remaining: Optional[List[np.ndarray]]
    fragments: Optional[List[np.ndarray]]
    seconds: dict
    network: Optional[TrackGraph] = None      # the stage's output graph (keep_graphs=True)
    remaining_graph: Optional[TrackGraph] = None    # next iteration's input
    remaining_vivl: Optional[np.ndarray] = None
    counts: Optional[dict] = None             # resident="device": gtf_extract_out_counts' six counts


ON_ERROR = ("raise", "name", "isolate")


@dataclasses.dataclass
class EventError:
    """The reference exception that ended one event of a batch (run_batch / build_events_dev with
    on_error="isolate"): where the loop was and what DeviceGraph.event_errors says of the event."""
    iteration: int          # 0: event conversion (build_events_dev)
    stage: str              # the stage string of the iteration's records, or "update"
    flags: int              # the event's GTF_ERR_* bits
    messages: List[str]
    first_node_id: int      # the node id of the event's first raising node
    n_raising: int          # how many of its nodes raised


class BatchRecords(list):
    """run_batch's list of K record lists; ``errors`` = {event: EventError} of the events cut out"""

    def __init__(self, *a):
        super().__init__(*a)
        self.errors = {}


class BatchError(ValueError):
    """on_error="name": raise_errors' exception with the failing events; ``events`` = {event: flags}"""

    def __init__(self, msg, events):
        super().__init__(msg)
        self.events = events


def _check_on_error(on_error):
    if on_error not in ON_ERROR:
        raise ValueError("on_error must be 'raise', 'name' or 'isolate'")


def _cut_failed(d, K, flags, on_error, iteration, stage, errors):
    """the error word of d's workspace is ``flags`` != 0: name the raising events (DeviceGraph.event_errors)
    and, on_error "isolate", record them in ``errors`` and cut them out of d. Returns (the child, the
    events cut). "name", or bits that no node recorded: raises."""
    from . import _native as nat
    messages = lambda f: [m for b, m in nat.ERR_FLAGS.items() if f & b]  # noqa: E731
    lead = "reference exception reproduced on device: " + "; ".join(messages(flags))
    r = d.event_errors(n_events=K)
    failed = [int(e) for e in np.flatnonzero(r["err_ev"])]
    if flags & ~int(np.bitwise_or.reduce(r["err_ev"], initial=np.uint32(0))):
        raise ValueError(lead)   # (raised outside the per-node path: no event to name)
    if on_error == "name":
        raise BatchError(lead + " -- " + "; ".join("event %d: %s; node id %d" % (
            e, "; ".join(messages(int(r["err_ev"][e]))), int(r["first_id"][e])) for e in failed),
            {e: int(r["err_ev"][e]) for e in failed})
    for e in failed:
        f = int(r["err_ev"][e])
        errors[e] = EventError(iteration, stage, f, messages(f), int(r["first_id"][e]), int(r["n_raising"][e]))
    child = d.subset(r["keep"], carry={"vivl": d.carried["vivl"], "event": d.carried["event"]}, keep_fresh=True)
    return child, failed


def event_layout(event_prefix: str, min_volume: int, max_volume: int, builder: str = "native", device="cuda"):
    """Host half of event conversion: the packed network in the reference's orders,
    with empty track_state_estimates dicts keyed in their set order and every edge
    active (helper.initialize_edge_activation). Returns (graph, vivl[N, 2]).

    builder "native": gtf_build_event_csr (C++, CSV rows -> CSR, CPython set orders
    reproduced); "device": gtf_build_event_csr_device (the same build on the GPU, the
    same arrays); "networkx": the reference's own construction through networkx and
    pack() (gtf.io.build_networkx) -- the slow path the native one is tested against."""
    from . import io
    if builder == "native":
        return io.build_event_csr(event_prefix, min_volume, max_volume)
    if builder == "device":
        return io.build_event_csr(event_prefix, min_volume, max_volume, device=device)
    if builder != "networkx":
        raise ValueError("builder must be 'native', 'device' or 'networkx'")
    import networkx as nx
    subs = io.build_networkx(event_prefix, min_volume, max_volume)
    for G in subs:
        for node in G.nodes():
            keys = list(set(nx.all_neighbors(G, node)))
            keys.reverse()
            G.nodes[node]["track_state_estimates"] = {k: {} for k in keys}
    g = pack(subs)
    vivl = np.array([(G.nodes[n]["volume_id"], G.nodes[n]["in_volume_layer_id"]) for G in subs for n in G.nodes],
                    dtype=np.float64).reshape(-1, 2)
    return g, vivl


def build_event(event_prefix: str, min_volume: int, max_volume: int, p: Params = None, device="cuda",
                builder: str = "device", tables: str = "host"):
    """event_conversion.py:53-101: CSVs -> packed network with track_state_estimates,
    activation 1, priors, mixture weights and degrees, all on the GPU (the graph build by
    gtf_build_event_csr_device; builder "native" for the host C++ one, the same arrays).
    tables: DeviceGraph's ("device": the schedules and slot tables by gtf_graph_prepare).
    Returns (graph, vivl[N, 2])."""
    from .device import DeviceGraph
    p = p or Params()
    g, vivl = event_layout(event_prefix, min_volume, max_volume, builder, device)
    if g.n_nodes == 0:
        return g, vivl
    d = DeviceGraph(g, device, tables=tables)
    d.clear_errors()
    d.track_state_estimates(p)
    d.node_ops(["priors_tse", "mw_tse", "degree"], p)
    d.raise_errors()
    d.download(g)
    refresh_send_mw(g)
    return g, vivl


def build_event_dev(event_prefix: str, min_volume: int, max_volume: int, p: Params = None, device="cuda",
                    mem: str = "torch", parse: str = "host"):
    """build_event (event_conversion.py:53-101) without its host round trips: the parsed CSV columns go
    up once and the packed network, its empty states and its tables are made in HBM
    (DeviceGraph.from_event: gtf_build_event_csr_device, gtf_event_pack, gtf_fill_columns,
    gtf_graph_prepare); the states, priors, mixture weights, degrees and send weights are computed on
    that object. Returns the DeviceGraph: run(d, None, resident="device") starts iteration 1 on it,
    d.host_graph() downloads what build_event returns.
    parse: "host" (io.read_nodes / read_edges, the definition) or "device": the files' bytes go up and
    gtf_csv_parse, gtf_event_window and gtf_event_radius_patch make the same columns there
    (io.read_nodes_dev / read_edges_dev). A file with a field outside the device parser's exact
    domain (csvdev.OutOfDomain) is read by the host reader instead; ``d.parse_info`` says which
    parser read each file ({"nodes": "device" | "host", "edges": ...}, with "nodes_reason" /
    "edges_reason" after a fallback). The same graph either way, bit for bit."""
    from .device import DeviceGraph
    p = p or Params()
    cols, info = _event_columns(event_prefix, min_volume, max_volume, device, mem, parse)
    d = DeviceGraph.from_event(*cols, device, mem)
    d.parse_info = info
    return _event_states(d, p)


def _event_columns(event_prefix, min_volume, max_volume, device, mem, parse):
    """from_event's eight columns of one event's files, by the host readers or the device parser
    (build_event_dev's ``parse``), and which parser read each file"""
    from . import io
    if parse not in ("host", "device"):
        raise ValueError("parse must be 'host' or 'device'")
    info = {"nodes": "host", "edges": "host"}
    if parse == "host":
        ids, x, y, z, r, layer = io.read_nodes(event_prefix + "nodes.csv", min_volume, max_volume)
        n2, n1 = io.read_edges(event_prefix + "edges.csv")
    else:
        from .csvdev import OutOfDomain
        from .metrics import _Mem
        mm = _Mem(device, mem)
        try:
            nd = io.read_nodes_dev(event_prefix + "nodes.csv", min_volume, max_volume, device, mem)
            ids, x, y, z, r, layer = nd.ids, nd.x, nd.y, nd.z, nd.r, nd.layer_id
            info["nodes"] = "device"
        except OutOfDomain as e:
            info["nodes_reason"] = str(e)
            host = io.read_nodes(event_prefix + "nodes.csv", min_volume, max_volume)
            if host[0].size and int(host[5].min()) < 0:
                raise ValueError("from_event: negative layer_id")
            ids, x, y, z, r, layer = (mm.from_host(a) for a in host)
        try:
            n2, n1, _ = io.read_edges_dev(event_prefix + "edges.csv", device, mem)
            info["edges"] = "device"
        except OutOfDomain as e:
            info["edges_reason"] = str(e)
            n2, n1 = (mm.from_host(a) for a in io.read_edges(event_prefix + "edges.csv"))
    return (ids, x, y, z, r, layer, n1, n2), info


def _event_states(d, p, on_error="raise"):
    """the states, priors, mixture weights, degrees and send weights of a fresh from_event /
    from_events graph (event_conversion.py:86-101), on that object. on_error (a fused graph):
    build_events_dev's"""
    if on_error != "raise":
        d.event_error_records = {}
    if d.n_nodes == 0:
        return d
    d.clear_errors()
    if on_error != "raise":
        d.track_node_errors()
    d.track_state_estimates(p)
    d.node_ops(["priors_tse", "mw_tse", "degree"], p)
    if on_error == "raise":
        d.raise_errors()
    else:
        flags = d.errors()
        if flags:
            records = {}
            c, failed = _cut_failed(d, d.n_events, flags, on_error, 0, "event_conversion", records)
            # the child stands in for the fused graph: whole events left, so no orphan key and the ids
            # and vivl resident (host_graph); the events cut hold no node
            c._event, c.parse_info, c.event_error_records = True, getattr(d, "parse_info", None), records
            c.event_nodes = [0 if e in records else n for e, n in enumerate(d.event_nodes)]
            d = c
            if d.n_nodes == 0:
                return d
    d.refresh_send_mw()
    return d


def build_events_dev(prefixes, min_volume: int, max_volume: int, p: Params = None, device="cuda",
                     mem: str = "torch", parse: str = "host", batch_parse: bool = False, on_error: str = "raise"):
    """build_event_dev for a batch of events in ONE build: every event's files are read as
    build_event_dev reads them (the device parse and its per-file host fallback stay per file;
    ``parse_info`` is the list of the events' records), DeviceGraph.from_events makes the fused graph --
    what DeviceGraph.concat of the events' build_event_dev graphs holds, bit for bit -- and the states,
    priors, mixture weights, degrees and send weights are computed ONCE on it. run_batch(d) runs the
    loop on it without a concat; d.n_events and d.event_nodes say how it divides.
    batch_parse (with parse="device"): the CSV front end is per batch too -- all nodes.csv in one
    gtf_csv_parse_ev, one gtf_event_window_ev and one radius patch (io.read_nodes_batch_dev), all
    edges.csv in one more parse (io.read_edges_batch_dev) -- and the fused columns go to
    DeviceGraph.from_fused without a gather. The same graph, bit for bit; ``parse_info`` is again one
    record per event, with "batch": the ParsedBatch infos of the two kinds.
    on_error: what a reference exception in the states' kernels does, as in run_batch. "raise" (default):
    DeviceGraph.raise_errors on the fused graph's error word. "name": the same exception as a BatchError
    that names the failing events. "isolate": the failing events are cut out of the returned graph
    (their ``event_nodes`` entry is 0, the others' nodes are untouched) and ``d.event_error_records`` =
    {event: EventError} with iteration 0; it is empty on a clean build."""
    from .device import DeviceGraph
    p = p or Params()
    _check_on_error(on_error)
    if batch_parse:
        if parse != "device":
            raise ValueError("batch_parse needs parse='device'")
        from . import io
        prefixes = list(prefixes)
        nd = io.read_nodes_batch_dev([q + "nodes.csv" for q in prefixes], min_volume, max_volume, device, mem)
        n2, n1, row_off, ed = io.read_edges_batch_dev([q + "edges.csv" for q in prefixes], device, mem)
        d = DeviceGraph.from_fused((nd.ids, nd.x, nd.y, nd.z, nd.r, nd.layer_id, n1, n2), nd.node_off, row_off, device, mem)
        d.parse_info = []
        for e in range(len(prefixes)):
            info = {"nodes": nd.files[e], "edges": ed.files[e], "batch": {"nodes": nd.parse, "edges": ed.info}}
            if nd.reasons[e]:
                info["nodes_reason"] = nd.reasons[e]
            if ed.reasons[e]:
                info["edges_reason"] = ed.reasons[e]
            d.parse_info.append(info)
        return _event_states(d, p, on_error)
    read = [_event_columns(prefix, min_volume, max_volume, device, mem, parse) for prefix in prefixes]
    d = DeviceGraph.from_events([cols for cols, _ in read], device, mem)
    d.parse_info = [info for _, info in read]
    return _event_states(d, p, on_error)


def _ids(g: TrackGraph, groups):
    return [g.node["node_id"][np.asarray(x, np.int64)] for x in groups]


def _dev_slice(d, t, start: int, n: int):
    """n elements of the device array t from element `start` on (a view, no copy)"""
    if d.torch is not None:
        return t[start:start + n]
    return t.view(start * t.dtype.itemsize, n, t.dtype)


def run_batch(ds, iterations: int = 3, p: Params = None, ex: extract.Params = None, scorers=None,
              lists: bool = True, first: int = 1, keep_graphs: bool = False,
              on_error: str = "raise") -> List[List[Iteration]]:
    """run(d, None, resident="device") for K resident events at once: ``ds`` (the DeviceGraphs of
    build_event_dev, one allocator and device) are fused by DeviceGraph.concat and the loop runs ONCE on
    the fused graph, so the synchronisations of an iteration -- the connected-components rounds, the
    counts read-backs, the subset plan -- are paid per batch instead of per event. Subgraphs of
    different events share no edge: every stage, the extraction and the node removal compute on the
    fused graph what they compute on each event, and gtf_event_split (extract.split_dev) takes each
    iteration's candidates, p-values, remaining and fragment groups and counts apart again. The event
    column travels through subset() as a carried column. Returns one List[Iteration] per event, equal
    to run()'s on that event alone: the same records, and as many -- an event's list ends at the first
    iteration it enters with no node left, as run() breaks. ``seconds`` are the batch's.
    scorers: None, or one metrics.DeviceScorer (or None) per event; scorers[e] receives event e's
    candidates of every iteration, group = (first + iterations - 1) - it as in run(); or ONE object with
    an add_batch method (metrics.BatchScorer), which gets one call per iteration for the whole batch:
    add_batch(cand_ptr, cand_ids, cand_first_dev, n_extracted, group, n_members=..., active=[the events
    that entered the iteration with nodes]) on the fused graph's own device arrays. lists=False: no
    node-id list crosses to the host. The input graphs are not modified.
    keep_graphs: every record also holds the event's stage output, remaining graph and remaining vivl
    (what run_pipeline.py saves), cut on the host (graph.split_events) from downloads of the fused
    graphs after each step -- as in run(), a record's remaining_graph ends holding the next stage's
    output and merged coordinates.
    on_error: what a reference exception in one event does to the batch.
    "raise" (default): DeviceGraph.raise_errors on the fused graph's error word, as run() raises; the
    word is the batch's, so the message does not say which event, and no record is returned.
    "name": the same exception as a BatchError whose text goes on with "event e: <its messages>; node id
    <its first raising node>" for every failing event; ``.events`` = {e: flags}.
    "isolate": the batch behaves as the per-event loop does. Every stage and update() runs with a per-node
    error array registered (DeviceGraph.track_node_errors: one zero fill, nothing else while the error
    word stays 0). When the word is set, gtf_event_errors names the raising events and
    subset(keep of the others) cuts them out BEFORE candidate order and extraction, so nothing reads a
    raised event's half-written state; events share no edge, so the child is the fused graph of the
    survivors, whose records stay those of run() on each alone. A failed event's list ends with its last
    clean iteration (a failure in the update() after iteration 2 keeps iteration 2's record), scorers see
    it as an event that ran out of nodes from then on, keep_graphs cuts the host copy in step, and the
    returned list (a BatchRecords) holds ``errors`` = {e: EventError(iteration, stage, flags, messages,
    first_node_id, n_raising)}, stage "update" for update(); empty on a clean run. Bits in the error
    word that no node recorded raise as "raise" does.
    ``ds`` may also be ONE fused graph as build_events_dev returns it (DeviceGraph.from_events: it holds
    ``event_nodes``): the loop starts on it without a concat, the events' node counts are its
    ``event_nodes`` and keep_graphs takes its own host_graph(). The same records; iteration ``first``
    runs on that object, as run() runs on a DeviceGraph input."""
    from .device import DeviceGraph
    p = p or Params()
    ex = ex or extract.Params()
    _check_on_error(on_error)
    track = on_error != "raise"
    fused = ds if isinstance(ds, DeviceGraph) else None
    if fused is not None and not hasattr(fused, "event_nodes"):
        raise ValueError("run_batch takes a list of resident events or one fused graph of build_events_dev")
    ds = [fused] if fused is not None else list(ds)
    K = fused.n_events if fused is not None else len(ds)
    batch_scorer = scorers if hasattr(scorers, "add_batch") else None
    if batch_scorer is not None:
        scorers = None
    if scorers is not None and len(scorers) != K:
        raise ValueError("scorers must hold one entry (a DeviceScorer or None) per event")
    for g in ds:
        if not isinstance(g, DeviceGraph):
            raise ValueError("run_batch takes resident events (the DeviceGraphs of build_event_dev)")
        if "node_id" not in g.t or "vivl" not in getattr(g, "carried", {}):
            raise ValueError("a DeviceGraph input must hold the node_id and vivl columns (DeviceGraph.from_event)")
    out = BatchRecords([] for _ in range(K))   # (a list of K lists; .errors stays empty unless on_error="isolate" cuts)
    if K == 0:
        return out
    t0 = time.perf_counter()
    d = fused if fused is not None else DeviceGraph.concat(ds)
    # the nodes every event enters the iteration with
    left = list(fused.event_nodes) if fused is not None else [g.n_nodes for g in ds]
    if fused is not None:
        G = fused.host_graph()[0] if keep_graphs else None
    else:
        G = concat([g.host_graph()[0] for g in ds]) if keep_graphs else None   # the fused graph's host copy
    last = first + iterations - 1
    for it in range(first, first + iterations):
        if d.n_nodes == 0:
            break
        if it > first:
            t0 = time.perf_counter()
        torch = d.torch
        d.clear_errors()
        if track:
            d.track_node_errors()
        if it == 1:
            stage = "clustering(track_state_estimates)"
            d.cluster("tse", CLUSTER_FIRST[0], CLUSTER_FIRST[1], p)
        elif it % 2 == 0:
            stage = "extrapolation"
            d.extrapolate(p)
        else:
            stage = "clustering(updated_track_states)"
            d.cluster("uts", CLUSTER_LATER[0], CLUSTER_LATER[1], p)
        if not track:
            d.raise_errors()
        else:
            flags = d.errors()
            if flags:   # the raising events leave before anything reads the stage's output
                d, failed = _cut_failed(d, K, flags, on_error, it, stage, out.errors)
                for e in failed:
                    left[e] = 0
                if keep_graphs:
                    G = d.to_host(G)
                if d.n_nodes == 0:
                    break
        if torch is not None:
            torch.cuda.synchronize(d.device)
        t1 = time.perf_counter()
        vivl_dev, event_dev = d.carried["vivl"], d.carried["event"]
        order = extract.candidate_order_dev(d)
        res = extract.run_dev(d, vivl_dev, ex, order)
        t2 = time.perf_counter()
        o = extract.outputs_dev(d, res, ex.numhits, ids=True, lists=False, members=True)
        sp = extract.split_dev(d, o, K)
        fc, fr, ff = (sp["first"][k] for k in ("cand", "rem", "frag"))
        if batch_scorer is not None:   # one call for the batch: the fused graph's own arrays
            batch_scorer.add_batch(o["cand_ptr"], o["cand_ids"], sp["cand_first_dev"], o["counts"]["n_extracted"],
                                   last - it, n_members=o["counts"]["n_extracted_nodes"],
                                   active=[left[e] > 0 for e in range(K)])
        if scorers is not None:
            at = 0   # event e's members start where the events before it end
            for e in range(K):
                ce = sp["counts"][e]
                if scorers[e] is not None and left[e] > 0:
                    scorers[e].add(_dev_slice(d, sp["cand_ptr_ev"], int(fc[e]) + e, ce["n_extracted"] + 1),
                                   _dev_slice(d, o["cand_ids"], at, ce["n_extracted_nodes"]), ce["n_extracted"],
                                   last - it, n_members=ce["n_extracted_nodes"])
                at += ce["n_extracted_nodes"]
        n_ext = o["counts"]["n_extracted"]
        if lists:
            h = extract.outputs_host(d, o)
        else:   # (the p-values are per candidate, not lists of node ids: they come back)
            h = {k: d._np(_dev_slice(d, o[k], 0, n_ext)) if n_ext else np.empty(0, np.float64)
                 for k in ("pval_xy", "pval_zr")}
        dnext = d.subset(o["keep"], gnn=res["gnn"], carry={"vivl": vivl_dev, "event": event_dev})
        dnext.refresh_send_mw()
        update_flags = 0
        if it % 2 == 0 and dnext.n_nodes:      # remove_state_metadata.py, as in run()
            dnext.clear_errors()
            if track:
                dnext.track_node_errors()
            dnext.update(p)
            if track:
                update_flags = dnext.errors()
            else:
                dnext.raise_errors()
        t3 = time.perf_counter()
        seconds = {"stage": t1 - t0, "extract": t2 - t1, "next": t3 - t2}
        if keep_graphs:   # after the step (it left d's arrays as the stage wrote them), as in run()
            ev = d._np(event_dev)
            nets = split_events(d.download(G), ev, K)
            G.node["gnn"] = d._np(res["gnn"]).reshape(-1, 4)
            for e, part in enumerate(split_events(G, ev, K)):   # the iteration's input graphs, as run() leaves them
                if out[e] and left[e] > 0:
                    out[e][-1].remaining_graph = part
            G = dnext.to_host(G)
            ev2 = d._np(dnext.carried["event"])
            rems, vivl2 = split_events(G, ev2, K), d._np(dnext.carried["vivl"]).reshape(-1, 2)
            cut = np.searchsorted(ev2, np.arange(K + 1))
        for e in range(K):
            if left[e] == 0:
                continue
            c0, c1 = int(fc[e]), int(fc[e + 1])
            grp = (lambda key, a, b: h[key][a:b]) if lists else (lambda key, a, b: None)
            out[e].append(Iteration(it, stage, grp("extracted", c0, c1), h["pval_xy"][c0:c1], h["pval_zr"][c0:c1],
                                    grp("remaining", int(fr[e]), int(fr[e + 1])),
                                    grp("fragments", int(ff[e]), int(ff[e + 1])), dict(seconds),
                                    counts=dict(sp["counts"][e])))
            if keep_graphs:
                rec = out[e][-1]
                rec.network, rec.remaining_graph, rec.remaining_vivl = nets[e], rems[e], vivl2[cut[e]:cut[e + 1]]
            left[e] = sp["counts"][e]["n_remaining_nodes"]
        if update_flags:   # update() raised: this iteration's records stand, the raising events end here
            dnext, failed = _cut_failed(dnext, K, update_flags, on_error, it, "update", out.errors)
            for e in failed:
                left[e] = 0
            if keep_graphs:
                G = dnext.to_host(G)
        d = dnext
    return out


def run(g, vivl, iterations: int = 3, p: Params = None, ex: extract.Params = None,
        device="cuda", first: int = 1, keep_graphs: bool = False, tables: str = "host",
        resident=False, host: TrackGraph = None, scorer=None, lists: bool = True) -> List[Iteration]:
    """Iterations ``first`` .. ``first + iterations - 1`` of the loop, starting from
    the stage input ``g`` (the event network for iteration 1). Stops early when
    nothing remains. keep_graphs: also return each iteration's stage output and
    remaining graphs (for saving, gtf.store). tables: passed to every DeviceGraph ("device":
    the schedules and slot tables by gtf_graph_prepare instead of the host builders).
    resident: the next iteration's graph is cut on the device -- DeviceGraph.subset(keep,
    gnn=merged coordinates) and refresh_send_mw() (gtf_graph_subset_plan / _apply,
    gtf_subset_gather, gtf_refresh_send_mw) instead of graph.subset + refresh_send_mw on the
    host and a fresh upload; an even iteration's update() runs on that object, and the next
    iteration's stage reuses it. The candidate order and the stage outputs
    (extract.candidate_order, extract.outputs) stay on the host, so the download after every
    stage stays, and the next iteration's host graph is the child's to_host(): what this mode
    removes is the host subset, the host refresh, the re-upload and the second DeviceGraph of
    even iterations. Same results, array for array.
    resident="device": the candidate order and the stage outputs run on the device as well
    (extract.candidate_order_dev / run_dev / outputs_dev: gtf_candidate_order_device,
    gtf_extract_candidates on the DeviceGraph's own buffers, gtf_extract_outputs), the keep mask
    goes to DeviceGraph.subset without leaving HBM, and vivl and node_id travel as carried node
    columns. No download, no host order or outputs, no to_host: per iteration the host receives
    the counts, the candidate / remaining / fragment node-id lists and the p-values (and, with
    keep_graphs, the graphs it asked for, downloaded after the step). Same Iteration records.
    g may then be the DeviceGraph of build_event_dev, with vivl=None: iteration ``first`` runs on that
    object (no upload at all), vivl is its carried column, and keep_graphs takes the host copy it needs
    from host_graph() -- or from ``host``, where the caller already holds that download (it is
    modified like a host ``g``). Any other ``resident`` with such an input raises ValueError, and so
    does ``host`` with a host ``g``.
    scorer, lists (resident="device" only; anything else raises ValueError): scorer, a
    metrics.DeviceScorer, receives every iteration's candidates as the device arrays of
    gtf_extract_outputs -- scorer.add(cand_ptr, cand_ids, n, group) with group = (first +
    iterations - 1) - it, so its result() is reconstruction_efficiency over the candidates of the
    iterations last, ..., first, as the reference reads them. lists=False: no node-id list crosses to
    the host; the records' candidates / remaining / fragments are None, their p-values stay, and
    ``counts`` holds the six counts (it does with lists=True as well)."""
    from .device import DeviceGraph
    p = p or Params()
    ex = ex or extract.Params()
    if resident not in (False, True, "device"):
        raise ValueError("resident must be False, True or 'device'")
    if resident != "device" and (scorer is not None or not lists):
        raise ValueError("scorer and lists=False need resident='device' (the other modes build the lists on the host)")
    out = []
    torch = None
    dnext = None   # resident: the DeviceGraph that already holds the iteration's input
    vivl_dev = None   # resident="device": vivl beside it
    if isinstance(g, DeviceGraph):
        # a resident event (build_event_dev): iteration `first` runs on the object itself
        if resident != "device":
            raise ValueError("a DeviceGraph input needs resident='device' (the other modes start from a host graph)")
        if vivl is not None:
            raise ValueError("a DeviceGraph input carries its own vivl (carried['vivl']): pass vivl=None")
        if "node_id" not in g.t or "vivl" not in getattr(g, "carried", {}):
            raise ValueError("a DeviceGraph input must hold the node_id and vivl columns (DeviceGraph.from_event)")
        dnext, vivl_dev = g, g.carried["vivl"]
        if host is not None and (host.n_nodes, host.n_slots) != (g.n_nodes, g.n_slots):
            raise ValueError("host must be the DeviceGraph input's own host_graph()")
        # (only the saved graphs need a host copy)
        g = (host if host is not None else dnext.host_graph()[0]) if keep_graphs else None
    else:
        if host is not None:
            raise ValueError("host goes with a DeviceGraph input only")
        vivl = np.asarray(vivl, np.float64).reshape(-1, 2)
        if vivl.shape[0] != g.n_nodes:
            raise ValueError("vivl must have one row per node")
    for it in range(first, first + iterations):
        if (dnext.n_nodes if resident == "device" and dnext is not None else g.n_nodes) == 0:
            break
        t0 = time.perf_counter()
        d = dnext if dnext is not None else DeviceGraph(g, device, tables=tables)
        dnext = None
        torch = d.torch
        d.clear_errors()
        if it == 1:
            stage = "clustering(track_state_estimates)"
            d.cluster("tse", CLUSTER_FIRST[0], CLUSTER_FIRST[1], p)
        elif it % 2 == 0:
            stage = "extrapolation"
            d.extrapolate(p)
        else:
            stage = "clustering(updated_track_states)"
            d.cluster("uts", CLUSTER_LATER[0], CLUSTER_LATER[1], p)
        d.raise_errors()
        torch.cuda.synchronize(d.device)
        t1 = time.perf_counter()
        if resident == "device":
            if vivl_dev is None:
                vivl_dev = d._dev_from(vivl)
            order = extract.candidate_order_dev(d)
            res = extract.run_dev(d, vivl_dev, ex, order)
            t2 = time.perf_counter()
            o = extract.outputs_dev(d, res, ex.numhits, ids=True, lists=False)
            counts = o["counts"]
            if scorer is not None:
                scorer.add(o["cand_ptr"], o["cand_ids"], counts["n_extracted"], (first + iterations - 1) - it,
                           n_members=counts["n_extracted_nodes"])
            if lists:
                o = extract.outputs_host(d, o)
            else:   # (the p-values are per candidate, not lists of node ids: they come back)
                o = dict(o, extracted=None, remaining=None, fragments=None,
                         **{k: d._np(o[k][:counts["n_extracted"]]) for k in ("pval_xy", "pval_zr")})
            dnext = d.subset(o["keep"], gnn=res["gnn"], carry={"vivl": vivl_dev})
            dnext.refresh_send_mw()
            if it % 2 == 0 and dnext.n_nodes:      # remove_state_metadata.py, as below
                dnext.clear_errors()
                dnext.update(p)
                dnext.raise_errors()
            t3 = time.perf_counter()
            rec = Iteration(it, stage, o["extracted"], o["pval_xy"], o["pval_zr"], o["remaining"], o["fragments"],
                            {"stage": t1 - t0, "extract": t2 - t1, "next": t3 - t2}, counts=counts)
            vivl_dev = dnext.carried["vivl"]
            if keep_graphs:
                # after the step (it left d's arrays as the stage wrote them). As the other modes:
                # the iteration's input graph (the previous record's remaining_graph) ends holding
                # the stage's output and the merged coordinates
                net = d.download(g).copy()
                g.node["gnn"] = d._np(res["gnn"]).reshape(-1, 4)
                g = dnext.to_host(g)
                rec.network, rec.remaining_graph = net, g
                rec.remaining_vivl = d._np(vivl_dev).reshape(-1, 2)
            out.append(rec)
            continue
        d.download(g)
        order = extract.candidate_order(g)            # members in the reference's candidate order
        res = extract.run(g, vivl, ex, order_key=order, d=d)
        t2 = time.perf_counter()
        o = extract.outputs(g, res, ex.numhits, order)
        net = g.copy() if keep_graphs else None       # the stage's output, before the merging mutation
        keep = np.zeros(g.n_nodes, bool)
        for r in o["remaining"]:
            keep[r] = True
        g.node["gnn"] = res["gnn"]                 # GNN_Measurement mutated in place by merging
        if resident:
            dnext = d.subset(keep, gnn=res["gnn"])
            dnext.refresh_send_mw()
            if it % 2 == 0 and dnext.n_nodes:      # remove_state_metadata.py, as below
                dnext.clear_errors()
                dnext.update(p)
                dnext.raise_errors()
            nxt = dnext.to_host(g)
        else:
            nxt = subset(g, keep)
            refresh_send_mw(nxt)
        if not resident and it % 2 == 0 and nxt.n_nodes:
            # remove_state_metadata.py on the remaining directory (run_gnn_trackml_mod.sh:137-139)
            du = DeviceGraph(nxt, device, tables=tables)
            du.clear_errors()
            du.update(p)
            du.raise_errors()
            du.download(nxt)
        t3 = time.perf_counter()
        rec = Iteration(it, stage, _ids(g, o["extracted"]), o["pval_xy"], o["pval_zr"],
                        _ids(g, o["remaining"]), _ids(g, o["fragments"]),
                        {"stage": t1 - t0, "extract": t2 - t1, "next": t3 - t2})
        if keep_graphs:
            rec.network, rec.remaining_graph, rec.remaining_vivl = net, nxt, vivl[keep]
        out.append(rec)
        g, vivl = nxt, vivl[keep]
    return out
