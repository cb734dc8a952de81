"""Physics metrics of the extracted candidates: track reconstruction
efficiency and track / particle purities, as src/extract/reconstruction_efficiency.py
computes them, vectorised over arrays (candidate member lists in CSR form, the hit
mapping as columns) instead of pandas row lookups per particle and per candidate.

Reference flow (reconstruction_efficiency.py):
  * reference tracks (:41-91): particles with pT = hypot(px, py) >= 1 GeV (:44-47);
    their hits within [min_volume, max_volume] (:50-59); a particle is a reference
    track when its hits span >= 4 distinct (volume_id, layer_id) (:66-78) and no two
    of them share (volume_id, layer_id, module_id) (:79-81);
  * per candidate, in file order (:118-183): the particle ids of its nodes'
    hit_dissociation, nodes in the candidate's node order and hits in each node's order
    (:125-131); the reconstructed particle = the most frequent id, ties to the id seen
    first (max over a Counter, :132-134); n_good its count;
  * matched when the particle is a reference track, n_good >= 0.5 * its reference hits
    (:150), and track purity n_good / #ids >= 0.5 and particle purity n_good / its hits
    in the region >= 0.5 (:154-163); a particle counts once, at its first matching
    candidate (:166-171);
  * efficiency = reconstructed * 100 / reference tracks, printed with 3 decimals (:213).

A node's hit_dissociation is construct_graph's (helper.py:466-479): the node's unique
hit ids in mapping-row order and each hit's particle id.

Two paths, the same numbers. :func:`reconstruction_efficiency` is host-side NumPy over
candidate lists: integer counting, enough for the ~10^3 candidates of one volume.
:class:`DeviceScorer` scores the resident loop's candidates where they are: the device
arrays of gtf_extract_outputs go into gtf_score_candidates (csrc/gtf_score.hip), once per
iteration, against the event's static tables (:func:`truth_tables`) uploaded once, and
gtf_score_finish returns the matched particles in match order; no candidate list crosses
to the host. :func:`truth_tables_dev` builds those tables on the device as well
(gtf_truth_build, csrc/gtf_truth.hip), from the columns uploaded once: the same arrays.
For a batch of events :func:`truth_tables_batch_dev` builds the tables of all of them in one call
(gtf_truth_build_ev, csrc/gtf_truth.hip): what truth_concat_dev of the per-event tables leaves.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Dict, Optional, Sequence

import numpy as np

PT_CUT = 1.0                  # reconstruction_efficiency.py:46
NUM_DISTINCT_LAYERS = 4       # :66


@dataclasses.dataclass
class HitMapping:
    """Columns of the event's hit mapping (event_truth/*-full-mapping-*.csv)."""
    node_idx: np.ndarray
    hit_id: np.ndarray
    particle_id: np.ndarray
    volume_id: np.ndarray
    layer_id: np.ndarray
    module_id: np.ndarray

    @classmethod
    def from_frame(cls, df):
        return cls(*(df[c].to_numpy(np.int64) for c in ("node_idx", "hit_id", "particle_id", "volume_id",
                                                        "layer_id", "module_id")))


@dataclasses.dataclass
class Result:
    n_reconstructed: int
    n_reference: int
    track_purities: np.ndarray       # one per reconstructed particle, in match order
    particle_purities: np.ndarray
    reconstructed_pid: np.ndarray    # per candidate: majority particle id
    n_good: np.ndarray               # per candidate: its count
    matched: np.ndarray              # per candidate: counted as a reconstruction (first match)

    @property
    def efficiency(self) -> float:
        return self.n_reconstructed * 100 / self.n_reference

    @property
    def efficiency_str(self) -> str:
        return "{:.3f}".format(self.efficiency)   # :214


def high_pt_particles(particle_id, px, py, pt_cut: float = PT_CUT) -> np.ndarray:
    """:44-47: ids of the particles with sqrt(px**2 + py**2) >= pt_cut"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    return np.asarray(particle_id, np.int64)[np.sqrt(px ** 2 + py ** 2) >= pt_cut]


def region_hits(m: HitMapping, truth_hit_id, truth_particle_id, pids, min_volume: int,
                max_volume: int) -> np.ndarray:
    """:50-59: rows of the mapping whose hit the truth file assigns to one of `pids`
    and whose volume lies in [min_volume, max_volume] -> boolean row mask"""
    sel_hits = np.asarray(truth_hit_id, np.int64)[np.isin(np.asarray(truth_particle_id, np.int64), pids)]
    return np.isin(m.hit_id, sel_hits) & (m.volume_id >= min_volume) & (m.volume_id <= max_volume)


def reference_tracks(m: HitMapping, rows: np.ndarray, num_layers: int = NUM_DISTINCT_LAYERS):
    """:63-91 -> (reference particle ids, their hit counts, every region particle's hit
    count as (ids, counts)). `rows` = region_hits mask."""
    pid, vol, lay, mod = m.particle_id[rows], m.volume_id[rows], m.layer_id[rows], m.module_id[rows]
    uniq, inv, nhits = np.unique(pid, return_inverse=True, return_counts=True)
    # distinct (volume, layer) per particle (:67)
    vl = np.unique(np.stack([inv, vol, lay], 1), axis=0)
    n_layers = np.bincount(vl[:, 0], minlength=uniq.size)
    # a (volume, layer, module) occurring twice for a particle (duplicated(keep=False), :79)
    vlm, cnt = np.unique(np.stack([inv, vol, lay, mod], 1), axis=0, return_counts=True)
    dup = np.zeros(uniq.size, bool)
    dup[vlm[cnt > 1, 0]] = True
    good = (n_layers >= num_layers) & ~dup
    return uniq[good], nhits[good], (uniq, nhits)


def node_particles(m: HitMapping, truth_hit_id=None, truth_particle_id=None):
    """construct_graph's hit_dissociation particle lists (helper.py:466-479) as a CSR over
    sorted node ids -> (node ids, ptr, particle ids). A node's hits are its unique hit ids
    in mapping-row order; each hit's particle comes from the truth columns (the mapping's
    own when none are given)."""
    node, hit = m.node_idx, m.hit_id
    # first occurrence of each (node, hit) pair, kept in row order (Series.unique)
    pairs = np.stack([node, hit], 1)
    _, first = np.unique(pairs, axis=0, return_index=True)
    first = np.sort(first)
    node, hit = node[first], hit[first]
    if truth_hit_id is None:
        th, tp = m.hit_id, m.particle_id
    else:
        th, tp = np.asarray(truth_hit_id, np.int64), np.asarray(truth_particle_id, np.int64)
    o = np.argsort(th, kind="stable")
    pos = np.searchsorted(th[o], hit)
    if np.any(pos >= th.size) or np.any(th[o][np.minimum(pos, th.size - 1)] != hit):
        raise ValueError("a mapped hit has no truth row (helper.__get_particle_id .item())")
    part = tp[o][pos]
    order = np.argsort(node, kind="stable")            # group by node, rows in order
    node, part = node[order], part[order]
    ids, starts = np.unique(node, return_index=True)
    ptr = np.append(starts, node.size).astype(np.int64)
    return ids, ptr, part


def candidate_particles(cand_ptr, cand_ids, node_ids, node_ptr, node_part):
    """per candidate, its nodes' particle lists concatenated in node order
    (:125-131) -> (candidate index per entry, particle per entry)"""
    cand_ptr, cand_ids = np.asarray(cand_ptr, np.int64), np.asarray(cand_ids, np.int64)
    k = np.searchsorted(node_ids, cand_ids)
    if np.any(k >= node_ids.size) or np.any(node_ids[np.minimum(k, node_ids.size - 1)] != cand_ids):
        raise ValueError("a candidate node has no hit_dissociation")
    lens = node_ptr[k + 1] - node_ptr[k]
    cand_of_node = np.repeat(np.arange(cand_ptr.size - 1), np.diff(cand_ptr))
    tot = int(lens.sum())
    starts = np.repeat(node_ptr[k], lens)
    offs = np.arange(tot) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(cand_of_node, lens), node_part[starts + offs]


def majority(n_cand: int, cand_of, part):
    """Counter + max(freq, key=freq.get) per candidate (:132-134): the most frequent id,
    ties to the first seen -> (particle id, count, total ids) per candidate"""
    pos = np.arange(part.size)
    key = np.lexsort((pos, part, cand_of))                 # by candidate, particle, position
    c, p = cand_of[key], part[key]
    new = np.ones(c.size, bool)
    new[1:] = (c[1:] != c[:-1]) | (p[1:] != p[:-1])
    grp = np.flatnonzero(new)
    g_cand, g_part, g_first = c[grp], p[grp], pos[key][grp]
    g_cnt = np.diff(np.append(grp, c.size))
    # best per candidate: max count, then smallest first position
    o = np.lexsort((g_first, -g_cnt, g_cand))
    take = np.ones(o.size, bool)
    take[1:] = g_cand[o][1:] != g_cand[o][:-1]
    best = o[take]
    pid = np.zeros(n_cand, np.int64)
    cnt = np.zeros(n_cand, np.int64)
    pid[g_cand[best]], cnt[g_cand[best]] = g_part[best], g_cnt[best]
    total = np.bincount(cand_of, minlength=n_cand)
    return pid, cnt, total


def reconstruction_efficiency(cand_ptr, cand_ids, m: HitMapping, particle_id, px, py, min_volume: int,
                              max_volume: int, truth_hit_id=None, truth_particle_id=None,
                              node_lists: Optional[Sequence[Sequence[int]]] = None) -> Result:
    """The whole script on arrays. Candidates as CSR (cand_ptr, cand_ids) of node ids in
    file order and node order; `node_lists` optionally gives the candidates' particle
    lists directly (their hit_dissociation as stored in the gpickles) instead."""
    th = m.hit_id if truth_hit_id is None else truth_hit_id
    tpid = m.particle_id if truth_particle_id is None else truth_particle_id
    rows = region_hits(m, th, tpid, high_pt_particles(particle_id, px, py), min_volume, max_volume)
    ref_ids, ref_hits, (reg_ids, reg_hits) = reference_tracks(m, rows)
    n_cand = len(cand_ptr) - 1
    if node_lists is None:
        nid, nptr, npart = node_particles(m, truth_hit_id, truth_particle_id)
        cand_of, part = candidate_particles(cand_ptr, cand_ids, nid, nptr, npart)
    else:
        cand_of = np.repeat(np.arange(n_cand), [len(x) for x in node_lists])
        part = np.concatenate([np.asarray(x, np.int64) for x in node_lists]) if n_cand else np.zeros(0, np.int64)
    pid, n_good, total = majority(n_cand, cand_of, part)
    ri = np.searchsorted(ref_ids, pid)
    is_ref = (ri < ref_ids.size) & (ref_ids[np.minimum(ri, max(ref_ids.size - 1, 0))] == pid) if ref_ids.size \
        else np.zeros(n_cand, bool)
    ref_n = np.where(is_ref, ref_hits[np.minimum(ri, max(ref_hits.size - 1, 0))] if ref_hits.size else 0, 1)
    gi = np.searchsorted(reg_ids, pid)
    reg_n = np.where(is_ref, reg_hits[np.minimum(gi, max(reg_ids.size - 1, 0))] if reg_ids.size else 0, 1)
    good_n = n_good * 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        tpur = good_n / total
        ppur = good_n / reg_n
    ok = is_ref & (good_n >= 0.5 * ref_n) & (tpur >= 0.5) & (ppur >= 0.5)
    # each particle once, at its first passing candidate (:166-171)
    idx = np.flatnonzero(ok)
    _, first = np.unique(pid[idx], return_index=True)
    first = np.sort(idx[first])
    matched = np.zeros(n_cand, bool)
    matched[first] = True
    return Result(int(first.size), int(ref_ids.size), tpur[first], ppur[first], pid, n_good, matched)


@dataclasses.dataclass
class TruthTables:
    """gtf_truth's arrays on the host (include/gtf.h), and the number of reference tracks"""
    node_id: np.ndarray      # [T] int64 ascending
    node_ptr: np.ndarray     # [T+1] int32
    node_part: np.ndarray    # [P] int64: node_particles' CSR
    part_id: np.ndarray      # [R] int64 ascending: the region particles
    part_hits: np.ndarray    # [R] int32: hits in the region (= reference hits, see reference_tracks)
    part_ref: np.ndarray     # [R] uint8: 1 = reference track
    n_reference: int


def truth_tables(m: HitMapping, particle_id, px, py, min_volume: int, max_volume: int, truth_hit_id=None,
                 truth_particle_id=None) -> TruthTables:
    """The event's static tables for the device scorer, from region_hits, reference_tracks
    (:41-91) and node_particles (helper.py:466-479) as reconstruction_efficiency uses them."""
    th = m.hit_id if truth_hit_id is None else truth_hit_id
    tpid = m.particle_id if truth_particle_id is None else truth_particle_id
    rows = region_hits(m, th, tpid, high_pt_particles(particle_id, px, py), min_volume, max_volume)
    ref_ids, _, (reg_ids, reg_hits) = reference_tracks(m, rows)
    nid, nptr, npart = node_particles(m, truth_hit_id, truth_particle_id)
    if npart.size > np.iinfo(np.int32).max:
        raise ValueError("more than 2^31 - 1 hit_dissociation entries")
    return TruthTables(nid.astype(np.int64), nptr.astype(np.int32), npart.astype(np.int64), reg_ids.astype(np.int64),
                       reg_hits.astype(np.int32), np.isin(reg_ids, ref_ids).astype(np.uint8), int(ref_ids.size))


class _Mem:
    """the two allocators of the device paths here (DeviceGraph's two, without a graph): "torch"
    (torch tensors, the stream torch is on) or "hip" (gtf.devmem, the default stream)"""

    def __init__(self, device="cuda", mem: str = "torch"):
        from . import _native as nat
        if mem not in ("torch", "hip"):
            raise ValueError("mem must be 'torch' or 'hip'")
        self.nat, self.mem = nat, mem
        if mem == "torch":
            import torch
            self.torch, self.device, self.lib = torch, torch.device(device), nat.lib()
        else:
            self.torch, self.device, self.lib = None, device, nat.lib(lean=True)
            nat.check(self.lib.gtf_device_init(int(str(device).split(":")[1]) if ":" in str(device) else 0))

    def empty(self, n, dtype):
        if self.torch is None:
            from .devmem import HipArray
            return HipArray(n, dtype)
        dt = np.dtype(dtype)
        # (torch has no unsigned 64-bit arithmetic; the bytes are what the library reads)
        name = {"uint64": "int64", "uint32": "int32"}.get(dt.name, dt.name)
        return self.torch.empty(n, dtype=getattr(self.torch, name), device=self.device)

    def from_host(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        if self.torch is None:
            from .devmem import HipArray
            return HipArray.from_numpy(a)
        return self.torch.from_numpy(a).to(self.device)

    def first(self, t, n):
        """the first n elements of a device array, as a view"""
        return t.view(0, n, t.dtype) if self.torch is None else t[:n]

    def host(self, t, n, dtype):
        """the first n elements as a host array of dtype (synchronises)"""
        if n == 0:
            return np.empty(0, dtype)
        a = self.first(t, n).numpy() if self.torch is None else t[:n].cpu().numpy()
        return a.view(dtype)

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)

    @property
    def stream(self):
        if self.torch is None:
            return ctypes.c_void_p(0)
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)


_TABLE_FIELDS = (("node_id", np.int64), ("node_ptr", np.int32), ("node_part", np.int64), ("part_id", np.int64),
                 ("part_hits", np.int32), ("part_ref", np.uint8))


class DeviceTruth:
    """truth_tables_dev's result: the six arrays of TruthTables on the device, trimmed views of the
    buffers gtf_truth_build filled, the number of reference tracks and the GtfTruth struct that
    gtf_score_candidates takes. host() downloads them as a TruthTables."""

    def __init__(self, mem: _Mem, arrays, truth, counts):
        self._m, self.truth, self.device, self.mem = mem, truth, mem.device, mem.mem
        self.n_nodes, self.n_entries = int(counts.n_nodes), int(counts.n_entries)
        self.n_particles, self.n_reference = int(counts.n_particles), int(counts.n_reference)
        sizes = (self.n_nodes, self.n_nodes + 1, self.n_entries, self.n_particles, self.n_particles, self.n_particles)
        self._buffers = arrays      # (the views point into them)
        for (name, _), a, n in zip(_TABLE_FIELDS, arrays, sizes):
            setattr(self, name, mem.first(a, n))

    def host(self) -> "TruthTables":
        """the tables as metrics.truth_tables returns them (synchronises)"""
        return TruthTables(*(self._m.host(getattr(self, name), getattr(self, name).numel(), dt)
                             for name, dt in _TABLE_FIELDS), self.n_reference)


def truth_tables_dev(m: HitMapping, particle_id, px, py, min_volume: int, max_volume: int, truth_hit_id=None,
                     truth_particle_id=None, device="cuda", mem: str = "torch") -> DeviceTruth:
    """truth_tables on the device (gtf_truth_build, csrc/gtf_truth.hip): the columns go up once
    and the six arrays stay there, array_equal to the host function's. Any column may be a device
    array of this allocator already (int64 ids, float64 px / py: gtf.csvdev.parse_dev, truth_files_dev);
    it is used where it is. The mapping's volume_id,
    layer_id and module_id must lie in [0, 2^21) (ValueError); a mapped hit without a truth row
    is the host's ValueError."""
    from . import _native as nat
    mm = _Mem(device, mem)

    def col(a, dt):   # a host column (uploaded below) or a device array as it is
        return a if hasattr(a, "data_ptr") else np.ascontiguousarray(a, dt).reshape(-1)

    def size(a):
        return int(a.numel()) if hasattr(a, "data_ptr") else int(a.size)

    cols = [col(getattr(m, c), np.int64) for c in ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")]
    n = size(cols[0])
    if any(size(c) != n for c in cols):
        raise ValueError("mapping columns of different lengths")
    truth = []
    if truth_hit_id is not None:
        truth = [col(a, np.int64) for a in (truth_hit_id, truth_particle_id)]
        if size(truth[0]) != size(truth[1]):
            raise ValueError("truth columns of different lengths")
        if size(truth[0]) == 0:      # (for the library n_truth == 0 means "the mapping's own columns")
            if n:
                raise ValueError("a mapped hit has no truth row (helper.__get_particle_id .item())")
            truth = []
    part = [col(particle_id, np.int64), col(px, np.float64), col(py, np.float64)]
    if not size(part[0]) == size(part[1]) == size(part[2]):
        raise ValueError("particle columns of different lengths")
    n_truth, n_part = size(truth[0]) if truth else 0, size(part[0])
    if min_volume > max_volume:
        raise ValueError("min_volume > max_volume")
    if max(n, n_truth, n_part) > 1 << 30:
        raise ValueError("more than 2^30 rows")
    dev = [(a if hasattr(a, "data_ptr") else mm.from_host(a)) if size(a) else None for a in cols + truth + part]
    d_truth = dev[6:8] if truth else [None, None]
    names = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id", "truth_hit", "truth_part",
             "part_id", "px", "py")
    tin = nat.GtfTruthIn(n_rows=n, n_truth=n_truth, n_particles=n_part, num_layers=NUM_DISTINCT_LAYERS,
                         min_volume=int(min_volume), max_volume=int(max_volume), pt_cut=PT_CUT,
                         **{k: mm.p(a) for k, a in zip(names, dev[:6] + d_truth + dev[-3:])})
    out = [mm.empty(max(n, 1) + (name == "node_ptr"), dt) for name, dt in _TABLE_FIELDS]
    buf = nat.GtfTruthBuf(*(mm.p(a) for a in out))
    nb = int(mm.lib.gtf_truth_build_workspace_bytes(n, n_truth, n_part))
    ws = mm.empty(nb, np.uint8)
    t, cnt = nat.GtfTruth(), nat.GtfTruthCounts()
    rc = mm.lib.gtf_truth_build(ctypes.byref(tin), ctypes.byref(buf), ctypes.byref(t), ctypes.byref(cnt), mm.p(ws),
                                ctypes.c_size_t(nb), mm.stream)
    if rc == -2 and cnt.error & nat.TRUTH_ERR_RANGE:
        raise ValueError("a volume_id, layer_id or module_id outside [0, %d): the device builder packs them "
                         "into one key (use metrics.truth_tables)" % nat.TRUTH_ID_LIMIT)
    if rc == -2 and cnt.error & nat.TRUTH_ERR_MISSING:
        raise ValueError("a mapped hit has no truth row (helper.__get_particle_id .item())")
    nat.check(rc)
    return DeviceTruth(mm, out, t, cnt)


MAPPING_COLUMNS = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")


def _read_truth_files(mm: _Mem, prefix: str, mapping: str):
    """the columns of one event's truth files, as truth_files_dev documents them -> (HitMapping,
    particle_id, px, py, truth hit_id or None, truth particle_id or None, info)"""
    import os
    from .csvdev import OutOfDomain, parse_dev
    info = {}

    def read(key, path, columns):
        try:
            c = parse_dev(path, columns, 1, mm=mm)
            info[key] = "device"
            return [c[name] for name, _ in columns]
        except OutOfDomain as e:
            import pandas as pd
            info[key], info[key + "_reason"] = "host", str(e)
            f = pd.read_csv(path, usecols=[name for name, _ in columns])
            return [f[name].to_numpy(np.dtype(t)) for name, t in columns]

    pid, px, py = read("particles", prefix + "particles.csv", (("particle_id", "int64"), ("px", "float64"), ("py", "float64")))
    m = HitMapping(*read("mapping", prefix + mapping, tuple((c, "int64") for c in MAPPING_COLUMNS)))
    th = tp = None
    if os.path.isfile(prefix + "truth.csv"):
        th, tp = read("truth", prefix + "truth.csv", (("hit_id", "int64"), ("particle_id", "int64")))
    return m, pid, px, py, th, tp, info


def truth_files_dev(prefix: str, mapping: str, min_volume: int, max_volume: int, device="cuda", mem: str = "torch"):
    """truth_tables_dev from the files reconstruction_efficiency.score reads (``prefix`` +
    "particles.csv", + ``mapping``, and + "truth.csv" where it exists), each parsed on the device
    (gtf.csvdev.parse_dev) with its columns chosen by header name, whatever else the file holds. A
    file with a field outside the parser's exact domain is read with pd.read_csv instead. Returns
    (DeviceTruth, {"particles" | "mapping" | "truth": "device" | "host"})."""
    m, pid, px, py, th, tp, info = _read_truth_files(_Mem(device, mem), prefix, mapping)
    return truth_tables_dev(m, pid, px, py, min_volume, max_volume, th, tp, device, mem), info


class DeviceScorer:
    """reconstruction_efficiency on the device (gtf_score_*, include/gtf.h): the tables go up
    once; add() scores one iteration's candidates from the device arrays gtf_extract_outputs
    wrote (extract.outputs_dev(lists=False): "cand_ptr", "cand_ids") and result() returns the
    Result the host function returns for the same candidates concatenated by ascending group.
    The reference reads iterations last, ..., 1 (score(cumulative=True)) while the loop
    produces 1, ..., last: pass group = last - iteration; the calls may come in any order and
    need distinct groups. mem "torch" (torch tensors, the stream torch is on) or "hip"
    (gtf.devmem, the default stream), as DeviceGraph. `tables` may be a DeviceTruth
    (truth_tables_dev): its arrays are used where they are, with its device and allocator."""

    def __init__(self, tables, device="cuda", mem: str = "torch"):
        on_dev = isinstance(tables, DeviceTruth)
        m = tables._m if on_dev else _Mem(device, mem)
        self._m, self.nat, self.tables, self.mem = m, m.nat, tables, m.mem
        self.torch, self.device, self.lib = m.torch, m.device, m.lib
        t = tables
        if on_dev:
            self.R, self.truth = t.n_particles, t.truth
        else:
            self.R = int(t.part_id.size)
            self._dev = [self._from(a) for a in (t.node_id, t.node_ptr, t.node_part, t.part_id, t.part_hits, t.part_ref)]
            self.truth = self.nat.GtfTruth(n_nodes=int(t.node_id.size), n_entries=int(t.node_part.size),
                                           n_particles=self.R,
                                           **{k: self._p(a) for k, a in zip(("node_id", "node_ptr", "node_part", "part_id",
                                                                             "part_hits", "part_ref"), self._dev)})
        nat = self.nat
        r1 = max(self.R, 1)
        self._state = [self._empty(r1, np.uint64), self._empty(r1, np.int32), self._empty(r1, np.int32),
                       self._empty(1, np.uint32)]
        self.state = nat.GtfScoreState(self.R, 0, *(self._p(a) for a in self._state))
        self.reset()

    # -- this scorer's allocator
    def _empty(self, n, dtype):
        return self._m.empty(n, dtype)

    def _from(self, a):
        return self._m.from_host(a)

    def _host(self, t, n, dtype):
        """the first n elements as a host array of dtype (synchronises)"""
        return self._m.host(t, n, dtype)

    _p = staticmethod(_Mem.p)

    @property
    def stream(self):
        return self._m.stream

    def reset(self):
        """forget every candidate scored so far (does not synchronise)"""
        self.nat.check(self.lib.gtf_score_reset(ctypes.byref(self.state), self.stream))
        self._per = []        # (group, n_cand, pid, n_good) device arrays of the per_candidate adds
        self._all_per = True
        self._keep = []       # mem "hip": the adds' workspaces, which a plain allocation would free at once

    def add(self, cand_ptr_dev, cand_ids_dev, n_cand: int, group: int, per_candidate: bool = False,
            n_members: Optional[int] = None):
        """Score n_cand candidates: cand_ptr_dev [n_cand + 1] int32 and cand_ids_dev int64 device
        arrays (gtf_extract_out's form). n_members: the host count of members when the caller has
        it (gtf_extract_out_counts.n_extracted_nodes), else the length of cand_ids_dev sizes the
        workspace. Nothing synchronises."""
        nat = self.nat
        n_cand, group = int(n_cand), int(group)
        if n_cand == 0:
            if per_candidate:
                self._per.append((group, 0, None, None))
            else:
                self._all_per = False
            return
        if not cand_ids_dev.numel():      # (candidates without a member: the library still wants an array)
            cand_ids_dev = self._empty(1, np.int64)
        cap = int(cand_ids_dev.numel()) if n_members is None else int(n_members)
        nb = int(self.lib.gtf_score_workspace_bytes(n_cand, cap))
        ws = self._empty(nb, np.uint8)
        out = nat.GtfScoreOut()
        if per_candidate:
            pid, good = self._empty(n_cand, np.int64), self._empty(n_cand, np.int32)
            out = nat.GtfScoreOut(self._p(pid), self._p(good), None, None)
            self._per.append((group, n_cand, pid, good))
        else:
            self._all_per = False
        nat.check(self.lib.gtf_score_candidates(ctypes.byref(self.truth), self._p(cand_ptr_dev), self._p(cand_ids_dev),
                                                n_cand, group, ctypes.byref(out), ctypes.byref(self.state),
                                                self._p(ws), ctypes.c_size_t(nb), self.stream))
        if self.torch is None:
            self._keep.append(ws)      # (until result() has synchronised)

    def result(self) -> Result:
        """The Result of everything added since the last reset (synchronises once). The purities
        are formed here, in fp64, from the integer records. reconstructed_pid / n_good / matched
        are filled when every add asked for per_candidate, concatenated by ascending group;
        else they are empty."""
        nat = self.nat
        r1 = max(self.R, 1)
        key, pid = self._empty(r1, np.uint64), self._empty(r1, np.int64)
        good, total, hits = (self._empty(r1, np.int32) for _ in range(3))
        nb = int(self.lib.gtf_score_finish_workspace_bytes(self.R))
        ws = self._empty(nb, np.uint8)
        cnt = nat.GtfScoreCounts()
        rc = self.lib.gtf_score_finish(ctypes.byref(self.truth), ctypes.byref(self.state), self._p(key), self._p(pid),
                                       self._p(good), self._p(total), self._p(hits), ctypes.byref(cnt), self._p(ws),
                                       ctypes.c_size_t(nb), self.stream)
        self._keep = []
        if rc == -2 and cnt.error & nat.SCORE_ERR_MISSING:
            raise ValueError("a candidate node has no hit_dissociation")
        nat.check(rc)
        n = int(cnt.n_reconstructed)
        g = self._host(good, n, np.int32) * 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            tpur = g / self._host(total, n, np.int32)
            ppur = g / self._host(hits, n, np.int32)
        if self._all_per and self._per:
            per = sorted(self._per, key=lambda x: x[0])
            start, at = {}, 0
            for grp, nc, _, _ in per:
                start[grp] = at
                at += nc
            rp = np.concatenate([self._host(p, nc, np.int64) for _, nc, p, _ in per])
            ng = np.concatenate([self._host(q, nc, np.int32) for _, nc, _, q in per]).astype(np.int64)
            matched = np.zeros(at, bool)
            k = self._host(key, n, np.uint64)
            matched[[start[int(x >> np.uint64(32))] + int(x & np.uint64(0xffffffff)) for x in k]] = True
        else:
            rp, ng, matched = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
        return Result(n, self.tables.n_reference, tpur, ppur, rp, ng, matched)


_OFFSET_FIELDS = ("node_off", "entry_off", "part_off")


@dataclasses.dataclass
class BatchTables:
    """gtf_truth_batch's arrays on the host (include/gtf.h): K events' TruthTables end to end. Ids of
    different events collide, so node_id and part_id ascend inside an event's segment only; node_ptr
    holds every event's pointers shifted by its entry_off, and one closing entry."""
    node_id: np.ndarray      # [sum T] int64
    node_ptr: np.ndarray     # [sum T + 1] int32
    node_part: np.ndarray    # [sum P] int64
    part_id: np.ndarray      # [sum R] int64
    part_hits: np.ndarray    # [sum R] int32
    part_ref: np.ndarray     # [sum R] uint8
    node_off: np.ndarray     # [K + 1] int32
    entry_off: np.ndarray    # [K + 1] int32
    part_off: np.ndarray     # [K + 1] int32
    scored: np.ndarray       # [K] uint8: 0 = an event without truth
    n_reference: list        # per event; None where it is not scored

    def event(self, e: int) -> Optional[TruthTables]:
        """event e's own tables again (None for an unscored event)"""
        if not self.scored[e]:
            return None
        n0, n1, e0 = int(self.node_off[e]), int(self.node_off[e + 1]), int(self.entry_off[e])
        p0, p1 = int(self.part_off[e]), int(self.part_off[e + 1])
        return TruthTables(self.node_id[n0:n1], (self.node_ptr[n0:n1 + 1] - e0).astype(np.int32),
                           self.node_part[e0:int(self.entry_off[e + 1])], self.part_id[p0:p1], self.part_hits[p0:p1],
                           self.part_ref[p0:p1], self.n_reference[e])


def _offsets(sizes) -> np.ndarray:
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    if off[-1] >= 1 << 31:
        raise ValueError("the tables sum to 2^31 or more nodes, entries or particles")
    return off.astype(np.int32)


def concat_tables(tables) -> BatchTables:
    """The host definition of gtf_truth_concat: the TruthTables of K events (None = an event without
    truth: empty tables, scored 0) laid end to end."""
    tables = list(tables)
    live = [t for t in tables if t is not None]

    def cat(name, dt):
        return np.concatenate([np.asarray(getattr(t, name), dt) for t in live]) if live else np.zeros(0, dt)

    size = lambda t, name: 0 if t is None else int(getattr(t, name).size)   # noqa: E731
    node_off, entry_off, part_off = (_offsets([size(t, name) for t in tables]) for name in ("node_id", "node_part", "part_id"))
    shift = [e for t, e in zip(tables, entry_off[:-1]) if t is not None]
    ptr = [np.asarray(t.node_ptr, np.int64)[:-1] + int(e) for t, e in zip(live, shift)] + [np.array([entry_off[-1]], np.int64)]
    return BatchTables(cat("node_id", np.int64), np.concatenate(ptr).astype(np.int32), cat("node_part", np.int64),
                       cat("part_id", np.int64), cat("part_hits", np.int32), cat("part_ref", np.uint8), node_off,
                       entry_off, part_off, np.array([t is not None for t in tables], np.uint8),
                       [None if t is None else int(t.n_reference) for t in tables])


class DeviceTruthBatch:
    """truth_concat_dev's result: the arrays of BatchTables on the device and the GtfTruthBatch struct
    gtf_score_candidates_ev takes. host() downloads them as a BatchTables."""

    def __init__(self, mem: _Mem, arrays, batch, scored, n_reference, keep):
        self._m, self.batch, self.device, self.mem = mem, batch, mem.device, mem.mem
        self.n_events, self.n_nodes = int(batch.n_events), int(batch.n_nodes)
        self.n_entries, self.n_particles = int(batch.n_entries), int(batch.n_particles)
        self.scored, self.n_reference = scored, n_reference
        self._buffers, self._keep = arrays, keep      # (the views point into them; the parts until the copy has run)
        K = self.n_events
        sizes = (self.n_nodes, self.n_nodes + 1, self.n_entries, self.n_particles, self.n_particles, self.n_particles,
                 K + 1, K + 1, K + 1)
        for name, a, n in zip([f for f, _ in _TABLE_FIELDS] + list(_OFFSET_FIELDS), arrays, sizes):
            setattr(self, name, mem.first(a, n))

    def host(self) -> BatchTables:
        """the tables as concat_tables returns them (synchronises)"""
        fields = list(_TABLE_FIELDS) + [(f, np.int32) for f in _OFFSET_FIELDS]
        return BatchTables(*(self._m.host(getattr(self, name), getattr(self, name).numel(), dt) for name, dt in fields),
                           self.scored.copy(), list(self.n_reference))


def truth_concat_dev(tables, device="cuda", mem: str = "torch") -> DeviceTruthBatch:
    """concat_tables on the device (gtf_truth_concat, csrc/gtf_score.hip): two launches whatever the
    number of events, nothing synchronises. Entries may be TruthTables (uploaded), DeviceTruth
    (truth_tables_dev: used where it is) or None (an event without truth). One allocator and one device:
    that of the DeviceTruth entries, which must agree, else ``device`` / ``mem``."""
    from . import _native as nat
    tables = list(tables)
    on_dev = [t for t in tables if isinstance(t, DeviceTruth)]
    mm = on_dev[0]._m if on_dev else _Mem(device, mem)
    if any((t.mem, str(t.device)) != (mm.mem, str(mm.device)) for t in on_dev):
        raise ValueError("truth_concat_dev: the DeviceTruth entries must share one allocator and one device")
    K = len(tables)
    sizes, parts, keep = (nat.GtfTruthSizes * max(K, 1))(), (nat.GtfTruthPart * max(K, 1))(), []
    names = [f for f, _ in _TABLE_FIELDS]
    for i, t in enumerate(tables):
        if t is None:
            continue
        if isinstance(t, DeviceTruth):
            arrays = [getattr(t, name) for name in names]
            n = (t.n_nodes, t.n_entries, t.n_particles)
        else:
            arrays = [mm.from_host(np.ascontiguousarray(getattr(t, name), dt)) if np.size(getattr(t, name)) else None
                      for name, dt in _TABLE_FIELDS]
            n = (int(t.node_id.size), int(t.node_part.size), int(t.part_id.size))
        keep.append(arrays)
        sizes[i].n_nodes, sizes[i].n_entries, sizes[i].n_particles = n
        parts[i].n_nodes, parts[i].n_entries, parts[i].n_particles = n
        for name, a in zip(names, arrays):
            setattr(parts[i], name, mm.p(a).value)
    T, P, R = (sum(getattr(sizes[i], f) for i in range(K)) for f in ("n_nodes", "n_entries", "n_particles"))
    if max(T, P, R) >= 1 << 31:
        raise ValueError("the tables sum to 2^31 or more nodes, entries or particles")
    out = [mm.empty(max(n, 1), dt) for (_, dt), n in zip(_TABLE_FIELDS, (T, T + 1, P, R, R, R))]
    out += [mm.empty(K + 1, np.int32) for _ in _OFFSET_FIELDS]
    scored = np.array([t is not None for t in tables], np.uint8)
    d_scored = mm.from_host(scored) if K and not scored.all() else None
    d_parts = mm.from_host(np.frombuffer(bytearray(parts), np.uint8)) if K else None
    buf = nat.GtfTruthBatchBuf(*(mm.p(a) for a in out[6:] + out[:6]))
    batch = nat.GtfTruthBatch(scored=mm.p(d_scored))
    nb = int(mm.lib.gtf_truth_concat_workspace_bytes(K))
    ws = mm.empty(nb, np.uint8)
    nat.check(mm.lib.gtf_truth_concat(sizes, mm.p(d_parts), K, ctypes.byref(buf), ctypes.byref(batch), mm.p(ws),
                                      ctypes.c_size_t(nb), mm.stream))
    keep += [d_parts, d_scored, ws]
    return DeviceTruthBatch(mm, out, batch, scored, [None if t is None else int(t.n_reference) for t in tables], keep)


def truth_tables_batch(parts, min_volume: int, max_volume: int) -> BatchTables:
    """The host definition of gtf_truth_build_ev: concat_tables of every event's truth_tables, one window
    for the batch. A part is (HitMapping, particle_id, px, py, truth_hit_id=None, truth_particle_id=None),
    or None for an event without truth (zero rows, scored 0)."""
    return concat_tables([None if p is None else truth_tables(p[0], p[1], p[2], p[3], min_volume, max_volume,
                                                              *tuple(p)[4:6]) for p in parts])


_BATCH_DTYPES = (np.int64,) * 9 + (np.float64,) * 2   # six mapping columns, truth_hit / truth_part, part_id; px, py


def _gather_dev(mm: _Mem, cols, dtypes, axes, n0, n1):
    """device columns of K events end to end, as DeviceGraph._gather_columns gathers an event's: the offsets
    of gtf_graph_concat with no structure output (two axes: sizes n0 and n1 per event) and
    gtf_concat_columns. cols[i][e]: column i of event e (None where it has no rows), 8 bytes a row, on
    axis axes[i]. No launch per event. -> one array per column (None for an empty axis)"""
    nat, L, K, C = mm.nat, mm.lib, len(n0), len(cols)
    total = (int(sum(n0)), int(sum(n1)))
    adr = lambda t: t.data_ptr() if t is not None and t.numel() else 0  # noqa: E731
    if any(adr(a) % 8 for c in cols for a in c):
        raise ValueError("truth_tables_batch_dev: a device column is not aligned to 8 bytes")
    dst = [mm.empty(total[ax], dt) if total[ax] else None for ax, dt in zip(axes, dtypes)]
    ptab = (nat.GtfConcatPart * K)(*[nat.GtfConcatPart(n0[e], n1[e], 0, 0, 0, 0, 0, 0, 0) for e in range(K)])
    pwords = ctypes.sizeof(nat.GtfConcatPart) // 8
    host = np.zeros(K * (pwords + C), np.int64)
    host[:K * pwords] = np.frombuffer(ptab, np.int64)
    for i in range(C):
        host[K * (pwords + i):K * (pwords + i + 1)] = [adr(cols[i][e]) if (n1 if axes[i] else n0)[e] else 0
                                                       for e in range(K)]
    tab = mm.from_host(host)
    nb = int(L.gtf_graph_concat_workspace_bytes(K))
    ws = mm.empty(nb, np.uint8)
    hs = (nat.GtfConcatSizes * K)(*[nat.GtfConcatSizes(n0[e], n1[e], 0, 0) for e in range(K)])
    nat.check(L.gtf_graph_concat(hs, ctypes.c_void_p(tab.data_ptr()), K, ctypes.byref(nat.GtfConcatOut()), mm.p(ws),
                                 ctypes.c_size_t(nb), mm.stream))
    cc = (nat.GtfConcatColumn * C)(*[nat.GtfConcatColumn(tab.data_ptr() + 8 * K * (pwords + i), mm.p(dst[i]), 8, axes[i])
                                     for i in range(C)])
    nat.check(L.gtf_concat_columns(mm.p(ws), K, total[0], total[1], cc, C, mm.stream))
    # the table and the workspace go out of scope with kernels in flight: a torch allocation is reused in
    # stream order, a plain one is freed at once
    if mm.torch is None:
        nat.check(L.gtf_stream_synchronize(None))
    return dst


def truth_tables_batch_dev(parts, min_volume: int, max_volume: int, device="cuda", mem: str = "torch") -> DeviceTruthBatch:
    """truth_tables_batch on the device in ONE build (gtf_truth_build_ev, csrc/gtf_truth.hip): what
    truth_concat_dev([truth_tables_dev(...) for each part]) leaves, word for word, with one synchronisation
    and a number of launches that does not depend on len(parts). The columns are all host arrays
    (concatenated, and uploaded once per column: eleven uploads whatever K) or all device arrays of this
    allocator (gathered by gtf_graph_concat's offsets and gtf_concat_columns, no launch per part); a mix
    is a ValueError. The ValueErrors of truth_tables_dev carry over with the event in the text."""
    return _truth_tables_batch_dev(parts, min_volume, max_volume, device, mem, lambda what: None)


def _truth_tables_batch_dev(parts, min_volume, max_volume, device, mem, mark, fused=None):
    """truth_tables_batch_dev; mark("build") / mark("built") are called around the library call
    (tools/batch_truth.py records device events there). fused: (the eleven device columns of the batch
    end to end -- the six mapping columns, truth hit and particle, particle id, px, py; None for one
    without rows --, row_off, truth_off, particle_off: host, [K + 1]) as csvdev.parse_batch_dev left
    them; ``parts`` then only says which events are scored (None: not) and nothing is gathered."""
    from . import _native as nat
    parts = list(parts)
    K = len(parts)
    if fused is not None:
        if min_volume > max_volume:
            raise ValueError("min_volume > max_volume")
        dev, offs = list(fused[0]), [np.ascontiguousarray(o, np.int64).reshape(-1) for o in fused[1:]]
        if len(dev) != 11 or len(offs) != 3 or any(o.size != K + 1 or o[0] != 0 or (np.diff(o) < 0).any() for o in offs):
            raise ValueError("fused: eleven columns and three offset arrays of K + 1 entries from 0, not decreasing")
        if max(int(o[-1]) for o in offs) > 1 << 30:
            raise ValueError("more than 2^30 rows")
        row_off, truth_off, particle_off = (np.ascontiguousarray(o, np.int32) for o in offs)
        N, NT, NP = int(row_off[-1]), int(truth_off[-1]), int(particle_off[-1])
        mm = _Mem(device, mem)
        dev = [a if total else None for a, total in zip(dev, [N] * 6 + [NT] * 2 + [NP] * 3)] if N else [None] * 11
        return _truth_build_ev(mm, parts, dev, row_off, truth_off, particle_off, min_volume, max_volume, mark)
    is_dev = lambda a: hasattr(a, "data_ptr")  # noqa: E731
    size = lambda a: 0 if a is None else int(a.numel()) if is_dev(a) else int(a.size)  # noqa: E731
    events = []      # per event its eleven columns (truth_hit / truth_part None: the mapping's own), or None
    for e, p in enumerate(parts):
        if p is None:
            events.append(None)
            continue
        p = tuple(p)
        if len(p) not in (4, 6):
            raise ValueError("event %d: a part is (HitMapping, particle_id, px, py[, truth_hit_id, truth_particle_id]) "
                             "or None" % e)
        th, tp = p[4:6] if len(p) == 6 else (None, None)
        if (th is None) != (tp is None):
            raise ValueError("event %d: truth_hit_id and truth_particle_id come together" % e)
        raw = [getattr(p[0], c) for c in MAPPING_COLUMNS] + [th, tp] + list(p[1:4])
        cols = [a if a is None or is_dev(a) else np.ascontiguousarray(a, dt).reshape(-1) for a, dt in zip(raw, _BATCH_DTYPES)]
        n = size(cols[0])
        if any(size(c) != n for c in cols[:6]):
            raise ValueError("event %d: mapping columns of different lengths" % e)
        if th is not None:
            if size(cols[6]) != size(cols[7]):
                raise ValueError("event %d: truth columns of different lengths" % e)
            if size(cols[6]) == 0:      # (for the library no truth rows means "the mapping's own columns")
                if n:
                    raise ValueError("event %d: a mapped hit has no truth row (helper.__get_particle_id .item())" % e)
                cols[6] = cols[7] = None
        if not size(cols[8]) == size(cols[9]) == size(cols[10]):
            raise ValueError("event %d: particle columns of different lengths" % e)
        events.append(cols)
    on_dev = [is_dev(a) for cols in events if cols is not None for a in cols if a is not None]
    if any(on_dev) and not all(on_dev):
        raise ValueError("truth_tables_batch_dev: the columns are all host arrays or all device arrays")
    if min_volume > max_volume:
        raise ValueError("min_volume > max_volume")
    sizes = [[0 if cols is None else size(cols[i]) for cols in events] for i in (0, 6, 8)]   # rows, truth rows, particles
    offs = [np.concatenate([[0], np.cumsum(s, dtype=np.int64)]) for s in sizes]
    if max(int(o[-1]) for o in offs) > 1 << 30:
        raise ValueError("more than 2^30 rows")
    row_off, truth_off, particle_off = (np.ascontiguousarray(o, np.int32) for o in offs)
    N, NT, NP = int(row_off[-1]), int(truth_off[-1]), int(particle_off[-1])
    mm = _Mem(device, mem)
    per_column = [[None if cols is None else cols[i] for cols in events] for i in range(11)]
    if not N:
        dev = [None] * 11          # (nothing is read)
    elif on_dev and on_dev[0] and K == 1:
        dev = [a if size(a) else None for a in events[0]]      # (one event: its columns are the batch's)
    elif on_dev and on_dev[0]:
        dev = _gather_dev(mm, per_column[:8], _BATCH_DTYPES[:8], [0] * 6 + [1] * 2, sizes[0], sizes[1])
        dev += _gather_dev(mm, per_column[8:], _BATCH_DTYPES[8:], [0] * 3, sizes[2], [0] * K) if NP else [None] * 3
    else:
        dev = [mm.from_host(np.concatenate([a for a in c if a is not None])) if total else None
               for c, total in zip(per_column, [N] * 6 + [NT] * 2 + [NP] * 3)]
    return _truth_build_ev(mm, parts, dev, row_off, truth_off, particle_off, min_volume, max_volume, mark)


def _truth_build_ev(mm, parts, dev, row_off, truth_off, particle_off, min_volume, max_volume, mark):
    """the one gtf_truth_build_ev of _truth_tables_batch_dev, on the batch's eleven device columns"""
    nat = mm.nat
    K = len(parts)
    N, NT, NP = int(row_off[-1]), int(truth_off[-1]), int(particle_off[-1])
    names = MAPPING_COLUMNS + ("truth_hit", "truth_part", "part_id", "px", "py")
    tin = nat.GtfTruthInEv(n_events=K, num_layers=NUM_DISTINCT_LAYERS, min_volume=int(min_volume),
                           max_volume=int(max_volume), pt_cut=PT_CUT, row_off=row_off.ctypes.data,
                           truth_off=truth_off.ctypes.data, particle_off=particle_off.ctypes.data,
                           **{k: mm.p(a) for k, a in zip(names, dev)})
    out = [mm.empty(max(N, 1) + (name == "node_ptr"), dt) for name, dt in _TABLE_FIELDS]
    out += [mm.empty(K + 1, np.int32) for _ in _OFFSET_FIELDS]
    scored = np.array([p is not None for p in parts], np.uint8)
    d_scored = mm.from_host(scored) if K and not scored.all() else None
    buf = nat.GtfTruthBatchBuf(*(mm.p(a) for a in out[6:] + out[:6]))
    batch = nat.GtfTruthBatch(scored=mm.p(d_scored))
    nb = int(mm.lib.gtf_truth_build_ev_workspace_bytes(N, NT, NP, K))
    ws = mm.empty(nb, np.uint8)
    cnt = (nat.GtfTruthCounts * max(K, 1))()
    mark("build")
    rc = mm.lib.gtf_truth_build_ev(ctypes.byref(tin), ctypes.byref(buf), ctypes.byref(batch), cnt, mm.p(ws),
                                   ctypes.c_size_t(nb), mm.stream)
    mark("built")
    if rc == -2:
        for e in range(K):
            if cnt[e].error & nat.TRUTH_ERR_RANGE:
                raise ValueError("event %d: a volume_id, layer_id or module_id outside [0, %d): the device builder "
                                 "packs them into one key (use metrics.truth_tables_batch)" % (e, nat.TRUTH_ID_LIMIT))
            if cnt[e].error & nat.TRUTH_ERR_MISSING:
                raise ValueError("event %d: a mapped hit has no truth row (helper.__get_particle_id .item())" % e)
    nat.check(rc)
    n_reference = [int(cnt[e].n_reference) if scored[e] else None for e in range(K)]
    return DeviceTruthBatch(mm, out, batch, scored, n_reference, [d_scored, ws, dev])


def truth_files_batch_dev(prefixes, mapping: str, min_volume: int, max_volume: int, device="cuda", mem: str = "torch",
                          batch_parse: bool = False):
    """truth_tables_batch_dev from the files of K events: each event's files are parsed as truth_files_dev
    parses them (per file, on the device; a file outside the parser's exact domain is read with
    pd.read_csv and uploaded), then ONE build makes the tables. ``prefixes``: one per event, or None for an
    event without truth. Returns (DeviceTruthBatch, [truth_files_dev's info per event, None without truth]).
    batch_parse: the files of one kind -- the particles, the mappings, and the truth.csv of the events that
    have one -- are each parsed in ONE call (csvdev.parse_batch_dev) and their fused columns go to the
    build as they are, without a gather. The same tables, word for word, and the same infos; the
    DeviceTruthBatch's ``parse_info`` holds the three ParsedBatch infos."""
    if batch_parse:
        return _truth_files_batch_parse(list(prefixes), mapping, min_volume, max_volume, device, mem,
                                        lambda what: None)
    mm = _Mem(device, mem)
    parts, infos = [], []
    for prefix in prefixes:
        if prefix is None:
            parts.append(None)
            infos.append(None)
            continue
        m, pid, px, py, th, tp, info = _read_truth_files(mm, prefix, mapping)
        cols = [a if a is None or hasattr(a, "data_ptr") else mm.from_host(a)
                for a in [getattr(m, c) for c in MAPPING_COLUMNS] + [pid, px, py, th, tp]]
        parts.append((HitMapping(*cols[:6]),) + tuple(cols[6:9]) + (() if th is None else tuple(cols[9:])))
        infos.append(info)
    return truth_tables_batch_dev(parts, min_volume, max_volume, device, mem), infos


class BatchScorer:
    """DeviceScorer for the K events of a fused graph at once (gtf_score_*_ev, csrc/gtf_score.hip): one
    add() per iteration takes the fused graph's candidates as gtf_extract_outputs and gtf_event_split
    left them -- the global cand_ptr / cand_ids and cand_first (extract.split_dev: "cand_first_dev") --
    and results() returns one Result per event, equal to what DeviceScorer.result() gives for that event
    alone (None for an event without truth). The number of launches does not depend on K; add() never
    synchronises, results() synchronises once for the batch. ``tables``: a DeviceTruthBatch, or a sequence
    of TruthTables / DeviceTruth / None that truth_concat_dev concatenates."""

    def __init__(self, tables, device="cuda", mem: str = "torch"):
        if not isinstance(tables, DeviceTruthBatch):
            tables = truth_concat_dev(tables, device, mem)
        m = tables._m
        self._m, self.nat, self.tables, self.mem = m, m.nat, tables, m.mem
        self.torch, self.device, self.lib = m.torch, m.device, m.lib
        self.K, self.R, self.batch = tables.n_events, tables.n_particles, tables.batch
        r1 = max(self.R, 1)
        self._state = [m.empty(r1, np.uint64), m.empty(r1, np.int32), m.empty(r1, np.int32), m.empty(2, np.uint32)]
        self.state = self.nat.GtfScoreStateEv(n_particles=self.R, **{k: m.p(a) for k, a in zip(
            ("best_key", "best_good", "best_total", "error"), self._state)})
        self.reset()

    _p = staticmethod(_Mem.p)

    @property
    def stream(self):
        return self._m.stream

    def reset(self, events=None):
        """forget every candidate scored so far; or, with ``events`` (K booleans), those of the marked
        events alone -- the others keep their claims, and the error words stay (does not synchronise)"""
        mask = None
        if events is None:
            self._per, self._all_per, self._keep = [], True, []
        else:
            ev = np.ascontiguousarray(np.asarray(events, bool).reshape(-1), np.uint8)
            if ev.size != self.K:
                raise ValueError("reset(events=...) takes one entry per event")
            if not self.K:
                return
            mask = self._m.from_host(ev)
            for rec in self._per:       # (the per-candidate lists of the marked events go with their claims)
                rec["dead"] = rec["dead"] | ev.astype(bool)
            self._keep.append(mask)
        self.nat.check(self.lib.gtf_score_reset_ev(ctypes.byref(self.state), ctypes.byref(self.batch), self._p(mask),
                                                   self.stream))

    def add(self, cand_ptr_dev, cand_ids_dev, cand_first_dev, n_cand: int, group: int, per_candidate: bool = False,
            n_members: Optional[int] = None):
        """Score the n_cand candidates of all events: cand_ptr_dev [n_cand + 1] int32 and cand_ids_dev int64
        (gtf_extract_out's form, not rebased), cand_first_dev [K + 1] int32 (candidate c belongs to the
        event e with cand_first[e] <= c < cand_first[e + 1]), all device arrays. n_members as
        DeviceScorer.add. Nothing synchronises."""
        nat = self.nat
        n_cand, group = int(n_cand), int(group)
        if n_cand == 0:
            if not per_candidate:
                self._all_per = False
            return
        if not cand_ids_dev.numel():      # (candidates without a member: the library still wants an array)
            cand_ids_dev = self._m.empty(1, np.int64)
        cap = int(cand_ids_dev.numel()) if n_members is None else int(n_members)
        nb = int(self.lib.gtf_score_ev_workspace_bytes(n_cand, cap, self.K))
        ws = self._m.empty(nb, np.uint8)
        out = nat.GtfScoreOut()
        if per_candidate:
            pid, good = self._m.empty(n_cand, np.int64), self._m.empty(n_cand, np.int32)
            out = nat.GtfScoreOut(self._p(pid), self._p(good), None, None)
            self._per.append({"group": group, "n": n_cand, "pid": pid, "good": good, "first": cand_first_dev,
                              "dead": np.zeros(self.K, bool)})
        else:
            self._all_per = False
        nat.check(self.lib.gtf_score_candidates_ev(ctypes.byref(self.batch), self._p(cand_ptr_dev),
                                                   self._p(cand_ids_dev), self._p(cand_first_dev), n_cand, group,
                                                   ctypes.byref(out), ctypes.byref(self.state), self._p(ws),
                                                   ctypes.c_size_t(nb), self.stream))
        if self.torch is None:
            self._keep.append(ws)      # (until results() has synchronised)

    def add_batch(self, cand_ptr_dev, cand_ids_dev, cand_first_dev, n_cand: int, group: int, n_members=None,
                  active=None):
        """what pipeline.run_batch calls once per iteration. ``active`` (the events that entered the
        iteration with nodes) is not needed here: an event without nodes has no candidates."""
        self.add(cand_ptr_dev, cand_ids_dev, cand_first_dev, n_cand, group, n_members=n_members)

    def results(self):
        """One Result per event (None where it has no truth) of everything added since the event's last
        reset; synchronises once. The purities are formed here, in fp64, from the integer records.
        reconstructed_pid / n_good / matched are filled when every add asked for per_candidate."""
        nat, m, K = self.nat, self._m, self.K
        r1 = max(self.R, 1)
        key, pid = m.empty(r1, np.uint64), m.empty(r1, np.int64)
        good, total, hits = (m.empty(r1, np.int32) for _ in range(3))
        first = m.empty(K + 1, np.int32)
        nb = int(self.lib.gtf_score_finish_ev_workspace_bytes(self.R, K))
        ws = m.empty(nb, np.uint8)
        n_rec, err = np.zeros(max(K, 1), np.int32), np.zeros(2, np.uint32)
        rc = self.lib.gtf_score_finish_ev(ctypes.byref(self.batch), ctypes.byref(self.state), self._p(key), self._p(pid),
                                          self._p(good), self._p(total), self._p(hits), self._p(first),
                                          ctypes.c_void_p(n_rec.ctypes.data), ctypes.c_void_p(err.ctypes.data),
                                          self._p(ws), ctypes.c_size_t(nb), self.stream)
        self._keep = []
        if rc == -2 and err[0] & nat.SCORE_ERR_MISSING:
            where = "event %d: " % int(err[1]) if int(err[1]) < K else ""
            raise ValueError(where + "a candidate node has no hit_dissociation")
        nat.check(rc)
        at = np.zeros(K + 1, np.int64)
        np.cumsum(n_rec[:K], out=at[1:])
        n = int(at[-1])
        g, t, h = (m.host(a, n, np.int32) for a in (good, total, hits))
        per = None
        if self._all_per and self._per:
            k = m.host(key, n, np.uint64)
            per = [dict(rec, first=m.host(rec["first"], K + 1, np.int32), pid=m.host(rec["pid"], rec["n"], np.int64),
                        good=m.host(rec["good"], rec["n"], np.int32)) for rec in sorted(self._per, key=lambda x: x["group"])]
        out = []
        for e in range(K):
            if not self.tables.scored[e]:
                out.append(None)
                continue
            a, b = int(at[e]), int(at[e + 1])
            ge = g[a:b] * 1.0
            with np.errstate(divide="ignore", invalid="ignore"):
                tpur, ppur = ge / t[a:b], ge / h[a:b]
            rp, ng, matched = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
            mine = [rec for rec in per if not rec["dead"][e]] if per is not None else []
            if mine:
                start, n_all = {}, 0
                for rec in mine:
                    start[rec["group"]] = n_all
                    n_all += int(rec["first"][e + 1]) - int(rec["first"][e])
                rp = np.concatenate([rec["pid"][rec["first"][e]:rec["first"][e + 1]] for rec in mine])
                ng = np.concatenate([rec["good"][rec["first"][e]:rec["first"][e + 1]] for rec in mine]).astype(np.int64)
                matched = np.zeros(n_all, bool)
                matched[[start[int(x >> np.uint64(32))] + int(x & np.uint64(0xffffffff)) for x in k[a:b]]] = True
            out.append(Result(b - a, self.tables.n_reference[e], tpur, ppur, rp, ng, matched))
        return out


def summary(r: Result) -> Dict[str, object]:
    return {"reconstructed": r.n_reconstructed, "reference": r.n_reference, "efficiency_pct": r.efficiency_str,
            "mean_track_purity": float(np.mean(r.track_purities)) if r.track_purities.size else None,
            "mean_particle_purity": float(np.mean(r.particle_purities)) if r.particle_purities.size else None}


def _truth_files_batch_parse(prefixes, mapping, min_volume, max_volume, device, mem, mark):
    """truth_files_batch_dev(batch_parse=True); mark as _truth_tables_batch_dev's, and "parsed" once the
    three kinds have been parsed"""
    import os
    from .csvdev import parse_batch_dev
    mm = _Mem(device, mem)
    K = len(prefixes)
    live = [e for e, q in enumerate(prefixes) if q is not None]
    with_truth = [e for e in live if os.path.isfile(prefixes[e] + "truth.csv")]
    infos = [None if q is None else {} for q in prefixes]
    batch_info, cols, offs = {}, {}, {}

    def read(key, events, suffix, columns):
        def host_reader(path):
            import pandas as pd
            f = pd.read_csv(path, usecols=[name for name, _ in columns])
            return [f[name].to_numpy(np.dtype(t)) for name, t in columns]

        c = parse_batch_dev([prefixes[e] + suffix for e in events], columns, 1, mm=mm, host_reader=host_reader)
        batch_info[key] = c.info
        sizes = np.zeros(K, np.int64)
        for k, e in enumerate(events):
            infos[e][key] = c.files[k]
            if c.reasons[k]:
                infos[e][key + "_reason"] = c.reasons[k]
            sizes[e] = int(c.row_off[k + 1]) - int(c.row_off[k])
        cols[key] = [c[name] for name, _ in columns]
        offs[key] = np.concatenate([[0], np.cumsum(sizes)])

    read("particles", live, "particles.csv", (("particle_id", "int64"), ("px", "float64"), ("py", "float64")))
    read("mapping", live, mapping, tuple((c, "int64") for c in MAPPING_COLUMNS))
    if with_truth:
        read("truth", with_truth, "truth.csv", (("hit_id", "int64"), ("particle_id", "int64")))
    else:
        cols["truth"], offs["truth"] = [None, None], np.zeros(K + 1, np.int64)
    for e in with_truth:    # (for the library no truth rows means "the mapping's own columns")
        if offs["truth"][e + 1] == offs["truth"][e] and offs["mapping"][e + 1] > offs["mapping"][e]:
            raise ValueError("event %d: a mapped hit has no truth row (helper.__get_particle_id .item())" % e)
    mark("parsed")
    d = _truth_tables_batch_dev([None if q is None else () for q in prefixes], min_volume, max_volume, device, mem, mark,
                                fused=(cols["mapping"] + cols["truth"] + cols["particles"], offs["mapping"],
                                       offs["truth"], offs["particles"]))
    d.parse_info = batch_info
    return d, infos
