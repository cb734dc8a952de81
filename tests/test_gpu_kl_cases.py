"""The directed parabolic-KL cases (kl_cases.py, pinned to the reference by test_kl_cases.py) on the GPU.

Every case runs through ParabolicKL in each node layout -- listed, ordered (with degree runs and, with
GTF_KL_DEG_RUNS=0, without), tile = 4, 256 and 1, each with the 3- / 4-edge nodes in the tiles and by
list; tile-only cases in the tiled layouts alone -- and in each arithmetic path (f64, f32, q32). The
pair and truth buffers are pre-filled with NaN / 0x7f (alloc fills the others with NaN), so a block of
nodes that is skipped shows; results are mapped back through pair_index / host_nodes / host_slots.

  * rows and truth flags exact against the record in every layout and path; the error word equals the
    case's class: GTF_ERR_SINGULAR_H (128) where the record raises and, additionally, where only the
    kernel's geometric rule does ("kernel" cases: the reference returns unbounded values there); the
    other nodes of such a case are checked like any other;
  * f64: kl within 1e-8 of exact_kl (well-conditioned cases; in the named ill-conditioned ones the rule
    of test_gpu_parabolic._check_rows_vs_oracle), sv / cov rtol 1e-8 and atol 1e-12 max, emp_var 1e-9,
    emp_mean 1e-12 relative and 1e-15 absolute against the record, inf against inf and NaN against NaN;
  * all layouts of one path equal its first layout bit for bit in every output;
  * f32 and q32: finiteness and error class as in f64 (q32 adds flags exactly where its fixed-point xB
    is 0 or x0, evaluated in NumPy from quantise_xy); in the fp32-checked cases every distance within
    1e-3 (the project's P99_BAR, here a maximum) of exact_kl -- q32 on the de-quantised coordinates;
  * the output-selection and stride cases through the C-ABI directly, between guard bytes, and the host
    refusals (status -2, outputs untouched).
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import kl_cases as KC
from guard_mem import FILL, GUARD
from gtf import _native as nat

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
P99_BAR = 1e-3
LAYOUTS = (("listed", {}, "1"), ("ordered", {"ordered": True}, "1"), ("ordered_no_runs", {"ordered": True}, "0"),
           ("tile4", {"tile": 4}, "1"), ("tile4_list_b1", {"tile": 4, "tile_b1": False}, "1"),
           ("tile256", {"tile": 256}, "1"), ("tile256_list_b1", {"tile": 256, "tile_b1": False}, "1"),
           ("tile1", {"tile": 1}, "1"), ("tile1_list_b1", {"tile": 1, "tile_b1": False}, "1"))
DTYPES = ("f64", "f32", "q32")
FIELDS = ("kl", "truth", "emp_var", "emp_mean", "sv", "cov")


def layouts_of(c):
    return [lay for lay in LAYOUTS if "tile" in lay[1] or not c.tile_only]


def build(c, kw, runs, dtype, monkeypatch):
    from gtf.parabolic import ParabolicKL
    monkeypatch.setenv("GTF_KL_DEG_RUNS", runs)
    return ParabolicKL(c.ptr, c.src, c.gnn, c.truth, device=DEVICE, with_single=c.with_single, compact=dtype == "q32",
                       sort_window=c.sort_window, **kw)


def run(c, k, dtype):
    """one launch into sentinel-filled buffers; every output in the caller's order, pairs sorted by
    (node, i, j), and the error word"""
    out = k.alloc(dtype, emp=True, states=dtype != "q32")
    out["_kl"].fill_(float("nan"))
    if "_truth" in out:
        out["_truth"].fill_(0x7f)
    k.err.zero_()
    k.run(out, dtype)
    node, i, j = k.pair_index()
    key = np.lexsort((j, i, node))
    rows = KC.pair_rows(c)
    assert all(np.array_equal(a[key], b) for a, b in zip((node, i, j), rows)), "pair rows"
    got = {"kl": out["kl"].cpu().numpy()[key].astype(np.float64)}
    if "truth" in out:
        got["truth"] = out["truth"].cpu().numpy()[key]
    for f in ("emp_var", "emp_mean"):
        got[f] = k.host_nodes(out[f].cpu().numpy()).astype(np.float64)
    if "sv" in out:
        got["sv"], got["cov"] = k.host_slots(out["sv"].cpu().numpy()), k.host_slots(out["cov"].cpu().numpy())
    return got, k.errors()


@functools.lru_cache(maxsize=None)
def expectations(name):
    """what the record and the kernel's rule say of a case, computed once"""
    c, rec = KC.BY_NAME[name], KC.record()[name]
    rows = KC.pair_rows(c)
    knodes, kmask = KC.kernel_raising(c)
    raised = set(rec["raised_nodes"].tolist())
    truth = rec["truth"].copy()
    if c.truth is not None and raised:   # the record has no flag where the reference raised: the flag's definition
        t = c.truth
        for p in np.nonzero(np.isin(rows[0], list(raised)))[0]:
            v, a, b = rows[0][p], c.src[c.ptr[rows[0][p]] + rows[1][p]], c.src[c.ptr[rows[0][p]] + rows[2][p]]
            truth[p] = int(t[v] == t[a] and t[a] == t[b] and t[v] == t[b])
    listed = c.listed()
    clean_nodes = np.array([v for v in listed if v not in raised and v not in set(knodes.tolist())], np.int64)
    slots = np.concatenate([np.arange(c.ptr[v], c.ptr[v + 1]) for v in clean_nodes]) if clean_nodes.size else np.zeros(0, np.int64)
    sing_pairs = np.zeros(rows[0].size, bool)        # pairs one of whose slots the kernel's rule names
    if kmask.any():
        sing_pairs = kmask[c.ptr[rows[0]] + rows[1]] | kmask[c.ptr[rows[0]] + rows[2]]
    err = KC.ERR_SINGULAR_H if (raised & set(listed.tolist())) or knodes.size else 0
    return dict(rows=rows, truth=truth, compared=KC.compared_pairs(c, rec), clean_nodes=clean_nodes, clean_slots=slots,
                sing_pairs=sing_pairs, err=err, raised=raised, unlisted=np.setdiff1d(np.arange(c.n_nodes), listed))


def check_f64(c, rec, e, got):
    ex = KC.conditioning(c.name)["exact"] if e["compared"].any() else np.full(e["compared"].size, np.nan)
    m = np.isfinite(ex)
    assert np.array_equal(m, e["compared"] & m) and (m.sum() == e["compared"].sum() or c.kind == "singular")
    kl = got["kl"]
    if c.name in KC.ILL:   # the named ill-conditioned cases: the rule of test_gpu_parabolic._check_rows_vs_oracle
        far = m & ~(np.abs(kl - rec["kl"]) <= 1e-8 * np.abs(rec["kl"]))
        eg, eo = np.abs(kl[far] - ex[far]), np.abs(rec["kl"][far] - ex[far])
        assert (eg <= np.maximum(10 * eo, 1e-8 * np.abs(ex[far]))).all(), (c.name, kl[far], rec["kl"][far], ex[far])
    else:
        r = KC.rel_to_exact(kl, ex)
        assert r.size == m.sum() and (r <= 1e-8).all(), (c.name, float(np.nanmax(r)) if r.size else 0.0)
    assert not np.isfinite(kl[e["sing_pairs"]]).any(), "a pair of a singular edge is not finite"
    check_moments(c, rec, e, got)
    if c.states and e["clean_slots"].size:
        s = e["clean_slots"]
        floor = {"sv": sv_floor(c, s), "cov": 0.0}
        for f, ax in (("sv", 1), ("cov", (1, 2))):
            a, b = got[f][s], rec[f][s]
            off = ~within(a, b, ax, floor[f]).reshape(s.size, -1).all(axis=1)
            for k in s[off]:   # the record itself is off (a pivot of one ulp): the exact state decides
                v = int(np.searchsorted(c.ptr, k, side="right") - 1)
                x = KC.exact_state(c.gnn[v], c.gnn[c.src[k], :2])[f == "cov"][None]
                assert not within(rec[f][k][None], x, ax).all() and within(got[f][k][None], x, ax).all(), (c.name, f, int(k))
            assert off.sum() == 0 or c.kind == "singular", (c.name, f, int(off.sum()))


def within(a, b, ax, floor=0.0):
    """the project's bar for states: rtol 1e-8 and atol 1e-12 of the state's largest entry"""
    return np.abs(a - b) <= 1e-12 * np.abs(b).max(axis=ax, keepdims=True) + 1e-8 * np.abs(b) + floor


def sv_floor(c, slots):
    """The resolution of sv = mB (a2, b2, 0) in fp64, per slot [S, 3]: mB = xb sa + yb ca - yt is a sum of
    products of the coordinates with a cosine and a sine that are each a few ulp off (the reference's
    cos / sin(2 pi - atan2) more than the kernel's x / h, y / h), so it is known to 16 ulp of |x| + |y| +
    |xb| + |yb| and no better. Against an ordinary mB of millimetres that is 1e-12 relative and changes
    nothing; for a neighbour collinear with the origin and the node (mB = 0 in exact arithmetic) sv is this
    rounding and nothing else, and a relative bar alone cannot hold for it."""
    v = np.searchsorted(c.ptr, slots, side="right") - 1
    out = np.zeros((slots.size, 3))
    for n, (k, node) in enumerate(zip(slots, v)):
        nb = c.gnn[c.src[k], :2]
        x0, xB, _ = KC.kernel_geometry(c.gnn[node], nb[None])
        with np.errstate(all="ignore"):
            r2 = 1.0 / (xB[0] * (xB[0] - x0))
        out[n, :2] = 16 * 2.0 ** -53 * (np.abs(c.gnn[node, :2]).sum() + np.abs(nb).sum()) * np.abs([r2, x0 * r2])
    return out


def check_moments(c, rec, e, got):
    v = e["clean_nodes"]
    for f, rf, rtol, atol in (("emp_var", "gvar", 1e-9, 0.0), ("emp_mean", "gmean", 1e-12, 1e-15)):
        a, b = got[f][v], rec[rf][v]
        fin = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[np.isinf(b)], b[np.isinf(b)]), (c.name, f)
        assert (np.abs(a[fin] - b[fin]) <= rtol * np.abs(b[fin]) + atol).all(), (c.name, f)
        assert np.isnan(got[f][e["unlisted"]]).all(), "an unlisted node's moments are not written"


def dequantised(c, k):
    """the case with the coordinates the q32 path sees (q * scale, exact in fp64), caller's node order"""
    q = k.host_nodes(k.q.cpu().numpy()).astype(np.float64) * k.scale
    g = c.gnn.copy()
    g[:, :2] = q
    return dataclasses.replace(c, gnn=g)


def q32_flags(c, k):
    """(any listed node flagged, bool per pair: one of its slots flagged) by the q32 rule in NumPy"""
    q = k.host_nodes(k.q.cpu().numpy())
    mask = np.zeros(int(c.ptr[-1]), bool)
    for v in c.listed():
        mask[c.ptr[v]:c.ptr[v + 1]] = KC.q32_singular(q[v], q[c.src[c.ptr[v]:c.ptr[v + 1]]], k.scale)
    rows = KC.pair_rows(c)
    pairs = mask[c.ptr[rows[0]] + rows[1]] | mask[c.ptr[rows[0]] + rows[2]] if rows[0].size else np.zeros(0, bool)
    return bool(mask.any()), pairs


@pytest.mark.parametrize("name", [c.name for c in KC.CASES])
def test_case_in_every_layout_and_path(name, monkeypatch):
    c, rec = KC.BY_NAME[name], KC.record()[name]
    e = expectations(name)
    cond = KC.conditioning(name) if c.kind in KC.VALUE_KINDS and rec["kl"].size else None
    for dtype in DTYPES:
        first = None
        for lname, kw, runs in layouts_of(c):
            k = build(c, kw, runs, dtype, monkeypatch)
            got, err = run(c, k, dtype)
            if first is None:
                first, k0 = got, k
            else:
                for f in got:
                    assert np.array_equal(got[f], first[f], equal_nan=got[f].dtype.kind == "f"), (name, dtype, lname, f)
            want_err = e["err"]
            if dtype == "q32":
                if got is first:   # (the fixed-point coordinates are the same in every layout)
                    qany, qpairs = q32_flags(c, k)
                assert qany or not e["raised"], "q32 raises wherever the reference raises"
                want_err = KC.ERR_SINGULAR_H if qany else 0
            assert err == want_err, (name, dtype, lname, err, want_err)
        got = first
        if "truth" in got:
            assert np.array_equal(got["truth"], e["truth"]), (name, dtype, "truth")
        else:
            assert c.truth is None
        if dtype == "f64":
            check_f64(c, rec, e, got)
            kl64 = got["kl"]
            continue
        # f32 / q32: the finiteness pattern of f64, and the distances of the fp32-checked cases
        sing = e["sing_pairs"]
        ex = cond["exact"] if cond else None
        if dtype == "q32":
            sing = sing | qpairs
            assert not np.isfinite(got["kl"][qpairs]).any()
            if cond and cond["fp32"]:
                ex, _ = KC.exact_pairs(dequantised(c, k0), rec, sensitivity=False)
            q = k0.host_nodes(k0.q.cpu().numpy())
            for f in ("emp_var", "emp_mean"):   # finite exactly where no fixed-point dx is 0
                v = e["clean_nodes"]
                fin = np.array([bool((q[c.src[c.ptr[u]:c.ptr[u + 1]], 0] != q[u, 0]).all()) for u in v], bool)
                assert np.array_equal(np.isfinite(got[f][v]), fin), (name, f)
                same = np.isfinite(rec["gvar" if f == "emp_var" else "gmean"][v]) == fin
                assert same.all() or c.kind == "singular", (name, f, "a dx that is 0 in fixed point only")
        else:
            check_moments(c, rec, e, got)     # (PathD<float> forms the moments in fp64 like PathD<double>)
            assert not np.isfinite(got["kl"][e["sing_pairs"]]).any()
        # finite where f64 is, up to the range of the format: 2^24 below FLT_MAX (the distance is a sum of
        # products that cancel, so its terms can exceed it) fp32 may overflow where fp64 does not
        with np.errstate(invalid="ignore"):
            inrange = ~sing & ~(np.abs(kl64) > np.finfo(np.float32).max / 2.0 ** 24)
        assert np.array_equal(np.isfinite(got["kl"][inrange]), np.isfinite(kl64[inrange])), (name, dtype, "finiteness")
        if cond and cond["fp32"]:
            m = np.isfinite(ex) & ~sing
            r = KC.rel_to_exact(np.where(m, got["kl"], np.nan), np.where(m, ex, np.nan))
            print("%-28s %s pairs %5d max |kl - exact| / |exact| %.3e" % (name, dtype, r.size, r.max() if r.size else 0.0))
            assert (r <= P99_BAR).all(), (name, dtype, float(r.max()))


# --------------------------------------------------------------------------- the C-ABI between guard bytes
OUT_CASE = "mix_all_buckets"
SIZES = {"kl": 8, "truth": 1, "emp_var": 8, "emp_mean": 8, "sv": 24, "cov": 72, "err": 4}
COUNT = {"kl": "p", "truth": "p", "emp_var": "n", "emp_mean": "n", "sv": "s", "cov": "s", "err": 1}


def guarded_call(k, dtype, fields, mutate=None, q=None):
    """gtf_parabolic_kl (dtype f64 / f32) or gtf_parabolic_kl_q32 with the outputs `fields`, each between
    guard bytes and pre-filled with the guard pattern; returns (status, {field: payload bytes})"""
    import torch
    n = {"p": max(k.n_pairs, 1), "n": max(k.n_nodes, 1), "s": max(k.n_slots, 1)}
    el = dict(SIZES)
    if dtype != "f64":
        el["kl"] = 4
    if dtype == "q32":
        el["emp_var"] = el["emp_mean"] = 4
    bufs, size = {}, {}
    for f in fields:
        size[f] = el[f] * (n[COUNT[f]] if COUNT[f] != 1 else 1)
        bufs[f] = torch.full((GUARD + size[f] + GUARD,), FILL, dtype=torch.uint8, device=k.device)
    if "err" in bufs:
        bufs["err"][GUARD:GUARD + 4] = 0
    at = lambda f: ctypes.c_void_p(bufs[f].data_ptr() + GUARD) if f in bufs else ctypes.c_void_p(0)  # noqa: E731
    g = nat.GtfKlGraph.from_buffer_copy(k._g)
    if mutate:
        mutate(g)
    s = ctypes.c_void_p(torch.cuda.current_stream(k.device).cuda_stream)
    if dtype == "q32":
        o = nat.GtfKlOut32(at("kl"), at("truth"), at("emp_var"), at("emp_mean"), at("err"))
        rc = nat.lib().gtf_parabolic_kl_q32(ctypes.byref(g), ctypes.byref(q if q is not None else k._q), ctypes.byref(o), s)
    else:
        o = nat.GtfKlOut(at("kl"), at("truth"), at("emp_var"), at("emp_mean"), at("sv"), at("cov"), at("err"))
        rc = nat.lib().gtf_parabolic_kl(ctypes.byref(g), nat.GTF_F64 if dtype == "f64" else nat.GTF_F32, ctypes.byref(o), s)
    torch.cuda.synchronize()
    pay = {}
    for f, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + size[f]:] == FILL).all(), ("guard bytes", f)
        pay[f] = h[GUARD:GUARD + size[f]]
    return rc, pay


def reference_bytes(k, dtype):
    """the outputs of ParabolicKL.run as bytes, per field"""
    out = k.alloc(dtype, emp=True, states=dtype != "q32")
    k.err.zero_()
    k.run(out, dtype)
    ref = {f: out[f].cpu().numpy().reshape(-1).view(np.uint8) for f in FIELDS if f in out}
    ref["err"] = k.err.cpu().numpy().view(np.uint8)
    return ref


OUTPUT_SETS = {
    "all": ("kl", "truth", "emp_var", "emp_mean", "sv", "cov", "err"),
    "no_truth": ("kl", "emp_var", "emp_mean", "sv", "cov", "err"),
    "no_emp_var": ("kl", "truth", "emp_mean", "sv", "cov", "err"),
    "emp_var_only": ("kl", "truth", "emp_var", "sv", "cov", "err"),      # alloc(emp="var")
    "no_err": ("kl", "truth", "emp_var", "emp_mean", "sv", "cov"),
    "no_states": ("kl", "truth", "emp_var", "emp_mean", "err"),
    "kl_alone": ("kl",),
}


@pytest.mark.parametrize("layout", ["listed", "ordered", "ordered_no_runs", "tile4", "tile256_list_b1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_capi_output_selection(layout, dtype, monkeypatch):
    """each optional output NULL in turn, emp_mean NULL (emp="var"), sv / cov given (the STATES kernels of
    every bucket) and not: what is asked for equals the full run bit for bit, nothing else is written"""
    c = KC.BY_NAME[OUT_CASE]
    lname, kw, runs = [lay for lay in LAYOUTS if lay[0] == layout][0]
    k = build(c, kw, runs, dtype, monkeypatch)
    ref = reference_bytes(k, dtype)
    dev_listed = np.isin(k.node_of if k.node_of is not None else np.arange(c.n_nodes), c.listed())
    assert 0 < dev_listed.sum() < c.n_nodes
    for sname, fields in OUTPUT_SETS.items():
        fields = tuple(f for f in fields if dtype != "q32" or f not in ("sv", "cov"))
        rc, pay = guarded_call(k, dtype, fields)
        assert rc == 0, (sname, nat.lib().gtf_last_error())
        for f, b in pay.items():
            if f in ("emp_var", "emp_mean"):   # unlisted nodes keep the fill (alloc's NaN in the reference run)
                w = 4 if dtype == "q32" else 8
                a, r = b.reshape(-1, w), ref[f].reshape(-1, w)
                assert np.array_equal(a[dev_listed], r[dev_listed]) and (a[~dev_listed] == FILL).all(), (sname, f)
            else:
                assert np.array_equal(b, ref[f]), (sname, f)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layout", ["listed", "ordered", "tile4"])
def test_capi_gnn_stride(layout, dtype, monkeypatch):
    """gnn_stride 0 and 4 (x, y, z, r rows) give stride 2's results bit for bit"""
    import torch
    c = KC.BY_NAME[OUT_CASE]
    lname, kw, runs = [lay for lay in LAYOUTS if lay[0] == layout][0]
    k = build(c, kw, runs, dtype, monkeypatch)
    assert k._g.gnn_stride == 2
    fields = OUTPUT_SETS["all"]
    rc, base = guarded_call(k, dtype, fields)
    assert rc == 0
    rows = c.gnn if k.node_of is None else c.gnn[k.node_of]
    rows = rows.copy()
    rows[:, 2:] = np.nan      # z and r are not read
    full = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).to(k.device)
    for stride in (0, 4):
        def mutate(g, stride=stride):
            g.gnn, g.gnn_stride = ctypes.c_void_p(full.data_ptr()), stride
        rc, pay = guarded_call(k, dtype, fields, mutate)
        assert rc == 0
        for f in fields:
            assert np.array_equal(pay[f], base[f]), (stride, f)


def test_capi_host_refusals(monkeypatch):
    """sv without cov, a truth output without graph truth, a bad stride, a bad ordered layout (and the q32
    entry's truth output without truth32, a bad scale): status -2, every output untouched"""
    c = KC.BY_NAME[OUT_CASE]
    k = build(c, {}, "1", "q32", monkeypatch)
    ko = build(c, {"ordered": True}, "1", "f64", monkeypatch)
    every = OUTPUT_SETS["all"]

    def refused(k, dtype, fields, mutate=None, q=None):
        rc, pay = guarded_call(k, dtype, fields, mutate, q)
        assert rc == -2, (rc, fields)
        for f, b in pay.items():
            assert (b == FILL).all() or (f == "err" and (b == 0).all()), f
        return nat.lib().gtf_last_error()

    def set_(**kw):
        def mutate(g):
            for f, v in kw.items():
                setattr(g, f, v)
        return mutate

    for dtype in ("f64", "f32"):
        refused(k, dtype, tuple(f for f in every if f != "cov"))
        refused(k, dtype, tuple(f for f in every if f != "sv"))
        refused(k, dtype, every, set_(truth=None))
        for stride in (1, 3, -2, 8):
            refused(k, dtype, every, set_(gnn_stride=stride))
        refused(ko, dtype, every, set_(n_d1=ko._g.count[0] + 1))
        refused(ko, dtype, every, set_(deg_runs=2))
        refused(ko, dtype, every, set_(slot0=-1))

        def short_runs(g):
            g.n_deg[0] = g.n_deg[0] + 1
        refused(ko, dtype, every, short_runs)
    q_every = ("kl", "truth", "emp_var", "emp_mean", "err")
    refused(k, "q32", q_every, q=nat.GtfKlQ32(k._q.xy, k._q.scale, None))
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        refused(k, "q32", q_every, q=nat.GtfKlQ32(k._q.xy, scale, k._q.truth32))
    # and the same calls, not mutated, are accepted
    assert guarded_call(k, "f64", every)[0] == 0 and guarded_call(ko, "f64", every)[0] == 0
    assert guarded_call(k, "q32", q_every)[0] == 0
