"""The compact (32-bit fixed-point) input mode of the parabolic KL stage, without a GPU: the
quantisation rule of gtf.parabolic.quantise_xy, the layout of gtf_kl_q32 / gtf_kl_out32
against include/gtf.h, the host-side validation of gtf_parabolic_kl_q32 (-2 before any
device work) and the Python wrapper's refusals."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")


@pytest.mark.parametrize("peak, log2_scale", [(175.69, -22), (1100.0, -19)])
def test_quantise_xy_rule(peak, log2_scale):
    """scale = 2^(e - 30), e the smallest integer with every |x|, |y| < 2^e; |q| < 2^30;
    q * scale within scale / 2 of the input"""
    from gtf.parabolic import quantise_xy
    rng = np.random.default_rng(1)
    xy = rng.uniform(-peak, peak, (1000, 2))
    xy[17, 1] = -peak                       # the largest magnitude, on a negative y
    gnn = np.concatenate([xy, rng.uniform(-3000, 3000, (1000, 2))], 1)   # z, r play no part
    q, scale = quantise_xy(gnn)
    assert q.dtype == np.int32 and q.shape == (1000, 2) and q.flags["C_CONTIGUOUS"]
    assert scale == 2.0 ** log2_scale
    m, e = np.frexp(scale)
    assert m == 0.5 and e - 1 == log2_scale    # a power of two
    assert np.abs(q.astype(np.int64)).max() < 2 ** 30
    assert np.abs(q * scale - xy).max() <= scale / 2
    q2, s2 = quantise_xy(xy)                  # [N, 2] input: the same
    assert s2 == scale and np.array_equal(q2, q)


def test_quantise_xy_edges():
    from gtf.parabolic import quantise_xy
    # exactly 2^e is not < 2^e: the next exponent
    q, scale = quantise_xy(np.array([[256.0, 1.0]]))
    assert scale == 2.0 ** -21 and q[0, 0] == 2 ** 29
    q, scale = quantise_xy(np.array([[np.nextafter(256.0, 0.0), 1.0]]))
    assert np.abs(q.astype(np.int64)).max() < 2 ** 30   # (would round to 2^30 at 2^-22)
    q, scale = quantise_xy(np.array([[255.0, -1.0]]))
    assert scale == 2.0 ** -22
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            quantise_xy(np.array([[1.0, 2.0], [bad, 0.0]]))
    # a given scale is kept; coordinates beyond its range raise
    q, scale = quantise_xy(np.array([[100.0, -3.0]]), scale=2.0 ** -22)
    assert scale == 2.0 ** -22 and q[0, 0] == 100 * 2 ** 22
    with pytest.raises(ValueError):
        quantise_xy(np.array([[256.0, 0.0]]), scale=2.0 ** -22)


def test_q32_struct_layout_matches_header():
    """offsetof() / sizeof() of gtf_kl_q32 and gtf_kl_out32 from a compiled C probe of the
    header against the ctypes mirrors"""
    from gtf import _native as nat
    py = {"gtf_kl_q32": nat.GtfKlQ32, "gtf_kl_out32": nat.GtfKlOut32}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as f:
            f.write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values())
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    assert [f for f, _ in nat.GtfKlOut32._fields_] == ["kl", "truth", "emp_var", "emp_mean", "err"]


def _graph_one_pair(nat, keep):
    """a listed graph of three nodes, node 2 with in-edges from 0 and 1 (one pair); the host
    arrays only have to be non-null: every case below is refused before any device work"""
    ptr = np.array([0, 0, 0, 2], np.int32)
    src = np.array([0, 1], np.int32)
    pair = np.array([0, 0, 0, 1], np.int64)
    lst = np.array([2], np.int32)
    keep += [ptr, src, pair, lst]
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    return nat.GtfKlGraph(3, 2, vp(ptr), vp(src), None, None, vp(pair),
                          (ctypes.c_void_p * 4)(lst.ctypes.data, None, None, None), (ctypes.c_int32 * 4)(1, 0, 0, 0))


@pytest.mark.parametrize("case, word", [("scale0", b"scale"), ("scale_inf", b"scale"), ("scale_nan", b"scale"),
                                        ("scale_neg", b"scale"), ("null_q", b"null argument"),
                                        ("null_out", b"null argument"), ("no_xy", b"missing arrays"),
                                        ("truth_without_truth32", b"truth32"), ("bad_list", b"bad node list")])
def test_q32_entry_point_validates_on_the_host(case, word):
    """gtf_parabolic_kl_q32 returns -2 with gtf_last_error naming the fault, without a GPU"""
    from gtf import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib()
    keep = []
    g = _graph_one_pair(nat, keep)
    xy = np.zeros(6, np.int32)
    t32 = np.zeros(3, np.int32)
    kl = np.zeros(1, np.float32)
    flag = np.zeros(1, np.int8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    q = nat.GtfKlQ32(vp(xy), 2.0 ** -22, vp(t32))
    o = nat.GtfKlOut32(vp(kl), None, None, None, None)
    qp, op = ctypes.byref(q), ctypes.byref(o)
    if case == "scale0":
        q.scale = 0.0
    elif case == "scale_inf":
        q.scale = float("inf")
    elif case == "scale_nan":
        q.scale = float("nan")
    elif case == "scale_neg":
        q.scale = -2.0 ** -22
    elif case == "null_q":
        qp = None
    elif case == "null_out":
        op = None
    elif case == "no_xy":
        q.xy = None
    elif case == "truth_without_truth32":
        q.truth32 = None
        o.truth = vp(flag)
    elif case == "bad_list":
        g.count[1] = 5            # a count without its list, in a listed graph
    rc = L.gtf_parabolic_kl_q32(ctypes.byref(g), qp, op, ctypes.c_void_p(0))
    msg = L.gtf_last_error()
    assert rc == -2 and msg.startswith(b"gtf_parabolic_kl_q32: ") and word in msg, (rc, msg)


def test_q32_and_f64_share_the_ordered_layout_checks():
    """the ordered-layout range checks are one function for both entry points: the same
    out-of-range graph is refused by each under its own name"""
    from gtf import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib()
    g = nat.GtfKlGraph(n_nodes=4, n_slots=4, gnn_stride=2)
    g.count[0], g.first[0], g.n_d1 = 4, 2, 0          # nodes [2, 6) of 4; 8 slots of 4
    z = ctypes.c_void_p(0)
    rc = L.gtf_parabolic_kl(ctypes.byref(g), 0, ctypes.byref(nat.GtfKlOut()), z)
    assert rc == -2 and L.gtf_last_error() == b"gtf_parabolic_kl: bad ordered layout"
    q = nat.GtfKlQ32(None, 2.0 ** -22, None)
    rc = L.gtf_parabolic_kl_q32(ctypes.byref(g), ctypes.byref(q), ctypes.byref(nat.GtfKlOut32()), z)
    assert rc == -2 and L.gtf_last_error() == b"gtf_parabolic_kl_q32: bad ordered layout"


def _cpu_kl(**kw):
    from gtf.parabolic import ParabolicKL
    gnn = np.array([[10.0, 5.0, 0, 11.18], [10.0, 0.5, 0, 10.0], [20.0, 1.0, 0, 20.0]])
    return ParabolicKL(np.array([0, 0, 2, 2], np.int32), np.array([0, 2], np.int32), gnn,
                       np.array([7, 7, 8], np.int64), device="cpu", **kw)


def test_wrapper_refusals_need_no_device():
    """run(out, "q32") on an object built without compact=True raises, alloc("q32",
    states=True) raises, buffers of another dtype are refused, and truth ids beyond int32
    are relabelled at construction (host tensors: nothing here launches)"""
    import torch
    from gtf.parabolic import ParabolicKL
    k = _cpu_kl()
    assert k.q is None and k.truth32 is None
    with pytest.raises(ValueError, match="compact=True"):
        k.run(k.alloc("q32"), "q32")
    kc = _cpu_kl(compact=True)
    with pytest.raises(ValueError, match="sv / cov"):
        kc.alloc("q32", states=True)
    with pytest.raises(ValueError, match="alloc"):
        kc.run(kc.alloc("f32"), "q32")          # emp_var is fp64 there
    out = kc.alloc("q32")
    assert out["kl"].dtype == out["emp_var"].dtype == out["emp_mean"].dtype == torch.float32
    assert kc.q.dtype == torch.int32 and tuple(kc.q.shape) == (3, 2) and kc.truth32.dtype == torch.int32
    assert kc.scale == 2.0 ** -25               # max |xy| = 20 < 2^5
    # truth ids beyond int32 (TrackML particle ids) go as dense labels, equal where the ids are
    big = np.array([932245878779936768, 7, 932245878779936768], np.int64)
    gnn = np.array([[10.0, 5.0, 0, 11.18], [10.0, 0.5, 0, 10.0], [20.0, 1.0, 0, 20.0]])
    kb = ParabolicKL(np.array([0, 0, 2, 2], np.int32), np.array([0, 2], np.int32), gnn, big, device="cpu",
                     compact=True)
    t32 = kb.truth32.numpy()
    assert t32.dtype == np.int32 and t32[0] == t32[2] != t32[1]
    assert kc.truth32.tolist() == [7, 7, 8]     # ids that fit are kept


def test_footprint_counts_the_chosen_path():
    """without compact the footprint is what it was; the q32 path counts the 8-byte
    coordinates and 4-byte ids instead of the 16- and 8-byte ones"""
    k, kc = _cpu_kl(), _cpu_kl(compact=True)
    o64, o32 = k.alloc("f64"), kc.alloc("q32")
    assert k.footprint_bytes(o64) == kc.footprint_bytes(kc.alloc("f64"))
    shared = sum(t.numel() * t.element_size() for t in [k.slot_ptr, k.slot_src, k.pair_ptr] + k.lists)
    assert k.footprint_bytes(o64) == shared + 3 * 24 + (8 + 1 + 2 * 3 * 8)    # one pair: kl, flag; moments
    assert kc.footprint_bytes(o32, "q32") == shared + 3 * 12 + (4 + 1 + 2 * 3 * 4)
