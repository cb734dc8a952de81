"""Hand-made inputs of gtf_event_errors / gtf.graph.event_errors, shared by the CPU self-check
(tests/test_event_error_cases.py) and the C-ABI test (tests/test_gpu_event_errors.py): (node_err [N] uint32,
event [N] int32 or None, K, mask, node_id [N] int64), and the definition once more as a plain Python loop."""
import numpy as np

TIE, NAN_KL, SEND = 8, 32, 1   # GTF_ERR_TIE_EMPTIED, GTF_ERR_NAN_KL, GTF_ERR_SEND_MW_MISSING
ALL = 0xFFFFFFFF


def _ids(n, seed=0):
    """distinct int64 node ids beyond 2^32, in no order"""
    return (np.random.RandomState(seed).permutation(n).astype(np.int64) + 1) * 4294967311 % (1 << 40)


def _case(sizes, raising, mask=ALL, event=True, seed=0):
    """events of ``sizes`` nodes; raising: {(event, node inside it): bits}"""
    sizes = np.asarray(sizes, np.int64)
    K, N = sizes.size, int(sizes.sum())
    ev = np.repeat(np.arange(K, dtype=np.int32), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    err = np.zeros(N, np.uint32)
    for (e, i), bits in raising.items():
        assert 0 <= i < sizes[e]
        err[off[e] + i] = bits
    return err, (ev if event else None), K, mask, _ids(N, seed)


def _random(seed):
    r = np.random.RandomState(seed)
    K = int(r.randint(1, 40))
    sizes = r.randint(0, 300, K) * (r.rand(K) > 0.2)
    N = int(sizes.sum())
    ev = np.repeat(np.arange(K, dtype=np.int32), sizes)
    err = np.where(r.rand(N) < 0.01, r.randint(1, 2048, N), 0).astype(np.uint32)
    mask = int(r.choice([ALL, TIE | NAN_KL, 0x7FF & ~TIE]))
    return err, ev, K, mask, _ids(N, seed)


def cases():
    """{name: (node_err, event, K, mask, node_id)}"""
    c = {
        "n0": _case([0, 0, 0], {}),
        "n0_k0": (np.zeros(0, np.uint32), np.zeros(0, np.int32), 0, ALL, np.zeros(0, np.int64)),
        "one_event_null": _case([300], {(0, 17): TIE, (0, 299): NAN_KL}, event=False),
        "one_event_null_clean": _case([65], {}, event=False),
        "first_node": _case([5, 70, 5], {(1, 0): TIE}),
        "last_node": _case([5, 70, 5], {(1, 69): TIE}),
        "or_together": _case([10, 10], {(1, 2): TIE, (1, 7): NAN_KL}),
        "masked_out": _case([10, 10, 10], {(0, 3): SEND, (2, 1): TIE | SEND}, mask=TIE),
        "every_event": _case([3, 64, 1, 257], {(0, 2): TIE, (1, 63): SEND, (2, 0): NAN_KL, (3, 256): TIE, (3, 0): SEND}),
        "empty_first_middle_last": _case([0, 0, 9, 0, 0, 130, 0], {(2, 8): TIE, (5, 129): SEND}),
        "wave_bounds": _case([1, 63, 64, 65, 1], {(1, 62): TIE, (2, 0): SEND, (3, 64): NAN_KL}),
        "block_bounds": _case([255, 256, 257, 1], {(0, 254): TIE, (1, 0): SEND, (1, 255): NAN_KL, (2, 256): TIE}),
        "clean": _case([100, 257, 3], {}),
    }
    for K in (65, 257, 2049):
        c["k%d" % K] = _case([1] * K, {(0, 0): TIE, (K // 2, 0): SEND, (K - 1, 0): NAN_KL | TIE})
    for seed in range(5):
        c["random%d" % seed] = _random(seed)
    return c


def bad_cases():
    """{name: (node_err, event, K, mask, node_id, the first offending node)}: event columns outside the contract"""
    err, ev, K, mask, ids = _case([40, 300, 40], {(1, 5): TIE})
    dec, neg, big = ev.copy(), ev.copy(), ev.copy()
    dec[200] = 0          # (so node 200 is below its predecessor; 201 is not a violation of node 200's value)
    neg[0] = -1
    big[379] = K
    return {"decreasing": (err, dec, K, mask, ids, 200), "minus_one": (err, neg, K, mask, ids, 0),
            "k": (err, big, K, mask, ids, 379)}


def by_loop(node_err, event, K, mask, node_id):
    """the definition as a plain loop over the nodes"""
    N = len(node_err)
    err_ev, n_raising = np.zeros(K, np.uint32), np.zeros(K, np.int32)
    first_node, first_id = np.full(K, -1, np.int32), np.full(K, -1, np.int64)
    for v in range(N):
        e = 0 if event is None else int(event[v])
        bits = int(node_err[v]) & mask
        if bits:
            err_ev[e] |= np.uint32(bits)
            n_raising[e] += 1
            if first_node[e] < 0:
                first_node[e], first_id[e] = v, node_id[v]
    keep = np.array([0 if err_ev[0 if event is None else int(event[v])] else 1 for v in range(N)], np.uint8)
    return err_ev, n_raising, first_node, first_id, keep
