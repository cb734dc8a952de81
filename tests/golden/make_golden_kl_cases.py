"""Golden record of the directed parabolic-KL cases (tests/kl_cases.py), made by the REFERENCE's own
functions of learn_KL_parabolic_model/src/generate_training_data.

Run where the reference lies beside the repository, never on the GPU box:

    python tests/golden/make_golden_kl_cases.py     # writes tests/golden/kl_cases.npz

utils.py imports modules that are not needed here and extract_metadata_trackml_parabolic_model.py is a
script (file reads at module level), so neither is imported: the functions are taken out of the files
with ``ast``, as make_golden_a15.py::reference_function does, and executed in a namespace holding what
the files' own imports bind (numpy as np, networkx as nx, ``from math import *``):

  utils.py                                          compute_track_state_estimates, rotate_track,
                                                    getAngleBetweenPoints, angle_trunc
  extract_metadata_trackml_parabolic_model.py       KLDistance, calc_pairwise_distances

Each case becomes a networkx.DiGraph whose nodes carry an object with .x and .y (``GNN_Measurement``)
and ``truth_particle``. compute_track_state_estimates loops over G.nodes() and stops at the first node
that raises; to know what it does at EVERY receiver it is called once per receiver on a view of the
graph whose nodes() yields that receiver alone (everything else is the DiGraph's). Then the script's
per-node loop (:56-98) is restated: the states in the dict's order (the reversed neighbour order,
utils.py:254-255), reshape to (num_edges, 3, 3), np.linalg.inv, calc_pairwise_distances, and the truth
flag of :95. Senders (no in-edge) have num_edges = 0 and are skipped by :62; their states, which the
reference also forms from their out-edges, are not visited here.

Per case the file holds, in the case's own slot / node / pair order (pairs node by node, row-major
lower triangle i > j over the slots):
  <case>__sv [S, 3], <case>__cov [S, 3, 3]    per slot (only for Case.states), NaN where the node raised
  <case>__gmean, <case>__gvar [N]             xy_edge_gradient_mean_var, NaN for nodes without in-edge
  <case>__kl [P], <case>__truth [P]           pairwise_distances[i][j] and the flag; NaN / 0 where raised
                                              (a case without truth ids has no flag: zeros)
  <case>__raised_nodes, <case>__raised        the receivers at which the reference raised, and the
                                              exception's type and source line for each
The file holds recorded results only; the inputs are rebuilt from kl_cases at test time.
"""
import ast
import math
import os
import sys
import traceback
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"),
                os.path.join(os.path.dirname(os.path.dirname(HERE)), "gnn-track-finding_amd")]

import networkx as nx  # noqa: E402
import numpy as np  # noqa: E402
from make_golden_a15 import REF_FILE as A15_FILE  # noqa: E402

import kl_cases as KC  # noqa: E402

REF_DIR = os.path.join(os.path.dirname(os.path.dirname(A15_FILE)), "learn_KL_parabolic_model", "src", "generate_training_data")
UTILS = os.path.join(REF_DIR, "utils.py")
SCRIPT = os.path.join(REF_DIR, "extract_metadata_trackml_parabolic_model.py")


def reference_functions():
    """the reference's own functions, compiled from its own source into one namespace"""
    ns = {"np": np, "nx": nx}
    ns.update({k: getattr(math, k) for k in dir(math) if not k.startswith("_")})   # from math import *
    for path, names in ((UTILS, ("compute_track_state_estimates", "rotate_track", "getAngleBetweenPoints", "angle_trunc")),
                        (SCRIPT, ("KLDistance", "calc_pairwise_distances"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in fn) == sorted(names)
        exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns


class Meas:
    def __init__(self, x, y):
        self.x, self.y = np.float64(x), np.float64(y)


class OneNode:
    """the DiGraph G as compute_track_state_estimates sees it when its loop visits node v alone"""

    class _Nodes:
        def __init__(self, G, v):
            self.G, self.v = G, v

        def __call__(self, *a, **k):
            return [self.v]

        def __getitem__(self, n):
            return self.G.nodes[n]

    def __init__(self, G, v):
        self._G = G
        self.nodes = OneNode._Nodes(G, v)

    def __getattr__(self, name):
        return getattr(self._G, name)


def digraph(c):
    G = nx.DiGraph()
    for v in range(c.n_nodes):
        G.add_node(v, GNN_Measurement=Meas(c.gnn[v, 0], c.gnn[v, 1]),
                   truth_particle=int(c.truth[v]) if c.truth is not None else 0)
    for v in range(c.n_nodes):
        for k in range(c.ptr[v], c.ptr[v + 1]):   # predecessors in slot order
            G.add_edge(int(c.src[k]), v)
    return G


def where_raised(exc):
    """the exception's type and the reference's line it came from; the script's loop is restated here, so
    its own np.linalg.inv (:78) is named by that line"""
    fs = [f for f in traceback.extract_tb(exc.__traceback__) if f.filename in (UTILS, SCRIPT)]
    if not fs:
        assert isinstance(exc, np.linalg.LinAlgError), exc
        return "%s %s:78" % (type(exc).__name__, os.path.basename(SCRIPT))
    f = fs[-1]
    return "%s %s:%d" % (type(exc).__name__, os.path.basename(f.filename), f.lineno)


def record_case(c, ref):
    G = digraph(c)
    S, N, pp = int(c.ptr[-1]), c.n_nodes, c.pair_ptr()
    sv, cov = np.full((S, 3), np.nan), np.full((S, 3, 3), np.nan)
    gmean, gvar = np.full(N, np.nan), np.full(N, np.nan)
    kl, truth = np.full(int(pp[-1]), np.nan), np.zeros(int(pp[-1]), np.int8)
    raised_nodes, raised = [], []
    for v in np.nonzero(c.degree > 0)[0]:
        v = int(v)
        lo, d = int(c.ptr[v]), int(c.degree[v])
        senders = [int(u) for u in c.src[lo:lo + d]]
        assert len(set(senders)) == d, "one dict entry per slot: a receiver's senders are distinct"
        try:
            ref["compute_track_state_estimates"]([OneNode(G, v)])
            attr = G.nodes[v]
            tse = attr["track_state_estimates"]
            gmean[v], gvar[v] = attr["xy_edge_gradient_mean_var"]
            keys = list(tse.keys())
            assert keys == senders[::-1]                         # the dict runs in reversed neighbour order
            for q, u in enumerate(keys):
                sv[lo + d - 1 - q] = tse[u]["edge_state_vector"]
                cov[lo + d - 1 - q] = tse[u]["edge_covariance"]
            if d <= 1:
                continue
            # the script's per-node loop (:60-98)
            num_edges = d
            edge_svs = np.array([comp["edge_state_vector"] for comp in tse.values()])
            edge_covs = np.array([comp["edge_covariance"] for comp in tse.values()])
            edge_covs = np.reshape(edge_covs[:, :, np.newaxis], (num_edges, 3, 3))
            inv_covs = np.linalg.inv(edge_covs)                  # :78
            dist = ref["calc_pairwise_distances"](num_edges, edge_svs, edge_covs, inv_covs)
            node_truth = attr["truth_particle"]
            for i in range(d):
                for j in range(i):       # slots i > j are the dict's entries d-1-i < d-1-j
                    kl[pp[v] + i * (i - 1) // 2 + j] = dist[d - 1 - j][d - 1 - i]
                    t1, t2 = G.nodes[keys[d - 1 - j]]["truth_particle"], G.nodes[keys[d - 1 - i]]["truth_particle"]
                    if c.truth is not None and (node_truth == t1) and (t1 == t2) and (node_truth == t2):
                        truth[pp[v] + i * (i - 1) // 2 + j] = 1
        except (np.linalg.LinAlgError, ZeroDivisionError, ValueError) as exc:   # the reference's own: recorded, not modelled
            raised_nodes.append(v)
            raised.append(where_raised(exc))
            sv[lo:lo + d], cov[lo:lo + d] = np.nan, np.nan
            kl[pp[v]:pp[v + 1]], truth[pp[v]:pp[v + 1]] = np.nan, 0
    out = {"gmean": gmean, "gvar": gvar, "kl": kl, "truth": truth}
    if c.states:
        out["sv"], out["cov"] = sv, cov
    if raised_nodes:
        out["raised_nodes"], out["raised"] = np.array(raised_nodes, np.int64), np.array(raised)
    return out


def main():
    ref = reference_functions()
    arrs = {}
    n_pairs = n_raised = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for c in KC.CASES:
            r = record_case(c, ref)
            for k, a in r.items():
                arrs[c.name + "__" + k] = a
            n_pairs += r["kl"].size
            if "raised" in r:
                n_raised += len(r["raised"])
                print("%-28s raised at %d nodes: %s" % (c.name, len(r["raised"]), sorted(set(r["raised"].tolist()))))
    path = os.path.join(HERE, "kl_cases.npz")
    np.savez_compressed(path, **arrs)
    print("wrote kl_cases.npz %.1f KB: %d cases, %d pairs, %d nodes with a recorded exception" % (
        os.path.getsize(path) / 1024, len(KC.CASES), n_pairs, n_raised))


if __name__ == "__main__":
    main()
