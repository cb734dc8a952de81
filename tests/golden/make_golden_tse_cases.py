"""Golden record of the directed a2 cases (tests/tse_cases.py), made by the REFERENCE's own
helper.compute_track_state_estimates (helper.py:238-452).

Run here (the container that holds /root/reference), never on the GPU box:

    python tests/golden/make_golden_tse_cases.py     # writes tests/golden/tse_cases.npz

Every case that is pinned to the reference (tse_cases.Case.ref is None) is built unpadded in the
reference's schema (tse_cases.build), without the placeholder dicts, and run as one subgraph. Per
case the file holds either the reference's outputs packed onto the input's slots
(``<case>__slot__<field>`` for tse_rank, tse_sv, tse_tau, tse_cov, tse_xyzr, tse_theta and
tse_var_ms; ``<case>__node__<field>`` for xy_mean_var, zr_mean_var, angle_of_rotation and
translation), or ``<case>__raised``: the exception's type and the innermost reference source line
it left from ("LinAlgError helper.py:384"). ``<case>__node_id`` / ``<case>__slot_key`` pin the
layout the arrays are in. The file holds recorded results only; the inputs are rebuilt from
tse_cases at test time.

The oracle-only cases (absent keys, sparse ranks, ranks in and against the slot order) are not
recorded: a dict of the reference holds every neighbour at dense ranks in reversed set order. Nor
are the padded variants and fillers of tse_cases.everything(): their padding is keyless slots.
"""
import copy
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]

import make_golden as M  # noqa: E402  (shims, reference imports and pack)
import numpy as np  # noqa: E402
from make_golden_pass_cases import where_raised  # noqa: E402

import tse_cases as TC  # noqa: E402

NODE_ATTR = {"xy_mean_var": "xy_edge_gradient_mean_var", "zr_mean_var": "zr_edge_gradient_mean_var",
             "angle_of_rotation": "angle_of_rotation", "translation": "translation"}


def main():
    arrs = {}
    n_out = n_raise = 0
    p = TC.P
    for case in TC.CASES:
        if case.ref is not None:
            print("%-28s oracle-only: %s" % (case.name, case.ref))
            continue
        G, names, _ = TC.build(case)
        gin = M.pack([G])
        arrs[case.name + "__node_id"] = gin.node["node_id"]
        arrs[case.name + "__slot_key"] = gin.slot["slot_key"]
        R = copy.deepcopy(G)
        for n in R.nodes:
            del R.nodes[n]["track_state_estimates"]
        try:
            with warnings.catch_warnings(), M._Quiet():
                warnings.simplefilter("ignore", RuntimeWarning)   # (divisions by zero are cases here)
                out = M.h.compute_track_state_estimates([R], p.sigma0xy, p.sigma0rz, p.sigma0rz2, p.endcap_boundary)
        except Exception as exc:   # the reference's own exception: recorded, not modelled
            arrs[case.name + "__raised"] = np.array(where_raised(exc))
            print("%-28s raised %s" % (case.name, arrs[case.name + "__raised"]))
            n_raise += 1
            continue
        gout = M.pack(out, like=gin)
        assert np.array_equal(gin.slot_ptr, gout.slot_ptr)
        for f in ("tse_rank",) + TC.FIELDS:
            arrs["%s__slot__%s" % (case.name, f)] = gout.slot[f]
        for f, attr in NODE_ATTR.items():
            arrs["%s__node__%s" % (case.name, f)] = np.array([np.asarray(out[0].nodes[n][attr], dtype=np.float64)
                                                             for n in out[0].nodes], dtype=np.float64).reshape(
                (gout.n_nodes,) + ((2,) if f != "angle_of_rotation" else ()))
        n_out += 1
    path = os.path.join(HERE, "tse_cases.npz")
    np.savez_compressed(path, **arrs)
    print("wrote tse_cases.npz %.1f KB: %d cases with outputs, %d with a recorded exception" % (
        os.path.getsize(path) / 1024, n_out, n_raise))


if __name__ == "__main__":
    main()
