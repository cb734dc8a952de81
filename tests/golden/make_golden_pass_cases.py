"""Golden record of the directed fused-pass cases (tests/pass_cases.py), made by the REFERENCE's
own stage functions.

Run here (the container that holds /root/reference), never on the GPU box:

    python tests/golden/make_golden_pass_cases.py     # writes tests/golden/pass_cases.npz

Every case is built unpadded in the reference's schema (pass_cases.build) and run, one component
at a time, through the stage it names: extrapolate_merged_states' message passing, priors,
reweights and degree (make_golden.run_extrapolate), remove_state_metadata.py (run_update),
clustering.cluster (run_cluster), the three chained for a full pass, or the helper functions a
list of node ops names. Per case the file holds either the output arrays of make_golden.OUT_FIELDS
packed onto the input's slots (``<case>__node__<field>`` / ``<case>__slot__<field>``), or
``<case>__raised``: the exception's type and the innermost reference source line it left from
("KeyError helper.py:131"). ``<case>__node_id`` / ``<case>__slot_key`` pin the layout the arrays
are in. The file holds recorded results only; the inputs are rebuilt from pass_cases at test time.

The padded variants of a case are not recorded: the padding (inactive in-edges without a dict key,
from senders without a merged state) changes nothing these functions compute at the case's own
nodes, so tests/test_pass_cases.py compares every variant with the one record.

Cases the reference cannot take, which stay oracle-only (pass_cases.Case.ref):

  * rw_w_one_threshold_one, rw_w_quarter_threshold_quarter, rw_w_quarter_threshold_ulp_above: the
    reference hard-codes reweight_threshold = 0.1 (helper.py:145), so it cannot run another
    threshold. The equality branch ``w < threshold`` is pinned to the reference by
    rw_w_equals_reference_threshold instead, whose weights are exactly 0.1;
  * cl_*_tie_empties_list under tie_policy="stop": the reference raises (clustering.py:116;
    recorded), and the merged state include/gtf.h promises to keep has no
    reference value.
"""
import copy
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]

import make_golden as M  # noqa: E402  (shims, reference imports, run_* and pack helpers)
import numpy as np  # noqa: E402

import pass_cases as PC  # noqa: E402

h = M.h
KEY = {"tse": "track_state_estimates", "uts": "updated_track_states"}


def _helpers(subs, op):
    subs = copy.deepcopy(subs)
    with M._Quiet():
        if op in ("priors_tse", "priors_uts"):
            h.compute_prior_probabilities(subs, KEY[op[-3:]])
        elif op in ("mw_tse", "mw_uts"):
            h.compute_mixture_weights(subs, KEY[op[-3:]])
        elif op == "reweight_uts":
            h.reweight(subs, KEY["uts"])
        elif op == "degree":
            for s in subs:
                for n in s.nodes:
                    s.nodes[n]["degree"] = h.query_node_degree_in_edges(s, n)
        else:
            raise KeyError(op)
    return subs


def run_reference(case, subs, p):
    """the case's stage through the reference; the P of make_golden carries the case's Params"""
    saved = dict(M.P)
    M.P.update(sigma0xy=p.sigma0xy, sigma0rz=p.sigma0rz, sigma0rz2=p.sigma0rz2, endcap_boundary=p.endcap_boundary,
               chi2_cut=p.chi2_cut)
    try:
        st = case.stage
        if st == "extrapolate":
            return M.run_extrapolate(subs)
        if st == "update":
            return M.run_update(subs)
        if st in ("cluster_uts", "cluster_tse"):
            return M.run_cluster(subs, KEY[st[-3:]], p.cluster_chi2, p.cluster_kl)
        if st == "full_pass":
            return M.run_cluster(M.run_update(M.run_extrapolate(subs)), KEY["uts"], p.cluster_chi2, p.cluster_kl)
        ops = list(st)
        while ops:
            if tuple(ops[:4]) == PC.UPDATE_OPS:
                subs, ops = M.run_update(subs), ops[4:]
            else:
                subs, ops = _helpers(subs, ops[0]), ops[1:]
        return subs
    finally:
        M.P.clear()
        M.P.update(saved)


def where_raised(exc):
    """'<type> <file>:<line>' of the innermost frame inside the reference's sources"""
    frames = [f for f in traceback.extract_tb(exc.__traceback__) if f.filename.startswith(M.REF)]
    f = frames[-1]
    return "%s %s:%d" % (type(exc).__name__, os.path.basename(f.filename), f.lineno)


def main():
    arrs = {}
    n_out = n_raise = 0
    for case in PC.CASES:
        if case.ref is not None:
            print("%-40s oracle-only: %s" % (case.name, case.ref))
            continue
        subs, names, _ = PC.build(case)
        gin = M.pack(subs)
        arrs[case.name + "__node_id"] = gin.node["node_id"]
        arrs[case.name + "__slot_key"] = gin.slot["slot_key"]
        try:
            out = run_reference(case, subs, PC.params_of(case.name))
        except Exception as exc:   # the reference's own exception: recorded, not modelled
            arrs[case.name + "__raised"] = np.array(where_raised(exc))
            print("%-40s raised %s" % (case.name, arrs[case.name + "__raised"]))
            n_raise += 1
            continue
        gout = M.pack(out, like=gin)
        assert np.array_equal(gin.slot_ptr, gout.slot_ptr) and np.array_equal(gin.slot["slot_key"], gout.slot["slot_key"])
        for k, v in M.pick(gout, M.OUT_FIELDS).items():
            if k.startswith(("node__", "slot__")):
                arrs[case.name + "__" + k] = v
        n_out += 1
    path = os.path.join(HERE, "pass_cases.npz")
    np.savez_compressed(path, **arrs)
    print("wrote pass_cases.npz %.1f KB: %d cases with outputs, %d with a recorded exception" % (
        os.path.getsize(path) / 1024, n_out, n_raise))


if __name__ == "__main__":
    main()
