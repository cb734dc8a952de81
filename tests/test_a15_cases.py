"""The directed a15 cases (a15_cases.py) on the CPU, before test_gpu_a15_cases.py holds the HIP
kernels to them.

  * every case reaches the branch it claims (its predicate on the oracle's output);
  * the oracle's four columns equal the record of the reference's own mahalanobis_distance
    (tests/golden/a15_cases.npz) at rtol 1e-12, non-finite entries equal in kind;
  * where the reference raised (C_i + C_j exactly singular, :37) the oracle raises the same type at
    the same pair and at no other; an orphan key raises the oracle's KeyError (:182-183);
  * a15_cases.expected is gtf_oracle.updated_state_pairs wherever that does not raise: the visit
    rule, the pair order and the truth flag have one statement;
  * every value compared as a finite number moves by less than 1e-9 relative when the coordinates
    are perturbed by +-2^-46 relative, each coordinate of each node on its own; only the coordinate
    that sits on a comparison is kept (an |x| of 600 or one ulp below is frozen, coordinates that
    must stay equal move by one common factor). No case and no node is exempt;
  * the schedule of everything(): more than one block of 2-lane and of 4-lane groups, both paths.

oracle/cpu_ref.cpp does not implement a15, so there is nothing of it to hold to the record.
"""
import os

import numpy as np
import pytest

import a15_cases as AC
import gtf_oracle as O
from fixtures import GOLDEN
from test_tse_cases import close

NAMES = [c.name for c in AC.CASES]


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(GOLDEN, "a15_cases.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch(name):
    case = AC.BY_NAME[name]
    info = AC.info_of(case)
    case.check(info)
    assert len(info["singular"]) == case.singular and bool(info["raised"]) == bool(case.err)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference_record(record, name):
    case = AC.BY_NAME[name]
    info = AC.info_of(case)
    if case.err:
        assert name + "__chi2" not in record.files
        with pytest.raises(O.ReferenceError_, match="KeyError.*182-183"):
            O.updated_state_pairs(info["g"], info["truth"])
        return
    assert np.array_equal(record[name + "__pair_ptr"], info["ptr"])
    for c in AC.COLS:
        close(info["cols"][c], record[name + "__" + c], 1e-12, (name, c))
    raised = record[name + "__raised_pairs"].tolist() if name + "__raised_pairs" in record.files else []
    assert raised == info["singular"]
    if raised:
        typ, where = str(record[name + "__raised"]).split()
        assert typ == "LinAlgError" and where == "calculate_distance_between_updated_track_states.py:37"
        with pytest.raises(np.linalg.LinAlgError):
            O.updated_state_pairs(info["g"], info["truth"])
        with pytest.raises(np.linalg.LinAlgError):
            AC.pair_of(info["g"], 0, raised[0])
    else:
        ptr, cols = O.updated_state_pairs(info["g"], info["truth"])
        assert np.array_equal(ptr, info["ptr"])
        for c in AC.COLS + ("truth",):
            assert np.array_equal(cols[c], info["cols"][c], equal_nan=True), c


def test_cases_are_well_conditioned():
    g, comps, truth = AC.everything()
    ptr, cols, sing, _ = AC.expected(g, truth)
    assert sum(1 for c in comps if c["case"].hold) >= 18
    for seed in range(3):
        p2, c2, s2, _ = AC.expected(AC.perturbed(g, comps, seed), truth)
        assert np.array_equal(p2, ptr) and s2 == sing
        for c in AC.COLS:
            close(c2[c], cols[c], 1e-9, (c, seed))


def test_big_star_sample_is_well_conditioned():
    g = AC.big_star(AC.BIG_CAP)
    P = AC.BIG_CAP * (AC.BIG_CAP - 1) // 2
    ts = [0, P - 1] + np.random.default_rng(2048).integers(0, P, 200).tolist()
    h = AC.perturbed(g, [], 1)
    for t in ts:
        close(np.array(AC.pair_of(h, 0, t)), np.array(AC.pair_of(g, 0, t)), 1e-9, t)


def test_schedule_of_everything():
    g, comps, _ = AC.everything()
    deg = np.diff(g.slot_ptr)
    assert int((deg <= 2).sum()) > 128 and int(((deg >= 3) & (deg <= 4)).sum()) > 64   # more than a block of each
    for edge in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 70, 130):
        assert (deg == edge).any(), edge
    ge, _, _ = AC.everything(True)
    de = np.diff(ge.slot_ptr)
    assert (de == 4).any() and (de == 66).any()      # an error of each kind in a group and in the wave path
