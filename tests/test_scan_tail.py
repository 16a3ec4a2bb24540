"""Scan tail on the host simulator: the per-batch state bytes, the planned
kernel's in-wave head resolution (head_action) and the fold by state must
leave ybg_sim_scan_fast bit-equal with ybg_sim_scan and the oracle, over
tablets whose batches abort never, rarely, in the middle of version chains
and always."""
import itertools

import pytest

import ybgpu as y
from scan_tail_cases import (TABLETS, env, oracle, res_tuple, sim_fast,
                             specs, tablet)


@pytest.mark.parametrize("expect_versions", [0, 1])
@pytest.mark.parametrize("plan", [1, 0])
@pytest.mark.parametrize("ivb", [1, 2, 3])
@pytest.mark.parametrize("name", TABLETS)
def test_sim_fast_equals_general_and_oracle(name, ivb, plan, expect_versions):
    _, built, _, aggs, _ = tablet(name)
    spec, _ = specs(name, expect_versions)
    with env(YBG_IVB=ivb, YBG_PLAN=plan):
        assert y.sim_scan_planned(spec) == bool(plan)
        got, nf = sim_fast(name, expect_versions)
        gen = res_tuple(y.sim_scan(spec, built[0], built[1], built[2]),
                        len(aggs))
    print(name, "ivb", ivb, "plan", plan, "fallback batches", nf)
    assert got == gen
    assert got == oracle(name)
    if ivb == 1:
        # the tablets' reason for being here: never / sometimes / always
        if name == "chains":
            assert nf == 0
        else:
            assert nf > 0


def test_all_abort_tablet_aborts_nearly_every_batch():
    """Nearly all one-interval batches abort (the few that hold no
    row-change entry do not), so the two-interval batches all do: their
    count is the batch count, at least half the one-interval count."""
    with env(YBG_IVB=1):
        n1 = sim_fast("all_abort", 1)[1]
    with env(YBG_IVB=2):
        n2 = sim_fast("all_abort", 1)[1]
    print("fallback batches: ivb 1", n1, "ivb 2", n2)
    assert n1 > 0 and 2 * n2 >= n1


def test_fallback_count_independent_of_plan():
    for name in TABLETS:
        with env(YBG_IVB=1, YBG_PLAN=1):
            a = sim_fast(name, 0)[1]
        with env(YBG_IVB=1, YBG_PLAN=0):
            b = sim_fast(name, 0)[1]
        assert a == b, name


def test_head_action_table():
    """Every input of the helper, against the rule written out: an aborted
    or inactive lane does nothing; a lane whose predecessor lane completed
    resolves its head locally (adds it unless the predecessor walked into
    it); everything else writes the record."""
    for lane, ok, p_ok, p_wn in itertools.product((0, 1, 63), (0, 1), (0, 1),
                                                  (0, 1)):
        if not ok:
            want = y.HEAD_NONE
        elif lane > 0 and p_ok:
            want = y.HEAD_NONE if p_wn else y.HEAD_FOLD
        else:
            want = y.HEAD_WRITE
        assert y.sim_head_action(lane, ok, p_ok, p_wn) == want, \
            (lane, ok, p_ok, p_wn)


@pytest.mark.parametrize("plan", [1, 0])
@pytest.mark.parametrize("ivb", [1, 2])
@pytest.mark.parametrize("name", TABLETS)
def test_sim_known_set_never_changes_result(name, ivb, plan):
    """A known abort set sends its batches straight to the general scanner.
    Exact, empty, everything or deliberately wrong: the result is the
    oracle's, and every batch that aborts still falls back."""
    _, built, _, aggs, _ = tablet(name)
    spec, _ = specs(name, 0)
    want = oracle(name)

    def run(known):
        r, ids = y.sim_scan_fast_known(spec, built[0], built[1], built[2],
                                       known)
        assert ids == sorted(set(ids))
        return res_tuple(r, len(aggs)), ids

    with env(YBG_IVB=ivb, YBG_PLAN=plan):
        got, aborts = run([])  # empty set: the plain fast scan
        assert got == want
        assert len(aborts) == sim_fast(name, 0)[1]
        n_b = max(aborts, default=0) + 200  # ids past the end are ignored
        for label, known in (("exact", aborts),
                             ("everything", list(range(n_b))),
                             ("wrong", list(range(0, n_b, 7)))):
            got, ids = run(known)
            assert got == want, label
            # the general scanner ran the listed batches and every abort
            assert set(aborts) <= set(ids), label
            if label == "exact":
                assert ids == aborts
            else:
                assert set(k for k in known if k <= max(ids)) <= set(ids)
