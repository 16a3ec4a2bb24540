"""CPU parity of the COLUMNAR SNAPSHOT: the host simulator
(ybg_sim_snapshot_query — block scan with predicates/aggregates stripped,
rows ordered by sort_key, the device snapshot's padded column layout, then
the snap_device.h row loop the gfx950 query kernel runs) against the CPU
oracle, on every shared parity run a snapshot can answer and on the
row-count edges of the two-rows-per-lane layout."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec, run_oracle, check_match
import snapshot_cases as sc


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def _sim(case, read_micros, preds, aggs, lower=None, upper=None):
    # the spec carries read time and bounds only: the build ignores its
    # predicates and aggregates
    spec = make_spec(case, read_micros, (), (), lower, upper)
    return y.sim_snapshot_query(spec, case["data"], case["offsets"],
                                case["n_blocks"], list(preds), list(aggs))


def test_sim_snapshot_vs_oracle_all_stageable_cases(cases):
    checked = 0
    skipped = set()
    for case, _ri, read_micros, preds, aggs, lower, upper in \
            sc.iter_runs(cases):
        if not y.stageable(case["schema"], preds, aggs):
            skipped.add(case["name"])
            continue
        sres = _sim(case, read_micros, preds, aggs, lower, upper)
        ores = run_oracle(case, read_micros, preds, aggs, lower, upper)
        try:
            check_match(sres, ores, aggs,
                        check_entries=lower is None and upper is None)
        except AssertionError as e:
            raise AssertionError(
                f"case {case['name']} read={read_micros}: {e}") from e
        checked += 1
    assert skipped == sc.NOT_STAGEABLE_CASES, skipped
    assert checked >= sc.N_STAGEABLE_RUNS, checked


def test_stageable_rejects_exactly_the_string_and_tuple_runs(cases):
    rejected = [case["name"]
                for case, _ri, _rm, preds, aggs, _lo, _hi in
                sc.iter_runs(cases)
                if not y.stageable(case["schema"], preds, aggs)]
    assert len(rejected) == sc.N_NOT_STAGEABLE_RUNS, rejected
    assert set(rejected) == sc.NOT_STAGEABLE_CASES
    # ... and the simulator's shared translation code agrees (rc 9)
    for case, _ri, read_micros, preds, aggs, lower, upper in \
            sc.iter_runs(cases):
        if y.stageable(case["schema"], preds, aggs):
            continue
        with pytest.raises(RuntimeError, match="rc=9"):
            _sim(case, read_micros, preds, aggs, lower, upper)


def test_stageable_rule_details():
    s = sc.EDGE_SCHEMA
    cnt = [y.Agg(y.AGG_COUNT_STAR, 0)]
    assert y.stageable(s, [], cnt)
    assert y.stageable(s, [y.Pred(1, 0, y.PRED_LT, 5, None, 0)], cnt)
    assert not y.stageable(s, [y.Pred(0, 3, y.PRED_LT, 5, None, 0)], cnt)
    assert not y.stageable(s, [y.Pred(1, 1, y.PRED_LT, 5, None, 0)], cnt)
    assert not y.stageable(s, [], [y.Agg(y.AGG_SUM_INT64, 3)])
    assert not y.stageable(s, [y.Pred(0, 0, y.PRED_GT, 0, None, 0)] * 9, cnt)
    assert not y.stageable(s, [], cnt * 9)
    # COUNT(*) ignores its column index
    assert y.stageable(s, [], [y.Agg(y.AGG_COUNT_STAR, 99)])


@pytest.mark.parametrize("n", sc.EDGE_SIZES)
def test_sim_snapshot_row_count_edges(n):
    case = sc.edge_tablet(n)
    preds, aggs = sc.edge_query()
    sres = _sim(case, sc.EDGE_READ, preds, aggs)
    ores = run_oracle(case, sc.EDGE_READ, preds, aggs)
    assert sres.rows_scanned == n
    check_match(sres, ores, aggs)
    # no-null-mask variant: the query never touches the NULL column
    preds2, aggs2 = sc.edge_query_no_null_col()
    check_match(_sim(case, sc.EDGE_READ, preds2, aggs2),
                run_oracle(case, sc.EDGE_READ, preds2, aggs2), aggs2)


@pytest.mark.parametrize("nulls", [False, True])
def test_sim_snapshot_kernel_shape_queries(nulls):
    """The queries test_snapshot_gpu.py uses to reach every kernel shape
    (2 / 5 predicates x 2 / 4 / 8 aggregates) against the oracle."""
    case = sc.edge_tablet(777, nulls=nulls)
    for n_preds, n_aggs in sc.KERNEL_SHAPES:
        preds, aggs = sc.shape_query(n_preds, n_aggs)
        check_match(_sim(case, sc.EDGE_READ, preds, aggs),
                    run_oracle(case, sc.EDGE_READ, preds, aggs), aggs)


def test_sim_snapshot_empty():
    case = sc.edge_tablet(65)
    preds, aggs = sc.edge_query()
    sres = _sim(case, sc.EDGE_READ_BEFORE, preds, aggs)
    assert sres.rows_scanned == 0 and sres.rows_matched == 0
    assert all(sres.aggs[i].is_null for i in range(len(aggs)))
    check_match(sres, run_oracle(case, sc.EDGE_READ_BEFORE, preds, aggs),
                aggs)
