"""CPU parity of SELECT on a columnar snapshot: the host simulator
(ybg_sim_snapshot_select — the snapshot layout, then the snap_device.h
predicate fold, bit packing, rank, output index and emit code the gfx950
kernels run, one simulated tile at a time) against the CPU oracle's matching
rows in key order. The scenarios live in snapshot_select_cases.py and run
again on the kernels in test_snapshot_select_gpu.py."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec, run_oracle
import snapshot_select_cases as ss


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def run(case, read_micros, preds, cols, limit=0, backward=False, row_lo=0,
        row_hi=None, cap=ss.CAP, lower=None, upper=None):
    # the spec carries read time and bounds only: the build ignores the rest
    spec = make_spec(case, read_micros, (), (), lower, upper)
    raw, res = y.sim_snapshot_select(
        spec, case["data"], case["offsets"], case["n_blocks"], list(preds),
        list(cols), limit, backward, row_lo, row_hi, cap)
    rows = y.decode_snapshot_rows(res, raw[0], raw[1], len(cols), cols, cap)
    return rows, raw, res


def test_tile_rows():
    T = ss.tile_rows()
    assert T >= 128 and T % 128 == 0   # whole waves of row pairs


def test_sim_select_vs_oracle_all_stageable_cases(cases):
    ss.scenario_parity(run, cases)


@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("n", ss.edge_sizes())
def test_sim_select_row_count_and_tile_edges(n, nulls):
    ss.scenario_edge(run, n, nulls)


def test_sim_select_many_tiles():
    """More tiles than workgroups and than one scan round (2.1M rows)."""
    ss.scenario_large(run)


def test_sim_select_empty():
    ss.scenario_empty(run)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("limit", ss.page_limits())
def test_sim_select_paging(limit, backward):
    ss.scenario_paging(run, limit, backward)


def test_sim_select_windows():
    ss.scenario_windows(run)


def test_sim_select_backward_limit():
    ss.scenario_backward_limit(run)


def test_sim_select_projection(cases):
    ss.scenario_projection(run, cases)


def test_sim_select_determinism(cases):
    """Every simulator call builds its own snapshot."""
    ss.scenario_determinism(lambda: run, cases)


def test_sim_select_interleaving():
    """The simulator holds no state between calls; the scenario still pins
    the three entry points against each other's stand-alone results."""
    def run_query(case, read_micros, preds, aggs):
        spec = make_spec(case, read_micros, (), ())
        r = y.sim_snapshot_query(spec, case["data"], case["offsets"],
                                 case["n_blocks"], list(preds), list(aggs))
        o = run_oracle(case, read_micros, preds, aggs)
        assert r.rows_matched == o.rows_matched
        return (r.rows_scanned, r.rows_matched,
                [(r.aggs[i].is_null, r.aggs[i].value_i64)
                 for i in range(len(aggs))])

    def run_group(case, read_micros, preds, aggs, group_col):
        spec = make_spec(case, read_micros, (), ())
        _g, raw, res = y.sim_snapshot_group_query(
            spec, case["data"], case["offsets"], case["n_blocks"],
            list(preds), list(aggs), group_col)
        return [bytes(memoryview(a).cast("B")[:res.n_groups * 8])
                for a in raw[:1]], res.n_groups, res.rows_matched

    ss.scenario_interleave(run, run_query, run_group)


def test_sim_select_errors(cases):
    """The simulator shares the translation code: the same codes (it
    reports no message text)."""
    ss.scenario_errors(run, cases)
