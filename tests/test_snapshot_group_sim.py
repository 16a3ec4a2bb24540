"""CPU parity of GROUP BY on a columnar snapshot: the host simulator
(ybg_sim_snapshot_group_query — the snapshot layout, then the snap_device.h
accumulate / flush / export code the gfx950 kernels run, one simulated
workgroup at a time) against the CPU oracle. Both levels (workgroup-local
table + flush, global table only) are forced through expect_groups; the
scenarios live in snapshot_group_cases.py and run again on the kernels in
test_snapshot_group_gpu.py."""
import pytest

import ybgpu as y
from parity_cases import make_spec
import snapshot_cases as sc
import snapshot_group_cases as gc


def run(case, read_micros, preds, aggs, group_col, group_is_key=False,
        expect_groups=0, cap=gc.CAP):
    # the spec carries the read time only: the build ignores the rest
    spec = make_spec(case, read_micros, (), ())
    return y.sim_snapshot_group_query(
        spec, case["data"], case["offsets"], case["n_blocks"], list(preds),
        list(aggs), group_col, group_is_key, expect_groups, cap)


def test_local_slots_follow_the_aggregate_cap():
    L2, L4, L8 = (gc.local_slots(n) for n in (2, 4, 8))
    assert gc.local_slots(1) == L2 and gc.local_slots(3) == L4
    assert gc.local_slots(5) == L8
    # powers of two, shrinking as the slot widens
    assert all(v > 0 and v & (v - 1) == 0 for v in (L2, L4, L8))
    assert L2 >= L4 >= L8


@pytest.mark.parametrize("n", sc.EDGE_SIZES)
def test_sim_group_row_count_edges(n):
    gc.scenario_row_count_edge(run, n)


def test_sim_group_empty():
    gc.scenario_empty(run)


@pytest.mark.parametrize("num_aggs", [2, 8])
@pytest.mark.parametrize("label", gc.CARD_LABELS)
def test_sim_group_cardinality_edges(label, num_aggs):
    gc.scenario_cardinality(run, label, num_aggs)


def test_sim_group_grid_stride():
    """524,801 rows: about a second in the simulator, so it runs here too."""
    gc.scenario_grid_stride(run)


def test_sim_group_on_key_column():
    gc.scenario_group_on_key_column(run)


def test_sim_group_column_kinds():
    gc.scenario_group_column_kinds(run)


def test_sim_group_null_group_next_to_minus_one():
    gc.scenario_null_group_next_to_minus_one(run)


def test_sim_group_nullable_specialisation():
    gc.scenario_nullable_specialisation(run)


def test_sim_group_in_and_in_range():
    gc.scenario_in_and_in_range(run)


def test_sim_group_doubles():
    gc.scenario_doubles(run)


def test_sim_group_poison():
    gc.scenario_poison(run)


def test_sim_group_determinism():
    """Every simulator call builds its own snapshot."""
    gc.scenario_determinism(lambda: run)


def test_sim_group_errors():
    """The simulator shares the translation code: the same codes (it
    reports no message text)."""
    gc.scenario_errors(run)
