"""The typed-value boundary matrix of value_matrix_cases.py on the host
simulators: the general scanner (sim_scan), the fast scanner with and
without the column plan (sim_scan_fast under YBG_PLAN 1 and 0), the
columnar snapshot's query, grouped query and select simulators, row
emission (sim_emit) and the block-path GROUP BY (sim_group), each against
the CPU oracle. Every test asserts how many checks each path executed: a
path may only be missing where the fast scanner declares the spec
ineligible (code 9), and then the count says so."""
import pytest

import ybgpu as y
import value_matrix_cases as vm
from scan_tail_cases import env

ENV = dict(YBG_IVB=None, YBG_BB=None, YBG_GRID=None, YBG_FAST=None)


def _raw(t):
    return t["data"], t["offsets"], t["n_blocks"]


class SimRunner:
    """The simulators as the scenarios' execution paths."""

    def scan_paths(self, t, preds, aggs):
        spec = vm.make_spec(t, preds, aggs)
        out = [("general", y.sim_scan(spec, *_raw(t)))]
        for plan in (1, 0):
            with env(YBG_PLAN=plan, **ENV):
                if plan == 0 and not self.planned(t, preds, aggs):
                    continue  # no plan: the same pass as above
                try:
                    res, _nf = y.sim_scan_fast(spec, *_raw(t))
                except RuntimeError as e:
                    if "rc=9" not in str(e):
                        raise
                    continue  # not eligible for the fast scanner
            out.append(("fast_planned" if plan and y.sim_scan_planned(spec)
                        else "fast", res))
        out.append(("snapshot", y.sim_snapshot_query(
            vm.make_spec(t), *_raw(t), list(preds), list(aggs))))
        return out

    def planned(self, t, preds, aggs):
        with env(YBG_PLAN=None, **ENV):
            return y.sim_scan_planned(vm.make_spec(t, preds, aggs))

    def row_paths(self, t):
        spec = vm.make_spec(t)
        spec.emit_rows = 1
        rows = y.sim_emit(spec, *_raw(t), row_cap=1 << 10, varlen_cap=1 << 12)
        cols = vm.select_cols(t)
        (datums, null_masks, _ids), res = y.sim_snapshot_select(
            vm.make_spec(t), *_raw(t), [], cols, cap=1 << 10)
        return [("emit", [kd + vals for kd, vals in rows]),
                ("snapshot_select", y.decode_snapshot_rows(
                    res, datums, null_masks, len(cols), cols, 1 << 10))]

    def group_paths(self, t, aggs, gcol):
        blk = y.sim_group(vm.make_spec(t, (), aggs, gcol), *_raw(t),
                          cap=1 << 10, key_bytes_cap=1 << 10)
        snap, _raw_out, _res = y.sim_snapshot_group_query(
            vm.make_spec(t), *_raw(t), [], list(aggs), gcol, cap=1 << 10)
        return [("block", blk), ("snapshot", snap)]

    def null_group_paths(self, t, aggs):
        out = [("sim_group",) + y.sim_group(
            vm.make_spec(t, (), aggs, 0), *_raw(t), cap=1 << 10,
            key_bytes_cap=1 << 10, raw=True)]
        out.append(("orcl_group",) + vm.oracle_groups(t, aggs, 0, raw=True))
        return out


RUN = SimRunner()
CELLS = [(dt, pv) for dt in vm.DTYPES for pv in (1, 2)]
IDS = ["%s_v%d" % (vm.NAMES[dt], pv) for dt, pv in CELLS]


@pytest.mark.parametrize("dt,pv", CELLS, ids=IDS)
def test_compare_ops_equal_oracle(dt, pv):
    n = len(vm.compare_queries(dt, pv))
    n_pairs = 6 * (len(vm.BOUNDARY[dt]) + len(vm.OUTSIDE[dt]))
    assert n == 2 * n_pairs + 3
    counts = vm.scenario_compare(RUN, dt, pv)
    print(vm.NAMES[dt], pv, dict(counts))
    assert counts["general"] == n and counts["snapshot"] == n
    # packed V2 rows with two aggregates are the fast scanner's: every such
    # spec runs on it, and again without the plan where it has one
    fast = counts["fast"] + counts["fast_planned"]
    if pv == 2:
        assert fast == n_pairs + counts["fast_planned"], dict(counts)
    assert set(counts) <= {"general", "snapshot", "fast", "fast_planned"}


@pytest.mark.parametrize("dt", vm.DTYPES, ids=[vm.NAMES[d] for d in vm.DTYPES])
def test_fast_scanner_decodes_narrow_columns(dt):
    """On the V2 tablet the fast scanner keeps some batches to itself (so it
    did decode column 0) and hands the others to the general scanner."""
    t = vm.tablet(dt, 2)
    queries = vm.compare_queries(dt, 2)
    _label, preds, aggs = queries[1]  # two aggregates
    spec = vm.make_spec(t, preds, aggs)
    with env(YBG_PLAN=None, **ENV):
        _res, nf = y.sim_scan_fast(spec, *_raw(t))
        batches = y.sim_fast_census(spec, *_raw(t))["batches"]
    print(vm.NAMES[dt], "fallback", nf, "of", batches)
    assert 0 < nf < batches


@pytest.mark.parametrize("pv", (1, 2))
def test_key_predicates_equal_oracle(pv):
    n = len(vm.key_queries(vm.tablet(y.T_INT64, pv)))
    assert n == 6 * (6 + 7)
    counts = vm.scenario_keys(RUN, pv)
    print(pv, dict(counts))
    assert counts["general"] == n and counts["snapshot"] == n


ROW_KEYS = [("tablet", dt, pv) for dt, pv in CELLS] + \
    [("special", "double_nan"), ("special", "float_nan")]


@pytest.mark.parametrize("t_key", ROW_KEYS,
                         ids=IDS + ["double_nan", "float_nan"])
def test_rows_equal_oracle(t_key):
    counts = vm.scenario_rows(RUN, t_key)
    assert dict(counts) == {"emit": 1, "snapshot_select": 1}


@pytest.mark.parametrize("name", ("double_nan", "float_nan"))
def test_fp_special_predicates_equal_oracle(name):
    counts = vm.scenario_special_fp(RUN, name)
    print(name, dict(counts))
    assert counts["oracle"] == 36
    assert counts["general"] == 36 and counts["snapshot"] == 36
    # an FP predicate has no column plan: one fast pass per spec
    assert counts["fast"] == 36 and counts["fast_planned"] == 0


def test_double_aggregates_bit_equal():
    counts = vm.scenario_double_aggs(RUN)
    print(dict(counts))
    assert counts["general"] == 6 and counts["snapshot"] == 6
    # a double aggregate has no column plan: one fast pass per spec
    assert counts["fast"] == 6 and counts["fast_planned"] == 0
    assert counts["group:block"] == 3 and counts["group:snapshot"] == 3


@pytest.mark.parametrize("dt", (y.T_INT64, y.T_UINT64),
                         ids=("int64", "uint64"))
def test_planned_extremes(dt):
    counts = vm.scenario_planned_extremes(RUN, dt)
    print(dict(counts))
    assert counts["general"] == 8 and counts["snapshot"] == 8
    assert counts["fast_planned"] == 8 and counts["fast"] == 8


def test_sum_int64_wraps_on_every_path():
    counts = vm.scenario_sum_wrap(RUN)
    print(dict(counts))
    assert counts["general"] == 2 and counts["snapshot"] == 2
    assert counts["fast_planned"] == 2 and counts["fast"] == 2
    assert counts["group:block"] == 1 and counts["group:snapshot"] == 1


@pytest.mark.parametrize("name", tuple(vm.GROUP_TABLETS))
def test_null_group_apart_from_minus_one(name):
    counts = vm.scenario_null_group(RUN, name)
    assert dict(counts) == {"sim_group": 1, "orcl_group": 1}


def test_unsigned_v1_and_column_updates_in_oracle():
    """The oracle reads UINT32 / UINT64 packed V1 values and column updates
    (type bytes 'O' and 'U'): zero-extended, every bit kept."""
    for dt in (y.T_UINT32, y.T_UINT64):
        vals = vm.BOUNDARY[dt]
        rows = vm.oracle_rows(("tablet", dt, 1))
        assert len(rows) == vm.N
        for r, row in enumerate(rows):
            want = vals[r % len(vals)]
            if r < vm.N // 2 and r % 3 == 0:
                want = vals[(r + 1) % len(vals)]
            if r >= vm.N - vm.N // 4 and r % 3 == 0:
                want = None
            assert row[2] == want and row[3] == r, (dt, r, row)
