"""SELECT on a columnar snapshot, on the GPU: k_snap_select_count / _scan /
_gather against the CPU oracle's matching rows in key order — the scenarios
of snapshot_select_cases.py that test_snapshot_select_sim.py runs on the
simulator — plus what only the device can show: byte-identical output across
separately built snapshots and equal to the simulator's, select interleaved
with query and group_query on one snapshot, error messages, memory and
timing accounting. All tests require an MI355X (gfx950)."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec
import snapshot_cases as sc
import snapshot_select_cases as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def _gpu():
    import gpu_scan
    if not gpu_scan.gpu_available():
        pytest.fail("no HIP device visible — gpu-marked test must run on GPU")
    return gpu_scan


def build_snapshot(case, read_micros, lower=None, upper=None):
    gpu_scan = _gpu()
    s = gpu_scan.GpuScan(make_spec(case, read_micros, (), (), lower, upper))
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    snap = s.snapshot()
    s.close()
    return snap


class Runner:
    """`run` of the shared scenarios: one snapshot per (tablet, read time,
    bounds), built on first use and kept for the following selects."""

    def __init__(self):
        self.snaps = {}

    def snapshot(self, case, read_micros, lower=None, upper=None):
        key = (case["name"], read_micros, bool(lower), bool(upper))
        if key not in self.snaps:
            self.snaps[key] = build_snapshot(case, read_micros, lower, upper)
        return self.snaps[key]

    def __call__(self, case, read_micros, preds, cols, limit=0,
                 backward=False, row_lo=0, row_hi=None, cap=ss.CAP,
                 lower=None, upper=None):
        snap = self.snapshot(case, read_micros, lower, upper)
        datums, null_masks, row_ids, res = snap.select_raw(
            list(preds), list(cols), limit, backward, row_lo, row_hi, cap)
        rows = y.decode_snapshot_rows(res, datums, null_masks, len(cols),
                                      cols, cap)
        return rows, (datums, null_masks, row_ids), res

    def close(self):
        for snap in self.snaps.values():
            snap.close()
        self.snaps = {}


@pytest.fixture
def run():
    r = Runner()
    yield r
    r.close()


def test_select_vs_oracle_all_stageable_cases(run, cases):
    ss.scenario_parity(run, cases)


@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("n", ss.edge_sizes())
def test_select_row_count_and_tile_edges(run, n, nulls):
    ss.scenario_edge(run, n, nulls)


def test_select_many_tiles(run):
    """More tiles than workgroups and than one scan round (2.1M rows)."""
    ss.scenario_large(run)


def test_select_empty(run):
    ss.scenario_empty(run)
    snap = run.snapshot(ss.edge_tablet(65), sc.EDGE_READ_BEFORE)
    assert snap.kernel_ms() == 0   # nothing was launched
    snap = run.snapshot(ss.edge_tablet(65), sc.EDGE_READ)
    assert snap.kernel_ms() == 0   # the last select had an empty window


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("limit", ss.page_limits())
def test_select_paging(run, limit, backward):
    ss.scenario_paging(run, limit, backward)


def test_select_windows(run):
    ss.scenario_windows(run)


def test_select_backward_limit(run):
    ss.scenario_backward_limit(run)


def test_select_projection(run, cases):
    ss.scenario_projection(run, cases)


def test_select_determinism_and_simulator(cases):
    """Two separately built snapshots, each selected twice: byte-identical
    row_ids / null_masks / datums, equal to the simulator's."""
    runners = []

    def fresh():
        runners.append(Runner())
        return runners[-1]

    try:
        raw, (case, read_micros, preds, cols, cap) = \
            ss.scenario_determinism(fresh, cases)
        assert len(runners) == 2
    finally:
        for r in runners:
            r.close()
    spec = make_spec(case, read_micros, (), ())
    sraw, sres = y.sim_snapshot_select(
        spec, case["data"], case["offsets"], case["n_blocks"], preds, cols,
        cap=cap)
    assert ss.raw_bytes(sraw, sres, len(cols), cap) == raw


def test_select_interleaved_with_query_and_group_query(run):
    def run_query(case, read_micros, preds, aggs):
        r = run.snapshot(case, read_micros).query(list(preds), list(aggs))
        return (r.rows_scanned, r.rows_matched,
                [(r.aggs[i].is_null, r.aggs[i].value_i64)
                 for i in range(len(aggs))])

    def run_group(case, read_micros, preds, aggs, group_col):
        keys, vals, cnts, res = run.snapshot(case, read_micros) \
            .group_query_raw(list(preds), list(aggs), group_col)
        n = res.n_groups
        return ([bytes(memoryview(a).cast("B")[:n * 8 * w])
                 for a, w in ((keys, 1), (vals, y.MAX_AGGS),
                              (cnts, y.MAX_AGGS))], n, res.rows_matched)

    ss.scenario_interleave(run, run_query, run_group)


def test_select_errors(run, cases):
    ss.scenario_errors(run, cases, message=True)


def test_select_memory_and_timing(run):
    T = ss.tile_rows()
    case = ss.edge_tablet(2 * T + 1)
    snap = run.snapshot(case, sc.EDGE_READ)
    cols = ss.all_cols(case["schema"])
    before = snap.info().device_bytes
    _rows, _raw, res = run(case, sc.EDGE_READ, [], cols)
    assert res.n_rows == 2 * T + 1
    assert snap.kernel_ms() > 0        # count + scan + gather
    after = snap.info().device_bytes
    # bitmap + tile arrays + header + output buffers, counted from now on
    assert after > before
    run(case, sc.EDGE_READ, [], cols)
    assert snap.info().device_bytes == after   # nothing regrown
    # no match: count + scan ran, the gather did not
    _rows, _raw, res = run(case, sc.EDGE_READ, [ss.NO_ROW], cols)
    assert res.n_rows == 0 and snap.kernel_ms() > 0
