"""GROUP BY on a columnar snapshot, on the GPU: k_snap_group_query at both
levels (workgroup-local LDS table + flush, global table only), the group
table init and the compact / sort / export kernels, against the CPU oracle —
the scenarios of snapshot_group_cases.py that test_snapshot_group_sim.py
runs on the simulator — plus what only the device can show: byte-identical
output across separately built snapshots and equal to the simulator's, the
block path's GROUP BY on the same tablet, error messages, and the plain
query undisturbed. All tests require an MI355X (gfx950)."""
import pytest

import ybgpu as y
from parity_cases import make_spec
import snapshot_cases as sc
import snapshot_group_cases as gc

pytestmark = pytest.mark.gpu


def _gpu():
    import gpu_scan
    if not gpu_scan.gpu_available():
        pytest.fail("no HIP device visible — gpu-marked test must run on GPU")
    return gpu_scan


def build_snapshot(case, read_micros):
    gpu_scan = _gpu()
    s = gpu_scan.GpuScan(make_spec(case, read_micros, (), ()))
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    snap = s.snapshot()
    s.close()
    return snap


class Runner:
    """`run` of the shared scenarios: one snapshot per (tablet, read time),
    built on first use and kept for the following queries."""

    def __init__(self):
        self.snaps = {}

    def snapshot(self, case, read_micros):
        key = (case["name"], read_micros)
        if key not in self.snaps:
            self.snaps[key] = build_snapshot(case, read_micros)
        return self.snaps[key]

    def __call__(self, case, read_micros, preds, aggs, group_col,
                 group_is_key=False, expect_groups=0, cap=gc.CAP):
        snap = self.snapshot(case, read_micros)
        keys, vals, cnts, res = snap.group_query_raw(
            list(preds), list(aggs), group_col, group_is_key, expect_groups,
            cap)
        groups = y.decode_snapshot_groups(res, keys, vals, cnts, list(aggs))
        return groups, (keys, vals, cnts), res

    def close(self):
        for snap in self.snaps.values():
            snap.close()
        self.snaps = {}


@pytest.fixture
def run():
    r = Runner()
    yield r
    r.close()


def sim_run(case, read_micros, preds, aggs, group_col, group_is_key=False,
            expect_groups=0, cap=gc.CAP):
    spec = make_spec(case, read_micros, (), ())
    return y.sim_snapshot_group_query(
        spec, case["data"], case["offsets"], case["n_blocks"], list(preds),
        list(aggs), group_col, group_is_key, expect_groups, cap)


@pytest.mark.parametrize("n", sc.EDGE_SIZES)
def test_group_row_count_edges(run, n):
    gc.scenario_row_count_edge(run, n)


def test_group_empty(run):
    gc.scenario_empty(run)
    snap = run.snapshot(gc.edge_tablet(65), sc.EDGE_READ_BEFORE)
    assert snap.kernel_ms() == 0   # nothing was launched


@pytest.mark.parametrize("num_aggs", [2, 8])
@pytest.mark.parametrize("label", gc.CARD_LABELS)
def test_group_cardinality_edges(run, label, num_aggs):
    gc.scenario_cardinality(run, label, num_aggs)


def test_group_grid_stride(run):
    gc.scenario_grid_stride(run)


def test_group_on_key_column(run):
    gc.scenario_group_on_key_column(run)


def test_group_column_kinds(run):
    gc.scenario_group_column_kinds(run)


def test_group_null_group_next_to_minus_one(run):
    gc.scenario_null_group_next_to_minus_one(run)


def test_group_nullable_specialisation(run):
    gc.scenario_nullable_specialisation(run)
    assert run.snapshot(gc.edge_tablet(777, nulls=False),
                        sc.EDGE_READ).info().nullable_cols == 0
    assert run.snapshot(gc.edge_tablet(777, nulls=True),
                        sc.EDGE_READ).info().nullable_cols == 0b010


def test_group_in_and_in_range(run):
    gc.scenario_in_and_in_range(run)


def test_group_doubles(run):
    gc.scenario_doubles(run)


def test_group_poison(run):
    gc.scenario_poison(run)


def test_group_determinism_and_block_path():
    """Two separately built snapshots, three queries each at both levels:
    byte-identical keys / vals / cnts, equal to the simulator's; the decoded
    groups equal the block path's GROUP BY (GpuScan.group_aggregate) bit for
    bit — double SUM included, both being exact fixed-point sums. The block
    path's order is unspecified: compared as a dict."""
    gpu_scan = _gpu()
    runners = []

    def fresh():
        runners.append(Runner())
        return runners[-1]

    try:
        raw, (case, preds, aggs) = gc.scenario_determinism(fresh)
        assert len(runners) == 2
        _sg, sraw, sres = sim_run(case, gc.READ, preds, aggs, 0)
        assert gc.raw_bytes(*sraw, sres) == raw
        got, _raw, _res = runners[0](case, gc.READ, preds, aggs, 0)
    finally:
        for r in runners:
            r.close()
    s = gpu_scan.GpuScan(gc.block_spec(case, gc.READ, preds, aggs, 0))
    try:
        s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                           case["total"])
        blk = s.group_aggregate(cap=gc.CAP, key_bytes_cap=1 << 12)
    finally:
        s.close()
    assert len(blk) == 97
    assert gc.same_bits(got, blk)


def test_group_errors_and_plain_query_undisturbed(run):
    gc.scenario_errors(run, message=True)
    # the snapshot answers plain query() identically before and after
    # grouped queries (they share the stream, the option-list buffer and
    # the timing events)
    case = gc.kinds_tablet()
    snap = run.snapshot(case, gc.READ)
    preds, aggs = gc.gen_preds(), gc.kinds_aggs()

    def plain():
        r = snap.query(preds, aggs)
        return (r.rows_scanned, r.rows_matched, r.entries_seen,
                [(r.aggs[i].is_null, r.aggs[i].value_i64)
                 for i in range(len(aggs))])

    before = plain()
    bytes_before = snap.info().device_bytes
    run(case, gc.READ, preds, aggs, 1)
    run(case, gc.READ, [], aggs, 0, expect_groups=10_000)
    assert plain() == before
    assert snap.kernel_ms() > 0
    # the group table and export scratch are counted from the first
    # grouped query on
    assert snap.info().device_bytes > bytes_before
    run(case, gc.READ, [], aggs, 0)
    assert snap.kernel_ms() > 0   # init + query + export of the grouped query
