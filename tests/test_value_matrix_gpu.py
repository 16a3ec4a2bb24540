"""The typed-value boundary matrix of value_matrix_cases.py on the GPU: the
three dispatch modes of test_wide_loads_gpu.py (default, YBG_PLAN=0,
YBG_FAST=0), GpuSnapshot.query / group_query / select, batch_rows and
group_aggregate, each against the CPU oracle, bit for bit. On packed V2
tablets the default mode must report the simulator's fallback count, below
the batch count: the fast kernel did decode the narrow columns. One snapshot
per tablet; a spec the fast kernel cannot take (more than two aggregates,
IN / IN_RANGE, key predicates) runs the default mode only, the other two
would launch the same general kernel."""
import pytest

import ybgpu as y
import value_matrix_cases as vm
from scan_tail_cases import env

pytestmark = pytest.mark.gpu

BASE = dict(YBG_IVB=None, YBG_BB=None, YBG_GRID=None)
MODES = (("default", {"YBG_PLAN": None, "YBG_FAST": None}),
         ("interpreted", {"YBG_PLAN": 0, "YBG_FAST": None}),
         ("general", {"YBG_PLAN": None, "YBG_FAST": 0}))
CAP = 1 << 10


def _raw(t):
    return t["data"], t["offsets"], t["n_blocks"]


def _fast_shape(preds, aggs):
    return len(aggs) <= 2 and all(
        not p.is_key_col and p.op <= y.PRED_NE for p in preds)


class GpuRunner:
    """The GPU as the scenarios' execution paths."""

    def __init__(self):
        import gpu_scan
        if not gpu_scan.gpu_available():
            pytest.fail("no HIP device visible — gpu-marked test must run "
                        "on GPU")
        self.gpu_scan = gpu_scan
        self.snaps = {}
        self.fast_batches = 0  # batches the fast kernel kept, over all runs

    def _scan(self, t, spec):
        s = self.gpu_scan.GpuScan(spec)
        s.feed_blocks_host(*_raw(t), t["total"])
        return s

    def snapshot(self, t):
        if t["name"] not in self.snaps:
            s = self._scan(t, vm.make_spec(t))
            try:
                self.snaps[t["name"]] = s.snapshot()
            finally:
                s.close()
        return self.snaps[t["name"]]

    def scan_paths(self, t, preds, aggs):
        spec = vm.make_spec(t, preds, aggs)
        fast_shape = _fast_shape(preds, aggs)
        out = []
        for mode, menv in (MODES if fast_shape else MODES[:1]):
            with env(**BASE, **menv):
                s = self._scan(t, spec)
                try:
                    s.execute()
                    res, retries = s.aggregates(), s.retry_batches()
                finally:
                    s.close()
                if not fast_shape or mode == "general":
                    assert retries == 0, (t["name"], mode, retries)
                else:
                    _r, nf = y.sim_scan_fast(spec, *_raw(t))
                    assert retries == nf, (t["name"], mode, retries, nf)
                    if t["pv"] == 2 and mode == "default":
                        n_b = y.sim_fast_census(spec, *_raw(t))["batches"]
                        assert retries < n_b, (t["name"], retries, n_b)
                        self.fast_batches += n_b - retries
            out.append((mode, res))
        out.append(("snapshot", self.snapshot(t).query(list(preds),
                                                       list(aggs))))
        return out

    def planned(self, t, preds, aggs):
        with env(**BASE, YBG_PLAN=None, YBG_FAST=None):
            s = self._scan(t, vm.make_spec(t, preds, aggs))
            try:
                s.execute()
                s.aggregates()
                return s.planned()
            finally:
                s.close()

    def row_paths(self, t):
        spec = vm.make_spec(t)
        spec.emit_rows = 1
        s = self._scan(t, spec)
        try:
            rows = s.batch_rows()
        finally:
            s.close()
        sel, _res = self.snapshot(t).select([], vm.select_cols(t), cap=CAP)
        return [("batch_rows", [kd + vals for kd, vals in rows]),
                ("snapshot_select", sel)]

    def group_paths(self, t, aggs, gcol):
        s = self._scan(t, vm.make_spec(t, (), aggs, gcol))
        try:
            blk = s.group_aggregate(cap=CAP, key_bytes_cap=CAP)
        finally:
            s.close()
        snap = self.snapshot(t).group_query([], list(aggs), gcol, cap=CAP)
        return [("block", blk), ("snapshot", snap)]

    def null_group_paths(self, t, aggs):
        spec = vm.make_spec(t, (), aggs, 0)
        s = self._scan(t, spec)
        out = []
        try:
            for run in ("first", "again"):  # the counters are reset per call
                keys, vals, cnts, kb, n = s.group_aggregate_raw(
                    cap=CAP, key_bytes_cap=CAP)
                ni = s.group_null_index()
                groups = y._decode_groups(spec.schema, 0, n, keys, vals,
                                          cnts, kb, len(aggs), spec.aggs, ni)
                out.append(("group_aggregate_" + run, groups, list(keys[:n]),
                            n, ni))
            assert s.group_aggregate(cap=CAP, key_bytes_cap=CAP) == groups
        finally:
            s.close()
        return out

    def close(self):
        for snap in self.snaps.values():
            snap.close()
        self.snaps = {}


@pytest.fixture
def run():
    r = GpuRunner()
    yield r
    r.close()


CELLS = [(dt, pv) for dt in vm.DTYPES for pv in (1, 2)]
IDS = ["%s_v%d" % (vm.NAMES[dt], pv) for dt, pv in CELLS]


@pytest.mark.parametrize("dt,pv", CELLS, ids=IDS)
def test_compare_ops_equal_oracle(run, dt, pv):
    n = len(vm.compare_queries(dt, pv))
    n_pairs = 6 * (len(vm.BOUNDARY[dt]) + len(vm.OUTSIDE[dt]))
    counts = vm.scenario_compare(run, dt, pv)
    print(vm.NAMES[dt], pv, dict(counts), "fast batches", run.fast_batches)
    assert counts["default"] == n and counts["snapshot"] == n
    assert counts["interpreted"] == n_pairs and counts["general"] == n_pairs
    if pv == 2:
        assert run.fast_batches >= n_pairs


@pytest.mark.parametrize("pv", (1, 2))
def test_key_predicates_equal_oracle(run, pv):
    counts = vm.scenario_keys(run, pv)
    assert counts["default"] == 78 and counts["snapshot"] == 78


ROW_KEYS = [("tablet", dt, pv) for dt, pv in CELLS] + \
    [("special", "double_nan"), ("special", "float_nan")]


@pytest.mark.parametrize("t_key", ROW_KEYS,
                         ids=IDS + ["double_nan", "float_nan"])
def test_rows_equal_oracle(run, t_key):
    counts = vm.scenario_rows(run, t_key)
    assert dict(counts) == {"batch_rows": 1, "snapshot_select": 1}


@pytest.mark.parametrize("name", ("double_nan", "float_nan"))
def test_fp_special_predicates_equal_oracle(run, name):
    counts = vm.scenario_special_fp(run, name)
    assert all(counts[p] == 36 for p in
               ("oracle", "default", "interpreted", "general",
                "snapshot")), counts
    assert run.fast_batches >= 36


def test_double_aggregates_bit_equal(run):
    counts = vm.scenario_double_aggs(run)
    assert all(counts[p] == 6 for p in
               ("default", "interpreted", "general", "snapshot")), counts
    assert counts["group:block"] == 3 and counts["group:snapshot"] == 3


@pytest.mark.parametrize("dt", (y.T_INT64, y.T_UINT64),
                         ids=("int64", "uint64"))
def test_planned_extremes(run, dt):
    counts = vm.scenario_planned_extremes(run, dt)
    assert all(counts[p] == 8 for p in
               ("default", "interpreted", "general", "snapshot")), counts
    assert run.fast_batches >= 8


def test_sum_int64_wraps_on_every_path(run):
    counts = vm.scenario_sum_wrap(run)
    assert all(counts[p] == 2 for p in
               ("default", "interpreted", "general", "snapshot")), counts
    assert counts["group:block"] == 1 and counts["group:snapshot"] == 1


@pytest.mark.parametrize("name", tuple(vm.GROUP_TABLETS))
def test_null_group_apart_from_minus_one(run, name):
    counts = vm.scenario_null_group(run, name)
    assert dict(counts) == {"group_aggregate_first": 1,
                            "group_aggregate_again": 1}


def test_null_index_needs_a_group_aggregate(run):
    t = vm.group_tablet("minus1_no_null")
    s = run._scan(t, vm.make_spec(t, (), [y.Agg(y.AGG_COUNT_STAR, 0)], 0))
    try:
        with pytest.raises(run.gpu_scan.GpuScanError):
            s.group_null_index()
    finally:
        s.close()
