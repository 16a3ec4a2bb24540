"""ORDER BY / top-N on a columnar snapshot, on the GPU:
k_snap_order_hist / _fix / _mark / _gather / _emit and the device radix sort
against the CPU oracle's matching rows sorted in Python — the scenarios of
snapshot_order_cases.py that test_snapshot_order_sim.py runs on the simulator
— plus what only the device can show: byte-identical output across separately
built snapshots and equal to the simulator's, ordered selects interleaved
with select, query and group_query on one snapshot, error messages, memory
and timing accounting. All tests require an MI355X (gfx950)."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec
import snapshot_cases as sc
import snapshot_order_cases as so
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


def build_snapshot(case, read_micros, lower=None, upper=None, strings=False):
    gpu_scan = _gpu()
    s = gpu_scan.GpuScan(make_spec(case, read_micros, (), (), lower, upper))
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    snap = s.snapshot(strings=strings)
    s.close()
    return snap


class Runner:
    """`run` of the shared scenarios: one snapshot per (tablet, read time,
    bounds, strings), built on first use and kept for the following calls."""

    def __init__(self):
        self.snaps = {}

    def snapshot(self, case, read_micros, lower=None, upper=None,
                 strings=False):
        key = (case["name"], read_micros, bool(lower), bool(upper), strings)
        if key not in self.snaps:
            self.snaps[key] = build_snapshot(case, read_micros, lower, upper,
                                             strings)
        return self.snaps[key]

    def __call__(self, case, read_micros, preds, cols, order_by,
                 descending=False, nulls_first=False, limit=0, after=None,
                 row_lo=0, row_hi=None, cap=so.CAP, lower=None, upper=None,
                 strings=False, varlen_cap=so.VCAP, backward=False):
        snap = self.snapshot(case, read_micros, lower, upper, strings)
        datums, null_masks, row_ids, varlen, vsize, res = \
            snap.select_ordered_raw(list(preds), list(cols), order_by,
                                    descending, nulls_first, limit, after,
                                    row_lo, row_hi, cap, varlen_cap, backward)
        strs = y.select_string_cols(case["schema"], cols) if strings else None
        rows = y.decode_snapshot_rows(res.r, datums, null_masks, len(cols),
                                      cols, cap, varlen, strs)
        return rows, (datums, null_masks, row_ids, varlen, vsize), res

    def close(self):
        for snap in self.snaps.values():
            snap.close()
        self.snaps = {}


@pytest.fixture
def run(monkeypatch):
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    r = Runner()
    yield r
    r.close()


def test_order_vs_oracle_all_stageable_cases(run, cases):
    so.scenario_parity(run, cases)


@pytest.mark.parametrize("n", ss.edge_sizes())
def test_order_tablet(run, n):
    so.scenario_order_tablet(run, n)


def test_order_keeps_bit_patterns(run):
    so.scenario_bits_kept(run)


def test_order_empty(run):
    so.scenario_empty(run)
    snap = run.snapshot(so.order_tablet(65), sc.EDGE_READ_BEFORE)
    assert snap.kernel_ms() == 0   # nothing was launched


@pytest.mark.parametrize("n", sorted({1025, 2 * ss.tile_rows() + 1}))
def test_order_both_selection_paths(run, n, monkeypatch):
    """Full depth (YBG_SNAP_ORDER_CAND=1) and the default early-out deliver
    byte-identical output; scenario_order_tablet pins digit_passes."""
    early = so.scenario_order_tablet(run, n)
    monkeypatch.setenv("YBG_SNAP_ORDER_CAND", "1")
    deep = so.scenario_order_tablet(run, n, cand_one=True)
    assert early == deep


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("ob", [(0, 0), (0, 1)])
def test_order_paging(run, ob, desc):
    n = 2 * ss.tile_rows() + 1
    for page in so.page_sizes(n):
        # page 1 walks every cursor position: on the small tablet only
        m = 129 if page == 1 else n
        for nf in (False, True):
            so.scenario_paging(run, m, ob, desc, nf,
                               page if page <= m else m + 1)


def test_order_more_tiles_than_the_grid(run, monkeypatch):
    so.scenario_large(run)
    monkeypatch.setenv("YBG_SNAP_ORDER_CAND", "1")
    so.scenario_large(run, cand_one=True)


def test_order_string_projection(run):
    so.scenario_strings(run)


def test_order_errors(run, cases):
    so.scenario_errors(run, cases, message=True)


def _determinism_query():
    n = 2 * ss.tile_rows() + 1
    return so.order_tablet(n), so.ORDER_PRED, so.ORDER_COLS, n


def test_order_determinism_and_simulator(monkeypatch):
    """Two separately built snapshots, each queried twice under both
    early-out settings: byte-identical row_ids / null_masks / datums, equal
    to the simulator's."""
    case, preds, cols, n = _determinism_query()
    queries = [dict(order_by=(0, 1), descending=True, limit=100),
               dict(order_by=(0, 0), nulls_first=True, limit=0),
               dict(order_by=(0, 5), limit=300, after=(0, so.I64_MAX, 40))]
    seen = {i: [] for i in range(len(queries))}
    runners = [Runner(), Runner()]
    try:
        for cand in (None, "1"):
            if cand is None:
                monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
            else:
                monkeypatch.setenv("YBG_SNAP_ORDER_CAND", cand)
            for r in runners:
                for _ in range(2):
                    for i, kw in enumerate(queries):
                        _rows, raw, res = r(case, so.ORDER_READ, preds, cols,
                                            cap=n, **kw)
                        assert res.r.n_rows > 0
                        seen[i].append(so.raw_bytes(raw, res, len(cols), n))
    finally:
        for r in runners:
            r.close()
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    spec = make_spec(case, so.ORDER_READ, (), ())
    for i, kw in enumerate(queries):
        assert len(seen[i]) == 8
        assert all(s == seen[i][0] for s in seen[i][1:]), i
        kw = dict(kw)
        sraw, sres = y.sim_snapshot_select_ordered(
            spec, case["data"], case["offsets"], case["n_blocks"],
            list(preds), list(cols), kw.pop("order_by"), cap=n, **kw)
        assert so.raw_bytes(sraw, sres, len(cols), n) == seen[i][0], i


def test_order_interleaved_with_select_query_and_group_query(run):
    T = ss.tile_rows()
    case = ss.edge_tablet(2 * T + 1)
    cols = ss.all_cols(case["schema"])
    preds, aggs = sc.edge_query()
    in_preds = [ss.key_in([3, T - 1, T, 2 * T])]
    snap = run.snapshot(case, sc.EDGE_READ)

    def order(p, **kw):
        rows, raw, res = run(case, sc.EDGE_READ, p, cols, (0, 1), **kw)
        return (rows, list(raw[2][:res.r.n_rows]), res.r.rows_matched,
                y.order_cursor(res), res.digit_passes)

    def select(p, **kw):
        datums, null_masks, row_ids, res = snap.select_raw(
            list(p), cols, cap=ss.CAP, **kw)
        return (y.decode_snapshot_rows(res, datums, null_masks, len(cols),
                                       cols, ss.CAP),
                list(row_ids[:res.n_rows]), res.rows_matched, res.resume_row)

    def query(p):
        r = snap.query(list(p), list(aggs))
        return (r.rows_scanned, r.rows_matched,
                [(r.aggs[i].is_null, r.aggs[i].value_i64)
                 for i in range(len(aggs))])

    def group(p):
        keys, vals, cnts, res = snap.group_query_raw(list(p), list(aggs), 2)
        n = res.n_groups
        return ([bytes(memoryview(a).cast("B")[:n * 8 * w])
                 for a, w in ((keys, 1), (vals, y.MAX_AGGS),
                              (cnts, y.MAX_AGGS))], n, res.rows_matched)

    alone = (order(preds, descending=True, limit=50), select(preds),
             query(preds), group(preds),
             order(in_preds, nulls_first=True),
             select(in_preds, backward=True, limit=3), query(in_preds))
    # the reference for the stand-alone ordered results
    full = so.ordered(so.matching(case, sc.EDGE_READ, preds, cols, (0, 1)),
                      y.T_DOUBLE, True, False)
    assert alone[0][0] == [w[1] for w in full[:50]]
    for _ in range(2):
        assert order(in_preds, nulls_first=True) == alone[4]
        assert query(preds) == alone[2]
        assert order(preds, descending=True, limit=50) == alone[0]
        assert select(preds) == alone[1]
        assert group(preds) == alone[3]
        assert order(preds, descending=True, limit=50) == alone[0]
        assert select(in_preds, backward=True, limit=3) == alone[5]
        assert order(in_preds, nulls_first=True) == alone[4]
        assert query(in_preds) == alone[6]
        assert select(preds) == alone[1]


def test_order_memory_and_timing(run):
    T = ss.tile_rows()
    n = 2 * T + 1
    case = so.order_tablet(n)
    snap = run.snapshot(case, so.ORDER_READ)
    before = snap.info().device_bytes
    _rows, _raw, res = run(case, so.ORDER_READ, [], so.ORDER_COLS, (0, 1),
                           limit=10, cap=n)
    assert res.r.n_rows == 10 and res.digit_passes == 1
    assert snap.kernel_ms() > 0
    after = snap.info().device_bytes
    # selected bitmap, tile arrays, bins, state, candidates, sort scratch and
    # output buffers, counted from now on
    assert after > before
    run(case, so.ORDER_READ, [], so.ORDER_COLS, (0, 1), limit=10, cap=n)
    assert snap.info().device_bytes == after   # nothing regrown
    # no match: the count pass ran
    _rows, _raw, res = run(case, so.ORDER_READ, [ss.NO_ROW], so.ORDER_COLS,
                           (0, 1), limit=10)
    assert res.r.n_rows == 0 and snap.kernel_ms() > 0
    assert snap.info().device_bytes == after
