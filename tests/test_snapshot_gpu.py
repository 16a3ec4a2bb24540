"""Columnar snapshot on the GPU: the snapshot build (block scan -> sort ->
per-column arrays) and the dense query kernel against the CPU oracle, the
row-count edges of the two-rows-per-lane layout, the no-null-mask kernel
variant, determinism across separately built snapshots, the code-9 error
rule, the YBG_STAGE=1 transparent mode and info(). All tests require an
MI355X (gfx950)."""
import struct

import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec, run_oracle, check_match
import snapshot_cases as sc

pytestmark = pytest.mark.gpu


def _gpu():
    import gpu_scan
    if not gpu_scan.gpu_available():
        pytest.fail("no HIP device visible — gpu-marked test must run on GPU")
    return gpu_scan


@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def oracle_results(cases):
    """Oracle result of every shared run, computed once for the module."""
    return {(case["name"], ri): run_oracle(case, rm, preds, aggs, lo, hi)
            for case, ri, rm, preds, aggs, lo, hi in sc.iter_runs(cases)}


def build_snapshot(case, read_micros, lower=None, upper=None):
    """Feed the case's tablet, build a snapshot, and close the scan handle
    BEFORE returning: the snapshot must own its memory."""
    gpu_scan = _gpu()
    spec = make_spec(case, read_micros, (), (), lower, upper)
    s = gpu_scan.GpuScan(spec)
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    snap = s.snapshot()
    s.close()
    return snap


def _bounds_key(b):
    return None if b is None else bytes(b[0].raw[:b[1]])


def test_snapshot_parity_all_stageable_cases(cases, oracle_results):
    checked = 0
    skipped = set()
    built = 0
    for case in cases:
        snaps = {}  # (read time, bounds) -> snapshot, shared by the runs
        try:
            for c, ri, rm, preds, aggs, lo, hi in sc.iter_runs([case]):
                if not y.stageable(case["schema"], preds, aggs):
                    skipped.add(case["name"])
                    continue
                key = (rm, _bounds_key(lo), _bounds_key(hi))
                if key not in snaps:
                    snaps[key] = build_snapshot(case, rm, lo, hi)
                    built += 1
                gres = snaps[key].query(list(preds), list(aggs))
                try:
                    check_match(gres, oracle_results[(case["name"], ri)],
                                aggs, check_entries=lo is None and hi is None)
                except AssertionError as e:
                    raise AssertionError(
                        f"case {case['name']} read={rm}: {e}") from e
                checked += 1
        finally:
            for snap in snaps.values():
                snap.close()
    assert skipped == sc.NOT_STAGEABLE_CASES, skipped
    assert checked >= sc.N_STAGEABLE_RUNS, checked
    # wide_fixed_32cols (2 runs) and in_list_preds (3 runs) share one
    # snapshot each: 3 fewer builds than runs
    assert built == checked - 3, (built, checked)


@pytest.mark.parametrize("n", sc.EDGE_SIZES)
def test_snapshot_row_count_edges(n):
    case = sc.edge_tablet(n)
    preds, aggs = sc.edge_query()
    snap = build_snapshot(case, sc.EDGE_READ)
    try:
        assert snap.info().n_rows == n
        check_match(snap.query(preds, aggs),
                    run_oracle(case, sc.EDGE_READ, preds, aggs), aggs)
    finally:
        snap.close()


def test_snapshot_empty():
    """Read time before every write: a valid snapshot of zero rows."""
    case = sc.edge_tablet(65)
    preds, aggs = sc.edge_query()
    snap = build_snapshot(case, sc.EDGE_READ_BEFORE)
    try:
        assert snap.info().n_rows == 0
        res = snap.query(preds, aggs)
        assert res.rows_scanned == 0 and res.rows_matched == 0
        assert all(res.aggs[i].is_null for i in range(len(aggs)))
        check_match(res, run_oracle(case, sc.EDGE_READ_BEFORE, preds, aggs),
                    aggs)
    finally:
        snap.close()


def test_snapshot_nullable_specialisation():
    preds, aggs = sc.edge_query()
    preds2, aggs2 = sc.edge_query_no_null_col()
    # no NULLs anywhere: nullable_cols == 0, the no-mask kernel variant
    dense = sc.edge_tablet(777, nulls=False)
    snap = build_snapshot(dense, sc.EDGE_READ)
    try:
        assert snap.info().nullable_cols == 0
        check_match(snap.query(preds, aggs),
                    run_oracle(dense, sc.EDGE_READ, preds, aggs), aggs)
    finally:
        snap.close()
    # NULLs only in a column the query does not reference
    sparse = sc.edge_tablet(777, nulls=True)
    snap = build_snapshot(sparse, sc.EDGE_READ)
    try:
        assert snap.info().nullable_cols == 0b010
        check_match(snap.query(preds2, aggs2),
                    run_oracle(sparse, sc.EDGE_READ, preds2, aggs2), aggs2)
        # and the masked variant on the same snapshot
        check_match(snap.query(preds, aggs),
                    run_oracle(sparse, sc.EDGE_READ, preds, aggs), aggs)
    finally:
        snap.close()


def test_snapshot_every_kernel_shape():
    """Every GT..NE instantiation of the query kernel runs at least once:
    predicate cap 4 and 8 (2 and 5 predicates) x aggregate cap 2 / 4 / 8,
    each without the null-mask read (dense tablet) and with it."""
    for nulls in (False, True):
        case = sc.edge_tablet(777, nulls=nulls)
        snap = build_snapshot(case, sc.EDGE_READ)
        try:
            assert bool(snap.info().nullable_cols) == nulls
            for n_preds, n_aggs in sc.KERNEL_SHAPES:
                preds, aggs = sc.shape_query(n_preds, n_aggs)
                ores = run_oracle(case, sc.EDGE_READ, preds, aggs)
                assert 0 < ores.rows_matched < 777
                try:
                    check_match(snap.query(preds, aggs), ores, aggs)
                except AssertionError as e:
                    raise AssertionError(
                        f"nulls={nulls} preds={n_preds} aggs={n_aggs}: {e}"
                    ) from e
        finally:
            snap.close()


def _range_sharded_tablet(rows=20000):
    """Range-sharded (no hash prefix): a leading-key IN predicate makes
    feed_blocks prune the uploaded block set."""
    schema = y.make_schema([y.KT_INT64],
                           [(10, y.T_INT64, 1), (11, y.T_INT64, 1)],
                           has_hash=False)
    b = y.Builder(schema)
    for r in range(rows):
        b.add_packed_row(1000, [(y.T_INT64, r), (y.T_INT64, r * 3)],
                         key_datums=(r,))
    _KEEP.append(b)
    from parity_cases import _case
    return _case("range_sharded", schema, b.finish(), [])


_KEEP = []


def test_snapshot_from_option_pruned_handle(monkeypatch):
    """A handle whose feed pruned blocks by its leading-key IN predicate
    does not hold every row inside the bounds: a snapshot build from it is
    refused (code 9), never silently short. The same handle still serves
    its own query in YBG_STAGE mode, and a handle opened without the
    predicate yields a snapshot that answers queries WITHOUT it exactly."""
    gpu_scan = _gpu()
    monkeypatch.delenv("YBG_NOPRUNE", raising=False)
    monkeypatch.delenv("YBG_STAGE", raising=False)
    case = _range_sharded_tablet()
    blob = b"".join(struct.pack("<q", v) for v in (5, 9177, 19998))
    buf = (y.C.c_uint8 * len(blob)).from_buffer_copy(blob)
    in_pred = [y.Pred(1, 0, y.PRED_IN, 0, buf, len(blob))]
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 1)]
    other = [y.Pred(0, 0, y.PRED_GE, 10_000, None, 0)]
    rm = 5000
    o_in = run_oracle(case, rm, in_pred, aggs)
    o_other = run_oracle(case, rm, other, aggs)
    o_all = run_oracle(case, rm, (), aggs)
    assert o_in.rows_matched == 3 and o_all.rows_scanned == 20000

    s = _run_handle(case, rm, in_pred, aggs, None, None)
    try:
        s.execute()
        blk = s.aggregates()
        assert blk.entries_seen < 2000      # the feed did prune
        with pytest.raises(gpu_scan.GpuScanError, match="rc=9"):
            s.snapshot()
        # its own query, staged: same contents as its block path
        monkeypatch.setenv("YBG_STAGE", "1")
        s.execute()
        assert s.staged()
        _same(s.aggregates(), blk, len(aggs))
        # a pruned scan visits fewer rows than the oracle's full scan by
        # design; what it selects and aggregates is the same
        assert blk.rows_matched == o_in.rows_matched
        for i in range(len(aggs)):
            assert blk.aggs[i].value_i64 == o_in.aggs[i].value_i64
        monkeypatch.delenv("YBG_STAGE")
    finally:
        s.close()

    # without the predicate on the handle: the whole tablet is staged
    snap = build_snapshot(case, rm)
    try:
        assert snap.info().n_rows == 20000
        check_match(snap.query([], aggs), o_all, aggs)
        check_match(snap.query(other, aggs), o_other, aggs)
        check_match(snap.query(in_pred, aggs), o_in, aggs)
    finally:
        snap.close()


def test_stage_survives_freed_option_list(cases, monkeypatch):
    """The handle keeps its own copy of the spec's option lists: a staged
    execute after the caller's buffer is gone still sees the list."""
    monkeypatch.setenv("YBG_STAGE", "1")
    case = next(c for c in cases if c["name"] == "in_list_preds")
    rm, preds, aggs = case["runs"][0][:3]
    src = preds[0]
    blob = bytes(src.bytes[:src.bytes_len])
    buf = (y.C.c_uint8 * len(blob)).from_buffer_copy(blob)
    mine = [y.Pred(0, 0, y.PRED_IN, 0, buf, len(blob))]
    s = _run_handle(case, rm, mine, aggs, None, None)
    try:
        y.C.memset(buf, 0xff, len(blob))    # the caller's list is gone
        s.execute()
        assert s.staged()
        check_match(s.aggregates(), run_oracle(case, rm, preds, aggs), aggs)
    finally:
        s.close()


def test_snapshot_determinism(cases):
    """Two separately built snapshots (emit order differs run to run), each
    queried twice: all four results bit-identical, double SUM included."""
    case = next(c for c in cases if c["name"] == "mixed_types")
    rm, preds, aggs = case["runs"][0][:3]
    results = []
    for _ in range(2):
        snap = build_snapshot(case, rm)
        try:
            results.append(snap.query(list(preds), list(aggs)))
            results.append(snap.query(list(preds), list(aggs)))
        finally:
            snap.close()
    r0 = results[0]
    assert r0.rows_matched > 0
    for r in results[1:]:
        assert r.rows_matched == r0.rows_matched
        for i in range(len(aggs)):
            assert r.aggs[i].value_i64 == r0.aggs[i].value_i64
            # bit-identical, not merely equal
            assert (struct.pack("<d", r.aggs[i].value_f64) ==
                    struct.pack("<d", r0.aggs[i].value_f64))


def test_snapshot_errors(cases):
    gpu_scan = _gpu()
    case = next(c for c in cases if c["name"] == "v1_nonnullable_fixed")
    # schema: int64, int32, STRING, int64
    rm = case["runs"][0][0]
    good_aggs = list(case["runs"][0][2])
    ores = run_oracle(case, rm, (), good_aggs)
    tup = next(c for c in cases if c["name"] == "in_tuple_keycols")
    cnt = [y.Agg(y.AGG_COUNT_STAR, 0)]
    bad = [
        ([y.Pred(0, 2, y.PRED_EQ, 0, None, 0)], cnt, "predicate 0"),
        (list(tup["runs"][0][1]), cnt, "predicate 0"),
        ([], [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 2)],
         "aggregate 1"),
        ([y.Pred(0, 4, y.PRED_GT, 0, None, 0)], cnt, "predicate 0"),
        ([], [y.Agg(y.AGG_SUM_INT64, 4)], "aggregate 0"),
        ([y.Pred(0, 0, y.PRED_GT, 0, None, 0)] * 9, cnt, "num_preds"),
    ]
    snap = build_snapshot(case, rm)
    try:
        for preds, aggs, names in bad:
            with pytest.raises(gpu_scan.GpuScanError) as ei:
                snap.query(preds, aggs)
            assert ei.value.code == 9, str(ei.value)
            assert names in str(ei.value), str(ei.value)
            # the snapshot still answers a valid query correctly
            check_match(snap.query([], good_aggs), ores, good_aggs)
    finally:
        snap.close()


def _run_handle(case, rm, preds, aggs, lo, hi):
    gpu_scan = _gpu()
    spec = make_spec(case, rm, preds, aggs, lo, hi)
    s = gpu_scan.GpuScan(spec)
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    return s


def _same(a, b, n_aggs):
    assert (a.rows_scanned, a.rows_matched, a.entries_seen) == \
        (b.rows_scanned, b.rows_matched, b.entries_seen)
    assert bytes(a.restart_ht) == bytes(b.restart_ht)
    for i in range(n_aggs):
        assert a.aggs[i].is_null == b.aggs[i].is_null
        assert a.aggs[i].value_i64 == b.aggs[i].value_i64
        assert a.aggs[i].value_f64 == b.aggs[i].value_f64 or \
            a.aggs[i].is_null


def test_stage_env_transparent_mode(cases, oracle_results, monkeypatch):
    monkeypatch.setenv("YBG_STAGE", "1")
    staged = unstaged = 0
    for case, ri, rm, preds, aggs, lo, hi in sc.iter_runs(cases):
        s = _run_handle(case, rm, preds, aggs, lo, hi)
        try:
            s.execute()
            res = s.aggregates()
            ok = y.stageable(case["schema"], preds, aggs)
            assert s.staged() == ok, case["name"]
            try:
                check_match(res, oracle_results[(case["name"], ri)], aggs,
                            check_entries=lo is None and hi is None)
            except AssertionError as e:
                raise AssertionError(
                    f"case {case['name']} read={rm} staged={ok}: {e}") from e
            if ok:
                # a second execute reuses the handle's snapshot
                s.execute()
                assert s.staged()
                _same(s.aggregates(), res, len(aggs))
                assert s.kernel_ms()[0] > 0 or res.rows_scanned == 0
                staged += 1
            else:
                unstaged += 1
        finally:
            s.close()
    assert staged >= sc.N_STAGEABLE_RUNS
    assert unstaged == sc.N_NOT_STAGEABLE_RUNS


def test_stage_env_unset_or_zero_takes_block_path(cases, monkeypatch):
    case = cases[0]
    rm, preds, aggs = case["runs"][0][:3]
    for val in (None, "0"):
        if val is None:
            monkeypatch.delenv("YBG_STAGE", raising=False)
        else:
            monkeypatch.setenv("YBG_STAGE", val)
        s = _run_handle(case, rm, preds, aggs, None, None)
        try:
            s.execute()
            s.aggregates()
            assert not s.staged()
        finally:
            s.close()


def test_stage_matches_block_path_bitwise(cases, monkeypatch):
    """Same struct contents from both modes, entries_seen and restart_ht
    included (integer aggregates: exact in any fold order)."""
    case = cases[0]  # config2_filtered_sum
    rm, preds, aggs = case["runs"][0][:3]
    out = []
    for val in ("0", "1"):
        monkeypatch.setenv("YBG_STAGE", val)
        s = _run_handle(case, rm, preds, aggs, None, None)
        try:
            s.execute()
            out.append(s.aggregates())
            assert s.staged() == (val == "1")
        finally:
            s.close()
    _same(out[0], out[1], len(aggs))


def test_snapshot_info(cases, oracle_results):
    case = next(c for c in cases if c["name"] == "mixed_types")
    rm = case["runs"][0][0]
    ores = oracle_results[("mixed_types", 0)]
    snap = build_snapshot(case, rm)
    try:
        info = snap.info()
        assert info.n_rows == ores.rows_scanned
        assert info.entries_seen == ores.entries_seen  # unbounded case
        # int64 + double value columns and the int64 key column are staged;
        # the string column (bit 2) is not
        assert info.staged_value_cols == 0b011
        assert info.device_bytes >= info.n_rows * (8 * 3 + 4)
        assert info.build_ms > 0
        snap.query([], [y.Agg(y.AGG_COUNT_STAR, 0)])
        assert snap.kernel_ms() > 0
    finally:
        snap.close()
