"""Column plan of the fast kernel (build_fast_plan + the planned
packed-row pass of scan_batch_fast), on the host simulator: a plannable
spec must run the planned pass and give bit-equal results with the
interpreted fast pass (YBG_PLAN=0) and the general simulator; a spec
outside the plan's rules must report no plan and stay bit-equal."""
import ctypes as C
import functools
import os
import struct

import pytest

import ybgpu as y

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
ROWS = 3000


def _u64(v):
    return v & ((1 << 64) - 1)


def _res(r):
    return (r.entries_seen, r.rows_scanned, r.rows_matched,
            tuple((r.aggs[i].is_null, r.aggs[i].value_i64) for i in range(2)),
            bytes(r.restart_ht[:r.restart_ht_len]))


def _spec(schema, preds=(), aggs=(), read=1_700_000_000_000_000, local=None,
          glob=None, expect_versions=0):
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(read, local, glob) if local else \
        y.read_time(read)
    spec.num_preds = len(preds)
    for i, p in enumerate(preds):
        spec.preds[i] = p
    spec.num_aggs = len(aggs)
    for i, a in enumerate(aggs):
        spec.aggs[i] = a
    spec.expect_versions = expect_versions
    return spec


def _pred(col, op, c):
    return y.Pred(0, col, op, _u64(c), None, 0)


# column values of row r; col 0 takes both signs, col 1 repeats, col 3 holds
# the int64 extremes in a few rows
def _row4(r):
    c3 = I64_MIN if r % 701 == 0 else (I64_MAX if r % 703 == 0 else -3 * r)
    return [r * 10 - 15000, (r * 7919) % 1000, r, c3]


@functools.lru_cache(maxsize=None)
def _tablet4():
    schema = y.make_schema([y.KT_INT64],
                           [(10 + i, y.T_INT64, 1) for i in range(4)])
    b = y.Builder(schema)
    seq = 1 << 50
    for r in range(ROWS):
        seq += 1
        b.add_packed_row(1000, [(y.T_INT64, v) for v in _row4(r)],
                         hash_=r // 512, key_datums=(r,), seq=seq)
    return schema, b.finish()


@functools.lru_cache(maxsize=None)
def _tablet8(narrow_middle):
    """8 value columns; the middle ones are int32 when narrow_middle."""
    mid = y.T_INT32 if narrow_middle else y.T_INT64
    dts = [y.T_INT64] + [mid] * 6 + [y.T_INT64]
    schema = y.make_schema([y.KT_INT64],
                           [(10 + i, dts[i], 1) for i in range(8)])
    b = y.Builder(schema)
    seq = 1 << 50
    for r in range(ROWS):
        seq += 1
        vals = [(dts[i], r * (i + 1) - 1000 * i) for i in range(8)]
        b.add_packed_row(1000, vals, hash_=r // 512, key_datums=(r,),
                         seq=seq)
    return schema, b.finish()


@functools.lru_cache(maxsize=None)
def _tablet_mixed():
    """int64, int32, double, int64: the widths and types the plan leaves to
    the interpreted pass."""
    dts = [y.T_INT64, y.T_INT32, y.T_DOUBLE, y.T_INT64]
    schema = y.make_schema([y.KT_INT64],
                           [(10 + i, dts[i], 1) for i in range(4)])
    b = y.Builder(schema)
    seq = 1 << 50
    for r in range(ROWS):
        seq += 1
        b.add_packed_row(1000, [(y.T_INT64, r - 1500), (y.T_INT32, r - 700),
                                (y.T_DOUBLE, r * 0.25), (y.T_INT64, 5 * r)],
                         hash_=r // 512, key_datums=(r,), seq=seq)
    return schema, b.finish()


@functools.lru_cache(maxsize=None)
def _tablet_mvcc():
    """test_fast_mvcc_and_restart's multi-version + tombstone data."""
    schema = y.make_schema([y.KT_INT64], [(10, y.T_INT64, 1)])
    b = y.Builder(schema)
    seq = 1 << 50
    for r in range(4000):
        for ht in (3000, 2000, 1000):
            seq += 1
            if r % 17 == 0 and ht == 3000:
                b.add_row_tombstone(ht, hash_=r // 512, key_datums=(r,),
                                    seq=seq)
            else:
                b.add_packed_row(ht, [(y.T_INT64, r * 7 + ht)],
                                 hash_=r // 512, key_datums=(r,), seq=seq)
    return schema, b.finish()


def _with_env(fn, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check(spec, built, want_plan, ivbs=(1, 2, 16)):
    """planned (or not) as expected, and YBG_PLAN=1 == YBG_PLAN=0 ==
    general simulator at every batch size, fallback count included."""
    data, offsets, nb = built[0], built[1], built[2]
    assert _with_env(lambda: y.sim_scan_planned(spec), YBG_PLAN=1) \
        == want_plan
    assert _with_env(lambda: y.sim_scan_planned(spec), YBG_PLAN=0) is False
    for ivb in ivbs:
        ref = _res(_with_env(lambda: y.sim_scan(spec, data, offsets, nb),
                             YBG_IVB=ivb))
        on, nf_on = _with_env(
            lambda: y.sim_scan_fast(spec, data, offsets, nb),
            YBG_IVB=ivb, YBG_PLAN=1)
        off, nf_off = _with_env(
            lambda: y.sim_scan_fast(spec, data, offsets, nb),
            YBG_IVB=ivb, YBG_PLAN=0)
        assert _res(on) == ref, ("plan", ivb)
        assert _res(off) == ref, ("interpreted", ivb)
        assert nf_on == nf_off, ivb
    return ref


SUM3 = [y.Agg(y.AGG_SUM_INT64, 3), y.Agg(y.AGG_COUNT_STAR, 0)]
OPS = [y.PRED_GT, y.PRED_GE, y.PRED_LT, y.PRED_LE, y.PRED_EQ]
PRESENT = 10 * 1234 - 15000  # col 0 of row 1234


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("c", [PRESENT - 1, PRESENT, PRESENT + 1,
                               I64_MIN, I64_MAX])
def test_plan_single_operator(op, c):
    schema, built = _tablet4()
    spec = _spec(schema, [_pred(0, op, c)], SUM3)
    ref = _check(spec, built, True)
    vals = [_row4(r)[0] for r in range(ROWS)]
    want = sum({y.PRED_GT: v > c, y.PRED_GE: v >= c, y.PRED_LT: v < c,
                y.PRED_LE: v <= c, y.PRED_EQ: v == c}[op] for v in vals)
    assert ref[2] == want  # the range fold selects what the operator says


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("c", [I64_MIN, I64_MAX, -1, 0])
def test_plan_extreme_values_in_data(op, c):
    """Predicates on the column that holds INT64_MIN / INT64_MAX."""
    schema, built = _tablet4()
    spec = _spec(schema, [_pred(3, op, c)],
                 [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 0)])
    _check(spec, built, True)


@pytest.mark.parametrize("preds,matched", [
    # a real intersection: 100 < col2 <= 2000
    ([(2, y.PRED_GT, 100), (2, y.PRED_LE, 2000)], 1900),
    # a single point
    ([(2, y.PRED_GE, 777), (2, y.PRED_LE, 777)], 1),
    ([(2, y.PRED_GE, 700), (2, y.PRED_EQ, 777), (2, y.PRED_LT, 778)], 1),
    # empty intersections
    ([(2, y.PRED_GT, 2000), (2, y.PRED_LT, 100)], 0),
    ([(2, y.PRED_EQ, 5), (2, y.PRED_EQ, 6)], 0),
    ([(2, y.PRED_GE, 10), (2, y.PRED_LE, 20), (2, y.PRED_GT, 20)], 0),
    ([(2, y.PRED_GT, I64_MAX), (2, y.PRED_GE, 0)], 0),
    ([(2, y.PRED_LT, I64_MIN), (2, y.PRED_LE, 10)], 0),
    # three predicates, real intersection, plus another column
    ([(2, y.PRED_GE, 10), (2, y.PRED_LT, 2500), (2, y.PRED_GT, 11),
      (1, y.PRED_LT, 500)], None),
])
def test_plan_predicates_intersect(preds, matched):
    schema, built = _tablet4()
    spec = _spec(schema, [_pred(*p) for p in preds], SUM3)
    ref = _check(spec, built, True)
    if matched is not None:
        assert ref[2] == matched


@pytest.mark.parametrize("preds,aggs", [
    # predicate and aggregate on the same column
    ([(0, y.PRED_GT, 0)], [y.Agg(y.AGG_SUM_INT64, 0),
                           y.Agg(y.AGG_COUNT, 0)]),
    # aggregate on a column with no predicate
    ([(0, y.PRED_LT, 0)], [y.Agg(y.AGG_SUM_INT64, 1),
                           y.Agg(y.AGG_SUM_INT64, 2)]),
    # COUNT(*) alone, with and without predicates
    ([(1, y.PRED_GE, 500)], [y.Agg(y.AGG_COUNT_STAR, 0)]),
    ([], [y.Agg(y.AGG_COUNT_STAR, 0)]),
    # no predicates at all
    ([], SUM3),
    ([], [y.Agg(y.AGG_COUNT, 2), y.Agg(y.AGG_SUM_INT64, 3)]),
    # the headline shape: three ranged columns and the sum
    ([(0, y.PRED_GT, 0), (1, y.PRED_LT, 750), (2, y.PRED_GE, 40)], SUM3),
    # four ranged columns
    ([(0, y.PRED_GT, -9000), (1, y.PRED_LT, 900), (2, y.PRED_GE, 40),
      (3, y.PRED_LE, -30)], SUM3),
    # no aggregates
    ([(0, y.PRED_GT, 0)], []),
])
def test_plan_aggregate_shapes(preds, aggs):
    schema, built = _tablet4()
    _check(_spec(schema, [_pred(*p) for p in preds], aggs), built, True)


@pytest.mark.parametrize("narrow_middle", [False, True])
@pytest.mark.parametrize("preds", [
    [(0, y.PRED_GT, 100)],
    [(0, y.PRED_GT, 100), (7, y.PRED_LE, 8 * 2500 - 7000)],
    [],
])
def test_plan_eight_columns_live_at_both_ends(narrow_middle, preds):
    """NC = 8: live columns first and last, inert ones (int64 or narrower)
    between them."""
    schema, built = _tablet8(narrow_middle)
    spec = _spec(schema, [_pred(*p) for p in preds],
                 [y.Agg(y.AGG_SUM_INT64, 7), y.Agg(y.AGG_SUM_INT64, 0)])
    _check(spec, built, True)


def test_plan_more_than_four_ranged_columns():
    """Five ranged columns run the 8-wide pass with padding slots."""
    schema, built = _tablet8(False)
    preds = [_pred(i, y.PRED_GE, 50 * (i + 1) - 1000 * i) for i in range(5)]
    _check(_spec(schema, preds, [y.Agg(y.AGG_COUNT_STAR, 0),
                                 y.Agg(y.AGG_SUM_INT64, 6)]), built, True)


@pytest.mark.parametrize("expect_versions", [0, 1])
def test_plan_mvcc_and_restart(expect_versions):
    schema, built = _tablet_mvcc()
    for read, local, glob in ((2500, 3500, 4500), (1500, 1500, None),
                              (500, 900, 1200), (9000, 9500, 9900)):
        spec = _spec(schema, [_pred(0, y.PRED_GT, 100)],
                     [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 0)],
                     read, local, glob or local,
                     expect_versions=expect_versions)
        _check(spec, built, True)
        _, nf = y.sim_scan_fast(spec, built[0], built[1], built[2])
        assert nf == 0


@pytest.mark.parametrize("preds,aggs", [
    # NE keeps the interpreted pass
    ([(0, y.PRED_NE, 17)], [y.Agg(y.AGG_COUNT_STAR, 0)]),
    ([(0, y.PRED_GT, 0), (3, y.PRED_NE, 50)], [y.Agg(y.AGG_SUM_INT64, 3)]),
    # a double predicate
    ([(2, y.PRED_GT,
       struct.unpack("<q", struct.pack("<d", 100.0))[0])],
     [y.Agg(y.AGG_COUNT_STAR, 0)]),
    # MIN / MAX / SUM_DOUBLE are not additive
    ([(0, y.PRED_GT, 0)], [y.Agg(y.AGG_MIN_INT64, 3)]),
    ([], [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_MAX_INT64, 0)]),
    ([], [y.Agg(y.AGG_SUM_DOUBLE, 2)]),
    # narrower widths are left to the interpreted pass: int32 predicate,
    # int32 sum
    ([(1, y.PRED_LT, -5)], [y.Agg(y.AGG_COUNT_STAR, 0)]),
    ([(0, y.PRED_LT, 5)], [y.Agg(y.AGG_SUM_INT64, 1)]),
])
def test_plan_ineligible_specs_stay_interpreted(preds, aggs):
    schema, built = _tablet_mixed()
    _check(_spec(schema, [_pred(*p) for p in preds], aggs), built, False)


def test_plan_count_on_narrow_column_is_planned():
    """COUNT reads no operand, so the column's width does not matter."""
    schema, built = _tablet_mixed()
    _check(_spec(schema, [_pred(0, y.PRED_GE, 0)],
                 [y.Agg(y.AGG_COUNT, 1), y.Agg(y.AGG_SUM_INT64, 3)]),
           built, True)


@pytest.mark.parametrize("nc_cap,ncols", [(4, 4), (8, 8), (4, 3), (8, 5)])
@pytest.mark.parametrize("align", range(8))
def test_plan_column_extraction_all_alignments(nc_cap, ncols, align):
    """plan_load_cols against a plain byte copy, the value starting at every
    alignment mod 8 and the last column ending exactly where the buffer's
    16 bytes of tail slack begin."""
    body = 3 + 8 * ncols
    slack = 16
    raw = (C.c_uint8 * (8 + align + body + slack))()
    start = (-C.addressof(raw)) % 8 + align  # (address of value) % 8 == align
    assert (C.addressof(raw) + start) % 8 == align
    assert start + body + slack <= len(raw)
    for i in range(len(raw)):
        raw[i] = (i * 37 + 11) & 0xff
    got = y.sim_plan_extract(raw, start, ncols, nc_cap)
    want = [struct.unpack_from("<Q", bytes(raw), start + 3 + 8 * k)[0]
            for k in range(ncols)]
    assert got == want
