"""Shared pieces of the ordered snapshot select tests
(test_snapshot_order_sim.py on the CPU simulator, test_snapshot_order_gpu.py
on the HIP kernels): the reference, the order tablet and the scenarios. A
scenario takes `run`:

    run(case, read_micros, preds, cols, order_by, descending=False,
        nulls_first=False, limit=0, after=None, row_lo=0, row_hi=None,
        cap=CAP, lower=None, upper=None, strings=False, varlen_cap=VCAP,
        backward=False)
      -> (rows, (datums, null_masks, row_ids, varlen, varlen_size), result)

rows being the decoded tuples (ybgpu.decode_snapshot_rows), result a
SnapshotOrderResult; errors raise with .code, .result and .varlen_size.

Reference: the oracle's matching rows in key order
(snapshot_select_cases.oracle_rows), sorted here by a key function written
from the contract in include/yb_gpu_scan.h; limit and cursor are slices of
that list. Every comparison is exact."""
import functools
import struct

import pytest

import ybgpu as y
from parity_cases import SCHEMA_4I, _case
import snapshot_cases as sc
import snapshot_select_cases as ss
import snapshot_string_cases as st

CAP = 1 << 12
VCAP = 1 << 18
I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)
U64 = (1 << 64) - 1

# Digit passes of a selection that runs to full depth (YBG_SNAP_ORDER_CAND=1):
# the key is NULL class (1 bit) + image (64) + position (32); the first digit
# takes the class and the image's top byte, then 7 image bytes, then 4
# position bytes.
FULL_DEPTH = 1 + 7 + 4

# stageable runs of parity_cases.build_cases(): pinned, so a silently skipped
# run fails (the same set as snapshot_select_cases.N_SELECT_RUNS)
N_ORDER_RUNS = 31

_KEEP = []


# ---- reference -------------------------------------------------------------

def _order_dtype(schema, order_by):
    is_key, col = order_by
    return y.T_INT64 if is_key else schema.value_cols[col].dtype


def value_key(dtype, datum, descending):
    """The value component of the order, for a non-NULL datum."""
    if dtype == y.T_DOUBLE:
        x = struct.unpack("<d", struct.pack("<Q", datum))[0]
    elif dtype == y.T_FLOAT:
        x = struct.unpack("<f", struct.pack("<I", datum & 0xffffffff))[0]
    else:
        x = datum - (1 << 64) if datum >= (1 << 63) else datum   # signed
        return -x if descending else x
    # -0.0 == 0.0 in Python too; every NaN is one class above every number
    k = (1, 0.0) if x != x else (0, x)
    return (-k[0], -k[1]) if descending else k


def sort_key(dtype, descending, nulls_first):
    def key(item):
        pos, _row, od = item
        if od is None:
            return (0 if nulls_first else 1, 0, pos)
        return (1 if nulls_first else 0, value_key(dtype, od, descending),
                pos)
    return key


def key_cols(schema):
    return [(1, c) for c in range(schema.num_hash_cols +
                                  schema.num_range_cols)]


_POS = {}


def positions(case, read_micros, lower=None, upper=None):
    """key tuple -> snapshot position (the index among the visible rows in
    key order)."""
    k = (case["name"], read_micros, bool(lower), bool(upper))
    if k not in _POS:
        rows = ss.oracle_rows(case, read_micros, [], key_cols(case["schema"]),
                              lower, upper)
        _POS[k] = {r: i for i, r in enumerate(rows)}
        assert len(_POS[k]) == len(rows)
    return _POS[k]


def matching(case, read_micros, preds, cols, order_by, lower=None,
             upper=None, pos_is_key=False):
    """[(position, projected row, order datum or None)] in key order.
    pos_is_key: a generated tablet (key = r, so position == key): skips the
    full scan that maps keys to positions."""
    kc = key_cols(case["schema"])
    rows = ss.oracle_rows(case, read_micros, preds,
                          kc + list(cols) + [order_by], lower, upper)
    nk = len(kc)
    if pos_is_key:
        return [(r[0], r[nk:-1], r[-1]) for r in rows]
    pos = positions(case, read_micros, lower, upper)
    return [(pos[r[:nk]], r[nk:-1], r[-1]) for r in rows]


def ordered(items, dtype, descending, nulls_first, row_lo=0, row_hi=None):
    win = [it for it in items
           if it[0] >= row_lo and (row_hi is None or it[0] < row_hi)]
    return sorted(win, key=sort_key(dtype, descending, nulls_first))


def cursor_of(item):
    pos, _row, od = item
    return (1 if od is None else 0, 0 if od is None else od, pos)


def check(run, case, read_micros, preds, cols, order_by, full, start=0,
          limit=0, descending=False, nulls_first=False, passes=None, **kw):
    """One call equals the slice full[start : start + limit] of the ordered
    reference, `start` > 0 passing the cursor of full[start - 1]."""
    after = cursor_of(full[start - 1]) if start else None
    want = full[start:start + limit] if limit else full[start:]
    kw.setdefault("cap", max(len(want), 1))
    rows, raw, res = run(case, read_micros, preds, cols, order_by,
                         descending=descending, nulls_first=nulls_first,
                         limit=limit, after=after, **kw)
    tag = (case["name"], order_by, descending, nulls_first, start, limit)
    assert res.r.n_rows == len(want), (tag, res.r.n_rows, len(want))
    assert list(raw[2][:res.r.n_rows]) == [w[0] for w in want], tag
    assert rows == [w[1] for w in want], (tag, next(
        (i, g, w[1]) for i, (g, w) in enumerate(zip(rows, want))
        if g != w[1]))
    assert res.r.rows_matched == len(full) - start, tag
    assert res.r.done == (1 if start + len(want) == len(full) else 0), tag
    assert res.r.resume_row == 0
    if want:
        assert y.order_cursor(res) == cursor_of(want[-1]), tag
    else:
        assert res.digit_passes == 0, tag
    if passes is not None:
        assert res.digit_passes == passes, (tag, res.digit_passes)
    return rows, raw, res


def raw_bytes(raw, res, num_cols, cap):
    """Everything a call wrote, as bytes (st.raw_bytes with the result's
    select part)."""
    return st.raw_bytes(raw, res.r, num_cols, cap)


def order_cols(schema):
    """Every numeric key and value column: what a select can be ordered by."""
    return ss.all_cols(schema)


# ---- 1. parity on the shared cases -----------------------------------------

def scenario_parity(run, cases):
    checked = 0
    for case, _ri, read_micros, preds, _aggs, lower, upper in \
            sc.iter_runs(cases):
        if not y.stageable(case["schema"], preds, ()):
            continue
        preds = list(preds)
        big = case["name"] == "config2_filtered_sum"
        if big:
            # 200k rows through the oracle's Python row callback are slow:
            # here the generated tablet's position == key and only limit=3
            # runs; the unlimited runs are on the 20k tablet below
            assert case["schema"] is SCHEMA_4I
        _parity_one(run, case, read_micros, preds, lower, upper,
                    pos_is_key=big, limits=(3,) if big else (0, 3))
        checked += 1
    assert checked == N_ORDER_RUNS == ss.N_SELECT_RUNS, checked
    case, preds = ss.filtered_20k()
    _parity_one(run, case, 1_700_000_000_000_000, preds, None, None,
                pos_is_key=True, limits=(0, 3))


def _parity_one(run, case, read_micros, preds, lower, upper, pos_is_key,
                limits):
    schema = case["schema"]
    cols = ss.all_cols(schema)
    assert order_cols(schema) == cols
    # one oracle scan: every order column is also projected
    base = matching(case, read_micros, preds, cols, cols[0], lower, upper,
                    pos_is_key)
    for j, ob in enumerate(cols):
        items = [(pos, row, row[j]) for pos, row, _od in base]
        for desc in (False, True):
            full = ordered(items, _order_dtype(schema, ob), desc, False)
            for limit in limits:
                check(run, case, read_micros, preds, cols, ob, full,
                      limit=limit, descending=desc, lower=lower, upper=upper)


# ---- 2. the order tablet ---------------------------------------------------

ORDER_SCHEMA = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_DOUBLE, 1), (12, y.T_INT32, 1),
     (13, y.T_FLOAT, 1), (14, y.T_BOOL, 1), (15, y.T_INT64, 1)])
ORDER_READ = 1_000_000     # after every write (rows are written at 1000 + r)

NEG_NAN_PAYLOAD = 0xFFF8000000000123   # sign bit set, quiet, payload 0x123
NEG_ZERO = 0x8000000000000000
NEG_ZERO_F = 0x80000000


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def order_double(r):
    cyc = (None, float("nan"), _f64(NEG_NAN_PAYLOAD), float("-inf"), -0.0,
           0.0, 1.5, float("inf"), -2.25, r * 0.5)
    return cyc[r % 10]


def order_float(r):
    cyc = (0.0, -0.0, float("nan"), 1.25, -3.5, r * 0.25, float("inf"),
           -float("nan"))
    return cyc[r % 8]


def order_edge_int(r):
    if r % 4 == (r // 4) % 4:      # one NULL in every four rows, rotating
        return None
    return (I64_MAX, I64_MIN, -1, 0)[r % 4]


@functools.lru_cache(maxsize=None)
def order_tablet(n):
    """n rows, int64 key r (position == r); value columns:
    0 int64 (r * 37) % 11 - 5: heavy ties, negatives;
    1 double cycling NULL, NaN, a negative NaN with a payload, -inf, -0.0,
      +0.0, 1.5, +inf, -2.25, r * 0.5;
    2 int32 r % 7, NULL on every 5th row;
    3 float cycling +0.0, -0.0, NaN, 1.25, -3.5, r * 0.25, +inf, -NaN;
    4 bool;
    5 int64 cycling INT64_MAX, INT64_MIN, -1, 0 with one NULL per four rows."""
    b = y.Builder(ORDER_SCHEMA)
    for r in range(n):
        b.add_packed_row(
            1000 + r,
            [(y.T_INT64, (r * 37) % 11 - 5), (y.T_DOUBLE, order_double(r)),
             (y.T_INT32, None if r % 5 == 4 else r % 7),
             (y.T_FLOAT, order_float(r)), (y.T_BOOL, (r // 3) % 2),
             (y.T_INT64, order_edge_int(r))],
            hash_=min(r // 64, 65535), key_datums=(r,))
    _KEEP.append(b)
    return _case("order_%d" % n, ORDER_SCHEMA, b.finish(), [])


ORDER_COLS = [(1, 0)] + [(0, c) for c in range(6)]
# a third of the rows, from every tile
ORDER_PRED = [y.Pred(0, 0, y.PRED_LT, (-1) & U64, None, 0)]


def order_items(n, preds, ob):
    return matching(order_tablet(n), ORDER_READ, preds, ORDER_COLS, ob)


def scenario_order_tablet(run, n, cand_one=False):
    """Every column x ASC/DESC x nulls_first over limits 1, 2, E - 1, E,
    E + 1 and 0; an odd window; a predicate that matches nothing. cand_one:
    the caller set YBG_SNAP_ORDER_CAND=1 (every selection runs to full
    depth). Returns every call's output bytes, in call order."""
    case = order_tablet(n)
    out = []
    for ob in ORDER_COLS:
        dtype = _order_dtype(ORDER_SCHEMA, ob)
        for preds in ([], ORDER_PRED):
            items = order_items(n, preds, ob)
            if not preds:
                assert len(items) == n
            for desc in (False, True):
                for nf in (False, True):
                    full = ordered(items, dtype, desc, nf)
                    E = len(full)
                    for limit in sorted({1, 2, E - 1, E, E + 1, 0}):
                        if limit < 0:
                            continue
                        sel = 0 < limit < E
                        passes = 0 if not sel else \
                            (FULL_DEPTH if cand_one else 1)
                        _r, raw, res = check(
                            run, case, ORDER_READ, preds, ORDER_COLS, ob,
                            full, limit=limit, descending=desc,
                            nulls_first=nf, passes=passes, cap=n + 1)
                        assert res.r.rows_scanned == n
                        out.append(raw_bytes(raw, res, len(ORDER_COLS),
                                             n + 1))
    # an odd window, with and without a limit that needs a selection
    if n >= 8:
        lo, hi = 3, n - 2
        for ob in ((0, 0), (0, 1)):
            items = order_items(n, [], ob)
            for desc in (False, True):
                full = ordered(items, _order_dtype(ORDER_SCHEMA, ob), desc,
                               False, lo, hi)
                assert len(full) == hi - lo
                for limit in (0, 2):
                    _r, raw, res = check(
                        run, case, ORDER_READ, [], ORDER_COLS, ob, full,
                        limit=limit, descending=desc, row_lo=lo, row_hi=hi,
                        cap=n + 1)
                    assert res.r.rows_scanned == hi - lo
                    out.append(raw_bytes(raw, res, len(ORDER_COLS), n + 1))
    # nothing matches
    for limit in (0, 3):
        rows, _raw, res = run(case, ORDER_READ, [ss.NO_ROW], ORDER_COLS,
                              (0, 1), limit=limit)
        assert rows == [] and res.r.n_rows == 0 and res.r.done == 1
        assert res.r.rows_matched == 0 and res.digit_passes == 0
        assert res.r.rows_scanned == n
    return out


def scenario_bits_kept(run):
    """Delivered datums are the rows' own bit patterns: -0.0 stays -0.0 and
    a NaN keeps its sign and payload, although they order as +0.0 / NaN."""
    n = 65
    case = order_tablet(n)
    for desc in (False, True):
        rows, _raw, _res = run(case, ORDER_READ, [], [(0, 1), (0, 3)],
                               (0, 1), descending=desc, cap=n)
        doubles = [r[0] for r in rows]
        assert NEG_ZERO in doubles and 0 in doubles
        assert NEG_NAN_PAYLOAD in doubles
        assert NEG_ZERO_F in [r[1] for r in rows]
        # the zero class and the NaN class are runs in position order
        want = ordered(matching(case, ORDER_READ, [], [(0, 1), (0, 3)],
                                (0, 1)), y.T_DOUBLE, desc, False)
        assert rows == [w[1] for w in want]


def scenario_empty(run):
    case = order_tablet(65)
    for after in (None, (0, 5, 3)):
        rows, _raw, res = run(case, sc.EDGE_READ_BEFORE, [], ORDER_COLS,
                              (0, 0), limit=3, after=after)
        assert rows == [] and res.r.done == 1 and res.digit_passes == 0
        assert res.r.rows_scanned == 0 and res.r.rows_matched == 0
        for lo, hi in ((10, 10), (11, 10), (65, None), (70, 80)):
            rows, _raw, res = run(case, ORDER_READ, [], ORDER_COLS, (0, 0),
                                  limit=3, after=after, row_lo=lo, row_hi=hi)
            assert rows == [] and res.r.done == 1 and res.digit_passes == 0
            assert res.r.rows_scanned == 0 and res.r.rows_matched == 0
    # a cursor at the very end of the order: no eligible row
    full = ordered(order_items(65, [], (0, 1)), y.T_DOUBLE, False, False)
    check(run, case, ORDER_READ, [], ORDER_COLS, (0, 1), full,
          start=len(full), limit=3, passes=0)
    check(run, case, ORDER_READ, [], ORDER_COLS, (0, 1), full,
          start=len(full), limit=0, passes=0)


# ---- 4. paging -------------------------------------------------------------

def page_sizes(E):
    return (1, 7, ss.tile_rows(), E + 1)


def scenario_paging(run, n, ob, desc, nulls_first, page):
    """Concatenated pages equal the unlimited result; the last page is done.
    page=1 puts a cursor on every row: inside runs of equal values, on a NaN,
    on -0.0, on a NULL."""
    case = order_tablet(n)
    full = ordered(order_items(n, [], ob), _order_dtype(ORDER_SCHEMA, ob),
                   desc, nulls_first)
    E = len(full)
    start, pages = 0, 0
    while True:
        _rows, _raw, res = check(run, case, ORDER_READ, [], ORDER_COLS, ob,
                                 full, start=start, limit=page,
                                 descending=desc, nulls_first=nulls_first,
                                 cap=max(page, 1))
        pages += 1
        start += res.r.n_rows
        if res.r.done:
            break
        assert res.r.n_rows == page and pages <= E
    assert start == E and pages == -(-E // page)


# ---- 5. more tiles than the grid -------------------------------------------

def large_rows():
    """(grid cap + 1) tiles and one row: a workgroup walks a second tile."""
    return (ss.GRID_CAP + 1) * ss.tile_rows() + 1


@functools.lru_cache(maxsize=None)
def large_tablet():
    built = y.generate(SCHEMA_4I, rows=large_rows(), seed=23)
    return _case("order_large", SCHEMA_4I, built, [])


def scenario_large(run, cand_one=False):
    case = large_tablet()
    R = 1_700_000_000_000_000
    cols = [(1, 0), (0, 1)]
    preds = [y.Pred(0, 0, y.PRED_LT, (1 << 40) // 100, None, 0)]
    for ob in ((0, 2), (1, 0)):
        items = matching(case, R, preds, cols, ob, pos_is_key=True)
        assert 3_000 < len(items) < 8_000
        # matches past the grid's first round of tiles
        assert items[-1][0] >= ss.GRID_CAP * ss.tile_rows()
        for desc in (False, True):
            full = ordered(items, y.T_INT64, desc, False)
            for limit in (1, 1000):
                _r, _raw, res = check(
                    run, case, R, preds, cols, ob, full, limit=limit,
                    descending=desc,
                    passes=FULL_DEPTH if cand_one else 1)
                assert res.r.rows_scanned == large_rows()
    # a cursor page deep inside the order
    full = ordered(matching(case, R, preds, cols, (0, 2), pos_is_key=True),
                   y.T_INT64, False, False)
    check(run, case, R, preds, cols, (0, 2), full, start=2000, limit=1000)


# ---- 6. string projection --------------------------------------------------

def scenario_strings(run):
    """A string and a numeric column projected from a string-staged snapshot,
    ordered by the numeric column, one string predicate."""
    T = ss.tile_rows()
    for n in (T + 1, 2 * T + 1):
        case = st.edge_tablet(n)
        cols = [(0, 0), (0, 1), (1, 1)]
        preds = [st.str_pred(0, 0, y.PRED_GE, b"0005")]
        items = matching(case, st.READ, preds, cols, (0, 1))
        assert 0 < len(items) < n
        for desc in (False, True):
            full = ordered(items, y.T_INT64, desc, False)
            for start, limit in ((0, 0), (0, 5), (5, T)):
                rows, raw, res = check(
                    run, case, st.READ, preds, cols, (0, 1), full,
                    start=start, limit=limit, descending=desc, strings=True,
                    cap=n, varlen_cap=VCAP)
                heap = st.canonical_heap(case, rows, cols)
                assert st.heap_of(raw) == heap and len(heap) > 0
                for i, row in enumerate(rows):
                    for j, v in enumerate(row):
                        if v is None:
                            assert raw[0][j * n + i] == 0
        # varlen_cap one byte short: code 8 and the size needed
        full = ordered(items, y.T_INT64, True, False)
        rows = [w[1] for w in full]
        need = len(st.canonical_heap(case, rows, cols))
        with pytest.raises(RuntimeError) as ei:
            run(case, st.READ, preds, cols, (0, 1), descending=True,
                strings=True, cap=n, varlen_cap=need - 1)
        assert ei.value.code == 8 and ei.value.varlen_size == need
        assert ei.value.result.r.n_rows == len(full)
        check(run, case, st.READ, preds, cols, (0, 1), full, descending=True,
              strings=True, cap=n, varlen_cap=need)


# ---- 7. errors -------------------------------------------------------------

def error_cases(cases):
    """(label, case, read, run kwargs, message fragment)."""
    mixed = next(c for c in cases if c["name"] == "mixed_types")
    strk = next(c for c in cases if c["name"] == "in_list_string")
    R = 1_700_000_000_000_000
    edge = order_tablet(65)
    E = ORDER_READ
    return [
        ("backward", edge, E, dict(cols=[(0, 0)], order_by=(0, 0),
                                   backward=True), "backward"),
        ("string order column", mixed, R,
         dict(cols=[(0, 0)], order_by=(0, 2)),
         "order column: string column 2"),
        ("string key order column", strk, R,
         dict(cols=[(1, 0)], order_by=(1, 1)),
         "order column: string key column 1"),
        ("order value column out of range", edge, E,
         dict(cols=[(0, 0)], order_by=(0, 6)),
         "order column: value column 6 out of range"),
        ("negative order column", edge, E,
         dict(cols=[(0, 0)], order_by=(0, -1)),
         "order column: value column -1 out of range"),
        ("order key column out of range", edge, E,
         dict(cols=[(0, 0)], order_by=(1, 1)),
         "order column: key column 1 out of range"),
        ("cursor_row 2^32", edge, E,
         dict(cols=[(0, 0)], order_by=(0, 0), after=(0, 0, 1 << 32)),
         "cursor_row 4294967296"),
        ("num_cols 0", edge, E, dict(cols=[], order_by=(0, 0)),
         "num_cols 0"),
        ("projected column out of range", edge, E,
         dict(cols=[(0, 0), (0, 9)], order_by=(0, 0)),
         "column 1: value column 9 out of range"),
        ("predicate column out of range", edge, E,
         dict(cols=[(0, 0)], order_by=(0, 0),
              preds=[y.Pred(0, 9, y.PRED_GT, 0, None, 0)]),
         "predicate 0: value column 9 out of range"),
    ]


def scenario_errors(run, cases, message=False):
    for label, case, read_micros, kw, frag in error_cases(cases):
        kw = dict(kw)
        preds = kw.pop("preds", [])
        cols = kw.pop("cols")
        ob = kw.pop("order_by")
        with pytest.raises(RuntimeError) as ei:
            run(case, read_micros, preds, cols, ob, **kw)
        assert ei.value.code == 9, (label, ei.value.code)
        if message:
            assert frag in str(ei.value), (label, str(ei.value))
        # the snapshot stays usable
        if case["name"].startswith("order_"):
            full = ordered(order_items(65, [], (0, 0)), y.T_INT64, False,
                           False)
            check(run, case, read_micros, [], ORDER_COLS, (0, 0), full,
                  limit=4)
    # cap one short: code 8, the count needed and the counters
    case = order_tablet(65)
    full = ordered(order_items(65, ORDER_PRED, (0, 1)), y.T_DOUBLE, True,
                   False)
    for kw, need in (({}, len(full)), ({"limit": 9}, 9)):
        with pytest.raises(RuntimeError) as ei:
            run(case, ORDER_READ, ORDER_PRED, ORDER_COLS, (0, 1),
                descending=True, cap=need - 1, **kw)
        assert ei.value.code == 8
        r = ei.value.result.r
        assert r.n_rows == need and r.done == 0
        assert r.rows_matched == len(full) and r.rows_scanned == 65
        if message:
            assert "%d rows exceed the output capacity %d" % (
                need, need - 1) in str(ei.value)
        check(run, case, ORDER_READ, ORDER_PRED, ORDER_COLS, (0, 1), full,
              descending=True, limit=kw.get("limit", 0))
