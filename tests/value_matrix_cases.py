"""Tablets, references and scenarios shared by test_value_matrix.py (host
simulators) and test_value_matrix_gpu.py (HIP kernels): what is STORED in a
value, varied over every numeric dtype at the boundaries of its width, on
every decoder — packed V1 and V2 rows, single-value column updates, the fast
kernel's in-loop extraction, the planned kernel's raw loads, row
materialisation, snapshot staging and the KT_INT32 / KT_INT64 key columns.

The reference is the CPU oracle on the same tablet; integers, row sets and
the double results asserted here are bit-equal. Where the oracle could share
a defect with the code under test or is undefined, the reference is plain
Python over the tablet's definition: the FP predicates on the NaN tablets
(scenario_special_fp), the overflowing SUM_INT64 and the -1 / NULL groups.
A scenario takes a
runner (the simulators or the GPU, see the two test files) and returns a
Counter of executed checks per execution path, so that a path that was
silently skipped shows.

A runner provides
  scan_paths(t, preds, aggs)  -> [(path, ScanResult)]
  planned(t, preds, aggs)     -> bool (default dispatch takes the plan)
  row_paths(t)                -> [(path, [(k0, k1, values...)])] in key order,
                                 the columns of select_cols(t)
  group_paths(t, aggs, gcol)  -> [(path, {key: (aggs...)})]
  null_group_paths(t, aggs)   -> [(path, groups, keys, n, null_index)]
where t is a tablet dict of tablet() / special() / group_tablet().

Integer predicates compare SIGNED 64-bit datums ("int compares signed" in
include/yb_gpu_scan.h), so UINT64 values at or above 2^63 compare as
negative on both sides, and MIN/MAX_INT64 order them so. The tests pin that
documented behaviour; they do not change it."""
import collections
import ctypes as C
import functools
import operator
import struct

import ybgpu as y
from parity_cases import make_orcl_spec
from snapshot_group_cases import fold_groups

U64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
READ = 5000
N = 300            # rows of a matrix tablet: 14+ blocks of 1 KiB
BLOCK = 1024
INF = float("inf")
NAN = float("nan")
FLT_MAX = 3.4028234663852886e38
FLT_SUB = 1.401298464324817e-45   # smallest float subnormal
DBL_MAX = 1.7976931348623157e308
DBL_SUB = 5e-324

INT_DTYPES = (y.T_BOOL, y.T_INT8, y.T_INT16, y.T_INT32, y.T_INT64,
              y.T_UINT32, y.T_UINT64)
NAMES = {y.T_BOOL: "bool", y.T_INT8: "int8", y.T_INT16: "int16",
         y.T_INT32: "int32", y.T_INT64: "int64", y.T_UINT32: "uint32",
         y.T_UINT64: "uint64", y.T_FLOAT: "float", y.T_DOUBLE: "double"}
DTYPES = tuple(NAMES)

# stored values and right-hand sides
BOUNDARY = {
    y.T_BOOL: (0, 1),
    y.T_INT8: (-128, -1, 0, 1, 127),
    y.T_INT16: (-32768, -129, -1, 0, 128, 32767),
    y.T_INT32: (-(1 << 31), -32769, -1, 0, 32768, (1 << 31) - 1),
    y.T_INT64: (I64_MIN, -(1 << 31) - 1, -1, 0, 1 << 31, I64_MAX),
    y.T_UINT32: (0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1),
    y.T_UINT64: (0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1),
    y.T_FLOAT: (-INF, -FLT_MAX, -1.5, -0.0, 0.0, FLT_SUB, 1.5, INF),
    y.T_DOUBLE: (-INF, -DBL_MAX, -1.5, -0.0, 0.0, DBL_SUB, 1.5,
                 float((1 << 53) + 2), INF),
}
# right-hand sides only: two values outside the column's width (the 64-bit
# dtypes have none; the FP dtypes take two finite values not stored)
OUTSIDE = {
    y.T_BOOL: (2, -1),
    y.T_INT8: (300, -(1 << 40)),
    y.T_INT16: (70000, -(1 << 40)),
    y.T_INT32: (1 << 31, -(1 << 40)),
    y.T_INT64: (),
    y.T_UINT32: (1 << 32, -1),
    y.T_UINT64: (),
    y.T_FLOAT: (FLT_MAX, -FLT_SUB),
    y.T_DOUBLE: (DBL_MAX, -DBL_SUB),
}
RANGE_KEYS = (-(1 << 31), -1, 0, 1, (1 << 31) - 1)
OPS = (y.PRED_GT, y.PRED_GE, y.PRED_LT, y.PRED_LE, y.PRED_EQ, y.PRED_NE)

_KEEP = []


def bits(dt, v):
    """The 64-bit datum pattern of v in a column (or right-hand side) of
    dtype dt."""
    if dt == y.T_DOUBLE:
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    if dt == y.T_FLOAT:
        return struct.unpack("<I", struct.pack("<f", v))[0]
    return v & U64


def _steady(r, n):
    """The third quarter of the rows: no column updates, no NULLs, and keys
    that differ in the last key column only. The fast kernel takes entries
    whose key changes within 16 bytes before the hybrid time and whose
    headers carry no delta widths, so it keeps these batches; it hands the
    others (see tablet()) to the general kernel."""
    return n // 2 <= r < n - n // 4


def hashed_key(r, n):
    """The KT_INT64 key of row r of n: ascending, both extremes included."""
    if r == 0:
        return I64_MIN
    if r == 1:
        return -(1 << 40)
    if r == n - 2:
        return 1 << 40
    if r == n - 1:
        return I64_MAX
    if _steady(r, n):
        return 0
    return r - n // 2


def range_key(r, n):
    """The KT_INT32 key of row r of n: cycles through the extremes; in the
    steady quarter it counts up across zero under one hashed key."""
    if _steady(r, n):
        return r - n // 2 - 30
    return RANGE_KEYS[r % len(RANGE_KEYS)]


def _build(name, col_types, rows, value_fn, pv, updates=None,
           block_size=BLOCK):
    """Tablet dict. Schema: hashed KT_INT64 key + KT_INT32 range key; value
    column 0 of col_types[0], the others INT64. value_fn(r) -> the row's
    values (None = NULL); updates(r) -> a later value of column 0 or
    nothing."""
    schema = y.make_schema([y.KT_INT64, y.KT_INT32],
                           [(10 + i, t, 1) for i, t in enumerate(col_types)])
    b = y.Builder(schema, block_size=block_size)
    for r in range(rows):
        kw = dict(hash_=r // 64,
                  key_datums=(hashed_key(r, rows), range_key(r, rows)))
        b.add_packed_row(1000, list(zip(col_types, value_fn(r))),
                         packed_version=pv, **kw)
        if updates is not None:
            u = updates(r)
            if u is not None:
                b.add_column_update(2000, 0, u[0], **kw)
    data, offsets, nb, total, _ = b.finish()
    _KEEP.append(b)
    return {"name": name, "schema": schema, "data": data, "offsets": offsets,
            "n_blocks": nb, "total": total, "rows": rows, "pv": pv,
            "kv_format": y.ENC_THREE_SHARED_PARTS}


def _nulls_last_quarter(r, n, v):
    """NULLs only in the last quarter: the fast kernel hands a batch with a
    null mask to the general kernel, the batches before stay on it."""
    return None if (r >= n - n // 4 and r % 3 == 0) else v


@functools.lru_cache(maxsize=None)
def tablet(dt, pv):
    """The matrix tablet of (dtype, packed version): column 0 cycles
    through the dtype's boundary values, column 1 is the row number. Every
    third row of the first half has a later column update of column 0 to
    the next boundary value (the single-value V1 decoder)."""
    vals = BOUNDARY[dt]

    def value_fn(r):
        return (_nulls_last_quarter(r, N, vals[r % len(vals)]), r)

    def updates(r):
        if r < N // 2 and r % 3 == 0:
            return (vals[(r + 1) % len(vals)],)
        return None

    t = _build("%s_v%d" % (NAMES[dt], pv), (dt, y.T_INT64), N, value_fn, pv,
               updates)
    assert t["n_blocks"] >= 8, t["n_blocks"]
    return t


def _quarters(r):
    return ((r * 7919) % 100003 - 50000) * 0.25


SPECIAL_ROWS = 240
SPECIALS = {
    # name: (dtype of column 0, values it cycles through)
    "double_nan": (y.T_DOUBLE, BOUNDARY[y.T_DOUBLE] + (NAN, -NAN)),
    "float_nan": (y.T_FLOAT, BOUNDARY[y.T_FLOAT] + (NAN, -NAN)),
    # every partial sum of multiples of 0.25 below 2^50 is exact in any order
    "double_sum": (y.T_DOUBLE, None),
    # one sign of zero only: MIN/MAX are then independent of the fold order
    "double_minmax": (y.T_DOUBLE, (-INF, -DBL_MAX, -1.5, -DBL_SUB, DBL_SUB,
                                   2.2250738585072014e-308, 1.5,
                                   float((1 << 53) + 2), DBL_MAX, INF)),
    "double_zeros": (y.T_DOUBLE, (0.0, -0.0, -0.0, 0.0, 0.0)),
    # SUM_INT64 over this column leaves the int64 range within two rows
    "int64_wrap": (y.T_INT64, (I64_MAX, I64_MAX, I64_MIN, I64_MAX, 1)),
}


@functools.lru_cache(maxsize=None)
def special(name):
    """Three value columns: column 0 as SPECIALS names it, column 1 the row
    number, column 2 the row number modulo 4 (the group column)."""
    dt, vals = SPECIALS[name]

    def value_fn(r):
        v = _quarters(r) if vals is None else vals[r % len(vals)]
        return (_nulls_last_quarter(r, SPECIAL_ROWS, v), r, r % 4)

    t = _build(name, (dt, y.T_INT64, y.T_INT64), SPECIAL_ROWS, value_fn, 2)
    t["values"] = [value_fn(r)[0] for r in range(SPECIAL_ROWS)]
    return t


GROUP_TABLETS = {
    # name: (group column dtype, its values by row % len, rows)
    "minus1_null_int64": (y.T_INT64, (-1, None, 0, 7, -1), 500),
    "minus1_null_int32": (y.T_INT32, (-1, None, 0, 7, -1), 500),
    "minus1_null_int8": (y.T_INT8, (-1, None, 0, 7, -1), 500),
    "minus1_no_null": (y.T_INT64, (-1, 0, 7), 300),
    "null_only": (y.T_INT64, (None,), 200),
}


@functools.lru_cache(maxsize=None)
def group_tablet(name):
    dt, vals, rows = GROUP_TABLETS[name]
    return _build(name, (dt, y.T_INT64), rows,
                  lambda r: (vals[r % len(vals)], r), 2)


# ---- specs and references --------------------------------------------------

def pred(t, op, v, col=0):
    """Compare predicate on value column col against v."""
    dt = t["schema"].value_cols[col].dtype
    return y.Pred(0, col, op, bits(dt, v), None, 0)


def key_pred(col, op, v):
    return y.Pred(1, col, op, v & U64, None, 0)


def in_pred(t, options, col=0):
    dt = t["schema"].value_cols[col].dtype
    raw = struct.pack("<%dQ" % len(options), *[bits(dt, o) for o in options])
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    _KEEP.append(buf)
    return y.Pred(0, col, y.PRED_IN, 0, buf, len(raw))


def range_pred(t, ranges, col=0):
    """ranges: (lo, hi, lo inclusive, hi inclusive)."""
    dt = t["schema"].value_cols[col].dtype
    raw = b"".join(struct.pack("<QQII", bits(dt, lo), bits(dt, hi),
                               (1 if li else 0) | (2 if hi_ else 0), 0)
                   for lo, hi, li, hi_ in ranges)
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    _KEEP.append(buf)
    return y.Pred(0, col, y.PRED_IN_RANGE, 0, buf, len(raw))


def make_spec(t, preds=(), aggs=(), group_col=None):
    spec = y.ScanSpec()
    spec.schema = t["schema"]
    spec.kv_format = t["kv_format"]
    spec.read_time = y.read_time(READ)
    spec.num_preds = len(preds)
    for i, p in enumerate(preds):
        spec.preds[i] = p
    spec.num_aggs = len(aggs)
    for i, a in enumerate(aggs):
        spec.aggs[i] = a
    if group_col is not None:
        spec.group_col = group_col + 1
    return spec


def oracle_scan(t, preds=(), aggs=(), collect_rows=False):
    return y.orcl_scan(t["data"], t["offsets"], t["n_blocks"],
                       y.orcl_schema_from(t["schema"]),
                       make_orcl_spec(READ, preds, aggs),
                       collect_rows=collect_rows)


def oracle_groups(t, aggs, gcol, raw=False):
    return y.orcl_group(t["data"], t["offsets"], t["n_blocks"],
                        y.orcl_schema_from(t["schema"]),
                        make_orcl_spec(READ, (), aggs), gcol, raw=raw,
                        cap=1 << 10, key_bytes_cap=1 << 10)


@functools.lru_cache(maxsize=None)
def oracle_rows(t_key):
    """The oracle's rows of a tablet as (k0, k1, values...) in key order,
    computed once. t_key: ("tablet", dt, pv) or ("special", name)."""
    t = tablet(*t_key[1:]) if t_key[0] == "tablet" else special(t_key[1])
    _, rows = oracle_scan(t, collect_rows=True)
    return tuple(kd + vals for kd, vals in rows)


DOUBLE_OPS = (y.AGG_SUM_DOUBLE, y.AGG_MIN_DOUBLE, y.AGG_MAX_DOUBLE)


def norm(res, aggs, f64_as_value=False):
    """(rows_scanned, rows_matched, ((is_null, value)...)): integers as
    they are, doubles as their bit pattern (or as floats, to compare with
    ==, when f64_as_value)."""
    out = []
    for i, a in enumerate(aggs):
        r = res.aggs[i]
        if r.is_null:
            out.append((1, None))
        elif a.op in DOUBLE_OPS:
            out.append((0, r.value_f64 if f64_as_value
                        else bits(y.T_DOUBLE, r.value_f64)))
        else:
            out.append((0, r.value_i64))
    return (res.rows_scanned, res.rows_matched, tuple(out))


def _check_scans(runner, t, queries, counts, f64_as_value=False,
                 want_fn=None):
    """Every path of every (label, preds, aggs) equals the oracle."""
    for label, preds, aggs in queries:
        if want_fn is None:
            ores, _ = oracle_scan(t, preds, aggs)
            want = norm(ores, aggs, f64_as_value)
        else:
            want = want_fn(label, preds, aggs)
        for path, res in runner.scan_paths(t, preds, aggs):
            got = norm(res, aggs, f64_as_value)
            assert got == want, (t["name"], label, path, got, want)
            counts[path] += 1


# ---- scenarios -------------------------------------------------------------

def compare_queries(dt, pv):
    """Scenario 1's queries: six ops times every right-hand side, one IN
    list and two IN_RANGE with negative and boundary options and both kinds
    of ends."""
    t = tablet(dt, pv)
    vals = BOUNDARY[dt]
    star, cnt, sum1 = (y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 0),
                       y.Agg(y.AGG_SUM_INT64, 1))
    aggs = [star, cnt, sum1]
    pairs = [[star, sum1], [cnt, star]]
    if dt in INT_DTYPES:
        mn, mx = y.Agg(y.AGG_MIN_INT64, 0), y.Agg(y.AGG_MAX_INT64, 0)
        aggs += [mn, mx]
        pairs = [[star, sum1], [cnt, mn], [mx, sum1]]
    out = []
    for v in vals + OUTSIDE[dt]:
        for op in OPS:
            # every aggregate at once (general and snapshot paths), and two
            # at a time, which is what the fast kernel takes
            out.append(("op%d %r" % (op, v), [pred(t, op, v)],
                        aggs))
            out.append(("op%d %r pair" % (op, v),
                        [pred(t, op, v)], pairs[len(out) // 2 % len(pairs)]))
    out.append(("in", [in_pred(t, (vals[0], vals[1], vals[-1])
                               + OUTSIDE[dt][:1])], aggs))
    lo, mid, hi = vals[0], vals[len(vals) // 2], vals[-1]
    out.append(("in_range", [range_pred(
        t, ((lo, vals[1], True, False), (mid, hi, False, True)))], aggs))
    out.append(("in_range_open", [range_pred(
        t, ((lo, mid, False, False), (hi, hi, True, True)))], aggs))
    return out


def scenario_compare(runner, dt, pv):
    counts = collections.Counter()
    _check_scans(runner, tablet(dt, pv), compare_queries(dt, pv), counts)
    return counts


def key_queries(t):
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 1)]
    out = []
    for v in (I64_MIN, -(1 << 40), -1, 0, 1 << 40, I64_MAX):
        for op in OPS:
            out.append(("k0 op%d %d" % (op, v), [key_pred(0, op, v)], aggs))
    # the last two are outside the KT_INT32 column's width
    for v in RANGE_KEYS + (1 << 31, -(1 << 31) - 1):
        for op in OPS:
            out.append(("k1 op%d %d" % (op, v), [key_pred(1, op, v)], aggs))
    return out


def scenario_keys(runner, pv):
    counts = collections.Counter()
    t = tablet(y.T_INT64, pv)
    _check_scans(runner, t, key_queries(t), counts)
    return counts


def select_cols(t):
    """Both key columns, then every value column."""
    return ((1, 0), (1, 1)) + tuple(
        (0, c) for c in range(t["schema"].num_value_cols))


def scenario_rows(runner, t_key):
    """Every column of every row, NULL masks included; values are datum
    bit patterns, so a NaN's payload and a zero's sign count. t_key as for
    oracle_rows."""
    counts = collections.Counter()
    t = tablet(*t_key[1:]) if t_key[0] == "tablet" else special(t_key[1])
    want = list(oracle_rows(t_key))
    assert len(want) == t["rows"]
    for path, rows in runner.row_paths(t):
        assert len(rows) == len(want), (path, len(rows))
        for g, w in zip(rows, want):
            assert tuple(g) == w, (t["name"], path, g, w)
        counts[path] += 1
    return counts


FP_SPECIAL_RHS = (NAN, 0.0, -0.0, INF, -INF, 1.5)
PY_OPS = {y.PRED_GT: operator.gt, y.PRED_GE: operator.ge,
          y.PRED_LT: operator.lt, y.PRED_LE: operator.le,
          y.PRED_EQ: operator.eq, y.PRED_NE: operator.ne}


def special_fp_queries(name):
    """(label, preds, aggs, (op, right-hand side))."""
    t = special(name)
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 0)]
    return [("op%d %r" % (op, v), [pred(t, op, v)], aggs, (op, v))
            for v in FP_SPECIAL_RHS for op in OPS]


def _stored(dt, v):
    """v as a column of dtype dt holds it (FLOAT rounds to 32 bits)."""
    return struct.unpack("<f", struct.pack("<f", v))[0] \
        if dt == y.T_FLOAT else v


def scenario_special_fp(runner, name):
    """Compares against NaN, signed zeros, infinities and a plain number on
    a column that holds NaN too; COUNT only. The reference is Python's float
    compare over the tablet's values, which is IEEE 754's (a NaN on either
    side fails every op but NE) and shares no code with the oracle; the
    oracle is checked against it like every other path."""
    counts = collections.Counter()
    t = special(name)
    dt = SPECIALS[name][0]
    vals = [_stored(dt, v) for v in t["values"] if v is not None]
    queries = special_fp_queries(name)
    want = {}
    for label, _preds, _aggs, (op, rhs) in queries:
        m = sum(1 for v in vals if PY_OPS[op](v, _stored(dt, rhs)))
        cnt = (0, m) if m else (1, None)
        want[label] = (SPECIAL_ROWS, m, (cnt, cnt))
    # a NaN row equals no number, and only the 1.5 rows equal 1.5
    assert want["op%d %r" % (y.PRED_EQ, NAN)][1] == 0
    assert want["op%d %r" % (y.PRED_NE, NAN)][1] == len(vals)
    assert want["op%d %r" % (y.PRED_EQ, 1.5)][1] == vals.count(1.5) > 0
    for label, preds, aggs, _ in queries:
        got = norm(oracle_scan(t, preds, aggs)[0], aggs)
        assert got == want[label], (name, label, "oracle", got, want[label])
        counts["oracle"] += 1
    _check_scans(runner, t, [q[:3] for q in queries], counts,
                 want_fn=lambda label, _p, _a: want[label])
    return counts


def _group_bits(row):
    """A group's aggregates with doubles as bit patterns."""
    return tuple(bits(y.T_DOUBLE, v) if isinstance(v, float) else v
                 for v in row)


def scenario_double_aggs(runner):
    """SUM / MIN / MAX_DOUBLE where they do not depend on the fold order:
    bit-equal to the oracle, plain and grouped; over +0.0 and -0.0 equal
    with ==, sign not asserted."""
    counts = collections.Counter()
    cases = (("double_sum", [y.AGG_SUM_DOUBLE], False),
             ("double_minmax", [y.AGG_MIN_DOUBLE, y.AGG_MAX_DOUBLE], False),
             ("double_zeros", [y.AGG_MIN_DOUBLE, y.AGG_MAX_DOUBLE], True))
    for name, ops, by_value in cases:
        t = special(name)
        # two aggregates: the fast kernel's cap
        aggs = [y.Agg(op, 0) for op in ops] + \
            [y.Agg(y.AGG_COUNT, 0)] * (2 - len(ops))
        queries = [("all", [], aggs),
                   ("row_ge_100", [pred(t, y.PRED_GE, 100, col=1)], aggs)]
        _check_scans(runner, t, queries, counts, f64_as_value=by_value)
        want = oracle_groups(t, aggs, 2)
        assert len(want) == 4
        for path, got in runner.group_paths(t, aggs, 2):
            assert set(got) == set(want), (name, path)
            for k, wv in want.items():
                if by_value:
                    assert got[k] == wv, (name, path, k, got[k], wv)
                else:
                    assert _group_bits(got[k]) == _group_bits(wv), \
                        (name, path, k, got[k], wv)
            counts["group:" + path] += 1
    return counts


def planned_extreme_queries(dt):
    """The plan compiler's edge branches at the ends of the int64 range."""
    t = tablet(dt, 2)
    aggs = [y.Agg(y.AGG_SUM_INT64, 1), y.Agg(y.AGG_COUNT_STAR, 0)]

    def p(op, v):
        return y.Pred(0, 0, op, v & U64, None, 0)

    return [("gt_max", [p(y.PRED_GT, I64_MAX)], aggs, 0),
            ("lt_min", [p(y.PRED_LT, I64_MIN)], aggs, 0),
            ("ge_min", [p(y.PRED_GE, I64_MIN)], aggs, None),
            ("le_max", [p(y.PRED_LE, I64_MAX)], aggs, None),
            ("eq_min", [p(y.PRED_EQ, I64_MIN)], aggs, None),
            ("eq_max", [p(y.PRED_EQ, I64_MAX)], aggs, None),
            ("crossed", [p(y.PRED_GT, 5), p(y.PRED_LT, 5)], aggs, 0),
            ("crossed_at_ends", [p(y.PRED_GE, I64_MAX), p(y.PRED_LE, I64_MIN)],
             aggs, 0)], t


def scenario_planned_extremes(runner, dt):
    counts = collections.Counter()
    queries, t = planned_extreme_queries(dt)
    for label, preds, aggs, matched in queries:
        assert runner.planned(t, preds, aggs), (NAMES[dt], label)
        if matched is not None:
            assert oracle_scan(t, preds, aggs)[0].rows_matched == matched
    _check_scans(runner, t, [q[:3] for q in queries], counts)
    # the all-rows and the extreme-value cases do match rows
    assert oracle_scan(t, *queries[2][1:3])[0].rows_matched > N // 2
    assert oracle_scan(t, *queries[4][1:3])[0].rows_matched > 0
    return counts


def _wrap(total):
    total &= U64
    return total - (1 << 64) if total >> 63 else total


def scenario_sum_wrap(runner):
    """SUM_INT64 past the int64 range wraps modulo 2^64 on every path. The
    reference is Python's sum: the oracle's signed += is undefined there."""
    counts = collections.Counter()
    t = special("int64_wrap")
    aggs = [y.Agg(y.AGG_SUM_INT64, 0), y.Agg(y.AGG_COUNT, 0)]
    vals = t["values"]

    def want_fn(label, preds, _aggs):
        sel = [v for r, v in enumerate(vals)
               if v is not None and (label == "all" or r >= 100)]
        n_rows = SPECIAL_ROWS if label == "all" else SPECIAL_ROWS - 100
        return (SPECIAL_ROWS, n_rows, ((0, _wrap(sum(sel))), (0, len(sel))))

    true_sum = sum(v for v in vals if v is not None)
    assert not I64_MIN <= true_sum <= I64_MAX  # the case does overflow
    queries = [("all", [], aggs),
               ("row_ge_100", [pred(t, y.PRED_GE, 100, col=1)], aggs)]
    _check_scans(runner, t, queries, counts, want_fn=want_fn)
    want = {}
    for r, v in enumerate(vals):
        if v is not None:
            s, c = want.get(r % 4, (0, 0))
            want[r % 4] = (_wrap(s + v), c + 1)
    for path, got in runner.group_paths(t, aggs, 2):
        assert got == want, (path, got, want)
        counts["group:" + path] += 1
    return counts


def scenario_null_group(runner, name):
    """Block-path GROUP BY keeps the NULL group apart from the group of an
    integer -1 (same 64-bit key): groups equal a Python fold over the
    oracle's rows, and the reported index names the NULL entry."""
    counts = collections.Counter()
    t = group_tablet(name)
    _, vals, rows = GROUP_TABLETS[name]
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 1)]
    want, n_rows = fold_groups(t, READ, (), aggs, 0, False)
    assert n_rows == rows
    assert len(want) == len(set(vals))
    if name.startswith("minus1_null"):
        assert sorted(v[0] for v in want.values()) == [100, 100, 100, 200]
        assert want[U64][0] == 200 and want[None][0] == 100
    has_null = None in vals
    for path, got, keys, n, null_index in runner.null_group_paths(t, aggs):
        assert got == want, (name, path, got, want)
        assert n == len(want), (name, path, n)
        if has_null:
            assert 0 <= null_index < n and keys[null_index] == U64, \
                (name, path, null_index)
        else:
            assert null_index == -1, (name, path, null_index)
        # every other all-ones key is the group of -1
        ones = [g for g in range(n) if keys[g] == U64 and g != null_index]
        assert len(ones) == (1 if -1 in vals else 0), (name, path, ones)
        counts[path] += 1
    return counts
