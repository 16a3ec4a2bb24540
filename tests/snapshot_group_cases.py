"""Shared pieces of the grouped columnar-snapshot tests
(test_snapshot_group_sim.py on the CPU simulator, test_snapshot_group_gpu.py
on the HIP kernels): the tablets, the queries, the references (orcl_group for
value-column grouping, a Python fold over the oracle's matching rows for
everything it cannot express) and the comparisons."""
import functools
import math
import struct

import ybgpu as y
from parity_cases import SCHEMA_4I, _case, make_orcl_spec
import snapshot_cases as sc

READ = 1_700_000_000_000_000   # after every write of the tablets below
U64 = (1 << 64) - 1
CAP = 1 << 12                  # output capacity of the small cases

_KEEP = []


def local_slots(num_aggs):
    """L: the local-table slot count, always asked of the library."""
    return y.snapshot_group_local_slots(num_aggs)


def levels(num_aggs):
    """(expect_groups hint, level it must select): forced two-level, forced
    global-only."""
    return ((1, 1), (local_slots(num_aggs) + 1, 0))


# ---- references ------------------------------------------------------------

def oracle_groups(case, read_micros, preds, aggs, group_col):
    """orcl_group on a VALUE column."""
    osc = y.orcl_schema_from(case["schema"])
    ospec = make_orcl_spec(read_micros, preds, aggs)
    return y.orcl_group(case["data"], case["offsets"], case["n_blocks"], osc,
                        ospec, group_col, kv_format=case["kv_format"])


def _i64(u):
    return u - (1 << 64) if u >> 63 else u


def _f64(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def fold_groups(case, read_micros, preds, aggs, group_col, group_is_key):
    """Python fold over the rows the oracle scan returns for (preds): the
    reference for key-column grouping and, independent of orcl_group, for
    groups whose key is 2**64 - 1 next to a NULL group. Returns ({key: (aggs...)}, rows
    matched); key = the datum as unsigned 64-bit, None for the NULL group."""
    osc = y.orcl_schema_from(case["schema"])
    ospec = make_orcl_spec(read_micros, preds, ())
    _res, rows = y.orcl_scan(case["data"], case["offsets"], case["n_blocks"],
                             osc, ospec, kv_format=case["kv_format"],
                             collect_rows=True)
    acc = {}
    for kd, vals in rows:
        k = kd[group_col] if group_is_key else vals[group_col]
        st = acc.setdefault(k, [[None, 0] for _ in aggs])
        for (v_c, a) in zip(st, aggs):
            if a.op == y.AGG_COUNT_STAR:
                v_c[0] = (v_c[0] or 0) + 1
                v_c[1] += 1
                continue
            d = vals[a.col]
            if d is None:
                continue
            v_c[1] += 1
            if a.op == y.AGG_COUNT:
                v_c[0] = (v_c[0] or 0) + 1
            elif a.op == y.AGG_SUM_INT64:
                s = (v_c[0] or 0) + _i64(d)
                v_c[0] = _i64(s & U64)
            elif a.op == y.AGG_SUM_DOUBLE:
                v_c[0] = (v_c[0] or 0.0) + _f64(d)
            elif a.op == y.AGG_MIN_INT64:
                v_c[0] = _i64(d) if v_c[0] is None else min(v_c[0], _i64(d))
            elif a.op == y.AGG_MAX_INT64:
                v_c[0] = _i64(d) if v_c[0] is None else max(v_c[0], _i64(d))
            elif a.op == y.AGG_MIN_DOUBLE:
                v_c[0] = _f64(d) if v_c[0] is None else min(v_c[0], _f64(d))
            elif a.op == y.AGG_MAX_DOUBLE:
                v_c[0] = _f64(d) if v_c[0] is None else max(v_c[0], _f64(d))
    out = {k: tuple(v if c else None for v, c in st)
           for k, st in acc.items()}
    return out, len(rows)


# ---- comparisons -----------------------------------------------------------

def check_groups(got, want, aggs, f64_rel=1e-9):
    """Key set, integer aggregates, counts (NULL-ness) and double MIN/MAX
    exact; double SUM within 1e-9 relative (test_group_parity.py's bar)."""
    assert set(got.keys()) == set(want.keys()), \
        (len(got), len(want), sorted(set(got) ^ set(want), key=str)[:8])
    for k, wv in want.items():
        gv = got[k]
        for a, ag in enumerate(aggs):
            if wv[a] is None or gv[a] is None:
                assert wv[a] is None and gv[a] is None, (k, a, gv[a], wv[a])
            elif ag.op == y.AGG_SUM_DOUBLE:
                if math.isnan(wv[a]) or math.isnan(gv[a]):
                    assert math.isnan(wv[a]) and math.isnan(gv[a]), (k, a)
                else:
                    assert abs(gv[a] - wv[a]) <= \
                        f64_rel * max(1.0, abs(wv[a])), (k, a, gv[a], wv[a])
            else:
                assert gv[a] == wv[a], (k, a, gv[a], wv[a])


def check_order(keys, res):
    """Keys strictly ascending as unsigned 64-bit, the NULL group last with
    key 0."""
    n = res.n_groups - (1 if res.has_null_group else 0)
    ks = [keys[i] for i in range(n)]
    assert all(a < b for a, b in zip(ks, ks[1:])), "keys not ascending"
    if res.has_null_group:
        assert keys[res.n_groups - 1] == 0


def raw_bytes(keys, vals, cnts, res):
    """The written part of the three output arrays, as bytes."""
    n = res.n_groups
    return (bytes(memoryview(keys).cast("B")[:n * 8]),
            bytes(memoryview(vals).cast("B")[:n * 8 * y.MAX_AGGS]),
            bytes(memoryview(cnts).cast("B")[:n * 8 * y.MAX_AGGS]))


def same_bits(a, b):
    """Two decoded group dicts equal bit for bit (NaN == NaN)."""
    def bits(v):
        return struct.pack("<d", v) if isinstance(v, float) else v
    return ({k: tuple(bits(v) for v in t) for k, t in a.items()} ==
            {k: tuple(bits(v) for v in t) for k, t in b.items()})


# ---- queries ---------------------------------------------------------------

def aggs2():
    return [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 1)]


def aggs8():
    """All eight ops over the (int64 group, int64, double) tablets."""
    return [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 2),
            y.Agg(y.AGG_SUM_INT64, 1), y.Agg(y.AGG_SUM_DOUBLE, 2),
            y.Agg(y.AGG_MIN_INT64, 1), y.Agg(y.AGG_MAX_INT64, 1),
            y.Agg(y.AGG_MIN_DOUBLE, 2), y.Agg(y.AGG_MAX_DOUBLE, 2)]


# ---- tablets ---------------------------------------------------------------

CARD_SCHEMA = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_INT64, 1), (12, y.T_DOUBLE, 1)])
CARD_ROWS = 1025   # 3 workgroups of 512 rows: one group is flushed by several


def cardinality_rows(n_groups):
    """1025 rows, or as many as the cardinality needs: 4 * L distinct
    groups at 2 aggregates (L = 512) do not fit 1025 rows."""
    return max(CARD_ROWS, n_groups)


@functools.lru_cache(maxsize=None)
def cardinality_tablet(n_groups):
    """cardinality_rows(n_groups) rows in exactly n_groups groups: group
    key (r % n_groups) * 7919 - 3 (row r of every workgroup's range hits
    every group when n_groups is small), int64 r * 3 - 500, double
    r * 0.25 - 7, NULL on every 5th row."""
    n = cardinality_rows(n_groups)
    b = y.Builder(CARD_SCHEMA)
    for r in range(n):
        dv = None if r % 5 == 0 else r * 0.25 - 7
        b.add_packed_row(1000 + r,
                         [(y.T_INT64, (r % n_groups) * 7919 - 3),
                          (y.T_INT64, r * 3 - 500), (y.T_DOUBLE, dv)],
                         hash_=r // 64, key_datums=(r,))
    _KEEP.append(b)
    return _case("card_%d" % n_groups, CARD_SCHEMA, b.finish(), [])


def grid_stride_rows():
    """kSnapMaxGrid x 512 + 513 rows with the shipped grid cap of 1024:
    every lane of the first workgroups makes a second trip."""
    return 1024 * 512 + 513


@functools.lru_cache(maxsize=None)
def grid_stride_tablet():
    built = y.generate(SCHEMA_4I, rows=grid_stride_rows(), seed=7,
                       group_mod=97)
    return _case("grid_stride", SCHEMA_4I, built, [])


KIND_SCHEMA = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_DOUBLE, 1), (12, y.T_INT32, 1),
     (13, y.T_BOOL, 1), (14, y.T_INT64, 1)])
KIND_ROWS = 257


@functools.lru_cache(maxsize=None)
def kinds_tablet():
    """257 rows. col 0: int64 in {-1, -5, 0, 3, 2**40} and NULL on every
    7th row (a -1 key next to the NULL group); col 1: double in {-2.5, 0.0,
    1e10, 7.25}; col 2: int32 in {-3 .. 3}; col 3: bool; col 4: int64 r."""
    b = y.Builder(KIND_SCHEMA)
    ints = (-1, -5, 0, 3, 1 << 40)
    dbls = (-2.5, 0.0, 1e10, 7.25)
    for r in range(KIND_ROWS):
        b.add_packed_row(
            1000 + r,
            [(y.T_INT64, None if r % 7 == 0 else ints[r % 5]),
             (y.T_DOUBLE, dbls[r % 4]), (y.T_INT32, r % 7 - 3),
             (y.T_BOOL, r % 2), (y.T_INT64, r)],
            hash_=r // 64, key_datums=(r,))
    _KEEP.append(b)
    return _case("kinds", KIND_SCHEMA, b.finish(), [])


def kinds_aggs():
    return [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 4),
            y.Agg(y.AGG_MAX_DOUBLE, 1), y.Agg(y.AGG_COUNT, 0)]


def gen_preds():
    """One IN and one IN_RANGE predicate on the kinds tablet (the general
    compare instantiation): int32 col in {-3, 0, 2}, col 4 in [10, 200]."""
    blob = b"".join(struct.pack("<q", v) for v in (-3, 0, 2))
    buf = (y.C.c_uint8 * len(blob)).from_buffer_copy(blob)
    rng = struct.pack("<qqq", 10, 200, 3)   # [lo, hi], both inclusive
    rbuf = (y.C.c_uint8 * len(rng)).from_buffer_copy(rng)
    _KEEP.extend([buf, rbuf])
    return [y.Pred(0, 2, y.PRED_IN, 0, buf, len(blob)),
            y.Pred(0, 4, y.PRED_IN_RANGE, 0, rbuf, len(rng))]


DBL_SCHEMA = y.make_schema([y.KT_INT64],
                           [(10, y.T_INT64, 1), (11, y.T_DOUBLE, 1)])


@functools.lru_cache(maxsize=None)
def doubles_tablet():
    """test_group_parity.py's _dataset_doubles shape: 20000 rows in 97
    groups, doubles uniform in +-1e6, one hybrid time."""
    import random
    b = y.Builder(DBL_SCHEMA)
    seq = 1 << 50
    rng = random.Random(777)
    for r in range(20000):
        seq += 1
        b.add_packed_row(1000, [(y.T_INT64, r % 97),
                                (y.T_DOUBLE, rng.uniform(-1e6, 1e6))],
                         hash_=r // 512, key_datums=(r,), seq=seq)
    _KEEP.append(b)
    return _case("doubles", DBL_SCHEMA, b.finish(), [])


def doubles_aggs():
    return [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_MIN_DOUBLE, 1),
            y.Agg(y.AGG_MAX_DOUBLE, 1), y.Agg(y.AGG_SUM_DOUBLE, 1)]


@functools.lru_cache(maxsize=None)
def poison_tablet():
    """Group 0 holds a 1e30 (outside the fixed-point range) next to
    ordinary values; groups 1 and 2 hold ordinary values only."""
    b = y.Builder(DBL_SCHEMA)
    seq = 1 << 50
    for r in range(300):
        seq += 1
        dv = 1e30 if r == 150 else r * 0.5
        b.add_packed_row(1000, [(y.T_INT64, r % 3), (y.T_DOUBLE, dv)],
                         hash_=r // 64, key_datums=(r,), seq=seq)
    _KEEP.append(b)
    return _case("poison", DBL_SCHEMA, b.finish(), [])


@functools.lru_cache(maxsize=None)
def edge_tablet(n, nulls=True):
    return sc.edge_tablet(n, nulls=nulls)


def block_spec(case, read_micros, preds, aggs, group_col):
    """The block path's (and ybg_sim_group's) spec for the same query on a
    value column."""
    from parity_cases import make_spec
    spec = make_spec(case, read_micros, preds, aggs)
    spec.group_col = group_col + 1
    return spec


STR_SCHEMA = y.make_schema(
    [y.KT_INT64, y.KT_STRING],
    [(10, y.T_INT64, 1), (11, y.T_STRING, 1), (12, y.T_INT64, 1)],
    num_hash_cols=1)


@functools.lru_cache(maxsize=None)
def string_tablet():
    """50 rows with a string value column and a string range-key column:
    what a grouped snapshot query must refuse to group on."""
    b = y.Builder(STR_SCHEMA)
    for r in range(50):
        b.add_packed_row(1000 + r,
                         [(y.T_INT64, r % 4), (y.T_STRING, b"s%d" % (r % 3)),
                          (y.T_INT64, r)],
                         hash_=0, key_datums=(r,), key_strs=(None, b"k"))
    _KEEP.append(b)
    return _case("strings", STR_SCHEMA, b.finish(), [])


# ---- scenarios -------------------------------------------------------------
# `run(case, read_micros, preds, aggs, group_col, group_is_key=False,
#      expect_groups=0, cap=CAP)` answers one grouped query on the case's
# snapshot — the simulator in test_snapshot_group_sim.py, the HIP kernels in
# test_snapshot_group_gpu.py — and returns (groups dict, (keys, vals, cnts),
# result struct); a non-zero code raises with .code and .result.

def _matched(want):
    """rows matched = sum of the COUNT(*) in aggregate slot 0."""
    return sum(v[0] for v in want.values())


def check_both_levels(run, case, read_micros, preds, aggs, group_col, want,
                      group_is_key=False, hints=None, n_rows=None):
    """The query at every hint in `hints` ((hint, expected level) pairs;
    default: forced two-level and forced global-only) against `want`, with
    the level, the counters and the order checked, and the raw output
    byte-identical across the levels."""
    raws = []
    for hint, level in (hints or levels(len(aggs))):
        got, raw, res = run(case, read_micros, preds, aggs, group_col,
                            group_is_key, hint)
        assert res.local_level == level, (hint, res.local_level)
        if n_rows is not None:
            assert res.rows_scanned == n_rows
        assert res.n_groups == len(want), (res.n_groups, len(want))
        assert res.has_null_group == (1 if None in want else 0)
        assert res.rows_matched == _matched(want)
        check_groups(got, want, aggs)
        check_order(raw[0], res)
        raws.append(raw_bytes(*raw, res))
    assert all(r == raws[0] for r in raws[1:]), "levels differ bitwise"
    return raws[0]


def scenario_row_count_edge(run, n):
    case = edge_tablet(n)
    preds, aggs = sc.edge_query()
    want = oracle_groups(case, sc.EDGE_READ, preds, aggs, 2)
    check_both_levels(run, case, sc.EDGE_READ, preds, aggs, 2, want,
                      n_rows=n)


def scenario_empty(run):
    case = edge_tablet(65)
    preds, aggs = sc.edge_query()
    for hint, level in levels(len(aggs)):
        got, _raw, res = run(case, sc.EDGE_READ_BEFORE, preds, aggs, 2,
                             False, hint)
        assert got == {} and res.n_groups == 0 and res.has_null_group == 0
        assert res.rows_scanned == 0 and res.rows_matched == 0
        assert res.local_level == level
    # rows, but none matches
    none = [y.Pred(0, 2, y.PRED_GT, 5000, None, 0)]
    got, _raw, res = run(case, sc.EDGE_READ, none, aggs, 2)
    assert got == {} and res.n_groups == 0 and res.rows_scanned == 65
    assert res.rows_matched == 0


CARD_LABELS = ("1", "L-1", "L", "L+1", "4L", "rows")


def scenario_cardinality(run, label, num_aggs):
    L = local_slots(num_aggs)
    n_groups = {"1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "4L": 4 * L,
                "rows": CARD_ROWS}[label]
    case = cardinality_tablet(n_groups)
    aggs = aggs2() if num_aggs == 2 else aggs8()
    want = oracle_groups(case, READ, [], aggs, 0)
    assert len(want) == n_groups
    # hint 0 (unknown) takes the two-level kernel: above L groups, rows
    # spill past the local table inside it
    hints = ((0, 1),) + levels(num_aggs)
    check_both_levels(run, case, READ, [], aggs, 0, want, hints=hints,
                      n_rows=cardinality_rows(n_groups))


def scenario_grid_stride(run):
    case = grid_stride_tablet()
    aggs = aggs2()
    want = oracle_groups(case, READ, [], aggs, 0)
    assert len(want) == 97
    check_both_levels(run, case, READ, [], aggs, 0, want,
                      hints=((0, 1),) + levels(2), n_rows=grid_stride_rows())


def scenario_group_on_key_column(run):
    case = kinds_tablet()
    aggs = kinds_aggs()
    want, n = fold_groups(case, READ, [], aggs, 0, True)
    assert len(want) == KIND_ROWS == n   # every row its own group
    check_both_levels(run, case, READ, [], aggs, 0, want, group_is_key=True)


def scenario_group_column_kinds(run):
    case = kinds_tablet()
    aggs = kinds_aggs()
    # double column: orcl_group; int64 / int32 hold a -1, which orcl_group's
    # decoder reads as its NULL marker: the row fold is the reference there
    check_both_levels(run, case, READ, [], aggs, 1,
                      oracle_groups(case, READ, [], aggs, 1))
    for col in (0, 2, 3):
        want, _n = fold_groups(case, READ, [], aggs, col, False)
        check_both_levels(run, case, READ, [], aggs, col, want)


def scenario_null_group_next_to_minus_one(run):
    case = kinds_tablet()
    aggs = kinds_aggs()
    want, _n = fold_groups(case, READ, [], aggs, 0, False)
    assert U64 in want and None in want and len(want) == 6
    for hint, _level in levels(len(aggs)):
        got, raw, res = run(case, READ, [], aggs, 0, False, hint)
        assert res.n_groups == 6 and res.has_null_group == 1
        keys = [raw[0][i] for i in range(6)]
        # unsigned order: 0, 3, 2**40, -5, -1, then the NULL group (key 0)
        assert keys == [0, 3, 1 << 40, (-5) & U64, U64, 0]
        assert got[U64] == want[U64] and got[None] == want[None]
        assert got[U64] != got[None]


def scenario_nullable_specialisation(run):
    preds, aggs = sc.edge_query()
    preds2, aggs2_ = sc.edge_query_no_null_col()
    dense = edge_tablet(777, nulls=False)
    check_both_levels(run, dense, sc.EDGE_READ, preds, aggs, 2,
                      oracle_groups(dense, sc.EDGE_READ, preds, aggs, 2))
    sparse = edge_tablet(777, nulls=True)
    check_both_levels(run, sparse, sc.EDGE_READ, preds2, aggs2_, 2,
                      oracle_groups(sparse, sc.EDGE_READ, preds2, aggs2_, 2))
    check_both_levels(run, sparse, sc.EDGE_READ, preds, aggs, 2,
                      oracle_groups(sparse, sc.EDGE_READ, preds, aggs, 2))
    # grouping ON the NULL-carrying double column: a NULL group appears
    cnt = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 0)]
    want = oracle_groups(sparse, sc.EDGE_READ, [], cnt, 1)
    assert None in want
    check_both_levels(run, sparse, sc.EDGE_READ, [], cnt, 1, want)


def scenario_in_and_in_range(run):
    case = kinds_tablet()
    aggs = kinds_aggs()
    preds = gen_preds()
    want = oracle_groups(case, READ, preds, aggs, 1)
    assert 0 < _matched(want) < KIND_ROWS
    check_both_levels(run, case, READ, preds, aggs, 1, want)


def scenario_doubles(run):
    """Against the oracle (SUM within 1e-9, the rest exact) and bit-equal
    to ybg_sim_group, the block path's simulator: both sums are exact."""
    case = doubles_tablet()
    aggs = doubles_aggs()
    want = oracle_groups(case, READ, [], aggs, 0)
    assert len(want) == 97
    check_both_levels(run, case, READ, [], aggs, 0, want)
    got, _raw, _res = run(case, READ, [], aggs, 0)
    blk = y.sim_group(block_spec(case, READ, [], aggs, 0), case["data"],
                      case["offsets"], case["n_blocks"])
    assert same_bits(got, blk)


def scenario_poison(run):
    case = poison_tablet()
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_DOUBLE, 1)]
    for hint, _level in levels(len(aggs)):
        got, _raw, res = run(case, READ, [], aggs, 0, False, hint)
        assert res.n_groups == 3
        assert math.isnan(got[0][1]) and got[0][0] == 100
        for k in (1, 2):   # halves sum exactly
            assert got[k] == (100, sum(r * 0.5 for r in range(300)
                                       if r % 3 == k))


def scenario_errors(run, message=False):
    """Code 9 for every unsupported query (with `message`, the text names
    the offender), the snapshot answering a valid query after each; code 8
    with the needed count when cap is one short."""
    case = string_tablet()
    cnt = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 2)]
    want = oracle_groups(case, READ, [], cnt, 0)
    bad = [
        # (preds, aggs, group_col, group_is_key, names)
        ([], cnt, 1, False, "group column"),            # string value column
        ([], cnt, 1, True, "group column"),             # string key column
        ([], cnt, 3, False, "group column"),            # out of range
        ([], cnt, -1, False, "group column"),
        ([], cnt, 2, True, "group column"),
        ([], [], 0, False, "num_aggs"),                 # no aggregate
        ([y.Pred(0, 1, y.PRED_EQ, 0, None, 0)], cnt, 0, False,
         "predicate 0"),
        ([], [cnt[0], y.Agg(y.AGG_COUNT, 1)], 0, False, "aggregate 1"),
        ([], cnt * 5, 0, False, "num_aggs"),
        ([y.Pred(0, 0, y.PRED_GT, 0, None, 0)] * 9, cnt, 0, False,
         "num_preds"),
    ]
    for preds, aggs, col, is_key, names in bad:
        try:
            run(case, READ, preds, aggs, col, is_key)
        except Exception as e:   # the runner's error type
            assert e.code == 9, str(e)
            if message:
                assert names in str(e), str(e)
        else:
            raise AssertionError("accepted: %s col %d" % (names, col))
        got, _raw, _res = run(case, READ, [], cnt, 0)
        check_groups(got, want, cnt)
    # output capacity one short of the group count
    try:
        run(case, READ, [], cnt, 0, cap=len(want) - 1)
    except Exception as e:
        assert e.code == 8, str(e)
        assert e.result.n_groups == len(want)
    else:
        raise AssertionError("cap too small accepted")
    got, _raw, _res = run(case, READ, [], cnt, 0, cap=len(want))
    check_groups(got, want, cnt)


def scenario_determinism(run_fresh, n_snapshots=2, n_queries=3):
    """run_fresh() -> a `run` bound to a SEPARATELY built snapshot of the
    doubles tablet. Raw keys / vals / cnts byte-identical across snapshots,
    repeated queries and both levels. Returns the common raw bytes."""
    case = doubles_tablet()
    aggs = doubles_aggs()
    preds = [y.Pred(1, 0, y.PRED_GE, 100, None, 0)]
    raws = []
    for _ in range(n_snapshots):
        run = run_fresh()
        for _q in range(n_queries):
            for hint, level in levels(len(aggs)):
                _got, raw, res = run(case, READ, preds, aggs, 0, False, hint)
                assert res.local_level == level
                raws.append(raw_bytes(*raw, res))
    assert len(raws) == n_snapshots * n_queries * 2
    assert all(r == raws[0] for r in raws[1:])
    return raws[0], (case, preds, aggs)
