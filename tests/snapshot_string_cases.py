"""Shared pieces of the string-snapshot tests (test_snapshot_strings_sim.py on
the CPU simulator, test_snapshot_strings_gpu.py on the HIP kernels): the
tablets, the references (always the CPU oracle on the same tablet) and the
scenarios. A scenario takes a runner `r` with

    r.query(case, read_micros, preds, aggs, strings=True) -> ScanResult
    r.group(case, read_micros, preds, aggs, group_col, group_is_key=False,
            strings=True) -> (groups dict, raw, result)
    r.select_var(case, read_micros, preds, cols, limit=0, backward=False,
                 row_lo=0, row_hi=None, cap=CAP, varlen_cap=VCAP,
                 strings=True)
        -> (rows, (datums, null_masks, row_ids, varlen, varlen_size), result)
    r.select_plain(case, read_micros, preds, cols, strings=True)
        -> (rows, raw, result)        # yb_gpu_snapshot_select

strings: whether the snapshot is built with stage_strings. rows are the
decoded tuples (strings as bytes, None for NULL). Errors raise with .code
(and .result / .varlen_size where the ABI fills them)."""
import ctypes as C
import functools
import struct

import ybgpu as y
from parity_cases import _case, check_match, make_orcl_spec, run_oracle
import snapshot_group_cases as sg

CAP = 1 << 12
VCAP = 1 << 18
READ = 1_000_000          # after every write (rows are written at 1000 + r)
CMP_OPS = (y.PRED_GT, y.PRED_GE, y.PRED_LT, y.PRED_LE, y.PRED_EQ, y.PRED_NE)

_KEEP = []


def tile_rows():
    """T: rows per compaction tile, always asked of the library."""
    return y.snapshot_select_tile_rows()


def edge_sizes():
    T = tile_rows()
    return (1, 2, T - 1, T, T + 1, 2 * T + 1)


def _buf(b):
    arr = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
    _KEEP.append(arr)
    return arr


def str_pred(is_key, col, op, rhs):
    """A compare predicate with a string rhs (the block path's ABI form)."""
    return y.Pred(1 if is_key else 0, col, op, 0, _buf(rhs), len(rhs))


def str_in(is_key, col, options):
    """IN over [u32 len][bytes] records."""
    blob = b"".join(struct.pack("<I", len(o)) + o for o in options)
    return y.Pred(1 if is_key else 0, col, y.PRED_IN, 0, _buf(blob),
                  len(blob))


# ---- references ------------------------------------------------------------

def oracle_rows(case, read_micros, preds, cols):
    """The oracle's matching rows in key order, projected on cols."""
    osc = y.orcl_schema_from(case["schema"])
    ospec = make_orcl_spec(read_micros, preds, ())
    _res, rows = y.orcl_scan(case["data"], case["offsets"], case["n_blocks"],
                             osc, ospec, kv_format=case["kv_format"],
                             collect_rows=True)
    return [tuple(kd[c] if is_key else vals[c] for is_key, c in cols)
            for kd, vals in rows]


def canonical_heap(case, rows, cols):
    """The heap select_var must deliver for `rows`: delivery order, within a
    row the projected string columns in projection order, back to back."""
    strs = y.select_string_cols(case["schema"], cols)
    return b"".join(v for row in rows for v, s in zip(row, strs)
                    if s and v is not None)


def heap_of(raw):
    return bytes(raw[3][:raw[4]])


def raw_bytes(raw, res, num_cols, cap):
    """The written part of the output arrays and the heap, as bytes."""
    datums, null_masks, row_ids, _varlen, _vs = raw
    n = res.n_rows
    d = memoryview(datums).cast("B")
    return (bytes(memoryview(row_ids).cast("B")[:n * 8]),
            bytes(memoryview(null_masks).cast("B")[:n * 4]),
            tuple(bytes(d[j * cap * 8:(j * cap + n) * 8])
                  for j in range(num_cols)),
            heap_of(raw))


def check_select(r, case, preds, cols, want=None, **kw):
    """select_var equals the oracle's rows (or `want`), its heap is the
    canonical one and NULL datums are 0."""
    if want is None:
        want = oracle_rows(case, READ, preds, cols)
        if kw.get("backward"):
            want = want[::-1]
    rows, raw, res = r.select_var(case, READ, preds, cols, **kw)
    assert rows == want, (case["name"], len(rows), len(want), next(
        ((i, g, w) for i, (g, w) in enumerate(zip(rows, want)) if g != w),
        None))
    assert res.n_rows == len(want)
    assert heap_of(raw) == canonical_heap(case, rows, cols)
    cap = kw.get("cap", CAP)
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            if v is None:
                assert raw[0][j * cap + i] == 0
    return rows, raw, res


def all_cols(schema):
    """Every key column, then every value column, strings included."""
    nk = schema.num_hash_cols + schema.num_range_cols
    return [(1, c) for c in range(nk)] + \
        [(0, c) for c in range(schema.num_value_cols)]


# ---- 1. parity on the existing string cases ---------------------------------

PARITY_CASES = ("string_eq_pred", "in_list_string", "mixed_types")
N_PARITY_RUNS = 4   # 1 + 2 + 1 runs, all accepted with strings=True


def scenario_parity(r, cases):
    """Every run of the three string-carrying parity cases: rows_matched and
    all aggregates, entries_seen included, equal the oracle's."""
    checked = 0
    for case in cases:
        if case["name"] not in PARITY_CASES:
            continue
        for run in case["runs"]:
            read_micros, preds, aggs = run[0], list(run[1]), list(run[2])
            assert y.stageable(case["schema"], preds, aggs, strings=True)
            got = r.query(case, read_micros, preds, aggs)
            check_match(got, run_oracle(case, read_micros, preds, aggs), aggs)
            if any((p.is_key_col and
                    case["schema"].key_types[p.col] == y.KT_STRING) or
                   (not p.is_key_col and
                    case["schema"].value_cols[p.col].dtype == y.T_STRING)
                   for p in preds):
                # a default snapshot keeps refusing the same query
                assert not y.stageable(case["schema"], preds, aggs)
            checked += 1
    assert checked == N_PARITY_RUNS, checked


def scenario_parity_select(r, cases):
    """in_list_string (string KEY column holding \\0): the string rows
    themselves, keys unescaped, equal the oracle's."""
    case = next(c for c in cases if c["name"] == "in_list_string")
    cols = all_cols(case["schema"])
    for run in case["runs"]:
        rows, _raw, _res = check_select(r, case, list(run[1]), cols)
        assert len(rows) > 0


def scenario_string_tablet(r):
    """snapshot_group_cases.string_tablet(): string predicates on its value
    and key column under plain, grouped and select queries."""
    case = sg.string_tablet()
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 2),
            y.Agg(y.AGG_COUNT, 1)]
    for preds in ([str_pred(0, 1, y.PRED_EQ, b"s1")],
                  [str_pred(0, 1, y.PRED_GT, b"s0"),
                   str_pred(1, 1, y.PRED_EQ, b"k")],
                  [str_pred(1, 1, y.PRED_LT, b"k")],
                  [str_in(0, 1, [b"s2", b"nope", b""])]):
        assert y.stageable(case["schema"], preds, aggs, strings=True)
        assert not y.stageable(case["schema"], preds, aggs)
        check_match(r.query(case, READ, preds, aggs),
                    run_oracle(case, READ, preds, aggs), aggs)
        gaggs = aggs[:2]
        groups, _raw, res = r.group(case, READ, preds, gaggs, 0)
        want = sg.oracle_groups(case, READ, preds, gaggs, 0)
        sg.check_groups(groups, want, gaggs)
        assert res.rows_matched == sum(v[0] for v in want.values())
        check_select(r, case, preds, all_cols(case["schema"]))


# ---- 2. the ordering corner tablet ------------------------------------------

CORNER_SCHEMA = y.make_schema(
    [y.KT_INT64, y.KT_STRING],
    [(10, y.T_STRING, 1), (11, y.T_INT64, 1)], num_hash_cols=1)

_P8 = b"prefix-8"          # the shared first 8 bytes
_P24 = b"twenty-four-bytes-long-"
CORNER_VALUES = [
    b"", None, b"a", b"a\x00", b"a\x00b",
    _P8[:7], _P8, _P8 + b"9", _P8 + b"16bytes!", _P8 + b"17 bytes!",
    _P24 + b"x", _P24 + b"y",
    b"\x7f", b"\x80", b"\xff", b"\x7f\xff", b"\x80\x00",
    b"b", b"a", b"", None, _P8, _P8 + b"9",   # duplicates
]
CORNER_ABSENT = [b"a\x00a", _P8 + b"8", b"\x00", _P24, b"zz", _P8[:4]]
# key strings hold \x00 (the \0\1 escape) and stay far under the oracle's
# 256-byte unescape buffer (key_unesc in orcl_scan.c)
CORNER_KEYS = [
    b"", b"\x00", b"\x00\x00", b"\x00\x01", b"a", b"a\x00", b"a\x00b",
    b"a\x00\x00", _P8[:7], _P8, _P8 + b"\x00", _P8 + b"\x00tail",
    _P8 + b"9", b"\x7f", b"\x80", b"\xff", b"\xff\x00", b"k\x00z",
    _P24 + b"\x00x", _P24 + b"\x00y",
]
CORNER_KEYS_ABSENT = [b"a\x00a", b"\x00\x02", _P8 + b"\x01", b"zz"]


@functools.lru_cache(maxsize=None)
def corner_tablet():
    """40 rows: row i has hashed key i // 8, range key CORNER_KEYS[i % 20]
    (each key string twice, under two hashed keys), string value
    CORNER_VALUES[i % 23] and int64 i."""
    b = y.Builder(CORNER_SCHEMA)
    for i in range(40):
        b.add_packed_row(
            1000 + i,
            [(y.T_STRING, CORNER_VALUES[i % len(CORNER_VALUES)]),
             (y.T_INT64, i)],
            hash_=i // 8, key_datums=(i // 20, 0),
            key_strs=(None, CORNER_KEYS[i % len(CORNER_KEYS)]))
    _KEEP.append(b)
    return _case("string_corners", CORNER_SCHEMA, b.finish(), [])


def corner_rhs(is_key):
    if is_key:
        return sorted(set(CORNER_KEYS)) + CORNER_KEYS_ABSENT
    return sorted({v for v in CORNER_VALUES if v is not None}) + \
        CORNER_ABSENT


CORNER_AGGS = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 0),
               y.Agg(y.AGG_SUM_INT64, 1)]
ID_COLS = [(0, 1)]


def scenario_corner_compare(r, is_key, op):
    """One op, every distinct value (and values no row holds) as rhs: the
    matching row set and the aggregates equal the oracle's."""
    case = corner_tablet()
    col = 1 if is_key else 0
    for rhs in corner_rhs(is_key):
        preds = [str_pred(is_key, col, op, rhs)]
        want = oracle_rows(case, READ, preds, ID_COLS)
        rows, _raw, res = r.select_var(case, READ, preds, ID_COLS)
        assert rows == want, (is_key, op, rhs, rows, want)
        assert res.rows_matched == len(want)
        check_match(r.query(case, READ, preds, CORNER_AGGS),
                    run_oracle(case, READ, preds, CORNER_AGGS), CORNER_AGGS)


def scenario_corner_in(r):
    case = corner_tablet()
    for is_key, col, opts in (
            (0, 0, [_P8 + b"9", b"no-such", b""]),
            (0, 0, [b"a\x00", b"a", _P24 + b"y"]),
            (0, 0, [b"missing"]),
            (1, 1, [b"a\x00b", b"absent", b""]),
            (1, 1, [b"\x00\x01", _P24 + b"\x00x"])):
        preds = [str_in(is_key, col, opts)]
        want = oracle_rows(case, READ, preds, ID_COLS)
        rows, _raw, _res = r.select_var(case, READ, preds, ID_COLS)
        assert rows == want, (is_key, opts, rows, want)
        check_match(r.query(case, READ, preds, CORNER_AGGS),
                    run_oracle(case, READ, preds, CORNER_AGGS), CORNER_AGGS)
    # the empty IN list matches nothing
    got = r.query(case, READ, [str_in(0, 0, [])], CORNER_AGGS)
    assert got.rows_matched == 0


def scenario_null_vs_empty(r):
    """EQ b"" matches the empty strings and not the NULLs; COUNT(col) skips
    exactly the NULLs."""
    case = corner_tablet()
    n_null = sum(1 for i in range(40)
                 if CORNER_VALUES[i % len(CORNER_VALUES)] is None)
    n_empty = sum(1 for i in range(40)
                  if CORNER_VALUES[i % len(CORNER_VALUES)] == b"")
    assert n_null > 0 and n_empty > 0
    got = r.query(case, READ, [str_pred(0, 0, y.PRED_EQ, b"")], CORNER_AGGS)
    assert got.rows_matched == n_empty
    assert got.aggs[1].value_i64 == n_empty        # none of them NULL
    got = r.query(case, READ, [], CORNER_AGGS)
    assert got.rows_matched == 40
    assert got.aggs[1].value_i64 == 40 - n_null
    # NE and GE b"" still fail on NULL
    got = r.query(case, READ, [str_pred(0, 0, y.PRED_GE, b"")], CORNER_AGGS)
    assert got.rows_matched == 40 - n_null
    got = r.query(case, READ, [str_pred(0, 0, y.PRED_NE, b"")], CORNER_AGGS)
    assert got.rows_matched == 40 - n_null - n_empty
    rows, raw, _res = r.select_var(case, READ, [], [(0, 0), (0, 1)])
    for i, row in enumerate(rows):
        v = CORNER_VALUES[row[1] % len(CORNER_VALUES)]
        assert row[0] == v
        if v is None:
            assert raw[0][i] == 0 and (raw[1][i] & 1)
        else:
            assert not raw[1][i] & 1


# ---- 3. shape edges ---------------------------------------------------------

EDGE_SCHEMA = y.make_schema(
    [y.KT_INT64, y.KT_STRING],
    [(10, y.T_STRING, 1), (11, y.T_INT64, 1)], num_hash_cols=1)


def edge_value(r):
    """Length r % 21 (0 .. 20: under, at and over the 8-byte prefix), NULL
    on every 7th row; many rows share their first 8 bytes."""
    if r % 7 == 3:
        return None
    return (b"%04d" % (r % 10) + b"-edge-" + b"%010d" % r)[:r % 21]


def edge_key(r):
    return b"k\x00%d" % (r % 13)


@functools.lru_cache(maxsize=None)
def edge_tablet(n):
    b = y.Builder(EDGE_SCHEMA)
    for r in range(n):
        b.add_packed_row(1000 + r,
                         [(y.T_STRING, edge_value(r)), (y.T_INT64, r)],
                         hash_=min(r // 64, 65535), key_datums=(r, 0),
                         key_strs=(None, edge_key(r)))
    _KEEP.append(b)
    return _case("string_edge_%d" % n, EDGE_SCHEMA, b.finish(), [])


def edge_preds(n):
    last = edge_value(n - 1) if edge_value(n - 1) is not None else b""
    return [
        [],
        [str_pred(0, 0, y.PRED_EQ, last)],
        [str_pred(0, 0, y.PRED_LT, b"0004-edge")],          # a tie on 8 bytes
        [str_pred(0, 0, y.PRED_GE, b"0005"),
         str_pred(1, 1, y.PRED_NE, edge_key(1))],
        [str_in(1, 1, [edge_key(0), edge_key(12), b"k"])],
    ]


def scenario_edge(r, n):
    case = edge_tablet(n)
    cols = all_cols(case["schema"])
    for preds in edge_preds(n):
        check_match(r.query(case, READ, preds, CORNER_AGGS),
                    run_oracle(case, READ, preds, CORNER_AGGS), CORNER_AGGS)
        rows, _raw, res = check_select(r, case, preds, cols,
                                       cap=max(n, 1))
        assert res.rows_scanned == n
        if not preds:
            assert len(rows) == n


LARGE_ROWS = 70_001   # > one 1024-thread block of the offsets' prefix sum


def scenario_large(r):
    """Several workgroups of the pack kernel, several blocks of the scans."""
    n = LARGE_ROWS
    case = edge_tablet(n)
    for preds in ([str_pred(0, 0, y.PRED_EQ, edge_value(n - 1))],
                  [str_pred(0, 0, y.PRED_LT, b"0004-edge")],
                  [str_pred(1, 1, y.PRED_EQ, edge_key(5)),
                   str_pred(0, 0, y.PRED_GT, b"0007-edge-00000600")]):
        check_match(r.query(case, READ, preds, CORNER_AGGS),
                    run_oracle(case, READ, preds, CORNER_AGGS), CORNER_AGGS)
    # the string rows of a selective predicate from all over the tablet
    preds = [str_pred(1, 1, y.PRED_EQ, edge_key(5)),
             str_pred(0, 0, y.PRED_GT, b"0007-edge-00000600")]
    rows, _raw, _res = check_select(r, case, preds,
                                    all_cols(case["schema"]), cap=1 << 14)
    assert len(rows) > 100
    # the last rows, all columns (the heap's far end)
    tail = [(r_, edge_key(r_), edge_value(r_), r_)
            for r_ in range(n - 700, n)]
    cols = [(1, 0), (1, 1), (0, 0), (0, 1)]
    check_select(r, case, [], cols, want=tail[::-1], backward=True,
                 limit=700)


# ---- 4. select_var ----------------------------------------------------------

def scenario_select_directions(r):
    case = edge_tablet(2 * tile_rows() + 1)
    cols = [(0, 0), (0, 1), (1, 1), (1, 0)]
    preds = [str_pred(0, 0, y.PRED_GE, b"0003")]
    check_select(r, case, preds, cols)
    check_select(r, case, preds, cols, backward=True)
    # a projection that repeats a string column
    check_select(r, case, preds, [(0, 0), (0, 0), (1, 1), (0, 0)])
    # no string column projected: select_var == select, empty heap
    rows, raw, res = r.select_var(case, READ, preds, [(0, 1), (1, 0)])
    prow, _praw, pres = r.select_plain(case, READ, preds, [(0, 1), (1, 0)])
    assert raw[4] == 0 and rows == prow and res.n_rows == pres.n_rows


def scenario_select_paging(r, limit, backward):
    """Limit pages concatenate to the unlimited result; every page's heap is
    re-based (canonical for that page alone)."""
    n = 2 * tile_rows() + 1
    case = edge_tablet(n)
    cols = [(0, 0), (0, 1), (1, 1)]
    preds = [str_pred(0, 0, y.PRED_GT, b"0002-edge")]
    want = oracle_rows(case, READ, preds, cols)
    if backward:
        want = want[::-1]
    got, lo, hi, pages = [], 0, None, 0
    while True:
        rows, raw, res = r.select_var(case, READ, preds, cols, limit=limit,
                                      backward=backward, row_lo=lo,
                                      row_hi=hi)
        assert heap_of(raw) == canonical_heap(case, rows, cols)
        got += rows
        pages += 1
        if res.done:
            break
        assert res.n_rows == limit
        if backward:
            hi = res.resume_row
        else:
            lo = res.resume_row
        assert pages < 10_000
    assert got == want
    assert pages >= -(-len(want) // limit)


def scenario_select_window(r):
    n = 2 * tile_rows() + 1
    case = edge_tablet(n)
    cols = [(0, 1), (0, 0), (1, 1)]
    T = tile_rows()
    for lo, hi in ((1, 2), (3, T + 8), (T - 1, T + 2), (T + 1, n - 1),
                   (5, 5), (n - 1, None)):
        hi_eff = n if hi is None else hi
        want = [(r_, edge_value(r_), edge_key(r_))
                for r_ in range(lo, hi_eff)]
        rows, _raw, res = check_select(r, case, [], cols, want=want,
                                       row_lo=lo, row_hi=hi)
        assert res.rows_scanned == max(0, hi_eff - lo)
        want_b = [w for w in want if w[1] is not None and w[1] >= b"0005"]
        check_select(r, case, [str_pred(0, 0, y.PRED_GE, b"0005")], cols,
                     want=want_b[::-1], row_lo=lo, row_hi=hi, backward=True)


def scenario_varlen_cap(r):
    """varlen_cap one byte short: error 8 with the size needed; after that
    the snapshot still answers."""
    case = edge_tablet(tile_rows() + 1)
    cols = [(0, 0), (1, 1)]
    rows, raw, res = check_select(r, case, [], cols)
    need = raw[4]
    assert need == len(canonical_heap(case, rows, cols)) > 0
    try:
        r.select_var(case, READ, [], cols, varlen_cap=need - 1)
        raise AssertionError("varlen_cap one byte short was accepted")
    except RuntimeError as e:
        assert e.code == 8, e
        assert e.varlen_size == need
        assert e.result.rows_matched == res.rows_matched
        assert e.result.done == 0
    rows2, raw2, _res2 = r.select_var(case, READ, [], cols, varlen_cap=need)
    assert rows2 == rows and heap_of(raw2) == heap_of(raw)
    # the row cap still reports first
    try:
        r.select_var(case, READ, [], cols, cap=len(rows) - 1)
        raise AssertionError("row cap one short was accepted")
    except RuntimeError as e:
        assert e.code == 8 and e.result.n_rows == len(rows)


# ---- 5. determinism ---------------------------------------------------------

def determinism_query():
    case = edge_tablet(2 * tile_rows() + 1)
    cols = [(0, 0), (1, 1), (0, 1), (0, 0)]
    preds = [str_pred(0, 0, y.PRED_NE, b"0001-edge")]
    return case, preds, cols


def scenario_determinism(fresh):
    """fresh() -> a runner with snapshots of its own. Two runners, two calls
    each: byte-identical arrays and heap. Returns the bytes."""
    case, preds, cols = determinism_query()
    seen = []
    for _ in range(2):
        r = fresh()
        for _ in range(2):
            _rows, raw, res = r.select_var(case, READ, preds, cols)
            seen.append(raw_bytes(raw, res, len(cols), CAP))
    assert len(seen[0][3]) > 0
    assert all(s == seen[0] for s in seen[1:])
    return seen[0]


# ---- 6. unchanged defaults and refusals -------------------------------------

def _refused(fn, needle=None):
    try:
        fn()
    except RuntimeError as e:
        assert e.code == 9, e
        if needle is not None:
            assert needle in str(e), str(e)
        return
    raise AssertionError("query was not refused")


def scenario_default_refuses(r, message=False):
    """A snapshot built the old way keeps refusing strings."""
    case = corner_tablet()
    sp = [str_pred(0, 0, y.PRED_EQ, b"a")]
    kp = [str_pred(1, 1, y.PRED_EQ, b"a")]
    star = [y.Agg(y.AGG_COUNT_STAR, 0)]
    m = "not staged" if message else None
    _refused(lambda: r.query(case, READ, sp, star, strings=False), m)
    _refused(lambda: r.query(case, READ, kp, star, strings=False), m)
    _refused(lambda: r.query(case, READ, [], [y.Agg(y.AGG_COUNT, 0)],
                             strings=False), m)
    _refused(lambda: r.select_plain(case, READ, [], [(0, 0)], strings=False),
             m)
    _refused(lambda: r.select_var(case, READ, [], [(1, 1)], strings=False),
             m)
    _refused(lambda: r.group(case, READ, sp, star, 1, strings=False), m)
    got = r.query(case, READ, [], star, strings=False)
    assert got.rows_matched == 40


def scenario_string_refusals(r, message=False):
    """Still error 9 on a string snapshot, each followed by a valid query."""
    case = corner_tablet()
    star = [y.Agg(y.AGG_COUNT_STAR, 0)]
    rng = struct.pack("<QQQ", 0, 1, 3)
    in_range = y.Pred(0, 0, y.PRED_IN_RANGE, 0, _buf(rng), len(rng))
    bad_list = y.Pred(0, 0, y.PRED_IN, 0, _buf(b"\x05\0\0\0ab"), 6)

    def ok():
        got = r.query(case, READ, [str_pred(0, 0, y.PRED_EQ, b"a")], star)
        assert got.rows_matched == sum(
            1 for i in range(40)
            if CORNER_VALUES[i % len(CORNER_VALUES)] == b"a")

    refusals = [
        (lambda: r.group(case, READ, [], star, 0), "group column"),
        (lambda: r.group(case, READ, [], star, 1, group_is_key=True),
         "group column"),
        (lambda: r.query(case, READ, [in_range], star), "IN_RANGE"),
        (lambda: r.query(case, READ, [bad_list], star), "malformed"),
        (lambda: r.select_plain(case, READ, [], [(0, 1), (0, 0)]),
         "yb_gpu_snapshot_select_var"),
        (lambda: r.select_plain(case, READ, [], [(1, 1)]),
         "yb_gpu_snapshot_select_var"),
    ]
    for op in (y.AGG_SUM_INT64, y.AGG_SUM_DOUBLE, y.AGG_MIN_INT64,
               y.AGG_MAX_INT64, y.AGG_MIN_DOUBLE, y.AGG_MAX_DOUBLE):
        refusals.append(
            (lambda op=op: r.query(case, READ, [], [y.Agg(op, 0)]), "COUNT"))
    for fn, needle in refusals:
        _refused(fn, needle if message else None)
        ok()
    assert not y.stageable(case["schema"], [in_range], star, strings=True)
    assert not y.stageable(case["schema"], [bad_list], star, strings=True)
    assert not y.stageable(case["schema"], [],
                           [y.Agg(y.AGG_MAX_INT64, 0)], strings=True)
    assert y.stageable(case["schema"], [], [y.Agg(y.AGG_COUNT, 0)],
                       strings=True)
