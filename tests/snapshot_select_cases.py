"""Shared pieces of the snapshot SELECT tests (test_snapshot_select_sim.py on
the CPU simulator, test_snapshot_select_gpu.py on the HIP kernels): the
reference (the oracle's matching rows in key order), the tablets and the
scenarios. A scenario takes `run`:

    run(case, read_micros, preds, cols, limit=0, backward=False, row_lo=0,
        row_hi=None, cap=CAP, lower=None, upper=None)
      -> (rows, (datums, null_masks, row_ids), result)

rows being the decoded tuples (ybgpu.decode_snapshot_rows); errors raise with
.code and .result."""
import ctypes as C
import functools
import struct

import pytest

import ybgpu as y
from parity_cases import SCHEMA_4I, _case, make_orcl_spec
import snapshot_cases as sc

CAP = 1 << 12
U64 = (1 << 64) - 1

# runs of parity_cases.build_cases() whose PREDICATES a snapshot can answer
# (y.stageable(schema, preds, ())): 35 runs minus string_eq_pred (1),
# in_list_string (2) and in_tuple_keycols (1). Computed once on the CPU from
# the cases; a silently skipped run fails the parity test.
N_SELECT_RUNS = 31

_KEEP = []


def tile_rows():
    """T: rows per compaction tile, always asked of the library."""
    return y.snapshot_select_tile_rows()


def edge_sizes():
    T = tile_rows()
    return tuple(sorted(set(sc.EDGE_SIZES) | {T - 1, T, T + 1, 2 * T + 1}))


@functools.lru_cache(maxsize=None)
def edge_tablet(n, nulls=True):
    return sc.edge_tablet(n, nulls)


def all_cols(schema):
    """Every non-string key column, then every non-string value column."""
    nk = schema.num_hash_cols + schema.num_range_cols
    cols = [(1, c) for c in range(nk) if schema.key_types[c] != y.KT_STRING]
    cols += [(0, c) for c in range(schema.num_value_cols)
             if schema.value_cols[c].dtype != y.T_STRING]
    return cols


def key_in(values):
    """key column 0 IN (values)."""
    buf = struct.pack("<%dq" % len(values), *values)
    arr = (C.c_uint8 * len(buf)).from_buffer_copy(buf)
    _KEEP.append(arr)
    return y.Pred(1, 0, y.PRED_IN, 0, arr, len(buf))


NO_ROW = y.Pred(1, 0, y.PRED_LT, 0, None, 0)   # keys are >= 0


# ---- reference -------------------------------------------------------------

def oracle_rows(case, read_micros, preds, cols, lower=None, upper=None):
    """The oracle's matching rows in key order, projected on cols."""
    osc = y.orcl_schema_from(case["schema"])
    ospec = make_orcl_spec(read_micros, preds, (), lower, upper)
    _res, rows = y.orcl_scan(case["data"], case["offsets"], case["n_blocks"],
                             osc, ospec, kv_format=case["kv_format"],
                             collect_rows=True)
    return [tuple(kd[c] if is_key else vals[c] for is_key, c in cols)
            for kd, vals in rows]


def oracle_count(case, read_micros, preds, lower=None, upper=None):
    osc = y.orcl_schema_from(case["schema"])
    ospec = make_orcl_spec(read_micros, preds, (), lower, upper)
    res, _ = y.orcl_scan(case["data"], case["offsets"], case["n_blocks"],
                         osc, ospec, kv_format=case["kv_format"])
    return res.rows_matched


def raw_bytes(raw, res, num_cols, cap):
    """The written part of the three output arrays, as bytes."""
    datums, null_masks, row_ids = raw
    n = res.n_rows
    d = memoryview(datums).cast("B")
    return (bytes(memoryview(row_ids).cast("B")[:n * 8]),
            bytes(memoryview(null_masks).cast("B")[:n * 4]),
            tuple(bytes(d[j * cap * 8:(j * cap + n) * 8])
                  for j in range(num_cols)))


def ids_of(raw, res):
    return list(raw[2][:res.n_rows])


def check_full(run, case, read_micros, preds, cols, want, lower=None,
               upper=None, cap=None):
    """An unlimited forward select equals the reference: count, order, every
    datum and every NULL; row_ids strictly ascending; counters and paging
    state of a complete result."""
    cap = max(len(want), 1) if cap is None else cap
    rows, raw, res = run(case, read_micros, preds, cols, cap=cap,
                         lower=lower, upper=upper)
    assert res.n_rows == len(want) == res.rows_matched, \
        (case["name"], res.n_rows, res.rows_matched, len(want))
    assert rows == want, (case["name"], next(
        (i, g, w) for i, (g, w) in enumerate(zip(rows, want)) if g != w))
    ids = ids_of(raw, res)
    assert all(a < b for a, b in zip(ids, ids[1:]))
    assert res.done == 1
    assert res.resume_row == res.rows_scanned   # row_hi clamped to n_rows
    return rows, raw, res


# ---- 1. parity on the shared cases -----------------------------------------

def filtered_20k():
    """config2_filtered_sum's shape at 20k rows (test_emit_parity.py)."""
    built = y.generate(SCHEMA_4I, rows=20_000, seed=7)
    preds = [y.Pred(0, 0, y.PRED_GT, 1 << 39, None, 0),
             y.Pred(0, 1, y.PRED_LT, 3 << 38, None, 0)]
    return _case("config2_20k", SCHEMA_4I, built, []), preds


def scenario_parity(run, cases):
    checked = 0
    for case, _ri, read_micros, preds, _aggs, lower, upper in \
            sc.iter_runs(cases):
        if not y.stageable(case["schema"], preds, ()):
            continue
        preds = list(preds)
        cols = all_cols(case["schema"])
        if case["name"] == "config2_filtered_sum":
            # 200k rows through the oracle's Python row callback are slow:
            # the match count here, the rows on the 20k tablet below
            _rows, _raw, res = run(case, read_micros, preds, cols, limit=1,
                                   cap=1)
            assert res.rows_matched == oracle_count(case, read_micros, preds)
            assert res.n_rows == 1 and res.done == 0
        else:
            want = oracle_rows(case, read_micros, preds, cols, lower, upper)
            check_full(run, case, read_micros, preds, cols, want, lower,
                       upper)
        checked += 1
    assert checked == N_SELECT_RUNS, checked
    case, preds = filtered_20k()
    cols = all_cols(case["schema"])
    want = oracle_rows(case, 1_700_000_000_000_000, preds, cols)
    assert len(want) > 0
    check_full(run, case, 1_700_000_000_000_000, preds, cols, want)


# ---- 2. row-count and tile edges -------------------------------------------

def edge_pred_shapes():
    T = tile_rows()
    return [("all", []), ("none", [NO_ROW]),
            ("edge_query", sc.edge_query()[0]),
            ("tile_seam", [key_in([T - 1, T])])]


def scenario_edge(run, n, nulls):
    case = edge_tablet(n, nulls)
    cols = all_cols(case["schema"])
    T = tile_rows()
    for name, preds in edge_pred_shapes():
        want = oracle_rows(case, sc.EDGE_READ, preds, cols)
        if name == "all":
            assert len(want) == n
        elif name == "none":
            assert want == []
        elif name == "tile_seam":
            assert len(want) == max(0, min(n, T + 1) - (T - 1))
        _rows, _raw, res = check_full(run, case, sc.EDGE_READ, preds, cols,
                                      want)
        assert res.rows_scanned == n


# ---- 2b. more tiles than the grid cap and than one scan round -------------

SCAN_ROUND_TILES = 4096   # kSnapScanThreads x kSnapScanVec tile counts
GRID_CAP = 1024           # kSnapMaxGrid workgroups


def large_rows():
    """One scan round of tiles, one whole tile and a 1-row tile more: the
    count / gather workgroups stride over tiles, the scan carries its
    running total into a second round."""
    return SCAN_ROUND_TILES * tile_rows() + tile_rows() + 1


@functools.lru_cache(maxsize=None)
def large_tablet():
    # generator rows: key = r in key order, so position == key
    built = y.generate(SCHEMA_4I, rows=large_rows(), seed=11)
    return _case("select_large", SCHEMA_4I, built, [])


def scenario_large(run):
    T = tile_rows()
    n = large_rows()
    case = large_tablet()
    R = 1_700_000_000_000_000
    cols = [(1, 0), (0, 0), (0, 3)]
    seams = [0, T - 1, T, GRID_CAP * T - 1, GRID_CAP * T, GRID_CAP * T + 1,
             SCAN_ROUND_TILES * T - 1, SCAN_ROUND_TILES * T,
             SCAN_ROUND_TILES * T + T - 1, n - 1]
    preds = [key_in(seams)]
    want = oracle_rows(case, R, preds, cols)
    assert [w[0] for w in want] == seams
    _rows, raw, res = check_full(run, case, R, preds, cols, want)
    assert ids_of(raw, res) == seams and res.rows_scanned == n
    # ~1 % of the rows, spread over every tile
    preds = [y.Pred(0, 0, y.PRED_LT, (1 << 40) // 100, None, 0)]
    want = oracle_rows(case, R, preds, cols)
    assert 15_000 < len(want) < 27_000
    _rows, raw, res = check_full(run, case, R, preds, cols, want)
    assert ids_of(raw, res) == [w[0] for w in want]
    # backward, limited, a window that starts inside the second scan round
    lo = SCAN_ROUND_TILES * T - 2 * T + 1
    tail = [w for w in want if w[0] >= lo]
    assert len(tail) > 3
    rows, raw, res = run(case, R, preds, cols, limit=3, backward=True,
                         row_lo=lo)
    assert rows == tail[::-1][:3] and res.rows_matched == len(tail)
    assert res.done == 0 and res.resume_row == tail[-3][0]


# ---- 3. empty snapshot, empty window ---------------------------------------

def scenario_empty(run):
    case = edge_tablet(65)
    cols = all_cols(case["schema"])
    for backward in (False, True):
        rows, _raw, res = run(case, sc.EDGE_READ_BEFORE, [], cols,
                              backward=backward)
        assert rows == [] and res.n_rows == 0 and res.done == 1
        assert res.rows_scanned == 0 and res.rows_matched == 0
        assert res.resume_row == 0
        for lo, hi in ((10, 10), (11, 10), (65, None), (70, 80)):
            rows, _raw, res = run(case, sc.EDGE_READ, [], cols, row_lo=lo,
                                  row_hi=hi, backward=backward)
            assert rows == [] and res.n_rows == 0 and res.done == 1, (lo, hi)
            assert res.rows_scanned == 0 and res.rows_matched == 0
            clamped = 65 if hi is None else min(hi, 65)
            assert res.resume_row == (lo if backward else clamped)


# ---- 4. paging -------------------------------------------------------------

def page_limits():
    return (1, 7, 64, 65, tile_rows() + 3)


def scenario_paging(run, limit, backward):
    T = tile_rows()
    n = 2 * T + 1
    case = edge_tablet(n)
    cols = all_cols(case["schema"])
    preds = sc.edge_query()[0]
    full, fraw, fres = run(case, sc.EDGE_READ, preds, cols)
    full_ids = ids_of(fraw, fres)
    assert fres.rows_matched == len(full) > limit
    got, got_ids = [], []
    lo, hi = 0, n
    pages = 0
    while True:
        rows, raw, res = run(case, sc.EDGE_READ, preds, cols, limit=limit,
                             backward=backward, row_lo=lo, row_hi=hi)
        pages += 1
        assert res.rows_matched == len(full) - len(got), pages
        assert res.rows_scanned == hi - lo
        assert res.n_rows == min(limit, res.rows_matched)
        got += rows
        got_ids += ids_of(raw, res)
        if res.done:
            assert res.n_rows == res.rows_matched
            assert res.resume_row == (lo if backward else hi)
            break
        assert res.n_rows == limit
        if backward:
            assert res.resume_row == got_ids[-1]
            hi = res.resume_row
        else:
            assert res.resume_row == got_ids[-1] + 1
            lo = res.resume_row
        assert pages <= len(full)
    assert pages == -(-len(full) // limit)
    if backward:
        got.reverse()
        got_ids.reverse()
    assert got_ids == full_ids
    assert got == full


# ---- 5. windows ------------------------------------------------------------

def scenario_windows(run):
    T = tile_rows()
    n = 2 * T + 1
    case = edge_tablet(n)
    cols = all_cols(case["schema"])
    preds = sc.edge_query()[0]
    full, fraw, fres = run(case, sc.EDGE_READ, preds, cols)
    full_ids = ids_of(fraw, fres)
    windows = [(1, n), (0, n - 2), (3, 2 * T - 1), (17, 17), (T - 1, T + 1),
               (T - 3, T + 4), (T, 2 * T), (2 * T - 1, n + 100), (5, None),
               (2 * T, None), (T + 1, T + 2)]
    for lo, hi in windows:
        chi = n if hi is None else min(hi, n)
        want = [(i, r) for i, r in zip(full_ids, full) if lo <= i < chi]
        for backward in (False, True):
            rows, raw, res = run(case, sc.EDGE_READ, preds, cols, row_lo=lo,
                                 row_hi=hi, backward=backward)
            w = want[::-1] if backward else want
            assert ids_of(raw, res) == [i for i, _ in w], (lo, hi, backward)
            assert rows == [r for _, r in w], (lo, hi, backward)
            assert res.rows_scanned == max(0, chi - lo)
            assert res.rows_matched == len(want) and res.done == 1
            assert res.resume_row == (lo if backward else chi)


# ---- 6. backward with limit ------------------------------------------------

def scenario_backward_limit(run):
    T = tile_rows()
    n = 2 * T + 1
    case = edge_tablet(n)
    cols = all_cols(case["schema"])
    preds = sc.edge_query()[0]
    full, fraw, fres = run(case, sc.EDGE_READ, preds, cols)
    full_ids = ids_of(fraw, fres)
    for k in (1, 2, 63, T + 1, len(full), len(full) + 5):
        rows, raw, res = run(case, sc.EDGE_READ, preds, cols, limit=k,
                             backward=True)
        kk = min(k, len(full))
        assert rows == full[::-1][:kk], k
        assert ids_of(raw, res) == full_ids[::-1][:kk]
        assert res.rows_matched == len(full)
        assert res.done == (1 if k >= len(full) else 0)
        # forward mirror: the first k
        rows, raw, res = run(case, sc.EDGE_READ, preds, cols, limit=k)
        assert rows == full[:kk] and ids_of(raw, res) == full_ids[:kk]


# ---- 7. projection ---------------------------------------------------------

def scenario_projection(run, cases):
    T = tile_rows()
    case = edge_tablet(T + 1)      # the double column is NULL every 3rd row
    preds = []
    # a single key column
    want = oracle_rows(case, sc.EDGE_READ, preds, [(1, 0)])
    check_full(run, case, sc.EDGE_READ, preds, [(1, 0)], want)
    # a repeated column, key and value mixed
    cols = [(0, 1), (1, 0), (0, 1), (0, 2), (0, 1)]
    want = oracle_rows(case, sc.EDGE_READ, preds, cols)
    _rows, raw, res = check_full(run, case, sc.EDGE_READ, preds, cols, want)
    datums, null_masks, _ids = raw
    cap = max(len(want), 1)
    for i in range(res.n_rows):
        # the NULL datum is 0; the mask holds the projected column's bit only
        if i % 3 == 0:
            assert null_masks[i] == 0b010
            assert datums[i] == datums[2 * cap + i] == datums[4 * cap + i] == 0
        else:
            assert null_masks[i] == 0
    # null_masks masked to the PROJECTED value columns: the NULL column left
    # out, the mask is 0 on every row
    cols = [(0, 0), (0, 2)]
    want = oracle_rows(case, sc.EDGE_READ, preds, cols)
    _rows, raw, res = check_full(run, case, sc.EDGE_READ, preds, cols, want)
    assert not any(raw[1][:res.n_rows])
    # nulls_packed: two NULL-carrying columns, one projected
    npk = next(c for c in cases if c["name"] == "nulls_packed")
    want = oracle_rows(npk, 1_000_000, [], [(0, 1)])
    _rows, raw, res = check_full(run, npk, 1_000_000, [], [(0, 1)], want)
    assert set(raw[1][:res.n_rows]) == {0, 0b10}
    # every YBG_MAX_SELECT_COLS slot filled, with repeats
    wide = next(c for c in cases if c["name"] == "wide_fixed_32cols")
    cols = [(0, c) for c in range(32)] + [(1, 0)] + \
           [(0, 31 - c) for c in range(y.MAX_SELECT_COLS - 33)]
    assert len(cols) == y.MAX_SELECT_COLS
    preds = [y.Pred(0, 16, y.PRED_GT, 20_000, None, 0)]
    want = oracle_rows(wide, 1_000_000, preds, cols)
    assert 0 < len(want) < 1500
    check_full(run, wide, 1_000_000, preds, cols, want)


# ---- 8. determinism --------------------------------------------------------

def scenario_determinism(fresh, cases):
    """fresh() -> a run on a separately built snapshot. Returns the raw
    bytes all four calls agree on."""
    case = next(c for c in cases if c["name"] == "mixed_types")
    read_micros, preds, _aggs = case["runs"][0]
    preds = list(preds)
    cols = all_cols(case["schema"])
    cap = 1 << 16
    seen = []
    for _ in range(2):
        run = fresh()
        for _ in range(2):
            _rows, raw, res = run(case, read_micros, preds, cols, cap=cap)
            assert res.n_rows > 0
            seen.append(raw_bytes(raw, res, len(cols), cap))
    assert all(s == seen[0] for s in seen[1:])
    return seen[0], (case, read_micros, preds, cols, cap)


# ---- 9. interleaving -------------------------------------------------------

def scenario_interleave(run, run_query, run_group):
    """run_query(case, read, preds, aggs) -> comparable plain result;
    run_group(case, read, preds, aggs, group_col) -> comparable groups."""
    T = tile_rows()
    case = edge_tablet(2 * T + 1)
    cols = all_cols(case["schema"])
    preds, aggs = sc.edge_query()
    in_preds = [key_in([3, T - 1, T, 2 * T])]

    def sel(p, **kw):
        rows, raw, res = run(case, sc.EDGE_READ, p, cols, **kw)
        return rows, ids_of(raw, res), res.rows_matched, res.resume_row

    alone = (sel(preds), run_query(case, sc.EDGE_READ, preds, aggs),
             run_group(case, sc.EDGE_READ, preds, aggs, 2),
             sel(in_preds, backward=True, limit=3),
             run_query(case, sc.EDGE_READ, in_preds, aggs))
    for _ in range(2):
        assert sel(in_preds, backward=True, limit=3) == alone[3]
        assert run_query(case, sc.EDGE_READ, preds, aggs) == alone[1]
        assert sel(preds) == alone[0]
        assert run_group(case, sc.EDGE_READ, preds, aggs, 2) == alone[2]
        assert sel(preds) == alone[0]
        assert run_query(case, sc.EDGE_READ, in_preds, aggs) == alone[4]
        assert run_group(case, sc.EDGE_READ, preds, aggs, 2) == alone[2]
        assert sel(in_preds, backward=True, limit=3) == alone[3]
    assert len(alone[3][0]) == 3 and alone[3][1] == [2 * T, T, T - 1]


# ---- 10. errors ------------------------------------------------------------

def error_cases(cases):
    """(label, case, read, preds, cols, message fragment)."""
    edge = edge_tablet(65)
    mixed = next(c for c in cases if c["name"] == "mixed_types")
    strk = next(c for c in cases if c["name"] == "in_list_string")
    streq = next(c for c in cases if c["name"] == "string_eq_pred")
    tup = next(c for c in cases if c["name"] == "in_tuple_keycols")
    R = 1_700_000_000_000_000
    over = [(0, 0)] * (y.MAX_SELECT_COLS + 1)
    return [
        ("string value column", mixed, R, [], [(0, 0), (0, 2)],
         "column 1: string column 2"),
        ("string key column", strk, R, [], [(1, 1)],
         "column 0: string key column 1"),
        ("value column out of range", edge, sc.EDGE_READ, [],
         [(0, 0), (0, 1), (0, 3)], "column 2: value column 3 out of range"),
        ("negative value column", edge, sc.EDGE_READ, [], [(0, -1)],
         "column 0: value column -1 out of range"),
        ("key column out of range", edge, sc.EDGE_READ, [], [(1, 1)],
         "column 0: key column 1 out of range"),
        ("num_cols 0", edge, sc.EDGE_READ, [], [], "num_cols 0"),
        ("num_cols over the cap", edge, sc.EDGE_READ, [], over,
         "num_cols %d over the cap %d" % (len(over), y.MAX_SELECT_COLS)),
        ("string predicate", streq, R, list(streq["runs"][0][1]), [(0, 1)],
         "predicate 0: string column 0"),
        ("IN_TUPLE", tup, R, list(tup["runs"][0][1]), [(0, 0)],
         "predicate 0: IN_TUPLE"),
    ]


def scenario_errors(run, cases, message=False):
    def valid(case, read_micros):
        cols = all_cols(case["schema"])
        want = oracle_rows(case, read_micros, [], cols)
        check_full(run, case, read_micros, [], cols, want)

    for label, case, read_micros, preds, cols, frag in error_cases(cases):
        with pytest.raises(RuntimeError) as ei:
            run(case, read_micros, preds, cols)
        assert ei.value.code == 9, (label, ei.value.code)
        if message:
            assert frag in str(ei.value), (label, str(ei.value))
        valid(case, read_micros)
    # cap one short: code 8, the count needed and the counters
    case = edge_tablet(65)
    cols = all_cols(case["schema"])
    preds = sc.edge_query()[0]
    want = oracle_rows(case, sc.EDGE_READ, preds, cols)
    assert len(want) > 1
    for kw, need in (({}, len(want)), ({"limit": 9}, 9),
                     ({"limit": 9, "backward": True}, 9)):
        with pytest.raises(RuntimeError) as ei:
            run(case, sc.EDGE_READ, preds, cols, cap=need - 1, **kw)
        assert ei.value.code == 8
        r = ei.value.result
        assert r.n_rows == need
        assert r.rows_matched == len(want) and r.rows_scanned == 65
        if message:
            assert "%d rows exceed the output capacity %d" % (
                need, need - 1) in str(ei.value)
        check_full(run, case, sc.EDGE_READ, preds, cols, want,
                   cap=len(want))
