"""Tablets and queries shared by test_fast_pipeline.py (host simulator) and
test_fast_pipeline_gpu.py: the fast scanner's trip order. A delta trip
issues the row's column loads and the next entry's window as soon as the
entry's lengths are known, before visibility is decided, so the smallest
shapes that can break it are entries whose value is not a full packed row
(the speculative column loads must not be issued, and their registers must
not carry over to the next row), version chains (the columns of an
invisible version must not be used), batches that abort after the early
issue, header lengths on both sides of the 16-byte window's on-demand
second half, and entry starts at every phase of a cache line.

walk() is a reference walk over the entry headers of a tablet (the forms
the fast scanner decodes; anything else skips to the next restart point),
so a test can assert that a tablet really holds the shape it names."""
import ctypes as C
import functools

import ybgpu as y
from scan_tail_cases import env, res_tuple  # noqa: F401
from wide_load_cases import val

I64, I32 = y.T_INT64, y.T_INT32
SUM, CNT, STAR = y.AGG_SUM_INT64, y.AGG_COUNT, y.AGG_COUNT_STAR
GT, GE, LT, LE = y.PRED_GT, y.PRED_GE, y.PRED_LT, y.PRED_LE
L4 = (I64,) * 4
MIXED = (I64, I32, I64, I64)
HT_BIG = 1_600_000_000_000_000


def _schema(key_types, col_types, has_hash=True):
    return y.make_schema(list(key_types),
                         [(10 + i, t, 1) for i, t in enumerate(col_types)],
                         has_hash=has_hash)


def _row(cols, r, salt=0):
    return [(t, (val(k, r) if t == I64 else r * 8 + k) + salt)
            for k, t in enumerate(cols)]


HEAD_Q = (((0, GE, val(0, 7)), (1, LT, val(1, 100000)), (2, GE, val(2, 3))),
          ((SUM, 3), (STAR, 0)))
COUNT_Q = ((), ((STAR, 0), (SUM, 0)))


def _tombs(rows, ri, last, plain=0):
    """Rows with tombstones in front of full rows. r % 3 == 0: a visible
    tombstone above the row (deleted); r % 7 == 3: a lone tombstone;
    r % 5 == 1: a tombstone above the read time in front of a visible
    row. last: 'tomb' ends the tablet on a lone tombstone, 'row' on a
    packed row. The first `plain` rows have no tombstone: they move the
    block boundaries against the pattern."""
    s = _schema((y.KT_INT64,), L4)
    b = y.Builder(s, restart_interval=ri)
    for r in range(rows):
        kw = dict(hash_=r // 64, key_datums=(r,))
        if r + 1 == rows and last == "tomb":
            b.add_row_tombstone(2000, **kw)
            break
        if r < plain:
            b.add_packed_row(2000, _row(L4, r), **kw)
            continue
        if r % 7 == 3 and r + 1 != rows:
            b.add_row_tombstone(3000, **kw)
            continue
        if r % 5 == 1:
            b.add_row_tombstone(9000, **kw)
        if r % 3 == 0 and r + 1 != rows:
            b.add_row_tombstone(3000, **kw)
        b.add_packed_row(2000, _row(L4, r), **kw)
    return s, b.finish(), HEAD_Q[0], HEAD_Q[1], (5000,)


def _chains(nver, ri, first_visible, rows=240, cols=L4, q=HEAD_Q):
    """nver versions per row at 1000 * (nver .. 1); the read time makes
    version number first_visible (0 = newest) the first visible one, nver =
    nothing visible."""
    s = _schema((y.KT_INT64,), cols)
    b = y.Builder(s, restart_interval=ri)
    for r in range(rows):
        for v in range(nver):
            ht = 1000 * (nver - v)
            b.add_packed_row(ht, _row(cols, r, salt=ht), hash_=r // 64,
                             key_datums=(r,))
    return s, b.finish(), q[0], q[1], (1000 * (nver - first_visible) + 500,)


def _late_abort(kind):
    """Batches that abort after the early issue: a column update (check 22),
    a hybrid time of 16 bytes or more (check 20), a V1 packed row or a row
    with a NULL (check 24), in the middle of intervals."""
    s = _schema((y.KT_INT64,), L4)
    b = y.Builder(s)
    for r in range(600):
        kw = dict(hash_=r // 64, key_datums=(r,))
        odd = r % 37 == 20
        if kind == "colupdate" and odd:
            b.add_column_update(3000, 2, r + 5, **kw)
        if kind == "ht16" and odd:
            b.add_packed_row(HT_BIG, _row(L4, r), write_id=1 << 30,
                             logical=4095, **kw)
        elif kind == "v1" and odd:
            b.add_packed_row(2000, _row(L4, r), packed_version=1, **kw)
        elif kind == "null" and odd:
            row = _row(L4, r)
            row[1] = (I64, None)
            b.add_packed_row(2000, row, **kw)
        else:
            b.add_packed_row(2000, _row(L4, r), **kw)
    read = (HT_BIG + 10,) if kind == "ht16" else (5000,)
    # (as in fast_header_cases.py the update is written in front of its row,
    # which is out of key order, so the query leaves the updated column
    # alone)
    return s, b.finish(), HEAD_Q[0][:2], HEAD_Q[1], read


def _headers(kind):
    """Header lengths nb = hl + ns1 + ns2 through key shapes: how many key
    bytes change between neighbours and how long the hybrid time is."""
    K2 = (y.KT_INT64, y.KT_INT64)
    K3 = (y.KT_INT64, y.KT_INT64, y.KT_INT32)
    K1 = (y.KT_INT64,)
    # kind: (key types, key datums of row r, write id, hybrid time of row r,
    # column types); the delta entries' nb measured by walk() in brackets
    kts, step, wid, ht, cols = {
        # one-microsecond steps [8, 11, 19]
        "ht_unit": (K1, lambda r: (r,), 0, lambda r: 1000 + r, L4),
        # millisecond steps of a long hybrid time [11, 12, 20]
        "ht_step": (K1, lambda r: (r,), 0, lambda r: HT_BIG + r * 1000, L4),
        # the same with a write id, and an INT32 column [13, 14, 22]: both
        # sides of the window's second half
        "ht_step_wid": (K1, lambda r: (r,), 70000,
                        lambda r: HT_BIG + r * 1000, MIXED),
        # a key carry every row, one hybrid time [21, 23, 24]
        "carry": (K1, lambda r: (r * 256 + 255,), 0, lambda r: 1000, L4),
        # both key columns change [16, 17, 25]: 25 aborts at check 16
        "two_keys_both": (K2, lambda r: (r, r << 40), 0,
                          lambda r: HT_BIG + r * 1000, L4),
        # three key columns, a long write id [24, 26, 29]
        "three_keys": (K3, lambda r: (r // 9, ((r // 3) % 3) << 58,
                                      (r % 3) << 28), 1 << 20,
                       lambda r: HT_BIG, L4),
    }[kind]
    s = _schema(kts, cols)
    b = y.Builder(s)
    for r in range(300):
        b.add_packed_row(ht(r), _row(cols, r), hash_=r // 128,
                         key_datums=step(r), write_id=wid)
    q = HEAD_Q if cols == L4 else (((0, GE, val(0, 7)),),
                                   ((SUM, 2), (SUM, 3)))
    return s, b.finish(), q[0], q[1], (HT_BIG + 10**9,)


# (18 plain rows put the end of the second block on a tombstone)
TOMB_CASES = {"tomb_last_tomb_ri16": (331, 16, "tomb", 18),
              "tomb_last_row_ri16": (330, 16, "row"),
              "tomb_last_tomb_ri1": (150, 1, "tomb"),
              "tomb_last_row_ri3": (331, 3, "row")}
CHAIN_CASES = dict(
    [("chain3_v%d_ri%d" % (v, ri), (3, ri, v)) for v in range(4)
     for ri in (2, 16)] +
    [("chain5_v%d_ri%d" % (v, ri), (5, ri, v)) for v in range(6)
     for ri in (3, 16)])
ABORT_CASES = ("colupdate", "ht16", "v1", "null")
HEADER_CASES = ("ht_unit", "ht_step", "ht_step_wid", "carry",
                "two_keys_both", "three_keys")
CASES = tuple(TOMB_CASES) + tuple(CHAIN_CASES) + tuple(
    "abort_" + k for k in ABORT_CASES) + tuple(
        "hdr_" + k for k in HEADER_CASES) + ("chain3_mixed_count",)


@functools.lru_cache(maxsize=None)
def case(name):
    """(schema, built, preds, aggs, read)."""
    if name in TOMB_CASES:
        return _tombs(*TOMB_CASES[name])
    if name in CHAIN_CASES:
        return _chains(*CHAIN_CASES[name])
    if name == "chain3_mixed_count":
        # the two-list plan form (operand loads apart from the range loads)
        return _chains(3, 16, 1, cols=MIXED, q=COUNT_Q)
    kind, _, arg = name.partition("_")
    return _late_abort(arg) if kind == "abort" else _headers(arg)


def specs(name, expect_versions=0):
    schema, _, preds, aggs, read = case(name)
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(*read)
    spec.expect_versions = expect_versions
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(*read)
    spec.num_preds = ospec.num_preds = len(preds)
    for i, (col, op, c) in enumerate(preds):
        c &= (1 << 64) - 1
        spec.preds[i] = y.Pred(0, col, op, c, None, 0)
        ospec.preds[i] = y.OrclPred(0, col, op, c, None, 0)
    spec.num_aggs = ospec.num_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        spec.aggs[i] = y.Agg(op, col)
        ospec.aggs[i] = y.OrclAgg(op, col)
    return spec, ospec


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's result tuple, computed once per case."""
    schema, built, _, aggs, _ = case(name)
    _, ospec = specs(name)
    ores, _ = y.orcl_scan(built[0], built[1], built[2],
                          y.orcl_schema_from(schema), ospec)
    return res_tuple(ores, len(aggs))


def sim_fast(name, expect_versions=0):
    """(result tuple, fallback batches) under the current environment."""
    _, built, _, aggs, _ = case(name)
    spec, _ = specs(name, expect_versions)
    r, nf = y.sim_scan_fast(spec, built[0], built[1], built[2])
    return res_tuple(r, len(aggs)), nf


def sim_general(name):
    _, built, _, aggs, _ = case(name)
    spec, _ = specs(name)
    return res_tuple(y.sim_scan(spec, built[0], built[1], built[2]),
                     len(aggs))


@functools.lru_cache(maxsize=None)
def walk(name):
    """Entries of the tablet as (offset in the buffer, kind, nb, value size,
    last of its block), kind 'restart' or 'delta'; nb is the header and key
    bytes in front of the value. Follows block_builder_internal.h for the
    forms the fast scanner decodes and skips to the next restart point at
    any other."""
    _, built, *_ = case(name)
    data, offsets, n_blocks, total = built[0], built[1], built[2], built[3]
    buf = C.string_at(data, total)
    out = []
    for bi in range(n_blocks):
        lo, hi = offsets[bi], offsets[bi + 1]
        nr = int.from_bytes(buf[hi - 4:hi], "little")
        ra = hi - 4 - 4 * nr
        starts = [int.from_bytes(buf[ra + 4 * i:ra + 4 * i + 4], "little")
                  for i in range(nr)] + [ra - lo]
        for i in range(nr):
            p, end, first = lo + starts[i], lo + starts[i + 1], True
            while p < end:
                e1, n = buf[p], 1
                if e1 & 0x80:
                    e1, n = (e1 & 0x7f) | (buf[p + 1] << 7), 2
                vs = e1 >> 2
                if first:
                    if (e1 & 1) or (buf[p + n] & 1) or buf[p + n] == 0:
                        break
                    nb = n + 1 + (buf[p + n] >> 1)
                elif e1 & 1:
                    nb = n + 1 + 2
                else:
                    e2 = buf[p + n]
                    if (e2 & 3) == 1 and not e2 & 4:
                        nb = n + 2 + ((e2 >> 3) & 7) + ((e2 >> 6) & 3)
                    elif (e2 & 7) == 7 and not e2 & 40:
                        o = n + 1
                        ns1 = buf[p + o]
                        o += 1
                        ns2 = 0
                        if e2 & 16:
                            ns2 = buf[p + o]
                            o += 1
                        nb = o + 1 + ns1 + ns2
                    else:
                        break
                out.append([p, "restart" if first else "delta", nb, vs,
                            False])
                first = False
                p += nb + vs
            if i + 1 == nr and out and p == end:
                out[-1][4] = True
    return tuple(tuple(e) for e in out)
