"""Tablets and queries shared by test_wide_loads.py (host simulator) and
test_wide_loads_gpu.py: the column plan's load groups and the restart
decode's 16-byte key chunks, at the smallest shapes at which either can go
wrong.

Plan cases. Value column k of row r holds (k << 40) + r * 8 + k (an INT32
column r * 8 + k), and every range names its own column's band, so a range
or a SUM that reads the wrong half of a 16-byte group, or the wrong group,
changes the result. Each case names the plan shape it must compile to
(ybgpu.sim_plan_shape): 0..4 / 8 ranged columns of the two-list form, or a
grouped shape.

Restart cases. The restart key length ns1 is rkb + 1 + ht_sz + 8, with rkb
= 5 + 9 per INT64 key + 5 per INT32 key (1 + ... without a hash column)
and ht_sz from the hybrid time and write id, so key schemas and write ids
place ns1 on both sides of every boundary of the chunked copy: two chunks
up to 32, a third up to 48, the loop past 48 with a second trip past 64,
the shortest key the fast path takes, the longest (72) and one above it
that aborts. Each case names the ns1 the census must report. rkb is a
multiple of 8 in k48 (24), k52 (32) and k72 (40) — the row compare ends on
a whole word — and is not in the others (6, 10, 14, 19, ...), where its
last word is masked. restart_interval 1 makes every entry a restart entry,
the last of each block and of the tablet included; 2 lets a version chain
continue across a restart and change at one; 16 with 16 k + 1 rows ends
the tablet on a restart entry."""
import functools

import ybgpu as y
from scan_tail_cases import env, res_tuple  # noqa: F401

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
READ = (5000,)


def val(k, r):
    return (k << 40) + r * 8 + k


def _schema(key_types, col_types, has_hash=True):
    return y.make_schema(list(key_types),
                         [(10 + i, t, 1) for i, t in enumerate(col_types)],
                         has_hash=has_hash)


def _rows(schema, key_types, col_types, rows, restart_interval=16, ht=1000,
          write_id=0, values=None):
    b = y.Builder(schema, restart_interval=restart_interval)
    for r in range(rows):
        vs = values(r) if values else [
            (t, val(k, r) if t == y.T_INT64 else r * 8 + k)
            for k, t in enumerate(col_types)]
        b.add_packed_row(ht, vs, hash_=r // 64,
                         key_datums=(7,) * (len(key_types) - 1) + (r,),
                         write_id=write_id)
    return b.finish()


L4 = (y.T_INT64,) * 4
L8 = (y.T_INT64,) * 8
MIXED = (y.T_INT64, y.T_INT32, y.T_INT64, y.T_INT64)
K1 = (y.KT_INT64,)
N = 700  # eight blocks of the four-column schema

SUM, CNT, STAR = y.AGG_SUM_INT64, y.AGG_COUNT, y.AGG_COUNT_STAR
GT, GE, LT, LE, EQ = (y.PRED_GT, y.PRED_GE, y.PRED_LT, y.PRED_LE, y.PRED_EQ)

# name: (column types, preds, aggs, plan shape)
PLAN_CASES = {
    "headline": (L4, ((0, GT, val(0, 10)), (1, LT, val(1, N - 10)),
                      (2, GE, val(2, 20))), ((SUM, 3), (STAR, 0)),
                 y.PLAN_SHAPE_TWO_PAIRS),
    "gap_two_singles": (MIXED, ((0, GE, val(0, 30)),), ((SUM, 2), (STAR, 0)),
                        1),
    "pair_odd_offset": (MIXED, ((2, GE, val(2, 30)),), ((SUM, 3), (STAR, 0)),
                        y.PLAN_SHAPE_PAIR),
    "three_adjacent": (L4, ((0, GE, val(0, 5)), (1, LE, val(1, N - 7))),
                       ((SUM, 2), (STAR, 0)), y.PLAN_SHAPE_PAIR_SINGLE),
    "ranged_and_summed": (L4, ((3, GE, val(3, 40)),), ((SUM, 3), (STAR, 0)),
                          1),
    "ranged_and_summed_pair": (L4, ((2, LT, val(2, N - 3)),
                                    (3, GE, val(3, 40))),
                               ((SUM, 3), (CNT, 2)), y.PLAN_SHAPE_PAIR),
    "count_only": (L4, (), ((STAR, 0), (CNT, 1)), 0),
    "count_one_pred": (L4, ((1, GE, val(1, 100)),), ((STAR, 0), (CNT, 1)), 1),
    "sum_only_pair": (L4, (), ((SUM, 2), (SUM, 3)), y.PLAN_SHAPE_PAIR),
    "eight_ranged": (L8, tuple((k, GE, val(k, 3 + k)) for k in range(8)),
                     ((SUM, 7), (STAR, 0)), 8),
    "five_ranged": (L8, tuple((k, LE, val(k, N - 4 - k))
                              for k in (0, 2, 4, 6, 7)),
                    ((SUM, 7), (SUM, 1)), 8),
    "descending_preds": (L4, ((2, GE, val(2, 20)), (1, LT, val(1, N - 10)),
                              (0, GT, val(0, 10))), ((SUM, 3), (STAR, 0)),
                         y.PLAN_SHAPE_TWO_PAIRS),
    "two_preds_one_column": (L4, ((1, GE, val(1, 50)), (1, LE, val(1, 600))),
                             ((SUM, 0), (STAR, 0)), y.PLAN_SHAPE_PAIR),
    "unsatisfiable": (L4, ((0, GT, val(0, 300)), (0, LT, val(0, 300))),
                      ((SUM, 1), (STAR, 0)), y.PLAN_SHAPE_PAIR),
    # extremes(): INT64_MIN / INT64_MAX in each half of the pair
    "extremes_low_half": (L4, ((0, LE, -1), (1, GE, 1)),
                          ((SUM, 0), (SUM, 1)), y.PLAN_SHAPE_PAIR),
    "extremes_high_half": (L4, ((0, GE, 1), (1, LE, -1)),
                           ((SUM, 1), (SUM, 2)), y.PLAN_SHAPE_PAIR_SINGLE),
    "sum_last_column": (L8, ((6, GE, val(6, 9)),), ((SUM, 7), (STAR, 0)),
                        y.PLAN_SHAPE_PAIR),
}


def extremes(r):
    a = (I64_MIN, I64_MAX, I64_MIN, I64_MAX)[r % 4]
    b = (I64_MAX, I64_MIN, I64_MIN, I64_MAX)[r % 4]
    return [(y.T_INT64, a), (y.T_INT64, b), (y.T_INT64, val(2, r)),
            (y.T_INT64, val(3, r))]


HT_BIG = 1_600_000_000_000_000
I64K, I32K = y.KT_INT64, y.KT_INT32
# name: (key types, has_hash, ht, write id, ns1; 0 = every batch aborts)
KEY_CASES = {
    "k_shortest": ((I32K,), False, HT_BIG, 0, 25),
    "k29": ((I32K,), True, HT_BIG, 0, 29),
    "k31": ((I32K,), True, HT_BIG, 300, 31),
    "k32": ((I32K,), True, HT_BIG, 1 << 20, 32),
    "k33": ((I64K,), True, HT_BIG, 0, 33),
    "k34": ((I64K,), True, 1000, 0, 34),
    "k47": ((I64K, I64K, I32K), True, HT_BIG, 0, 47),
    "k48": ((I64K, I32K, I32K, I32K), True, HT_BIG, 0, 48),
    "k49": ((I64K, I32K, I32K, I32K), True, 1000, 0, 49),
    "k52": ((I64K, I64K, I64K), True, 1000, 0, 52),
    "k63": ((I64K,) + (I32K,) * 6, True, HT_BIG, 0, 63),
    "k64": ((I64K,) + (I32K,) * 6, True, 1000, 0, 64),
    "k65": ((I64K,) + (I32K,) * 6, True, 1000, 1, 65),
    "k72": ((I64K,) * 3 + (I32K,) * 4, True, 1000, 0, 72),
    "k_too_long": ((I64K,) * 4 + (I32K,) * 3, True, 1000, 0, 0),
}
KEY_ROWS = 150
KEY_QUERY = (((0, GE, val(0, 7)),), ((SUM, 1), (STAR, 0)))

# name: restart interval; rows with tombstones and three-version chains
CHAIN_CASES = {"tomb_ri1": 1, "tomb_ri16": 16, "chains_ri1": 1,
               "chains_ri2": 2, "last_restart_ri16": 16}

CASES = tuple(PLAN_CASES) + tuple(
    "%s_ri%d" % (k, ri) for k in KEY_CASES for ri in (1, 16)) + tuple(
        CHAIN_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(schema, built, preds, aggs, read)."""
    if name in PLAN_CASES:
        cols, preds, aggs, _ = PLAN_CASES[name]
        s = _schema(K1, cols)
        values = extremes if name.startswith("extremes") else None
        return s, _rows(s, K1, cols, N, values=values), preds, aggs, READ
    if name in CHAIN_CASES:
        ri = CHAIN_CASES[name]
        s = _schema(K1, L4)
        b = y.Builder(s, restart_interval=ri)
        rows = 16 * 20 + 1 if name == "last_restart_ri16" else 400
        for r in range(rows):
            kw = dict(hash_=r // 64, key_datums=(r,))
            row = [(y.T_INT64, val(k, r)) for k in range(4)]
            if name.startswith("tomb"):
                # hl = 2 restart entries (one-byte value) next to hl = 3
                if r % 7 == 3:
                    b.add_row_tombstone(3000, **kw)
                    continue
                if r % 3 == 0:
                    b.add_row_tombstone(3000, **kw)
                b.add_packed_row(2000, row, **kw)
            elif name.startswith("chains"):
                for ht in (3000, 2000, 1000):
                    b.add_packed_row(
                        ht, [(t, v + ht) for t, v in row], **kw)
            else:
                b.add_packed_row(1000, row, **kw)
        read = (2500,) if name.startswith("chains") else READ
        return (s, b.finish(), ((0, GE, val(0, 7)), (1, LT, val(1, 390))),
                ((SUM, 3), (STAR, 0)), read)
    key, _, ri = name.rpartition("_ri")
    kts, has_hash, ht, wid, _ = KEY_CASES[key]
    cols = (y.T_INT64, y.T_INT64)
    s = _schema(kts, cols, has_hash=has_hash)
    built = _rows(s, kts, cols, KEY_ROWS, restart_interval=int(ri), ht=ht,
                  write_id=wid)
    return s, built, KEY_QUERY[0], KEY_QUERY[1], (ht + 10,)


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


def census(name):
    _, built, *_ = case(name)
    return y.sim_fast_census(specs(name)[0], built[0], built[1], built[2])
