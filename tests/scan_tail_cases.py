"""Tablets, specs and helpers shared by test_scan_tail.py (host simulator)
and test_scan_tail_gpu.py: four tablets whose batches abort sometimes,
never, in the middle of version chains and nearly always."""
import functools
import os

import ybgpu as y

HEADLINE = [(0, y.PRED_GT, 1 << 39), (1, y.PRED_LT, 3 << 38),
            (2, y.PRED_GE, 1 << 36)]


def res_tuple(r, na):
    return (r.entries_seen, r.rows_scanned, r.rows_matched,
            tuple((r.aggs[i].is_null,
                   None if r.aggs[i].is_null else r.aggs[i].value_i64)
                  for i in range(na)),
            bytes(r.restart_ht[:r.restart_ht_len]))


def _schema4():
    return y.make_schema([y.KT_INT64],
                         [(10 + i, y.T_INT64, 1) for i in range(4)])


@functools.lru_cache(maxsize=None)
def tablet(name):
    """(schema, built, preds, aggs, read) of the four tablets."""
    count_sum0 = [(y.AGG_COUNT_STAR, 0), (y.AGG_SUM_INT64, 0)]
    if name == "single":  # 1 250 intervals, a few aborts (code 15)
        schema = _schema4()
        return (schema, y.generate(schema, rows=20000, seed=42, versions=1),
                HEADLINE, [(y.AGG_SUM_INT64, 3), (y.AGG_COUNT_STAR, 0)],
                (1_700_000_000_000_000,))
    if name == "chains":  # no aborts; heads walked into at every boundary
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
        return (schema, b.finish(), [(0, y.PRED_GT, 100)], count_sum0,
                (2500, 3500, 4500))
    if name == "chains_few":  # aborts in the middle of version chains
        schema = _schema4()
        return (schema, y.generate(schema, rows=6000, seed=7, versions=3,
                                   ht_step_micros=1000),
                [], count_sum0, (1_600_000_000_001_500,))
    assert name == "all_abort"  # every batch aborts (code 16)
    schema = _schema4()
    return (schema, y.generate(schema, rows=6000, seed=42, versions=5,
                               ht_step_micros=1_000_000),
            [], count_sum0, (1_600_000_002_500_000,))


TABLETS = ("single", "chains", "chains_few", "all_abort")


def specs(name, expect_versions):
    schema, _, preds, aggs, read = tablet(name)
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(*read)
    spec.expect_versions = expect_versions
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(*read)
    spec.num_preds = ospec.num_preds = len(preds)
    for i, (col, op, c) in enumerate(preds):
        spec.preds[i] = y.Pred(0, col, op, c, None, 0)
        ospec.preds[i] = y.OrclPred(0, col, op, c, None, 0)
    spec.num_aggs = ospec.num_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        spec.aggs[i] = y.Agg(op, col)
        ospec.aggs[i] = y.OrclAgg(op, col)
    return spec, ospec


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's result tuple, computed once per tablet."""
    schema, built, _, aggs, _ = tablet(name)
    _, ospec = specs(name, 0)
    ores, _ = y.orcl_scan(built[0], built[1], built[2],
                          y.orcl_schema_from(schema), ospec)
    return res_tuple(ores, len(aggs))


class env:
    """Set environment knobs for a block; None unsets."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def sim_fast(name, expect_versions):
    """(result tuple, fallback batches) under the current environment."""
    _, built, _, aggs, _ = tablet(name)
    spec, _ = specs(name, expect_versions)
    r, nf = y.sim_scan_fast(spec, built[0], built[1], built[2])
    return res_tuple(r, len(aggs)), nf
