"""The planned fast kernel on the GPU: YBG_PLAN=1 (planned kernel),
YBG_PLAN=0 (interpreted fast kernel), YBG_FAST=0 (general kernel) and the
CPU oracle must agree bit for bit, and yb_gpu_scan_planned must say which
kernel ran."""
import functools
import os

import pytest

import ybgpu as y

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
MODES = (("plan", {"YBG_PLAN": "1"}, True),
         ("interpreted", {"YBG_PLAN": "0"}, False),
         ("general", {"YBG_FAST": "0"}, False))


def _u64(v):
    return v & ((1 << 64) - 1)


def _res(r, na):
    return (r.entries_seen, r.rows_scanned, r.rows_matched,
            tuple((r.aggs[i].is_null,
                   None if r.aggs[i].is_null else r.aggs[i].value_i64)
                  for i in range(na)),
            bytes(r.restart_ht[:r.restart_ht_len]))


@functools.lru_cache(maxsize=None)
def _tablet():
    """20 000 rows of 4 int64 columns: ~1 250 restart intervals, several
    workgroups."""
    schema = y.make_schema([y.KT_INT64],
                           [(10 + i, y.T_INT64, 1) for i in range(4)])
    return schema, y.generate(schema, rows=20000, seed=42, versions=1)


@functools.lru_cache(maxsize=None)
def _tablet_mvcc():
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


def _specs(schema, preds, aggs, read, expect_versions=0):
    """(GPU spec, oracle spec) for value-column predicates (col, op, c)."""
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(*read)
    spec.expect_versions = expect_versions
    ospec = y.OrclScanSpec()
    ospec.read_time = y.orcl_read_time(*read)
    spec.num_preds = ospec.num_preds = len(preds)
    for i, (col, op, c) in enumerate(preds):
        spec.preds[i] = y.Pred(0, col, op, _u64(c), None, 0)
        ospec.preds[i] = y.OrclPred(0, col, op, _u64(c), None, 0)
    spec.num_aggs = ospec.num_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        spec.aggs[i] = y.Agg(op, col)
        ospec.aggs[i] = y.OrclAgg(op, col)
    return spec, ospec


def _gpu(spec, built, env, na, executes=1):
    """Run under env; returns ([result tuple per execute], planned flag)."""
    from gpu_scan import GpuScan
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = GpuScan(spec)
        try:
            s.feed_blocks_host(built[0], built[1], built[2], built[3])
            outs = []
            for _ in range(executes):
                s.execute()
                outs.append(_res(s.aggregates(), na))
            return outs, s.planned()
        finally:
            s.close()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check_all_modes(schema, built, preds, aggs, read, expect_versions=0,
                     plannable=True):
    spec, ospec = _specs(schema, preds, aggs, read, expect_versions)
    na = len(aggs)
    ores, _ = y.orcl_scan(built[0], built[1], built[2],
                          y.orcl_schema_from(schema), ospec)
    want = _res(ores, na)
    for name, env, says_plan in MODES:
        (got,), planned = _gpu(spec, built, env, na)
        assert planned == (says_plan and plannable), name
        # entries, rows, aggregates with their null flags and restart bytes
        # against the oracle; the three GPU modes are then equal to each
        # other too
        assert got == want, name
    return want


HEADLINE = [(0, y.PRED_GT, 1 << 39), (1, y.PRED_LT, 3 << 38),
            (2, y.PRED_GE, 1 << 36)]
SUM3 = [(y.AGG_SUM_INT64, 3), (y.AGG_COUNT_STAR, 0)]
READ = (1_700_000_000_000_000,)


@pytest.mark.parametrize("preds,aggs", [
    (HEADLINE, SUM3),
    # empty ranges: an unsatisfiable pair, and the two saturating constants
    ([(0, y.PRED_GT, 1 << 39), (0, y.PRED_LT, 1 << 38)], SUM3),
    ([(1, y.PRED_GT, I64_MAX)], SUM3),
    ([(1, y.PRED_LT, I64_MIN)], SUM3),
    # no predicates
    ([], SUM3),
    ([], [(y.AGG_COUNT_STAR, 0)]),
    # predicate and aggregate on one column; a single point that matches
    # nothing in random data; four ranged columns
    ([(3, y.PRED_LE, 1 << 39)], [(y.AGG_SUM_INT64, 3), (y.AGG_COUNT, 3)]),
    ([(2, y.PRED_GE, 12345), (2, y.PRED_LE, 12345)], SUM3),
    (HEADLINE + [(3, y.PRED_GT, 1 << 30)], SUM3),
])
def test_plan_gpu_modes_agree(preds, aggs):
    schema, built = _tablet()
    want = _check_all_modes(schema, built, preds, aggs, READ)
    if preds == HEADLINE:
        assert 0 < want[2] < want[1]  # the headline filter really filters


@pytest.mark.parametrize("expect_versions", [0, 1])
@pytest.mark.parametrize("read", [(2500, 3500, 4500), (1500, 1500, 1500),
                                  (500, 900, 1200)])
def test_plan_gpu_mvcc(expect_versions, read):
    schema, built = _tablet_mvcc()
    _check_all_modes(schema, built, [(0, y.PRED_GT, 100)],
                     [(y.AGG_COUNT_STAR, 0), (y.AGG_SUM_INT64, 0)], read,
                     expect_versions)


def test_plan_gpu_two_executes_identical():
    schema, built = _tablet()
    spec, _ = _specs(schema, HEADLINE, SUM3, READ)
    outs, planned = _gpu(spec, built, {"YBG_PLAN": "1"}, 2, executes=2)
    assert planned
    assert outs[0] == outs[1]


def test_plan_gpu_ne_predicate_not_planned():
    schema, built = _tablet()
    _check_all_modes(schema, built,
                     [(0, y.PRED_GT, 1 << 39), (1, y.PRED_NE, 12345)], SUM3,
                     READ, plannable=False)
