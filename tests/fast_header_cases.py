"""Tablets and specs shared by test_fast_header.py (host simulator) and
test_fast_header_gpu.py: the smallest shapes at which the fast kernel's
entry-header reads (whatever loads them: the register window today) and
its shuffle epilogue can go wrong.

Row counts put the last entry of an interval, of a block and of the tablet
directly before the buffer's tail slack and produce one-entry intervals
(the four-column schema fills a 4 KB block at 91-93 rows); the 2 000 and
6 000-row tablets change the hash at every row, so every delta entry is the
general form with ns1 = 10, and the 200 000-row tablet changes it every
third row, so general-form entries mix with case 2.1.1 inside one wave (the
generator spreads 65 536 hash values over the rows); the one-column schema
has a value shorter than 16 bytes and a one-byte first header varint; five
versions per
row give skipped versions, rows with nothing visible and the fused
extraction shape; the builder tablets abort batches to the general kernel;
restart interval 1 makes the batch count equal the row count, for idle
lanes, idle waves and a wave boundary at every position of the epilogue."""
import functools

import ybgpu as y
from scan_tail_cases import HEADLINE, env, res_tuple  # noqa: F401

ROW_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 90, 91, 92, 93, 94,
              182, 183, 184, 185, 186, 2000, 6000)
MIXED_ROWS = 200_000  # four-column schema only
MVCC_ROWS = (1, 17, 33, 93, 2000)
EPILOGUE_BATCHES = (1, 63, 64, 65, 255, 256, 257)

MVCC_BASE = 1_600_000_000_000_000
MVCC_READ = (MVCC_BASE + 2_500_000,)  # the benchmark's mvcc read time
BELOW_READ = (MVCC_BASE - 1,)         # below every version
I64_MAX = (1 << 63) - 1


def _schema(ncols):
    return y.make_schema([y.KT_INT64],
                         [(10 + i, y.T_INT64, 1) for i in range(ncols)])


SUM3 = ((y.AGG_SUM_INT64, 3), (y.AGG_COUNT_STAR, 0))
COUNT_SUM0 = ((y.AGG_COUNT_STAR, 0), (y.AGG_SUM_INT64, 0))
ONE_PRED = ((0, y.PRED_GT, 1 << 39),)


def _names():
    out = []
    for n in ROW_COUNTS:
        out.append("c4_%d" % n)
        out.append("c1_%d" % n)
    out.append("c4_%d" % MIXED_ROWS)
    for n in MVCC_ROWS:
        out.append("mvcc_%d" % n)
        out.append("mvccbelow_%d" % n)
    out += ["tombstones", "colupdate"]
    out += ["epi_%d" % n for n in EPILOGUE_BATCHES]
    out += ["epi_restart_one"]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(name):
    """(schema, built, preds, aggs, read, expect_versions)."""
    kind, _, arg = name.partition("_")
    if kind == "c4":
        s = _schema(4)
        return (s, y.generate(s, rows=int(arg), seed=42, versions=1),
                tuple(HEADLINE), SUM3, (1_700_000_000_000_000,), 0)
    if kind == "c1":
        s = _schema(1)
        return (s, y.generate(s, rows=int(arg), seed=42, versions=1),
                ONE_PRED, COUNT_SUM0, (1_700_000_000_000_000,), 0)
    if kind in ("mvcc", "mvccbelow"):
        s = _schema(4)
        built = y.generate(s, rows=int(arg), seed=42, versions=5,
                           ht_base_micros=MVCC_BASE,
                           ht_step_micros=1_000_000)
        return (s, built, (), COUNT_SUM0,
                MVCC_READ if kind == "mvcc" else BELOW_READ, 1)
    if name == "tombstones":
        # every 5th row's newest version is a row tombstone, every 7th row
        # is a lone tombstone: row exists / deleted / never visible
        s = _schema(1)
        b = y.Builder(s)
        for r in range(700):
            if r % 7 == 3:
                b.add_row_tombstone(3000, hash_=r // 64, key_datums=(r,))
                continue
            if r % 5 == 0:
                b.add_row_tombstone(3000, hash_=r // 64, key_datums=(r,))
            b.add_packed_row(2000, [(y.T_INT64, r * 11 + 1)],
                             hash_=r // 64, key_datums=(r,))
        return (s, b.finish(), ((0, y.PRED_GT, 50),), COUNT_SUM0, (5000,), 0)
    if name == "colupdate":
        # column updates in the middle of batches: those batches abort to
        # the general kernel, the neighbours' heads and walks must agree
        s = _schema(4)
        b = y.Builder(s)
        for r in range(600):
            if r % 37 == 20:
                b.add_column_update(3000, 2, r + 5, hash_=r // 64,
                                    key_datums=(r,))
            b.add_packed_row(2000, [(y.T_INT64, r * 3 + k) for k in range(4)],
                             hash_=r // 64, key_datums=(r,))
        return (s, b.finish(), ((0, y.PRED_GE, 30),), SUM3, (5000,), 0)
    if name == "epi_restart_one":
        # track_restart on (local limit above the read time) and exactly one
        # record in (read, local]: one lane of one wave holds a candidate
        s = _schema(1)
        b = y.Builder(s, restart_interval=1)
        for r in range(200):
            b.add_packed_row(3000 if r == 137 else 1000,
                             [(y.T_INT64, r)], hash_=r // 64,
                             key_datums=(r,))
        return (s, b.finish(), (), COUNT_SUM0, (2000, 4000, 4000), 0)
    assert kind == "epi"
    # one batch per row (restart interval 1, YBG_IVB=1); operands near
    # INT64_MAX so the sum wraps and the wrapped bits are what is compared
    s = _schema(1)
    b = y.Builder(s, restart_interval=1)
    for r in range(int(arg)):
        b.add_packed_row(1000, [(y.T_INT64, I64_MAX - r * 3)],
                         hash_=r // 64, key_datums=(r,))
    return (s, b.finish(), (), COUNT_SUM0, (5000,), 0)


CASES = _names()


def specs(name, expect_versions=None):
    schema, _, preds, aggs, read, ev = case(name)
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(*read)
    spec.expect_versions = ev if expect_versions is None else expect_versions
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
    """The oracle's result tuple, computed once per case."""
    schema, built, _, aggs, _, _ = case(name)
    _, ospec = specs(name)
    ores, _ = y.orcl_scan(built[0], built[1], built[2],
                          y.orcl_schema_from(schema), ospec)
    return res_tuple(ores, len(aggs))


def sim_fast(name, expect_versions=None):
    """(result tuple, fallback batches) under the current environment."""
    _, built, _, aggs, _, _ = case(name)
    spec, _ = specs(name, expect_versions)
    r, nf = y.sim_scan_fast(spec, built[0], built[1], built[2])
    return res_tuple(r, len(aggs)), nf


def sim_general(name):
    _, built, _, aggs, _, _ = case(name)
    spec, _ = specs(name)
    return res_tuple(y.sim_scan(spec, built[0], built[1], built[2]),
                     len(aggs))
