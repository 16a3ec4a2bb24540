"""Shared pieces of the columnar-snapshot tests (test_snapshot_sim.py on the
CPU simulator, test_snapshot_gpu.py on the HIP kernels): iteration over the
shared parity runs, and the small row-count-edge tablets."""
import ybgpu as y
from parity_cases import _case

# parity_cases.build_cases(): 35 runs; exactly these 4 runs (3 cases) use
# what a snapshot does not stage — a string column or IN_TUPLE
NOT_STAGEABLE_CASES = {"string_eq_pred", "in_list_string", "in_tuple_keycols"}
N_NOT_STAGEABLE_RUNS = 4
N_STAGEABLE_RUNS = 31

# where the two-rows-per-lane tail, the wave tail (64 lanes = 128 rows) and
# the workgroup tail (256 lanes = 512 rows) can go wrong
EDGE_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025)
EDGE_READ = 1_000_000      # after every write (rows are written at 1000 + r)
EDGE_READ_BEFORE = 500     # before every write: the empty snapshot

EDGE_SCHEMA = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_DOUBLE, 1), (12, y.T_INT32, 1)])

_KEEP = []


def iter_runs(cases):
    """(case, run index, read_micros, preds, aggs, lower, upper) for every
    run of every case."""
    for case in cases:
        for ri, run in enumerate(case["runs"]):
            lower = run[3] if len(run) > 3 else None
            upper = run[4] if len(run) > 4 else None
            yield case, ri, run[0], run[1], run[2], lower, upper


def edge_tablet(n, nulls=True):
    """n rows: int64 key r, values (r * 7 - 1000, r * 0.5 + 0.25, r % 1000);
    with `nulls`, the double column is NULL on every 3rd row."""
    b = y.Builder(EDGE_SCHEMA)
    for r in range(n):
        dv = None if (nulls and r % 3 == 0) else r * 0.5 + 0.25
        b.add_packed_row(1000 + r,
                         [(y.T_INT64, r * 7 - 1000), (y.T_DOUBLE, dv),
                          (y.T_INT32, r % 1000)],
                         hash_=r // 64, key_datums=(r,))
    _KEEP.append(b)
    return _case("edge_%d_%s" % (n, "nulls" if nulls else "dense"),
                 EDGE_SCHEMA, b.finish(), [])


def edge_query():
    """Two predicates + all eight aggregate ops (touches the NULL column)."""
    preds = [y.Pred(0, 0, y.PRED_GT, (-900) & (2**64 - 1), None, 0),
             y.Pred(0, 2, y.PRED_LT, 990, None, 0)]
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_COUNT, 1),
            y.Agg(y.AGG_SUM_INT64, 0), y.Agg(y.AGG_SUM_DOUBLE, 1),
            y.Agg(y.AGG_MIN_INT64, 0), y.Agg(y.AGG_MAX_INT64, 2),
            y.Agg(y.AGG_MIN_DOUBLE, 1), y.Agg(y.AGG_MAX_DOUBLE, 1)]
    return preds, aggs


# (predicates, aggregates) counts that select each compile-time shape of the
# GT..NE query kernel: predicate cap 4 / 8 x aggregate cap 2 / 4 / 8. Every
# shape references the double column, so the dense tablet runs its no-mask
# variant and the NULL-carrying tablet its masked one.
KERNEL_SHAPES = [(np_, na) for np_ in (2, 5) for na in (2, 4, 8)]


def shape_query(n_preds, n_aggs):
    """GT..NE predicates on value and key columns + the first n_aggs of
    edge_query()'s aggregates (COUNT(*), COUNT(double col), ...)."""
    import struct
    one = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
    pool = [y.Pred(0, 0, y.PRED_GT, (-900) & (2**64 - 1), None, 0),
            y.Pred(0, 2, y.PRED_LT, 990, None, 0),
            y.Pred(0, 1, y.PRED_GT, one, None, 0),
            y.Pred(1, 0, y.PRED_GE, 1, None, 0),
            y.Pred(0, 0, y.PRED_NE, 1100, None, 0)]   # row 300
    return pool[:n_preds], edge_query()[1][:n_aggs]


def edge_query_no_null_col():
    """References only columns 0 and 2 (never the NULL-carrying double)."""
    preds = [y.Pred(0, 0, y.PRED_GE, 0, None, 0),
             y.Pred(0, 2, y.PRED_NE, 5, None, 0)]
    aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 0),
            y.Agg(y.AGG_MAX_INT64, 2)]
    return preds, aggs
