#!/usr/bin/env python3
"""ORDER BY / top-N micro-bench: the ordered snapshot select against (b)
today's route — the key-order select of every match plus
numpy.argpartition / argsort on the host — and (c) yb_gpu_snapshot_query with
COUNT(*) and the same predicate, the floor the count pass alone costs; on the
benchmark's default tablet (filtersum schema, 100M rows), predicate
col0 < t at roughly 0.01 %, 1 %, 10 % and 100 % selectivity, the key and
value column 3 projected, ordered by value column 2, limits 10, 1000 and
1M. The modes run in one process, alternated after warm-up; medians with
min / max are written as one JSON file. Two more tablets measure the
selection's corner cases at 10 % selectivity (predicate on column 1): a
16-distinct-value order column (one LDS bin per wave) and a two-valued one
with LIMIT 10 (full depth through the position digits, early-out off and
on).

  snap_order_bench.py [--rows N] [--reps R] [--out FILE] [--check]
  snap_order_bench.py --profile-run [--rows N] [--reps R]
      ordered selects only: the run to put under
      `rocprofv3 --kernel-trace --stats -- python ...`

--check compares the ordered select with the host route's rows, once per
selectivity and limit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                              "snap_order_bench.json"))
ap.add_argument("--check", action="store_true")
ap.add_argument("--profile-run", action="store_true")
args = ap.parse_args()

import ybgpu as y  # noqa: E402
from gpu_scan import GpuScan  # noqa: E402

WARMUP = 2
SELECTIVITIES = [("0.01%", int((1 << 40) * 1e-4)), ("1%", (1 << 40) // 100),
                 ("10%", (1 << 40) // 10), ("100%", 1 << 41)]
LIMITS = (10, 1000, 1_000_000)
COLS = [(1, 0), (0, 3)]
ORDER_BY = (0, 2)
READ = 1_700_000_000_000_000
schema = y.make_schema([y.KT_INT64],
                       [(10 + i, y.T_INT64, 1) for i in range(4)])


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "n": len(xs)}


def build(group_mod):
    t0 = time.time()
    data, offsets, nb, total, _ne = y.generate(
        schema, rows=args.rows, seed=42, versions=1,
        ht_base_micros=1_600_000_000_000_000, ht_step_micros=1000,
        group_mod=group_mod)
    gen_s = time.time() - t0
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(READ)
    s = GpuScan(spec)
    s.feed_blocks_host(data, offsets, nb, total)
    snap = s.snapshot()
    s.close()
    # three 100M-row tablets in one process: give the host copy back
    import ctypes as C
    lib = y.product()
    lib.ybg_free.restype = None
    lib.ybg_free.argtypes = [C.c_void_p]
    lib.ybg_free(C.cast(data, C.c_void_p))
    lib.ybg_free(C.cast(offsets, C.c_void_p))
    return snap, gen_s


def measure(snap, preds, order_by, limit, cap, host_cols, reps, modes_wanted):
    """Alternate the wanted modes; returns {mode: {wall_ms, kernel_ms}} and
    the ordered select's last result."""
    count_aggs = [y.Agg(y.AGG_COUNT_STAR, 0)]
    last = {}

    def do_ordered():
        out = snap.select_ordered_raw(preds, COLS, order_by, limit=limit,
                                      cap=cap)
        last["ordered"] = out
        return snap.kernel_ms()

    def do_host():
        # today's route: every match in key order, then the host picks and
        # sorts the first `limit` by the order column (stable, so ties keep
        # key order as the ordered select's do)
        datums, _nm, ids, res = snap.select_raw(preds, host_cols, cap=CAP_ALL)
        kms = snap.kernel_ms()
        n = res.n_rows
        oc = np.ctypeslib.as_array(datums)[(len(host_cols) - 1) * CAP_ALL:
                                           (len(host_cols) - 1) * CAP_ALL + n]
        oc = oc.view(np.int64)
        if limit < n:
            part = np.argpartition(oc, limit - 1)[:limit]
            # rows tied with the limit-th value: take them in key order
            kth = oc[part].max()
            low = np.flatnonzero(oc < kth)
            tie = np.flatnonzero(oc == kth)[:limit - len(low)]
            pick = np.concatenate([low, tie])
        else:
            pick = np.arange(n)
        pick = pick[np.argsort(oc[pick], kind="stable")]
        last["host"] = (pick, np.ctypeslib.as_array(ids)[:n])
        return kms

    def do_count():
        r = snap.query(preds, count_aggs)
        last["count"] = r.rows_matched
        return snap.kernel_ms()

    fns = {"ordered": do_ordered, "host_sort": do_host,
           "count_query": do_count}
    wall = {m: [] for m in modes_wanted}
    kern = {m: [] for m in modes_wanted}
    for rep in range(WARMUP + reps):
        for m in modes_wanted:     # alternated: drift hits every mode alike
            t0 = time.perf_counter()
            kms = fns[m]()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= WARMUP:
                wall[m].append(dt)
                kern[m].append(kms)
    return ({m: {"wall_ms": stats(wall[m]), "kernel_ms": stats(kern[m])}
             for m in modes_wanted}, last)


entries = []
snap, gen_s = build(0)
info = snap.info()
CAP_ALL = info.n_rows
HOST_COLS = COLS + [ORDER_BY]
bytes_before = info.device_bytes
for label, thr in SELECTIVITIES:
    preds = [y.Pred(0, 0, y.PRED_LT, thr, None, 0)]
    for limit in LIMITS:
        modes = ["ordered"] if args.profile_run else \
            ["ordered", "host_sort", "count_query"]
        res, last = measure(snap, preds, ORDER_BY, limit, limit, HOST_COLS,
                            args.reps, modes)
        ores = last["ordered"][5]
        entry = {"label": label, "threshold": thr, "limit": limit,
                 "rows_matched": ores.r.rows_matched,
                 "rows_delivered": ores.r.n_rows,
                 "digit_passes": ores.digit_passes, "modes": res}
        if not args.profile_run:
            assert last["count"] == ores.r.rows_matched
            o, h, c = (res[m] for m in ("ordered", "host_sort",
                                        "count_query"))
            entry["ordered_over_count_kernel"] = \
                o["kernel_ms"]["median"] / c["kernel_ms"]["median"]
            entry["host_over_ordered_wall"] = \
                h["wall_ms"]["median"] / o["wall_ms"]["median"]
            # beats the host route by more than that route's own spread
            entry["ordered_beats_host_beyond_spread"] = bool(
                h["wall_ms"]["median"] - o["wall_ms"]["median"] >
                h["wall_ms"]["max"] - h["wall_ms"]["min"])
            if args.check:
                pick, ids = last["host"]
                got = np.ctypeslib.as_array(last["ordered"][2])[
                    :ores.r.n_rows]
                assert (got == ids[pick]).all(), (label, limit)
                entry["checked_rows_against_host_sort"] = int(len(pick))
        entries.append(entry)
        print(json.dumps(entry), flush=True)
bytes_after = snap.info().device_bytes
snap.close()

corner = []
for name, mod, limits, cands in (("16_distinct", 16, (10, 1000), (None,)),
                                 ("two_valued", 2, (10,), (None, "1"))):
    snap, _g = build(mod)
    CAP_ALL = snap.info().n_rows
    preds = [y.Pred(0, 1, y.PRED_LT, (1 << 40) // 10, None, 0)]
    for limit in limits:
        for cand in cands:
            if cand is None:
                os.environ.pop("YBG_SNAP_ORDER_CAND", None)
            else:
                os.environ["YBG_SNAP_ORDER_CAND"] = cand
            modes = ["ordered"] if args.profile_run else \
                ["ordered", "count_query"]
            res, last = measure(snap, preds, (0, 0), limit, limit,
                                COLS + [(0, 0)], args.reps, modes)
            ores = last["ordered"][5]
            e = {"case": name, "order_column_values": mod, "limit": limit,
                 "YBG_SNAP_ORDER_CAND": cand,
                 "rows_matched": ores.r.rows_matched,
                 "digit_passes": ores.digit_passes, "modes": res}
            corner.append(e)
            print(json.dumps(e), flush=True)
    os.environ.pop("YBG_SNAP_ORDER_CAND", None)
    snap.close()

if not args.profile_run:
    result = {"rows": info.n_rows, "reps": args.reps, "warmup": WARMUP,
              "projected_columns": COLS, "order_by": ORDER_BY,
              "candidate_rows_default": y.snapshot_order_candidate_rows(),
              "generate_s": gen_s, "snapshot_build_ms": info.build_ms,
              "snapshot_device_bytes_before": bytes_before,
              "snapshot_device_bytes_after": bytes_after,
              "selectivities": entries, "corner_cases": corner}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
