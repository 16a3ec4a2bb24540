#!/usr/bin/env python3
"""SELECT micro-bench: the snapshot select (count / scan / gather + D2H)
against two references that run existing code — (a) yb_gpu_snapshot_query
with COUNT(*) and the same predicate on the same snapshot, (b) the block
path's emit_rows + yb_gpu_scan_next_batch with the same predicate — on the
benchmark's default tablet (filtersum schema, 100M rows), at predicate
thresholds of roughly 0.01 %, 1 %, 10 % and 100 % selectivity, two projected
columns (the key and value column 3). The three modes run in the same
process, alternated after warm-up; medians with min / max are written as one
JSON file.

  snap_select_bench.py [--rows N] [--reps R] [--out FILE] [--check]
  snap_select_bench.py --profile-run [--rows N] [--reps R]
      selects only, R per selectivity in order: the run to put under
      `rocprofv3 --kernel-trace --stats -- python ...`
  snap_select_bench.py --merge-trace KERNEL_TRACE.csv [--reps R] [--out FILE]
      per-kernel split of that run into FILE's "kernel_split" entries

--check compares the select's raw output with (b)'s rows ordered by
sort_key, once per selectivity (b) can hold."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                              "snap_select_bench.json"))
ap.add_argument("--check", action="store_true")
ap.add_argument("--profile-run", action="store_true")
ap.add_argument("--merge-trace", metavar="CSV")
args = ap.parse_args()

WARMUP = 2
# value column 0 is uniform in [0, 2^40): col0 < threshold
SELECTIVITIES = [("0.01%", int((1 << 40) * 1e-4)), ("1%", (1 << 40) // 100),
                 ("10%", (1 << 40) // 10), ("100%", 1 << 41)]
KERNELS = ("k_snap_select_count", "k_snap_select_scan",
           "k_snap_select_gather")


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "n": len(xs)}


def merge_trace():
    """The profile run launches, per selectivity in order, `reps` selects:
    the i-th select's kernels are the i-th occurrence of each name."""
    per = {k: [] for k in KERNELS}
    with open(args.merge_trace, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    per[k].append((int(row["Start_Timestamp"]),
                                   (int(row["End_Timestamp"]) -
                                    int(row["Start_Timestamp"])) / 1e6))
    for k in KERNELS:
        per[k] = [ms for _t, ms in sorted(per[k])]
        assert len(per[k]) == args.reps * len(SELECTIVITIES), \
            (k, len(per[k]))
    with open(args.out) as f:
        result = json.load(f)
    for i, entry in enumerate(result["selectivities"]):
        lo, hi = i * args.reps, (i + 1) * args.reps
        # the first repetition of each selectivity may regrow the output
        # buffers: medians over all, min / max shown
        entry["kernel_split_ms"] = {k: stats(per[k][lo:hi]) for k in KERNELS}
    result["kernel_split_source"] = \
        "rocprofv3 --kernel-trace --stats, separate run, %d selects per " \
        "selectivity" % args.reps
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps([e["kernel_split_ms"]
                      for e in result["selectivities"]]))


if args.merge_trace:
    merge_trace()
    sys.exit(0)

import ybgpu as y  # noqa: E402
from gpu_scan import GpuScan, GpuScanError  # noqa: E402

rows = args.rows
schema = y.make_schema([y.KT_INT64],
                       [(10 + i, y.T_INT64, 1) for i in range(4)])
COLS = [(1, 0), (0, 3)]
READ = 1_700_000_000_000_000

t0 = time.time()
data, offsets, nb, total, _ne = y.generate(
    schema, rows=rows, seed=42, versions=1,
    ht_base_micros=1_600_000_000_000_000, ht_step_micros=1000)
gen_s = time.time() - t0


def make_spec(preds, emit):
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(READ)
    spec.num_preds = len(preds)
    for i, p in enumerate(preds):
        spec.preds[i] = p
    spec.emit_rows = 1 if emit else 0
    return spec


s = GpuScan(make_spec([], False))
s.feed_blocks_host(data, offsets, nb, total)
t0 = time.time()
snap = s.snapshot()
build_wall_ms = (time.time() - t0) * 1e3
s.close()
info = snap.info()
bytes_before = info.device_bytes
CAP = info.n_rows


def check_against_block(blk, raw, res):
    """select's raw output == the block path's rows ordered by sort_key."""
    import ctypes as C
    import numpy as np
    b = y.RowBatch()
    rc = blk._lib.yb_gpu_scan_next_batch(blk._h, C.byref(b))
    assert rc == 0, rc
    n = b.n_rows
    assert n == res.n_rows, (n, res.n_rows)
    sort_key = np.ctypeslib.as_array(b.sort_key, (n,))
    keys = np.ctypeslib.as_array(b.key_datums, (n,))
    dat = np.ctypeslib.as_array(b.datums, (n, 4))
    nulls = np.ctypeslib.as_array(b.null_masks, (n,))
    perm = np.argsort(sort_key, kind="stable")
    datums, null_masks, row_ids = raw
    got = np.ctypeslib.as_array(datums)
    assert (got[:n] == keys[perm]).all()
    want3 = np.where((nulls[perm] >> 3) & 1, 0, dat[perm, 3])
    assert (got[CAP:CAP + n] == want3).all()
    assert (np.ctypeslib.as_array(null_masks)[:n] ==
            (nulls[perm] & 0b1000)).all()
    ids = np.ctypeslib.as_array(row_ids)[:n]
    assert (ids[1:] > ids[:-1]).all()
    return int(n)


entries = []
for label, thr in SELECTIVITIES:
    preds = [y.Pred(0, 0, y.PRED_LT, thr, None, 0)]
    count_aggs = [y.Agg(y.AGG_COUNT_STAR, 0)]

    def do_select():
        raw = snap.select_raw(preds, COLS, cap=CAP)
        return snap.kernel_ms(), raw

    if args.profile_run:
        for _ in range(args.reps):
            do_select()
        continue

    def do_count():
        r = snap.query(preds, count_aggs)
        return snap.kernel_ms(), r

    blk = GpuScan(make_spec(preds, True))
    blk.feed_blocks_host(data, offsets, nb, total)

    def do_block():
        import ctypes as C
        b = y.RowBatch()
        rc = blk._lib.yb_gpu_scan_next_batch(blk._h, C.byref(b))
        if rc:
            raise GpuScanError(blk._lib.yb_gpu_last_error().decode())
        return blk.kernel_ms()[0], b

    modes = [("select", do_select), ("count_query", do_count),
             ("block_emit", do_block)]
    skipped = {}
    wall = {m: [] for m, _ in modes}
    kern = {m: [] for m, _ in modes}
    matched = None
    checked = None
    for rep in range(WARMUP + args.reps):
        for name, fn in modes:     # alternated: drift hits every mode alike
            if name in skipped:
                continue
            t0 = time.perf_counter()
            try:
                kms, out = fn()
            except GpuScanError as e:
                # the block path's emit buffers hold at most 32Mi rows
                skipped[name] = str(e)
                continue
            dt = (time.perf_counter() - t0) * 1e3
            if name == "select":
                assert matched in (None, out[3].rows_matched)
                matched = out[3].rows_matched
                assert out[3].n_rows == matched and out[3].done == 1
            elif name == "count_query":
                assert out.rows_matched == matched
            else:
                assert out.n_rows == matched
            if rep >= WARMUP:
                wall[name].append(dt)
                kern[name].append(kms)
    if args.check and "block_emit" not in skipped:
        _kms, raw = do_select()
        checked = check_against_block(blk, raw[:3], raw[3])
    blk.close()
    entry = {"label": label, "threshold": thr, "rows_matched": matched,
             "selectivity": matched / info.n_rows,
             "checked_rows_against_block_path": checked,
             "skipped": skipped,
             "modes": {m: ({"wall_ms": stats(wall[m]),
                            "kernel_ms": stats(kern[m])} if wall[m] else None)
                       for m, _ in modes}}
    sel = entry["modes"]["select"]
    cnt = entry["modes"]["count_query"]
    entry["select_over_count_kernel"] = \
        sel["kernel_ms"]["median"] / cnt["kernel_ms"]["median"]
    if entry["modes"]["block_emit"]:
        entry["block_over_select_wall"] = \
            entry["modes"]["block_emit"]["wall_ms"]["median"] / \
            sel["wall_ms"]["median"]
    entries.append(entry)
    print(json.dumps(entry), flush=True)

if not args.profile_run:
    result = {"rows": info.n_rows, "reps": args.reps, "warmup": WARMUP,
              "projected_columns": COLS, "tile_rows":
                  y.snapshot_select_tile_rows(),
              "generate_s": gen_s, "snapshot_build_ms": info.build_ms,
              "snapshot_build_wall_ms": build_wall_ms,
              "snapshot_device_bytes_before_select": bytes_before,
              "snapshot_device_bytes_after_select": snap.info().device_bytes,
              "selectivities": entries}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
snap.close()
