#!/usr/bin/env python3
"""String-predicate micro-bench: does the staged 8-byte prefix column pay?

On the benchmark's groupby tablet (32-byte string column) one EQ and one LT
string predicate with COUNT(*) run three ways, alternated in one process:
  prefix     the library as built: the predicate streams the prefix column
             and only a tie on all 8 bytes reads the string heap
  heap_only  a library built with -DYBG_SNAP_STR_HEAP_ONLY (every compare
             reads off[] and the heap), given in YBG_SO_HEAP; skipped when
             unset
  block      the block path (yb_gpu_scan_execute) with the same predicate
Medians with min / max of the kernel times go to one JSON file, with the
string build's build_ms and device_bytes.

usage: YBG_SO_HEAP=/path/libybgpu.so snap_string_bench.py [rows [reps [out]]]
"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ybgpu as y  # noqa: E402
import gpu_scan  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(
    ROOT, "profiles", "snap_string_bench.json")
WARMUP = 3
STR_COL = 3

schema = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_INT64, 1), (12, y.T_DOUBLE, 1),
     (13, y.T_STRING, 1)])
star = [y.Agg(y.AGG_COUNT_STAR, 0)]
_keep = []


def str_pred(op, rhs):
    buf = (C.c_uint8 * len(rhs)).from_buffer_copy(rhs)
    _keep.append(buf)
    return y.Pred(0, STR_COL, op, 0, buf, len(rhs))


def make_spec(preds):
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(1_700_000_000_000_000)
    spec.num_preds = len(preds)
    for i, p in enumerate(preds):
        spec.preds[i] = p
    spec.num_aggs = 1
    spec.aggs[0] = star[0]
    return spec


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "n": len(xs)}


def string_snapshot(data, offsets, nb, total):
    s = gpu_scan.GpuScan(make_spec([]))
    s.feed_blocks_host(data, offsets, nb, total)
    snap = s.snapshot(strings=True)
    s.close()
    return snap


data, offsets, nb, total, _ne = y.generate(
    schema, rows=rows, seed=42, versions=1,
    ht_base_micros=1_600_000_000_000_000, ht_step_micros=1000, group_mod=16)

snaps = {"prefix": string_snapshot(data, offsets, nb, total)}
info = snaps["prefix"].info()
sinfo = snaps["prefix"].string_info()
heap_so = os.environ.get("YBG_SO_HEAP")
if heap_so:
    # a second library in the same process: handles made while it is the
    # product library keep calling it
    main_lib = y._product
    y._product = C.CDLL(heap_so)
    snaps["heap_only"] = string_snapshot(data, offsets, nb, total)
    y._product = main_lib

# EQ: the string of the first row (one 32-byte random string: nearly every
# row differs inside the prefix). LT: a one-byte rhs in the middle of the
# alphabet (about half the rows pass, none ties).
rows0, _res = snaps["prefix"].select([], [(0, STR_COL)], limit=1)
queries = {"EQ": str_pred(y.PRED_EQ, rows0[0][0]),
           "LT": str_pred(y.PRED_LT, b"h")}

result = {"rows": rows, "reps": reps, "warmup": WARMUP,
          "string_build_ms": info.build_ms,
          "string_device_bytes": info.device_bytes,
          "string_bytes": sinfo.string_bytes[STR_COL], "queries": {}}
for qname, pred in queries.items():
    block = gpu_scan.GpuScan(make_spec([pred]))
    block.feed_blocks_host(data, offsets, nb, total)

    def run_block():
        block.execute()
        return block.aggregates().rows_matched, block.kernel_ms()[0]

    def run_snap(snap):
        def run():
            res = snap.query([pred], star)
            return res.rows_matched, snap.kernel_ms()
        return run

    modes = [(name, run_snap(snap)) for name, snap in snaps.items()]
    modes.append(("block", run_block))
    kern = {m: [] for m, _ in modes}
    matched = {}
    for rep in range(WARMUP + reps):
        for name, fn in modes:     # alternated: drift hits every mode alike
            m, ms = fn()
            matched[name] = m
            if rep >= WARMUP:
                kern[name].append(ms)
    assert len(set(matched.values())) == 1, matched
    result["queries"][qname] = {
        "rows_matched": matched["prefix"],
        "kernel_ms": {m: stats(kern[m]) for m, _ in modes}}
    block.close()

for snap in snaps.values():
    snap.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
