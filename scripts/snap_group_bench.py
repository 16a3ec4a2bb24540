#!/usr/bin/env python3
"""GROUP BY micro-bench: the block path (k_group over the SST blocks) against
the grouped snapshot query at both levels (workgroup-local LDS table + flush,
global table only), on the benchmark's groupby tablet at 16 and 65,536
groups. The three modes run on the same tablet in the same process,
alternated; medians with min / max are written as one JSON file.

usage: snap_group_bench.py [rows [reps [out.json]]]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ybgpu as y  # noqa: E402
from gpu_scan import GpuScan  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(
    ROOT, "profiles", "snap_group_bench.json")
CAP = 1 << 17
WARMUP = 3

# bench.py --workload groupby: schema, generator call and the two int64
# range predicates (the string predicate dropped: a snapshot stages no
# strings), COUNT(*) + SUM(col 1) grouped on value column 0
schema = y.make_schema(
    [y.KT_INT64],
    [(10, y.T_INT64, 1), (11, y.T_INT64, 1), (12, y.T_DOUBLE, 1),
     (13, y.T_STRING, 1)])
preds = [y.Pred(0, 1, y.PRED_GT, 1 << 38, None, 0),
         y.Pred(0, 1, y.PRED_LT, 3 << 38, None, 0)]
aggs = [y.Agg(y.AGG_COUNT_STAR, 0), y.Agg(y.AGG_SUM_INT64, 1)]
L = y.snapshot_group_local_slots(len(aggs))


def stats(xs):
    if not any(xs):
        return None   # this mode reports no kernel time
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "n": len(xs)}


def checksum(n, vals):
    cnt = sm = 0
    for g in range(n):
        cnt += vals[g * y.MAX_AGGS]
        sm += vals[g * y.MAX_AGGS + 1]
    return n, cnt, sm & ((1 << 64) - 1)


def one_cardinality(group_mod):
    t0 = time.time()
    data, offsets, nb, total, _ne = y.generate(
        schema, rows=rows, seed=42, versions=1,
        ht_base_micros=1_600_000_000_000_000, ht_step_micros=1000,
        group_mod=group_mod)
    gen_s = time.time() - t0
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.group_col = 1
    spec.read_time = y.read_time(1_700_000_000_000_000)
    spec.num_preds = len(preds)
    for i, p in enumerate(preds):
        spec.preds[i] = p
    spec.num_aggs = len(aggs)
    for i, a in enumerate(aggs):
        spec.aggs[i] = a
    s = GpuScan(spec)
    s.feed_blocks_host(data, offsets, nb, total)
    t0 = time.time()
    snap = s.snapshot()
    build_wall_ms = (time.time() - t0) * 1e3
    info = snap.info()

    sums = {}

    # check: fold the output into a checksum (warm-up repetitions only,
    # so the Python fold stays out of the timed ones)
    def block(check):
        _k, vals, _c, _kb, n = s.group_aggregate_raw(cap=CAP,
                                                     key_bytes_cap=1 << 12)
        if check:
            sums["block"] = checksum(n, vals)
        return s.kernel_ms()[0]

    def snap_mode(name, hint):
        def run(check):
            _k, vals, _c, res = snap.group_query_raw(
                preds, aggs, 0, expect_groups=hint, cap=CAP)
            if check:
                assert res.local_level == (1 if hint <= L else 0)
                sums[name] = checksum(res.n_groups, vals)
            return snap.kernel_ms()
        return run

    modes = [("block", block), ("snap_two_level", snap_mode("snap_two_level", 1)),
             ("snap_global_only", snap_mode("snap_global_only", L + 1))]
    wall = {m: [] for m, _ in modes}
    kern = {m: [] for m, _ in modes}
    for rep in range(WARMUP + reps):
        for name, fn in modes:     # alternated: drift hits every mode alike
            t0 = time.perf_counter()
            kms = fn(rep < WARMUP)
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= WARMUP:
                wall[name].append(dt)
                kern[name].append(kms)
    # the three modes answer the same question
    assert sums["block"] == sums["snap_two_level"] == \
        sums["snap_global_only"], sums
    tl = wall["snap_two_level"]
    go = wall["snap_global_only"]
    out = {"group_mod": group_mod,
           "global_only_over_two_level_wall":
               statistics.median(go) / statistics.median(tl), "groups": sums["block"][0],
           "rows_matched": sums["block"][1], "generate_s": gen_s,
           "snapshot_build_ms": info.build_ms,
           "snapshot_build_wall_ms": build_wall_ms,
           "snapshot_device_bytes": snap.info().device_bytes,
           "modes": {m: {"wall_ms": stats(wall[m]),
                         "kernel_ms": stats(kern[m])} for m, _ in modes}}
    # yb_gpu_scan_kernel_ms reports nothing for the block path's grouped
    # scan (kernel_ms null): the ratios are taken on wall time
    for m in ("snap_two_level", "snap_global_only"):
        out["modes"][m]["block_over_this_wall"] = \
            out["modes"]["block"]["wall_ms"]["median"] / \
            out["modes"][m]["wall_ms"]["median"]
    snap.close()
    s.close()
    y.product().ybg_free(data)
    y.product().ybg_free(offsets)
    return out


result = {"rows": rows, "reps": reps, "warmup": WARMUP, "local_slots": L,
          "cardinalities": [one_cardinality(16), one_cardinality(65536)]}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
