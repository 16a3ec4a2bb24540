#!/usr/bin/env python3
"""Census of the fast kernel's entry loop, on the CPU (host simulator).

Replays the head of a generated tablet through scan_batch_fast with the
per-trip hook on, 64 consecutive batches in lockstep the way a wave runs
them, and prints where the trips go: trips per wave-batch, lane utilisation,
trips per path (interval switch, restart, frequent, case 2.1.1, general
form), the sp / ns1 / ns2 histograms of the delta entries, and the byte-loop
iterations a wave runs (the longest lane's count) against the per-lane mean.

  scripts/fast_census.py --workload filtersum --rows 100000000 \\
      --blocks 40000 --ivb 2

--workload picks the benchmark's generator call and query (filtersum, mvcc);
groupby runs k_group, not the fast kernel, and is reported as such.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ybgpu as y  # noqa: E402


def bench_case(workload):
    """(schema, preds, aggs, versions, read_micros, expect_versions) of
    bench.py's workload."""
    schema = y.make_schema([y.KT_INT64],
                           [(10 + i, y.T_INT64, 1) for i in range(4)])
    if workload == "filtersum":
        return (schema,
                [(0, y.PRED_GT, 1 << 39), (1, y.PRED_LT, 3 << 38),
                 (2, y.PRED_GE, 1 << 36)],
                [(y.AGG_SUM_INT64, 3), (y.AGG_COUNT_STAR, 0)], 1,
                1_700_000_000_000_000, 0)
    return (schema, [], [(y.AGG_COUNT_STAR, 0), (y.AGG_SUM_INT64, 0)], 5,
            1_600_000_002_500_000, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", default="filtersum",
                    choices=["filtersum", "mvcc", "groupby"])
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--blocks", type=int, default=40000,
                    help="blocks to replay from the tablet's head (0 = all)")
    ap.add_argument("--ivb", type=int, default=2,
                    help="intervals per batch (YBG_IVB)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.workload == "groupby":
        print("groupby: the grouped scan runs k_group (scan_one_interval), "
              "not scan_batch_fast; nothing to count")
        return
    schema, preds, aggs, versions, read, ev = bench_case(args.workload)
    data, offsets, nb, total, ne = y.generate(
        schema, rows=args.rows, seed=args.seed, versions=versions,
        ht_base_micros=1_600_000_000_000_000,
        ht_step_micros=1_000_000 if versions > 1 else 1000)
    spec = y.ScanSpec()
    spec.schema = schema
    spec.kv_format = y.ENC_THREE_SHARED_PARTS
    spec.read_time = y.read_time(read)
    spec.expect_versions = ev
    spec.num_preds = len(preds)
    for i, (col, op, c) in enumerate(preds):
        spec.preds[i] = y.Pred(0, col, op, c, None, 0)
    spec.num_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        spec.aggs[i] = y.Agg(op, col)
    os.environ["YBG_IVB"] = str(args.ivb)
    c = y.sim_fast_census(spec, data, offsets, nb, args.blocks)
    if args.json:
        print(json.dumps(c))
        return
    w = max(c["waves"], 1)
    wt = max(c["wave_trips"], 1)
    dt = max(c["wave_delta_trips"], 1)
    de = max(c["lane_delta_entries"], 1)
    print(f"{args.workload}: rows={args.rows} blocks={nb} "
          f"replayed={min(args.blocks, nb) if args.blocks else nb} "
          f"ivb={args.ivb} waves={c['waves']} batches={c['batches']} "
          f"aborted={c['aborted']}")
    print(f"  trips per wave-batch      {c['wave_trips'] / w:8.2f}")
    print(f"  lane utilisation          {c['lane_trips'] / (64.0 * wt):8.3f}")
    for k in ("switch", "restart", "frequent", "c211", "general"):
        print(f"  wave trips with {k:9s} {c['wave_trips_' + k] / w:8.2f}"
              f"   (lane entries {c['lane_trips_' + k]})")
    print(f"  wave trips with a delta   {c['wave_delta_trips'] / w:8.2f}")
    print(f"  wave trips, two paths     "
          f"{c['wave_multi_path_trips'] / w:8.2f}")
    print(f"  tail-patch iterations per delta trip: lockstep "
          f"{c['tail_iters_lockstep'] / dt:.2f}, lane mean "
          f"{c['tail_iters_lanes'] / de:.2f}")
    print(f"  LDS byte-loop iterations per delta trip: lockstep "
          f"{c['lds_iters_lockstep'] / dt:.2f}, lane mean "
          f"{c['lds_iters_lanes'] / de:.2f}")
    for h in ("sp", "ns1", "ns2"):
        hist = c[h + "_hist"]
        tot = max(sum(hist.values()), 1)
        top = sorted(hist.items(), key=lambda kv: -kv[1])[:6]
        print(f"  {h:3s} " + "  ".join(f"{k}: {100.0 * v / tot:.2f}%"
                                       for k, v in top))


if __name__ == "__main__":
    main()
