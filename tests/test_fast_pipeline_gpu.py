"""The fast scanner's trip order on the GPU: the default dispatch (planned
kernel), the interpreted fast kernel (YBG_PLAN=0), the general kernel
(YBG_FAST=0) and the benchmark's batch size (YBG_IVB=2 YBG_BB=0) equal the
CPU oracle bit for bit over the table of fast_pipeline_cases.py, in both
extraction shapes (expect_versions), and retry_batches() reports the
simulator's fallback count. Each handle executes twice, so the second run
takes the known-abort path. Every aggregate is an integer: equal means
equal bits."""
import pytest

from fast_pipeline_cases import (CASES, case, env, oracle, res_tuple,
                                 sim_fast, specs)

pytestmark = pytest.mark.gpu

MODES = (("default", {"YBG_PLAN": None, "YBG_FAST": None, "YBG_IVB": None,
                      "YBG_BB": None}),
         ("interpreted", {"YBG_PLAN": 0, "YBG_FAST": None, "YBG_IVB": None,
                          "YBG_BB": None}),
         ("general", {"YBG_PLAN": None, "YBG_FAST": 0, "YBG_IVB": None,
                      "YBG_BB": None}),
         ("ivb2", {"YBG_PLAN": None, "YBG_FAST": None, "YBG_IVB": 2,
                   "YBG_BB": 0}))


def _run(name, expect_versions):
    from gpu_scan import GpuScan
    _, built, _, aggs, _ = case(name)
    spec, _ = specs(name, expect_versions)
    s = GpuScan(spec)
    try:
        s.feed_blocks_host(built[0], built[1], built[2], built[3])
        out = []
        for _ in range(2):
            s.execute()
            out.append((res_tuple(s.aggregates(), len(aggs)),
                        s.retry_batches(), s.planned()))
        return out
    finally:
        s.close()


@pytest.mark.parametrize("name", CASES)
def test_pipeline_gpu_modes_equal_oracle(name):
    want = oracle(name)
    for mode, menv in MODES:
        for ev in (0, 1):
            with env(YBG_GRID=None, **menv):
                runs = _run(name, ev)
                nf = sim_fast(name, ev)[1]
            for got, retries, planned in runs:
                print(name, mode, "versions", ev, "retry", retries, "sim", nf,
                      got)
                assert planned == (mode in ("default", "ivb2")), mode
                assert got == want, (mode, ev)
                assert retries == (0 if mode == "general" else nf), (mode, ev)
