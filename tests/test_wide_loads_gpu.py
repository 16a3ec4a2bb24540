"""The column plan's load groups and the restart decode's 16-byte key chunks
on the GPU: the default dispatch (planned kernel), the interpreted fast
kernel (YBG_PLAN=0) and the general kernel (YBG_FAST=0) equal the CPU
oracle bit for bit over the table of wide_load_cases.py, planned() is true
where a plan exists, and retry_batches() reports the simulator's fallback
count. Each handle executes twice, so the second run takes the known-abort
path. Every aggregate is an integer: equal means equal bits."""
import pytest

from wide_load_cases import CASES, case, env, oracle, res_tuple, sim_fast, specs

pytestmark = pytest.mark.gpu

MODES = (("default", {"YBG_PLAN": None, "YBG_FAST": None}),
         ("interpreted", {"YBG_PLAN": 0, "YBG_FAST": None}),
         ("general", {"YBG_PLAN": None, "YBG_FAST": 0}))


def _run(name):
    from gpu_scan import GpuScan
    _, built, _, aggs, _ = case(name)
    spec, _ = specs(name)
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
def test_wide_loads_gpu_modes_equal_oracle(name):
    want = oracle(name)
    for mode, menv in MODES:
        with env(YBG_IVB=None, YBG_BB=None, YBG_GRID=None, **menv):
            runs = _run(name)
            nf = sim_fast(name)[1]
        for got, retries, planned in runs:
            print(name, mode, "retry", retries, "sim", nf, got)
            assert planned == (mode == "default"), mode
            assert got == want, mode
            assert retries == (0 if mode == "general" else nf), mode
    # the benchmark's batch size (two intervals per batch, fixed)
    with env(YBG_IVB=2, YBG_BB=0, YBG_GRID=None, YBG_PLAN=None,
             YBG_FAST=None):
        runs = _run(name)
        nf = sim_fast(name)[1]
    for got, retries, planned in runs:
        print(name, "ivb2", "retry", retries, "sim", nf, got)
        assert planned and got == want and retries == nf
