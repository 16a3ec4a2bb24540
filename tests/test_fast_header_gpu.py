"""Entry-header reads at the edges of intervals, blocks and the tablet, and
the shuffle epilogue of the planned fast kernel, on the GPU: the default
dispatch, the interpreted fast kernel (YBG_PLAN=0) and the general kernel
(YBG_FAST=0) equal the CPU oracle bit for bit over the edge table of
fast_header_cases.py, and retry_batches() reports the simulator's fallback
count. Every aggregate is an integer: equal means
equal bits."""
import pytest

from fast_header_cases import (CASES, case, env, oracle, res_tuple, sim_fast,
                               specs)

pytestmark = pytest.mark.gpu

MODES = (("default", {"YBG_PLAN": None, "YBG_FAST": None}),
         ("interpreted", {"YBG_PLAN": 0, "YBG_FAST": None}),
         ("general", {"YBG_PLAN": None, "YBG_FAST": 0}))


def _run(name):
    from gpu_scan import GpuScan
    _, built, _, aggs, _, _ = case(name)
    spec, _ = specs(name)
    s = GpuScan(spec)
    try:
        s.feed_blocks_host(built[0], built[1], built[2], built[3])
        s.execute()
        return (res_tuple(s.aggregates(), len(aggs)), s.retry_batches(),
                s.planned())
    finally:
        s.close()


@pytest.mark.parametrize("name", CASES)
def test_fast_header_gpu_modes_equal_oracle(name):
    want = oracle(name)
    # The dispatch's own batch size: one interval per batch on tablets this
    # small (so the epilogue cases have one batch per row), block-aligned
    # only where every block is a single interval — the decomposition the
    # simulator walks by default.
    for mode, menv in MODES:
        with env(YBG_IVB=None, YBG_BB=None, YBG_GRID=None, **menv):
            got, retries, planned = _run(name)
            nf = sim_fast(name)[1]
        print(name, mode, "retry", retries, "sim", nf, got)
        assert planned == (mode == "default"), mode
        assert got == want, mode
        assert retries == (0 if mode == "general" else nf), mode
    # the benchmark's batch size (two intervals per batch, fixed)
    with env(YBG_IVB=2, YBG_BB=0, YBG_GRID=None, YBG_PLAN=None,
             YBG_FAST=None):
        got, retries, planned = _run(name)
        nf = sim_fast(name)[1]
    print(name, "ivb2", "retry", retries, "sim", nf, got)
    assert planned and got == want and retries == nf
