"""Scan tail on the GPU: per-batch state bytes, in-wave head resolution in
the planned fast kernel and the single fold launch (k_fold). The planned
kernel, the interpreted fast kernel (YBG_PLAN=0) and the general kernel
(YBG_FAST=0) must equal the CPU oracle bit for bit on every execute of a
handle, over batch decompositions that put lane, wave, workgroup and
grid-stride pass boundaries and an incomplete wave into play, and
retry_batches() must report the simulator's fallback count. The first
execute of a handle has no known abort set; the later ones start the general
kernel from the remembered set next to the fast kernel."""
import pytest

from scan_tail_cases import (TABLETS, env, oracle, res_tuple, sim_fast,
                             specs, tablet)

pytestmark = pytest.mark.gpu

MODES = (("plan", {"YBG_PLAN": 1, "YBG_FAST": None}),
         ("interpreted", {"YBG_PLAN": 0, "YBG_FAST": None}),
         ("general", {"YBG_PLAN": None, "YBG_FAST": 0}))


def _run(name, executes=3, bb_per_execute=None):
    """One handle under the current environment: ([result tuple per
    execute], [retry_batches() per execute], planned flag)."""
    from gpu_scan import GpuScan
    _, built, _, aggs, _ = tablet(name)
    spec, _ = specs(name, 1 if name != "single" else 0)
    s = GpuScan(spec)
    try:
        s.feed_blocks_host(built[0], built[1], built[2], built[3])
        outs, retries = [], []
        for i in range(executes):
            bb = ({} if bb_per_execute is None
                  else {"YBG_BB": bb_per_execute[i]})
            with env(**bb):
                s.execute()
                outs.append(res_tuple(s.aggregates(), len(aggs)))
                retries.append(s.retry_batches())
        return outs, retries, s.planned()
    finally:
        s.close()


# YBG_IVB=1 with YBG_GRID=2 on the 20 000-row tablet: 1 250 batches over a
# 512-thread span, three grid-stride passes, the last with three full waves
# and one of 34 lanes
@pytest.mark.parametrize("bb", [0, 1])
@pytest.mark.parametrize("grid", [1, 2, None])
@pytest.mark.parametrize("ivb", [1, 2])
@pytest.mark.parametrize("name", TABLETS)
def test_tail_gpu_modes_equal_oracle(name, ivb, grid, bb):
    want = oracle(name)
    for mode, menv in MODES:
        with env(YBG_IVB=ivb, YBG_GRID=grid, YBG_BB=bb, **menv):
            outs, retries, planned = _run(name)
            nf = sim_fast(name, 1 if name != "single" else 0)[1]
        print(name, mode, "ivb", ivb, "grid", grid, "bb", bb, "retry",
              retries, "sim", nf)
        assert planned == (mode == "plan"), mode
        assert outs == [want] * 3, mode
        assert retries[0] == retries[1] == retries[2], mode
        if mode == "general":
            assert retries[0] == 0
        elif bb == 0:
            # the simulator walks the fixed-ivb decomposition
            assert retries[0] == nf, mode


@pytest.mark.parametrize("name", ["single", "chains_few"])
def test_tail_gpu_batch_decomposition_toggled_between_executes(name):
    """Fixed-ivb and block-aligned batches alternate on one handle: the
    state bytes and head records of one decomposition must not leak into
    the next."""
    want = oracle(name)
    with env(YBG_IVB=1, YBG_GRID=2, YBG_PLAN=1, YBG_FAST=None):
        outs, _, planned = _run(name, executes=5,
                                bb_per_execute=(0, 0, 1, 1, 0))
    assert planned
    assert outs == [want] * 5


@pytest.mark.parametrize("name", TABLETS)
def test_tail_gpu_known_set_off(name):
    """YBG_KNOWN=0 keeps every execute on the serial order."""
    want = oracle(name)
    with env(YBG_IVB=1, YBG_GRID=2, YBG_BB=0, YBG_KNOWN=0, YBG_PLAN=1,
             YBG_FAST=None):
        outs, retries, planned = _run(name)
        nf = sim_fast(name, 1 if name != "single" else 0)[1]
    assert planned
    assert outs == [want] * 3
    assert retries == [nf] * 3
