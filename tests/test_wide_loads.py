"""The column plan's load groups and the restart decode's 16-byte key chunks
on the host simulator (the same scan_device.h code the kernels compile):
the fast path — planned and interpreted, both extraction shapes — equals
the general path and the CPU oracle bit for bit over the table of
wide_load_cases.py, under one, two and four intervals per batch. Every
aggregate is an integer: equal means equal bits."""
import pytest

import ybgpu as y
from wide_load_cases import (CASES, CHAIN_CASES, KEY_CASES, KEY_ROWS,
                             PLAN_CASES, case, census, env, oracle, sim_fast,
                             sim_general, specs)


@pytest.mark.parametrize("name", CASES)
def test_wide_loads_sim_equals_oracle(name):
    want = oracle(name)
    for ivb in (1, 2, 4):
        for plan in (1, 0):
            with env(YBG_IVB=ivb, YBG_PLAN=plan):
                assert y.sim_scan_planned(specs(name)[0]) == bool(plan)
                plain, nf = sim_fast(name, expect_versions=0)
                fused, nf2 = sim_fast(name, expect_versions=1)
                general = sim_general(name)
            assert general == want, (ivb, plan)
            assert plain == want, (ivb, plan)
            assert fused == want, (ivb, plan)
            assert nf == nf2


@pytest.mark.parametrize("name", tuple(PLAN_CASES))
def test_plan_compiles_to_the_named_shape(name):
    assert y.sim_plan_shape(specs(name)[0]) == PLAN_CASES[name][3]
    # a result no row satisfies would hide a swapped half
    want = oracle(name)
    if name != "unsatisfiable":
        assert 0 < want[2] < want[1] or not PLAN_CASES[name][1]
    else:
        assert want[2] == 0 and want[1] > 0


@pytest.mark.parametrize("key", tuple(KEY_CASES))
def test_restart_keys_have_the_named_length(key):
    ns1 = KEY_CASES[key][4]
    with env(YBG_IVB=1, YBG_PLAN=1):
        c = census(key + "_ri1")
        nf = sim_fast(key + "_ri1")[1]
        nf16 = sim_fast(key + "_ri16")[1]
    if ns1 == 0:  # above kFastKeyCap - 8: every batch goes to the general path
        assert c["aborted"] == c["batches"] == KEY_ROWS == nf
        assert nf16 > 0
        return
    assert (c["restart_ns1_min"], c["restart_ns1_max"]) == (ns1, ns1)
    # (with interval 16 a few batches abort in the delta decode, where the
    # hash changes: not this test's subject)
    assert c["aborted"] == 0 and nf == 0 and nf16 < KEY_ROWS // 8
    # one batch per row; a batch also walks into the next batch's restart
    assert c["lane_trips_restart"] == 2 * KEY_ROWS - 1


def test_chain_cases_reach_the_paths_they_name():
    with env(YBG_IVB=1, YBG_PLAN=1):
        for name in CHAIN_CASES:
            c = census(name)
            assert c["lane_trips_restart"] > 0, name
            assert c["aborted"] == 0 or not name.endswith("ri1"), name
        # every entry a restart entry; with interval 2 every other one, so
        # chains of three both continue across a restart and change at one
        assert census("chains_ri1")["lane_delta_entries"] == 0
        assert census("chains_ri2")["lane_delta_entries"] > 0
        assert census("tomb_ri1")["lane_delta_entries"] == 0
    # 16 k + 1 rows: the tablet's last entry is a restart entry
    assert case("last_restart_ri16")[1][4] % 16 == 1
