"""Entry-header reads of the fast batch scanner at the edges of intervals,
blocks and the tablet, on the host simulator (the same scan_device.h code
the kernels compile): the fast path — planned and interpreted, both
extraction shapes — equals the general path and the CPU oracle bit for bit over the edge table of fast_header_cases.py,
under one, two and four intervals per batch. Every aggregate is an integer:
equal means equal bits."""
import pytest

import ybgpu as y
from fast_header_cases import (CASES, EPILOGUE_BATCHES, MIXED_ROWS, case, env,
                               oracle, sim_fast, sim_general, specs)


@pytest.mark.parametrize("name", CASES)
def test_fast_header_sim_equals_oracle(name):
    want = oracle(name)
    for ivb in (1, 2, 4):
        for plan in (1, 0):
            with env(YBG_IVB=ivb, YBG_PLAN=plan):
                spec, _ = specs(name)
                assert y.sim_scan_planned(spec) == bool(plan)
                got, _ = sim_fast(name)
                fused, _ = sim_fast(name, expect_versions=1)
                plain, _ = sim_fast(name, expect_versions=0)
                general = sim_general(name)
            assert general == want, (ivb, plan)
            assert got == want, (ivb, plan)
            assert fused == want, (ivb, plan)
            assert plain == want, (ivb, plan)


def test_fast_header_cases_reach_the_paths_they_name():
    """The table does what its comments say: the small tablets are all
    general-form entries, the 200 000-row one mixes them with case 2.1.1
    inside a wave, the one-column schema has the short value,
    the builder tablets abort batches and the others do not, and restart
    interval 1 gives one batch per row."""
    with env(YBG_IVB=1, YBG_PLAN=1):
        for name in ("c4_2000", "c4_6000"):
            _, built, *_ = case(name)
            c = y.sim_fast_census(specs(name)[0], built[0], built[1],
                                  built[2])
            assert c["lane_trips_general"] > 0
            assert c["ns1_hist"].get(10, 0) > 0
            assert c["wave_multi_path_trips"] > 0
            assert c["lane_trips_restart"] > 0 and c["lane_trips_switch"] > 0
        name = "c4_%d" % MIXED_ROWS
        _, built, *_ = case(name)
        c = y.sim_fast_census(specs(name)[0], built[0], built[1], built[2],
                              max_blocks=200)
        assert 4 * c["lane_trips_general"] > c["lane_delta_entries"]
        assert 4 * c["lane_trips_c211"] > c["lane_delta_entries"]
        assert 2 * c["wave_multi_path_trips"] > c["wave_delta_trips"]
        for n in EPILOGUE_BATCHES:
            _, built, *_ = case("epi_%d" % n)
            c = y.sim_fast_census(specs("epi_%d" % n)[0], built[0],
                                  built[1], built[2])
            assert c["batches"] == n and c["aborted"] == 0
            assert c["waves"] == (n + 63) // 64
        assert sim_fast("colupdate")[1] > 0
        assert sim_fast("c4_93")[1] == 0
        assert sim_fast("c1_93")[1] == 0
        assert sim_fast("epi_restart_one")[0][4] != b""
    # the one-column packed row: '|' + version + flags + 8 bytes < 16
    _, built, *_ = case("c1_1")
    assert built[3] < case("c4_1")[1][3]


def test_fast_census_counts_are_consistent():
    """Lockstep counts bound the per-lane means: a wave runs at least as
    many trips and byte-loop iterations as its longest lane."""
    name = "c4_6000"
    _, built, *_ = case(name)
    with env(YBG_IVB=2, YBG_PLAN=1):
        c = y.sim_fast_census(specs(name)[0], built[0], built[1], built[2])
        half = y.sim_fast_census(specs(name)[0], built[0], built[1],
                                 built[2], max_blocks=built[2] // 2)
    assert c["lane_trips"] == sum(c["lane_trips_" + k] for k in
                                  ("switch", "restart", "frequent", "c211",
                                   "general"))
    assert c["lane_trips"] <= 64 * c["wave_trips"]
    assert c["tail_iters_lanes"] <= 64 * c["tail_iters_lockstep"]
    assert c["lds_iters_lanes"] <= 64 * c["lds_iters_lockstep"]
    assert sum(c["sp_hist"].values()) == c["lane_delta_entries"]
    assert sum(c["ns1_hist"].values()) == c["lane_delta_entries"]
    assert 0 < half["batches"] < c["batches"]
