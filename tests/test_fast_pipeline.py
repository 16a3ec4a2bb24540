"""The fast scanner's trip order on the host simulator (the same
scan_device.h code the kernels compile): the fast path, planned and
interpreted, both extraction shapes, equals the general path and the CPU
oracle bit for bit over the table of fast_pipeline_cases.py under one, two
and four intervals per batch, and the tablets hold the shapes they name.
Every aggregate is an integer: equal means equal bits."""
import pytest

import ybgpu as y
from fast_pipeline_cases import (ABORT_CASES, CASES, CHAIN_CASES,
                                 HEADER_CASES, TOMB_CASES, case, env, oracle,
                                 sim_fast, sim_general, specs, walk)


@pytest.mark.parametrize("name", CASES)
def test_pipeline_sim_equals_oracle(name):
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


def _v2len(name):
    # the full packed row: the longest value of the tablet
    return max(e[3] for e in walk(name))


@pytest.mark.parametrize("name", tuple(TOMB_CASES))
def test_short_values_sit_where_the_case_says(name):
    ents = walk(name)
    full = _v2len(name)
    last = ents[-1]
    assert last[4], "the walk reached the tablet's end"
    if "last_tomb" in name:
        assert last[3] == 1
    else:
        assert last[3] == full
    if name.endswith("ri16"):
        assert last[1] == "delta"
    # a tombstone directly in front of a full row, and a block ending on one
    pairs = {(a[3], b[3]) for a, b in zip(ents, ents[1:])}
    assert (1, full) in pairs and (full, 1) in pairs
    if name == "tomb_last_tomb_ri16":
        assert any(e[4] and e[3] == 1 for e in ents[:-1]), \
            "no inner block ends on a tombstone"
    # some rows are deleted, some survive
    want = oracle(name)
    assert 0 < want[2] < want[1]


def test_chains_cover_every_first_visible_position():
    for nver in (3, 5):
        rows = set()
        for name, (n, ri, v) in CHAIN_CASES.items():
            if n != nver:
                continue
            want = oracle(name)
            rows.add((v, want[1] > 0))
            assert (want[1] > 0) == (v < nver), name
            # interval shorter than a chain: chains cross restart points
            if ri < nver:
                kinds = [e[1] for e in walk(name)]
                assert kinds.count("restart") * ri >= len(kinds) - ri
        assert rows == {(v, v < nver) for v in range(nver + 1)}
    # different first-visible versions give different sums
    sums = {oracle("chain3_v%d_ri16" % v)[3] for v in range(3)}
    assert len(sums) == 3


@pytest.mark.parametrize("kind", ABORT_CASES)
def test_late_aborts_fall_back(kind):
    name = "abort_" + kind
    with env(YBG_IVB=1, YBG_PLAN=1):
        got, nf = sim_fast(name)
    n_odd = len([r for r in range(600) if r % 37 == 20])
    # a batch is one interval here; an odd entry aborts its own batch and
    # the batch that walks into it
    assert n_odd <= nf <= 2 * n_odd + 2, nf
    assert got == oracle(name)


def test_header_lengths_and_entry_phases():
    nbs, mod16, mod128 = set(), set(), set()
    for name in CASES:
        for p, kind, nb, _, _ in walk(name):
            if kind == "delta":
                nbs.add(nb)
                mod16.add(p % 16)
                mod128.add(p % 128)
    print("delta nb:", sorted(nbs))
    print("p mod 16:", sorted(mod16))
    print("p mod 128:", sorted(mod128))
    # both sides of the window's second half (nb > 13), of the key carry
    # (7 / 8) and of check 16 (24 passes, 25 aborts)
    assert {7, 8, 12, 13, 14, 16, 17, 24, 25} <= nbs, sorted(nbs)
    assert any(m % 2 for m in mod16) and len(mod16) == 16
    assert any(m > 96 for m in mod128), "no window straddles a cache line"
    # nb = 25 aborts, nb = 24 does not
    with env(YBG_IVB=1, YBG_PLAN=1):
        for kind in HEADER_CASES:
            name = "hdr_" + kind
            worst = max(e[2] for e in walk(name) if e[1] == "delta")
            nf = sim_fast(name)[1]
            print(name, "max nb", worst, "fallbacks", nf)
            if worst > 24:
                assert nf > 0, name
            else:
                # only the entries at the tablet's two hash changes
                assert nf <= 2, name


def test_interval_switches_contiguous_and_not():
    # inside a block the next interval starts where the last one ended; at a
    # block's end the restart array and the trailer lie in between
    _, built, *_ = case("chain3_v1_ri2")
    assert built[2] > 1  # more than one block
    ents = walk("chain3_v1_ri2")
    nxt = {a[0] + a[2] + a[3] == b[0] for a, b in zip(ents, ents[1:])
           if b[1] == "restart"}
    assert nxt == {True, False}
