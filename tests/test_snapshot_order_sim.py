"""CPU parity of ORDER BY / top-N on a columnar snapshot: the host simulator
(ybg_sim_snapshot_select_ordered — the snapshot layout, then the
snap_device.h key image, digit, selection state, gather and emit code the
gfx950 kernels run, one simulated tile at a time, std::stable_sort standing
in for the device sort) against the CPU oracle's matching rows sorted in
Python. The scenarios live in snapshot_order_cases.py and run again on the
kernels in test_snapshot_order_gpu.py."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec
import snapshot_order_cases as so
import snapshot_select_cases as ss


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def run(case, read_micros, preds, cols, order_by, descending=False,
        nulls_first=False, limit=0, after=None, row_lo=0, row_hi=None,
        cap=so.CAP, lower=None, upper=None, strings=False,
        varlen_cap=so.VCAP, backward=False):
    # the spec carries read time and bounds only: the build ignores the rest
    spec = make_spec(case, read_micros, (), (), lower, upper)
    raw, res = y.sim_snapshot_select_ordered(
        spec, case["data"], case["offsets"], case["n_blocks"], list(preds),
        list(cols), order_by, descending, nulls_first, limit, after, row_lo,
        row_hi, cap, varlen_cap, strings, backward)
    strs = y.select_string_cols(case["schema"], cols) if strings else None
    rows = y.decode_snapshot_rows(res.r, raw[0], raw[1], len(cols), cols,
                                  cap, raw[3], strs)
    return rows, raw, res


def test_candidate_rows_default():
    assert y.snapshot_order_candidate_rows() >= 2


def test_sim_order_vs_oracle_all_stageable_cases(cases):
    so.scenario_parity(run, cases)


@pytest.mark.parametrize("n", ss.edge_sizes())
def test_sim_order_tablet(n, monkeypatch):
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    so.scenario_order_tablet(run, n)


def test_sim_order_keeps_bit_patterns():
    so.scenario_bits_kept(run)


def test_sim_order_empty():
    so.scenario_empty(run)


@pytest.mark.parametrize("n", sorted({1025, 2 * ss.tile_rows() + 1}))
def test_sim_order_both_selection_paths(n, monkeypatch):
    """Full depth (YBG_SNAP_ORDER_CAND=1) and the default early-out deliver
    byte-identical output; scenario_order_tablet pins digit_passes."""
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    early = so.scenario_order_tablet(run, n)
    monkeypatch.setenv("YBG_SNAP_ORDER_CAND", "1")
    deep = so.scenario_order_tablet(run, n, cand_one=True)
    assert early == deep


def test_sim_order_small_candidate_buffer(monkeypatch):
    """A threshold between the two: the selection descends until the bucket
    fits, and the output does not change."""
    n = 1025
    case = so.order_tablet(n)
    full = so.ordered(so.order_items(n, [], (0, 4)), y.T_BOOL, False, False)
    seen = []
    for cand, passes in ((None, 1), ("16", None), ("2", None),
                         ("1", so.FULL_DEPTH)):
        if cand is None:
            monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
        else:
            monkeypatch.setenv("YBG_SNAP_ORDER_CAND", cand)
        _rows, raw, res = so.check(run, case, so.ORDER_READ, [],
                                   so.ORDER_COLS, (0, 4), full, limit=10,
                                   passes=passes, cap=n)
        # a bool column: 512 equal values cannot fit 16 candidates before
        # the position digits split them
        if cand in ("16", "2"):
            assert 9 <= res.digit_passes <= so.FULL_DEPTH
        seen.append(so.raw_bytes(raw, res, len(so.ORDER_COLS), n))
    assert all(s == seen[0] for s in seen[1:])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("ob", [(0, 0), (0, 1)])
def test_sim_order_paging(ob, desc, monkeypatch):
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    n = 2 * ss.tile_rows() + 1
    for page in so.page_sizes(n):
        # page 1 walks every cursor position: on the small tablet only
        m = 129 if page == 1 else n
        for nf in (False, True):
            so.scenario_paging(run, m, ob, desc, nf,
                               page if page <= m else m + 1)


def test_sim_order_more_tiles_than_the_grid(monkeypatch):
    monkeypatch.delenv("YBG_SNAP_ORDER_CAND", raising=False)
    so.scenario_large(run)
    monkeypatch.setenv("YBG_SNAP_ORDER_CAND", "1")
    so.scenario_large(run, cand_one=True)


def test_sim_order_string_projection():
    so.scenario_strings(run)


def test_sim_order_errors(cases):
    """The simulator shares the translation code: the same codes (it
    reports no message text)."""
    so.scenario_errors(run, cases)
