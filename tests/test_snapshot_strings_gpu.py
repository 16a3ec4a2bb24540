"""String columns on a columnar snapshot, on the GPU: the stage_strings build
(k_emit into a counted heap, k_snap_str_len / exclusive scan /
k_snap_str_pack), the string predicates of the three query kernels and
yb_gpu_snapshot_select_var against the CPU oracle — the scenarios of
snapshot_string_cases.py that test_snapshot_strings_sim.py runs on the
simulator — plus what only the device can show: byte-identical output across
separately built snapshots and equal to the simulator's, string_info, error
messages and memory accounting. All tests require an MI355X (gfx950)."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec
import snapshot_string_cases as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def _gpu():
    import gpu_scan
    if not gpu_scan.gpu_available():
        pytest.fail("no HIP device visible — gpu-marked test must run on GPU")
    return gpu_scan


def build_snapshot(case, read_micros, strings):
    gpu_scan = _gpu()
    s = gpu_scan.GpuScan(make_spec(case, read_micros, (), ()))
    s.feed_blocks_host(case["data"], case["offsets"], case["n_blocks"],
                       case["total"])
    snap = s.snapshot(strings=strings)
    s.close()
    return snap


class Runner:
    """One snapshot per (tablet, read time, strings), built on first use and
    kept for the following queries."""

    def __init__(self):
        self.snaps = {}

    def snapshot(self, case, read_micros, strings=True):
        key = (case["name"], read_micros, strings)
        if key not in self.snaps:
            self.snaps[key] = build_snapshot(case, read_micros, strings)
        return self.snaps[key]

    def query(self, case, read_micros, preds, aggs, strings=True):
        return self.snapshot(case, read_micros, strings).query(
            list(preds), list(aggs))

    def group(self, case, read_micros, preds, aggs, group_col,
              group_is_key=False, strings=True):
        snap = self.snapshot(case, read_micros, strings)
        keys, vals, cnts, res = snap.group_query_raw(
            list(preds), list(aggs), group_col, group_is_key, cap=st.CAP)
        return (y.decode_snapshot_groups(res, keys, vals, cnts, list(aggs)),
                (keys, vals, cnts), res)

    def select_var(self, case, read_micros, preds, cols, limit=0,
                   backward=False, row_lo=0, row_hi=None, cap=st.CAP,
                   varlen_cap=st.VCAP, strings=True):
        snap = self.snapshot(case, read_micros, strings)
        datums, null_masks, row_ids, varlen, vsize, res = \
            snap.select_var_raw(list(preds), list(cols), limit, backward,
                                row_lo, row_hi, cap, varlen_cap)
        rows = y.decode_snapshot_rows(
            res, datums, null_masks, len(cols), cols, cap, varlen,
            y.select_string_cols(case["schema"], cols))
        return rows, (datums, null_masks, row_ids, varlen, vsize), res

    def select_plain(self, case, read_micros, preds, cols, strings=True):
        snap = self.snapshot(case, read_micros, strings)
        datums, null_masks, row_ids, res = snap.select_raw(
            list(preds), list(cols), cap=st.CAP)
        rows = y.decode_snapshot_rows(res, datums, null_masks, len(cols),
                                      cols, st.CAP)
        return rows, (datums, null_masks, row_ids), res

    def close(self):
        for snap in self.snaps.values():
            snap.close()
        self.snaps = {}


@pytest.fixture
def r():
    runner = Runner()
    yield runner
    runner.close()


def test_strings_parity_on_string_cases(r, cases):
    st.scenario_parity(r, cases)


def test_strings_parity_select(r, cases):
    st.scenario_parity_select(r, cases)


def test_strings_group_string_tablet(r):
    st.scenario_string_tablet(r)


@pytest.mark.parametrize("op", st.CMP_OPS)
@pytest.mark.parametrize("is_key", [0, 1])
def test_strings_corner_compare(r, is_key, op):
    st.scenario_corner_compare(r, is_key, op)


def test_strings_corner_in(r):
    st.scenario_corner_in(r)


def test_strings_null_is_not_empty(r):
    st.scenario_null_vs_empty(r)


@pytest.mark.parametrize("n", st.edge_sizes())
def test_strings_shape_edges(r, n):
    st.scenario_edge(r, n)


def test_strings_large(r):
    st.scenario_large(r)


def test_strings_select_directions(r):
    st.scenario_select_directions(r)
    # GpuSnapshot.select picks select_var for a string projection
    case = st.edge_tablet(2 * st.tile_rows() + 1)
    cols = [(0, 0), (0, 1), (1, 1)]
    rows, res = r.snapshot(case, st.READ).select([], cols, limit=50)
    assert res.n_rows == 50
    assert rows == [(st.edge_value(i), i, st.edge_key(i)) for i in range(50)]


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("limit", [1, 7, 600])
def test_strings_select_paging(r, limit, backward):
    st.scenario_select_paging(r, limit, backward)


def test_strings_select_window(r):
    st.scenario_select_window(r)


def test_strings_varlen_cap(r):
    st.scenario_varlen_cap(r)


def test_strings_determinism_and_simulator():
    """Two separately built snapshots, each selected twice: byte-identical
    row_ids / null_masks / datums / heap, equal to the simulator's."""
    runners = []

    def fresh():
        runners.append(Runner())
        return runners[-1]

    try:
        raw = st.scenario_determinism(fresh)
        assert len(runners) == 2
    finally:
        for runner in runners:
            runner.close()
    case, preds, cols = st.determinism_query()
    sraw, sres = y.sim_snapshot_select_var(
        make_spec(case, st.READ, (), ()), case["data"], case["offsets"],
        case["n_blocks"], preds, cols, cap=st.CAP, varlen_cap=st.VCAP)
    assert st.raw_bytes(sraw, sres, len(cols), st.CAP) == raw


def test_default_snapshot_refuses_strings(r):
    st.scenario_default_refuses(r, message=True)
    info = r.snapshot(st.corner_tablet(), st.READ, strings=False) \
        .string_info()
    assert info.staged_string_value_cols == 0
    assert info.staged_string_key_cols == 0
    assert not any(info.string_bytes) and not any(info.key_string_bytes)


def test_string_snapshot_refusals(r):
    st.scenario_string_refusals(r, message=True)


def test_strings_info_and_device_bytes(r):
    n = st.tile_rows() + 1
    case = st.edge_tablet(n)
    plain = r.snapshot(case, st.READ, strings=False)
    snap = r.snapshot(case, st.READ, strings=True)
    info, sinfo = snap.info(), snap.string_info()
    # staged_value_cols keeps meaning "numeric staged"
    assert info.staged_value_cols == plain.info().staged_value_cols == 0b10
    assert info.n_rows == n
    assert sinfo.staged_string_value_cols == 0b01
    assert sinfo.staged_string_key_cols == 0b10
    vbytes = sum(len(st.edge_value(i) or b"") for i in range(n))
    kbytes = sum(len(st.edge_key(i)) for i in range(n))
    assert sinfo.string_bytes[0] == vbytes
    assert sinfo.key_string_bytes[1] == kbytes
    assert sinfo.string_bytes[1] == 0 and sinfo.key_string_bytes[0] == 0
    # off + pfx (16 B per row) plus the bytes, per staged string column
    assert info.device_bytes - plain.info().device_bytes >= \
        2 * 16 * n + vbytes + kbytes
    cols = st.all_cols(case["schema"])
    st.check_select(r, case, [], cols)
    after = snap.info().device_bytes
    assert after > info.device_bytes     # select scratch, offsets, heap
    st.check_select(r, case, [], cols)
    assert snap.info().device_bytes == after   # nothing regrown
