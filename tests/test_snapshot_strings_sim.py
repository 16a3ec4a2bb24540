"""CPU parity of string columns on a columnar snapshot: the host simulator
(ybg_sim_snapshot_query_ex / _group_query_ex / _select_var — the off / bytes
/ pfx layout of a stage_strings build, then the snap_device.h prefix compare,
heap tie-break, emit and string copy code the gfx950 kernels run) against the
CPU oracle on the same tablet. The scenarios live in
snapshot_string_cases.py and run again on the kernels in
test_snapshot_strings_gpu.py."""
import pytest

import ybgpu as y
from parity_cases import build_cases, make_spec
import snapshot_string_cases as st


@pytest.fixture(scope="module")
def cases():
    return build_cases()


class SimRunner:
    """Every call builds its own simulated snapshot."""

    @staticmethod
    def _spec(case, read_micros):
        # the spec carries the read time only: the build ignores the rest
        return make_spec(case, read_micros, (), ())

    def query(self, case, read_micros, preds, aggs, strings=True):
        return y.sim_snapshot_query(
            self._spec(case, read_micros), case["data"], case["offsets"],
            case["n_blocks"], list(preds), list(aggs), strings=strings)

    def group(self, case, read_micros, preds, aggs, group_col,
              group_is_key=False, strings=True):
        return y.sim_snapshot_group_query(
            self._spec(case, read_micros), case["data"], case["offsets"],
            case["n_blocks"], list(preds), list(aggs), group_col,
            group_is_key, strings=strings)

    def select_var(self, case, read_micros, preds, cols, limit=0,
                   backward=False, row_lo=0, row_hi=None, cap=st.CAP,
                   varlen_cap=st.VCAP, strings=True):
        raw, res = y.sim_snapshot_select_var(
            self._spec(case, read_micros), case["data"], case["offsets"],
            case["n_blocks"], list(preds), list(cols), limit, backward,
            row_lo, row_hi, cap, varlen_cap, strings)
        rows = y.decode_snapshot_rows(
            res, raw[0], raw[1], len(cols), cols, cap, raw[3],
            y.select_string_cols(case["schema"], cols))
        return rows, raw, res

    def select_plain(self, case, read_micros, preds, cols, strings=True):
        # the plain select = select_var's contract without a heap; the
        # simulator's plain entry point builds without strings
        if not strings:
            raw, res = y.sim_snapshot_select(
                self._spec(case, read_micros), case["data"], case["offsets"],
                case["n_blocks"], list(preds), list(cols), cap=st.CAP)
        else:
            raw, res = _sim_select_plain_on_strings(
                self._spec(case, read_micros), case, preds, cols)
        rows = y.decode_snapshot_rows(res, raw[0], raw[1], len(cols), cols,
                                      st.CAP)
        return rows, raw, res


def _sim_select_plain_on_strings(spec, case, preds, cols):
    """yb_gpu_snapshot_select's contract on a string snapshot:
    ybg_sim_snapshot_select_var with no varlen_size."""
    import ctypes as C
    f = y._sig(y.product(), "ybg_sim_snapshot_select_var", C.c_int,
               [C.POINTER(y.ScanSpec), C.POINTER(C.c_uint8),
                C.POINTER(C.c_uint64), C.c_uint64,
                C.POINTER(y.SnapshotSelect), C.c_int, C.POINTER(C.c_uint64),
                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64,
                C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64),
                C.POINTER(y.SnapshotSelectResult)])
    q = y.snapshot_select(list(preds), list(cols))
    cap = st.CAP
    datums = (C.c_uint64 * (cap * max(1, len(cols))))()
    null_masks = (C.c_uint32 * cap)()
    row_ids = (C.c_uint64 * cap)()
    res = y.SnapshotSelectResult()
    rc = f(C.byref(spec), case["data"], case["offsets"], case["n_blocks"],
           C.byref(q), 1, datums, null_masks, row_ids, cap, None, 0, None,
           C.byref(res))
    if rc:
        err = RuntimeError(f"ybg_sim_snapshot_select_var failed rc={rc}")
        err.code = rc
        err.result = res
        raise err
    return (datums, null_masks, row_ids), res


@pytest.fixture
def r():
    return SimRunner()


def test_sim_strings_parity_on_string_cases(r, cases):
    st.scenario_parity(r, cases)


def test_sim_strings_parity_select(r, cases):
    st.scenario_parity_select(r, cases)


def test_sim_strings_group_string_tablet(r):
    st.scenario_string_tablet(r)


@pytest.mark.parametrize("op", st.CMP_OPS)
@pytest.mark.parametrize("is_key", [0, 1])
def test_sim_strings_corner_compare(r, is_key, op):
    st.scenario_corner_compare(r, is_key, op)


def test_sim_strings_corner_in(r):
    st.scenario_corner_in(r)


def test_sim_strings_null_is_not_empty(r):
    st.scenario_null_vs_empty(r)


@pytest.mark.parametrize("n", st.edge_sizes())
def test_sim_strings_shape_edges(r, n):
    st.scenario_edge(r, n)


def test_sim_strings_large(r):
    st.scenario_large(r)


def test_sim_strings_select_directions(r):
    st.scenario_select_directions(r)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("limit", [1, 7, 600])
def test_sim_strings_select_paging(r, limit, backward):
    st.scenario_select_paging(r, limit, backward)


def test_sim_strings_select_window(r):
    st.scenario_select_window(r)


def test_sim_strings_varlen_cap(r):
    st.scenario_varlen_cap(r)


def test_sim_strings_determinism():
    st.scenario_determinism(SimRunner)


def test_sim_default_snapshot_refuses_strings(r):
    st.scenario_default_refuses(r)


def test_sim_string_snapshot_refusals(r):
    st.scenario_string_refusals(r)


def test_stageable_strings_flag():
    """stageable(strings=False) is today's answer; strings=True adds exactly
    string compares / IN and COUNT(string)."""
    case = st.corner_tablet()
    sc = case["schema"]
    sp = [st.str_pred(0, 0, y.PRED_LE, b"a")]
    kp = [st.str_in(1, 1, [b"a", b""])]
    cnt = [y.Agg(y.AGG_COUNT, 0)]
    for preds, aggs in ((sp, []), (kp, []), ([], cnt)):
        assert not y.stageable(sc, preds, aggs)
        assert y.stageable(sc, preds, aggs, strings=True)
    num = [y.Pred(0, 1, y.PRED_GT, 3, None, 0)]
    assert y.stageable(sc, num, [y.Agg(y.AGG_SUM_INT64, 1)])
    assert y.stageable(sc, num, [y.Agg(y.AGG_SUM_INT64, 1)], strings=True)
