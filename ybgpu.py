"""ybgpu — ctypes bindings for the MI355X-native DocDB scan path.

Product library:  yugabyte-db_amd/libybgpu.so  (C ABI: include/yb_gpu_scan.h)
Oracle library:   oracle/liborcl.so            (TEST INFRASTRUCTURE ONLY:
    only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
    call the oracle — see oracle/orcl.h.)
"""
import ctypes as C
import os

_ROOT = os.path.dirname(os.path.abspath(__file__))
_PRODUCT_SO = os.environ.get(
    "YBG_SO", os.path.join(_ROOT, "yugabyte-db_amd", "libybgpu.so"))
_ORACLE_SO = os.path.join(_ROOT, "oracle", "liborcl.so")

MAX_COLS = 32
MAX_KEYCOLS = 8
MAX_PREDS = 8
MAX_AGGS = 8
MAX_HT = 16

# dtypes (ybg_dtype_t / orcl_dtype_t share values)
T_BOOL, T_INT8, T_INT16, T_INT32, T_INT64 = 0, 1, 2, 3, 4
T_UINT32, T_UINT64, T_FLOAT, T_DOUBLE, T_STRING = 5, 6, 7, 8, 9
KT_INT64, KT_INT32, KT_STRING = 0, 1, 2
ENC_SHARED_PREFIX, ENC_THREE_SHARED_PARTS = 0, 1
PRED_GT, PRED_GE, PRED_LT, PRED_LE, PRED_EQ, PRED_NE, PRED_IN, \
    PRED_IN_TUPLE, PRED_IN_RANGE = range(9)
(AGG_COUNT, AGG_COUNT_STAR, AGG_SUM_INT64, AGG_SUM_DOUBLE,
 AGG_MIN_INT64, AGG_MAX_INT64, AGG_MIN_DOUBLE, AGG_MAX_DOUBLE) = range(8)


class ValueCol(C.Structure):
    _fields_ = [("column_id", C.c_int32), ("dtype", C.c_int32),
                ("nullable", C.c_int32)]


class Schema(C.Structure):
    _fields_ = [
        ("has_hash", C.c_int32),
        ("num_hash_cols", C.c_int32),
        ("num_range_cols", C.c_int32),
        ("key_types", C.c_int32 * MAX_KEYCOLS),
        ("num_value_cols", C.c_int32),
        ("value_cols", ValueCol * MAX_COLS),
    ]


class ReadTime(C.Structure):
    _fields_ = [
        ("read", C.c_uint8 * MAX_HT), ("read_len", C.c_int32),
        ("local_limit", C.c_uint8 * MAX_HT), ("local_limit_len", C.c_int32),
        ("global_limit", C.c_uint8 * MAX_HT), ("global_limit_len", C.c_int32),
    ]


class Pred(C.Structure):
    _fields_ = [
        ("is_key_col", C.c_int32), ("col", C.c_int32), ("op", C.c_int32),
        ("datum", C.c_uint64), ("bytes", C.POINTER(C.c_uint8)),
        ("bytes_len", C.c_uint64),
    ]


class Agg(C.Structure):
    _fields_ = [("op", C.c_int32), ("col", C.c_int32)]


class ScanSpec(C.Structure):
    _fields_ = [
        ("schema", Schema),
        ("kv_format", C.c_int32),
        ("read_time", ReadTime),
        ("num_preds", C.c_int32),
        ("preds", Pred * MAX_PREDS),
        ("num_aggs", C.c_int32),
        ("aggs", Agg * MAX_AGGS),
        ("lower_bound", C.POINTER(C.c_uint8)), ("lower_bound_len", C.c_uint64),
        ("upper_bound", C.POINTER(C.c_uint8)), ("upper_bound_len", C.c_uint64),
        ("emit_rows", C.c_int32),
        ("row_limit", C.c_uint64),
        ("group_col", C.c_int32),  # 0 = none, else 1 + value column index
        ("backward", C.c_int32),   # descending delivery order
        ("expect_versions", C.c_int32),  # MVCC-heavy hint (kernel shape)
    ]


class AggResult(C.Structure):
    _fields_ = [("value_i64", C.c_int64), ("value_f64", C.c_double),
                ("is_null", C.c_int32), ("pad_", C.c_int32)]


class ScanResult(C.Structure):
    _fields_ = [("rows_scanned", C.c_uint64), ("rows_matched", C.c_uint64),
                ("entries_seen", C.c_uint64), ("aggs", AggResult * MAX_AGGS),
                ("restart_ht", C.c_uint8 * MAX_HT),
                ("restart_ht_len", C.c_uint32), ("pad2_", C.c_uint32)]


class RowBatch(C.Structure):
    _fields_ = [
        ("n_rows", C.c_uint64), ("n_key_cols", C.c_uint64),
        ("n_value_cols", C.c_uint64),
        ("sort_key", C.POINTER(C.c_uint64)),
        ("key_datums", C.POINTER(C.c_uint64)),
        ("datums", C.POINTER(C.c_uint64)),
        ("null_masks", C.POINTER(C.c_uint32)),
        ("hashes", C.POINTER(C.c_uint16)),
        ("varlen", C.POINTER(C.c_uint8)),
        ("varlen_size", C.c_uint64),
    ]


class Key(C.Structure):
    _fields_ = [
        ("hash", C.c_uint16),
        ("datums", C.c_uint64 * MAX_KEYCOLS),
        ("strs", C.POINTER(C.c_uint8) * MAX_KEYCOLS),
        ("str_lens", C.c_uint64 * MAX_KEYCOLS),
    ]


class RowVals(C.Structure):
    _fields_ = [
        ("datums", C.c_uint64 * MAX_COLS),
        ("strs", C.POINTER(C.c_uint8) * MAX_COLS),
        ("str_lens", C.c_uint64 * MAX_COLS),
        ("null", C.c_uint8 * MAX_COLS),
    ]


class GenParams(C.Structure):
    _fields_ = [
        ("rows", C.c_uint64), ("seed", C.c_uint64),
        ("packed_version", C.c_int32), ("kv_format", C.c_int32),
        ("block_size", C.c_uint32), ("restart_interval", C.c_int32),
        ("versions", C.c_int32),
        ("ht_base_micros", C.c_uint64), ("ht_step_micros", C.c_uint64),
        ("nthreads", C.c_int32),
        ("group_mod", C.c_uint64),
    ]


def _sig(lib, name, res, args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = args
    return f


_product = None
_oracle = None


def product():
    """The product library (GPU path + generator)."""
    global _product
    if _product is None:
        _product = C.CDLL(_PRODUCT_SO)
    return _product


def oracle():
    """The CPU oracle — TEST INFRASTRUCTURE ONLY."""
    global _oracle
    if _oracle is None:
        _oracle = C.CDLL(_ORACLE_SO)
    return _oracle


def make_schema(key_types, value_cols, has_hash=True, num_hash_cols=1):
    """value_cols: list of (column_id, dtype, nullable)."""
    s = Schema()
    s.has_hash = 1 if has_hash else 0
    s.num_hash_cols = num_hash_cols if has_hash else 0
    s.num_range_cols = len(key_types) - s.num_hash_cols
    for i, kt in enumerate(key_types):
        s.key_types[i] = kt
    s.num_value_cols = len(value_cols)
    for i, (cid, dt, nul) in enumerate(value_cols):
        s.value_cols[i] = ValueCol(cid, dt, nul)
    return s


def read_time(read_micros, local_micros=None, global_micros=None, lib=None):
    rt = ReadTime()
    lib = lib or product()
    f = _sig(lib, "ybg_read_time_init", None,
             [C.POINTER(ReadTime), C.c_uint64, C.c_uint64, C.c_uint64])
    local_micros = read_micros if local_micros is None else local_micros
    global_micros = local_micros if global_micros is None else global_micros
    f(C.byref(rt), read_micros << 12, local_micros << 12, global_micros << 12)
    return rt


def generate(schema, rows, seed=42, packed_version=2,
             kv_format=ENC_THREE_SHARED_PARTS, block_size=4096,
             restart_interval=16, versions=1, ht_base_micros=1_600_000_000_000_000,
             ht_step_micros=1000, nthreads=0, group_mod=0):
    """Run the multithreaded dataset generator. Returns (data, offsets,
    n_blocks, total_bytes, n_entries); data/offsets are ctypes pointers owned
    by the caller (freed via ybg_free at process exit — we keep them)."""
    lib = product()
    f = _sig(lib, "ybg_generate", C.c_int,
             [C.POINTER(Schema), C.POINTER(GenParams),
              C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_uint64)),
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
              C.POINTER(C.c_uint64)])
    p = GenParams(rows, seed, packed_version, kv_format, block_size,
                  restart_interval, versions, ht_base_micros, ht_step_micros,
                  nthreads, group_mod)
    data = C.POINTER(C.c_uint8)()
    offsets = C.POINTER(C.c_uint64)()
    n_blocks = C.c_uint64()
    total = C.c_uint64()
    n_entries = C.c_uint64()
    rc = f(C.byref(schema), C.byref(p), C.byref(data), C.byref(offsets),
           C.byref(n_blocks), C.byref(total), C.byref(n_entries))
    assert rc == 0
    return data, offsets, n_blocks.value, total.value, n_entries.value


class Builder:
    """Low-level tablet builder (entries must be added in key order)."""

    def __init__(self, schema, kv_format=ENC_THREE_SHARED_PARTS,
                 block_size=4096, restart_interval=16):
        lib = product()
        self._lib = lib
        self._schema = schema
        self._create = _sig(lib, "ybg_builder_create", C.c_void_p,
                            [C.POINTER(Schema), C.c_int, C.c_size_t, C.c_int])
        self._h = self._create(C.byref(schema), kv_format, block_size,
                               restart_interval)
        self._add_packed = _sig(lib, "ybg_builder_add_packed_row", C.c_int,
                                [C.c_void_p, C.POINTER(Key), C.c_uint64,
                                 C.c_uint32, C.c_uint64, C.c_int,
                                 C.POINTER(RowVals)])
        self._add_col = _sig(lib, "ybg_builder_add_column_update", C.c_int,
                             [C.c_void_p, C.POINTER(Key), C.c_int, C.c_uint64,
                              C.c_uint32, C.c_uint64, C.c_uint64,
                              C.POINTER(C.c_uint8), C.c_uint64, C.c_int])
        self._add_tomb = _sig(lib, "ybg_builder_add_row_tombstone", C.c_int,
                              [C.c_void_p, C.POINTER(Key), C.c_uint64,
                               C.c_uint32, C.c_uint64])
        self._finish = _sig(lib, "ybg_builder_finish", C.c_int,
                            [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)),
                             C.POINTER(C.POINTER(C.c_uint64)),
                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                             C.POINTER(C.c_uint64)])
        self._seq = 1 << 50
        self._keepalive = []

    def _key(self, hash_=0, datums=(), strs=()):
        k = Key()
        k.hash = hash_
        for i, d in enumerate(datums):
            k.datums[i] = d & 0xFFFFFFFFFFFFFFFF
        for i, s in enumerate(strs):
            if s is not None:
                buf = C.create_string_buffer(s, len(s))
                self._keepalive.append(buf)
                k.strs[i] = C.cast(buf, C.POINTER(C.c_uint8))
                k.str_lens[i] = len(s)
        return k

    def add_packed_row(self, ht_micros, values, hash_=0, key_datums=(),
                       key_strs=(), write_id=0, packed_version=2, seq=None,
                       logical=0):
        """values: list of (dtype, value-or-None[null]) per schema order;
        ints as int, doubles as float, strings as bytes."""
        k = self._key(hash_, key_datums, key_strs)
        v = RowVals()
        import struct
        for i, (dt, val) in enumerate(values):
            if val is None:
                v.null[i] = 1
            elif dt == T_DOUBLE:
                v.datums[i] = struct.unpack("<Q", struct.pack("<d", val))[0]
            elif dt == T_FLOAT:
                v.datums[i] = struct.unpack("<I", struct.pack("<f", val))[0]
            elif dt == T_STRING:
                buf = C.create_string_buffer(val, len(val))
                self._keepalive.append(buf)
                v.strs[i] = C.cast(buf, C.POINTER(C.c_uint8))
                v.str_lens[i] = len(val)
            else:
                v.datums[i] = val & 0xFFFFFFFFFFFFFFFF
        seq = self._next_seq(seq)
        rc = self._add_packed(self._h, C.byref(k), (ht_micros << 12) | logical,
                              write_id, seq, packed_version, C.byref(v))
        assert rc == 0

    def add_column_update(self, ht_micros, col_idx, value, hash_=0,
                          key_datums=(), key_strs=(), write_id=0, seq=None,
                          null=False, logical=0):
        import struct
        k = self._key(hash_, key_datums, key_strs)
        datum = 0
        sp = None
        slen = 0
        dt = self._schema.value_cols[col_idx].dtype
        if value is None:
            null = True
        elif dt == T_DOUBLE:
            datum = struct.unpack("<Q", struct.pack("<d", value))[0]
        elif dt == T_FLOAT:
            datum = struct.unpack("<I", struct.pack("<f", value))[0]
        elif dt == T_STRING:
            buf = C.create_string_buffer(value, len(value))
            self._keepalive.append(buf)
            sp = C.cast(buf, C.POINTER(C.c_uint8))
            slen = len(value)
        else:
            datum = value & 0xFFFFFFFFFFFFFFFF
        seq = self._next_seq(seq)
        rc = self._add_col(self._h, C.byref(k), col_idx,
                           (ht_micros << 12) | logical, write_id, seq, datum,
                           sp, slen, 1 if null else 0)
        assert rc == 0

    def add_row_tombstone(self, ht_micros, hash_=0, key_datums=(), key_strs=(),
                          write_id=0, seq=None, logical=0):
        k = self._key(hash_, key_datums, key_strs)
        seq = self._next_seq(seq)
        rc = self._add_tomb(self._h, C.byref(k), (ht_micros << 12) | logical,
                            write_id, seq)
        assert rc == 0

    def _next_seq(self, seq):
        if seq is None:
            seq = self._seq
            self._seq += 1
        return seq

    def finish(self):
        data = C.POINTER(C.c_uint8)()
        offsets = C.POINTER(C.c_uint64)()
        n_blocks = C.c_uint64()
        total = C.c_uint64()
        n_entries = C.c_uint64()
        rc = self._finish(self._h, C.byref(data), C.byref(offsets),
                          C.byref(n_blocks), C.byref(total), C.byref(n_entries))
        assert rc == 0
        return data, offsets, n_blocks.value, total.value, n_entries.value

    def finish_sst(self, compression=0):
        """Finish as a complete BlockBasedTable SST file; returns
        (data_ptr, total_bytes, n_blocks, n_entries). compression: 0 none,
        1 snappy, 4 = LZ4 (blocks that do not shrink stay uncompressed)."""
        lib = product()
        f = _sig(lib, "ybg_builder_finish_sst2", C.c_int,
                 [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint8)),
                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                  C.POINTER(C.c_uint64)])
        data = C.POINTER(C.c_uint8)()
        total = C.c_uint64()
        n_blocks = C.c_uint64()
        n_entries = C.c_uint64()
        rc = f(self._h, compression, C.byref(data), C.byref(total),
               C.byref(n_blocks), C.byref(n_entries))
        assert rc == 0
        return data, total.value, n_blocks.value, n_entries.value


def sst_index(file_ptr, size=None, verify=True, cap=1 << 20):
    """Parse an SST file's footer + index: data-block (offset, size) lists.
    Raises RuntimeError on corrupt input. file_ptr: ctypes pointer or
    bytes."""
    lib = product()
    f = _sig(lib, "ybg_sst_index", C.c_int,
             [C.POINTER(C.c_uint8), C.c_uint64, C.c_int,
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64,
              C.POINTER(C.c_uint64)])
    if isinstance(file_ptr, (bytes, bytearray)):
        buf = (C.c_uint8 * len(file_ptr)).from_buffer_copy(file_ptr)
        file_ptr = C.cast(buf, C.POINTER(C.c_uint8))
        size = len(buf)
    offs = (C.c_uint64 * cap)()
    szs = (C.c_uint64 * cap)()
    n = C.c_uint64()
    rc = f(file_ptr, size, 1 if verify else 0, offs, szs, cap, C.byref(n))
    if rc:
        err = _sig(lib, "yb_gpu_last_error", C.c_char_p, [])
        raise RuntimeError("sst_index: rc=%d %s" % (rc, err().decode()))
    return list(offs[:n.value]), list(szs[:n.value])


# ---------------------------------------------------------------------------
# Oracle wrappers (TEST INFRASTRUCTURE ONLY)
# ---------------------------------------------------------------------------

class OrclRow(C.Structure):
    _fields_ = [
        ("key_datums", C.c_uint64 * MAX_KEYCOLS),
        ("key_str", C.POINTER(C.c_uint8) * MAX_KEYCOLS),
        ("key_str_len", C.c_uint32 * MAX_KEYCOLS),
        ("datums", C.c_uint64 * MAX_COLS),
        ("strp", C.POINTER(C.c_uint8) * MAX_COLS),
        ("strlen_", C.c_uint32 * MAX_COLS),
        ("null_mask", C.c_uint32),
        ("seq_in_scan", C.c_uint64),
    ]


ORCL_ROW_CB = C.CFUNCTYPE(C.c_int, C.POINTER(OrclRow), C.c_void_p)


class OrclValueCol(C.Structure):
    _fields_ = [("column_id", C.c_int32), ("dtype", C.c_int32),
                ("nullable", C.c_int32)]


class OrclSchema(C.Structure):
    _fields_ = [
        ("has_hash", C.c_int), ("num_hash_cols", C.c_int),
        ("num_range_cols", C.c_int), ("key_types", C.c_int * MAX_KEYCOLS),
        ("num_value_cols", C.c_int), ("value_cols", OrclValueCol * MAX_COLS),
    ]


class OrclReadTime(C.Structure):
    _fields_ = [
        ("read", C.c_uint8 * MAX_HT), ("read_len", C.c_size_t),
        ("local_limit", C.c_uint8 * MAX_HT), ("local_limit_len", C.c_size_t),
        ("global_limit", C.c_uint8 * MAX_HT), ("global_limit_len", C.c_size_t),
    ]


class OrclPred(C.Structure):
    _fields_ = [("is_key_col", C.c_int), ("col", C.c_int), ("op", C.c_int),
                ("datum", C.c_uint64), ("bytes", C.POINTER(C.c_uint8)),
                ("bytes_len", C.c_size_t)]


class OrclAgg(C.Structure):
    _fields_ = [("op", C.c_int), ("col", C.c_int)]


class OrclScanSpec(C.Structure):
    _fields_ = [
        ("read_time", OrclReadTime),
        ("num_preds", C.c_int), ("preds", OrclPred * MAX_PREDS),
        ("num_aggs", C.c_int), ("aggs", OrclAgg * MAX_AGGS),
        ("lower_bound", C.POINTER(C.c_uint8)), ("lower_bound_len", C.c_size_t),
        ("upper_bound", C.POINTER(C.c_uint8)), ("upper_bound_len", C.c_size_t),
    ]


class OrclAggResult(C.Structure):
    _fields_ = [("value_i64", C.c_int64), ("value_f64", C.c_double),
                ("is_null", C.c_int)]


class OrclScanResult(C.Structure):
    _fields_ = [("rows_scanned", C.c_uint64), ("rows_matched", C.c_uint64),
                ("entries_seen", C.c_uint64),
                ("aggs", OrclAggResult * MAX_AGGS),
                ("restart_ht", C.c_uint8 * MAX_HT),
                ("restart_ht_len", C.c_uint32), ("pad2_", C.c_uint32)]


def sim_scan(spec, data, offsets, n_blocks):
    """Run the host SIMULATOR of the GPU per-interval algorithm
    (scan_device.h via ybg_sim_scan) — TEST INFRASTRUCTURE; sequentially
    executes the exact device code path on CPU."""
    lib = product()
    f = _sig(lib, "ybg_sim_scan", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(ScanResult)])
    res = ScanResult()
    rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(res))
    if rc != 0:
        raise RuntimeError(f"ybg_sim_scan failed rc={rc}")
    return res


class SnapshotQuery(C.Structure):
    """ybg_snapshot_query_t."""
    _fields_ = [("num_preds", C.c_int32), ("preds", Pred * MAX_PREDS),
                ("num_aggs", C.c_int32), ("aggs", Agg * MAX_AGGS)]


class SnapshotInfo(C.Structure):
    """ybg_snapshot_info_t."""
    _fields_ = [("n_rows", C.c_uint64), ("entries_seen", C.c_uint64),
                ("device_bytes", C.c_uint64), ("build_ms", C.c_double),
                ("staged_value_cols", C.c_uint32),
                ("nullable_cols", C.c_uint32),
                ("restart_ht", C.c_uint8 * MAX_HT),
                ("restart_ht_len", C.c_uint32)]


class SnapshotBuildOpts(C.Structure):
    """ybg_snapshot_build_opts_t."""
    _fields_ = [("stage_strings", C.c_int32), ("reserved", C.c_int32 * 7)]


class SnapshotStringInfo(C.Structure):
    """ybg_snapshot_string_info_t."""
    _fields_ = [("staged_string_value_cols", C.c_uint32),
                ("staged_string_key_cols", C.c_uint32),
                ("string_bytes", C.c_uint64 * MAX_COLS),
                ("key_string_bytes", C.c_uint64 * MAX_KEYCOLS)]


def snapshot_query(preds, aggs):
    """Pack predicate / aggregate lists into a SnapshotQuery. Counts over
    the ABI caps are passed through (the ABI answers them with code 9); only
    the first MAX_PREDS / MAX_AGGS entries are copied."""
    q = SnapshotQuery()
    q.num_preds = len(preds)
    for i, p in enumerate(preds[:MAX_PREDS]):
        q.preds[i] = p
    q.num_aggs = len(aggs)
    for i, a in enumerate(aggs[:MAX_AGGS]):
        q.aggs[i] = a
    return q


def _string_in_list_ok(p):
    """[u32 len][bytes] records that fill bytes_len exactly."""
    raw = bytes(p.bytes[:p.bytes_len]) if p.bytes_len else b""
    o = 0
    while o + 4 <= len(raw):
        o += 4 + int.from_bytes(raw[o:o + 4], "little")
    return o == len(raw)


def stageable(schema, preds, aggs, strings=False):
    """Can a columnar snapshot answer this query? Mirrors the ABI's code-9
    rule (yb_gpu_snapshot_query): GT..NE / IN / IN_RANGE predicates on
    numeric value or key columns, aggregates on numeric value columns,
    indices in range, counts within the caps. strings=True: the rule of a
    snapshot built with stage_strings — also GT..NE / IN on string value
    and key columns and COUNT on a string value column."""
    if len(preds) > MAX_PREDS or len(aggs) > MAX_AGGS:
        return False
    nk = schema.num_hash_cols + schema.num_range_cols
    for p in preds:
        if p.op == PRED_IN_TUPLE or not PRED_GT <= p.op <= PRED_IN_RANGE:
            return False
        is_str = False
        if p.is_key_col:
            if not 0 <= p.col < nk:
                return False
            is_str = schema.key_types[p.col] == KT_STRING
        else:
            if not 0 <= p.col < schema.num_value_cols:
                return False
            is_str = schema.value_cols[p.col].dtype == T_STRING
        if is_str:
            if not strings or p.op == PRED_IN_RANGE:
                return False
            if p.bytes_len and not p.bytes:
                return False
            if p.op == PRED_IN and not _string_in_list_ok(p):
                return False
            continue
        if p.op == PRED_IN and (not p.bytes or p.bytes_len % 8):
            return False
        if p.op == PRED_IN_RANGE and (not p.bytes or not p.bytes_len
                                      or p.bytes_len % 24):
            return False
    for a in aggs:
        if not AGG_COUNT <= a.op <= AGG_MAX_DOUBLE:
            return False
        if a.op == AGG_COUNT_STAR:
            continue
        if not 0 <= a.col < schema.num_value_cols:
            return False
        if schema.value_cols[a.col].dtype == T_STRING and \
                not (strings and a.op == AGG_COUNT):
            return False
    return True


def sim_snapshot_query(spec, data, offsets, n_blocks, preds, aggs,
                       strings=False):
    """Host SIMULATOR of the columnar snapshot (ybg_sim_snapshot_query) —
    TEST INFRASTRUCTURE: builds the snapshot layout from the spec's read
    time and bounds (its predicates/aggregates are ignored) and runs the
    device row loop (snap_device.h) over it for (preds, aggs).
    strings=True builds it with stage_strings (ybg_sim_snapshot_query_ex).
    A non-zero code raises RuntimeError carrying .code."""
    lib = product()
    q = snapshot_query(preds, aggs)
    res = ScanResult()
    if strings:
        f = _sig(lib, "ybg_sim_snapshot_query_ex", C.c_int,
                 [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
                  C.POINTER(C.c_uint64), C.c_uint64,
                  C.POINTER(SnapshotQuery), C.c_int, C.POINTER(ScanResult)])
        rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q), 1,
               C.byref(res))
    else:
        f = _sig(lib, "ybg_sim_snapshot_query", C.c_int,
                 [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
                  C.POINTER(C.c_uint64), C.c_uint64,
                  C.POINTER(SnapshotQuery), C.POINTER(ScanResult)])
        rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q),
               C.byref(res))
    if rc != 0:
        err = RuntimeError(f"ybg_sim_snapshot_query failed rc={rc}")
        err.code = rc
        raise err
    return res


class SnapshotGroupQuery(C.Structure):
    """ybg_snapshot_group_query_t."""
    _fields_ = [("num_preds", C.c_int32), ("preds", Pred * MAX_PREDS),
                ("num_aggs", C.c_int32), ("aggs", Agg * MAX_AGGS),
                ("group_is_key_col", C.c_int32), ("group_col", C.c_int32),
                ("expect_groups", C.c_uint64)]


class SnapshotGroupResult(C.Structure):
    """ybg_snapshot_group_result_t."""
    _fields_ = [("n_groups", C.c_uint64), ("rows_scanned", C.c_uint64),
                ("rows_matched", C.c_uint64), ("entries_seen", C.c_uint64),
                ("has_null_group", C.c_int32), ("local_level", C.c_int32),
                ("restart_ht", C.c_uint8 * MAX_HT),
                ("restart_ht_len", C.c_uint32)]


def snapshot_group_query(preds, aggs, group_col, group_is_key=False,
                         expect_groups=0):
    """Pack a grouped snapshot query (counts over the caps pass through,
    as in snapshot_query)."""
    q = SnapshotGroupQuery()
    q.num_preds = len(preds)
    for i, p in enumerate(preds[:MAX_PREDS]):
        q.preds[i] = p
    q.num_aggs = len(aggs)
    for i, a in enumerate(aggs[:MAX_AGGS]):
        q.aggs[i] = a
    q.group_is_key_col = 1 if group_is_key else 0
    q.group_col = group_col
    q.expect_groups = expect_groups
    return q


def snapshot_group_local_slots(num_aggs):
    """LDS-level slot count of the grouped snapshot kernel a query with
    num_aggs aggregates selects (ybg_snapshot_group_local_slots)."""
    f = _sig(product(), "ybg_snapshot_group_local_slots", C.c_uint64,
             [C.c_int32])
    return f(num_aggs)


def decode_snapshot_groups(res, keys, vals, cnts, aggs):
    """Grouped snapshot output -> {key: (aggs...)} in the shape of
    _decode_groups: key None for the NULL group (flagged by the result, so
    a key of 2**64 - 1 stays a key); doubles decoded from bit patterns."""
    import struct
    out = {}
    n = res.n_groups
    for g in range(n):
        k = None if (res.has_null_group and g == n - 1) else keys[g]
        row = []
        for a, ag in enumerate(aggs):
            c = cnts[g * MAX_AGGS + a]
            v = vals[g * MAX_AGGS + a]
            if c == 0:
                row.append(None)
            elif ag.op in (AGG_SUM_DOUBLE, AGG_MIN_DOUBLE, AGG_MAX_DOUBLE):
                row.append(struct.unpack("<d", struct.pack("<q", v))[0])
            else:
                row.append(v)
        out[k] = tuple(row)
    return out


def sim_snapshot_group_query(spec, data, offsets, n_blocks, preds, aggs,
                             group_col, group_is_key=False, expect_groups=0,
                             cap=1 << 16, strings=False):
    """Host SIMULATOR of the grouped snapshot query
    (ybg_sim_snapshot_group_query) — TEST INFRASTRUCTURE: the snapshot
    layout built as in sim_snapshot_query, then the device accumulate /
    flush / export code one simulated workgroup at a time. Returns
    (groups dict, (keys, vals, cnts) raw ctypes arrays, result struct);
    raises RuntimeError carrying .code and .result on a non-zero code.
    strings=True builds the snapshot with stage_strings
    (ybg_sim_snapshot_group_query_ex)."""
    lib = product()
    f = _sig(lib, "ybg_sim_snapshot_group_query_ex", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64,
              C.POINTER(SnapshotGroupQuery), C.c_int, C.POINTER(C.c_uint64),
              C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_uint64,
              C.POINTER(SnapshotGroupResult)]) if strings else _sig(
        lib, "ybg_sim_snapshot_group_query", C.c_int,
        [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
         C.POINTER(C.c_uint64), C.c_uint64,
         C.POINTER(SnapshotGroupQuery), C.POINTER(C.c_uint64),
         C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_uint64,
         C.POINTER(SnapshotGroupResult)])
    q = snapshot_group_query(preds, aggs, group_col, group_is_key,
                             expect_groups)
    keys = (C.c_uint64 * max(cap, 1))()
    vals = (C.c_int64 * (max(cap, 1) * MAX_AGGS))()
    cnts = (C.c_uint64 * (max(cap, 1) * MAX_AGGS))()
    res = SnapshotGroupResult()
    if strings:
        rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q), 1, keys,
               vals, cnts, cap, C.byref(res))
    else:
        rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q), keys,
               vals, cnts, cap, C.byref(res))
    if rc != 0:
        err = RuntimeError(f"ybg_sim_snapshot_group_query failed rc={rc}")
        err.code = rc
        err.result = res
        raise err
    groups = decode_snapshot_groups(res, keys, vals, cnts, list(aggs))
    return groups, (keys, vals, cnts), res


MAX_SELECT_COLS = MAX_COLS + MAX_KEYCOLS
ROW_END = 2**64 - 1


class SelectCol(C.Structure):
    """ybg_select_col_t."""
    _fields_ = [("is_key_col", C.c_int32), ("col", C.c_int32)]


class SnapshotSelect(C.Structure):
    """ybg_snapshot_select_t."""
    _fields_ = [("num_preds", C.c_int32), ("preds", Pred * MAX_PREDS),
                ("num_cols", C.c_int32),
                ("cols", SelectCol * MAX_SELECT_COLS),
                ("backward", C.c_int32),
                ("row_lo", C.c_uint64), ("row_hi", C.c_uint64),
                ("row_limit", C.c_uint64)]


class SnapshotSelectResult(C.Structure):
    """ybg_snapshot_select_result_t."""
    _fields_ = [("n_rows", C.c_uint64), ("rows_scanned", C.c_uint64),
                ("rows_matched", C.c_uint64), ("resume_row", C.c_uint64),
                ("done", C.c_int32), ("entries_seen", C.c_uint64),
                ("restart_ht", C.c_uint8 * MAX_HT),
                ("restart_ht_len", C.c_uint32)]


def snapshot_select(preds, cols, limit=0, backward=False, row_lo=0,
                    row_hi=None):
    """Pack a snapshot select. cols: (is_key_col, col) pairs or SelectCol.
    Counts over the caps pass through (the ABI answers them with code 9);
    row_hi None = to the end."""
    q = SnapshotSelect()
    q.num_preds = len(preds)
    for i, p in enumerate(preds[:MAX_PREDS]):
        q.preds[i] = p
    q.num_cols = len(cols)
    for i, c in enumerate(cols[:MAX_SELECT_COLS]):
        q.cols[i] = c if isinstance(c, SelectCol) else \
            SelectCol(1 if c[0] else 0, c[1])
    q.backward = 1 if backward else 0
    q.row_lo = row_lo
    q.row_hi = ROW_END if row_hi is None else row_hi
    q.row_limit = limit
    return q


def snapshot_select_tile_rows():
    """Rows per compaction tile of the select kernels
    (ybg_snapshot_select_tile_rows)."""
    return _sig(product(), "ybg_snapshot_select_tile_rows", C.c_uint64, [])()


def select_string_cols(schema, cols):
    """Per projected column: is it a string column of the schema?"""
    out = []
    for c in cols:
        is_key, col = (c.is_key_col, c.col) if isinstance(c, SelectCol) else c
        if is_key:
            out.append(schema.key_types[col] == KT_STRING)
        else:
            out.append(schema.value_cols[col].dtype == T_STRING)
    return out


def decode_snapshot_rows(res, datums, null_masks, num_cols, cols, cap,
                         varlen=None, string_cols=None):
    """Select output -> [(projected values..., None for NULL)], one tuple
    per delivered row in delivery order. cols: the (is_key_col, col) pairs
    of the projection; cap: the capacity the arrays were passed with.
    string_cols (select_string_cols) marks the projected string columns:
    their (len << 40) | offset datums are decoded to bytes from varlen."""
    cols = [(c.is_key_col, c.col) if isinstance(c, SelectCol) else c
            for c in cols]
    n = res.n_rows
    by_col = [datums[j * cap:j * cap + n] for j in range(num_cols)]
    if string_cols and any(string_cols):
        mask = (1 << 40) - 1
        for j in range(num_cols):
            if string_cols[j]:
                by_col[j] = [bytes(varlen[(d & mask):(d & mask) + (d >> 40)])
                             for d in by_col[j]]
    rows = list(zip(*by_col))
    for i, nm in enumerate(null_masks[:n]):
        if nm:
            rows[i] = tuple(
                None if (not cols[j][0] and (nm >> cols[j][1]) & 1)
                else rows[i][j] for j in range(num_cols))
    return rows


def sim_snapshot_select(spec, data, offsets, n_blocks, preds, cols, limit=0,
                        backward=False, row_lo=0, row_hi=None, cap=1 << 16):
    """Host SIMULATOR of the snapshot select (ybg_sim_snapshot_select) —
    TEST INFRASTRUCTURE: the snapshot layout built as in sim_snapshot_query,
    then the device bit packing / rank / gather code one simulated tile at a
    time. Returns ((datums, null_masks, row_ids) raw ctypes arrays, result
    struct); raises RuntimeError carrying .code and .result on a non-zero
    code."""
    lib = product()
    f = _sig(lib, "ybg_sim_snapshot_select", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(SnapshotSelect),
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
              C.POINTER(C.c_uint64), C.c_uint64,
              C.POINTER(SnapshotSelectResult)])
    q = snapshot_select(preds, cols, limit, backward, row_lo, row_hi)
    n = max(cap, 1)
    datums = (C.c_uint64 * (n * max(1, min(len(cols), MAX_SELECT_COLS))))()
    null_masks = (C.c_uint32 * n)()
    row_ids = (C.c_uint64 * n)()
    res = SnapshotSelectResult()
    rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q), datums,
           null_masks, row_ids, cap, C.byref(res))
    if rc != 0:
        err = RuntimeError(f"ybg_sim_snapshot_select failed rc={rc}")
        err.code = rc
        err.result = res
        raise err
    return (datums, null_masks, row_ids), res


def sim_snapshot_select_var(spec, data, offsets, n_blocks, preds, cols,
                            limit=0, backward=False, row_lo=0, row_hi=None,
                            cap=1 << 16, varlen_cap=1 << 20, strings=True):
    """Host SIMULATOR of yb_gpu_snapshot_select_var
    (ybg_sim_snapshot_select_var) — TEST INFRASTRUCTURE, as
    sim_snapshot_select; the snapshot is built with stage_strings unless
    strings=False. Returns ((datums, null_masks, row_ids, varlen,
    varlen_size) raw arrays, result struct); raises RuntimeError carrying
    .code, .result and .varlen_size on a non-zero code."""
    lib = product()
    f = _sig(lib, "ybg_sim_snapshot_select_var", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(SnapshotSelect),
              C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64, C.POINTER(C.c_uint64),
              C.POINTER(SnapshotSelectResult)])
    q = snapshot_select(preds, cols, limit, backward, row_lo, row_hi)
    n = max(cap, 1)
    datums = (C.c_uint64 * (n * max(1, min(len(cols), MAX_SELECT_COLS))))()
    null_masks = (C.c_uint32 * n)()
    row_ids = (C.c_uint64 * n)()
    varlen = (C.c_uint8 * max(varlen_cap, 1))()
    vsize = C.c_uint64()
    res = SnapshotSelectResult()
    rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q),
           1 if strings else 0, datums, null_masks, row_ids, cap, varlen,
           varlen_cap, C.byref(vsize), C.byref(res))
    if rc != 0:
        err = RuntimeError(f"ybg_sim_snapshot_select_var failed rc={rc}")
        err.code = rc
        err.result = res
        err.varlen_size = vsize.value
        raise err
    return (datums, null_masks, row_ids, varlen, vsize.value), res


class SnapshotOrder(C.Structure):
    """ybg_snapshot_order_t."""
    _fields_ = [("sel", SnapshotSelect),
                ("order_is_key_col", C.c_int32), ("order_col", C.c_int32),
                ("descending", C.c_int32), ("nulls_first", C.c_int32),
                ("have_cursor", C.c_int32), ("cursor_is_null", C.c_int32),
                ("cursor_datum", C.c_uint64), ("cursor_row", C.c_uint64)]


class SnapshotOrderResult(C.Structure):
    """ybg_snapshot_order_result_t."""
    _fields_ = [("r", SnapshotSelectResult),
                ("cursor_is_null", C.c_int32),
                ("cursor_datum", C.c_uint64), ("cursor_row", C.c_uint64),
                ("digit_passes", C.c_uint32)]


def snapshot_order(preds, cols, order_by, descending=False,
                   nulls_first=False, limit=0, after=None, row_lo=0,
                   row_hi=None, backward=False):
    """Pack an ordered snapshot select. order_by: (is_key_col, col);
    after: the cursor (is_null, datum, row) a previous result carried
    (order_cursor), or None."""
    q = SnapshotOrder()
    q.sel = snapshot_select(preds, cols, limit, backward, row_lo, row_hi)
    q.order_is_key_col = 1 if order_by[0] else 0
    q.order_col = order_by[1]
    q.descending = 1 if descending else 0
    q.nulls_first = 1 if nulls_first else 0
    if after is not None:
        q.have_cursor = 1
        q.cursor_is_null = 1 if after[0] else 0
        q.cursor_datum = after[1]
        q.cursor_row = after[2]
    return q


def order_cursor(res):
    """The cursor of an ordered select's result (the last delivered row), to
    pass as `after`; None when nothing was delivered."""
    if not res.r.n_rows:
        return None
    return (res.cursor_is_null, res.cursor_datum, res.cursor_row)


def snapshot_order_candidate_rows():
    """Default early-out threshold of the ordered select
    (ybg_snapshot_order_candidate_rows)."""
    return _sig(product(), "ybg_snapshot_order_candidate_rows", C.c_uint64,
                [])()


def sim_snapshot_select_ordered(spec, data, offsets, n_blocks, preds, cols,
                                order_by, descending=False,
                                nulls_first=False, limit=0, after=None,
                                row_lo=0, row_hi=None, cap=1 << 16,
                                varlen_cap=1 << 20, strings=False,
                                backward=False):
    """Host SIMULATOR of yb_gpu_snapshot_select_ordered
    (ybg_sim_snapshot_select_ordered) — TEST INFRASTRUCTURE, as
    sim_snapshot_select_var. Returns ((datums, null_masks, row_ids, varlen,
    varlen_size) raw arrays, SnapshotOrderResult); raises RuntimeError
    carrying .code, .result and .varlen_size on a non-zero code."""
    lib = product()
    f = _sig(lib, "ybg_sim_snapshot_select_ordered", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(SnapshotOrder),
              C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64, C.POINTER(C.c_uint64),
              C.POINTER(SnapshotOrderResult)])
    q = snapshot_order(preds, cols, order_by, descending, nulls_first, limit,
                       after, row_lo, row_hi, backward)
    n = max(cap, 1)
    datums = (C.c_uint64 * (n * max(1, min(len(cols), MAX_SELECT_COLS))))()
    null_masks = (C.c_uint32 * n)()
    row_ids = (C.c_uint64 * n)()
    varlen = (C.c_uint8 * max(varlen_cap, 1))()
    vsize = C.c_uint64()
    res = SnapshotOrderResult()
    rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(q),
           1 if strings else 0, datums, null_masks, row_ids, cap, varlen,
           varlen_cap, C.byref(vsize), C.byref(res))
    if rc != 0:
        err = RuntimeError(f"ybg_sim_snapshot_select_ordered failed rc={rc}")
        err.code = rc
        err.result = res
        err.varlen_size = vsize.value
        raise err
    return (datums, null_masks, row_ids, varlen, vsize.value), res


def sim_scan_fast(spec, data, offsets, n_blocks):
    """Host simulator of the SPECIALIZED fast batch scanner
    (scan_batch_fast + general fallback per aborted batch) — TEST
    INFRASTRUCTURE. Returns (ScanResult, n_fallback_batches); raises on
    ineligible specs (rc 9)."""
    lib = product()
    f = _sig(lib, "ybg_sim_scan_fast", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(ScanResult),
              C.POINTER(C.c_uint64)])
    res = ScanResult()
    nf = C.c_uint64()
    rc = f(C.byref(spec), data, offsets, n_blocks, C.byref(res),
           C.byref(nf))
    if rc != 0:
        raise RuntimeError(f"ybg_sim_scan_fast failed rc={rc}")
    return res, nf.value


def sim_scan_fast_known(spec, data, offsets, n_blocks, known_ids):
    """sim_scan_fast given a known abort set (batch ids, any order): listed
    batches go straight to the general scanner — TEST INFRASTRUCTURE.
    Returns (ScanResult, ids of every batch the general scanner ran)."""
    f = _sig(product(), "ybg_sim_scan_fast_known", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64),
              C.c_uint64, C.POINTER(ScanResult), C.POINTER(C.c_uint64),
              C.POINTER(C.c_uint64), C.c_uint64])
    res = ScanResult()
    nf = C.c_uint64()
    known = (C.c_uint64 * max(len(known_ids), 1))(*known_ids)
    cap = 1 << 16
    while True:
        ids = (C.c_uint64 * cap)()
        rc = f(C.byref(spec), data, offsets, n_blocks, known, len(known_ids),
               C.byref(res), C.byref(nf), ids, cap)
        if rc != 0:
            raise RuntimeError(f"ybg_sim_scan_fast_known failed rc={rc}")
        if nf.value <= cap:
            return res, list(ids[:nf.value])
        cap = nf.value


def sim_fast_census(spec, data, offsets, n_blocks, max_blocks=0):
    """Per-trip census of the fast kernel's entry loop over the first
    max_blocks blocks (0 = all), 64 consecutive batches replayed in lockstep
    as one wave (ybg_sim_fast_census) — MEASUREMENT TOOL. Returns a dict of
    counters plus the sp / ns1 / ns2 histograms of the delta entries."""
    f = _sig(product(), "ybg_sim_fast_census", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64,
              C.POINTER(C.c_uint64)])
    out = (C.c_uint64 * 208)()
    rc = f(C.byref(spec), data, offsets, n_blocks, max_blocks, out)
    if rc != 0:
        raise RuntimeError(f"ybg_sim_fast_census failed rc={rc}")
    kinds = ("switch", "restart", "frequent", "c211", "general")
    c = {"waves": out[0], "batches": out[1], "aborted": out[2],
         "wave_trips": out[3], "lane_trips": out[4],
         "wave_delta_trips": out[10], "wave_multi_path_trips": out[11],
         "tail_iters_lockstep": out[17], "tail_iters_lanes": out[18],
         "lds_iters_lockstep": out[19], "lds_iters_lanes": out[20],
         "lane_delta_entries": out[21],
         "restart_ns1_min": out[22], "restart_ns1_max": out[23]}
    for i, k in enumerate(kinds):
        c["wave_trips_" + k] = out[5 + i]
        c["lane_trips_" + k] = out[12 + i]
    c["sp_hist"] = {i: out[32 + i] for i in range(128) if out[32 + i]}
    c["ns1_hist"] = {i: out[160 + i] for i in range(32) if out[160 + i]}
    c["ns2_hist"] = {i: out[192 + i] for i in range(16) if out[192 + i]}
    return c


def sim_scan_planned(spec):
    """True when sim_scan_fast runs this spec through the planned
    packed-row pass (column plan built and YBG_PLAN not 0) — the
    simulator's yb_gpu_scan_planned. TEST INFRASTRUCTURE."""
    f = _sig(product(), "ybg_sim_scan_planned", C.c_int,
             [C.POINTER(ScanSpec)])
    return bool(f(C.byref(spec)))


PLAN_SHAPE_PAIR, PLAN_SHAPE_PAIR_SINGLE, PLAN_SHAPE_TWO_PAIRS = 16, 17, 18


def sim_plan_shape(spec):
    """The compiled shape of the spec's column plan: the ranged-column count
    of the two-list form (0..4, 8), one of the grouped PLAN_SHAPE_* codes, or
    -1 without a plan (ybg_sim_plan_shape). TEST INFRASTRUCTURE."""
    f = _sig(product(), "ybg_sim_plan_shape", C.c_int, [C.POINTER(ScanSpec)])
    return f(C.byref(spec))


HEAD_NONE, HEAD_FOLD, HEAD_WRITE = 0, 1, 2


def sim_head_action(lane, ok, p_ok, p_wn):
    """The planned fast kernel's per-lane head-row decision (scan_device.h
    head_action) — TEST ONLY. Returns HEAD_NONE / HEAD_FOLD / HEAD_WRITE."""
    f = _sig(product(), "ybg_sim_head_action", C.c_int,
             [C.c_uint, C.c_int, C.c_int, C.c_int])
    return f(lane, int(ok), int(p_ok), int(p_wn))


def sim_plan_extract(buf, value_off, ncols, nc_cap):
    """The planned pass's column extraction over a packed row of ncols
    int64 columns whose value starts at buf[value_off] — TEST ONLY.
    buf: ctypes c_uint8 array. Returns the ncols raw u64 values."""
    f = _sig(product(), "ybg_sim_plan_extract", C.c_int,
             [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)])
    out = (C.c_uint64 * 8)()
    rc = f(C.addressof(buf) + value_off, ncols, nc_cap, out)
    if rc != 0:
        raise RuntimeError(f"ybg_sim_plan_extract failed rc={rc}")
    return list(out[:ncols])


def sim_emit(spec, data, offsets, n_blocks, row_cap=1 << 20,
             varlen_cap=1 << 24):
    """Host-simulator row emission (exact device emit path, serial) —
    TEST INFRASTRUCTURE. Returns list of rows sorted by sort_key:
    (key_datums tuple, value tuple with None for NULL / bytes for strings)."""
    lib = product()
    f = _sig(lib, "ybg_sim_emit", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
              C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
              C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_uint64,
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    nk = spec.schema.num_hash_cols + spec.schema.num_range_cols
    nc = spec.schema.num_value_cols
    sort_key = (C.c_uint64 * row_cap)()
    key_datums = (C.c_uint64 * (row_cap * max(nk, 1)))()
    datums = (C.c_uint64 * (row_cap * max(nc, 1)))()
    null_masks = (C.c_uint32 * row_cap)()
    varlen = (C.c_uint8 * varlen_cap)()
    n_rows = C.c_uint64()
    vl = C.c_uint64()
    rc = f(C.byref(spec), data, offsets, n_blocks, row_cap, sort_key,
           key_datums, datums, null_masks, varlen, varlen_cap,
           C.byref(n_rows), C.byref(vl))
    if rc != 0:
        raise RuntimeError(f"ybg_sim_emit rc={rc}")
    return decode_batch_rows(spec.schema, n_rows.value, sort_key, key_datums,
                             datums, null_masks, varlen)


def decode_batch_rows(schema, n_rows, sort_key, key_datums, datums,
                      null_masks, varlen):
    """Decode emitted rows into python tuples, sorted by sort_key."""
    nk = schema.num_hash_cols + schema.num_range_cols
    nc = schema.num_value_cols
    rows = []
    for r in range(n_rows):
        kd = []
        for c in range(nk):
            d = key_datums[r * max(nk, 1) + c]
            if schema.key_types[c] == KT_STRING:
                off = d & ((1 << 40) - 1)
                ln = d >> 40
                kd.append(bytes(varlen[off:off + ln]))
            else:
                kd.append(d)
        vals = []
        nm = null_masks[r]
        for c in range(nc):
            if (nm >> c) & 1:
                vals.append(None)
            elif schema.value_cols[c].dtype == T_STRING:
                d = datums[r * max(nc, 1) + c]
                off = d & ((1 << 40) - 1)
                ln = d >> 40
                vals.append(bytes(varlen[off:off + ln]))
            else:
                vals.append(datums[r * max(nc, 1) + c])
        rows.append((sort_key[r], tuple(kd), tuple(vals)))
    rows.sort(key=lambda t: t[0])
    return [(kd, vals) for (_, kd, vals) in rows]


def _decode_groups(schema, group_col, n, keys, vals, cnts, key_bytes,
                   num_aggs, aggs, null_index=-1):
    """Decode group arrays into {key: (vals...)}; key None for the NULL
    group, which is entry null_index (-1: none) — its keys[] value 2**64 - 1
    is also the datum of an integer -1, which stays a key; doubles decoded
    from bit patterns."""
    import struct
    out = {}
    is_str = schema.value_cols[group_col].dtype == T_STRING
    for g in range(n):
        kv = keys[g]
        if g == null_index:
            k = None
        elif is_str:
            off, ln = kv & ((1 << 40) - 1), kv >> 40
            k = bytes(key_bytes[off:off + ln])
        else:
            k = kv
        row = []
        for a in range(num_aggs):
            c = cnts[g * MAX_AGGS + a]
            v = vals[g * MAX_AGGS + a]
            if c == 0:
                row.append(None)
            elif aggs[a].op in (AGG_SUM_DOUBLE, AGG_MIN_DOUBLE,
                                AGG_MAX_DOUBLE):
                row.append(struct.unpack("<d", struct.pack("<q", v))[0])
            else:
                row.append(v)
        out[k] = tuple(row)
    return out


def sim_group(spec, data, offsets, n_blocks, cap=1 << 20,
              key_bytes_cap=1 << 24, return_restart=False, raw=False):
    """Host-simulator GROUP BY — TEST INFRASTRUCTURE. raw=True returns
    (groups, keys, n, null_index): the key array as exported and the entry
    of the NULL group (-1 without one)."""
    lib = product()
    f = _sig(lib, "ybg_sim_group_ex", C.c_int,
             [C.POINTER(ScanSpec), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
              C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
              C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_uint64,
              C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
              C.POINTER(C.c_uint32), C.POINTER(C.c_int64)])
    keys = (C.c_uint64 * cap)()
    vals = (C.c_int64 * (cap * MAX_AGGS))()
    cnts = (C.c_uint64 * (cap * MAX_AGGS))()
    kb = (C.c_uint8 * key_bytes_cap)()
    n = C.c_uint64()
    rht = (C.c_uint8 * MAX_HT)()
    rlen = C.c_uint32()
    ni = C.c_int64(-1)
    rc = f(C.byref(spec), data, offsets, n_blocks, keys, vals, cnts, kb,
           key_bytes_cap, cap, C.byref(n), rht, C.byref(rlen), C.byref(ni))
    if rc != 0:
        raise RuntimeError(f"ybg_sim_group rc={rc}")
    groups = _decode_groups(spec.schema, spec.group_col - 1, n.value, keys,
                            vals, cnts, kb, spec.num_aggs, spec.aggs,
                            ni.value)
    if raw:
        return groups, keys, n.value, ni.value
    if return_restart:
        return groups, bytes(rht[:rlen.value])
    return groups


def orcl_group(data, offsets, n_blocks, schema, spec, group_col,
               kv_format=ENC_THREE_SHARED_PARTS, cap=1 << 20,
               key_bytes_cap=1 << 24, num_aggs=None, aggs=None, raw=False):
    """Oracle GROUP BY — TEST INFRASTRUCTURE. raw=True as in sim_group.
    An oracle library built before orcl_group_scan_ex (an older oracle/
    run with these bindings) does not say which entry is the NULL group.
    The oracle exports that group last, and it exists exactly when
    COUNT(*) exceeds COUNT(group column) over the same scan, so a second
    oracle scan settles it without guessing from the key."""
    lib = oracle()
    args = [C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t),
            C.c_size_t, C.c_int, C.POINTER(OrclSchema),
            C.POINTER(OrclScanSpec), C.c_int, C.POINTER(C.c_uint64),
            C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
            C.POINTER(C.c_uint8), C.c_size_t, C.c_size_t,
            C.POINTER(C.c_size_t)]
    has_ex = hasattr(lib, "orcl_group_scan_ex")
    f = _sig(lib, "orcl_group_scan_ex", C.c_int,
             args + [C.POINTER(C.c_int64)]) if has_ex else \
        _sig(lib, "orcl_group_scan", C.c_int, args)
    base = C.cast(data, C.c_void_p).value
    blocks = (C.POINTER(C.c_uint8) * n_blocks)()
    sizes = (C.c_size_t * n_blocks)()
    for i in range(n_blocks):
        blocks[i] = C.cast(base + offsets[i], C.POINTER(C.c_uint8))
        sizes[i] = offsets[i + 1] - offsets[i]
    keys = (C.c_uint64 * cap)()
    vals = (C.c_int64 * (cap * MAX_AGGS))()
    cnts = (C.c_uint64 * (cap * MAX_AGGS))()
    kb = (C.c_uint8 * key_bytes_cap)()
    n = C.c_size_t()
    osc = schema
    ni = C.c_int64(-1)
    call = (blocks, sizes, n_blocks, kv_format, C.byref(osc), C.byref(spec),
            group_col, keys, vals, cnts, kb, key_bytes_cap, cap, C.byref(n))
    rc = f(*call, C.byref(ni)) if has_ex else f(*call)
    if rc != 0:
        raise RuntimeError(f"orcl_group_scan rc={rc}")
    if not has_ex:
        cspec = OrclScanSpec.from_buffer_copy(spec)
        cspec.num_aggs = 2
        cspec.aggs[0] = OrclAgg(AGG_COUNT_STAR, 0)
        cspec.aggs[1] = OrclAgg(AGG_COUNT, group_col)
        cres, _ = orcl_scan(data, offsets, n_blocks, schema, cspec,
                            kv_format=kv_format)
        star, col = [0 if a.is_null else a.value_i64 for a in cres.aggs[:2]]
        ni.value = n.value - 1 if star > col else -1

    class _S:
        pass

    # adapt orcl schema for the decoder
    sch = _S()
    sch.value_cols = osc.value_cols
    groups = _decode_groups(sch, group_col, n.value, keys, vals, cnts, kb,
                            spec.num_aggs, spec.aggs, ni.value)
    if raw:
        return groups, keys, n.value, ni.value
    return groups


def orcl_schema_from(schema):
    o = OrclSchema()
    o.has_hash = schema.has_hash
    o.num_hash_cols = schema.num_hash_cols
    o.num_range_cols = schema.num_range_cols
    for i in range(MAX_KEYCOLS):
        o.key_types[i] = schema.key_types[i]
    o.num_value_cols = schema.num_value_cols
    for i in range(schema.num_value_cols):
        o.value_cols[i] = OrclValueCol(schema.value_cols[i].column_id,
                                       schema.value_cols[i].dtype,
                                       schema.value_cols[i].nullable)
    return o


def orcl_read_time(read_micros, local_micros=None, global_micros=None,
                   logical=0):
    lib = oracle()
    rt = OrclReadTime()
    f = _sig(lib, "orcl_read_time_init", None,
             [C.POINTER(OrclReadTime), C.c_uint64, C.c_uint64, C.c_uint64])
    local_micros = read_micros if local_micros is None else local_micros
    global_micros = local_micros if global_micros is None else global_micros
    f(C.byref(rt), (read_micros << 12) | logical, local_micros << 12,
      global_micros << 12)
    return rt


def orcl_scan(data, offsets, n_blocks, schema, spec, kv_format=ENC_THREE_SHARED_PARTS,
              collect_rows=False, block_lo=0):
    """Run the oracle over a block array (as returned by generate()/Builder).
    `block_lo` starts the scan at a later block (contiguous sub-range; rows
    straddling the cut are attributed per-range — measurement use only).
    Returns (OrclScanResult, rows or None). TEST INFRASTRUCTURE ONLY."""
    lib = oracle()
    f = _sig(lib, "orcl_scan", C.c_int,
             [C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t),
              C.c_size_t, C.c_int, C.POINTER(OrclSchema),
              C.POINTER(OrclScanSpec), C.POINTER(OrclScanResult),
              ORCL_ROW_CB, C.c_void_p])
    base = C.cast(data, C.c_void_p).value
    blocks = (C.POINTER(C.c_uint8) * n_blocks)()
    sizes = (C.c_size_t * n_blocks)()
    for i in range(n_blocks):
        blocks[i] = C.cast(base + offsets[block_lo + i], C.POINTER(C.c_uint8))
        sizes[i] = offsets[block_lo + i + 1] - offsets[block_lo + i]
    res = OrclScanResult()
    rows = [] if collect_rows else None

    if collect_rows:
        sc = schema

        def cb(rowp, _arg):
            r = rowp.contents
            vals = []
            for i in range(sc.num_value_cols):
                if (r.null_mask >> i) & 1:
                    vals.append(None)
                elif sc.value_cols[i].dtype == T_STRING:
                    vals.append(C.string_at(r.strp[i], r.strlen_[i]))
                else:
                    vals.append(r.datums[i])
            nk = sc.num_hash_cols + sc.num_range_cols
            kd = []
            for i in range(nk):
                if sc.key_types[i] == KT_STRING:
                    kd.append(C.string_at(r.key_str[i], r.key_str_len[i]))
                else:
                    kd.append(r.key_datums[i])
            rows.append((tuple(kd), tuple(vals)))
            return 0

        cbf = ORCL_ROW_CB(cb)
    else:
        cbf = C.cast(None, ORCL_ROW_CB)
    rc = f(blocks, sizes, n_blocks, kv_format, C.byref(schema), C.byref(spec),
           C.byref(res), cbf, None)
    if rc != 0:
        raise RuntimeError(f"orcl_scan failed rc={rc}")
    return res, rows


def snappy_compress(data):
    """Host snappy compressor (generator codec; tests)."""
    lib = product()
    f = _sig(lib, "ybg_snappy_compress", C.c_int64,
             [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64])
    src = (C.c_uint8 * len(data)).from_buffer_copy(data)
    cap = len(data) * 2 + 64
    dst = (C.c_uint8 * cap)()
    n = f(src, len(data), dst, cap)
    assert n > 0
    return bytes(dst[:n])


_GUARD = 64


def _uncompress_guarded(f, data, cap, guard):
    """Call a host decompressor with capacity cap. With guard, the
    destination is followed by 64 bytes of 0xA5 that must come back
    unchanged: a decoder that writes past its capacity trips the assert."""
    src = (C.c_uint8 * len(data)).from_buffer_copy(data)
    dst = (C.c_uint8 * (cap + (_GUARD if guard else 0)))()
    if guard:
        C.memset(C.byref(dst, cap), 0xA5, _GUARD)
    n = f(src, len(data), dst, cap)
    if guard:
        assert bytes(dst[cap:]) == b"\xa5" * _GUARD, \
            "decompressor wrote past its capacity"
    return n, dst


def snappy_uncompress(data, cap, guard=False):
    """Host snappy decompressor (same code the GPU kernel runs)."""
    lib = product()
    f = _sig(lib, "ybg_snappy_uncompress", C.c_int64,
             [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64])
    n, dst = _uncompress_guarded(f, data, cap, guard)
    if n < 0:
        raise RuntimeError("snappy_uncompress failed")
    return bytes(dst[:n])


class TxnStatus(C.Structure):
    """ybg_txn_status_t / orcl_txn_status_t (same layout)."""
    _fields_ = [("txn_id", C.c_uint32), ("status", C.c_int32),
                ("commit_ht", C.c_uint64)]


TXN_PENDING, TXN_COMMITTED, TXN_ABORTED = 0, 1, 2


def make_txns(table):
    """table: dict txn_id -> ("committed", commit_ht_micros, logical?) |
    "pending" | "aborted". Returns a ctypes TxnStatus array."""
    arr = (TxnStatus * max(len(table), 1))()
    for i, (tid, st) in enumerate(sorted(table.items())):
        arr[i].txn_id = tid
        if st == "pending":
            arr[i].status = TXN_PENDING
        elif st == "aborted":
            arr[i].status = TXN_ABORTED
        else:
            arr[i].status = TXN_COMMITTED
            ht = st[1] if isinstance(st, tuple) else st
            arr[i].commit_ht = ht << 12
    return arr, len(table)


class Intents:
    """Intent-stream builder (provisional records of in-flight
    transactions; post-DecodeStrongWriteIntent form — see
    include/yb_gpu_scan.h)."""

    def __init__(self, schema):
        lib = product()
        self._lib = lib
        self._schema = schema
        create = _sig(lib, "ybg_intents_create", C.c_void_p,
                      [C.POINTER(Schema)])
        self._h = create(C.byref(schema))
        self._add_packed = _sig(lib, "ybg_intents_add_packed_row", C.c_int,
                                [C.c_void_p, C.POINTER(Key), C.c_uint64,
                                 C.c_uint32, C.c_uint32, C.c_int,
                                 C.POINTER(RowVals)])
        self._add_col = _sig(lib, "ybg_intents_add_column_update", C.c_int,
                             [C.c_void_p, C.POINTER(Key), C.c_int,
                              C.c_uint64, C.c_uint32, C.c_uint32,
                              C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64,
                              C.c_int])
        self._add_tomb = _sig(lib, "ybg_intents_add_row_tombstone", C.c_int,
                              [C.c_void_p, C.POINTER(Key), C.c_uint64,
                               C.c_uint32, C.c_uint32])
        self._data = _sig(lib, "ybg_intents_data", C.c_int,
                          [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)),
                           C.POINTER(C.c_uint64)])
        self._keepalive = []

    def _key(self, hash_=0, datums=(), strs=()):
        k = Key()
        k.hash = hash_
        for i, d in enumerate(datums):
            k.datums[i] = d & 0xFFFFFFFFFFFFFFFF
        for i, s in enumerate(strs):
            if s is not None:
                buf = C.create_string_buffer(s, len(s))
                self._keepalive.append(buf)
                k.strs[i] = C.cast(buf, C.POINTER(C.c_uint8))
                k.str_lens[i] = len(s)
        return k

    def add_packed_row(self, write_ht_micros, txn_id, values, hash_=0,
                       key_datums=(), key_strs=(), write_id=0,
                       packed_version=2, logical=0):
        import struct
        k = self._key(hash_, key_datums, key_strs)
        v = RowVals()
        for i, (dt, val) in enumerate(values):
            if val is None:
                v.null[i] = 1
            elif dt == T_DOUBLE:
                v.datums[i] = struct.unpack("<Q", struct.pack("<d", val))[0]
            elif dt == T_FLOAT:
                v.datums[i] = struct.unpack("<I", struct.pack("<f", val))[0]
            elif dt == T_STRING:
                buf = C.create_string_buffer(val, len(val))
                self._keepalive.append(buf)
                v.strs[i] = C.cast(buf, C.POINTER(C.c_uint8))
                v.str_lens[i] = len(val)
            else:
                v.datums[i] = val & 0xFFFFFFFFFFFFFFFF
        rc = self._add_packed(self._h, C.byref(k),
                              (write_ht_micros << 12) | logical, write_id,
                              txn_id, packed_version, C.byref(v))
        assert rc == 0

    def add_column_update(self, write_ht_micros, txn_id, col_idx, value,
                          hash_=0, key_datums=(), key_strs=(), write_id=0,
                          null=False, logical=0):
        import struct
        k = self._key(hash_, key_datums, key_strs)
        datum = 0
        sp = None
        slen = 0
        dt = self._schema.value_cols[col_idx].dtype
        if value is None:
            null = True
        elif dt == T_DOUBLE:
            datum = struct.unpack("<Q", struct.pack("<d", value))[0]
        elif dt == T_STRING:
            buf = C.create_string_buffer(value, len(value))
            self._keepalive.append(buf)
            sp = C.cast(buf, C.POINTER(C.c_uint8))
            slen = len(value)
        else:
            datum = value & 0xFFFFFFFFFFFFFFFF
        rc = self._add_col(self._h, C.byref(k), col_idx,
                           (write_ht_micros << 12) | logical, write_id,
                           txn_id, datum, sp, slen, 1 if null else 0)
        assert rc == 0

    def add_row_tombstone(self, write_ht_micros, txn_id, hash_=0,
                          key_datums=(), key_strs=(), write_id=0,
                          logical=0):
        k = self._key(hash_, key_datums, key_strs)
        rc = self._add_tomb(self._h, C.byref(k),
                            (write_ht_micros << 12) | logical, write_id,
                            txn_id)
        assert rc == 0

    def blob(self):
        p = C.POINTER(C.c_uint8)()
        n = C.c_uint64()
        rc = self._data(self._h, C.byref(p), C.byref(n))
        assert rc == 0
        return p, n.value


def merge_intents(data, offsets, n_blocks, intents_blob, blob_len, txns,
                  n_txns, kv_format=ENC_THREE_SHARED_PARTS):
    """Product-side feed-time resolve+merge (ybg_merge_intents). Returns
    (merged_data, merged_offsets, n_blocks, total) as ctypes buffers the
    caller can pass to feed/sim APIs (freed at process exit)."""
    lib = product()
    f = _sig(lib, "ybg_merge_intents", C.c_int,
             [C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.c_uint64,
              C.c_int, C.POINTER(C.c_uint8), C.c_uint64,
              C.POINTER(TxnStatus), C.c_uint32,
              C.POINTER(C.POINTER(C.c_uint8)),
              C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64),
              C.POINTER(C.c_uint64)])
    ob = C.POINTER(C.c_uint8)()
    oo = C.POINTER(C.c_uint64)()
    on = C.c_uint64()
    ot = C.c_uint64()
    rc = f(data, offsets, n_blocks, kv_format, intents_blob, blob_len, txns,
           n_txns, C.byref(ob), C.byref(oo), C.byref(on), C.byref(ot))
    if rc != 0:
        raise RuntimeError(f"ybg_merge_intents rc={rc}")
    return ob, oo, on.value, ot.value


def orcl_scan_intents(data, offsets, n_blocks, schema, spec, intents_blob,
                      blob_len, txns, n_txns,
                      kv_format=ENC_THREE_SHARED_PARTS):
    """Oracle runtime two-stream merge scan — TEST INFRASTRUCTURE."""
    lib = oracle()
    f = _sig(lib, "orcl_scan_intents", C.c_int,
             [C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t),
              C.c_size_t, C.c_int, C.POINTER(OrclSchema),
              C.POINTER(OrclScanSpec), C.POINTER(C.c_uint8), C.c_size_t,
              C.POINTER(TxnStatus), C.c_uint32,
              C.POINTER(OrclScanResult), ORCL_ROW_CB, C.c_void_p])
    base = C.cast(data, C.c_void_p).value
    blocks = (C.POINTER(C.c_uint8) * n_blocks)()
    sizes = (C.c_size_t * n_blocks)()
    for i in range(n_blocks):
        blocks[i] = C.cast(base + offsets[i], C.POINTER(C.c_uint8))
        sizes[i] = offsets[i + 1] - offsets[i]
    res = OrclScanResult()
    rc = f(blocks, sizes, n_blocks, kv_format, C.byref(schema),
           C.byref(spec), intents_blob, blob_len, txns, n_txns,
           C.byref(res), C.cast(None, ORCL_ROW_CB), None)
    if rc != 0:
        raise RuntimeError(f"orcl_scan_intents rc={rc}")
    return res


def encode_dockey(schema, hash_=0, key_datums=(), key_strs=()):
    """Encode a DocKey from key-column datums (ybg_encode_dockey) —
    bounds / paging-state construction helper."""
    lib = product()
    f = _sig(lib, "ybg_encode_dockey", C.c_size_t,
             [C.POINTER(Schema), C.POINTER(Key), C.POINTER(C.c_uint8),
              C.c_size_t])
    k = Key()
    k.hash = hash_
    keep = []
    for i, d in enumerate(key_datums):
        k.datums[i] = d & 0xFFFFFFFFFFFFFFFF
    for i, s in enumerate(key_strs):
        if s is not None:
            buf = C.create_string_buffer(s, len(s))
            keep.append(buf)
            k.strs[i] = C.cast(buf, C.POINTER(C.c_uint8))
            k.str_lens[i] = len(s)
    out = (C.c_uint8 * 512)()
    n = f(C.byref(schema), C.byref(k), out, 512)
    assert n > 0
    return bytes(out[:n])


def lz4_compress(data):
    """Host lz4 compressor (generator codec; tests)."""
    lib = product()
    f = _sig(lib, "ybg_lz4_compress", C.c_int64,
             [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64])
    src = (C.c_uint8 * len(data)).from_buffer_copy(data)
    cap = len(data) * 2 + 64
    dst = (C.c_uint8 * cap)()
    n = f(src, len(data), dst, cap)
    assert n > 0
    return bytes(dst[:n])



def lz4_uncompress(data, cap, guard=False):
    """Host lz4 decompressor (same code the GPU kernel runs)."""
    lib = product()
    f = _sig(lib, "ybg_lz4_uncompress", C.c_int64,
             [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64])
    n, dst = _uncompress_guarded(f, data, cap, guard)
    if n < 0:
        raise RuntimeError("lz4_uncompress failed")
    return bytes(dst[:n])




# ---- SST bloom filter (docdb_filter_policy / rocksdb FixedSizeFilter) ----

def filter_slice_size():
    lib = product()
    return _sig(lib, "ybg_filter_slice_size", C.c_uint64, [])()


def filter_from_sst(data, offsets, n_blocks, kv_format=1):
    """Build the tablet's bloom filter (concatenated fixed-size slices)."""
    lib = product()
    f = _sig(lib, "ybg_filter_from_sst", C.c_int,
             [C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.c_uint64,
              C.c_int, C.POINTER(C.c_uint8), C.c_uint64,
              C.POINTER(C.c_uint64)])
    cap = filter_slice_size() * (2 + n_blocks)
    out = (C.c_uint8 * cap)()
    out_len = C.c_uint64(0)
    rc = f(data, offsets, n_blocks, kv_format, out, cap, C.byref(out_len))
    if rc:
        raise RuntimeError(f"ybg_filter_from_sst rc={rc}")
    return bytes(out[:out_len.value])


def filter_may_match(filt, key):
    lib = product()
    f = _sig(lib, "ybg_filter_may_match", C.c_int,
             [C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint8),
              C.c_uint64])
    fb = (C.c_uint8 * len(filt)).from_buffer_copy(filt)
    kb = (C.c_uint8 * len(key)).from_buffer_copy(key)
    return f(fb, len(filt), kb, len(key))


def filter_key_prefix_len(key):
    lib = product()
    f = _sig(lib, "ybg_filter_key_prefix_len", C.c_uint64,
             [C.POINTER(C.c_uint8), C.c_uint64])
    kb = (C.c_uint8 * len(key)).from_buffer_copy(key)
    return f(kb, len(key))
