"""GpuScan — thin Python wrapper over the product C ABI
(include/yb_gpu_scan.h). This is the PRODUCT path: it requires an MI355X
(gfx950) and fails loudly when no HIP device or extension is present — there
is no CPU fallback."""
import ctypes as C

import ybgpu as y


class GpuScanError(RuntimeError):
    pass


def _lib():
    lib = y.product()
    f = lib.yb_gpu_scan_open
    f.restype = C.c_int
    f.argtypes = [C.POINTER(y.ScanSpec), C.POINTER(C.c_void_p)]
    lib.yb_gpu_scan_feed_blocks.restype = C.c_int
    lib.yb_gpu_scan_feed_blocks.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.c_uint64,
        C.c_int]
    lib.yb_gpu_scan_execute.restype = C.c_int
    lib.yb_gpu_scan_execute.argtypes = [C.c_void_p]
    lib.yb_gpu_scan_wait.restype = C.c_int
    lib.yb_gpu_scan_wait.argtypes = [C.c_void_p]
    lib.yb_gpu_scan_aggregate.restype = C.c_int
    lib.yb_gpu_scan_aggregate.argtypes = [C.c_void_p,
                                          C.POINTER(y.ScanResult)]
    lib.yb_gpu_scan_next_batch.restype = C.c_int
    lib.yb_gpu_scan_next_batch.argtypes = [C.c_void_p,
                                           C.POINTER(y.RowBatch)]
    lib.yb_host_iter_open.restype = C.c_void_p
    lib.yb_host_iter_open.argtypes = [C.POINTER(y.ScanSpec),
                                      C.POINTER(C.c_uint8),
                                      C.POINTER(C.c_uint64), C.c_uint64]
    lib.yb_host_iter_next.restype = C.c_int
    lib.yb_host_iter_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint32),
                                      C.POINTER(C.POINTER(C.c_uint8))]
    lib.yb_host_iter_close.restype = None
    lib.yb_host_iter_close.argtypes = [C.c_void_p]
    lib.yb_gpu_scan_group_aggregate.restype = C.c_int
    lib.yb_gpu_scan_group_aggregate.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_uint64, C.c_uint64,
        C.POINTER(C.c_uint64)]
    if hasattr(lib, "yb_gpu_scan_group_null_index"):  # as retry_batches below
        lib.yb_gpu_scan_group_null_index.restype = C.c_int
        lib.yb_gpu_scan_group_null_index.argtypes = [C.c_void_p,
                                                     C.POINTER(C.c_int64)]
    lib.yb_gpu_scan_restart_data.restype = C.c_int
    lib.yb_gpu_scan_restart_data.argtypes = [
        C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    lib.yb_gpu_scan_kernel_ms.restype = C.c_int
    lib.yb_gpu_scan_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]
    lib.yb_gpu_scan_close.restype = C.c_int
    lib.yb_gpu_scan_close.argtypes = [C.c_void_p]
    lib.yb_gpu_scan_staged.restype = C.c_int
    lib.yb_gpu_scan_staged.argtypes = [C.c_void_p]
    # absent from a library built before the column plan (YBG_SO may load
    # one for a before/after measurement)
    if hasattr(lib, "yb_gpu_scan_planned"):
        lib.yb_gpu_scan_planned.restype = C.c_int
        lib.yb_gpu_scan_planned.argtypes = [C.c_void_p]
    if hasattr(lib, "yb_gpu_scan_retry_batches"):  # same: newer than the plan
        lib.yb_gpu_scan_retry_batches.restype = C.c_int
        lib.yb_gpu_scan_retry_batches.argtypes = [C.c_void_p,
                                                  C.POINTER(C.c_uint64)]
    lib.yb_gpu_snapshot_build.restype = C.c_int
    lib.yb_gpu_snapshot_build.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.yb_gpu_snapshot_info.restype = C.c_int
    lib.yb_gpu_snapshot_info.argtypes = [C.c_void_p,
                                         C.POINTER(y.SnapshotInfo)]
    lib.yb_gpu_snapshot_query.restype = C.c_int
    lib.yb_gpu_snapshot_query.argtypes = [C.c_void_p,
                                          C.POINTER(y.SnapshotQuery),
                                          C.POINTER(y.ScanResult)]
    lib.yb_gpu_snapshot_group_query.restype = C.c_int
    lib.yb_gpu_snapshot_group_query.argtypes = [
        C.c_void_p, C.POINTER(y.SnapshotGroupQuery), C.POINTER(C.c_uint64),
        C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_uint64,
        C.POINTER(y.SnapshotGroupResult)]
    lib.yb_gpu_snapshot_select.restype = C.c_int
    lib.yb_gpu_snapshot_select.argtypes = [
        C.c_void_p, C.POINTER(y.SnapshotSelect), C.POINTER(C.c_uint64),
        C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64,
        C.POINTER(y.SnapshotSelectResult)]
    if hasattr(lib, "yb_gpu_snapshot_build_ex"):  # newer than the select
        lib.yb_gpu_snapshot_build_ex.restype = C.c_int
        lib.yb_gpu_snapshot_build_ex.argtypes = [
            C.c_void_p, C.POINTER(y.SnapshotBuildOpts),
            C.POINTER(C.c_void_p)]
        lib.yb_gpu_snapshot_string_info.restype = C.c_int
        lib.yb_gpu_snapshot_string_info.argtypes = [
            C.c_void_p, C.POINTER(y.SnapshotStringInfo)]
        lib.yb_gpu_snapshot_select_var.restype = C.c_int
        lib.yb_gpu_snapshot_select_var.argtypes = [
            C.c_void_p, C.POINTER(y.SnapshotSelect), C.POINTER(C.c_uint64),
            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64,
            C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64),
            C.POINTER(y.SnapshotSelectResult)]
    if hasattr(lib, "yb_gpu_snapshot_select_ordered"):  # newer than strings
        lib.yb_gpu_snapshot_select_ordered.restype = C.c_int
        lib.yb_gpu_snapshot_select_ordered.argtypes = [
            C.c_void_p, C.POINTER(y.SnapshotOrder), C.POINTER(C.c_uint64),
            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64,
            C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint64),
            C.POINTER(y.SnapshotOrderResult)]
    lib.yb_gpu_snapshot_kernel_ms.restype = C.c_int
    lib.yb_gpu_snapshot_kernel_ms.argtypes = [C.c_void_p,
                                              C.POINTER(C.c_double)]
    lib.yb_gpu_snapshot_close.restype = C.c_int
    lib.yb_gpu_snapshot_close.argtypes = [C.c_void_p]
    lib.yb_gpu_last_error.restype = C.c_char_p
    lib.yb_gpu_available.restype = C.c_int
    return lib


def gpu_available():
    return bool(_lib().yb_gpu_available())


class GpuScan:
    def __init__(self, spec):
        self._lib = _lib()
        self._h = C.c_void_p()
        self._spec = spec  # keep alive (aux pointers)
        rc = self._lib.yb_gpu_scan_open(C.byref(spec), C.byref(self._h))
        if rc:
            raise GpuScanError(
                f"yb_gpu_scan_open rc={rc}: "
                f"{self._lib.yb_gpu_last_error().decode()}")

    def _check(self, rc, what):
        if rc:
            raise GpuScanError(
                f"{what} rc={rc}: {self._lib.yb_gpu_last_error().decode()}")

    def feed_blocks_host(self, data, offsets, n_blocks, total_bytes):
        del total_bytes
        self._check(
            self._lib.yb_gpu_scan_feed_blocks(self._h, data, offsets,
                                              n_blocks, 0),
            "feed_blocks")

    def feed_blocks_intents(self, data, offsets, n_blocks, intents_blob,
                            blob_len, txns, n_txns):
        """Feed regular blocks + an intent stream (resolve + merge + feed;
        yb_gpu_scan_feed_blocks_intents)."""
        f = self._lib.yb_gpu_scan_feed_blocks_intents
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint8),
                      C.POINTER(C.c_uint64), C.c_uint64,
                      C.POINTER(C.c_uint8), C.c_uint64,
                      C.POINTER(y.TxnStatus), C.c_uint32]
        self._check(f(self._h, data, offsets, n_blocks, intents_blob,
                      blob_len, txns, n_txns), "feed_blocks_intents")

    def feed_blocks_bloom(self, data, offsets, n_blocks, filt):
        """feed_blocks + bloom consultation: a point scan whose pinned key
        prefix the filter proves absent feeds nothing and reports empty
        (yb_gpu_scan_feed_blocks_bloom)."""
        f = self._lib.yb_gpu_scan_feed_blocks_bloom
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint8),
                      C.POINTER(C.c_uint64), C.c_uint64, C.c_int,
                      C.POINTER(C.c_uint8), C.c_uint64]
        fb = (C.c_uint8 * len(filt)).from_buffer_copy(filt) if filt else None
        self._check(f(self._h, data, offsets, n_blocks, 0, fb,
                      len(filt) if filt else 0), "feed_blocks_bloom")

    def feed_sst(self, file_ptr, size, verify=True):
        """Feed a complete BlockBasedTable SST file (footer + index block
        parsed host-side; block checksums verified when verify)."""
        import ctypes as C
        f = self._lib.yb_gpu_scan_feed_sst
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.c_int]
        self._check(f(self._h, file_ptr, size, 1 if verify else 0),
                    "feed_sst")

    def execute(self):
        self._check(self._lib.yb_gpu_scan_execute(self._h), "execute")

    def wait(self):
        self._check(self._lib.yb_gpu_scan_wait(self._h), "wait")

    def aggregates(self):
        res = y.ScanResult()
        self._check(self._lib.yb_gpu_scan_aggregate(self._h, C.byref(res)),
                    "aggregate")
        return res

    def batch_rows(self):
        """Materialize matching rows (next_batch) and decode into python
        tuples sorted by sort_key."""
        b = y.RowBatch()
        self._check(self._lib.yb_gpu_scan_next_batch(self._h, C.byref(b)),
                    "next_batch")
        return y.decode_batch_rows(self._spec.schema, b.n_rows, b.sort_key,
                                   b.key_datums, b.datums, b.null_masks,
                                   b.varlen)

    def group_aggregate_raw(self, cap=1 << 20, key_bytes_cap=1 << 24):
        """GROUP BY partial aggregates: raw ctypes arrays
        (keys, vals, cnts, key_bytes, n_groups). Output buffers are
        allocated once and reused (zeroed ctypes allocation of the full
        capacity measured ~30 ms/step); only the first n_groups entries
        are written by the call."""
        gb = getattr(self, "_group_bufs", None)
        if gb is None or gb[0] != cap or gb[1] != key_bytes_cap:
            gb = (cap, key_bytes_cap,
                  (C.c_uint64 * cap)(),
                  (C.c_int64 * (cap * y.MAX_AGGS))(),
                  (C.c_uint64 * (cap * y.MAX_AGGS))(),
                  (C.c_uint8 * key_bytes_cap)())
            self._group_bufs = gb
        keys, vals, cnts, kb = gb[2], gb[3], gb[4], gb[5]
        n = C.c_uint64()
        self._check(
            self._lib.yb_gpu_scan_group_aggregate(
                self._h, keys, vals, cnts, kb, key_bytes_cap, cap,
                C.byref(n)), "group_aggregate")
        return keys, vals, cnts, kb, n.value

    def group_null_index(self):
        """The entry of the last group_aggregate's output that is the
        NULL-key group, -1 when there is none. Its keys[] value 2**64 - 1 is
        also the datum of an integer -1 (yb_gpu_scan_group_null_index)."""
        i = C.c_int64()
        self._check(
            self._lib.yb_gpu_scan_group_null_index(self._h, C.byref(i)),
            "group_null_index")
        return i.value

    def group_aggregate(self, cap=1 << 20, key_bytes_cap=1 << 24):
        """GROUP BY partial aggregates (spec.group_col must be set):
        {key: (aggs...)}, None keying the NULL group."""
        keys, vals, cnts, kb, n = self.group_aggregate_raw(cap, key_bytes_cap)
        return y._decode_groups(self._spec.schema, self._spec.group_col - 1,
                                n, keys, vals, cnts, kb,
                                self._spec.num_aggs, self._spec.aggs,
                                self.group_null_index())

    def restart_data(self):
        """Read-restart data of the last execute/group_aggregate
        (GetReadRestartData analog): encoded DocHybridTime bytes, b'' when
        no restart is needed."""
        ht = (C.c_uint8 * y.MAX_HT)()
        ln = C.c_uint32()
        self._check(
            self._lib.yb_gpu_scan_restart_data(self._h, ht, C.byref(ln)),
            "restart_data")
        return bytes(ht[:ln.value])

    def kernel_ms(self):
        total = C.c_double()
        decode = C.c_double()
        self._check(
            self._lib.yb_gpu_scan_kernel_ms(self._h, C.byref(total),
                                            C.byref(decode)), "kernel_ms")
        return total.value, decode.value

    def staged(self):
        """True when the last execute was answered from a columnar snapshot
        (YBG_STAGE=1 transparent mode)."""
        return bool(self._lib.yb_gpu_scan_staged(self._h))

    def planned(self):
        """True when the last execute launched the planned fast kernel (the
        query compiled into a column plan; YBG_PLAN=0 turns it off)."""
        return bool(self._lib.yb_gpu_scan_planned(self._h))

    def retry_batches(self):
        """Batches the last execute handed from the fast kernel to the
        general kernel (0 when no fast kernel ran). Waits for the execute."""
        n = C.c_uint64()
        self._check(
            self._lib.yb_gpu_scan_retry_batches(self._h, C.byref(n)),
            "retry_batches")
        return n.value

    def snapshot(self, strings=False):
        """Build a columnar snapshot of the fed tablet at this handle's read
        time and bounds (yb_gpu_snapshot_build). The snapshot owns its
        memory: it stays valid after this handle is closed. strings=True
        stages the string value and key columns too
        (yb_gpu_snapshot_build_ex with stage_strings)."""
        h = C.c_void_p()
        if strings:
            opts = y.SnapshotBuildOpts()
            opts.stage_strings = 1
            self._check(self._lib.yb_gpu_snapshot_build_ex(
                self._h, C.byref(opts), C.byref(h)), "snapshot_build_ex")
        else:
            self._check(self._lib.yb_gpu_snapshot_build(self._h, C.byref(h)),
                        "snapshot_build")
        return GpuSnapshot(self._lib, h, self._spec.schema)

    def close(self):
        if self._h:
            self._lib.yb_gpu_scan_close(self._h)
            self._h = None


class GpuSnapshot:
    """Columnar snapshot: the rows visible at one read time as dense
    device-resident column arrays, answering numeric predicate/aggregate
    queries, GROUP BY and ordered row fetches with the streaming kernels;
    built with strings=True also string predicates and string fetches."""

    def __init__(self, lib, handle, schema=None):
        self._lib = lib
        self._h = handle
        self._schema = schema  # tells select() which columns are strings

    def _check(self, rc, what):
        if rc:
            err = GpuScanError(
                f"{what} rc={rc}: {self._lib.yb_gpu_last_error().decode()}")
            err.code = rc
            raise err

    def info(self):
        out = y.SnapshotInfo()
        self._check(self._lib.yb_gpu_snapshot_info(self._h, C.byref(out)),
                    "snapshot_info")
        return out

    def string_info(self):
        """Which string columns are staged and their heap bytes
        (yb_gpu_snapshot_string_info); all zero without strings=True."""
        out = y.SnapshotStringInfo()
        self._check(
            self._lib.yb_gpu_snapshot_string_info(self._h, C.byref(out)),
            "snapshot_string_info")
        return out

    def query(self, preds, aggs):
        """Run one query; returns a ScanResult. Unsupported queries raise
        GpuScanError with .code == 9 (nothing is launched)."""
        q = y.snapshot_query(preds, aggs)
        res = y.ScanResult()
        self._check(
            self._lib.yb_gpu_snapshot_query(self._h, C.byref(q),
                                            C.byref(res)), "snapshot_query")
        return res

    def group_query_raw(self, preds, aggs, group_col, group_is_key=False,
                        expect_groups=0, cap=1 << 20):
        """GROUP BY on the snapshot (yb_gpu_snapshot_group_query): raw
        ctypes arrays (keys, vals, cnts) plus the SnapshotGroupResult. The
        first result.n_groups entries are written: ascending by key as an
        unsigned 64-bit pattern, the NULL group (result.has_null_group)
        last. Output buffers are allocated once per capacity and reused,
        like GpuScan.group_aggregate_raw's. Errors raise GpuScanError with
        .code (9 unsupported query, 8 cap too small) and .result."""
        gb = getattr(self, "_group_bufs", None)
        if gb is None or gb[0] != cap:
            n = max(cap, 1)
            gb = (cap, (C.c_uint64 * n)(), (C.c_int64 * (n * y.MAX_AGGS))(),
                  (C.c_uint64 * (n * y.MAX_AGGS))())
            self._group_bufs = gb
        keys, vals, cnts = gb[1], gb[2], gb[3]
        q = y.snapshot_group_query(preds, aggs, group_col, group_is_key,
                                   expect_groups)
        res = y.SnapshotGroupResult()
        rc = self._lib.yb_gpu_snapshot_group_query(
            self._h, C.byref(q), keys, vals, cnts, cap, C.byref(res))
        if rc:
            err = GpuScanError(
                f"snapshot_group_query rc={rc}: "
                f"{self._lib.yb_gpu_last_error().decode()}")
            err.code = rc
            err.result = res
            raise err
        return keys, vals, cnts, res

    def group_query(self, preds, aggs, group_col, group_is_key=False,
                    expect_groups=0, cap=1 << 20):
        """GROUP BY on the snapshot: {key: (aggs...)} in the shape of
        GpuScan.group_aggregate, None keying the NULL group. expect_groups
        is a hint (0 = unknown) that picks the kernel level, never the
        result."""
        keys, vals, cnts, res = self.group_query_raw(
            preds, aggs, group_col, group_is_key, expect_groups, cap)
        return y.decode_snapshot_groups(res, keys, vals, cnts, list(aggs))

    def select_raw(self, preds, cols, limit=0, backward=False, row_lo=0,
                   row_hi=None, cap=1 << 16):
        """Row fetch on the snapshot (yb_gpu_snapshot_select): raw ctypes
        arrays (datums, null_masks, row_ids) plus the SnapshotSelectResult.
        The first result.n_rows rows are written, ascending by snapshot
        position (descending with backward); projected column j of row i is
        datums[j * cap + i]. Output buffers are allocated once per
        (capacity, column count) and reused, like group_query_raw's. Errors
        raise GpuScanError with .code (9 unsupported query, 8 cap too small)
        and .result."""
        ncols = max(1, min(len(cols), y.MAX_SELECT_COLS))
        sb = getattr(self, "_select_bufs", None)
        if sb is None or sb[0] != (cap, ncols):
            n = max(cap, 1)
            sb = ((cap, ncols), (C.c_uint64 * (n * ncols))(),
                  (C.c_uint32 * n)(), (C.c_uint64 * n)())
            self._select_bufs = sb
        datums, null_masks, row_ids = sb[1], sb[2], sb[3]
        q = y.snapshot_select(preds, cols, limit, backward, row_lo, row_hi)
        res = y.SnapshotSelectResult()
        rc = self._lib.yb_gpu_snapshot_select(
            self._h, C.byref(q), datums, null_masks, row_ids, cap,
            C.byref(res))
        if rc:
            err = GpuScanError(
                f"snapshot_select rc={rc}: "
                f"{self._lib.yb_gpu_last_error().decode()}")
            err.code = rc
            err.result = res
            raise err
        return datums, null_masks, row_ids, res

    def select_var_raw(self, preds, cols, limit=0, backward=False, row_lo=0,
                       row_hi=None, cap=1 << 16, varlen_cap=1 << 20):
        """Row fetch with string projection (yb_gpu_snapshot_select_var):
        select_raw's arrays plus the varlen heap and its size — (datums,
        null_masks, row_ids, varlen, varlen_size, result). A projected
        string column's datum is (len << 40) | offset into varlen, 0 for a
        NULL. Errors raise GpuScanError with .code (8: cap or varlen_cap too
        small), .result and .varlen_size (the heap size needed)."""
        ncols = max(1, min(len(cols), y.MAX_SELECT_COLS))
        sb = getattr(self, "_select_var_bufs", None)
        if sb is None or sb[0] != (cap, ncols, varlen_cap):
            n = max(cap, 1)
            sb = ((cap, ncols, varlen_cap), (C.c_uint64 * (n * ncols))(),
                  (C.c_uint32 * n)(), (C.c_uint64 * n)(),
                  (C.c_uint8 * max(varlen_cap, 1))())
            self._select_var_bufs = sb
        datums, null_masks, row_ids, varlen = sb[1], sb[2], sb[3], sb[4]
        q = y.snapshot_select(preds, cols, limit, backward, row_lo, row_hi)
        res = y.SnapshotSelectResult()
        vsize = C.c_uint64()
        rc = self._lib.yb_gpu_snapshot_select_var(
            self._h, C.byref(q), datums, null_masks, row_ids, cap, varlen,
            varlen_cap, C.byref(vsize), C.byref(res))
        if rc:
            err = GpuScanError(
                f"snapshot_select_var rc={rc}: "
                f"{self._lib.yb_gpu_last_error().decode()}")
            err.code = rc
            err.result = res
            err.varlen_size = vsize.value
            raise err
        return datums, null_masks, row_ids, varlen, vsize.value, res

    def select(self, preds, cols, limit=0, backward=False, row_lo=0,
               row_hi=None, cap=1 << 16, varlen_cap=1 << 20):
        """SELECT cols WHERE preds on the snapshot, in key order: returns
        (rows, result) with rows = [(projected values..., None for NULL)].
        cols: (is_key_col, col) pairs. Page with limit and
        result.resume_row (the next row_lo, or row_hi when backward) until
        result.done. A projected string column (snapshot built with
        strings=True) goes through select_var and comes back as bytes."""
        strs = None
        if self._schema is not None and len(cols) <= y.MAX_SELECT_COLS:
            try:
                strs = y.select_string_cols(self._schema, cols)
            except IndexError:  # out of range: the ABI names the offender
                strs = None
        if strs and any(strs):
            datums, null_masks, _ids, varlen, _vs, res = self.select_var_raw(
                preds, cols, limit, backward, row_lo, row_hi, cap, varlen_cap)
            return y.decode_snapshot_rows(res, datums, null_masks, len(cols),
                                          cols, cap, varlen, strs), res
        datums, null_masks, _ids, res = self.select_raw(
            preds, cols, limit, backward, row_lo, row_hi, cap)
        return y.decode_snapshot_rows(res, datums, null_masks,
                                      len(cols), cols, cap), res

    def select_ordered_raw(self, preds, cols, order_by, descending=False,
                           nulls_first=False, limit=0, after=None, row_lo=0,
                           row_hi=None, cap=1 << 16, varlen_cap=1 << 20,
                           backward=False):
        """ORDER BY / top-N on the snapshot
        (yb_gpu_snapshot_select_ordered): select_var_raw's arrays —
        (datums, null_masks, row_ids, varlen, varlen_size, result) with a
        SnapshotOrderResult. order_by: (is_key_col, col); after: a previous
        result's cursor (y.order_cursor). Errors raise GpuScanError with
        .code, .result and .varlen_size."""
        ncols = max(1, min(len(cols), y.MAX_SELECT_COLS))
        sb = getattr(self, "_order_bufs", None)
        if sb is None or sb[0] != (cap, ncols, varlen_cap):
            n = max(cap, 1)
            sb = ((cap, ncols, varlen_cap), (C.c_uint64 * (n * ncols))(),
                  (C.c_uint32 * n)(), (C.c_uint64 * n)(),
                  (C.c_uint8 * max(varlen_cap, 1))())
            self._order_bufs = sb
        datums, null_masks, row_ids, varlen = sb[1], sb[2], sb[3], sb[4]
        q = y.snapshot_order(preds, cols, order_by, descending, nulls_first,
                             limit, after, row_lo, row_hi, backward)
        res = y.SnapshotOrderResult()
        vsize = C.c_uint64()
        rc = self._lib.yb_gpu_snapshot_select_ordered(
            self._h, C.byref(q), datums, null_masks, row_ids, cap, varlen,
            varlen_cap, C.byref(vsize), C.byref(res))
        if rc:
            err = GpuScanError(
                f"snapshot_select_ordered rc={rc}: "
                f"{self._lib.yb_gpu_last_error().decode()}")
            err.code = rc
            err.result = res
            err.varlen_size = vsize.value
            raise err
        return datums, null_masks, row_ids, varlen, vsize.value, res

    def select_ordered(self, preds, cols, order_by, descending=False,
                       nulls_first=False, limit=0, after=None, row_lo=0,
                       row_hi=None, cap=1 << 16, varlen_cap=1 << 20):
        """SELECT cols WHERE preds ORDER BY order_by [DESC] LIMIT limit on
        the snapshot: returns (rows, cursor, result). rows as select()'s;
        cursor is the last delivered row's place in the order (None when
        nothing was delivered): pass it as `after` for the next page until
        result.r.done. Ties are broken by snapshot position, ascending."""
        strs = None
        if self._schema is not None and len(cols) <= y.MAX_SELECT_COLS:
            try:
                strs = y.select_string_cols(self._schema, cols)
            except IndexError:  # out of range: the ABI names the offender
                strs = None
        datums, null_masks, _ids, varlen, _vs, res = self.select_ordered_raw(
            preds, cols, order_by, descending, nulls_first, limit, after,
            row_lo, row_hi, cap, varlen_cap)
        rows = y.decode_snapshot_rows(res.r, datums, null_masks, len(cols),
                                      cols, cap, varlen, strs)
        return rows, y.order_cursor(res), res

    def kernel_ms(self):
        ms = C.c_double()
        self._check(self._lib.yb_gpu_snapshot_kernel_ms(self._h,
                                                        C.byref(ms)),
                    "snapshot_kernel_ms")
        return ms.value

    def close(self):
        if self._h:
            self._lib.yb_gpu_snapshot_close(self._h)
            self._h = None
