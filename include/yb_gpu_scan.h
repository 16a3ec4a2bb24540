/*
 * include/yb_gpu_scan.h — the drop-in C ABI for the MI355X-native DocDB
 * SST-block scan-and-filter path.
 *
 * This ABI is the boundary a YugabyteDB tablet server would call through in
 * place of the CPU DocRowwiseIterator row loop. Each entry point names the
 * reference interface it replaces (paths relative to yugabyte/yugabyte-db):
 *
 *   yb_gpu_scan_open        ~ YQLStorageIf::GetIterator + DocRowwiseIterator
 *                             ctor/Init  (src/yb/docdb/ql_storage_interface.h:
 *                             37-120, doc_rowwise_iterator.h:52-81,
 *                             doc_rowwise_iterator.cc:165-231)
 *   yb_gpu_scan_feed_blocks ~ the BoundedRocksDbIterator data source — the
 *                             already-flushed, decompressed data blocks a
 *                             tablet scan walks (rocksdb/table/block.cc)
 *   yb_gpu_scan_execute     ~ PgsqlReadOperation::ExecuteScalar row loop
 *                             (src/yb/docdb/pgsql_operation.cc:2808-2931)
 *   yb_gpu_scan_aggregate   ~ EvalAggregate/PopulateAggregate
 *                             (src/yb/docdb/pgsql_operation.cc:3171-3186)
 *   yb_gpu_scan_next_batch  ~ YQLRowwiseIteratorIf::PgFetchNext(PgTableRow*)
 *                             batched (src/yb/docdb/
 *                             ql_rowwise_iterator_interface.h:32-97)
 *   yb_gpu_scan_paging_state~ SetPagingState (pgsql_operation.cc:2908-2922)
 *
 * Error convention mirrors yb::Status (src/yb/util/status_fwd.h): int code
 * (0 = OK) + message via yb_gpu_last_error. No exceptions cross the ABI.
 * Threading: one handle == one HIP stream, single caller per handle
 * (CheckInitOnce, doc_rowwise_iterator.cc:128-135); different handles are
 * independent (one per tablet/GPU).
 *
 * The same library also exports the synthetic tablet generator (the write
 * path needed to build benchmark/parity datasets — BlockBuilder
 * rocksdb/table/block_builder.cc, RowPacker dockv/packed_row.cc).
 */
#ifndef YB_GPU_SCAN_H
#define YB_GPU_SCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- shared descriptors -------------------------------------------------- */

/* Value-column data types (DataType subset — src/yb/common/value.messages.h).
 * Values match oracle/orcl.h orcl_dtype_t for test convenience. */
typedef enum {
  YBG_T_BOOL = 0,
  YBG_T_INT8 = 1,
  YBG_T_INT16 = 2,
  YBG_T_INT32 = 3,
  YBG_T_INT64 = 4,
  YBG_T_UINT32 = 5,
  YBG_T_UINT64 = 6,
  YBG_T_FLOAT = 7,
  YBG_T_DOUBLE = 8,
  YBG_T_STRING = 9,
} ybg_dtype_t;

typedef enum {
  YBG_KT_INT64 = 0,
  YBG_KT_INT32 = 1,
  YBG_KT_STRING = 2,
} ybg_keytype_t;

/* src/yb/rocksdb/types.h:50-56 KeyValueEncodingFormat */
typedef enum {
  YBG_ENC_SHARED_PREFIX = 0,
  YBG_ENC_THREE_SHARED_PARTS = 1,
} ybg_kv_format_t;

#define YBG_MAX_COLS 32
#define YBG_MAX_KEYCOLS 8
#define YBG_MAX_PREDS 8
#define YBG_MAX_AGGS 8
#define YBG_MAX_HT 16

typedef struct {
  int32_t column_id;
  int32_t dtype;    /* ybg_dtype_t */
  int32_t nullable; /* affects V1 packing varlen-ness (schema_packing.cc:45-49) */
} ybg_value_col_t;

typedef struct {
  int32_t has_hash;
  int32_t num_hash_cols;
  int32_t num_range_cols;
  int32_t key_types[YBG_MAX_KEYCOLS]; /* ybg_keytype_t */
  int32_t num_value_cols;
  ybg_value_col_t value_cols[YBG_MAX_COLS];
} ybg_schema_t;

/* Encoded read-time limits (EncodedReadHybridTime —
 * src/yb/docdb/intent_aware_iterator.h:61-77). */
typedef struct {
  uint8_t read[YBG_MAX_HT];         int32_t read_len;
  uint8_t local_limit[YBG_MAX_HT];  int32_t local_limit_len;
  uint8_t global_limit[YBG_MAX_HT]; int32_t global_limit_len;
} ybg_read_time_t;

/* Helper: build the three encoded limits from plain hybrid times
 * (micros<<12|logical) with write_id = kMaxWriteId
 * (intent_aware_iterator.cc:1446-1455). */
void ybg_read_time_init(ybg_read_time_t *rt, uint64_t read_ht,
                        uint64_t local_limit_ht, uint64_t global_limit_ht);

typedef enum {
  /* Typed compares of the column datum with pred.datum. Integer columns
   * compare as signed 64-bit (UINT64 values from 2^63 up compare as
   * negative). FLOAT and DOUBLE columns compare as IEEE 754 has it: -0.0
   * equals +0.0, and with a NaN on either side every op is false except
   * NE, which is true; IN and IN_RANGE likewise never match a NaN. A NULL
   * column fails every predicate. */
  YBG_PRED_GT = 0, YBG_PRED_GE, YBG_PRED_LT, YBG_PRED_LE,
  YBG_PRED_EQ, YBG_PRED_NE,
  /* IN-list membership. NUMERIC column: bytes = n x 8-byte little-endian
   * datum bit patterns (the column dtype's representation), bytes_len =
   * 8n. STRING column (value or key): bytes = [u32 LE length][raw bytes]
   * records back to back, bytes_len covering them exactly (key-column
   * options are given UNESCAPED; the kernels compare against the
   * zero-escaped rowkey form on the fly, doc_kv_util.h:101-167).
   * This is the scan-side equivalent of the reference's hybrid-scan
   * option filters (docdb/hybrid_scan_choices.h:43-60, IN extraction
   * qlexpr/ql_scanspec.cc:323-346): on a brute-force bandwidth-bound GPU
   * scan the discrete options become a filter, not a seek plan. */
  YBG_PRED_IN,
  /* Tuple membership over MULTIPLE numeric KEY columns — the reference's
   * multi-column option groups ((r1,r3) IN ((1,3),(5,6)) ...),
   * docdb/hybrid_scan_choices.h:43-77. bytes layout:
   *   [u32 LE ncols][u32 LE key-col index x ncols]
   *   [tuples: ncols x 8-byte LE datum patterns each]
   * is_key_col must be 1; col is ignored. */
  YBG_PRED_IN_TUPLE,
  /* Option RANGES over a NUMERIC column (key or value) — the reference's
   * mixed bound options (docdb/hybrid_scan_choices.h:43-77 OptionRange):
   * bytes = n x 24-byte records
   *   [u64 LE lo][u64 LE hi][u32 LE flags: bit0 lo incl, bit1 hi incl]
   *   [u32 pad]
   * true when the column datum falls in ANY range. Numeric bounds use
   * the column dtype's bit pattern (int compares signed, double/float
   * as FP). Range options on the leading range-key column of a
   * range-sharded table also PRUNE the scanned block set (see
   * yb_gpu_scan_feed_blocks). */
  YBG_PRED_IN_RANGE,
} ybg_pred_op_t;

typedef struct {
  int32_t is_key_col;
  int32_t col;
  int32_t op;       /* ybg_pred_op_t */
  uint64_t datum;   /* numeric rhs bit pattern (dtype of the column) */
  const uint8_t *bytes; /* string rhs */
  uint64_t bytes_len;
} ybg_pred_t;

/* Unspecified results (they depend on the order in which rows and
 * partials are folded, which differs between kernels and runs):
 *  - MIN/MAX_DOUBLE over a column holding NaN: a NaN is kept or dropped
 *    depending on where it is met (every `<` / `>` with a NaN is false).
 *  - MIN/MAX_DOUBLE over both +0.0 and -0.0: the result compares equal to
 *    zero; its sign is unspecified.
 *  - SUM_DOUBLE whose partial sums round or overflow, e.g. the cancelling
 *    DBL_MAX, -DBL_MAX, 1.0: any summation order's result may be returned.
 *    Sums whose every partial sum is exact are bit-reproducible.
 * COUNT ops and every integer aggregate are exact and order-independent. */
typedef enum {
  YBG_AGG_COUNT = 0,
  YBG_AGG_COUNT_STAR = 1,
  /* Sums the column's 64-bit datum (narrow ints sign-extended, UINT32
   * zero-extended) modulo 2^64: on overflow the result wraps as two's
   * complement, identically on every execution path. */
  YBG_AGG_SUM_INT64 = 2,
  YBG_AGG_SUM_DOUBLE = 3,
  YBG_AGG_MIN_INT64 = 4,
  YBG_AGG_MAX_INT64 = 5,
  YBG_AGG_MIN_DOUBLE = 6,
  YBG_AGG_MAX_DOUBLE = 7,
} ybg_agg_op_t;

typedef struct {
  int32_t op;  /* ybg_agg_op_t */
  int32_t col; /* value column index */
} ybg_agg_t;

/* Scan spec — the YQLScanSpec/DocPgsqlScanSpec surface reduced to what the
 * hot path consumes (qlexpr/ql_scanspec.h:200-267 bounds;
 * pgsql_operation.cc:602-668 predicates; :3171-3186 aggregates). */
typedef struct {
  ybg_schema_t schema;
  int32_t kv_format; /* ybg_kv_format_t */
  ybg_read_time_t read_time;
  int32_t num_preds;
  ybg_pred_t preds[YBG_MAX_PREDS];
  int32_t num_aggs;
  ybg_agg_t aggs[YBG_MAX_AGGS];
  const uint8_t *lower_bound; uint64_t lower_bound_len; /* incl., encoded DocKey */
  const uint8_t *upper_bound; uint64_t upper_bound_len; /* excl. */
  int32_t emit_rows;  /* 1: materialize matching rows (next_batch) */
  uint64_t row_limit; /* 0 = unlimited; else paging after this many rows */
  /* GROUP BY (config #5 "GROUP-BY-key partial aggregates"):
   * 0 = plain aggregates, else 1 + value-column index to group on. */
  int32_t group_col;
  /* Scan direction (doc_rowwise_iterator.cc:690-818 FetchNextImpl is
   * direction-templated; SkipFutureRecords<Direction::kBackward>,
   * intent_aware_iterator.cc:1319ff). On this engine the bandwidth-bound
   * full scan is direction-NEUTRAL (every block is scanned in parallel
   * and visibility picks the same newest version either way); backward is
   * a DELIVERY-ORDER property of the boundary: rows come back in
   * descending DocKey order, row_limit pages deliver the highest keys
   * first, and the paging state becomes an EXCLUSIVE upper bound for the
   * resumed scan. Aggregate results are unaffected by direction. */
  int32_t backward;
  /* Caller hint: nonzero when the scan expects multi-version rows — a
   * historical-snapshot read (ReadHybridTime in the past of recent
   * writes) or a not-yet-compacted history window. The reference's
   * callers know this when they build the read operation
   * (docdb/doc_read_context.h read time + retention policy); here it
   * selects the version-chain-optimized decode shape of the fast scan
   * kernel (a measured +16% on MVCC-heavy data, -4% on single-version
   * data — results are identical either way, 0 is always safe). */
  int32_t expect_versions;
} ybg_scan_spec_t;

/* ---- scan handle --------------------------------------------------------- */

typedef struct ybg_scan ybg_scan_t;

/* Last error message for the calling thread. */
const char *yb_gpu_last_error(void);

/* Open a scan. Returns 0 and sets *out on success; nonzero error code
 * otherwise. Requires a visible MI355X (gfx950) device: this is the GPU
 * product path — there is NO CPU fallback. */
int yb_gpu_scan_open(const ybg_scan_spec_t *spec, ybg_scan_t **out);

/* Feed the tablet's data blocks. blocks: concatenated raw block contents
 * (uncompressed, no 5-byte file trailer); offsets[i]..offsets[i+1] delimit
 * block i (offsets has n+1 entries). The memory is borrowed for the handle's
 * lifetime. `device` nonzero means `blocks` is already a device pointer
 * (resident in HBM); otherwise it is copied host->device once here. */
int yb_gpu_scan_feed_blocks(ybg_scan_t *s, const uint8_t *blocks,
                            const uint64_t *offsets, uint64_t n_blocks,
                            int device);

/* Feed a complete BlockBasedTable SST file (host memory): parses the
 * version-2 footer + index block (rocksdb/table/format.cc:59-155,
 * block_based_table_builder.cc:658-700), optionally verifies every data
 * block's masked-crc32c trailer, strips trailers and feeds the data
 * blocks. kNoCompression blocks only (the reference-supported uncompressed
 * configuration, docdb_rocksdb_util.cc:200-221). */
int yb_gpu_scan_feed_sst(ybg_scan_t *s, const uint8_t *file, uint64_t size,
                         int verify_checksums);

/* Run the scan asynchronously on the handle's stream. */
int yb_gpu_scan_execute(ybg_scan_t *s);

/* Block until the scan completes; returns status. */
int yb_gpu_scan_wait(ybg_scan_t *s);

typedef struct {
  int64_t value_i64;
  double value_f64;
  int32_t is_null;
  int32_t pad_;
} ybg_agg_result_t;

typedef struct {
  uint64_t rows_scanned;  /* visible rows visited */
  uint64_t rows_matched;  /* rows passing predicates */
  uint64_t entries_seen;  /* KV entries decoded */
  ybg_agg_result_t aggs[YBG_MAX_AGGS];
  /* Read-restart data (GetReadRestartData analog,
   * intent_aware_iterator.cc:1400-1410): when local_limit > read and a
   * visible record committed in (read, local_limit], the ENCODED
   * DocHybridTime of the newest such record (the max seen commit time,
   * smallest encoded bytes). restart_ht_len == 0 means no restart. */
  uint8_t restart_ht[YBG_MAX_HT];
  uint32_t restart_ht_len;
  uint32_t pad2_;
} ybg_scan_result_t;

/* Fetch aggregate results (implies wait). */
int yb_gpu_scan_aggregate(ybg_scan_t *s, ybg_scan_result_t *out);

/* GROUP BY (spec.group_col >= 0): run the grouped scan and return the
 * per-group partials. keys[g]: numeric group key datum, or for string group
 * columns (len<<40)|offset into key_bytes. vals/cnts:
 * [n_groups * YBG_MAX_AGGS], aggregate g of group i at i * YBG_MAX_AGGS + g
 * (value bit pattern + non-null contribution count; cnt==0 <=> NULL).
 * Entries come in no particular order. The group of rows whose group column
 * is NULL has keys[g] == ~0, which is also the datum of an integer -1:
 * yb_gpu_scan_group_null_index tells the two apart.
 * Returns 0 and *n_groups on success; error if cap exceeded. Integer
 * aggregates are exact; grouped double SUM uses device atomics and is only
 * reproducible up to summation order. */
int yb_gpu_scan_group_aggregate(ybg_scan_t *s, uint64_t *keys,
                                int64_t *vals, uint64_t *cnts,
                                uint8_t *key_bytes, uint64_t key_bytes_cap,
                                uint64_t cap, uint64_t *n_groups);

/* Which entry of the yb_gpu_scan_group_aggregate output is the NULL-key
 * group: *index_out in [0, n_groups), or -1 when no row had a NULL group
 * column. Every other entry with keys[g] == ~0 is the group of the integer
 * -1. Valid only when the latest yb_gpu_scan_group_aggregate call on this
 * handle succeeded; error 4 otherwise. */
int yb_gpu_scan_group_null_index(ybg_scan_t *s, int64_t *index_out);

/* Materialized row batch (PgTableRow analog — dockv/pg_row.h:91-179).
 * Row order within the batch is by (sort_key) = the row's position in the
 * tablet (block index << 32 | entry ordinal); rows are emitted unsorted —
 * callers needing key order sort by sort_key. */
typedef struct {
  uint64_t n_rows;
  uint64_t n_key_cols;
  uint64_t n_value_cols;
  const uint64_t *sort_key;   /* [n_rows] */
  const uint64_t *key_datums; /* [n_rows * n_key_cols] */
  const uint64_t *datums;     /* [n_rows * n_value_cols]; string cols: offset
                                 into varlen heap (hi32 = len) */
  const uint32_t *null_masks; /* [n_rows] bit i = value col i NULL */
  const uint16_t *hashes;     /* [n_rows] kUInt16Hash prefix (hash schemas) */
  const uint8_t *varlen;      /* varlen heap */
  uint64_t varlen_size;
} ybg_row_batch_t;

/* Fetch the materialized matching rows (host-visible; implies wait).
 * Valid until the next execute/close on this handle. */
int yb_gpu_scan_next_batch(ybg_scan_t *s, ybg_row_batch_t *out);

/* Read-restart data of the last execute/group_aggregate
 * (GetReadRestartData analog — intent_aware_iterator.cc:1400-1410): the
 * encoded DocHybridTime (smallest encoded = max commit time) of a visible
 * record committed in (read, local_limit], i.e. the time the statement
 * must restart at. *len_out == 0 means no restart. The plain aggregate
 * path also reports this in ybg_scan_result_t.restart_ht; this entry
 * point exists for the GROUP BY path, whose result shape has no restart
 * field. ht_out must hold YBG_MAX_HT bytes. */
int yb_gpu_scan_restart_data(ybg_scan_t *s, uint8_t *ht_out,
                             uint32_t *len_out);

/* ---- SST bloom filter (docdb_filter_policy / rocksdb FixedSizeFilter,
 * SURVEY 8f-2). Exact reference bit format: 64-byte cache-line blocks,
 * 5-byte trailer, rocksdb::Hash(0xbc9f1d34) with signed-char tail
 * (rocksdb/util/bloom.cc:43-62,384-452; util/hash.cc:32-77). Keys are
 * transformed to the DocKeyPart::kUpToHashOrFirstRange prefix
 * (DocDbAwareV3FilterPolicy, docdb/docdb_filter_policy.cc:110-117).
 * The filter is an optimization only: scan results are identical with
 * or without it. */
uint64_t ybg_filter_slice_size(void);
/* Build a filter over every distinct key prefix of a finished tablet.
 * out receives concatenated fixed-size slices (out_len a multiple of
 * ybg_filter_slice_size()). 0 ok, 8 cap too small, 3 corruption. */
int ybg_filter_from_sst(const uint8_t *data, const uint64_t *offsets,
                        uint64_t n_blocks, int kv_format, uint8_t *out,
                        uint64_t cap, uint64_t *out_len);
/* KeyMayMatch: 1 = prefix may exist, 0 = definitely absent. */
int ybg_filter_may_match(const uint8_t *filt, uint64_t filt_len,
                         const uint8_t *key, uint64_t key_len);
/* Test hook: extracted kUpToHashOrFirstRange prefix length (0 =
 * unparseable => always-match). */
uint64_t ybg_filter_key_prefix_len(const uint8_t *key, uint64_t key_len);
/* feed_blocks + bloom consultation: when the spec's DocKey bounds pin a
 * single filter prefix and the filter proves it absent, the scan is
 * answered empty without uploading any block. filter may be NULL. */
int yb_gpu_scan_feed_blocks_bloom(ybg_scan_t *s, const uint8_t *blocks,
                                  const uint64_t *offsets,
                                  uint64_t n_blocks, int device_resident,
                                  const uint8_t *filter,
                                  uint64_t filter_len);

/* Resumable position (pgsql_operation.cc:2796-2806, 2908-2922): for an
 * unlimited scan reports length 0 (complete). row_limit paging requires
 * delivered-row ORDER, which the batch ABI leaves to the row-at-a-time
 * adapter — use yb_host_iter_paging_state (host_iterator.h); calling this
 * on a limited scan returns an error directing there. */
int yb_gpu_scan_paging_state(ybg_scan_t *s, uint8_t *key_out, size_t cap,
                             size_t *len_out);

/* Kernel-time accounting for the last execute (HIP events on the handle's
 * stream): total kernel ms and the dominant (decode) kernel's ms. */
int yb_gpu_scan_kernel_ms(ybg_scan_t *s, double *total_ms, double *decode_ms);

int yb_gpu_scan_close(ybg_scan_t *s);

/* Returns 1 if the last yb_gpu_scan_execute on this handle was answered from
 * a columnar snapshot (YBG_STAGE=1 transparent mode, below), 0 if it ran the
 * block-bytes path. */
int yb_gpu_scan_staged(ybg_scan_t *s);

/* Returns 1 if the last yb_gpu_scan_execute on this handle launched the
 * planned fast kernel (the query compiled into a column plan: range
 * predicates on 8-byte integer columns, SUM_INT64 / COUNT / COUNT(*)), 0 if
 * it ran the interpreted fast kernel, the general kernel or a snapshot.
 * YBG_PLAN=0 forces 0. Results are identical either way. */
int yb_gpu_scan_planned(ybg_scan_t *s);

/* How many batches the last yb_gpu_scan_execute on this handle handed from
 * the fast kernel to the general kernel (entry forms outside the fast
 * shape): the batches of the handle's remembered abort set, launched next to
 * the fast kernel, plus the ones that aborted late. Waits for the execute.
 * 0 when the execute did not run a fast kernel (general dispatch, snapshot,
 * bloom-rejected). Returns 0 or an error code. YBG_KNOWN=0 keeps every
 * execute on the serial order (fast kernel, then the retry launch); results
 * are identical either way. */
int yb_gpu_scan_retry_batches(ybg_scan_t *s, uint64_t *n_out);

/* ---- columnar snapshot ---------------------------------------------------
 *
 * A DIFFERENT STORAGE CONTRACT from the rest of this header: everything
 * above scans the reference's SST block bytes as they are; a snapshot is
 * "rows visible at one read time, staged once, queried many times" — the
 * role a read-point-pinned scan over an immutable tablet plays in the
 * reference (one DocRowwiseIterator per statement at a fixed
 * ReadHybridTime, doc_rowwise_iterator.cc:165-231; many statements of one
 * transaction share the read point). It is an additional mode: the
 * block-bytes path stays the default.
 *
 * Staged: every non-STRING value column and every non-STRING key column
 * (key columns indexed like ybg_row_batch_t.key_datums), one 8-byte datum
 * per row per column in the bit pattern yb_gpu_scan_next_batch delivers,
 * plus one uint32 null mask per row (ybg_row_batch_t.null_masks layout).
 * String columns are not staged unless the snapshot is built with
 * yb_gpu_snapshot_build_ex and stage_strings (below). Rows are held in
 * tablet key order.
 *
 *   yb_gpu_snapshot_build ~ DocRowwiseIterator ctor/Init + the full
 *                           FetchNext loop at the read point, with its
 *                           output kept resident instead of streamed
 *   yb_gpu_snapshot_query ~ PgsqlReadOperation::ExecuteScalar row loop +
 *                           EvalAggregate (pgsql_operation.cc:2808-2931,
 *                           3171-3186) over the staged rows
 */
typedef struct ybg_snapshot ybg_snapshot_t;

/* Build from a FED handle. Contents: every row visible at s->spec.read_time
 * inside s->spec's DocKey bounds. The spec's predicates, aggregates,
 * row_limit, group_col, emit_rows and backward are IGNORED for the build.
 * The snapshot owns its memory and stays valid after yb_gpu_scan_close(s).
 * Feed-time block pruning by the DocKey bounds is consistent with that (the
 * bounds stay part of the snapshot). A handle whose feed pruned blocks by
 * a leading-range-key IN / IN_RANGE predicate (yb_gpu_scan_feed_blocks on
 * a range-sharded table) no longer holds every row inside the bounds: the
 * build refuses it with error 9 — build from a handle opened without that
 * predicate. (The YBG_STAGE=1 mode below still stages such a handle: there
 * every query is the handle's own spec, predicate included.)
 * Errors: 4 not fed, 6 corrupt entries, 8 row capacity, 9 option-pruned
 * handle, 10 device. */
int yb_gpu_snapshot_build(ybg_scan_t *s, ybg_snapshot_t **out);

typedef struct {
  uint64_t n_rows;          /* visible rows staged */
  uint64_t entries_seen;    /* KV entries the build scan decoded */
  uint64_t device_bytes;    /* HBM held by the snapshot */
  double   build_ms;        /* device time of the build (events) */
  uint32_t staged_value_cols; /* bit i: value col i staged (numeric) */
  uint32_t nullable_cols;   /* bit i: value col i has >=1 NULL in the snapshot */
  uint8_t  restart_ht[YBG_MAX_HT]; uint32_t restart_ht_len; /* as ybg_scan_result_t */
} ybg_snapshot_info_t;
int yb_gpu_snapshot_info(ybg_snapshot_t *sn, ybg_snapshot_info_t *out);

/* Build with options. opts == NULL or stage_strings == 0 is exactly
 * yb_gpu_snapshot_build (which is a call of this). With stage_strings every
 * STRING value column and every STRING key column is staged too, key strings
 * UNESCAPED, in the form yb_gpu_scan_next_batch delivers. Per staged string
 * column the snapshot holds, in row order, n_rows + 1 uint64 byte offsets,
 * the strings back to back, and one uint64 per row with the string's first
 * 8 bytes (big-endian, zero padded) that the predicates stream; all three
 * are a pure function of the rows. Errors: as yb_gpu_snapshot_build; 8 also
 * when the strings exceed 2^40 bytes.
 *
 * On a string-staged snapshot yb_gpu_snapshot_query, _group_query, _select
 * and _select_var additionally accept
 *   - predicates GT, GE, LT, LE, EQ, NE and IN on staged string value and
 *     key columns, in the block path's ABI form (compare: bytes / bytes_len
 *     is the rhs; IN: bytes is a list of [u32 len][bytes] records; key
 *     operands unescaped) and with its semantics: byte-wise unsigned memcmp
 *     order, a proper prefix sorts first, a predicate on a NULL string
 *     fails, the empty string is a value and not NULL;
 *   - YBG_AGG_COUNT on a string value column (it reads only the null bit).
 * Still error 9 there: IN_RANGE on a string column, SUM / MIN / MAX on a
 * string column, a string GROUP BY column, and a string column in the
 * projection of yb_gpu_snapshot_select (use yb_gpu_snapshot_select_var).
 * ybg_snapshot_info_t.staged_value_cols keeps meaning "numeric staged";
 * device_bytes includes the string storage. */
typedef struct {
  int32_t stage_strings;    /* 1: stage string value and key columns */
  int32_t reserved[7];      /* must be zero */
} ybg_snapshot_build_opts_t;
int yb_gpu_snapshot_build_ex(ybg_scan_t *s, const ybg_snapshot_build_opts_t *opts,
                             ybg_snapshot_t **out);

typedef struct {
  uint32_t staged_string_value_cols;  /* bit i: STRING value col i staged */
  uint32_t staged_string_key_cols;    /* bit i: STRING key col i staged */
  uint64_t string_bytes[YBG_MAX_COLS];        /* heap bytes per value column */
  uint64_t key_string_bytes[YBG_MAX_KEYCOLS]; /* heap bytes per key column */
} ybg_snapshot_string_info_t;
/* All fields zero on a snapshot built without strings. */
int yb_gpu_snapshot_string_info(ybg_snapshot_t *sn, ybg_snapshot_string_info_t *out);

typedef struct {
  int32_t num_preds; ybg_pred_t preds[YBG_MAX_PREDS];
  int32_t num_aggs;  ybg_agg_t  aggs[YBG_MAX_AGGS];
} ybg_snapshot_query_t;

/* Synchronous. Fills rows_scanned (= n_rows), rows_matched, entries_seen
 * (= the build's), aggs[], restart_ht (= the build's).
 * Predicates: GT..NE, IN and IN_RANGE on any staged value or key column;
 * aggregates: all eight ops on staged value columns. Anything else (string
 * column, IN_TUPLE, column index out of range, num_preds/num_aggs over the
 * caps) returns 9 with a message naming the offending predicate or
 * aggregate, and launches nothing. NULL semantics are the scan path's: a
 * predicate on a NULL operand fails; COUNT(col), SUM, MIN, MAX skip NULLs;
 * an aggregate with no contribution reports is_null. Results — double SUM
 * included — are bit-identical across repeated queries and across
 * separately built snapshots of the same tablet. */
int yb_gpu_snapshot_query(ybg_snapshot_t *sn, const ybg_snapshot_query_t *q,
                          ybg_scan_result_t *out);
/* GROUP BY on a snapshot: predicates as for yb_gpu_snapshot_query, 1 to
 * YBG_MAX_AGGS aggregates (all eight ops), one group column — any staged
 * value column or staged key column (every numeric column: int64, int32,
 * double, bool). */
typedef struct {
  int32_t num_preds; ybg_pred_t preds[YBG_MAX_PREDS];
  int32_t num_aggs;  ybg_agg_t  aggs[YBG_MAX_AGGS];
  int32_t group_is_key_col;   /* like ybg_pred_t.is_key_col */
  int32_t group_col;          /* like ybg_pred_t.col */
  uint64_t expect_groups;     /* hint; 0 = unknown */
} ybg_snapshot_group_query_t;

typedef struct {
  uint64_t n_groups;          /* incl. the NULL-key group */
  uint64_t rows_scanned, rows_matched, entries_seen;
  int32_t  has_null_group;    /* 1: LAST entry is the NULL-key group, keys[] = 0 */
  int32_t  local_level;       /* 1: the LDS-level kernel ran, 0: global-only */
  uint8_t  restart_ht[YBG_MAX_HT]; uint32_t restart_ht_len;  /* the build's */
} ybg_snapshot_group_result_t;

/* Synchronous. keys: [cap]; vals / cnts: [cap * YBG_MAX_AGGS].
 * Layout: entry i holds keys[i] and vals / cnts[i * YBG_MAX_AGGS + g] for
 *   aggregate g: value bit pattern + contribution count, cnt == 0 <=> NULL;
 *   columns past num_aggs are written as zero.
 * Order: ascending by the group key datum taken as an UNSIGNED 64-bit
 *   pattern (the bit pattern yb_gpu_scan_next_batch delivers for the
 *   column). This is a canonical order, not SQL order: negative integers
 *   and doubles do not sort numerically.
 * NULL group: rows whose group-column value is NULL (key columns are never
 *   NULL) form one group; if present it is the LAST entry, its keys[] is 0
 *   and out->has_null_group is 1 — it cannot be mistaken for any key value
 *   (a tablet holding both key -1 and NULL keys yields two groups).
 * Determinism: keys, vals and cnts are byte-identical across repeated
 *   queries, across separately built snapshots of the same tablet, and
 *   whichever kernel level ran. Double SUM accumulates as 128-bit 2^-60
 *   fixed point, so it is exact in any order; a non-finite operand or one
 *   outside +-2^66 poisons that group's sum to NaN (the block path's rule).
 * Levels: with expect_groups <= ybg_snapshot_group_local_slots(num_aggs)
 *   (0 = unknown included) rows are first aggregated in a workgroup-local
 *   LDS table that is flushed once into the global table; a larger hint
 *   sends every row straight to the global table. The hint never changes
 *   the result; out->local_level reports the level that ran.
 * Semantics: NULL handling is yb_gpu_snapshot_query's. An empty snapshot or
 *   a query no row matches returns n_groups == 0 (n_rows == 0 launches
 *   nothing).
 * Errors: 9, naming the offender, launching nothing and leaving the
 *   snapshot usable, for everything yb_gpu_snapshot_query rejects, a string
 *   or out-of-range group column, and num_aggs == 0. 8 when cap is smaller
 *   than the group count (out->n_groups then holds the count needed) or the
 *   group table overflows. 10 device.
 * Memory: the first grouped query allocates the snapshot's group table
 *   (capacity = the smallest power of two >= 2 * n_rows, clamped to
 *   [1024, 2^20]) and its export scratch; ybg_snapshot_info_t.device_bytes
 *   includes them from then on.
 * yb_gpu_snapshot_kernel_ms then reports table init + query + export. */
int yb_gpu_snapshot_group_query(ybg_snapshot_t *sn,
                                const ybg_snapshot_group_query_t *q,
                                uint64_t *keys, int64_t *vals, uint64_t *cnts,
                                uint64_t cap,
                                ybg_snapshot_group_result_t *out);
/* LDS-level slot count of the kernel instantiation a query with num_aggs
 * aggregates selects (tests derive cardinalities from it). */
uint64_t ybg_snapshot_group_local_slots(int32_t num_aggs);

/* SELECT on a snapshot: the matching rows themselves, in tablet key order,
 * with a projection, a position window, a row limit and a resume position.
 *
 *   yb_gpu_snapshot_select ~ PgsqlReadOperation::ExecuteScalar row loop +
 *                            PgFetchNext over the staged rows
 *                            (pgsql_operation.cc:2808-2931); resume_row
 *                            plays the role of SetPagingState's next row
 *                            key (pgsql_operation.cc:2796-2806, 2908-2922)
 */
#define YBG_MAX_SELECT_COLS (YBG_MAX_COLS + YBG_MAX_KEYCOLS)
typedef struct { int32_t is_key_col; int32_t col; } ybg_select_col_t;   /* as ybg_pred_t.is_key_col / .col */

typedef struct {
  int32_t num_preds; ybg_pred_t preds[YBG_MAX_PREDS];        /* rules of yb_gpu_snapshot_query */
  int32_t num_cols;  ybg_select_col_t cols[YBG_MAX_SELECT_COLS]; /* projection, 1..cap, repeats allowed */
  int32_t backward;          /* 1: deliver in descending key order */
  uint64_t row_lo, row_hi;   /* window of snapshot positions [row_lo, row_hi); row_hi is clamped to n_rows
                                (UINT64_MAX = to the end); row_lo >= row_hi is an empty window */
  uint64_t row_limit;        /* 0 = unlimited */
} ybg_snapshot_select_t;

typedef struct {
  uint64_t n_rows;           /* rows delivered */
  uint64_t rows_scanned;     /* positions in the window */
  uint64_t rows_matched;     /* matching rows in the window (>= n_rows) */
  uint64_t resume_row;       /* see Paging */
  int32_t  done;             /* 1: every matching row of the window was delivered */
  uint64_t entries_seen; uint8_t restart_ht[YBG_MAX_HT]; uint32_t restart_ht_len;  /* the build's */
} ybg_snapshot_select_result_t;

/* Synchronous, on the snapshot's own stream, like the other two queries.
 * row_ids / null_masks: [cap]; datums: [num_cols * cap].
 * Order: a position is a row's index in the snapshot; snapshot rows are held
 *   in tablet key order. Delivered rows are ascending by position, or
 *   descending with backward.
 * row_ids[i]: delivered row i's position.
 * datums: column-major — projected column j of delivered row i is at
 *   datums[j * cap + i], in the bit pattern yb_gpu_scan_next_batch delivers.
 *   The datum of a NULL is written as 0.
 * null_masks[i]: ybg_row_batch_t.null_masks layout (bit c = value column c
 *   is NULL), masked to the projected value columns, so the output bytes are
 *   a pure function of the rows. Key columns are never NULL.
 * Limit: forward delivers the first row_limit matches of the window,
 *   backward the last row_limit matches, highest first. rows_matched always
 *   counts every match in the window.
 * Paging: done = (n_rows == rows_matched). Forward: resume_row is the last
 *   delivered position + 1, or row_hi (clamped) when done; the next page
 *   passes it as row_lo. Backward: resume_row is the last (lowest) delivered
 *   position, or row_lo when done; the next page passes it as row_hi. The
 *   concatenated pages equal the unlimited result exactly.
 * Determinism: datums, null_masks and row_ids are byte-identical across
 *   repeated calls and across separately built snapshots of the same tablet.
 * Errors: 9, naming the offender, launching nothing and leaving the snapshot
 *   usable, for everything yb_gpu_snapshot_query rejects in a predicate, a
 *   projected string or out-of-range column, num_cols == 0 and num_cols over
 *   YBG_MAX_SELECT_COLS. 8 when cap is smaller than the number of rows to
 *   deliver (out->n_rows then holds the count needed; the other counters
 *   are filled). 10 device.
 * An empty snapshot or an empty window launches nothing and returns zero
 *   rows with done = 1.
 * Memory: the first select allocates the snapshot's select scratch (match
 *   bitmap, per-tile counts and offsets) and its device output buffers, the
 *   latter grown on demand; ybg_snapshot_info_t.device_bytes includes them
 *   from then on.
 * yb_gpu_snapshot_kernel_ms then reports count + scan + gather. */
int yb_gpu_snapshot_select(ybg_snapshot_t *sn, const ybg_snapshot_select_t *q,
                           uint64_t *datums, uint32_t *null_masks, uint64_t *row_ids,
                           uint64_t cap, ybg_snapshot_select_result_t *out);
/* The select with string projection, on a snapshot built with
 * stage_strings. Everything documented for yb_gpu_snapshot_select holds
 * (order, window, limit, paging, determinism, errors), plus:
 * datums: a projected string column's datum is (len << 40) | offset into
 *   varlen (the ybg_row_batch_t convention); a NULL is written as 0.
 * varlen: [varlen_cap]. The heap is canonical: delivered rows in delivery
 *   order, within a row the projected string columns in projection order
 *   (a repeated column repeats its bytes), bytes back to back with no
 *   padding. varlen[0 .. *varlen_size) is therefore a pure function of the
 *   delivered rows: byte-identical across calls and across separately built
 *   snapshots of the same tablet.
 * Errors: also 8 when varlen_cap is smaller than the bytes to deliver;
 *   *varlen_size then holds the size needed and the counters are filled as
 *   for the row cap.
 * With no string column projected it equals yb_gpu_snapshot_select, with
 *   *varlen_size == 0.
 * Memory: the per-row offsets, the scan scratch and the device heap are
 *   snapshot-owned, grown on demand and counted in device_bytes.
 * yb_gpu_snapshot_kernel_ms then also covers the string copy. */
int yb_gpu_snapshot_select_var(ybg_snapshot_t *sn, const ybg_snapshot_select_t *q,
                               uint64_t *datums, uint32_t *null_masks, uint64_t *row_ids,
                               uint64_t cap, uint8_t *varlen, uint64_t varlen_cap,
                               uint64_t *varlen_size, ybg_snapshot_select_result_t *out);
/* Rows per compaction tile of the select kernels (tests derive edges from
 * it). */
uint64_t ybg_snapshot_select_tile_rows(void);

/* ORDER BY / top-N on a snapshot: the matching rows of a window ordered by
 * one numeric value or key column, the first row_limit of them delivered,
 * with a cursor for the next page.
 *
 *   yb_gpu_snapshot_select_ordered ~ the sort node ABOVE
 *                            PgsqlReadOperation::ExecuteScalar
 *                            (pgsql_operation.cc:2808-2931), which the
 *                            reference does NOT push down to the tablet: like
 *                            GROUP BY this is the snapshot contract's own
 *                            extension, not a transcription.
 */
typedef struct {
  ybg_snapshot_select_t sel;     /* preds, projection, window [row_lo,row_hi), row_limit (0 = all);
                                    sel.backward must be 0 (error 9) */
  int32_t order_is_key_col, order_col;   /* as ybg_pred_t.is_key_col / .col */
  int32_t descending;            /* 0 ASC, 1 DESC */
  int32_t nulls_first;           /* 0: NULLs after every value (both directions), 1: before */
  int32_t have_cursor;           /* 1: deliver only rows strictly after the cursor in the order */
  int32_t cursor_is_null;
  uint64_t cursor_datum, cursor_row;
} ybg_snapshot_order_t;

typedef struct {
  ybg_snapshot_select_result_t r;  /* n_rows delivered; rows_scanned = window positions;
                                      rows_matched = matching rows of the window that lie after the
                                      cursor; done = (n_rows == rows_matched); resume_row unused (0) */
  int32_t  cursor_is_null; uint64_t cursor_datum, cursor_row;  /* last delivered row; valid if n_rows > 0 */
  uint32_t digit_passes;           /* selection passes that ran (0: no selection was needed) */
} ybg_snapshot_order_result_t;

/* Synchronous, on the snapshot's own stream. Output arrays, projection
 * rules, string projection and the error-8 handling are
 * yb_gpu_snapshot_select_var's: datums column-major with stride cap, a
 * NULL's datum 0, null_masks masked to the projection, a projected string
 * column (string-staged snapshot) on the canonical varlen heap in delivery
 * order. With no string column projected varlen may be NULL with
 * varlen_cap 0. row_ids[i] is delivered row i's snapshot position.
 * The order is total (no two rows tie): three components, compared
 *   lexicographically.
 *   1. NULL class: a row whose order column is NULL sorts after every
 *      non-NULL row, or before with nulls_first; descending does not move
 *      it. Key columns are never NULL.
 *   2. value: integer, bool and key columns compare as signed 64-bit datums
 *      (the predicates' rule; UINT64 values from 2^63 up sort as negative).
 *      DOUBLE and FLOAT (float bits in the datum's low 32 bits) compare
 *      numerically with -0.0 == +0.0 and every NaN equal to every other NaN
 *      and greater than every number, +inf included (PostgreSQL's rule), so
 *      under DESC the NaNs come first among the non-NULLs. descending
 *      reverses this component only.
 *   3. snapshot position, ascending in BOTH directions (ORDER BY col DESC,
 *      <tablet key> ASC): the result is the stable sort of the key-order
 *      select.
 *   Delivered datums are the rows' own bit patterns (a NaN keeps its
 *   payload, -0.0 stays -0.0).
 * Limit and paging: the first row_limit rows of the order are delivered
 *   (0 = all). out->cursor_* is the last delivered row's NULL class, order
 *   datum and position; passed back with have_cursor = 1 only rows strictly
 *   after it are eligible, and the concatenated pages equal the unlimited
 *   result exactly. cursor_datum goes through the same value mapping (a -0.0
 *   cursor stands for the zero class, any NaN for the NaN class).
 * digit_passes: histogram passes of the radix select that ran (8-bit
 *   digits, at most 12). 0 when no selection was needed: row_limit 0, or a
 *   limit at or above the eligible count. The eligible count comes from the
 *   count pass, or with a cursor from one marking pass over the matches.
 * Errors: 9, naming the offender, launching nothing and leaving the snapshot
 *   usable, for everything yb_gpu_snapshot_select_var rejects,
 *   sel.backward != 0, a STRING or out-of-range order column and
 *   cursor_row >= 2^32. 8 when cap (r.n_rows then holds the count needed) or
 *   varlen_cap (*varlen_size the size needed) is too small. 10 device.
 * An empty snapshot, an empty window or no eligible row returns zero rows,
 *   done = 1 and digit_passes = 0.
 * Determinism: datums, null_masks, row_ids and the heap are byte-identical
 *   across repeated calls, across separately built snapshots of one tablet
 *   and across every setting of YBG_SNAP_ORDER_CAND.
 * Memory: the selection scratch (a second bitmap and tile arrays, the digit
 *   histogram) is allocated by the first ordered select, the candidate and
 *   sort buffers are grown on demand; ybg_snapshot_info_t.device_bytes
 *   includes them from then on. The select's bitmap, tile arrays and output
 *   buffers are shared.
 * yb_gpu_snapshot_kernel_ms then reports every launch of the call. */
int yb_gpu_snapshot_select_ordered(ybg_snapshot_t *sn, const ybg_snapshot_order_t *q,
                                   uint64_t *datums, uint32_t *null_masks, uint64_t *row_ids,
                                   uint64_t cap, uint8_t *varlen, uint64_t varlen_cap,
                                   uint64_t *varlen_size, ybg_snapshot_order_result_t *out);
/* Default early-out threshold of the ordered select: the radix select stops
 * descending once the bucket that holds the limit-th row has at most this
 * many rows; the rows at or below the bucket are then compacted and sorted.
 * YBG_SNAP_ORDER_CAND=n in the environment (read per call) overrides it;
 * n = 1 switches the early-out off (every digit pass runs). */
uint64_t ybg_snapshot_order_candidate_rows(void);

/* Device time (events) of the last query: query kernel + final reduce. */
int yb_gpu_snapshot_kernel_ms(ybg_snapshot_t *sn, double *query_ms);
int yb_gpu_snapshot_close(ybg_snapshot_t *sn);

/* Transparent mode: with YBG_STAGE=1 in the environment (read at execute
 * time), yb_gpu_scan_execute on a plain aggregate handle (no emit_rows,
 * group_col or row_limit) whose predicates and aggregates a snapshot can
 * answer builds a snapshot on the handle's first execute, keeps it on the
 * handle, and answers that and later executes with the query kernel;
 * yb_gpu_scan_aggregate returns the same contents as the block path and
 * yb_gpu_scan_kernel_ms reports the query kernel's time. Ineligible handles
 * silently take the block path; unset or 0 changes nothing. The mode is
 * unchanged by string staging: it keeps building numeric-only snapshots, so
 * a handle with a string predicate or aggregate keeps taking the block
 * path. */

/* Returns 1 if a gfx950-class HIP device is visible. */
int yb_gpu_available(void);

/* Select the HIP device subsequent handles bind to (one rank per GPU). */
int yb_gpu_set_device(int device);

/* ---- synthetic tablet generator (write path) ----------------------------- */

typedef struct ybg_builder ybg_builder_t;

/* Create a tablet builder. block_size_target: flush threshold in bytes
 * (--db_block_size_bytes, dockv/packed_row.cc:39; configs use 4096).
 * restart_interval: 16 (rocksdb/table.h:150). */
ybg_builder_t *ybg_builder_create(const ybg_schema_t *schema, int kv_format,
                                  size_t block_size_target,
                                  int restart_interval);

/* Row key for the builder: datums for int key cols, bytes for string cols. */
typedef struct {
  uint16_t hash;       /* kUInt16Hash prefix value (when schema.has_hash) */
  uint64_t datums[YBG_MAX_KEYCOLS];
  const uint8_t *strs[YBG_MAX_KEYCOLS];
  uint64_t str_lens[YBG_MAX_KEYCOLS];
} ybg_key_t;

/* Column values for a packed row: numeric bit patterns / string slices;
 * null[i] nonzero => NULL. */
typedef struct {
  uint64_t datums[YBG_MAX_COLS];
  const uint8_t *strs[YBG_MAX_COLS];
  uint64_t str_lens[YBG_MAX_COLS];
  uint8_t null[YBG_MAX_COLS];
} ybg_rowvals_t;

/* Append entries IN KEY ORDER (caller guarantees DocDB ordering:
 * user_key asc; for equal user keys impossible here since HT differs).
 * ht = micros<<12|logical. seq: rocksdb sequence number for the internal
 * key suffix (dbformat.h:84-110; initial seqno 1<<50 per
 * docdb_rocksdb_util.cc:170). packed_version: 1 or 2. */
int ybg_builder_add_packed_row(ybg_builder_t *b, const ybg_key_t *key,
                               uint64_t ht, uint32_t write_id, uint64_t seq,
                               int packed_version, const ybg_rowvals_t *vals);

/* Column update entry ('K' + svarint(column_id) subkey; value = single V1
 * value). null nonzero writes a column tombstone. */
int ybg_builder_add_column_update(ybg_builder_t *b, const ybg_key_t *key,
                                  int value_col_idx, uint64_t ht,
                                  uint32_t write_id, uint64_t seq,
                                  uint64_t datum, const uint8_t *str,
                                  uint64_t str_len, int null);

/* Row tombstone (bare key, value = kTombstone 'X'). */
int ybg_builder_add_row_tombstone(ybg_builder_t *b, const ybg_key_t *key,
                                  uint64_t ht, uint32_t write_id, uint64_t seq);

/* Append a fully custom entry (tests): raw user key + raw value. The
 * internal key suffix fixed64(seq<<8|kTypeValue) is appended here. */
int ybg_builder_add_raw(ybg_builder_t *b, const uint8_t *user_key,
                        size_t user_key_len, uint64_t seq,
                        const uint8_t *value, size_t value_len);

/* Finish: flush last block. Returns pointers valid until destroy. */
int ybg_builder_finish(ybg_builder_t *b, const uint8_t **data,
                       const uint64_t **offsets, uint64_t *n_blocks,
                       uint64_t *total_bytes, uint64_t *n_entries);

/* Finish as a complete SST FILE (data blocks + [type|masked-crc32c]
 * trailers + empty metaindex + shared-prefix index block + version-2
 * footer). Pointer valid until destroy. */
int ybg_builder_finish_sst(ybg_builder_t *b, const uint8_t **data,
                           uint64_t *total_bytes, uint64_t *n_blocks,
                           uint64_t *n_entries);

/* Host block-entry decode + first-key helpers (the intent merge's and
 * block pruning's decoder; exposed for CPU tests). */
int ybg_decode_block(const uint8_t *blk, uint64_t size, int kv_format,
                     uint8_t *keys_out, uint64_t keys_cap,
                     uint32_t *key_lens, uint8_t *vals_out,
                     uint64_t vals_cap, uint32_t *val_lens,
                     uint64_t cap_entries, uint64_t *n_entries);
int ybg_block_first_key(const uint8_t *blk, uint64_t size, int kv_format,
                        uint8_t *out, uint64_t cap, uint64_t *len);

/* Parse an SST file and report its data-block (offset, size) handles —
 * the exact parser yb_gpu_scan_feed_sst uses (exposed for CPU tests). */
int ybg_sst_index(const uint8_t *file, uint64_t size, int verify,
                  uint64_t *offsets, uint64_t *sizes, uint64_t cap,
                  uint64_t *n_blocks);

void ybg_builder_destroy(ybg_builder_t *b);

/* ---- Intents-DB merge (docdb/intent_aware_iterator.cc:983-1011
 * ProcessIntent + DecodeStrongWriteIntent; transaction status resolution
 * docdb/transaction_status_cache.cc) ----------------------------------
 *
 * The reference scans TWO sorted streams: the regular DB and the intents
 * DB holding provisional (in-flight transaction) records; each intent is
 * resolved against the transaction status cache, and a committed intent
 * behaves as a regular record positioned at its COMMIT hybrid time whose
 * value carries the intent WRITE time as a kHybridTime control prefix
 * (the committed-intent visibility rule, :1249-1267). Aborted and
 * still-pending foreign intents are invisible.
 *
 * This implementation resolves and merges at FEED time: committed intents
 * are synthesized into regular-format records and merge-rebuilt into the
 * affected data blocks (intents are sparse; untouched blocks are reused
 * byte-identical), so every scan then exercises the same committed-intent
 * visibility rule on device. The intent stream is accepted in its
 * post-DecodeStrongWriteIntent form: user key (DocKey [+ subkey], no HT
 * suffix) + write DocHybridTime fields + provisional value body. The
 * intents-DB KEY encoding (intent type sets, reverse txn index) is not
 * transcribed — it is consumed before this boundary. */
typedef struct {
  uint32_t txn_id;
  int32_t status;      /* 0 pending, 1 committed, 2 aborted */
  uint64_t commit_ht;  /* micros<<12|logical, valid when committed */
} ybg_txn_status_t;

/* Intent-stream builder (test/ingest helper). Records may be added in any
 * order; resolution sorts. Value forms mirror the regular builder. */
typedef struct ybg_intents ybg_intents_t;
ybg_intents_t *ybg_intents_create(const ybg_schema_t *schema);
int ybg_intents_add_packed_row(ybg_intents_t *it, const ybg_key_t *key,
                               uint64_t write_ht, uint32_t write_id,
                               uint32_t txn_id, int packed_version,
                               const ybg_rowvals_t *vals);
int ybg_intents_add_column_update(ybg_intents_t *it, const ybg_key_t *key,
                                  int value_col_idx, uint64_t write_ht,
                                  uint32_t write_id, uint32_t txn_id,
                                  uint64_t datum, const uint8_t *str,
                                  uint64_t str_len, int null);
int ybg_intents_add_row_tombstone(ybg_intents_t *it, const ybg_key_t *key,
                                  uint64_t write_ht, uint32_t write_id,
                                  uint32_t txn_id);
int ybg_intents_data(ybg_intents_t *it, const uint8_t **blob,
                     uint64_t *len);
void ybg_intents_destroy(ybg_intents_t *it);

/* Resolve the intent stream against the status table and merge committed
 * intents into the data blocks (host-side; affected blocks are decoded,
 * merge-inserted in internal-key order and re-encoded with the standard
 * BlockBuilder; untouched blocks copy through). Outputs are malloc'd —
 * free with ybg_free. */
int ybg_merge_intents(const uint8_t *blocks, const uint64_t *offsets,
                      uint64_t n_blocks, int kv_format,
                      const uint8_t *intents, uint64_t intents_len,
                      const ybg_txn_status_t *txns, uint32_t n_txns,
                      uint8_t **out_blocks, uint64_t **out_offsets,
                      uint64_t *out_n_blocks, uint64_t *out_total);

/* Feed regular blocks + an intent stream: resolve + merge + feed. */
int yb_gpu_scan_feed_blocks_intents(ybg_scan_t *s, const uint8_t *blocks,
                                    const uint64_t *offsets,
                                    uint64_t n_blocks,
                                    const uint8_t *intents,
                                    uint64_t intents_len,
                                    const ybg_txn_status_t *txns,
                                    uint32_t n_txns);

/* One-call multi-threaded benchmark dataset generator.
 * Produces `rows` rows of the given schema in one tablet: hash prefix walks
 * 0..65535 monotonically, one int64 range key column ascending, packed-row
 * (version as given) values seeded deterministically (seed). versions>1
 * writes that many MVCC versions per row at increasing HTs (newest at
 * ht_base + (versions-1)*ht_step). Caller frees *data with ybg_free. */
typedef struct {
  uint64_t rows;
  uint64_t seed;
  int packed_version;      /* 1 or 2 */
  int kv_format;           /* ybg_kv_format_t */
  uint32_t block_size;     /* e.g. 4096 */
  int restart_interval;    /* 16 */
  int versions;            /* MVCC versions per row (config 4: 5) */
  uint64_t ht_base_micros; /* first version's HT physical micros */
  uint64_t ht_step_micros; /* HT increment between versions */
  int nthreads;            /* 0 = hw concurrency */
  uint64_t group_mod;      /* >0: value column 0 becomes (value %% group_mod)
                              — bounded group-key cardinality for GROUP BY
                              benchmarks */
} ybg_gen_params_t;

int ybg_generate(const ybg_schema_t *schema, const ybg_gen_params_t *p,
                 uint8_t **data, uint64_t **offsets, uint64_t *n_blocks,
                 uint64_t *total_bytes, uint64_t *n_entries);

void ybg_free(void *p);

/* Encode a DocKey (doc_key.h:40-63) from key-column values (paging-state
 * serialization). Returns encoded length, 0 if cap too small. */
size_t ybg_encode_dockey(const ybg_schema_t *schema, const ybg_key_t *key,
                         uint8_t *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* YB_GPU_SCAN_H */
