// yugabyte-db_amd/csrc/snap_device.h — columnar-snapshot query logic: the
// per-row predicate/aggregate evaluation over dense per-column arrays, and
// the host-side translation of an ABI query into the POD kernel argument.
// Compiled into the HIP query kernel (snap_gpu.hip) AND the host simulator
// (scan_host_sim.cc), with the same DEV macro convention as scan_device.h.
//
// A snapshot is a DIFFERENT storage contract from "scan the reference's
// SST block bytes" (DESIGN.md §4): rows visible at one read time, staged
// once as one 8-byte datum per row per numeric column (the emit_row /
// pred_cmp_fast bit pattern) plus one null-mask word per row.
#ifndef YBG_SNAP_DEVICE_H
#define YBG_SNAP_DEVICE_H

#include <cstdio>
#include <vector>

#include "scan_device.h"

// host + device helpers (sizing rules shared by the build, the kernels and
// the simulator)
#ifdef YBG_HOST_SIM
#define YBG_HD inline
#else
#define YBG_HD __host__ __device__ inline
#endif

namespace ybgdev {

constexpr int kSnapThreads = 256;
// rows per lane per column access: 2 x 8-byte datums = one 16-byte load
constexpr int kSnapVec = 2;
// the query grid is a pure function of n_rows: one workgroup per 256 row
// pairs, capped here (grid-stride beyond). 1024 = 4 workgroups on each of
// the 256 CUs: resident in ONE round for every kernel variant that reaches
// 4 waves/SIMD. Measured on the 100M-row headline query (profiles/README.md,
// compile-time A/B through this macro): 0.67 ms at 1024 vs 0.71 / 0.76 /
// 0.73 ms at 1536 / 1792 / 2048, where a second, mostly empty round of
// workgroups trails the first.
#ifndef YBG_SNAP_MAX_GRID
#define YBG_SNAP_MAX_GRID 1024
#endif
constexpr uint64_t kSnapMaxGrid = YBG_SNAP_MAX_GRID;
// wave partial: matched, {val,cnt} x MAX_AGGS
constexpr int kSnapPartialStride = 1 + 2 * YBG_MAX_AGGS;

// Column-array length for n rows: rounded up to the per-lane vector width
// plus one vector of (zeroed) slack, so a full-width last load stays inside
// the allocation.
YBG_HD uint64_t snap_padded_rows(uint64_t n) {
  return (n + kSnapVec - 1) / kSnapVec * kSnapVec + kSnapVec;
}

YBG_HD uint64_t snap_grid(uint64_t n_rows) {
  uint64_t pairs = (n_rows + kSnapVec - 1) / kSnapVec;
  uint64_t g = (pairs + kSnapThreads - 1) / kSnapThreads;
  return g > kSnapMaxGrid ? kSnapMaxGrid : g;
}

struct SnapPred {
  const uint64_t* col;  // staged column array
  PredC pc;             // IN / IN_RANGE: datum = (count << 32) | aux offset
  uint32_t null_m;      // null-mask bit of the column (0: never NULL)
  uint32_t pad_;
};

struct SnapAgg {
  const uint64_t* col;  // nullptr: operand value unused (COUNT / COUNT(*))
  int32_t op;
  uint32_t null_m;      // null-mask bit of the operand (0: never NULL)
};

// The query kernel's argument (POD, passed by value).
struct SnapQuery {
  uint64_t n_rows;
  int32_t num_preds, num_aggs;
  SnapPred preds[YBG_MAX_PREDS];
  SnapAgg aggs[YBG_MAX_AGGS];
  const uint32_t* nullmask;  // [padded rows]
  const uint8_t* aux;        // IN / IN_RANGE lists
  int32_t any_nullable;      // some referenced column holds a NULL
  int32_t general;           // some predicate is IN / IN_RANGE
};

// Staged column table of one snapshot (device pointers; host pointers in
// the simulator).
struct SnapCols {
  const uint64_t* val[YBG_MAX_COLS];
  const uint64_t* key[YBG_MAX_KEYCOLS];
  const uint32_t* nullmask;
  uint32_t nullable_cols;  // bit i: value col i has >= 1 NULL
};

// One row. pv/av: the row's predicate / aggregate operand datums (slot i of
// the query), nm: its null mask (ignored unless NULLS), valid: the row
// exists (false for the padding row of an odd tail). NULL semantics are the
// scan path's (eval_col / acc_row): a predicate on NULL fails; COUNT(col),
// SUM, MIN, MAX skip NULL operands.
template <int NP, int NA, bool NULLS, bool GEN>
DEV void snap_row(const SnapQuery& q, const uint64_t* pv, const uint64_t* av,
                  uint32_t nm, bool valid, uint64_t* matched,
                  uint64_t* agg_val, uint64_t* agg_cnt) {
  bool pass = valid;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i >= q.num_preds) continue;
    const SnapPred& p = q.preds[i];
    bool ok = GEN ? pred_compare(p.pc, pv[i], nullptr, 0, q.aux)
                  : pred_cmp_fast(p.pc, pv[i]);
    if (NULLS) ok = ok & ((nm & p.null_m) == 0);
    pass = pass & ok;
  }
  *matched += pass ? 1 : 0;
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    if (g >= q.num_aggs) continue;
    const SnapAgg& a = q.aggs[g];
    bool contrib = pass;
    if (NULLS) contrib = contrib & ((nm & a.null_m) == 0);
    if (contrib) combine_datum(a.op, &agg_val[g], &agg_cnt[g], av[g]);
  }
}

// ---------------------------------------------------------------------------
// Host-side: ABI query -> SnapQuery. Returns 0, or 9 with a message naming
// the offending predicate / aggregate (nothing may be launched then).
// cols == nullptr validates only (column pointers left null). IN / IN_RANGE
// lists are appended to *aux; the caller uploads it and sets out->aux.
// ---------------------------------------------------------------------------
inline int snap_build_query(const ybg_schema_t& sc, const SnapCols* cols,
                            int32_t num_preds, const ybg_pred_t* preds,
                            int32_t num_aggs, const ybg_agg_t* aggs,
                            uint64_t n_rows, std::vector<uint8_t>* aux,
                            SnapQuery* out, char* err, size_t err_cap) {
  memset(out, 0, sizeof(*out));
  const int nk = sc.num_hash_cols + sc.num_range_cols;
  if (num_preds < 0 || num_preds > YBG_MAX_PREDS) {
    snprintf(err, err_cap, "snapshot query: num_preds %d over the cap %d",
             num_preds, YBG_MAX_PREDS);
    return 9;
  }
  if (num_aggs < 0 || num_aggs > YBG_MAX_AGGS) {
    snprintf(err, err_cap, "snapshot query: num_aggs %d over the cap %d",
             num_aggs, YBG_MAX_AGGS);
    return 9;
  }
  out->n_rows = n_rows;
  out->num_preds = num_preds;
  out->num_aggs = num_aggs;
  if (cols) out->nullmask = cols->nullmask;
  const uint32_t nullable = cols ? cols->nullable_cols : 0xffffffffu;
  for (int i = 0; i < num_preds; ++i) {
    const ybg_pred_t& p = preds[i];
    SnapPred& sp = out->preds[i];
    if (p.op == YBG_PRED_IN_TUPLE) {
      snprintf(err, err_cap,
               "snapshot query: predicate %d: IN_TUPLE is not supported", i);
      return 9;
    }
    if (p.op < YBG_PRED_GT || p.op > YBG_PRED_IN_RANGE) {
      snprintf(err, err_cap, "snapshot query: predicate %d: unknown op %d",
               i, p.op);
      return 9;
    }
    int dt;
    if (p.is_key_col) {
      if (p.col < 0 || p.col >= nk) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: key column %d out of range",
                 i, p.col);
        return 9;
      }
      if (sc.key_types[p.col] == YBG_KT_STRING) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: string key column %d is not "
                 "staged", i, p.col);
        return 9;
      }
      dt = YBG_T_INT64;  // key datums are sign-extended (key_col_value)
      if (cols) sp.col = cols->key[p.col];
      sp.null_m = 0;
    } else {
      if (p.col < 0 || p.col >= sc.num_value_cols) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: value column %d out of range",
                 i, p.col);
        return 9;
      }
      dt = sc.value_cols[p.col].dtype;
      if (dt == YBG_T_STRING) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: string column %d is not "
                 "staged", i, p.col);
        return 9;
      }
      if (cols) sp.col = cols->val[p.col];
      sp.null_m = 1u << p.col;
      if (nullable & sp.null_m) out->any_nullable = 1;
    }
    sp.pc.opdt = (uint32_t)p.op | ((uint32_t)dt << 8);
    sp.pc.datum = p.datum;
    if (p.op == YBG_PRED_IN || p.op == YBG_PRED_IN_RANGE) {
      const uint64_t rec = p.op == YBG_PRED_IN ? 8 : 24;
      if (!p.bytes || p.bytes_len % rec ||
          (p.op == YBG_PRED_IN_RANGE && p.bytes_len == 0) ||
          p.bytes_len / rec > 0xffffffffull) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: malformed option list", i);
        return 9;
      }
      uint64_t off = aux->size();
      if (off + p.bytes_len > 0xffffffffull) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: option lists too large", i);
        return 9;
      }
      aux->insert(aux->end(), p.bytes, p.bytes + p.bytes_len);
      sp.pc.datum = ((p.bytes_len / rec) << 32) | off;
      out->general = 1;
    }
  }
  for (int g = 0; g < num_aggs; ++g) {
    const ybg_agg_t& a = aggs[g];
    SnapAgg& sa = out->aggs[g];
    if (a.op < YBG_AGG_COUNT || a.op > YBG_AGG_MAX_DOUBLE) {
      snprintf(err, err_cap, "snapshot query: aggregate %d: unknown op %d",
               g, a.op);
      return 9;
    }
    sa.op = a.op;
    if (a.op == YBG_AGG_COUNT_STAR) continue;  // no operand
    if (a.col < 0 || a.col >= sc.num_value_cols) {
      snprintf(err, err_cap,
               "snapshot query: aggregate %d: value column %d out of range",
               g, a.col);
      return 9;
    }
    if (sc.value_cols[a.col].dtype == YBG_T_STRING) {
      snprintf(err, err_cap,
               "snapshot query: aggregate %d: string column %d is not staged",
               g, a.col);
      return 9;
    }
    sa.null_m = 1u << a.col;
    if (nullable & sa.null_m) out->any_nullable = 1;
    // COUNT(col) needs the null bit only, never the datum
    if (cols && a.op != YBG_AGG_COUNT) sa.col = cols->val[a.col];
  }
  // windowed-load tail slack for the option lists (load_u64_una)
  aux->insert(aux->end(), 16, 0);
  return 0;
}

// Final result record of a query (k_snap_reduce output / simulator fold).
struct SnapResult {
  uint64_t matched;
  uint64_t agg_val[YBG_MAX_AGGS];
  uint64_t agg_cnt[YBG_MAX_AGGS];
};

// SnapResult + the build's scan statistics -> ABI result struct (same
// conversions as yb_gpu_scan_aggregate).
inline void snap_fill_result(const SnapResult& r, uint64_t n_rows,
                             uint64_t entries_seen, const uint8_t* restart_ht,
                             uint32_t restart_len, int32_t num_aggs,
                             const ybg_agg_t* aggs, ybg_scan_result_t* out) {
  memset(out, 0, sizeof(*out));
  out->rows_scanned = n_rows;
  out->rows_matched = r.matched;
  out->entries_seen = entries_seen;
  if (restart_len > YBG_MAX_HT) restart_len = YBG_MAX_HT;
  memcpy(out->restart_ht, restart_ht, restart_len);
  out->restart_ht_len = restart_len;
  for (int g = 0; g < num_aggs; ++g) {
    ybg_agg_result_t& a = out->aggs[g];
    a.is_null = (r.agg_cnt[g] == 0);
    switch (aggs[g].op) {
      case YBG_AGG_SUM_DOUBLE:
      case YBG_AGG_MIN_DOUBLE:
      case YBG_AGG_MAX_DOUBLE: {
        double dd;
        memcpy(&dd, &r.agg_val[g], 8);
        a.value_f64 = dd;
        break;
      }
      default:
        a.value_i64 = (int64_t)r.agg_val[g];
        break;
    }
  }
}

}  // namespace ybgdev

#endif  // YBG_SNAP_DEVICE_H
