// yugabyte-db_amd/csrc/snap_device.h — columnar-snapshot query logic: the
// per-row predicate/aggregate evaluation over dense per-column arrays, the
// grouped query's accumulate / flush / export, the select's per-tile bit
// packing / rank / output index / emit, the ordered select's key image /
// digit / selection state / gather / emit, and the host-side translation of
// an ABI query into the POD kernel argument.
// Compiled into the HIP query kernels (snap_gpu.hip) AND the host simulator
// (scan_host_sim.cc), with the same DEV macro convention as scan_device.h.
//
// A snapshot is a DIFFERENT storage contract from "scan the reference's
// SST block bytes" (DESIGN.md §4): rows visible at one read time, staged
// once as one 8-byte datum per row per numeric column (the emit_row /
// pred_cmp_fast bit pattern) plus one null-mask word per row. A snapshot
// built with stage_strings also holds every string column as an offsets
// array, a byte heap and an 8-byte prefix column (SnapStrCol).
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

// One staged string column, in snapshot row order; every array is a pure
// function of the rows.
//   off[n_rows + 1]: byte offsets into `bytes`; row r's string is
//     bytes[off[r], off[r + 1]). A NULL has length 0 (the null mask tells it
//     from the empty string).
//   bytes[off[n_rows] + 16]: the strings back to back, then 16 zero bytes.
//   pfx[padded rows]: the string's first min(len, 8) bytes, big-endian (byte
//     0 most significant), zero padded; 0 for a NULL. Padded and tail-zeroed
//     like a numeric column, so a predicate streams it with the same 16-byte
//     row-pair load.
struct SnapStrCol {
  const uint64_t* off;  // nullptr: column not staged
  const uint8_t* bytes;
  const uint64_t* pfx;
};

// Heap side of a string predicate slot (the slot's `col` is the pfx array).
// The record lives in the query's aux buffer, 8-byte aligned, at the offset
// the slot's pc.pad_ holds: SnapQuery keeps the layout the numeric-only
// kernels were compiled against.
struct SnapStrRef {
  const uint64_t* off;
  const uint8_t* bytes;
  uint64_t rhs_pfx;  // compares: the rhs's padded prefix, computed on the host
};

// The query kernel's argument (POD, passed by value).
struct SnapQuery {
  uint64_t n_rows;
  int32_t num_preds, num_aggs;
  SnapPred preds[YBG_MAX_PREDS];
  SnapAgg aggs[YBG_MAX_AGGS];
  const uint32_t* nullmask;  // [padded rows]
  const uint8_t* aux;        // IN / IN_RANGE lists, string rhs bytes
  int32_t any_nullable;      // some referenced column holds a NULL
  int32_t general;           // kSnapGenFast / List / Str: the compare code
                             // the predicates need
};

// Staged column table of one snapshot (device pointers; host pointers in
// the simulator).
struct SnapCols {
  const uint64_t* val[YBG_MAX_COLS];
  const uint64_t* key[YBG_MAX_KEYCOLS];
  const uint32_t* nullmask;
  uint32_t nullable_cols;  // bit i: value col i has >= 1 NULL
  SnapStrCol sval[YBG_MAX_COLS];    // staged string value / key columns
  SnapStrCol skey[YBG_MAX_KEYCOLS];
};

// Padded prefix of a string (SnapStrCol.pfx).
YBG_HD uint64_t snap_str_prefix(const uint8_t* s, uint64_t len) {
  uint64_t p = 0;
  for (uint64_t k = 0; k < 8; ++k)
    p = (p << 8) | (k < len ? (uint64_t)s[k] : 0ull);
  return p;
}

// A string predicate on row `row` of slot i; pfx: the row's prefix datum.
//
// Compares. memcmp order of two strings a, b is decided by their padded
// prefixes P(a), P(b) whenever these differ, by a plain unsigned 64-bit
// compare. Let k < 8 be the first byte where P(a) and P(b) differ. If
// k < min(len a, len b), byte k is real in both strings and all earlier
// bytes are equal, so memcmp decides on the same byte the same way. Otherwise
// one string, say a, ends at or before k (both cannot: two pad bytes are
// both 0 and would not differ). Bytes [0, k) are equal, and there a's pad
// zeros face real zero bytes of b, so a is a proper prefix of b[0, k] and
// memcmp puts a first; P(a)[k] is pad 0 and P(b)[k] differs from it, hence
// is larger, so P(a) < P(b) as well. Equal prefixes decide nothing ("a" vs
// "a\0"): only that tie reads the heap, through pred_compare's string
// branch, so both paths keep one definition of the order.
// IN always reads the heap (pred_compare's string-list branch).
DEV bool snap_str_pred(const SnapQuery& q, int i, uint64_t pfx,
                       uint64_t row) {
  const PredC& pc = q.preds[i].pc;
  const SnapStrRef& s = *reinterpret_cast<const SnapStrRef*>(q.aux + pc.pad_);
#ifndef YBG_SNAP_STR_HEAP_ONLY  // measurement build: every compare is a tie
  const uint32_t op = pc.opdt & 0xff;
  if (op != YBG_PRED_IN && pfx != s.rhs_pfx) {
    const bool lt = pfx < s.rhs_pfx;
    switch (op) {
      case YBG_PRED_GT: case YBG_PRED_GE: return !lt;
      case YBG_PRED_LT: case YBG_PRED_LE: return lt;
      case YBG_PRED_EQ: return false;
      default: return true;
    }
  }
#endif
  const uint64_t o0 = s.off[row], o1 = s.off[row + 1];
  return pred_compare(pc, 0, s.bytes + o0, (uint32_t)(o1 - o0), q.aux);
}

// Compare code of a kernel instantiation (template parameter GEN, picked
// from SnapQuery.general): typed GT..NE compares only; + IN / IN_RANGE lists
// through pred_compare; + string slots. The string branch has an
// instantiation of its own so that numeric list queries run the code they
// ran before it existed.
constexpr int kSnapGenFast = 0, kSnapGenList = 1, kSnapGenStr = 2;

// The predicate fold of one row, shared by the plain, grouped and select
// paths: branch-free AND of every predicate slot below num_preds. row: the
// row's snapshot position, used by string slots (kSnapGenStr only) for the
// heap access; a row that is not `valid` never reaches the heap (its
// position may lie past the offsets array).
template <int NP, bool NULLS, int GEN>
DEV bool snap_pred_pass(const SnapQuery& q, const uint64_t* pv, uint32_t nm,
                        bool valid, uint64_t row) {
  bool pass = valid;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i >= q.num_preds) continue;
    const SnapPred& p = q.preds[i];
    bool ok;
    if constexpr (GEN == kSnapGenStr) {
      if ((p.pc.opdt >> 8) == YBG_T_STRING)
        ok = valid && snap_str_pred(q, i, pv[i], row);
      else
        ok = pred_compare(p.pc, pv[i], nullptr, 0, q.aux);
    } else if constexpr (GEN == kSnapGenList) {
      ok = pred_compare(p.pc, pv[i], nullptr, 0, q.aux);
    } else {
      ok = pred_cmp_fast(p.pc, pv[i]);
    }
    if (NULLS) ok = ok & ((nm & p.null_m) == 0);
    pass = pass & ok;
  }
  return pass;
}

// One row. pv/av: the row's predicate / aggregate operand datums (slot i of
// the query), nm: its null mask (ignored unless NULLS), valid: the row
// exists (false for the padding row of an odd tail). NULL semantics are the
// scan path's (eval_col / acc_row): a predicate on NULL fails; COUNT(col),
// SUM, MIN, MAX skip NULL operands.
template <int NP, int NA, bool NULLS, int GEN>
DEV void snap_row(const SnapQuery& q, const uint64_t* pv, const uint64_t* av,
                  uint32_t nm, bool valid, uint64_t row, uint64_t* matched,
                  uint64_t* agg_val, uint64_t* agg_cnt) {
  const bool pass = snap_pred_pass<NP, NULLS, GEN>(q, pv, nm, valid, row);
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
// GROUP BY on a snapshot. Every passing row is accumulated into a group
// table with order-independent integer atomics (add / min / max / or; double
// SUM as 128-bit 2^-60 fixed point), so the exported groups are bit-identical
// whatever the arrival order and whichever of the two levels ran:
//   LOCAL: a workgroup-local open-addressing table (LDS on the device, a
//     heap array in the simulator) absorbs the rows; a row whose group finds
//     no slot within kSnapLocalProbes probes goes straight to the global
//     table; after the row loop the workgroup flushes every occupied local
//     slot with ONE find-or-insert plus one set of atomics.
//   global-only: every row goes to the global table (group_accum_from).
// ---------------------------------------------------------------------------

// Workgroup-scope accesses of the local table's claim protocol (agent scope
// would write the L2 back on every release).
#ifdef YBG_HOST_SIM
static inline unsigned ybg_wg_load_u32(unsigned* p) { return *p; }
static inline unsigned long long ybg_wg_load_u64(unsigned long long* p) {
  return *p;
}
static inline void ybg_wg_store_u64(unsigned long long* p,
                                    unsigned long long v) {
  *p = v;
}
static inline void ybg_wg_store_rel_u32(unsigned* p, unsigned v) { *p = v; }
#else
__device__ __forceinline__ unsigned ybg_wg_load_u32(unsigned* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ unsigned long long ybg_wg_load_u64(
    unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ybg_wg_store_u64(unsigned long long* p,
                                                 unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ybg_wg_store_rel_u32(unsigned* p,
                                                     unsigned v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#endif

// Aggregate cap (2 / 4 / 8) of the kernel instantiation a query selects.
YBG_HD int snap_group_na(int32_t num_aggs) {
  return num_aggs <= 2 ? 2 : (num_aggs <= 4 ? 4 : 8);
}
// Local-table slot count per aggregate cap: the widest power of two that
// keeps the table (SnapLocalTable<NA>, 16 + 24 * NA bytes per slot) under
// the 40 KiB that leave 4 workgroups per CU resident (kSnapMaxGrid).
constexpr int snap_group_local_slots(int na_cap) {
  return na_cap <= 2 ? 512 : (na_cap <= 4 ? 256 : 128);
}
// probes a row spends on the local table before it spills to the global one
constexpr int kSnapLocalProbes = 4;
// iterations of one local lookup, waits on a slot being claimed included
constexpr int kSnapLocalIters = 64;

// Global group-table capacity: smallest power of two >= 2 * n_rows, clamped
// to [1024, 2^20].
YBG_HD uint64_t snap_group_table_cap(uint64_t n_rows) {
  uint64_t cap = 1024;
  while (cap < 2 * n_rows && cap < (1ull << 20)) cap <<= 1;
  return cap;
}

// Workgroup-local group table. Slot L is the NULL-key group. state[]:
// 0 empty / 2 claiming / 1 ready, as in GroupCtx. poison[]: bit g = the
// slot's double SUM of aggregate g met a value outside the fixed-point range.
template <int NA>
struct SnapLocalTable {
  static constexpr int L = snap_group_local_slots(NA);
  unsigned long long key[L + 1];
  unsigned long long val[(L + 1) * NA];  // low word of a double SUM
  unsigned long long hi[(L + 1) * NA];   // its high word
  unsigned long long cnt[(L + 1) * NA];
  unsigned state[L + 1];
  unsigned poison[L + 1];
};

// The grouped query kernel's argument (POD, passed by value).
struct SnapGroupQuery {
  SnapQuery q;
  const uint64_t* grp_col;  // staged group column
  uint32_t grp_null_m;      // its null-mask bit (0: never NULL)
  uint32_t pad_;
};

// One passing row, with group_accum_from's field names.
struct SnapGroupRow {
  uint64_t grp_datum;
  uint64_t agg_datum[YBG_MAX_AGGS];
  uint32_t grp_len;   // 0: numeric group key
  uint32_t agg_null;  // bit g: operand of aggregate g is NULL
  uint32_t grp_null;
};

struct SnapOps {
  int32_t num_aggs;
  int32_t op[YBG_MAX_AGGS];
};

// Slots [first, L] in steps of `step` back to empty (device: first =
// threadIdx.x, step = blockDim.x, followed by a barrier).
template <int NA>
DEV void snap_local_init(const SnapQuery& q, SnapLocalTable<NA>* t,
                         int first, int step) {
  for (int i = first; i <= SnapLocalTable<NA>::L; i += step) {
    t->key[i] = 0;
    t->state[i] = 0;
    t->poison[i] = 0;
#pragma unroll
    for (int g = 0; g < NA; ++g) {
      t->val[i * NA + g] = (unsigned long long)group_init_value(
          g < q.num_aggs ? q.aggs[g].op : 0);
      t->hi[i * NA + g] = 0;
      t->cnt[i * NA + g] = 0;
    }
  }
}

// Local slot of a non-NULL group key, or -1: no slot within
// kSnapLocalProbes probes (the row then goes to the global table). As in
// grp_find_or_insert, an iteration completes before a slot that is being
// claimed is looked at again, so divergent lanes reconverge; the loop is
// bounded either way.
template <int NA>
DEV int snap_local_find_or_insert(SnapLocalTable<NA>* t, uint64_t kv) {
  constexpr unsigned mask = SnapLocalTable<NA>::L - 1;
  const unsigned h = (unsigned)grp_mix(kv);
  int probe = 0;
  for (int it = 0; probe < kSnapLocalProbes && it < kSnapLocalIters; ++it) {
    const unsigned i = (h + (unsigned)probe) & mask;
    unsigned st = ybg_wg_load_u32(&t->state[i]);
    if (st == 0) {
      st = atomicCAS(&t->state[i], 0u, 2u);
      if (st == 0) {
        ybg_wg_store_u64(&t->key[i], kv);
        ybg_wg_store_rel_u32(&t->state[i], 1u);
        return (int)i;
      }
    }
    if (st == 1) {
      if (ybg_wg_load_u64(&t->key[i]) == kv) return (int)i;
      ++probe;
    }
    // st == 2: another lane is publishing this slot; retry the same probe
  }
  return -1;
}

// Accumulate one passing row: local table first, global table on a miss.
template <int NA>
DEV void snap_local_accum(const SnapQuery& q, SnapLocalTable<NA>* t,
                          const GroupCtx& gc, const SnapGroupRow& r) {
  int slot;
  if (r.grp_null) {
    slot = SnapLocalTable<NA>::L;
    if (ybg_wg_load_u32(&t->state[slot]) != 1)
      ybg_wg_store_rel_u32(&t->state[slot], 1u);
  } else {
    slot = snap_local_find_or_insert<NA>(t, r.grp_datum);
    if (slot < 0) {
      group_accum_from<NA>(q, gc, r);
      return;
    }
  }
  unsigned long long* v = t->val + slot * NA;
  unsigned long long* c = t->cnt + slot * NA;
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    if (g >= q.num_aggs) continue;
    const int op = q.aggs[g].op;
    if (op != YBG_AGG_COUNT_STAR && ((r.agg_null >> g) & 1)) continue;
    const uint64_t d = r.agg_datum[g];
    switch (op) {
      case YBG_AGG_COUNT_STAR:
      case YBG_AGG_COUNT:
        atomicAdd(&v[g], 1ull);
        break;
      case YBG_AGG_SUM_INT64:
        atomicAdd(&v[g], d);
        break;
      case YBG_AGG_SUM_DOUBLE: {
        unsigned long long lo, hi;
        if (f64_to_fixed128(d, &lo, &hi))
          add_fixed128(&v[g], &t->hi[slot * NA + g], lo, hi);
        else
          ybg_atomic_or_u32(&t->poison[slot], 1u << g);
        break;
      }
      case YBG_AGG_MIN_INT64:
        ybg_atomic_min_i64((long long*)&v[g], (long long)d);
        break;
      case YBG_AGG_MAX_INT64:
        ybg_atomic_max_i64((long long*)&v[g], (long long)d);
        break;
      case YBG_AGG_MIN_DOUBLE:
        ybg_atomic_min_u64(&v[g], f64_ordered(d));
        break;
      case YBG_AGG_MAX_DOUBLE:
        ybg_atomic_max_u64(&v[g], f64_ordered(d));
        break;
      default:
        break;
    }
    // COUNT ops: cnt = val at export, as in the global table
    if (op != YBG_AGG_COUNT_STAR && op != YBG_AGG_COUNT)
      atomicAdd(&c[g], 1ull);
  }
}

// Fold local slot i (0..L) into the global table: one find-or-insert, then
// one atomic per aggregate word that holds a contribution. Runs after the
// workgroup's rows are all in (device: behind a barrier).
template <int NA>
DEV void snap_local_flush_slot(const SnapQuery& q, SnapLocalTable<NA>* t,
                               int i, const GroupCtx& gc) {
  if (t->state[i] != 1) return;
  uint64_t slot;
  if (i == SnapLocalTable<NA>::L) {
    slot = gc.cap;  // the NULL-key group
    if (ybg_atomic_load_u32(&gc.state[slot]) != 1)
      ybg_atomic_store_rel_u32(&gc.state[slot], 1u);
  } else {
    slot = grp_find_or_insert(gc, t->key[i], false);
    if (slot == ~0ull) {
      atomicAdd(gc.overflow, 1ull);
      return;
    }
  }
  long long* v = gc.vals + slot * YBG_MAX_AGGS;
  unsigned long long* c = gc.cnts + slot * YBG_MAX_AGGS;
  const unsigned poison = t->poison[i];
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    if (g >= q.num_aggs) continue;
    const int op = q.aggs[g].op;
    const unsigned long long lv = t->val[i * NA + g];
    const unsigned long long lc = t->cnt[i * NA + g];
    switch (op) {
      case YBG_AGG_COUNT_STAR:
      case YBG_AGG_COUNT:
        if (lv) atomicAdd((unsigned long long*)&v[g], lv);
        break;
      case YBG_AGG_SUM_INT64:
        if (lc) atomicAdd((unsigned long long*)&v[g], lv);
        break;
      case YBG_AGG_SUM_DOUBLE:
        if ((poison >> g) & 1)
          ybg_atomic_or_u32(&gc.poison[slot * YBG_MAX_AGGS + g], 1u);
        if (lv | t->hi[i * NA + g])
          group_add_fixed128(gc, slot, g, lv, t->hi[i * NA + g]);
        break;
      case YBG_AGG_MIN_INT64:
        if (lc) ybg_atomic_min_i64(&v[g], (long long)lv);
        break;
      case YBG_AGG_MAX_INT64:
        if (lc) ybg_atomic_max_i64(&v[g], (long long)lv);
        break;
      case YBG_AGG_MIN_DOUBLE:
        if (lc) ybg_atomic_min_u64((unsigned long long*)&v[g], lv);
        break;
      case YBG_AGG_MAX_DOUBLE:
        if (lc) ybg_atomic_max_u64((unsigned long long*)&v[g], lv);
        break;
      default:
        break;
    }
    if (lc) atomicAdd(&c[g], lc);
  }
}

// One row of the grouped query: snap_row's predicate fold, then the row's
// group datum / aggregate operands into `tab` (LOCAL) or the global table.
// gv: the row's group-column datum.
template <int NP, int NA, bool NULLS, int GEN, bool LOCAL>
DEV void snap_group_row(const SnapGroupQuery& gq, const uint64_t* pv,
                        const uint64_t* av, uint64_t gv, uint32_t nm,
                        bool valid, uint64_t row, uint64_t* matched,
                        SnapLocalTable<NA>* tab, const GroupCtx& gc) {
  const SnapQuery& q = gq.q;
  if (!snap_pred_pass<NP, NULLS, GEN>(q, pv, nm, valid, row)) return;
  *matched += 1;
  SnapGroupRow r;
  r.grp_datum = gv;
  r.grp_len = 0;
  r.grp_null = NULLS ? ((nm & gq.grp_null_m) != 0) : 0;
  r.agg_null = 0;
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    r.agg_datum[g] = av[g];
    if (NULLS && g < q.num_aggs && (nm & q.aggs[g].null_m))
      r.agg_null |= 1u << g;
  }
  if (LOCAL)
    snap_local_accum<NA>(q, tab, gc, r);
  else
    group_accum_from<NA>(q, gc, r);
}

// Export of global-table slot `slot` as output entry `idx`: decoded values
// and the COUNT cnt = val rule, all YBG_MAX_AGGS columns written (zero past
// num_aggs) so the output bytes are a pure function of the groups.
DEV void snap_group_export_slot(const SnapOps& ops, const GroupCtx& gc,
                                uint64_t slot, uint64_t key, uint64_t idx,
                                uint64_t* keys, long long* vals,
                                unsigned long long* cnts) {
  keys[idx] = key;
  for (int g = 0; g < YBG_MAX_AGGS; ++g) {
    long long v = 0;
    unsigned long long c = 0;
    if (g < ops.num_aggs) {
      const int op = ops.op[g];
      v = group_export_value(op, gc.vals[slot * YBG_MAX_AGGS + g],
                             gc.vals_hi[slot * YBG_MAX_AGGS + g],
                             gc.poison[slot * YBG_MAX_AGGS + g]);
      c = (op == YBG_AGG_COUNT_STAR || op == YBG_AGG_COUNT)
              ? (unsigned long long)v
              : gc.cnts[slot * YBG_MAX_AGGS + g];
    }
    vals[idx * YBG_MAX_AGGS + g] = v;
    cnts[idx * YBG_MAX_AGGS + g] = c;
  }
}

// ---------------------------------------------------------------------------
// SELECT on a snapshot: an order-preserving stream compaction in three
// launches, no workgroup ever waiting on another.
//   count:  workgroup-sized contiguous TILES of kSnapTileRows positions; the
//     predicate fold of every row becomes one bit of the tile's match bitmap
//     (bit b of word w of the tile = position tile * kSnapTileRows + 64 * w
//     + b); each wave writes its 128 rows' match count into its own 16-bit
//     lane of the tile's tile_cnt[] word, so no wave waits for another.
//   scan:   one workgroup, exclusive prefix sum of the tile counts in tile order
//     -> tile_off[], the total, and the delivered rank range [first, end)
//     implied by limit and direction (snap_select_range).
//   gather: per tile, rank of a match = tile_off + set bits below it in the
//     tile; ranks inside [first, end) are written to output index
//     rank - first (forward) or end - 1 - rank (backward).
// The tile arrays are indexed relative to the window's first tile; the
// bitmap by absolute position.
// ---------------------------------------------------------------------------
constexpr uint64_t kSnapTileRows = (uint64_t)kSnapThreads * kSnapVec;  // 512
constexpr int kSnapTileWords = (int)(kSnapTileRows / 64);              // 8
constexpr int kSnapScanThreads = 1024;
constexpr int kSnapScanVec = 4;  // tile counts per scan thread per round
static_assert(kSnapThreads / 64 == 4, "tile_cnt packs four 16-bit counts");

// The window of one select: positions [lo, hi), hi <= n_rows, lo < hi.
struct SnapWindow {
  uint64_t lo, hi;
  uint64_t tile_lo;  // lo / kSnapTileRows
  uint64_t n_tiles;  // tiles that intersect the window
};

YBG_HD SnapWindow snap_select_window(uint64_t lo, uint64_t hi) {
  SnapWindow w;
  w.lo = lo;
  w.hi = hi;
  w.tile_lo = lo / kSnapTileRows;
  w.n_tiles = (hi + kSnapTileRows - 1) / kSnapTileRows - w.tile_lo;
  return w;
}

// tile_cnt / tile_off length: whole scan-thread vectors
YBG_HD uint64_t snap_select_tile_slots(uint64_t n_tiles) {
  return (n_tiles + kSnapScanVec - 1) / kSnapScanVec * kSnapScanVec;
}

// Matches of a tile from its tile_cnt word (one 16-bit count per wave).
YBG_HD uint32_t snap_select_tile_count(uint64_t w) {
  return (uint32_t)((w & 0xffff) + ((w >> 16) & 0xffff) +
                    ((w >> 32) & 0xffff) + (w >> 48));
}

// Scan output: matches in the window and the delivered rank range.
struct SnapSelectHdr {
  uint64_t total, first, end;
};

// Delivered ranks of `total` matches: forward the first `limit`, backward
// the last `limit` (0 = unlimited).
YBG_HD void snap_select_range(uint64_t total, uint64_t limit, int backward,
                              SnapSelectHdr* h) {
  const uint64_t n = (limit && limit < total) ? limit : total;
  h->total = total;
  h->first = backward ? total - n : 0;
  h->end = backward ? total : n;
}

// Even bits of the result = the low 32 bits of x.
YBG_HD uint64_t snap_spread32(uint64_t x) {
  x &= 0xffffffffull;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// Bit packing of one wave: b0 / b1 are the ballots of the lanes' first /
// second row (lane l owns rows 2l and 2l + 1 of the wave's 128), w[0..1]
// the same 128 pass bits in position order.
YBG_HD void snap_select_pack(uint64_t b0, uint64_t b1, uint64_t* w) {
  w[0] = snap_spread32(b0) | (snap_spread32(b1) << 1);
  w[1] = snap_spread32(b0 >> 32) | (snap_spread32(b1 >> 32) << 1);
}

YBG_HD int snap_popc64(uint64_t x) {
#ifdef YBG_HOST_SIM
  return __builtin_popcountll(x);
#else
  return __popcll(x);
#endif
}

// Set bits of the tile's bitmap words below bit `b` (0 .. kSnapTileRows - 1).
YBG_HD uint32_t snap_select_rank(const uint64_t* words, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int w = 0; w < kSnapTileWords; ++w) {
    const uint32_t lo = (uint32_t)w * 64;
    uint64_t m = words[w];
    if (b < lo + 64) m = b > lo ? m & ((1ull << (b - lo)) - 1) : 0;
    r += (uint32_t)snap_popc64(m);
  }
  return r;
}

// Output index of match number `rank`; false: outside the delivered range.
YBG_HD bool snap_select_out_index(const SnapSelectHdr& h, int backward,
                                  uint64_t rank, uint64_t* idx) {
  if (rank < h.first || rank >= h.end) return false;
  *idx = backward ? h.end - 1 - rank : rank - h.first;
  return true;
}

struct SnapSelCol {
  const uint64_t* col;  // staged column array; string column: its off array
  uint32_t null_m;      // null-mask bit of a value column, 0 for a key column
  uint32_t is_str;      // 1: string column (select_var)
};

// The gather kernel's argument (POD, passed by value).
struct SnapSelect {
  int32_t num_cols;
  int32_t backward;
  SnapSelCol cols[YBG_MAX_SELECT_COLS];
  const uint32_t* nullmask;  // nullptr: no projected column holds a NULL
  uint32_t proj_mask;        // null-mask bits of the projected value columns
  uint32_t num_str;          // projected string columns (repeats counted)
  const uint8_t* str_bytes[YBG_MAX_SELECT_COLS];  // heap of string column j
};

struct SnapSelectOut {
  uint64_t* row_ids;     // [cap]
  uint32_t* null_masks;  // [cap]
  uint64_t* datums;      // [num_cols * cap], column-major
  uint64_t cap;
};

// One delivered row: position `pos` to output index `idx`. The null word is
// masked to the projected value columns and a NULL's datum is written as 0.
// A string column's datum is its length << 40 here; snap_select_strcopy_row
// ORs the heap offset in.
DEV void snap_select_emit(const SnapSelect& s, const SnapSelectOut& o,
                          uint64_t pos, uint64_t idx) {
  const uint32_t nm = s.nullmask ? (s.nullmask[pos] & s.proj_mask) : 0u;
  o.row_ids[idx] = pos;
  o.null_masks[idx] = nm;
  for (int j = 0; j < s.num_cols; ++j) {
    const SnapSelCol& c = s.cols[j];
    uint64_t v = c.col[pos];
    if (c.is_str) v = (c.col[pos + 1] - v) << 40;
    o.datums[(uint64_t)j * o.cap + idx] = (nm & c.null_m) ? 0 : v;
  }
}

// select_var, after the gather. The output heap is canonical: delivered rows
// in delivery order, within a row the projected string columns in projection
// order, bytes back to back.
// Bytes delivered row `idx` puts on the heap.
DEV uint64_t snap_select_row_strlen(const SnapSelect& s,
                                    const SnapSelectOut& o, uint64_t idx) {
  uint64_t t = 0;
  for (int j = 0; j < s.num_cols; ++j)
    if (s.cols[j].is_str) t += o.datums[(uint64_t)j * o.cap + idx] >> 40;
  return t;
}

// Copy delivered row idx's strings to heap + row_off and complete their
// datums to (len << 40) | offset (ybg_row_batch_t convention). A NULL keeps
// datum 0 and takes no bytes.
DEV void snap_select_strcopy_row(const SnapSelect& s, const SnapSelectOut& o,
                                 uint64_t idx, uint64_t row_off,
                                 uint8_t* heap) {
  const uint64_t pos = o.row_ids[idx];
  const uint32_t nm = o.null_masks[idx];
  uint64_t at = row_off;
  for (int j = 0; j < s.num_cols; ++j) {
    const SnapSelCol& c = s.cols[j];
    if (!c.is_str || (nm & c.null_m)) continue;
    uint64_t* d = &o.datums[(uint64_t)j * o.cap + idx];
    const uint64_t len = *d >> 40;
    const uint8_t* src = s.str_bytes[j] + c.col[pos];
    for (uint64_t k = 0; k < len; ++k) heap[at + k] = src[k];
    *d |= at;
    at += len;
  }
}

// The two rows of one gather lane: bits b and b + 1 of tile `tile` (absolute
// index), `words` being the tile's bitmap, `off` its exclusive match offset.
DEV void snap_select_gather_pair(const SnapSelect& s, const SnapSelectOut& o,
                                 const SnapSelectHdr& h,
                                 const uint64_t* words, uint64_t tile,
                                 uint64_t off, uint32_t b) {
  // constant-indexed select, so `words` stays in registers
  uint64_t w = 0;
#pragma unroll
  for (int i = 0; i < kSnapTileWords; ++i)
    if ((b >> 6) == (uint32_t)i) w = words[i];
  const uint32_t two = (uint32_t)(w >> (b & 63)) & 3u;
  if (!two) return;
  uint64_t rank = off + snap_select_rank(words, b);
  uint64_t idx;
  if (two & 1u) {
    if (snap_select_out_index(h, s.backward, rank, &idx))
      snap_select_emit(s, o, tile * kSnapTileRows + b, idx);
    ++rank;
  }
  if (two & 2u) {
    if (snap_select_out_index(h, s.backward, rank, &idx))
      snap_select_emit(s, o, tile * kSnapTileRows + b + 1, idx);
  }
}

// ---------------------------------------------------------------------------
// ORDER BY / top-N on a snapshot: a radix select between the select's match
// bitmap and its emit. Every row has a selection key that cannot tie,
//   (NULL class: 1 bit, value image: 64 bits, position: 32 bits),
// compared lexicographically, so "the first n rows of the order" is "the
// rows whose key is <= the n-th smallest key" and no tie ranking exists.
//   hist:  one digit of the key per pass, most significant first: pass 0 is
//     the NULL class plus the image's top byte (9 bits), passes 1..7 the
//     other image bytes, passes 8..11 the position bytes. A pass counts the
//     matched, eligible (after the cursor) rows whose higher digits equal
//     the prefix fixed so far.
//   fix:   one workgroup prefix-sums the bins, fixes the digit that holds
//     the k-th key and writes the SnapOrderState for the next pass and the
//     host.
//   mark:  rows whose key prefix is <= the fixed prefix ("selected") become
//     a second bitmap with the select's per-tile counts; the select's scan
//     turns those into offsets.
//   gather / sort / emit: the selected rows' (image, class | position) pairs
//     in position order, a stable radix sort on the image (and one more bit
//     for the class), snap_select_emit of the first n.
// 8-bit digits: a 256-bin (512 for pass 0) workgroup histogram is 2 KiB of
// LDS, so four workgroups per CU stay resident like every other snapshot
// kernel, the flush is at most 512 global adds per workgroup, and the fix
// kernel is one 512-thread scan. 11-bit digits would save three of the
// twelve passes at full depth, but full depth is the rare case (the
// early-out below usually stops after one or two passes) and the 2048-bin
// flush per workgroup would cost every pass.
// ---------------------------------------------------------------------------
constexpr int kSnapOrderBins = 512;
constexpr int kSnapOrderPasses = 12;
// default early-out threshold (ybg_snapshot_order_candidate_rows)
constexpr uint64_t kSnapOrderCand = 1ull << 20;
constexpr int kSnapOrderInt = 0, kSnapOrderDouble = 1, kSnapOrderFloat = 2;

struct SnapOrderKey {
  uint64_t img;
  uint32_t pos;
  uint32_t cls;
};

// The order kernels' argument (POD, passed by value).
struct SnapOrder {
  const uint64_t* col;       // staged order column
  const uint32_t* nullmask;  // nullptr: the order column holds no NULL
  uint32_t null_m;
  int32_t kind;              // kSnapOrderInt / Double / Float
  int32_t descending, nulls_first, have_cursor;
  uint32_t pad_;
  SnapOrderKey cursor;
};

// Selection state, device resident; written by the fix step only.
struct SnapOrderState {
  SnapOrderKey prefix;  // digits fixed so far, the rest zero
  uint64_t img_mask;    // bits of the key the fixed digits cover
  uint32_t pos_mask;
  uint32_t cls_mask;
  uint64_t k;         // the wanted key is the k-th (1-based) of the bucket
  uint64_t below;     // eligible rows whose prefix is below the fixed one
  uint64_t bucket;    // eligible rows whose prefix equals it
  uint64_t eligible;  // matched rows after the cursor (pass 0's total)
  uint32_t depth;     // digits fixed
  uint32_t pad_;
};

// 64-bit image of an order datum: unsigned order of the images = the value
// order of the contract. Integers flip the sign bit; doubles and floats are
// canonicalised (-0.0 -> +0.0, every NaN -> the quiet NaN above +inf) and
// sign-magnitude -> biased; a float's 32 ordered bits sit in the image's
// high half so the first passes already split them. DESC complements.
YBG_HD uint64_t snap_order_image(int kind, uint64_t datum, int descending) {
  uint64_t img;
  if (kind == kSnapOrderDouble) {
    uint64_t d = datum;
    if ((d & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
      d = 0x7ff8000000000000ull;
    else if (d == 0x8000000000000000ull)
      d = 0;
    img = d ^ ((d >> 63) ? ~0ull : (1ull << 63));
  } else if (kind == kSnapOrderFloat) {
    uint32_t f = (uint32_t)datum;
    if ((f & 0x7fffffffu) > 0x7f800000u)
      f = 0x7fc00000u;
    else if (f == 0x80000000u)
      f = 0;
    img = (uint64_t)(f ^ ((f >> 31) ? 0xffffffffu : 0x80000000u)) << 32;
  } else {
    img = datum ^ (1ull << 63);
  }
  return descending ? ~img : img;
}

// Key of a row (or of the cursor). A NULL's image is 0: NULL rows differ by
// position only.
YBG_HD SnapOrderKey snap_order_key(const SnapOrder& o, uint64_t datum,
                                   bool is_null, uint64_t pos) {
  SnapOrderKey k;
  k.cls = (is_null ? 1u : 0u) ^ (o.nulls_first ? 1u : 0u);
  k.img = is_null ? 0 : snap_order_image(o.kind, datum, o.descending);
  k.pos = (uint32_t)pos;
  return k;
}

YBG_HD bool snap_order_is_null(const SnapOrder& o, uint32_t cls) {
  return (cls ^ (o.nulls_first ? 1u : 0u)) != 0;
}

// a > b
YBG_HD bool snap_order_after(const SnapOrderKey& a, const SnapOrderKey& b) {
  if (a.cls != b.cls) return a.cls > b.cls;
  if (a.img != b.img) return a.img > b.img;
  return a.pos > b.pos;
}

// Key of one row and whether it takes part: matched (its bit of the match
// bitmap) and, with a cursor, strictly after it.
YBG_HD bool snap_order_row(const SnapOrder& o, uint64_t datum, uint32_t nm,
                           uint64_t pos, bool matched, SnapOrderKey* k) {
  *k = snap_order_key(o, datum, (nm & o.null_m) != 0, pos);
  return matched && (!o.have_cursor || snap_order_after(*k, o.cursor));
}

YBG_HD uint32_t snap_order_digit(const SnapOrderKey& k, int pass) {
  if (pass == 0) return (k.cls << 8) | (uint32_t)(k.img >> 56);
  if (pass < 8) return (uint32_t)(k.img >> (56 - 8 * pass)) & 0xffu;
  return (k.pos >> (24 - 8 * (pass - 8))) & 0xffu;
}

// The key's fixed digits equal the prefix.
YBG_HD bool snap_order_in_bucket(const SnapOrderKey& k,
                                 const SnapOrderState& st) {
  return (((k.img ^ st.prefix.img) & st.img_mask) |
          ((k.pos ^ st.prefix.pos) & st.pos_mask) |
          ((k.cls ^ st.prefix.cls) & st.cls_mask)) == 0;
}

// The key's fixed digits are at or below the prefix: the row is delivered or
// still a candidate. With every digit fixed this is "key <= the k-th key".
YBG_HD bool snap_order_selected(const SnapOrderKey& k,
                                const SnapOrderState& st) {
  const uint32_t c = k.cls & st.cls_mask;
  if (c != st.prefix.cls) return c < st.prefix.cls;
  const uint64_t i = k.img & st.img_mask;
  if (i != st.prefix.img) return i < st.prefix.img;
  return (k.pos & st.pos_mask) <= st.prefix.pos;
}

// Fix step of pass `pass`, given the winning digit: `excl` bucket rows lie
// in lower bins, `cnt` in the digit's own (excl < st->k <= excl + cnt).
YBG_HD void snap_order_advance(SnapOrderState* st, int pass, uint32_t digit,
                               uint64_t excl, uint64_t cnt) {
  st->below += excl;
  st->k -= excl;
  st->bucket = cnt;
  if (pass == 0) {
    st->prefix.cls = digit >> 8;
    st->prefix.img = (uint64_t)(digit & 0xffu) << 56;
  } else if (pass < 8) {
    st->prefix.img |= (uint64_t)digit << (56 - 8 * pass);
  } else {
    st->prefix.pos |= digit << (24 - 8 * (pass - 8));
  }
  const int depth = pass + 1;
  st->depth = (uint32_t)depth;
  st->cls_mask = 1u;
  st->img_mask = depth >= 8 ? ~0ull : ~0ull << (64 - 8 * depth);
  st->pos_mask = depth <= 8 ? 0u : ~0u << (32 - 8 * (depth - 8));
}

// Pass 0 learns the eligible count: `total` rows, of which the first
// min(limit, total) are wanted. False: every eligible row is delivered and
// the state stays at depth 0 (everything "selected").
YBG_HD bool snap_order_begin(SnapOrderState* st, uint64_t total,
                             uint64_t limit) {
  st->eligible = total;
  st->bucket = total;
  st->k = (limit && limit < total) ? limit : total;
  return limit && limit < total;
}

// Host: are more digit passes needed after the state the fix step wrote?
// cand: the early-out threshold (< 2: off).
YBG_HD bool snap_order_more(const SnapOrderState& st, uint64_t limit,
                            uint64_t cand) {
  if (!limit || limit >= st.eligible) return false;
  if (st.depth >= (uint32_t)kSnapOrderPasses) return false;
  return !(cand >= 2 && st.bucket <= cand);
}

// The two rows of one gather lane (bits b, b + 1 of `tile`, whose selected
// bitmap is `words` and exclusive offset `off`): their sort records to
// candidate slot = rank, so candidates stand in position order.
//   ckey[rank] = image, cval[rank] = class << 32 | position.
DEV void snap_order_gather_pair(const SnapOrder& o, const uint64_t* words,
                                uint64_t tile, uint64_t off, uint32_t b,
                                uint64_t* ckey, uint64_t* cval) {
  uint64_t w = 0;
#pragma unroll
  for (int i = 0; i < kSnapTileWords; ++i)
    if ((b >> 6) == (uint32_t)i) w = words[i];
  const uint32_t two = (uint32_t)(w >> (b & 63)) & 3u;
  if (!two) return;
  uint64_t rank = off + snap_select_rank(words, b);
#pragma unroll
  for (uint32_t j = 0; j < 2; ++j) {
    if (!((two >> j) & 1u)) continue;
    const uint64_t pos = tile * kSnapTileRows + b + j;
    const uint32_t nm = o.nullmask ? o.nullmask[pos] : 0u;
    const SnapOrderKey k =
        snap_order_key(o, o.col[pos], (nm & o.null_m) != 0, pos);
    ckey[rank] = k.img;
    cval[rank] = ((uint64_t)k.cls << 32) | k.pos;
    ++rank;
  }
}

// The last delivered row, for the next page.
struct SnapOrderCursor {
  uint64_t datum, row;
  uint32_t is_null, pad_;
};

// Delivered row idx of n from its sorted record.
DEV void snap_order_emit(const SnapOrder& o, const SnapSelect& s,
                         const SnapSelectOut& so, uint64_t rec, uint64_t idx,
                         uint64_t n, SnapOrderCursor* cur) {
  const uint64_t pos = rec & 0xffffffffull;
  snap_select_emit(s, so, pos, idx);
  if (idx + 1 == n) {
    const bool nul = snap_order_is_null(o, (uint32_t)(rec >> 32));
    cur->is_null = nul ? 1u : 0u;
    cur->datum = nul ? 0 : o.col[pos];
    cur->row = pos;
    cur->pad_ = 0;
  }
}

// ---------------------------------------------------------------------------
// Host-side: ABI query -> SnapQuery. Returns 0, or 9 with a message naming
// the offending predicate / aggregate (nothing may be launched then).
// cols == nullptr validates only (column pointers left null). IN / IN_RANGE
// lists are appended to *aux; the caller uploads it and sets out->aux.
// ---------------------------------------------------------------------------
// One predicate on a staged string column -> its slot: its SnapStrRef, then
// the rhs bytes (a compare) or the [u32 len][bytes] option records (IN) go
// to *aux, the latter in the block path's PredC form. IN_RANGE is refused.
inline int snap_build_str_pred(const ybg_pred_t& p, const SnapStrCol& str,
                               int i, std::vector<uint8_t>* aux, SnapPred* sp,
                               char* err, size_t err_cap) {
  if (p.op == YBG_PRED_IN_RANGE) {
    snprintf(err, err_cap,
             "snapshot query: predicate %d: IN_RANGE is not supported on a "
             "string column", i);
    return 9;
  }
  aux->resize((aux->size() + 7) / 8 * 8, 0);
  const uint64_t ref_off = aux->size();
  const uint64_t off = ref_off + sizeof(SnapStrRef);
  if ((p.bytes_len && !p.bytes) || p.bytes_len > 0xffffffffull ||
      off + p.bytes_len > 0xffffffffull) {
    snprintf(err, err_cap,
             "snapshot query: predicate %d: malformed string operand", i);
    return 9;
  }
  uint64_t head = p.bytes_len;  // compare: rhs length
  if (p.op == YBG_PRED_IN) {
    uint64_t o = 0, cnt = 0;
    while (o + 4 <= p.bytes_len) {
      uint32_t ol;
      memcpy(&ol, p.bytes + o, 4);
      o += 4 + (uint64_t)ol;
      ++cnt;
    }
    if (o != p.bytes_len) {
      snprintf(err, err_cap,
               "snapshot query: predicate %d: malformed option list", i);
      return 9;
    }
    head = cnt;
  }
  SnapStrRef ref;
  ref.off = str.off;
  ref.bytes = str.bytes;
  ref.rhs_pfx =
      p.op == YBG_PRED_IN ? 0 : snap_str_prefix(p.bytes, p.bytes_len);
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(&ref);
  aux->insert(aux->end(), rb, rb + sizeof(ref));
  if (p.bytes_len) aux->insert(aux->end(), p.bytes, p.bytes + p.bytes_len);
  sp->pc.opdt = (uint32_t)p.op | ((uint32_t)YBG_T_STRING << 8);
  sp->pc.datum = (head << 32) | off;
  sp->pc.pad_ = (uint32_t)ref_off;
  return 0;
}

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
      const SnapStrCol* str = nullptr;
      if (sc.key_types[p.col] == YBG_KT_STRING) {
        if (!cols || !cols->skey[p.col].off) {
          snprintf(err, err_cap,
                   "snapshot query: predicate %d: string key column %d is not "
                   "staged", i, p.col);
          return 9;
        }
        str = &cols->skey[p.col];
      }
      dt = str ? YBG_T_STRING
               : YBG_T_INT64;  // key datums are sign-extended (key_col_value)
      if (cols) sp.col = str ? str->pfx : cols->key[p.col];
      sp.null_m = 0;
      if (str) {
        int rc = snap_build_str_pred(p, *str, i, aux, &sp, err, err_cap);
        if (rc) return rc;
        out->general = kSnapGenStr;
        continue;
      }
    } else {
      if (p.col < 0 || p.col >= sc.num_value_cols) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: value column %d out of range",
                 i, p.col);
        return 9;
      }
      dt = sc.value_cols[p.col].dtype;
      if (dt == YBG_T_STRING && (!cols || !cols->sval[p.col].off)) {
        snprintf(err, err_cap,
                 "snapshot query: predicate %d: string column %d is not "
                 "staged", i, p.col);
        return 9;
      }
      if (cols)
        sp.col = dt == YBG_T_STRING ? cols->sval[p.col].pfx : cols->val[p.col];
      sp.null_m = 1u << p.col;
      if (nullable & sp.null_m) out->any_nullable = 1;
      if (dt == YBG_T_STRING) {
        int rc = snap_build_str_pred(p, cols->sval[p.col], i, aux, &sp, err,
                                     err_cap);
        if (rc) return rc;
        out->general = kSnapGenStr;
        continue;
      }
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
      if (out->general < kSnapGenList) out->general = kSnapGenList;
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
      if (!cols || !cols->sval[a.col].off) {
        snprintf(err, err_cap,
                 "snapshot query: aggregate %d: string column %d is not "
                 "staged", g, a.col);
        return 9;
      }
      if (a.op != YBG_AGG_COUNT) {
        snprintf(err, err_cap,
                 "snapshot query: aggregate %d: only COUNT is supported on "
                 "string column %d", g, a.col);
        return 9;
      }
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

// ABI grouped query -> SnapGroupQuery: snap_build_query's rules for the
// predicates and aggregates, plus the group column (any staged value or key
// column) and at least one aggregate.
inline int snap_build_group_query(const ybg_schema_t& sc,
                                  const SnapCols* cols,
                                  const ybg_snapshot_group_query_t& gq,
                                  uint64_t n_rows, std::vector<uint8_t>* aux,
                                  SnapGroupQuery* out, char* err,
                                  size_t err_cap) {
  memset(out, 0, sizeof(*out));
  int rc = snap_build_query(sc, cols, gq.num_preds, gq.preds, gq.num_aggs,
                            gq.aggs, n_rows, aux, &out->q, err, err_cap);
  if (rc) return rc;
  if (gq.num_aggs == 0) {
    snprintf(err, err_cap,
             "snapshot group query: num_aggs 0: a grouped query needs at "
             "least one aggregate");
    return 9;
  }
  const int nk = sc.num_hash_cols + sc.num_range_cols;
  if (gq.group_is_key_col) {
    if (gq.group_col < 0 || gq.group_col >= nk) {
      snprintf(err, err_cap,
               "snapshot group query: group column: key column %d out of "
               "range", gq.group_col);
      return 9;
    }
    if (sc.key_types[gq.group_col] == YBG_KT_STRING) {
      snprintf(err, err_cap,
               "snapshot group query: group column: string key column %d is "
               "not staged", gq.group_col);
      return 9;
    }
    if (cols) out->grp_col = cols->key[gq.group_col];
  } else {
    if (gq.group_col < 0 || gq.group_col >= sc.num_value_cols) {
      snprintf(err, err_cap,
               "snapshot group query: group column: value column %d out of "
               "range", gq.group_col);
      return 9;
    }
    if (sc.value_cols[gq.group_col].dtype == YBG_T_STRING) {
      snprintf(err, err_cap,
               "snapshot group query: group column: string column %d is not "
               "staged", gq.group_col);
      return 9;
    }
    if (cols) out->grp_col = cols->val[gq.group_col];
    out->grp_null_m = 1u << gq.group_col;
    const uint32_t nullable = cols ? cols->nullable_cols : 0xffffffffu;
    if (nullable & out->grp_null_m) out->q.any_nullable = 1;
  }
  return 0;
}

// ABI select -> SnapQuery (predicates, zero aggregates) + SnapSelect (the
// projection: any staged value or key column, 1 .. YBG_MAX_SELECT_COLS
// entries, repeats allowed).
// allow_strings (yb_gpu_snapshot_select_var): staged string columns may be
// projected too.
inline int snap_build_select(const ybg_schema_t& sc, const SnapCols* cols,
                             const ybg_snapshot_select_t& sq, uint64_t n_rows,
                             std::vector<uint8_t>* aux, SnapQuery* out_q,
                             SnapSelect* out, char* err, size_t err_cap,
                             bool allow_strings = false) {
  memset(out, 0, sizeof(*out));
  int rc = snap_build_query(sc, cols, sq.num_preds, sq.preds, 0, nullptr,
                            n_rows, aux, out_q, err, err_cap);
  if (rc) return rc;
  if (sq.num_cols == 0) {
    snprintf(err, err_cap,
             "snapshot select: num_cols 0: a select needs at least one "
             "projected column");
    return 9;
  }
  if (sq.num_cols < 0 || sq.num_cols > YBG_MAX_SELECT_COLS) {
    snprintf(err, err_cap, "snapshot select: num_cols %d over the cap %d",
             sq.num_cols, YBG_MAX_SELECT_COLS);
    return 9;
  }
  const int nk = sc.num_hash_cols + sc.num_range_cols;
  const uint32_t nullable = cols ? cols->nullable_cols : 0xffffffffu;
  out->num_cols = sq.num_cols;
  out->backward = sq.backward ? 1 : 0;
  for (int j = 0; j < sq.num_cols; ++j) {
    const ybg_select_col_t& c = sq.cols[j];
    SnapSelCol& o = out->cols[j];
    if (c.is_key_col) {
      if (c.col < 0 || c.col >= nk) {
        snprintf(err, err_cap,
                 "snapshot select: column %d: key column %d out of range", j,
                 c.col);
        return 9;
      }
      if (sc.key_types[c.col] == YBG_KT_STRING) {
        if (!cols || !cols->skey[c.col].off) {
          snprintf(err, err_cap,
                   "snapshot select: column %d: string key column %d is not "
                   "staged", j, c.col);
          return 9;
        }
        if (!allow_strings) {
          snprintf(err, err_cap,
                   "snapshot select: column %d: string key column %d needs "
                   "yb_gpu_snapshot_select_var", j, c.col);
          return 9;
        }
        o.col = cols->skey[c.col].off;
        o.is_str = 1;
        out->str_bytes[j] = cols->skey[c.col].bytes;
        ++out->num_str;
      } else if (cols) {
        o.col = cols->key[c.col];
      }
    } else {
      if (c.col < 0 || c.col >= sc.num_value_cols) {
        snprintf(err, err_cap,
                 "snapshot select: column %d: value column %d out of range",
                 j, c.col);
        return 9;
      }
      if (sc.value_cols[c.col].dtype == YBG_T_STRING) {
        if (!cols || !cols->sval[c.col].off) {
          snprintf(err, err_cap,
                   "snapshot select: column %d: string column %d is not "
                   "staged", j, c.col);
          return 9;
        }
        if (!allow_strings) {
          snprintf(err, err_cap,
                   "snapshot select: column %d: string column %d needs "
                   "yb_gpu_snapshot_select_var", j, c.col);
          return 9;
        }
        o.col = cols->sval[c.col].off;
        o.is_str = 1;
        out->str_bytes[j] = cols->sval[c.col].bytes;
        ++out->num_str;
      } else if (cols) {
        o.col = cols->val[c.col];
      }
      o.null_m = 1u << c.col;
      out->proj_mask |= o.null_m;
    }
  }
  // the null word is read only when a projected column can hold a NULL
  if (cols && (out->proj_mask & nullable)) out->nullmask = cols->nullmask;
  return 0;
}

// Counters and paging state of a select from the scan's header. w: the
// clamped window (lo >= hi: empty), delivered: the header's rank range,
// first_pos / last_pos: the lowest / highest delivered position (ignored
// when nothing was delivered).
inline void snap_select_fill(uint64_t lo, uint64_t hi, const SnapSelectHdr& h,
                             int backward, uint64_t first_pos,
                             uint64_t last_pos,
                             ybg_snapshot_select_result_t* out) {
  const uint64_t n = h.end - h.first;
  out->n_rows = n;
  out->rows_scanned = hi > lo ? hi - lo : 0;
  out->rows_matched = h.total;
  out->done = n == h.total ? 1 : 0;
  if (backward)
    out->resume_row = out->done ? lo : first_pos;
  else
    out->resume_row = out->done ? hi : last_pos + 1;
}

// ABI ordered select -> SnapQuery + SnapSelect (snap_build_select's rules,
// string projection allowed) + SnapOrder.
inline int snap_build_order(const ybg_schema_t& sc, const SnapCols* cols,
                            const ybg_snapshot_order_t& oq, uint64_t n_rows,
                            std::vector<uint8_t>* aux, SnapQuery* out_q,
                            SnapSelect* out_sel, SnapOrder* out, char* err,
                            size_t err_cap) {
  memset(out, 0, sizeof(*out));
  int rc = snap_build_select(sc, cols, oq.sel, n_rows, aux, out_q, out_sel,
                             err, err_cap, true);
  if (rc) return rc;
  if (oq.sel.backward) {
    snprintf(err, err_cap,
             "snapshot ordered select: backward %d: the direction is "
             "`descending`, sel.backward must be 0", oq.sel.backward);
    return 9;
  }
  const int nk = sc.num_hash_cols + sc.num_range_cols;
  int dt;
  if (oq.order_is_key_col) {
    if (oq.order_col < 0 || oq.order_col >= nk) {
      snprintf(err, err_cap,
               "snapshot ordered select: order column: key column %d out of "
               "range", oq.order_col);
      return 9;
    }
    if (sc.key_types[oq.order_col] == YBG_KT_STRING) {
      snprintf(err, err_cap,
               "snapshot ordered select: order column: string key column %d "
               "is not supported", oq.order_col);
      return 9;
    }
    dt = YBG_T_INT64;
    if (cols) out->col = cols->key[oq.order_col];
  } else {
    if (oq.order_col < 0 || oq.order_col >= sc.num_value_cols) {
      snprintf(err, err_cap,
               "snapshot ordered select: order column: value column %d out "
               "of range", oq.order_col);
      return 9;
    }
    dt = sc.value_cols[oq.order_col].dtype;
    if (dt == YBG_T_STRING) {
      snprintf(err, err_cap,
               "snapshot ordered select: order column: string column %d is "
               "not supported", oq.order_col);
      return 9;
    }
    if (cols) out->col = cols->val[oq.order_col];
    out->null_m = 1u << oq.order_col;
    const uint32_t nullable = cols ? cols->nullable_cols : 0xffffffffu;
    if (cols && (nullable & out->null_m)) out->nullmask = cols->nullmask;
  }
  if (oq.have_cursor && oq.cursor_row >= (1ull << 32)) {
    snprintf(err, err_cap,
             "snapshot ordered select: cursor_row %llu: positions are below "
             "2^32", (unsigned long long)oq.cursor_row);
    return 9;
  }
  out->kind = dt == YBG_T_DOUBLE ? kSnapOrderDouble
              : dt == YBG_T_FLOAT ? kSnapOrderFloat : kSnapOrderInt;
  out->descending = oq.descending ? 1 : 0;
  out->nulls_first = oq.nulls_first ? 1 : 0;
  out->have_cursor = oq.have_cursor ? 1 : 0;
  if (out->have_cursor)
    out->cursor = snap_order_key(*out, oq.cursor_datum,
                                 oq.cursor_is_null != 0, oq.cursor_row);
  return 0;
}

// Early-out threshold of a call: YBG_SNAP_ORDER_CAND, else the default.
inline uint64_t snap_order_cand_env() {
  const char* e = getenv("YBG_SNAP_ORDER_CAND");
  if (!e || !*e) return kSnapOrderCand;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return v ? v : kSnapOrderCand;
}

// Counters of an ordered select: n delivered of `eligible`.
inline void snap_order_fill(uint64_t lo, uint64_t hi, uint64_t n,
                            uint64_t eligible, uint32_t passes,
                            const SnapOrderCursor* cur,
                            ybg_snapshot_order_result_t* out) {
  out->r.n_rows = n;
  out->r.rows_scanned = hi > lo ? hi - lo : 0;
  out->r.rows_matched = eligible;
  out->r.done = n == eligible ? 1 : 0;
  out->r.resume_row = 0;
  out->digit_passes = passes;
  if (cur && n) {
    out->cursor_is_null = (int32_t)cur->is_null;
    out->cursor_datum = cur->datum;
    out->cursor_row = cur->row;
  }
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
