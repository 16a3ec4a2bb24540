// yugabyte-db_amd/csrc/scan_host_sim.cc — host-side simulator of the GPU
// per-interval scan algorithm (scan_device.h), sequentially executing the
// exact device code path including head-row deferral, tail walks and
// continuation-flag resolution. TEST INFRASTRUCTURE: lets the CPU test suite
// pin the device algorithm against the oracle without a GPU. Exported as
// ybg_sim_scan from the product library (never used on the product path).
extern "C" unsigned long long ybg_fast_abort_hist[32];
extern "C" unsigned long long ybg_fast_abort_hist[32] = {0};
#define YBG_FABORT(n) do { ++ybg_fast_abort_hist[n]; return 0; } while (0)
// Per-trip census of scan_batch_fast (ybg_sim_fast_census): one record per
// loop trip while a sink is installed, nothing otherwise.
struct YbgCensusRec { unsigned char kind, sp, ns1, ns2, l1, l2; };
struct YbgCensusSink { YbgCensusRec* rec; unsigned n, cap; };
static YbgCensusSink* ybg_census_sink = nullptr;
#define YBG_CENSUS_REC(kind_, sp_, ns1_, ns2_, l1_, l2_)                     \
  do {                                                                       \
    if (ybg_census_sink && ybg_census_sink->n < ybg_census_sink->cap)        \
      ybg_census_sink->rec[ybg_census_sink->n++] = YbgCensusRec{             \
          (unsigned char)(kind_), (unsigned char)(sp_),                      \
          (unsigned char)(ns1_), (unsigned char)(ns2_),                      \
          (unsigned char)(l1_), (unsigned char)(l2_)};                       \
  } while (0)
#define YBG_HOST_SIM 1
#define YBG_DEV_QUAL inline
#include "scan_device.h"
#include "snap_device.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

using namespace ybgdev;

namespace {
// Intervals per batch, as the kernels read it (YBG_IVB): the sim loops
// over the same batch decomposition so C > 1 is parity-testable on CPU.
uint64_t sim_ivb() {
  if (const char* e = getenv("YBG_IVB")) {
    long v = atol(e);
    if (v >= 1 && v <= 4096) return (uint64_t)v;
  }
  return 1;
}

// Interval table from the blocks' restart arrays (k_count_restarts +
// k_emit_intervals, serial). Returns 3 on a malformed block.
int build_intervals(const uint8_t* data, const uint64_t* offsets,
                    uint64_t n_blocks, std::vector<Interval>* ivs) {
  for (uint64_t b = 0; b < n_blocks; ++b) {
    uint64_t sz = offsets[b + 1] - offsets[b];
    if (sz < 8) return 3;
    const uint8_t* blk = data + offsets[b];
    uint32_t nr = load_le32_u(blk + sz - 4);
    if (nr == 0 || (uint64_t)nr * 4 + 4 > sz) return 3;
    uint32_t restarts_off = (uint32_t)(sz - 4 - (uint64_t)nr * 4);
    for (uint32_t r = 0; r < nr; ++r) {
      uint32_t start = load_le32_u(blk + restarts_off + 4ull * r);
      uint32_t end = (r + 1 < nr)
                         ? load_le32_u(blk + restarts_off + 4ull * (r + 1))
                         : restarts_off;
      ivs->push_back(Interval{(uint32_t)b, start, end});
    }
  }
  return 0;
}

// DevSpec + aux bytes from the ABI spec (the translation yb_gpu_scan_open
// uses), with the same 16 bytes of windowed-load tail slack.
void build_spec(const ybg_scan_spec_t* spec, DevSpec* d,
                std::vector<unsigned char>* aux) {
  aux->assign(1 << 20, 0);
  uint32_t aux_len = 0;
  build_dev_spec(spec, d, aux->data(), &aux_len, (uint32_t)aux->size());
  aux->resize(aux_len + 16, 0);
}

// Counters, aggregates and the restart-min slot bht[3..5] = {hi, lo, len}
// (process_entry tracking) into the ABI result.
void store_result(const DevSpec& d, uint64_t entries, uint64_t scanned,
                  uint64_t matched, const uint64_t* agg_val,
                  const uint64_t* agg_cnt, const uint64_t* bht,
                  ybg_scan_result_t* out) {
  memset(out, 0, sizeof(*out));
  out->entries_seen = entries;
  out->rows_scanned = scanned;
  out->rows_matched = matched;
  out->restart_ht_len =
      unpack_restart_ht(bht[3], bht[4], bht[5], out->restart_ht);
  for (int g = 0; g < d.num_aggs; ++g) {
    out->aggs[g].is_null = (agg_cnt[g] == 0);
    switch (d.aggs[g].op) {
      case YBG_AGG_SUM_DOUBLE:
      case YBG_AGG_MIN_DOUBLE:
      case YBG_AGG_MAX_DOUBLE: {
        double dd;
        memcpy(&dd, &agg_val[g], 8);
        out->aggs[g].value_f64 = dd;
        break;
      }
      default:
        out->aggs[g].value_i64 = (int64_t)agg_val[g];
        break;
    }
  }
}

// One batch through scan_batch_fast in the shape the GPU dispatch picks:
// NC, FUSE and PLAN mirror it so CPU fuzz covers every compiled shape of
// the fast kernel.
int fast_batch(const DevSpec& d, const FastPlan& plan, bool planned,
               const uint8_t* data, const uint64_t* offsets,
               const Interval* ivs, uint64_t n_ivs, uint64_t lo, uint64_t hi,
               uint8_t* key, uint64_t* rmin, uint32_t* e32, uint32_t* s32,
               uint32_t* m32, uint64_t* agg_val, uint64_t* agg_cnt,
               HeadOut<2>* ho, bool* wn) {
  auto call_fast = [&](auto nc_tag, auto plan_tag) {
    constexpr int N = decltype(nc_tag)::value;
    constexpr bool P = decltype(plan_tag)::value;
    auto run = [&](auto fuse_tag) {
      constexpr bool F = decltype(fuse_tag)::value;
      return scan_batch_fast<2, N, F, P>(d, data, offsets, ivs, n_ivs, lo, hi,
                                         key, rmin, e32, s32, m32, agg_val,
                                         agg_cnt, ho, wn, &plan);
    };
    return d.fuse_hint ? run(std::true_type{}) : run(std::false_type{});
  };
  using std::integral_constant;
  const std::true_type plan_on{};
  const std::false_type plan_off{};
  if (planned) {
    switch (fast_plan_nr(plan)) {
      case 0: return call_fast(integral_constant<int, 0>{}, plan_on);
      case 1: return call_fast(integral_constant<int, 1>{}, plan_on);
      case 2: return call_fast(integral_constant<int, 2>{}, plan_on);
      case 3: return call_fast(integral_constant<int, 3>{}, plan_on);
      case 4: return call_fast(integral_constant<int, 4>{}, plan_on);
      case kPlanShapeP1:
        return call_fast(integral_constant<int, kPlanShapeP1>{}, plan_on);
      case kPlanShapeP1S1:
        return call_fast(integral_constant<int, kPlanShapeP1S1>{}, plan_on);
      case kPlanShapeP2:
        return call_fast(integral_constant<int, kPlanShapeP2>{}, plan_on);
      default: return call_fast(integral_constant<int, 8>{}, plan_on);
    }
  }
  if (d.num_value_cols <= 4)
    return call_fast(integral_constant<int, 4>{}, plan_off);
  return call_fast(integral_constant<int, 8>{}, plan_off);
}
}  // namespace

extern "C" {

// Mirrors yb_gpu_scan_open's spec translation + k_scan + k_reduce, serially.
int ybg_sim_scan(const ybg_scan_spec_t* spec, const uint8_t* data,
                 const uint64_t* offsets, uint64_t n_blocks,
                 ybg_scan_result_t* out) {
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);

  std::vector<Interval> ivs;
  if (int rc = build_intervals(data, offsets, n_blocks, &ivs)) return rc;
  uint64_t n_ivs = ivs.size();

  // ---- per-batch scan (k_scan body, serial) ----
  const uint64_t ivb = sim_ivb();
  const uint64_t n_b = (n_ivs + ivb - 1) / ivb;
  uint64_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[YBG_MAX_AGGS] = {0}, agg_cnt[YBG_MAX_AGGS] = {0};
  std::vector<HeadOut<YBG_MAX_AGGS>> heads(n_b);
  std::vector<uint8_t> walked(n_b, 0);
  alignas(8) uint8_t key[kKeyCap];
  alignas(8) uint8_t rk_save[kKeyCap];
  uint64_t bht[6] = {0, 0, 0, 0, 0, 0};
  for (uint64_t b = 0; b < n_b; ++b) {
    bool wn = false;
    uint32_t e32 = 0, s32 = 0, m32 = 0;
    uint64_t lo = b * ivb;
    uint64_t hi = lo + ivb < n_ivs ? lo + ivb : n_ivs;
    if (!scan_one_interval<YBG_MAX_AGGS>(d, data, offsets, ivs.data(), n_ivs,
                                         lo, hi, aux.data(), key, rk_save,
                                         bht, &e32, &s32, &m32, agg_val,
                                         agg_cnt, &heads[b], &wn, nullptr))
      return 6;
    entries += e32;
    scanned += s32;
    matched += m32;
    walked[b] = wn ? 1 : 0;
  }
  // head ownership resolution (shfl relay / cont flags, serial equivalent)
  for (uint64_t b = 0; b < n_b; ++b) {
    bool consumed = b > 0 && walked[b - 1];
    if (consumed) continue;
    scanned += heads[b].scanned;
    matched += heads[b].matched;
    agg_combine(d, agg_val, agg_cnt, heads[b].val, heads[b].cnt);
  }

  store_result(d, entries, scanned, matched, agg_val, agg_cnt, bht, out);
  return 0;
}

// Fast-path simulator: runs scan_batch_fast per batch with the general
// scan_one_interval as the per-batch fallback (the retry protocol the GPU
// dispatch uses). n_fallback_out reports how many batches aborted — tests
// assert 0 on eligible data and bit-exact results either way.
// Head rows follow the kernels' state-byte protocol: batch b sits in lane
// b % 64; the planned pass resolves a head inside the wave (head_action,
// the kernel's own decision) when the predecessor lane completed on the
// fast path, every other head is left pending and folded by state, as
// k_fold does.
// A known abort set (known_ids, any order, ids past the batch count
// ignored) models the GPU dispatch's remembered set: listed batches go
// straight to the general scanner, every other batch that aborts still
// falls back, so the result never depends on the set. fallback_ids_out
// (capacity fallback_cap) receives the ids of all batches the general
// scanner ran, ascending.
int ybg_sim_scan_fast_known(const ybg_scan_spec_t* spec, const uint8_t* data,
                            const uint64_t* offsets, uint64_t n_blocks,
                            const uint64_t* known_ids, uint64_t n_known,
                            ybg_scan_result_t* out, uint64_t* n_fallback_out,
                            uint64_t* fallback_ids_out,
                            uint64_t fallback_cap) {
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);
  if (!fast_eligible(d)) return 9;

  std::vector<Interval> ivs;
  if (int rc = build_intervals(data, offsets, n_blocks, &ivs)) return rc;
  uint64_t n_ivs = ivs.size();
  const uint64_t ivb = sim_ivb();
  const uint64_t n_b = (n_ivs + ivb - 1) / ivb;
  uint64_t entries = 0, scanned = 0, matched = 0, fallbacks = 0;
  uint64_t agg_val[2] = {0, 0}, agg_cnt[2] = {0, 0};
  std::vector<HeadOut<2>> heads(n_b);
  std::vector<uint8_t> state(n_b, 0);    // the per-batch state byte
  std::vector<uint8_t> fast_ok(n_b, 0);  // completed by scan_batch_fast
  std::vector<uint8_t> known(n_b, 0);    // the bitmap k_scan_fast tests
  for (uint64_t i = 0; i < n_known; ++i)
    if (known_ids[i] < n_b) known[known_ids[i]] = 1;
  alignas(8) uint8_t key[kKeyCap];
  alignas(8) uint8_t rk_save[kKeyCap];
  uint64_t bht[6] = {0, 0, 0, 0, 0, 0};
  // the GPU dispatch's choice: a plannable spec runs the planned pass
  FastPlan plan;
  const bool planned = build_fast_plan(d, &plan) && fast_plan_enabled();
  for (uint64_t b = 0; b < n_b; ++b) {
    bool wn = false;
    uint32_t e32 = 0, s32 = 0, m32 = 0;
    uint64_t lo = b * ivb;
    uint64_t hi = lo + ivb < n_ivs ? lo + ivb : n_ivs;
    int rc = 0;  // known: skipped by the fast kernel, run from the list
    if (!known[b])
      rc = fast_batch(d, plan, planned, data, offsets, ivs.data(), n_ivs, lo,
                      hi, key, bht + 3, &e32, &s32, &m32, agg_val, agg_cnt,
                      &heads[b], &wn);
    if (!rc) {
      if (fallback_ids_out && fallbacks < fallback_cap)
        fallback_ids_out[fallbacks] = b;
      ++fallbacks;
      uint64_t av8[YBG_MAX_AGGS] = {0}, ac8[YBG_MAX_AGGS] = {0};
      HeadOut<YBG_MAX_AGGS> ho8;
      e32 = s32 = m32 = 0;
      if (!scan_one_interval<YBG_MAX_AGGS>(
              d, data, offsets, ivs.data(), n_ivs, lo, hi, aux.data(), key,
              rk_save, bht, &e32, &s32, &m32, av8, ac8, &ho8, &wn, nullptr))
        return 6;
      for (int g = 0; g < 2; ++g) {
        combine1(d.agg_op[g], &agg_val[g], &agg_cnt[g], av8[g], ac8[g]);
        heads[b].val[g] = ho8.val[g];
        heads[b].cnt[g] = ho8.cnt[g];
      }
      heads[b].scanned = ho8.scanned;
      heads[b].matched = ho8.matched;
    }
    entries += e32;
    scanned += s32;
    matched += m32;
    fast_ok[b] = rc ? 1 : 0;
    const uint8_t w = wn ? kBatchWalked : 0;
    if (rc && planned) {
      // k_scan_fast<PLAN>: the lane relay (lane 0's shuffle input is unused)
      const bool p_ok = b > 0 && fast_ok[b - 1];
      const bool p_wn = b > 0 && (state[b - 1] & kBatchWalked);
      const HeadAction act =
          head_action((unsigned)(b % 64), true, p_ok, p_wn);
      if (act == kHeadFold) {
        scanned += heads[b].scanned;
        matched += heads[b].matched;
        for (int g = 0; g < 2; ++g) {
          agg_val[g] += heads[b].val[g];
          agg_cnt[g] += heads[b].cnt[g];
        }
      }
      state[b] = w | (act == kHeadWrite ? kBatchHeadPending : 0);
    } else {
      // interpreted fast kernel and the general (retry) kernel
      state[b] = w | kBatchHeadPending;
    }
  }
  // k_fold: pending heads the predecessor did not walk into
  for (uint64_t b = 0; b < n_b; ++b) {
    if (!(state[b] & kBatchHeadPending)) continue;
    if (b > 0 && (state[b - 1] & kBatchWalked)) continue;
    scanned += heads[b].scanned;
    matched += heads[b].matched;
    for (int g = 0; g < d.num_aggs && g < 2; ++g)
      combine1(d.agg_op[g], &agg_val[g], &agg_cnt[g], heads[b].val[g],
               heads[b].cnt[g]);
  }
  store_result(d, entries, scanned, matched, agg_val, agg_cnt, bht, out);
  if (n_fallback_out) *n_fallback_out = fallbacks;
  return 0;
}

int ybg_sim_scan_fast(const ybg_scan_spec_t* spec, const uint8_t* data,
                      const uint64_t* offsets, uint64_t n_blocks,
                      ybg_scan_result_t* out, uint64_t* n_fallback_out) {
  return ybg_sim_scan_fast_known(spec, data, offsets, n_blocks, nullptr, 0,
                                 out, n_fallback_out, nullptr, 0);
}

// Census of the fast kernel's entry loop (scripts/fast_census.py): replays
// the first max_blocks blocks (0 = all) through scan_batch_fast with the
// per-trip hook on, 64 consecutive batches at a time, and counts them the
// way a wave runs them — trip t of the wave holds every lane's trip t, a
// path costs the wave a pass when ANY lane takes it, and a byte loop runs
// to the longest lane's count. out[] (kCensusWords u64):
//   0 waves, 1 batches, 2 aborted batches, 3 wave trips, 4 lane trips,
//   5..9 wave trips holding kind 0..4 (switch, restart, frequent, 2.1.1,
//   general), 10 wave trips holding a delta entry, 11 wave trips holding
//   two or more of {restart, frequent/2.1.1, general}, 12..16 lane trips
//   per kind, 17 / 18 tail-patch iterations lockstep / summed over lanes,
//   19 / 20 the same for the LDS byte loops, 21 lane delta entries,
//   22 / 23 shortest / longest restart key (ns1 of kind 1; 0 = none),
//   32.. sp histogram (128), 160.. ns1 (32), 192.. ns2 (16) over lane
//   delta entries.
enum { kCensusWords = 208 };
int ybg_sim_fast_census(const ybg_scan_spec_t* spec, const uint8_t* data,
                        const uint64_t* offsets, uint64_t n_blocks,
                        uint64_t max_blocks, uint64_t* out) {
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);
  if (!fast_eligible(d)) return 9;
  if (max_blocks && max_blocks < n_blocks) n_blocks = max_blocks;
  std::vector<Interval> ivs;
  if (int rc = build_intervals(data, offsets, n_blocks, &ivs)) return rc;
  const uint64_t n_ivs = ivs.size();
  const uint64_t ivb = sim_ivb();
  const uint64_t n_b = (n_ivs + ivb - 1) / ivb;
  FastPlan plan;
  const bool planned = build_fast_plan(d, &plan) && fast_plan_enabled();
  memset(out, 0, kCensusWords * sizeof(uint64_t));
  const unsigned kCap = 1u << 16;
  std::vector<YbgCensusRec> recs(64 * (size_t)kCap);
  alignas(8) uint8_t key[kKeyCap];
  for (uint64_t w0 = 0; w0 < n_b; w0 += 64) {
    unsigned cnt[64] = {0};
    unsigned max_n = 0;
    const unsigned lanes = (unsigned)(n_b - w0 < 64 ? n_b - w0 : 64);
    for (unsigned l = 0; l < lanes; ++l) {
      const uint64_t b = w0 + l;
      const uint64_t lo = b * ivb;
      const uint64_t hi = lo + ivb < n_ivs ? lo + ivb : n_ivs;
      YbgCensusSink sink = {recs.data() + (size_t)l * kCap, 0, kCap};
      uint32_t e32 = 0, s32 = 0, m32 = 0;
      uint64_t av[2] = {0, 0}, ac[2] = {0, 0}, rmin[3] = {0, 0, 0};
      HeadOut<2> ho;
      bool wn = false;
      ybg_census_sink = &sink;
      const int rc = fast_batch(d, plan, planned, data, offsets, ivs.data(),
                                n_ivs, lo, hi, key, rmin, &e32, &s32, &m32,
                                av, ac, &ho, &wn);
      ybg_census_sink = nullptr;
      if (!rc) out[2] += 1;
      cnt[l] = sink.n;
      if (sink.n > max_n) max_n = sink.n;
    }
    out[0] += 1;
    out[1] += lanes;
    out[3] += max_n;
    for (unsigned t = 0; t < max_n; ++t) {
      unsigned kinds = 0, m1 = 0, m2 = 0, ml1 = 0, ml2 = 0;
      for (unsigned l = 0; l < lanes; ++l) {
        if (t >= cnt[l]) continue;
        const YbgCensusRec& r = recs[(size_t)l * kCap + t];
        out[4] += 1;
        out[12 + r.kind] += 1;
        kinds |= 1u << r.kind;
        if (r.kind == 1) {
          if (!out[22] || r.ns1 < out[22]) out[22] = r.ns1;
          if (r.ns1 > out[23]) out[23] = r.ns1;
        }
        if (r.kind < 2) continue;
        out[21] += 1;
        out[18] += (uint64_t)r.ns1 + r.ns2;
        out[20] += (uint64_t)r.l1 + r.l2;
        out[32 + (r.sp & 127)] += 1;
        out[160 + (r.ns1 & 31)] += 1;
        out[192 + (r.ns2 & 15)] += 1;
        if (r.ns1 > m1) m1 = r.ns1;
        if (r.ns2 > m2) m2 = r.ns2;
        if (r.l1 > ml1) ml1 = r.l1;
        if (r.l2 > ml2) ml2 = r.l2;
      }
      for (int k = 0; k < 5; ++k) out[5 + k] += (kinds >> k) & 1;
      if (kinds & 0x1c) out[10] += 1;
      const int paths = ((kinds >> 1) & 1) + ((kinds & 0xc) ? 1 : 0) +
                        ((kinds >> 4) & 1);
      if (paths >= 2) out[11] += 1;
      out[17] += m1 + m2;
      out[19] += ml1 + ml2;
    }
  }
  return 0;
}

// 1 when ybg_sim_scan_fast would run this spec through the planned pass
// (build_fast_plan succeeds and YBG_PLAN does not turn it off), else 0 —
// the simulator-side yb_gpu_scan_planned.
int ybg_sim_scan_planned(const ybg_scan_spec_t* spec) {
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);
  FastPlan plan;
  return build_fast_plan(d, &plan) && fast_plan_enabled() ? 1 : 0;
}

// TEST ONLY: the compiled shape of the spec's column plan (fast_plan_nr:
// 0..4 or 8 ranged columns of the two-list form, 16 one pair, 17 a pair
// and a single, 18 two pairs), -1 when the spec has no plan.
int ybg_sim_plan_shape(const ybg_scan_spec_t* spec) {
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);
  FastPlan plan;
  return build_fast_plan(d, &plan) ? fast_plan_nr(plan) : -1;
}

// TEST ONLY: the planned kernel's per-lane head decision (head_action).
int ybg_sim_head_action(unsigned lane, int ok, int p_ok, int p_wn) {
  return (int)head_action(lane, ok != 0, p_ok != 0, p_wn != 0);
}

// TEST ONLY: the planned pass's column extraction (plan_load_cols) over a
// packed row of ncols (<= 8) int64 columns starting at `value`, every
// column listed; out[k] = column k. nc_cap picks the compiled count (4 or
// 8); slots past ncols are padding and read the value start.
int ybg_sim_plan_extract(const uint8_t* value, int ncols, int nc_cap,
                         uint64_t* out) {
  if (ncols < 1 || ncols > nc_cap || (nc_cap != 4 && nc_cap != 8)) return 1;
  uint8_t off[8] = {0};  // slots past ncols are padding, as in a plan
  for (int k = 0; k < ncols; ++k) off[k] = (uint8_t)(3 + 8 * k);
  uint64_t uv[8] = {0};
  if (nc_cap == 4) plan_load_cols<4>(off, value, uv);
  else plan_load_cols<8>(off, value, uv);
  for (int k = 0; k < ncols; ++k) out[k] = uv[k];
  return 0;
}

// Sequential emit-mode simulator: pass 1 computes walked flags, pass 2
// re-runs the exact device emit path. Caller provides output arrays.
int ybg_sim_emit(const ybg_scan_spec_t* spec, const uint8_t* data,
                 const uint64_t* offsets, uint64_t n_blocks,
                 uint64_t row_cap, uint64_t* sort_key, uint64_t* key_datums,
                 uint64_t* datums, uint32_t* null_masks, uint8_t* varlen,
                 uint64_t varlen_cap, uint64_t* n_rows_out,
                 uint64_t* varlen_out) {
  std::vector<uint16_t> hashes(row_cap);
  DevSpec d;
  std::vector<unsigned char> aux;
  ybg_scan_spec_t spec2 = *spec;
  spec2.emit_rows = 1;
  build_spec(&spec2, &d, &aux);

  std::vector<Interval> ivs;
  if (int rc = build_intervals(data, offsets, n_blocks, &ivs)) return rc;
  uint64_t n_ivs = ivs.size();
  const uint64_t ivb = sim_ivb();
  const uint64_t n_b = (n_ivs + ivb - 1) / ivb;
  uint32_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[YBG_MAX_AGGS] = {0}, agg_cnt[YBG_MAX_AGGS] = {0};
  std::vector<uint32_t> head_consumed(n_ivs ? n_ivs : 1, 0);
  alignas(8) uint8_t key[kKeyCap];
  alignas(8) uint8_t rk_save[kKeyCap];
  uint64_t bht[6] = {0, 0, 0, 0, 0, 0};
  HeadOut<YBG_MAX_AGGS> ho;
  // flags pre-pass (write_all_flags form): per-interval head consumption
  // is written inside the walk via iv_flags
  for (uint64_t b = 0; b < n_b; ++b) {
    bool wn = false;
    uint64_t lo = b * ivb;
    uint64_t hi = lo + ivb < n_ivs ? lo + ivb : n_ivs;
    if (!scan_one_interval<YBG_MAX_AGGS>(d, data, offsets, ivs.data(), n_ivs,
                                         lo, hi, aux.data(), key, rk_save,
                                         bht, &entries, &scanned, &matched,
                                         agg_val, agg_cnt, &ho, &wn,
                                         head_consumed.data()))
      return 6;
  }

  unsigned long long row_counter = 0, varlen_counter = 0, overflow = 0;
  EmitCtx ec;
  ec.sort_key = sort_key;
  ec.key_datums = key_datums;
  ec.datums = datums;
  ec.null_masks = null_masks;
  ec.hashes = hashes.data();
  ec.varlen = varlen;
  ec.varlen_cap = varlen_cap;
  ec.row_counter = &row_counter;
  ec.varlen_counter = &varlen_counter;
  ec.overflow = &overflow;
  ec.row_cap = row_cap;
  ec.nk = spec->schema.num_hash_cols + spec->schema.num_range_cols;
  ec.nc = spec->schema.num_value_cols;
  ec.head_consumed = head_consumed.data();
  uint64_t rowbuf[YBG_MAX_COLS];
  uint32_t lenbuf[YBG_MAX_COLS];
  for (uint64_t j = 0; j < n_ivs; ++j) {
    bool wn = false;
    HeadOut<YBG_MAX_AGGS> ho2;
    if (!scan_one_interval<YBG_MAX_AGGS, true>(
            d, data, offsets, ivs.data(), n_ivs, j, j + 1, aux.data(), key,
            rk_save, bht, &entries, &scanned, &matched, agg_val, agg_cnt,
            &ho2, &wn, nullptr, &ec, rowbuf, lenbuf))
      return 6;
  }
  // set on overflow too: the counters then hold the sizes needed
  *n_rows_out = row_counter;
  *varlen_out = varlen_counter;
  if (overflow) return 8;
  return 0;
}

// Sequential GROUP BY simulator: flags pass + grouped pass + export,
// running the exact device code path.
// null_index_out: the output entry of the NULL-key group, -1 without one
// (the simulator's yb_gpu_scan_group_null_index).
int ybg_sim_group_ex(const ybg_scan_spec_t* spec, const uint8_t* data,
                     const uint64_t* offsets, uint64_t n_blocks,
                     uint64_t* keys_out, long long* vals_out,
                     unsigned long long* cnts_out, uint8_t* key_bytes_out,
                     uint64_t key_bytes_cap, uint64_t cap, uint64_t* n_out,
                     uint8_t* restart_out, uint32_t* restart_len_out,
                     int64_t* null_index_out) {
  if (null_index_out) *null_index_out = -1;
  DevSpec d;
  std::vector<unsigned char> aux;
  build_spec(spec, &d, &aux);
  if (d.group_col < 0) return 9;

  std::vector<Interval> ivs;
  if (int rc = build_intervals(data, offsets, n_blocks, &ivs)) return rc;
  uint64_t n_ivs = ivs.size();
  const uint64_t ivb = sim_ivb();
  const uint64_t n_b = (n_ivs + ivb - 1) / ivb;
  uint32_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[YBG_MAX_AGGS] = {0}, agg_cnt[YBG_MAX_AGGS] = {0};
  std::vector<uint8_t> walked(n_b, 0);
  std::vector<GroupHead> gheads(n_b ? n_b : 1);
  alignas(8) uint8_t key[kKeyCap];
  alignas(8) uint8_t rk_save[kKeyCap];
  uint64_t bht[6] = {0, 0, 0, 0, 0, 0};

  uint64_t gcap = 1ull << 18;
  std::vector<unsigned long long> gkey(gcap + 1, 0);
  std::vector<unsigned> state(gcap + 1, 0);
  std::vector<long long> vals((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned long long> cnts((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned long long> vals_hi((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned> poison((gcap + 1) * YBG_MAX_AGGS, 0);
  for (uint64_t i = 0; i <= gcap; ++i)
    for (int g = 0; g < d.num_aggs; ++g)
      vals[i * YBG_MAX_AGGS + g] = group_init_value(d.aggs[g].op);
  unsigned long long overflow = 0;
  GroupCtx gc;
  gc.gkey = gkey.data();
  gc.state = state.data();
  gc.vals = vals.data();
  gc.cnts = cnts.data();
  gc.vals_hi = vals_hi.data();
  gc.poison = poison.data();
  gc.cap = gcap;
  gc.overflow = &overflow;
  gc.data = data;
  for (uint64_t b = 0; b < n_b; ++b) {
    bool wn = false;
    HeadOut<YBG_MAX_AGGS> ho;
    gheads[b].hit = 0;
    uint64_t lo = b * ivb;
    uint64_t hi = lo + ivb < n_ivs ? lo + ivb : n_ivs;
    if (!scan_one_interval<YBG_MAX_AGGS, false, true>(
            d, data, offsets, ivs.data(), n_ivs, lo, hi, aux.data(), key,
            rk_save, bht, &entries, &scanned, &matched, agg_val, agg_cnt, &ho,
            &wn, nullptr, nullptr, nullptr, nullptr, &gc, &gheads[b]))
      return 6;
    walked[b] = wn ? 1 : 0;
  }
  // head-ownership resolution (single-pass protocol, serial equivalent)
  for (uint64_t b = 0; b < n_b; ++b) {
    bool consumed = b > 0 && walked[b - 1];
    if (!consumed && gheads[b].hit)
      group_accum_rec<YBG_MAX_AGGS>(d, gc, gheads[b]);
  }
  if (overflow) return 8;
  if (restart_len_out) {  // restart-min slot, as ybg_sim_scan reports it
    *restart_len_out = 0;
    if (restart_out)
      *restart_len_out =
          unpack_restart_ht(bht[3], bht[4], bht[5], restart_out);
  }
  bool grp_is_str =
      d.cols[d.group_col].dtype == YBG_T_STRING;
  uint64_t n = 0, boff = 0;
  for (uint64_t i = 0; i <= gcap; ++i) {
    if (state[i] != 1) continue;
    if (n >= cap) return 8;
    uint64_t kv = gkey[i];
    if (i == gcap) {
      kv = ~0ull;
      if (null_index_out) *null_index_out = (int64_t)n;
    } else if (grp_is_str) {
      uint32_t len = (uint32_t)(kv >> 40);
      if (boff + len > key_bytes_cap) return 8;
      const uint8_t* src = data + (kv & ((1ull << 40) - 1));
      memcpy(key_bytes_out + boff, src, len);
      kv = ((uint64_t)len << 40) | boff;
      boff += len;
    }
    keys_out[n] = kv;
    for (int g = 0; g < YBG_MAX_AGGS; ++g) {
      int op = g < d.num_aggs ? d.agg_op[g] : -1;
      long long v = group_export_value(op, vals[i * YBG_MAX_AGGS + g],
                                       vals_hi[i * YBG_MAX_AGGS + g],
                                       poison[i * YBG_MAX_AGGS + g]);
      vals_out[n * YBG_MAX_AGGS + g] = v;
      cnts_out[n * YBG_MAX_AGGS + g] =
          (op == YBG_AGG_COUNT_STAR || op == YBG_AGG_COUNT)
              ? (unsigned long long)v
              : cnts[i * YBG_MAX_AGGS + g];
    }
    ++n;
  }
  *n_out = n;
  return 0;
}

int ybg_sim_group(const ybg_scan_spec_t* spec, const uint8_t* data,
                  const uint64_t* offsets, uint64_t n_blocks,
                  uint64_t* keys_out, long long* vals_out,
                  unsigned long long* cnts_out, uint8_t* key_bytes_out,
                  uint64_t key_bytes_cap, uint64_t cap, uint64_t* n_out,
                  uint8_t* restart_out, uint32_t* restart_len_out) {
  return ybg_sim_group_ex(spec, data, offsets, n_blocks, keys_out, vals_out,
                          cnts_out, key_bytes_out, key_bytes_cap, cap, n_out,
                          restart_out, restart_len_out, nullptr);
}

}  // extern "C"

namespace {
// The columnar snapshot's build, serially: block scan with predicates and
// aggregates stripped -> rows ordered by sort_key -> dense padded column
// arrays, exactly the device snapshot's layout. `cols` points into the
// vectors held here.
struct SimSnapshot {
  uint64_t n = 0;
  ybg_scan_result_t stats;
  std::vector<std::vector<uint64_t>> val, key;
  std::vector<uint32_t> nullmask;
  // stage_strings: off / bytes / pfx per string column (SnapStrCol layout)
  struct Str {
    std::vector<uint64_t> off, pfx;
    std::vector<uint8_t> bytes;
  };
  std::vector<Str> sval, skey;
  SnapCols cols;
};

int sim_snapshot_build(const ybg_scan_spec_t* spec, const uint8_t* data,
                       const uint64_t* offsets, uint64_t n_blocks,
                       SimSnapshot* sn, bool stage_strings = false) {
  ybg_scan_spec_t bs = *spec;
  bs.num_preds = 0;
  bs.num_aggs = 0;
  bs.emit_rows = 0;
  bs.row_limit = 0;
  bs.group_col = 0;
  bs.backward = 0;
  // scan statistics + exact visible-row count (the build's flags pass)
  ybg_scan_result_t& stats = sn->stats;
  int rc = ybg_sim_scan(&bs, data, offsets, n_blocks, &stats);
  if (rc) return rc;
  const ybg_schema_t& sc = spec->schema;
  const int nk = sc.num_hash_cols + sc.num_range_cols;
  const int nc = sc.num_value_cols;
  const uint64_t cap = stats.rows_scanned ? stats.rows_scanned : 1;
  std::vector<uint64_t> sort_key(cap), key_aos(cap * (nk ? nk : 1)),
      dat_aos(cap * (nc ? nc : 1));
  std::vector<uint32_t> null_aos(cap);
  uint64_t n = 0, vl = 0;
  std::vector<uint8_t> heap;
  if (stage_strings) {
    // the device build's counting pass: a heap of capacity 0 takes no byte
    // and leaves the exact size on the varlen counter
    uint8_t none = 0;
    rc = ybg_sim_emit(&bs, data, offsets, n_blocks, cap, sort_key.data(),
                      key_aos.data(), dat_aos.data(), null_aos.data(), &none,
                      0, &n, &vl);
    if (rc && rc != 8) return rc;
    if (n != stats.rows_scanned) return 8;
    heap.assign(vl + 16, 0);
  }
  // varlen heap absent: string datums are dropped, as in the device build
  rc = ybg_sim_emit(&bs, data, offsets, n_blocks, cap, sort_key.data(),
                    key_aos.data(), dat_aos.data(), null_aos.data(),
                    stage_strings ? heap.data() : nullptr,
                    stage_strings ? vl : 0, &n, &vl);
  if (rc) return rc;
  if (n != stats.rows_scanned) return 8;
  sn->n = n;

  std::vector<uint32_t> perm(n);
  for (uint64_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
  std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    return sort_key[a] < sort_key[b];
  });
  const uint64_t padded = snap_padded_rows(n);
  std::vector<std::vector<uint64_t>>& val = sn->val;
  std::vector<std::vector<uint64_t>>& key = sn->key;
  std::vector<uint32_t>& nullmask = sn->nullmask;
  val.resize(nc);
  key.resize(nk);
  nullmask.assign(padded, 0);
  SnapCols& cols = sn->cols;
  memset(&cols, 0, sizeof(cols));
  for (int c = 0; c < nc; ++c) {
    if (sc.value_cols[c].dtype == YBG_T_STRING) continue;
    val[c].assign(padded, 0);
    for (uint64_t r = 0; r < n; ++r)
      val[c][r] = dat_aos[(uint64_t)perm[r] * nc + c];
    cols.val[c] = val[c].data();
  }
  for (int c = 0; c < nk; ++c) {
    if (sc.key_types[c] == YBG_KT_STRING) continue;
    key[c].assign(padded, 0);
    for (uint64_t r = 0; r < n; ++r)
      key[c][r] = key_aos[(uint64_t)perm[r] * nk + c];
    cols.key[c] = key[c].data();
  }
  const uint32_t nc_mask = nc >= 32 ? 0xffffffffu : ((1u << nc) - 1u);
  for (uint64_t r = 0; r < n; ++r) {
    nullmask[r] = null_aos[perm[r]];
    cols.nullable_cols |= nullmask[r] & nc_mask;
  }
  cols.nullmask = nullmask.data();
  if (stage_strings) {
    // k_snap_str_len / exclusive scan / k_snap_str_pack, serially
    sn->sval.resize(nc);
    sn->skey.resize(nk);
    for (int pass = 0; pass < nk + nc; ++pass) {
      const bool is_key = pass < nk;
      const int c = is_key ? pass : pass - nk;
      if (is_key ? sc.key_types[c] != YBG_KT_STRING
                 : sc.value_cols[c].dtype != YBG_T_STRING)
        continue;
      const std::vector<uint64_t>& aos = is_key ? key_aos : dat_aos;
      const int stride = is_key ? nk : nc;
      SimSnapshot::Str& st = is_key ? sn->skey[c] : sn->sval[c];
      st.off.assign(n + 1, 0);
      st.pfx.assign(padded, 0);
      for (uint64_t r = 0; r < n; ++r)
        st.off[r + 1] =
            st.off[r] + (aos[(uint64_t)perm[r] * stride + c] >> 40);
      st.bytes.assign(st.off[n] + 16, 0);
      for (uint64_t r = 0; r < n; ++r) {
        const uint64_t d = aos[(uint64_t)perm[r] * stride + c];
        const uint64_t len = d >> 40;
        const uint8_t* src = heap.data() + (d & ((1ull << 40) - 1));
        if (len) memcpy(st.bytes.data() + st.off[r], src, len);
        st.pfx[r] = snap_str_prefix(src, len);
      }
      (is_key ? cols.skey[c] : cols.sval[c]) =
          SnapStrCol{st.off.data(), st.bytes.data(), st.pfx.data()};
    }
  }
  return 0;
}
}  // namespace

extern "C" {

// Columnar-snapshot simulator: the build (sim_snapshot_build) followed by
// the snap_device.h row loop, sequentially. `query` is a
// ybg_snapshot_query_t. Returns 9 for a query the ABI rejects (same
// translation code).
int ybg_sim_snapshot_query_ex(const ybg_scan_spec_t* spec,
                              const uint8_t* data, const uint64_t* offsets,
                              uint64_t n_blocks,
                              const ybg_snapshot_query_t* query,
                              int stage_strings, ybg_scan_result_t* out);

int ybg_sim_snapshot_query(const ybg_scan_spec_t* spec, const uint8_t* data,
                           const uint64_t* offsets, uint64_t n_blocks,
                           const ybg_snapshot_query_t* query,
                           ybg_scan_result_t* out) {
  return ybg_sim_snapshot_query_ex(spec, data, offsets, n_blocks, query, 0,
                                   out);
}

// stage_strings: the snapshot is built as yb_gpu_snapshot_build_ex builds it
// with that option.
int ybg_sim_snapshot_query_ex(const ybg_scan_spec_t* spec,
                              const uint8_t* data, const uint64_t* offsets,
                              uint64_t n_blocks,
                              const ybg_snapshot_query_t* query,
                              int stage_strings, ybg_scan_result_t* out) {
  SimSnapshot snap;
  int rc = sim_snapshot_build(spec, data, offsets, n_blocks, &snap,
                              stage_strings != 0);
  if (rc) return rc;
  const ybg_schema_t& sc = spec->schema;
  const SnapCols& cols = snap.cols;
  const uint64_t n = snap.n;
  const ybg_scan_result_t& stats = snap.stats;

  SnapQuery q;
  std::vector<uint8_t> aux;
  char err[192];
  rc = snap_build_query(sc, &cols, query->num_preds, query->preds,
                        query->num_aggs, query->aggs, n, &aux, &q, err,
                        sizeof(err));
  if (rc) return rc;
  q.aux = aux.data();
  SnapResult res;
  memset(&res, 0, sizeof(res));
  // row pairs in ascending order, as one device lane walks them; the
  // null-mask variant is chosen like the kernel dispatch chooses it
  const uint64_t n_pairs = (n + kSnapVec - 1) / kSnapVec;
  auto run = [&](auto nulls_tag, auto gen_tag) {
    constexpr bool NULLS = decltype(nulls_tag)::value;
    constexpr int GEN = decltype(gen_tag)::value;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
      for (int k = 0; k < kSnapVec; ++k) {
        const uint64_t r = pi * kSnapVec + k;
        uint64_t pv[YBG_MAX_PREDS] = {0}, av[YBG_MAX_AGGS] = {0};
        for (int i = 0; i < q.num_preds; ++i) pv[i] = q.preds[i].col[r];
        for (int g = 0; g < q.num_aggs; ++g)
          if (q.aggs[g].col) av[g] = q.aggs[g].col[r];
        snap_row<YBG_MAX_PREDS, YBG_MAX_AGGS, NULLS, GEN>(
            q, pv, av, NULLS ? q.nullmask[r] : 0u, r < n, r, &res.matched,
            res.agg_val, res.agg_cnt);
      }
    }
  };
  using Fast = std::integral_constant<int, kSnapGenFast>;
  using List = std::integral_constant<int, kSnapGenList>;
  using Str = std::integral_constant<int, kSnapGenStr>;
  if (q.any_nullable) {
    if (q.general == kSnapGenStr) run(std::true_type{}, Str{});
    else if (q.general) run(std::true_type{}, List{});
    else run(std::true_type{}, Fast{});
  } else {
    if (q.general == kSnapGenStr) run(std::false_type{}, Str{});
    else if (q.general) run(std::false_type{}, List{});
    else run(std::false_type{}, Fast{});
  }
  snap_fill_result(res, n, stats.entries_seen, stats.restart_ht,
                   stats.restart_ht_len, query->num_aggs, query->aggs, out);
  return 0;
}

}  // extern "C"

namespace {

// k_snap_group_query, one simulated workgroup at a time: workgroup w of
// snap_grid(n) walks the row pairs the device gives its 256 lanes
// (grid-stride included) into its own local table, then flushes it.
template <int NA, bool NULLS, int GEN, bool LOCAL>
void sim_group_rows(const SnapGroupQuery& gq, const GroupCtx& gc,
                    uint64_t* matched) {
  const SnapQuery& q = gq.q;
  const uint64_t n = q.n_rows;
  const uint64_t n_pairs = (n + kSnapVec - 1) / kSnapVec;
  const uint64_t grid = snap_grid(n);
  const uint64_t span = grid * kSnapThreads;
  std::vector<SnapLocalTable<NA>> tab_mem(LOCAL ? 1 : 0);
  SnapLocalTable<NA>* tab = LOCAL ? tab_mem.data() : nullptr;
  for (uint64_t w = 0; w < grid; ++w) {
    if (LOCAL) snap_local_init<NA>(q, tab, 0, 1);
    for (uint64_t t = 0; t < (uint64_t)kSnapThreads; ++t) {
      for (uint64_t pi = w * kSnapThreads + t; pi < n_pairs; pi += span) {
        for (int k = 0; k < kSnapVec; ++k) {
          const uint64_t r = pi * kSnapVec + k;
          uint64_t pv[YBG_MAX_PREDS] = {0}, av[NA] = {0};
          for (int i = 0; i < q.num_preds; ++i) pv[i] = q.preds[i].col[r];
          for (int g = 0; g < q.num_aggs; ++g)
            if (q.aggs[g].col) av[g] = q.aggs[g].col[r];
          snap_group_row<YBG_MAX_PREDS, NA, NULLS, GEN, LOCAL>(
              gq, pv, av, gq.grp_col[r], NULLS ? q.nullmask[r] : 0u, r < n,
              r, matched, tab, gc);
        }
      }
    }
    if (LOCAL)
      for (int i = 0; i <= SnapLocalTable<NA>::L; ++i)
        snap_local_flush_slot<NA>(q, tab, i, gc);
  }
}

template <int NA>
void sim_group_dispatch(const SnapGroupQuery& gq, const GroupCtx& gc,
                        bool local, uint64_t* matched) {
  // the string instantiation stands in for the list one here: it runs the
  // same pred_compare for a non-string slot
  const int v = (gq.q.any_nullable ? 4 : 0) | (gq.q.general ? 2 : 0) |
                (local ? 1 : 0);
  constexpr int G = kSnapGenStr;
  switch (v) {
    case 0: sim_group_rows<NA, false, 0, false>(gq, gc, matched); break;
    case 1: sim_group_rows<NA, false, 0, true>(gq, gc, matched); break;
    case 2: sim_group_rows<NA, false, G, false>(gq, gc, matched); break;
    case 3: sim_group_rows<NA, false, G, true>(gq, gc, matched); break;
    case 4: sim_group_rows<NA, true, 0, false>(gq, gc, matched); break;
    case 5: sim_group_rows<NA, true, 0, true>(gq, gc, matched); break;
    case 6: sim_group_rows<NA, true, G, false>(gq, gc, matched); break;
    default: sim_group_rows<NA, true, G, true>(gq, gc, matched); break;
  }
}

}  // namespace

extern "C" {

// Grouped columnar-snapshot simulator: yb_gpu_snapshot_group_query's
// contract (codes 8 / 9 included) from the same translation, accumulate,
// flush and export code, serially. The level is chosen from expect_groups
// like the device dispatch chooses it.
int ybg_sim_snapshot_group_query_ex(
    const ybg_scan_spec_t* spec, const uint8_t* data, const uint64_t* offsets,
    uint64_t n_blocks, const ybg_snapshot_group_query_t* query,
    int stage_strings, uint64_t* keys, int64_t* vals, uint64_t* cnts,
    uint64_t cap, ybg_snapshot_group_result_t* out);

int ybg_sim_snapshot_group_query(const ybg_scan_spec_t* spec,
                                 const uint8_t* data, const uint64_t* offsets,
                                 uint64_t n_blocks,
                                 const ybg_snapshot_group_query_t* query,
                                 uint64_t* keys, int64_t* vals,
                                 uint64_t* cnts, uint64_t cap,
                                 ybg_snapshot_group_result_t* out) {
  return ybg_sim_snapshot_group_query_ex(spec, data, offsets, n_blocks, query,
                                         0, keys, vals, cnts, cap, out);
}

// stage_strings: as in ybg_sim_snapshot_query_ex.
int ybg_sim_snapshot_group_query_ex(
    const ybg_scan_spec_t* spec, const uint8_t* data, const uint64_t* offsets,
    uint64_t n_blocks, const ybg_snapshot_group_query_t* query,
    int stage_strings, uint64_t* keys, int64_t* vals, uint64_t* cnts,
    uint64_t cap, ybg_snapshot_group_result_t* out) {
  memset(out, 0, sizeof(*out));
  SimSnapshot snap;
  int rc = sim_snapshot_build(spec, data, offsets, n_blocks, &snap,
                              stage_strings != 0);
  if (rc) return rc;
  const uint64_t n = snap.n;
  SnapGroupQuery gq;
  std::vector<uint8_t> aux;
  char err[192];
  rc = snap_build_group_query(spec->schema, &snap.cols, *query, n, &aux, &gq,
                              err, sizeof(err));
  if (rc) return rc;
  gq.q.aux = aux.data();
  out->rows_scanned = n;
  out->entries_seen = snap.stats.entries_seen;
  memcpy(out->restart_ht, snap.stats.restart_ht, snap.stats.restart_ht_len);
  out->restart_ht_len = snap.stats.restart_ht_len;
  const int na = snap_group_na(gq.q.num_aggs);
  const bool local = query->expect_groups <= (uint64_t)snap_group_local_slots(na);
  out->local_level = local ? 1 : 0;
  if (n == 0) return 0;

  // the snapshot's global table, initialized as k_snap_group_init does
  const uint64_t gcap = snap_group_table_cap(n);
  std::vector<unsigned long long> gkey(gcap + 1, 0);
  std::vector<unsigned> state(gcap + 1, 0);
  std::vector<long long> gvals((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned long long> gcnts((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned long long> vals_hi((gcap + 1) * YBG_MAX_AGGS, 0);
  std::vector<unsigned> poison((gcap + 1) * YBG_MAX_AGGS, 0);
  SnapOps ops;
  memset(&ops, 0, sizeof(ops));
  ops.num_aggs = gq.q.num_aggs;
  for (int g = 0; g < gq.q.num_aggs; ++g) ops.op[g] = gq.q.aggs[g].op;
  for (uint64_t i = 0; i <= gcap; ++i)
    for (int g = 0; g < ops.num_aggs; ++g)
      gvals[i * YBG_MAX_AGGS + g] = group_init_value(ops.op[g]);
  unsigned long long overflow = 0;
  GroupCtx gc;
  gc.gkey = gkey.data();
  gc.state = state.data();
  gc.vals = gvals.data();
  gc.cnts = gcnts.data();
  gc.vals_hi = vals_hi.data();
  gc.poison = poison.data();
  gc.cap = gcap;
  gc.overflow = &overflow;
  gc.data = nullptr;

  uint64_t matched = 0;
  switch (na) {
    case 2: sim_group_dispatch<2>(gq, gc, local, &matched); break;
    case 4: sim_group_dispatch<4>(gq, gc, local, &matched); break;
    default: sim_group_dispatch<8>(gq, gc, local, &matched); break;
  }
  if (overflow) return 8;
  out->rows_matched = matched;

  // export: occupied slots ordered by key (unsigned), the NULL group last
  std::vector<std::pair<uint64_t, uint64_t>> order;  // (key, slot)
  for (uint64_t i = 0; i < gcap; ++i)
    if (state[i] == 1) order.emplace_back(gkey[i], i);
  std::sort(order.begin(), order.end());
  const int has_null = state[gcap] == 1 ? 1 : 0;
  out->n_groups = order.size() + (uint64_t)has_null;
  out->has_null_group = has_null;
  if (out->n_groups > cap) return 8;
  for (uint64_t i = 0; i < order.size(); ++i)
    snap_group_export_slot(ops, gc, order[i].second, order[i].first, i, keys,
                           (long long*)vals, (unsigned long long*)cnts);
  if (has_null)
    snap_group_export_slot(ops, gc, gcap, 0, order.size(), keys,
                           (long long*)vals, (unsigned long long*)cnts);
  return 0;
}

}  // extern "C"

namespace {

// k_snap_select_count, one simulated tile at a time: the lanes' two row
// slots become the wave ballots, packed into the tile's bitmap words by the
// shared code.
template <bool NULLS, int GEN>
void sim_select_count(const SnapQuery& q, const SnapWindow& win,
                      uint64_t* bitmap, uint64_t* tile_cnt) {
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    const uint64_t tile = win.tile_lo + t;
    uint64_t cnt = 0;  // one 16-bit count per wave
    for (int wave = 0; wave < kSnapThreads / 64; ++wave) {
      uint64_t b[kSnapVec] = {0, 0};
      for (int lane = 0; lane < 64; ++lane) {
        const uint64_t r0 =
            tile * kSnapTileRows + (uint64_t)(wave * 64 + lane) * kSnapVec;
        const bool ld = r0 < win.hi && r0 + kSnapVec > win.lo;
        for (int k = 0; k < kSnapVec; ++k) {
          const uint64_t r = r0 + k;
          uint64_t pv[YBG_MAX_PREDS] = {0};
          if (ld)
            for (int i = 0; i < q.num_preds; ++i) pv[i] = q.preds[i].col[r];
          const bool m = snap_pred_pass<YBG_MAX_PREDS, NULLS, GEN>(
              q, pv, (NULLS && ld) ? q.nullmask[r] : 0u,
              r >= win.lo && r < win.hi, r);
          if (m) b[k] |= 1ull << lane;
        }
      }
      snap_select_pack(b[0], b[1], bitmap + tile * kSnapTileWords + wave * 2);
      cnt |= (uint64_t)(snap_popc64(b[0]) + snap_popc64(b[1]))
             << (16 * wave);
    }
    tile_cnt[t] = cnt;
  }
}

}  // namespace

extern "C" {

// The tile width the simulator walks (= ybg_snapshot_select_tile_rows; the
// stand-alone driver links no device code).
uint64_t ybg_sim_snapshot_select_tile_rows(void) { return kSnapTileRows; }

// Select simulator: yb_gpu_snapshot_select's contract (codes 8 / 9
// included) from the same translation, bit packing, rank, output index and
// emit code, the tiles walked serially.
int ybg_sim_snapshot_select_var(
    const ybg_scan_spec_t* spec, const uint8_t* data, const uint64_t* offsets,
    uint64_t n_blocks, const ybg_snapshot_select_t* query, int stage_strings,
    uint64_t* datums, uint32_t* null_masks, uint64_t* row_ids, uint64_t cap,
    uint8_t* varlen, uint64_t varlen_cap, uint64_t* varlen_size,
    ybg_snapshot_select_result_t* out);

int ybg_sim_snapshot_select(const ybg_scan_spec_t* spec, const uint8_t* data,
                            const uint64_t* offsets, uint64_t n_blocks,
                            const ybg_snapshot_select_t* query,
                            uint64_t* datums, uint32_t* null_masks,
                            uint64_t* row_ids, uint64_t cap,
                            ybg_snapshot_select_result_t* out) {
  return ybg_sim_snapshot_select_var(spec, data, offsets, n_blocks, query, 0,
                                     datums, null_masks, row_ids, cap,
                                     nullptr, 0, nullptr, out);
}

// yb_gpu_snapshot_select_var's contract on a snapshot built with or without
// stage_strings; varlen_size == nullptr: yb_gpu_snapshot_select's (a string
// projection is refused).
int ybg_sim_snapshot_select_var(
    const ybg_scan_spec_t* spec, const uint8_t* data, const uint64_t* offsets,
    uint64_t n_blocks, const ybg_snapshot_select_t* query, int stage_strings,
    uint64_t* datums, uint32_t* null_masks, uint64_t* row_ids, uint64_t cap,
    uint8_t* varlen, uint64_t varlen_cap, uint64_t* varlen_size,
    ybg_snapshot_select_result_t* out) {
  memset(out, 0, sizeof(*out));
  if (varlen_size) *varlen_size = 0;
  SimSnapshot snap;
  int rc = sim_snapshot_build(spec, data, offsets, n_blocks, &snap,
                              stage_strings != 0);
  if (rc) return rc;
  const uint64_t n_rows = snap.n;
  SnapQuery q;
  SnapSelect sel;
  std::vector<uint8_t> aux;
  char err[192];
  rc = snap_build_select(spec->schema, &snap.cols, *query, n_rows, &aux, &q,
                         &sel, err, sizeof(err), varlen_size != nullptr);
  if (rc) return rc;
  q.aux = aux.data();
  out->entries_seen = snap.stats.entries_seen;
  memcpy(out->restart_ht, snap.stats.restart_ht, snap.stats.restart_ht_len);
  out->restart_ht_len = snap.stats.restart_ht_len;
  const uint64_t hi = query->row_hi < n_rows ? query->row_hi : n_rows;
  const uint64_t lo = query->row_lo;
  SnapSelectHdr h = {0, 0, 0};
  if (lo >= hi) {
    snap_select_fill(lo, hi, h, sel.backward, 0, 0, out);
    return 0;
  }
  const SnapWindow win = snap_select_window(lo, hi);
  const uint64_t tiles = (n_rows + kSnapTileRows - 1) / kSnapTileRows;
  std::vector<uint64_t> bitmap(tiles * kSnapTileWords, 0);
  std::vector<uint64_t> tile_cnt(win.n_tiles);
  std::vector<uint32_t> tile_off(win.n_tiles);
  const int v = (q.any_nullable ? 2 : 0) | (q.general ? 1 : 0);
  // as in sim_group_dispatch: the string instantiation covers the lists
  switch (v) {
    case 0: sim_select_count<false, kSnapGenFast>(q, win, bitmap.data(),
                                                  tile_cnt.data()); break;
    case 1: sim_select_count<false, kSnapGenStr>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
    case 2: sim_select_count<true, kSnapGenFast>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
    default: sim_select_count<true, kSnapGenStr>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
  }
  // k_snap_select_scan, serially
  uint64_t total = 0;
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    tile_off[t] = (uint32_t)total;
    total += snap_select_tile_count(tile_cnt[t]);
  }
  snap_select_range(total, query->row_limit, sel.backward, &h);
  const uint64_t n = h.end - h.first;
  if (n > cap) {
    snap_select_fill(lo, hi, h, sel.backward, 0, 0, out);
    out->done = 0;
    out->resume_row = 0;
    return 8;
  }
  if (n == 0) {
    snap_select_fill(lo, hi, h, sel.backward, 0, 0, out);
    return 0;
  }
  // k_snap_select_gather: straight into the caller's arrays (pitch cap)
  const SnapSelectOut so = {row_ids, null_masks, datums, cap};
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    const uint64_t off = tile_off[t];
    const uint64_t cnt = snap_select_tile_count(tile_cnt[t]);
    if (cnt == 0 || off + cnt <= h.first || off >= h.end) continue;
    const uint64_t tile = win.tile_lo + t;
    for (uint32_t lane = 0; lane < (uint32_t)kSnapThreads; ++lane)
      snap_select_gather_pair(sel, so, h, bitmap.data() + tile * kSnapTileWords,
                              tile, off, lane * kSnapVec);
  }
  if (sel.num_str) {
    // k_snap_select_strlen / exclusive scan / k_snap_select_strcopy
    std::vector<uint64_t> row_off(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i)
      row_off[i + 1] = row_off[i] + snap_select_row_strlen(sel, so, i);
    *varlen_size = row_off[n];
    if (row_off[n] > varlen_cap) {
      snap_select_fill(lo, hi, h, sel.backward, 0, 0, out);
      out->done = 0;
      out->resume_row = 0;
      return 8;
    }
    for (uint64_t i = 0; i < n; ++i)
      snap_select_strcopy_row(sel, so, i, row_off[i], varlen);
  }
  snap_select_fill(lo, hi, h, sel.backward, row_ids[n - 1], row_ids[n - 1],
                   out);
  return 0;
}

}  // extern "C"

namespace {

// The simulated lane (tile, lane): its two match bits and row pair, as
// snap_order_load hands them to the kernels.
struct SimOrderLane {
  uint32_t two;
  uint64_t r0, v[kSnapVec];
  uint32_t nm[kSnapVec];
};

SimOrderLane sim_order_load(const SnapOrder& o, const uint64_t* bitmap,
                            uint64_t tile, uint32_t lane) {
  SimOrderLane l;
  const uint32_t b = lane * kSnapVec;
  const uint64_t w = bitmap[tile * kSnapTileWords + (b >> 6)];
  l.two = (uint32_t)(w >> (b & 63)) & 3u;
  l.r0 = tile * kSnapTileRows + b;
  for (int k = 0; k < kSnapVec; ++k) {
    l.v[k] = l.two ? o.col[l.r0 + k] : 0;
    l.nm[k] = (l.two && o.nullmask) ? o.nullmask[l.r0 + k] : 0u;
  }
  return l;
}

// k_snap_order_hist, the tiles walked serially.
void sim_order_hist(const SnapOrder& o, const SnapWindow& win, int pass,
                    const SnapOrderState& st, const uint64_t* bitmap,
                    const uint64_t* tile_cnt, uint64_t* bins) {
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    if (tile_cnt[t] == 0) continue;
    for (uint32_t lane = 0; lane < (uint32_t)kSnapThreads; ++lane) {
      const SimOrderLane l = sim_order_load(o, bitmap, win.tile_lo + t, lane);
      for (int k = 0; k < kSnapVec; ++k) {
        SnapOrderKey key;
        if (snap_order_row(o, l.v[k], l.nm[k], l.r0 + k, (l.two >> k) & 1u,
                           &key) &&
            snap_order_in_bucket(key, st))
          ++bins[snap_order_digit(key, pass)];
      }
    }
  }
}

// k_snap_order_fix, serially; the bins are left zeroed.
void sim_order_fix(int pass, uint64_t limit, uint64_t* bins,
                   SnapOrderState* st) {
  uint64_t total = 0;
  for (int i = 0; i < kSnapOrderBins; ++i) total += bins[i];
  const bool go = pass != 0 || snap_order_begin(st, total, limit);
  uint64_t excl = 0;
  for (int i = 0; i < kSnapOrderBins && go; ++i) {
    const uint64_t cnt = bins[i];
    if (cnt && excl < st->k && st->k <= excl + cnt) {
      snap_order_advance(st, pass, (uint32_t)i, excl, cnt);
      break;
    }
    excl += cnt;
  }
  for (int i = 0; i < kSnapOrderBins; ++i) bins[i] = 0;
}

// k_snap_order_mark + k_snap_select_scan; returns the selected total.
uint64_t sim_order_mark(const SnapOrder& o, const SnapWindow& win,
                        const SnapOrderState& st, const uint64_t* bitmap,
                        const uint64_t* tile_cnt, uint64_t* sel_bitmap,
                        uint64_t* sel_cnt, uint32_t* tile_off) {
  uint64_t total = 0;
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    const uint64_t tile = win.tile_lo + t;
    uint64_t cnt = 0;
    for (int wave = 0; wave < kSnapThreads / 64 && tile_cnt[t]; ++wave) {
      uint64_t b[kSnapVec] = {0, 0};
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const SimOrderLane l =
            sim_order_load(o, bitmap, tile, (uint32_t)wave * 64 + lane);
        for (int k = 0; k < kSnapVec; ++k) {
          SnapOrderKey key;
          if (snap_order_row(o, l.v[k], l.nm[k], l.r0 + k, (l.two >> k) & 1u,
                             &key) &&
              snap_order_selected(key, st))
            b[k] |= 1ull << lane;
        }
      }
      snap_select_pack(b[0], b[1],
                       sel_bitmap + tile * kSnapTileWords + wave * 2);
      cnt |= (uint64_t)(snap_popc64(b[0]) + snap_popc64(b[1])) << (16 * wave);
    }
    sel_cnt[t] = cnt;
    tile_off[t] = (uint32_t)total;
    total += snap_select_tile_count(cnt);
  }
  return total;
}

}  // namespace

extern "C" {

// Ordered-select simulator: yb_gpu_snapshot_select_ordered's contract (codes
// 8 / 9 included) from the same key, digit, state, gather and emit code; the
// tiles are walked serially and std::stable_sort stands in for the device
// radix sort. Honours YBG_SNAP_ORDER_CAND.
int ybg_sim_snapshot_select_ordered(
    const ybg_scan_spec_t* spec, const uint8_t* data, const uint64_t* offsets,
    uint64_t n_blocks, const ybg_snapshot_order_t* query, int stage_strings,
    uint64_t* datums, uint32_t* null_masks, uint64_t* row_ids, uint64_t cap,
    uint8_t* varlen, uint64_t varlen_cap, uint64_t* varlen_size,
    ybg_snapshot_order_result_t* out) {
  memset(out, 0, sizeof(*out));
  uint64_t vs_local = 0;
  if (!varlen_size) varlen_size = &vs_local;
  *varlen_size = 0;
  SimSnapshot snap;
  int rc = sim_snapshot_build(spec, data, offsets, n_blocks, &snap,
                              stage_strings != 0);
  if (rc) return rc;
  const uint64_t n_rows = snap.n;
  SnapQuery q;
  SnapSelect sel;
  SnapOrder ord;
  std::vector<uint8_t> aux;
  char err[192];
  rc = snap_build_order(spec->schema, &snap.cols, *query, n_rows, &aux, &q,
                        &sel, &ord, err, sizeof(err));
  if (rc) return rc;
  q.aux = aux.data();
  out->r.entries_seen = snap.stats.entries_seen;
  memcpy(out->r.restart_ht, snap.stats.restart_ht,
         snap.stats.restart_ht_len);
  out->r.restart_ht_len = snap.stats.restart_ht_len;
  const uint64_t hi = query->sel.row_hi < n_rows ? query->sel.row_hi : n_rows;
  const uint64_t lo = query->sel.row_lo;
  if (lo >= hi) {
    snap_order_fill(lo, hi, 0, 0, 0, nullptr, out);
    return 0;
  }
  const uint64_t limit = query->sel.row_limit;
  const uint64_t cand = snap_order_cand_env();
  const SnapWindow win = snap_select_window(lo, hi);
  const uint64_t tiles = (n_rows + kSnapTileRows - 1) / kSnapTileRows;
  std::vector<uint64_t> bitmap(tiles * kSnapTileWords, 0);
  std::vector<uint64_t> sel_bitmap(tiles * kSnapTileWords, 0);
  std::vector<uint64_t> tile_cnt(win.n_tiles), sel_cnt(win.n_tiles);
  std::vector<uint32_t> tile_off(win.n_tiles);
  const int v = (q.any_nullable ? 2 : 0) | (q.general ? 1 : 0);
  switch (v) {
    case 0: sim_select_count<false, kSnapGenFast>(q, win, bitmap.data(),
                                                  tile_cnt.data()); break;
    case 1: sim_select_count<false, kSnapGenStr>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
    case 2: sim_select_count<true, kSnapGenFast>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
    default: sim_select_count<true, kSnapGenStr>(q, win, bitmap.data(),
                                                 tile_cnt.data()); break;
  }
  SnapOrderState st;
  memset(&st, 0, sizeof(st));
  uint64_t bins[kSnapOrderBins] = {0};
  // eligible rows: the matches, or with a cursor the matches after it
  bool marked = ord.have_cursor != 0;
  uint64_t eligible = 0;
  if (marked) {
    eligible = sim_order_mark(ord, win, st, bitmap.data(), tile_cnt.data(),
                              sel_bitmap.data(), sel_cnt.data(),
                              tile_off.data());
  } else {
    for (uint64_t t = 0; t < win.n_tiles; ++t) {
      tile_off[t] = (uint32_t)eligible;
      eligible += snap_select_tile_count(tile_cnt[t]);
    }
  }
  const uint64_t n = (limit && limit < eligible) ? limit : eligible;
  if (n > cap) {
    snap_order_fill(lo, hi, n, eligible, 0, nullptr, out);
    out->r.done = 0;
    return 8;
  }
  if (n == 0) {
    snap_order_fill(lo, hi, 0, 0, 0, nullptr, out);
    return 0;
  }
  uint32_t passes = 0;
  uint64_t c = eligible;
  if (n < eligible) {
    for (int pass = 0; pass < kSnapOrderPasses; ++pass) {
      sim_order_hist(ord, win, pass, st, bitmap.data(), tile_cnt.data(), bins);
      sim_order_fix(pass, limit, bins, &st);
      ++passes;
      if (!snap_order_more(st, limit, cand)) break;
    }
    c = sim_order_mark(ord, win, st, bitmap.data(), tile_cnt.data(),
                       sel_bitmap.data(), sel_cnt.data(), tile_off.data());
    marked = true;
  }
  if (c < n) return 10;
  // k_snap_order_gather, the sort(s), k_snap_order_emit
  std::vector<uint64_t> ckey(c), cval(c);
  const uint64_t* gb = marked ? sel_bitmap.data() : bitmap.data();
  const uint64_t* gc = marked ? sel_cnt.data() : tile_cnt.data();
  for (uint64_t t = 0; t < win.n_tiles; ++t) {
    if (snap_select_tile_count(gc[t]) == 0) continue;
    const uint64_t tile = win.tile_lo + t;
    for (uint32_t lane = 0; lane < (uint32_t)kSnapThreads; ++lane)
      snap_order_gather_pair(ord, gb + tile * kSnapTileWords, tile,
                             tile_off[t], lane * kSnapVec, ckey.data(),
                             cval.data());
  }
  std::vector<uint64_t> idx(c);
  for (uint64_t i = 0; i < c; ++i) idx[i] = i;
  std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
    return ckey[a] < ckey[b];
  });
  if (ord.nullmask)
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
      return (cval[a] >> 32) < (cval[b] >> 32);
    });
  const SnapSelectOut so = {row_ids, null_masks, datums, cap};
  SnapOrderCursor cur;
  memset(&cur, 0, sizeof(cur));
  for (uint64_t i = 0; i < n; ++i)
    snap_order_emit(ord, sel, so, cval[idx[i]], i, n, &cur);
  if (sel.num_str) {
    std::vector<uint64_t> row_off(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i)
      row_off[i + 1] = row_off[i] + snap_select_row_strlen(sel, so, i);
    *varlen_size = row_off[n];
    if (row_off[n] > varlen_cap) {
      snap_order_fill(lo, hi, n, eligible, passes, nullptr, out);
      out->r.done = 0;
      return 8;
    }
    for (uint64_t i = 0; i < n; ++i)
      snap_select_strcopy_row(sel, so, i, row_off[i], varlen);
  }
  snap_order_fill(lo, hi, n, eligible, passes, &cur, out);
  return 0;
}

}  // extern "C"
