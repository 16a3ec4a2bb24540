// yugabyte-db_amd/csrc/scan_gpu.hip — CDNA4 (gfx950) kernels + host ABI for
// the DocDB SST-block scan-and-filter hot path.
//
// What the GPU replaces (reference yugabyte/yugabyte-db):
//   BlockIter::ParseNextKey delta decode   rocksdb/table/block.cc:287-454
//   SkipFutureRecords MVCC visibility      docdb/intent_aware_iterator.cc:1223-1317
//   FlatGetHelper row assembly             docdb/doc_reader.cc:1826-1925
//   packed row decode V1/V2                dockv/schema_packing.cc:489-497,1043-1121
//   FilteringIterator::CheckFilter         docdb/pgsql_operation.cc:602-668
//   EvalAggregate / DoEvalTSCall           docdb/doc_expr.cc:248-395
//
// Execution model (MI355X-first; HBM-bound integer/byte work — MFMA unused):
//  * Parallel unit = one RESTART INTERVAL (16 entries, rocksdb/table.h:150).
//    The per-entry key delta chain is serial inside an interval; a 100M-row
//    tablet has ~6M intervals >> the ~1M threads of a full launch, so one
//    THREAD per interval with a contiguous grid-stride mapping (adjacent
//    lanes = adjacent intervals => a wave streams a contiguous span of the
//    block array through L1/L2).
//  * Reconstructed keys live in LDS (128 B/thread); the finalized row's key
//    bytes are saved to a per-thread global scratch (L1-resident) because
//    the in-place delta update destroys them.
//  * Rows straddling interval boundaries, with NO inter-workgroup sync:
//    every interval DEFERS its first (head) row — ownership unknown — and
//    WALKS its last (tail) row forward across interval/block boundaries.
//    After the pass, lane l learns from lane l-1 (shfl / LDS relay) whether
//    its head row was already consumed by the predecessor's walk; only
//    intervals at workgroup boundaries (1 in 256) write a global head record
//    + continuation flag, folded by the final reduction.
//  * The fold (k_fold; k_reduce on the grouped scan) combines wave partials
//    and head records IN FIXED ORDER => results (including double SUM) are
//    deterministic run-to-run.
//
// The per-interval algorithm itself lives in scan_device.h and is also
// compiled into a host simulator (scan_host_sim.cc) for CPU-side testing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "scan_device.h"
#include "snap_internal.h"
#include "sst_internal.h"
#include "bloom_filter.h"
#include "snappy_dev.h"
#include "lz4_dev.h"

using namespace ybgdev;

namespace {

// The spec lives in constant memory: its fields are read throughout the hot
// loop, and passing it by value made the compiler hold/spill hundreds of
// SGPRs per wave (PMC showed ~19.6 GB of scratch write traffic per 100M-row
// dispatch from the spill save/restore around the interval loop).
__constant__ DevSpec c_spec;

// ---------------------------------------------------------------------------
// Scaffolding shared by the scan kernels
// ---------------------------------------------------------------------------

// batch j = ivb CONSECUTIVE intervals — or one BLOCK's intervals when
// batch_lo is set (block-aligned batches keep lanes phase-locked on the
// 16-entry restart cadence)
__device__ __forceinline__ void batch_bounds(
    const uint64_t* __restrict__ batch_lo, uint64_t j, uint64_t ivb,
    uint64_t n_ivs, uint64_t* lo, uint64_t* hi) {
  *lo = batch_lo ? batch_lo[j] : j * ivb;
  *hi = batch_lo ? batch_lo[j + 1] : *lo + ivb;
  if (*hi > n_ivs) *hi = n_ivs;
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int off) {
  return (uint64_t)__shfl_down((unsigned long long)v, off);
}

// Wave restart-minimum into the wave's partial record, run by lane 0:
// lane l's candidate {hi, lo, len} sits at slots[(tid + l) * stride + off]
// (cold: len == 0 for every lane unless track_restart saw candidates).
__device__ __forceinline__ void wave_restart_min(
    const uint64_t* slots, int stride, int off, uint64_t* __restrict__ prec) {
  uint64_t mh = 0, ml = 0, mn = 0;
  for (int l = 0; l < 64; ++l) {
    const uint64_t* rr = slots + (size_t)(threadIdx.x + l) * stride + off;
    if (rr[2] == 0) continue;
    if (mn == 0 || u128_slice_cmp(rr[0], rr[1], (uint32_t)rr[2], mh, ml,
                                  (uint32_t)mn) < 0) {
      mh = rr[0];
      ml = rr[1];
      mn = rr[2];
    }
  }
  prec[4 + 2 * YBG_MAX_AGGS] = mh;
  prec[4 + 2 * YBG_MAX_AGGS + 1] = ml;
  prec[4 + 2 * YBG_MAX_AGGS + 2] = mn;
}

// Kernel epilogue: fold the wave's counters and aggregates into its partial
// record (fixed lane order => deterministic), then the restart minimum.
// Called by every thread of the block; red_val / red_cnt are kThreads-sized
// LDS arrays.
template <int NA>
__device__ __forceinline__ void wave_fold_partials(
    const DevSpec& sp, uint32_t entries, uint32_t scanned, uint32_t matched,
    uint32_t errs, const uint64_t* agg_val, const uint64_t* agg_cnt,
    uint64_t* red_val, uint64_t* red_cnt, const uint64_t* rslots,
    int rstride, int roff, uint64_t* __restrict__ partials) {
  unsigned lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    entries += __shfl_down(entries, off);
    scanned += __shfl_down(scanned, off);
    matched += __shfl_down(matched, off);
    errs += __shfl_down(errs, off);
  }
  uint64_t wave_id = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  uint64_t* prec = partials + wave_id * kPartialStride;
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    if (g >= sp.num_aggs) continue;
    red_val[threadIdx.x] = agg_val[g];
    red_cnt[threadIdx.x] = agg_cnt[g];
    __syncthreads();
    if (lane == 0) {
      uint64_t av = 0, ac = 0;
      for (int l = 0; l < 64; ++l)
        combine1(sp.agg_op[g], &av, &ac, red_val[threadIdx.x + l],
                 red_cnt[threadIdx.x + l]);
      prec[4 + 2 * g] = av;
      prec[4 + 2 * g + 1] = ac;
    }
    __syncthreads();
  }
  if (lane == 0) {
    prec[0] = entries;
    prec[1] = scanned;
    prec[2] = matched;
    prec[3] = errs;
    wave_restart_min(rslots, rstride, roff, prec);
  }
}

// ---------------------------------------------------------------------------
// Phase-1 scan kernel (aggregate mode): one thread per interval
// ---------------------------------------------------------------------------

// Head resolution is GLOBAL: every batch writes its deferred head record
// (compact 2*NA+2 u64 stride) and its state byte (scan_device.h
// kBatchWalked | kBatchHeadPending); k_fold adds the pending head records
// whose predecessor batch did not walk into them. No relay, no
// syncthreads, and batches may be processed by ANY kernel in any launch
// (the fast kernel + its retry pass rely on this). The planned fast kernel
// resolves most heads inside the wave and leaves only the rest pending.
// retry_ids/retry_n, when set, make the kernel process only the listed
// batches (the fast kernel's aborts).
template <int NA, int WPS>
__global__ __launch_bounds__(kThreads, WPS) void k_scan(
    const uint8_t* __restrict__ data,
    const uint64_t* __restrict__ block_offsets,
    const Interval* __restrict__ ivs, uint64_t n_ivs,
    const uint8_t* __restrict__ aux, uint8_t* __restrict__ rk_save_buf,
    uint64_t* __restrict__ partials, uint64_t* __restrict__ bheads,
    uint8_t* __restrict__ walked, uint32_t* __restrict__ iv_flags,
    int write_all_flags, uint64_t ivb, uint64_t n_bat,
    const uint64_t* __restrict__ batch_lo,
    const uint64_t* __restrict__ retry_ids,
    const unsigned long long* __restrict__ retry_n) {
  const DevSpec& sp = c_spec;
  __shared__ uint8_t key_scratch[kThreads * kKeyCap];
  __shared__ uint64_t bht_scratch[kThreads * 6];
  uint8_t* key = key_scratch + (size_t)threadIdx.x * kKeyCap;
  uint64_t* bht = bht_scratch + (size_t)threadIdx.x * 6;
  bht[5] = 0;  // restart-min slot empty (bht[3..5] = {hi, lo, len})
  const uint32_t gtid = blockIdx.x * kThreads + threadIdx.x;
  uint8_t* rk_save = rk_save_buf + (size_t)gtid * kKeyCap;
  const uint64_t span = (uint64_t)gridDim.x * kThreads;
  const uint64_t n_work = retry_ids ? *retry_n : n_bat;
  constexpr int kHS = 2 * NA + 2;  // bheads stride

  uint32_t entries = 0, scanned = 0, matched = 0, errs = 0;
  // NA-sized and only ever constant-indexed (all loops over them unrolled):
  // any runtime index would force these accumulators into scratch memory,
  // and with them every per-row aggregate update in the hot loop (measured
  // as ~19.6 GB/dispatch of scratch write traffic before this was fixed).
  uint64_t agg_val[NA], agg_cnt[NA];
#pragma unroll
  for (int g = 0; g < NA; ++g) { agg_val[g] = 0; agg_cnt[g] = 0; }

  for (uint64_t i0 = gtid; i0 < n_work; i0 += span) {
    const uint64_t j = retry_ids ? retry_ids[i0] : i0;
    HeadOut<NA> ho;
    bool walked_next = false;
    uint64_t lo, hi;
    batch_bounds(batch_lo, j, ivb, n_ivs, &lo, &hi);
    if (!scan_one_interval<NA>(sp, data, block_offsets, ivs, n_ivs, lo, hi,
                               aux, key, rk_save, bht, &entries, &scanned,
                               &matched, agg_val, agg_cnt, &ho,
                               &walked_next,
                               write_all_flags ? iv_flags : nullptr)) {
      errs += 1;
    }
    // head record + walked flag, written out here and in k_scan_fast: moved
    // into a shared inline function (any signature) these nine lines changed
    // both kernels' register allocation, and k_scan_fast<3,4,false> went
    // from 3 to 4 waves/SIMD
    uint64_t* hr = bheads + j * kHS;
#pragma unroll
    for (int g = 0; g < NA; ++g) {
      hr[2 * g] = ho.val[g];
      hr[2 * g + 1] = ho.cnt[g];
    }
    hr[2 * NA] = ho.scanned;
    hr[2 * NA + 1] = ho.matched;
    walked[j] = kBatchHeadPending | (walked_next ? kBatchWalked : 0);
  }

  __shared__ uint64_t red_val[kThreads], red_cnt[kThreads];
  wave_fold_partials<NA>(sp, entries, scanned, matched, errs, agg_val,
                         agg_cnt, red_val, red_cnt, bht_scratch, 6, 3,
                         partials);
}

// ---------------------------------------------------------------------------
// Specialized fast kernel (scan_batch_fast body): NA = 2, small LDS
// footprint (80 B of rowkey scratch + 3 restart slots per thread), no
// rk_save, no relay. Batches outside the fast shape are appended to the
// retry list and re-run by k_scan in retry mode; head resolution is the
// same global bheads/walked protocol.
// ---------------------------------------------------------------------------

// known_bits, when set, is the handle's remembered abort set (one bit per
// batch): a listed batch is skipped at once, the general kernel is already
// running it from the known list (see "Known abort set" in the host code).
// A wave's 64 batches share one word.
__device__ __forceinline__ bool batch_known(
    const uint64_t* __restrict__ known_bits, uint64_t j) {
  return known_bits && ((known_bits[j >> 6] >> (j & 63)) & 1);
}

// PLAN: the packed-row pass runs from a compiled column plan that arrives
// by value in the kernarg segment (scan_device.h FastPlan); the
// interpreted kernel takes an empty struct in its place.
struct NoPlan {};
template <bool PLAN>
using PlanArg = std::conditional_t<PLAN, FastPlan, NoPlan>;

template <int WPS, int NC, bool FUSE = false, bool PLAN = false>
__global__ __launch_bounds__(kThreads, WPS) void k_scan_fast(
    const uint8_t* __restrict__ data,
    const uint64_t* __restrict__ block_offsets,
    const Interval* __restrict__ ivs, uint64_t n_ivs,
    uint64_t* __restrict__ partials, uint64_t* __restrict__ bheads,
    uint8_t* __restrict__ walked, uint64_t ivb, uint64_t n_bat,
    const uint64_t* __restrict__ batch_lo,
    uint64_t* __restrict__ retry_ids,
    unsigned long long* __restrict__ retry_n,
    const uint64_t* __restrict__ known_bits, const PlanArg<PLAN> plan) {
  const DevSpec& sp = c_spec;
  const FastPlan* pl = nullptr;
  if constexpr (PLAN) pl = &plan;
  // 16-byte aligned: the restart decode reads and writes a lane's slot in
  // aligned 8- and 16-byte LDS accesses (kFastKeyCap is a multiple of 16)
  __shared__ __attribute__((aligned(16))) uint8_t
      key_scratch[kThreads * kFastKeyCap];
  __shared__ uint64_t rmin_scratch[kThreads * 3];
  uint8_t* key = key_scratch + (size_t)threadIdx.x * kFastKeyCap;
  uint64_t* rmin = rmin_scratch + (size_t)threadIdx.x * 3;
  rmin[2] = 0;
  const uint32_t gtid = blockIdx.x * kThreads + threadIdx.x;
  const uint64_t span = (uint64_t)gridDim.x * kThreads;
  constexpr int NA = 2;
  constexpr int kHS = 2 * NA + 2;

  uint32_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[NA], agg_cnt[NA];
#pragma unroll
  for (int g = 0; g < NA; ++g) { agg_val[g] = 0; agg_cnt[g] = 0; }

  if constexpr (PLAN) {
    // Heads resolved inside the wave. span is a multiple of the wave size,
    // so lane l holds batch j and lane l-1 batch j-1 in every pass: the
    // loop is wave-uniform (an active flag, no early exit) so the shuffles
    // run converged. Every plan slot is an additive wrapping int64
    // (SUM_INT64, COUNT, COUNT(*)), so adding a head row here instead of in
    // the fold cannot change a bit of the result. Only heads whose
    // predecessor is in another wave or did not complete here go through
    // the global record.
    const unsigned lane = threadIdx.x & 63;
    for (uint64_t j0 = 0; j0 < n_bat; j0 += span) {
      const uint64_t j = j0 + gtid;
      HeadOut<NA> ho;
      bool walked_next = false;
      bool ok = false;
      if (j < n_bat && !batch_known(known_bits, j)) {
        uint64_t lo, hi;
        batch_bounds(batch_lo, j, ivb, n_ivs, &lo, &hi);
        ok = scan_batch_fast<NA, NC, FUSE, PLAN>(
            sp, data, block_offsets, ivs, n_ivs, lo, hi, key, rmin, &entries,
            &scanned, &matched, agg_val, agg_cnt, &ho, &walked_next, pl);
        if (!ok) {
          unsigned long long slot = atomicAdd(retry_n, 1ull);
          retry_ids[slot] = j;
        }
      }
      const int wn = (ok && walked_next) ? 1 : 0;
      const int p_ok = __shfl_up(ok ? 1 : 0, 1);
      const int p_wn = __shfl_up(wn, 1);
      const HeadAction act = head_action(lane, ok, p_ok != 0, p_wn != 0);
      if (act == kHeadFold) {
        scanned += ho.scanned;
        matched += ho.matched;
#pragma unroll
        for (int g = 0; g < NA; ++g) {
          agg_val[g] += ho.val[g];
          agg_cnt[g] += ho.cnt[g];
        }
      } else if (act == kHeadWrite) {
        uint64_t* hr = bheads + j * kHS;
#pragma unroll
        for (int g = 0; g < NA; ++g) {
          hr[2 * g] = ho.val[g];
          hr[2 * g + 1] = ho.cnt[g];
        }
        hr[2 * NA] = ho.scanned;
        hr[2 * NA + 1] = ho.matched;
      }
      if (ok)
        walked[j] = (uint8_t)(wn | (act == kHeadWrite ? kBatchHeadPending : 0));
    }
  } else {
    for (uint64_t j = gtid; j < n_bat; j += span) {
      if (batch_known(known_bits, j)) continue;
      HeadOut<NA> ho;
      bool walked_next = false;
      uint64_t lo, hi;
      batch_bounds(batch_lo, j, ivb, n_ivs, &lo, &hi);
      if (!scan_batch_fast<NA, NC, FUSE, PLAN>(
              sp, data, block_offsets, ivs, n_ivs, lo, hi, key, rmin,
              &entries, &scanned, &matched, agg_val, agg_cnt, &ho,
              &walked_next, pl)) {
        unsigned long long slot = atomicAdd(retry_n, 1ull);
        retry_ids[slot] = j;
        continue;
      }
      uint64_t* hr = bheads + j * kHS;
#pragma unroll
      for (int g = 0; g < NA; ++g) {
        hr[2 * g] = ho.val[g];
        hr[2 * g + 1] = ho.cnt[g];
      }
      hr[2 * NA] = ho.scanned;
      hr[2 * NA + 1] = ho.matched;
      walked[j] = kBatchHeadPending | (walked_next ? kBatchWalked : 0);
    }
  }

  // errs = 0: the fast scanner aborts a batch instead of failing it
  if constexpr (PLAN) {
    // Every plan slot is a wrapping 64-bit add (the in-wave head fold above
    // already depends on it), so a shuffle tree gives the bits the serial
    // lane-order fold gave: no LDS round trip, no barrier, no operator
    // switch. Same record layout, k_fold reads it unchanged.
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      entries += __shfl_down(entries, off);
      scanned += __shfl_down(scanned, off);
      matched += __shfl_down(matched, off);
#pragma unroll
      for (int g = 0; g < NA; ++g) {
        agg_val[g] += shfl_down_u64(agg_val[g], off);
        agg_cnt[g] += shfl_down_u64(agg_cnt[g], off);
      }
    }
    const unsigned lane = threadIdx.x & 63;
    const uint64_t wave_id =
        ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    uint64_t* prec = partials + wave_id * kPartialStride;
    if (lane == 0) {
      prec[0] = entries;
      prec[1] = scanned;
      prec[2] = matched;
      prec[3] = 0;
#pragma unroll
      for (int g = 0; g < NA; ++g) {
        // slots the query does not use stay as the serial fold leaves them
        if (g >= sp.num_aggs) continue;
        prec[4 + 2 * g] = agg_val[g];
        prec[4 + 2 * g + 1] = agg_cnt[g];
      }
    }
    // restart minimum: cold, a candidate exists only when track_restart saw
    // one. Lane 0 reads slots its own wave's lanes wrote, so a wave-scope
    // fence orders them; no workgroup barrier.
    if (__any(rmin[2] != 0)) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (lane == 0) wave_restart_min(rmin_scratch, 3, 0, prec);
    } else if (lane == 0) {
      prec[4 + 2 * YBG_MAX_AGGS] = 0;
      prec[4 + 2 * YBG_MAX_AGGS + 1] = 0;
      prec[4 + 2 * YBG_MAX_AGGS + 2] = 0;
    }
  } else {
    __shared__ uint64_t red_val[kThreads], red_cnt[kThreads];
    wave_fold_partials<NA>(sp, entries, scanned, matched, 0, agg_val,
                           agg_cnt, red_val, red_cnt, rmin_scratch, 3, 0,
                           partials);
  }
}

// ---------------------------------------------------------------------------
// Row-emission kernel (next_batch): a flags pre-pass (k_scan with
// write_all_flags) resolves head-row ownership for every interval; this
// kernel then re-walks intervals and materializes matching rows. 128-thread
// workgroups: each thread carries key scratch + a row buffer in LDS.
// ---------------------------------------------------------------------------

constexpr int kEmitThreads = 128;

// Row buffers live in DYNAMIC shared memory sized to the actual column
// count at launch: the static worst-case (kEmitThreads * YBG_MAX_COLS
// datum + length slots = 64 KB) pinned the kernel at 1 wave/SIMD; a
// 4-column schema now fits ~4 workgroups per CU.
__global__ __launch_bounds__(kEmitThreads) void k_emit(
    const uint8_t* __restrict__ data,
    const uint64_t* __restrict__ block_offsets,
    const Interval* __restrict__ ivs, uint64_t n_ivs,
    const uint8_t* __restrict__ aux, uint8_t* __restrict__ rk_save_buf,
    EmitCtx ec, unsigned long long* __restrict__ err_counter, int nc_pad) {
  const DevSpec& sp = c_spec;
  __shared__ uint8_t key_scratch[kEmitThreads * kKeyCap];
  __shared__ uint64_t bht_scratch[kEmitThreads * 6];
  extern __shared__ uint64_t emit_dyn[];  // rowbuf | lenbuf
  uint64_t* rowbuf = emit_dyn;
  uint32_t* lenbuf = (uint32_t*)(emit_dyn + (size_t)kEmitThreads * nc_pad);
  uint64_t* bht = bht_scratch + (size_t)threadIdx.x * 6;
  bht[5] = 0;
  uint8_t* key = key_scratch + (size_t)threadIdx.x * kKeyCap;
  uint64_t* rb = rowbuf + (size_t)threadIdx.x * nc_pad;
  uint32_t* lb = lenbuf + (size_t)threadIdx.x * nc_pad;
  const uint32_t gtid = blockIdx.x * kEmitThreads + threadIdx.x;
  uint8_t* rk_save = rk_save_buf + (size_t)gtid * kKeyCap;
  const uint64_t span = (uint64_t)gridDim.x * kEmitThreads;

  uint32_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[2] = {0, 0}, agg_cnt[2] = {0, 0};
  for (uint64_t j = gtid; j < n_ivs; j += span) {
    HeadOut<2> ho;
    bool wn = false;
    if (!scan_one_interval<2, true>(sp, data, block_offsets, ivs, n_ivs, j,
                                    j + 1, aux, key, rk_save, bht, &entries,
                                    &scanned, &matched, agg_val, agg_cnt,
                                    &ho, &wn, nullptr, &ec, rb, lb)) {
      atomicAdd(err_counter, 1ull);
    }
  }
}

// ---------------------------------------------------------------------------
// GROUP BY kernels: init table, grouped scan (after a flags pre-pass),
// export compacted groups (string exemplar bytes copied to a device heap).
// ---------------------------------------------------------------------------

__global__ void k_group_init(DevSpec sp, GroupCtx gc) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t n = gc.cap + 1;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    gc.state[i] = 0;
    gc.gkey[i] = 0;
    for (int g = 0; g < sp.num_aggs; ++g) {
      gc.vals[i * YBG_MAX_AGGS + g] = group_init_value(sp.aggs[g].op);
      gc.cnts[i * YBG_MAX_AGGS + g] = 0;
      gc.vals_hi[i * YBG_MAX_AGGS + g] = 0;
      gc.poison[i * YBG_MAX_AGGS + g] = 0;
    }
  }
}

// Single-pass GROUP BY: same head-deferral protocol as k_scan — no flags
// pre-pass. Non-head rows accumulate into the device hash table directly;
// each interval's head row is deferred as a GroupHead record, applied
// in-kernel once the lane relay resolves ownership, with workgroup-first
// intervals going through the global record + cont-flag path
// (k_group_heads folds those).
template <int NA, int WPS>
__global__ __launch_bounds__(kThreads, WPS) void k_group(
    const uint8_t* __restrict__ data,
    const uint64_t* __restrict__ block_offsets,
    const Interval* __restrict__ ivs, uint64_t n_ivs,
    const uint8_t* __restrict__ aux, uint8_t* __restrict__ rk_save_buf,
    GroupCtx gc, GroupHead* __restrict__ gheads,
    uint32_t* __restrict__ cont_flags,
    unsigned long long* __restrict__ err_counter,
    uint64_t* __restrict__ partials, uint64_t ivb) {
  const DevSpec& sp = c_spec;
  __shared__ uint8_t key_scratch[kThreads * kKeyCap];
  __shared__ uint8_t wave_relay[kThreads / 64 + 1];
  // 6 slots/thread: bht[0..2] packed-row write time, bht[3..5] the
  // restart-min candidate process_entry tracks when sp.track_restart
  // (a 3-slot array here clobbered the neighbour's write-time slots and
  // overran the shared array for threadIdx kThreads-1)
  __shared__ uint64_t bht_scratch[kThreads * 6];
  uint64_t* bht = bht_scratch + (size_t)threadIdx.x * 6;
  bht[5] = 0;
  uint8_t* key = key_scratch + (size_t)threadIdx.x * kKeyCap;
  const uint32_t gtid = blockIdx.x * kThreads + threadIdx.x;
  uint8_t* rk_save = rk_save_buf + (size_t)gtid * kKeyCap;
  const uint64_t span = (uint64_t)gridDim.x * kThreads;
  const uint64_t n_batches = (n_ivs + ivb - 1) / ivb;
  uint32_t entries = 0, scanned = 0, matched = 0;
  uint64_t agg_val[NA] = {0}, agg_cnt[NA] = {0};

  for (uint64_t j0 = 0; j0 < n_batches; j0 += span) {
    const uint64_t j = j0 + gtid;
    const bool active = j < n_batches;
    HeadOut<NA> ho;
    GroupHead gh;
    gh.hit = 0;
    bool walked_next = false;
    if (active) {
      uint64_t lo, hi;
      batch_bounds(nullptr, j, ivb, n_ivs, &lo, &hi);
      if (!scan_one_interval<NA, false, true>(
              sp, data, block_offsets, ivs, n_ivs, lo, hi, aux, key, rk_save,
              bht, &entries, &scanned, &matched, agg_val, agg_cnt, &ho,
              &walked_next, nullptr, nullptr, nullptr, nullptr, &gc, &gh)) {
        atomicAdd(err_counter, 1ull);
      }
    }
    unsigned lane = threadIdx.x & 63;
    unsigned wave = threadIdx.x >> 6;
    int wn = walked_next ? 1 : 0;
    int from_prev_lane = __shfl_up(wn, 1);
    if (lane == 63) wave_relay[wave + 1] = (uint8_t)wn;
    __syncthreads();
    bool head_consumed;
    if (threadIdx.x == 0) {
      head_consumed = false;  // resolved via the global record instead
    } else if (lane == 0) {
      head_consumed = wave_relay[wave] != 0;
    } else {
      head_consumed = from_prev_lane != 0;
    }
    __syncthreads();
    if (active) {
      if (threadIdx.x == 0) {
        gheads[j / kThreads] = gh;
      } else if (!head_consumed && gh.hit) {
        group_accum_rec<NA>(sp, gc, gh);
      }
      if (walked_next && ((j + 1) % kThreads) == 0 && (j + 1) < n_batches)
        cont_flags[(j + 1) / kThreads] = 1;
    }
    __syncthreads();
  }
  // read-restart fold, as in k_scan: wave minimum of the encoded-HT
  // restart candidates into the partial record's restart slots (the other
  // slots were zeroed host-side; k_reduce folds these into DevResult so
  // group scans report GetReadRestartData like plain scans)
  if (sp.track_restart && (threadIdx.x & 63) == 0) {
    uint64_t wave_id = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    wave_restart_min(bht_scratch, 6, 3, partials + wave_id * kPartialStride);
  }
}

template <int NA>
__global__ void k_group_heads(GroupCtx gc,
                              const GroupHead* __restrict__ gheads,
                              const uint32_t* __restrict__ cont_flags,
                              uint64_t n_heads) {
  const DevSpec& sp = c_spec;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_heads; i += stride)
    if (cont_flags[i] == 0 && gheads[i].hit)
      group_accum_rec<NA>(sp, gc, gheads[i]);
}

__global__ void k_group_export(DevSpec sp, GroupCtx gc,
                               uint64_t* __restrict__ out_keys,
                               long long* __restrict__ out_vals,
                               unsigned long long* __restrict__ out_cnts,
                               uint8_t* __restrict__ out_bytes,
                               uint64_t bytes_cap, uint64_t out_cap,
                               unsigned long long* __restrict__ counters) {
  // counters[0] = groups, counters[1] = bytes, counters[2] = overflow,
  // counters[3] = 1 + the output slot of the NULL-key group (0: none)
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t n = gc.cap + 1;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  bool grp_is_str = sp.group_col >= 0 &&
                    sp.cols[sp.group_col].dtype == YBG_T_STRING;
  for (; i < n; i += stride) {
    if (gc.state[i] != 1) continue;
    unsigned long long slot = atomicAdd(&counters[0], 1ull);
    if (slot >= out_cap) {
      atomicAdd(&counters[2], 1ull);
      continue;
    }
    uint64_t kv = gc.gkey[i];
    if (i == gc.cap) {
      // the NULL-key group: its key reads like the datum of -1, so the
      // slot is recorded (yb_gpu_scan_group_null_index)
      kv = ~0ull;
      counters[3] = slot + 1;
    } else if (grp_is_str) {
      uint32_t len = (uint32_t)(kv >> 40);
      unsigned long long off = atomicAdd(&counters[1], len);
      if (off + len > bytes_cap) {
        atomicAdd(&counters[2], 1ull);
        kv = 0;
      } else {
        const uint8_t* src = gc.data + (kv & ((1ull << 40) - 1));
        for (uint32_t b = 0; b < len; ++b) out_bytes[off + b] = src[b];
        kv = ((uint64_t)len << 40) | off;
      }
    }
    out_keys[slot] = kv;
    for (int g = 0; g < sp.num_aggs; ++g) {
      int op = sp.agg_op[g];
      long long v = group_export_value(
          op, gc.vals[i * YBG_MAX_AGGS + g],
          gc.vals_hi[i * YBG_MAX_AGGS + g],
          gc.poison[i * YBG_MAX_AGGS + g]);
      out_vals[slot * YBG_MAX_AGGS + g] = v;
      // COUNT ops skip the per-row cnt atomic: cnt == val by definition
      out_cnts[slot * YBG_MAX_AGGS + g] =
          (op == YBG_AGG_COUNT_STAR || op == YBG_AGG_COUNT)
              ? (unsigned long long)v
              : gc.cnts[i * YBG_MAX_AGGS + g];
    }
  }
}

// ---------------------------------------------------------------------------
// Final reduction: single workgroup, fixed order => deterministic
// ---------------------------------------------------------------------------

struct DevResult {
  uint64_t entries, scanned, matched, errs;
  uint64_t agg_val[YBG_MAX_AGGS];
  uint64_t agg_cnt[YBG_MAX_AGGS];
  uint64_t restart_hi, restart_lo, restart_len;
};

// Fold kernel: ONE launch turns the wave partial records, the batch state
// bytes and the pending head records into DevResult.
//  * Workgroup c owns a contiguous range of partial records and a
//    contiguous range of batches. A thread reads its records whole, in
//    index order (only the aggregate slots in use; the restart triple only
//    under track_restart), then its batches' state bytes four at a time (a
//    wave reads 256 contiguous bytes) and loads d_heads[j] only where the
//    head is pending and the predecessor did not walk into it.
//  * Threads combine in fixed lane order (shuffles), waves in fixed wave
//    order (LDS), and the workgroup writes one chunk record.
//  * The workgroup then takes a ticket; the one drawing the last ticket
//    folds the chunk records IN INDEX ORDER (never arrival order) into
//    DevResult and sets the ticket counter back to 0. No workgroup waits
//    for another.
// The fold tree is a fixed function of the grid and the batch count, so
// results (double SUM included) are bit-identical run to run.
// hstride = the bheads per-batch record stride (2 * dispatch-NA + 2).
constexpr int kFoldGrid = 512;
constexpr int kFoldThreads = 256;

struct FoldAcc {
  uint64_t cnt[4];  // entries, scanned, matched, errs
  uint64_t av[YBG_MAX_AGGS], ac[YBG_MAX_AGGS];
  uint64_t rh, rl, rn;  // restart minimum (rn == 0: none)
};

__device__ __forceinline__ void fold_restart(FoldAcc* a, uint64_t h,
                                             uint64_t l, uint64_t n) {
  if (n == 0) return;
  if (a->rn == 0 || u128_slice_cmp(h, l, (uint32_t)n, a->rh, a->rl,
                                   (uint32_t)a->rn) < 0) {
    a->rh = h;
    a->rl = l;
    a->rn = n;
  }
}

// one partial-layout record into the accumulator
__device__ __forceinline__ void fold_record(const DevSpec& sp, bool restart,
                                            FoldAcc* a, const uint64_t* r) {
#pragma unroll
  for (int s = 0; s < 4; ++s) a->cnt[s] += r[s];
#pragma unroll
  for (int g = 0; g < YBG_MAX_AGGS; ++g) {
    if (g >= sp.num_aggs) continue;
    combine1(sp.agg_op[g], &a->av[g], &a->ac[g], r[4 + 2 * g],
             r[4 + 2 * g + 1]);
  }
  if (restart) {
    const int rb = 4 + 2 * YBG_MAX_AGGS;
    fold_restart(a, r[rb], r[rb + 1], r[rb + 2]);
  }
}

// Workgroup reduction of every thread's accumulator into thread 0's:
// lanes by a fixed shuffle tree, then the waves in wave order through LDS.
// lds holds (kFoldThreads / 64) * kPartialStride u64.
__device__ __forceinline__ void fold_workgroup(const DevSpec& sp,
                                               bool restart, FoldAcc* a,
                                               uint64_t* lds) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int s = 0; s < 4; ++s) a->cnt[s] += shfl_down_u64(a->cnt[s], off);
#pragma unroll
    for (int g = 0; g < YBG_MAX_AGGS; ++g) {
      if (g >= sp.num_aggs) continue;  // workgroup-uniform
      uint64_t bv = shfl_down_u64(a->av[g], off);
      uint64_t bc = shfl_down_u64(a->ac[g], off);
      combine1(sp.agg_op[g], &a->av[g], &a->ac[g], bv, bc);
    }
    if (restart) {
      uint64_t h = shfl_down_u64(a->rh, off);
      uint64_t l = shfl_down_u64(a->rl, off);
      uint64_t n = shfl_down_u64(a->rn, off);
      fold_restart(a, h, l, n);
    }
  }
  if (lane == 0) {
    uint64_t* w = lds + wave * kPartialStride;
#pragma unroll
    for (int s = 0; s < 4; ++s) w[s] = a->cnt[s];
#pragma unroll
    for (int g = 0; g < YBG_MAX_AGGS; ++g) {
      w[4 + 2 * g] = a->av[g];
      w[4 + 2 * g + 1] = a->ac[g];
    }
    w[4 + 2 * YBG_MAX_AGGS] = a->rh;
    w[4 + 2 * YBG_MAX_AGGS + 1] = a->rl;
    w[4 + 2 * YBG_MAX_AGGS + 2] = a->rn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kFoldThreads / 64; ++v)
      fold_record(sp, restart, a, lds + v * kPartialStride);
  }
}

__global__ __launch_bounds__(kFoldThreads) void k_fold(
    DevSpec sp, const uint64_t* __restrict__ partials, uint64_t n_partials,
    const uint64_t* __restrict__ bheads, const uint8_t* __restrict__ state,
    uint64_t n_batches, int hstride, uint64_t* chunk, unsigned* ticket,
    DevResult* __restrict__ out) {
  __shared__ uint64_t lds[(kFoldThreads / 64) * kPartialStride];
  __shared__ unsigned s_ticket;
  const unsigned t = threadIdx.x;
  const uint64_t nch = gridDim.x;
  const bool restart = sp.track_restart != 0;
  FoldAcc a;
  memset(&a, 0, sizeof(a));

  // partial records [plo, phi)
  const uint64_t pl = (n_partials + nch - 1) / nch;
  const uint64_t plo = blockIdx.x * pl;
  const uint64_t phi = plo + pl < n_partials ? plo + pl : n_partials;
  for (uint64_t i = plo + t; i < phi; i += kFoldThreads)
    fold_record(sp, restart, &a, partials + i * kPartialStride);

  // batches [hlo, hhi), hlo a multiple of 4: a thread takes 4 consecutive
  // state bytes in one aligned load (the array is padded to a multiple of
  // 4 bytes) plus the byte before them
  const uint64_t hl = (((n_batches + nch - 1) / nch) + 3) & ~3ull;
  const uint64_t hlo = blockIdx.x * hl;
  const uint64_t hhi = hlo + hl < n_batches ? hlo + hl : n_batches;
  for (uint64_t j4 = hlo + 4ull * t; j4 < hhi; j4 += 4ull * kFoldThreads) {
    uint32_t st4;
    __builtin_memcpy(&st4, state + j4, 4);
    uint32_t prev = j4 > 0 ? state[j4 - 1] : 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint64_t j = j4 + b;
      const uint32_t st = (st4 >> (8 * b)) & 0xff;
      if (j < hhi && (st & kBatchHeadPending) && !(prev & kBatchWalked)) {
        const uint64_t* hr = bheads + j * hstride;
        a.cnt[1] += hr[hstride - 2];
        a.cnt[2] += hr[hstride - 1];
#pragma unroll
        for (int g = 0; g < YBG_MAX_AGGS; ++g) {
          if (g >= sp.num_aggs) continue;
          combine1(sp.agg_op[g], &a.av[g], &a.ac[g], hr[2 * g],
                   hr[2 * g + 1]);
        }
      }
      prev = st;
    }
  }

  fold_workgroup(sp, restart, &a, lds);
  uint64_t* mine = chunk + (uint64_t)blockIdx.x * kPartialStride;
  if (t == 0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) mine[s] = a.cnt[s];
#pragma unroll
    for (int g = 0; g < YBG_MAX_AGGS; ++g) {
      mine[4 + 2 * g] = a.av[g];
      mine[4 + 2 * g + 1] = a.ac[g];
    }
    mine[4 + 2 * YBG_MAX_AGGS] = a.rh;
    mine[4 + 2 * YBG_MAX_AGGS + 1] = a.rl;
    mine[4 + 2 * YBG_MAX_AGGS + 2] = a.rn;
    __threadfence();  // the record is visible before the ticket is taken
    s_ticket = atomicAdd(ticket, 1u);
  }
  __syncthreads();
  if (s_ticket != nch - 1) return;  // workgroup-uniform

  // last workgroup: every chunk record is written and fenced. Thread t
  // folds records t, t + 256, ... in index order; the reads bypass the
  // non-coherent cache path (agent-scope atomic loads).
  __threadfence();
  memset(&a, 0, sizeof(a));
  for (uint64_t i = t; i < nch; i += kFoldThreads) {
    uint64_t r[kPartialStride];
#pragma unroll
    for (int k = 0; k < kPartialStride; ++k)
      r[k] = ybg_atomic_load_u64(
          (unsigned long long*)(chunk + i * kPartialStride + k));
    fold_record(sp, restart, &a, r);
  }
  __syncthreads();  // lds is reused
  fold_workgroup(sp, restart, &a, lds);
  if (t == 0) {
    out->entries = a.cnt[0];
    out->scanned = a.cnt[1];
    out->matched = a.cnt[2];
    out->errs = a.cnt[3];
    for (int g = 0; g < YBG_MAX_AGGS; ++g) {
      out->agg_val[g] = a.av[g];
      out->agg_cnt[g] = a.ac[g];
    }
    out->restart_hi = a.rh;
    out->restart_lo = a.rl;
    out->restart_len = a.rn;
    *ticket = 0;  // every workgroup has drawn: ready for the next launch
  }
}

// Single-workgroup reduction of the grouped scan's partial records and
// workgroup-boundary head records (cont_flags protocol).
__global__ __launch_bounds__(256) void k_reduce(
    DevSpec sp, const uint64_t* __restrict__ partials, uint64_t n_partials,
    const uint64_t* __restrict__ heads, const uint32_t* __restrict__ cont_flags,
    uint64_t n_heads, DevResult* __restrict__ out) {
  __shared__ uint64_t sval[256], scnt[256], scal[256];
  const unsigned t = threadIdx.x;

  for (int s = 0; s < 4; ++s) {
    uint64_t acc = 0;
    for (uint64_t i = t; i < n_partials; i += 256)
      acc += partials[i * kPartialStride + s];
    if (s == 1 || s == 2) {  // scanned/matched also live in head records
      for (uint64_t i = t; i < n_heads; i += 256)
        if (cont_flags[i] == 0)
          acc += heads[i * kHeadStride + 2 * YBG_MAX_AGGS + (s - 1)];
    }
    scal[t] = acc;
    __syncthreads();
    if (t == 0) {
      uint64_t total = 0;
      for (int i = 0; i < 256; ++i) total += scal[i];
      (&out->entries)[s] = total;
    }
    __syncthreads();
  }

  for (int g = 0; g < sp.num_aggs; ++g) {
    int op = sp.aggs[g].op;
    uint64_t av = 0, ac = 0;
    for (uint64_t i = t; i < n_partials; i += 256)
      combine1(op, &av, &ac, partials[i * kPartialStride + 4 + 2 * g],
               partials[i * kPartialStride + 4 + 2 * g + 1]);
    for (uint64_t i = t; i < n_heads; i += 256) {
      if (cont_flags[i] != 0) continue;
      combine1(op, &av, &ac, heads[i * kHeadStride + 2 * g],
               heads[i * kHeadStride + 2 * g + 1]);
    }
    sval[t] = av;
    scnt[t] = ac;
    __syncthreads();
    if (t == 0) {
      uint64_t fv = 0, fc = 0;
      for (int i = 0; i < 256; ++i) combine1(op, &fv, &fc, sval[i], scnt[i]);
      out->agg_val[g] = fv;
      out->agg_cnt[g] = fc;
    }
    __syncthreads();
  }
  {
    // restart-min over the chunk records (len 0 = none)
    const int rb = 4 + 2 * YBG_MAX_AGGS;
    uint64_t mh = 0, ml = 0, mn = 0;
    for (uint64_t i = t; i < n_partials; i += 256) {
      uint64_t n = partials[i * kPartialStride + rb + 2];
      if (n == 0) continue;
      uint64_t h = partials[i * kPartialStride + rb];
      uint64_t l = partials[i * kPartialStride + rb + 1];
      if (mn == 0 ||
          u128_slice_cmp(h, l, (uint32_t)n, mh, ml, (uint32_t)mn) < 0) {
        mh = h;
        ml = l;
        mn = n;
      }
    }
    sval[t] = mh;
    scnt[t] = ml;
    scal[t] = mn;
    __syncthreads();
    if (t == 0) {
      uint64_t fh = 0, fl = 0, fn = 0;
      for (int i = 0; i < 256; ++i) {
        if (scal[i] == 0) continue;
        if (fn == 0 || u128_slice_cmp(sval[i], scnt[i], (uint32_t)scal[i],
                                      fh, fl, (uint32_t)fn) < 0) {
          fh = sval[i];
          fl = scnt[i];
          fn = scal[i];
        }
      }
      out->restart_hi = fh;
      out->restart_lo = fl;
      out->restart_len = fn;
    }
  }
}

// Per-block decompression at feed time: one thread per data block (~1M
// blocks >> threads), serial decode per thread — snappy (type 1,
// snappy_dev.h) or LZ4 (type 4, lz4_dev.h, varint32 raw-length framing
// per rocksdb util/compression.h). type 0 blocks copy through in u64
// chunks.
__global__ __launch_bounds__(256) void k_snappy(
    const uint8_t* __restrict__ src_blob,
    const uint64_t* __restrict__ src_off,
    const uint64_t* __restrict__ src_len,
    const uint64_t* __restrict__ dst_off, const uint8_t* __restrict__ types,
    uint64_t n_blocks, uint8_t* __restrict__ out, uint64_t out_cap,
    unsigned long long* __restrict__ err) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_blocks; i += stride) {
    const uint8_t* src = src_blob + src_off[i];
    uint64_t n = src_len[i];
    uint8_t* dst = out + dst_off[i];
    uint64_t cap = dst_off[i + 1] - dst_off[i];  // exact slot, never the
                                                 // neighbour's bytes
    if (types[i] == 1) {
      if (ybsnappy::snappy_uncompress(src, n, dst, cap) < 0)
        atomicAdd(err, 1ull);
    } else if (types[i] == 4) {
      // skip the varint32 raw-length prefix (validated host-side)
      uint64_t o = 0;
      while (o < n && (src[o] & 0x80)) ++o;
      ++o;
      if (o > n || yblz4::lz4_uncompress(src + o, n - o, dst, cap) !=
                       (int64_t)cap)
        atomicAdd(err, 1ull);
    } else {
      for (uint64_t b = 0; b + 8 <= n; b += 8) {
        uint64_t w;
        __builtin_memcpy(&w, src + b, 8);
        __builtin_memcpy(dst + b, &w, 8);
      }
      for (uint64_t b = n & ~7ull; b < n; ++b) dst[b] = src[b];
    }
  }
}

// Data-block trailer verification on DEVICE (util/crc32c crc32c.cc,
// masked per format.h:212): one thread per block, slicing-by-4 over LDS
// tables built at launch. Replaces the ~2.2 GB/s host verify on the SST
// feed path.
__global__ __launch_bounds__(256) void k_crc32c(
    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs,
    const uint64_t* __restrict__ szs, uint64_t n_blocks,
    unsigned long long* __restrict__ err) {
  __shared__ uint32_t t[4][256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k)
      c = (c & 1) ? (0x82F63B78u ^ (c >> 1)) : (c >> 1);
    t[0][i] = c;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    uint32_t c = t[0][i];
    for (int s = 1; s < 4; ++s) {
      c = t[0][c & 0xff] ^ (c >> 8);
      t[s][i] = c;
    }
  }
  __syncthreads();
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_blocks; i += stride) {
    const uint8_t* p = blob + offs[i];
    uint64_t n = szs[i] + 1;  // block bytes + trailer type byte
    uint32_t c = 0xffffffffu;
    while (n >= 4) {
      uint32_t lo;
      __builtin_memcpy(&lo, p, 4);
      lo ^= c;
      c = t[3][lo & 0xff] ^ t[2][(lo >> 8) & 0xff] ^
          t[1][(lo >> 16) & 0xff] ^ t[0][lo >> 24];
      p += 4;
      n -= 4;
    }
    for (uint64_t k = 0; k < n; ++k)
      c = t[0][(c ^ p[k]) & 0xff] ^ (c >> 8);
    c ^= 0xffffffffu;
    uint32_t masked = ((c >> 15) | (c << 17)) + 0xa282ead8u;  // kCrcMaskDelta
    uint32_t want;
    __builtin_memcpy(&want, blob + offs[i] + szs[i] + 1, 4);
    if (masked != want) atomicAdd(err, 1ull);
  }
}

}  // namespace

// ===========================================================================
// Host ABI
// ===========================================================================

namespace {

thread_local std::string g_err;

}  // namespace

// shared with the snapshot code (snap_gpu.hip) through snap_internal.h
int ybgint::set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

using ybgint::set_err;

#define HIP_TRY(x)                                                        \
  do {                                                                    \
    hipError_t _e = (x);                                                  \
    if (_e != hipSuccess)                                                 \
      return set_err(10, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define HIP_WARN(x) \
  do { hipError_t _e = (x); (void)_e; } while (0)

}  // namespace

struct ybg_scan {
  ybg_scan_spec_t spec;
  DevSpec dspec;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_mid = nullptr, ev_end = nullptr;
  uint8_t* d_data = nullptr;
  bool d_data_owned = false;
  uint64_t* d_offsets = nullptr;
  Interval* d_ivs = nullptr;
  uint64_t n_ivs = 0;
  uint64_t ivb = 1;       // intervals per batch (one thread's stream)
  uint64_t n_batches = 0;
  uint64_t* d_batch_lo = nullptr;  // block-aligned batches (YBG_BB=1):
                                   // batch b = intervals [lo[b], lo[b+1])
  uint64_t n_blocks = 0;
  uint64_t total_bytes = 0;
  uint8_t* d_aux = nullptr;
  uint8_t* d_rk_save = nullptr;
  uint64_t* d_partials = nullptr;  // 3 regions: main | retry/known | late
  uint64_t n_partials = 0;
  uint64_t* d_heads = nullptr;   // per-batch head records (stride hstride)
  uint8_t* d_walked = nullptr;   // per-batch state byte (kBatchWalked |
                                 // kBatchHeadPending)
  uint64_t* d_retry = nullptr;   // fast-kernel aborted batch ids
  unsigned long long* d_retry_n = nullptr;
  uint32_t* d_cont = nullptr;    // k_group relay flags (per 256 batches)
  uint64_t n_heads = 0;          // = n_batches
  uint64_t n_gheads = 0;         // = ceil(n_batches / kThreads)
  int na_cap = 2;
  int hstride = 6;
  DevResult* d_result = nullptr;
  uint64_t* d_chunk = nullptr;  // k_fold chunk records (kFoldGrid)
  unsigned* d_fold_ticket = nullptr;  // k_fold arrival counter, 0 at rest
  uint64_t last_retry_batches = 0;  // batches the last execute handed to
                                    // the general kernel (known + late)
  unsigned long long* h_retry_n = nullptr;  // pinned: d_retry_n of the last
                                            // fast execute, copied after it
  bool retry_pending = false;  // ...not yet looked at by wait
  // Known abort set (see yb_gpu_scan_execute): the batches the fast kernel
  // aborted in an earlier execute of this handle, as a sorted id list and a
  // bitmap, valid for one batch decomposition and kernel variant
  hipStream_t stream2 = nullptr;  // runs the known-list launch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  struct KnownKey {
    uint64_t n_bat = 0, ivb = 0;
    bool bb = false;
    int variant = -1;
    bool operator==(const KnownKey& o) const {
      return n_bat == o.n_bat && ivb == o.ivb && bb == o.bb &&
             variant == o.variant;
    }
  };
  bool known_valid = false;
  KnownKey known_key;
  std::vector<uint64_t> known_ids;  // sorted ascending
  uint64_t* d_known = nullptr;      // known_ids on the device
  unsigned long long* d_known_n = nullptr;
  uint64_t* d_known_bits = nullptr;  // one bit per batch
  // the last fast execute: its key, how many known batches it launched,
  // and whether wait may learn from it (YBG_KNOWN)
  KnownKey last_key;
  uint64_t last_known_n = 0;
  bool last_learn = false;
  int grid = 0;
  bool executed = false;
  // bloom filter proved the scan's pinned key prefix absent at feed
  // time: no data was uploaded, every result surface reports empty
  bool bloom_rejected = false;
  double last_total_ms = 0, last_decode_ms = 0;
  std::vector<uint8_t> aux_host;
  // handle-owned copies of the caller's bound and option-list bytes:
  // s->spec points into these, so the spec stays readable after open
  // (snapshot builds and staged executes translate it again later)
  std::vector<std::vector<uint8_t>> spec_bytes;
  // feed dropped blocks because of a leading-key IN / IN_RANGE predicate
  // (not only DocKey bounds): the fed set no longer holds every row inside
  // the bounds
  bool pruned_by_options = false;
  // emit (next_batch) buffers
  uint32_t* d_flags_all = nullptr;
  uint64_t emit_row_cap = 0;
  uint64_t* d_em_sort = nullptr;
  uint64_t* d_em_key = nullptr;
  uint64_t* d_em_dat = nullptr;
  uint32_t* d_em_null = nullptr;
  uint16_t* d_em_hash = nullptr;
  uint8_t* d_em_varlen = nullptr;
  uint64_t em_varlen_cap = 0;
  unsigned long long* d_em_counters = nullptr;  // rows, varlen, overflow, err
  std::vector<uint64_t> h_sort, h_key, h_dat;
  std::vector<uint32_t> h_null;
  std::vector<uint16_t> h_hash;
  std::vector<uint8_t> h_varlen;
  // group-by buffers
  GroupCtx gc = {};
  GroupHead* d_gheads = nullptr;
  uint64_t group_cap = 0;
  uint64_t* d_gk_out = nullptr;
  long long* d_gv_out = nullptr;
  unsigned long long* d_gc_out = nullptr;
  uint8_t* d_gb_out = nullptr;
  unsigned long long* d_g_counters = nullptr;
  int64_t group_null_index = -1;  // of the last successful group_aggregate
  bool group_done = false;
  // YBG_STAGE=1 transparent mode: columnar snapshot built on the first
  // eligible execute and kept for the handle's lifetime
  ybg_snapshot_t* stage_snap = nullptr;
  bool stage_failed = false;  // the build failed once: stay on the block path
  bool staged_last = false;   // last execute was answered from the snapshot
  bool planned_last = false;  // last execute launched the planned fast kernel
};

extern "C" {

const char* yb_gpu_last_error(void) { return g_err.c_str(); }

int yb_gpu_available(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n > 0;
}

int yb_gpu_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return 0;
}

int yb_gpu_scan_open(const ybg_scan_spec_t* spec, ybg_scan_t** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return set_err(2,
                   "no HIP device visible — the GPU product path has no CPU "
                   "fallback (oracle/ is test infrastructure only)");
  for (int i = 0; i < spec->num_preds; ++i) {
    const ybg_pred_t& p = spec->preds[i];
    if (p.op == YBG_PRED_IN_TUPLE) {
      if (!p.is_key_col || !p.bytes || p.bytes_len < 4)
        return set_err(9, "IN_TUPLE requires key columns and a tuple list");
      uint32_t nc;
      memcpy(&nc, p.bytes, 4);
      int nk = spec->schema.num_hash_cols + spec->schema.num_range_cols;
      if (nc == 0 || nc > (uint32_t)nk ||
          p.bytes_len < 4 + 4ull * nc ||
          (p.bytes_len - 4 - 4ull * nc) % (8ull * nc))
        return set_err(9, "malformed IN_TUPLE list");
      for (uint32_t c = 0; c < nc; ++c) {
        uint32_t ci;
        memcpy(&ci, p.bytes + 4 + 4ull * c, 4);
        if (ci >= (uint32_t)nk ||
            spec->schema.key_types[ci] == YBG_KT_STRING)
          return set_err(9, "IN_TUPLE columns must be numeric key columns");
      }
      continue;
    }
    if (p.op == YBG_PRED_IN_RANGE) {
      bool is_str = p.is_key_col
                        ? spec->schema.key_types[p.col] == YBG_KT_STRING
                        : spec->schema.value_cols[p.col].dtype ==
                              YBG_T_STRING;
      if (is_str || !p.bytes || p.bytes_len == 0 || p.bytes_len % 24)
        return set_err(9, "IN_RANGE needs a numeric column and n x "
                          "24-byte range records");
      continue;
    }
    if (p.op != YBG_PRED_IN) continue;
    bool is_str = p.is_key_col
                      ? spec->schema.key_types[p.col] == YBG_KT_STRING
                      : spec->schema.value_cols[p.col].dtype == YBG_T_STRING;
    if (!p.bytes)
      return set_err(9, "IN list missing");
    if (is_str) {
      // [u32 LE length][bytes] records, exactly covering bytes_len
      uint64_t o = 0;
      while (o + 4 <= p.bytes_len) {
        uint32_t ol;
        memcpy(&ol, p.bytes + o, 4);
        o += 4ull + ol;
      }
      if (o != p.bytes_len)
        return set_err(9, "malformed string IN list");
    } else if (p.bytes_len % 8) {
      return set_err(9, "IN list must be n x 8-byte datum patterns");
    }
  }
  auto* s = new ybg_scan();
  s->spec = *spec;
  {
    auto own = [&](const uint8_t** p, uint64_t len) {
      if (!*p || !len) return;
      s->spec_bytes.emplace_back(*p, *p + len);
      *p = s->spec_bytes.back().data();
    };
    s->spec_bytes.reserve(YBG_MAX_PREDS + 2);  // no reallocation below
    own(&s->spec.lower_bound, s->spec.lower_bound_len);
    own(&s->spec.upper_bound, s->spec.upper_bound_len);
    for (int i = 0; i < s->spec.num_preds && i < YBG_MAX_PREDS; ++i)
      own(&s->spec.preds[i].bytes, s->spec.preds[i].bytes_len);
  }
  s->aux_host.resize(1 << 20);
  uint32_t aux_len = 0;
  build_dev_spec(spec, &s->dspec, s->aux_host.data(), &aux_len,
                 (uint32_t)s->aux_host.size());
  // 16 bytes of tail slack: the device predicate paths read the aux
  // buffer through load_u64_una (up to 11 bytes past a position)
  s->aux_host.resize(aux_len + 16, 0);

  hipError_t e;
  if ((e = hipStreamCreate(&s->stream)) != hipSuccess ||
      (e = hipEventCreate(&s->ev_start)) != hipSuccess ||
      (e = hipEventCreate(&s->ev_mid)) != hipSuccess ||
      (e = hipEventCreate(&s->ev_end)) != hipSuccess ||
      (e = hipStreamCreate(&s->stream2)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming)) !=
          hipSuccess ||
      (e = hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming)) !=
          hipSuccess) {
    delete s;
    return set_err(10, hipGetErrorString(e));
  }
  HIP_TRY(hipMalloc(&s->d_aux, s->aux_host.size()));
  HIP_TRY(hipMemcpy(s->d_aux, s->aux_host.data(), s->aux_host.size(),
                    hipMemcpyHostToDevice));
  *out = s;
  return 0;
}

}  // extern "C"

namespace {

// ---------------------------------------------------------------------
// Index-guided block pruning (docdb/hybrid_scan_choices.cc seek plans +
// rocksdb index-based block selection, index_reader.cc): a bounded or
// option-constrained scan only needs the blocks whose key range
// intersects the allowed key set. Block separators = each block's first
// internal key (the role the SST index keys play in the reference).
// Pruning is a strict superset selection: the per-row bound checks and
// option FILTERS still run, so a conservative selection cannot change
// results — parity tests pin it against unpruned scans and the oracle.
// ---------------------------------------------------------------------

struct KeyRange {
  std::vector<uint8_t> lo;  // inclusive prefix; empty = -inf
  std::vector<uint8_t> hi;  // exclusive prefix; empty = +inf
};

// encoded key-prefix successor: the smallest byte string > p as a prefix
std::vector<uint8_t> prefix_succ(std::vector<uint8_t> p) {
  while (!p.empty()) {
    if (p.back() != 0xff) {
      p.back() += 1;
      return p;
    }
    p.pop_back();
  }
  return p;  // empty = +inf
}

void enc_key_int(int kt, uint64_t v, std::vector<uint8_t>* out) {
  if (kt == YBG_KT_INT64) {
    out->push_back(0x49);  // kInt64B
    uint64_t u = v ^ 0x8000000000000000ull;
    for (int i = 7; i >= 0; --i) out->push_back((uint8_t)(u >> (8 * i)));
  } else {
    out->push_back(0x48);  // kInt32B
    uint32_t u = (uint32_t)v ^ 0x80000000u;
    for (int i = 3; i >= 0; --i) out->push_back((uint8_t)(u >> (8 * i)));
  }
}

// prefix vs full-key compare: memcmp over min length; a proper prefix
// sorts first (all keys starting with it come after or at it)
int pfx_cmp(const std::vector<uint8_t>& a, const uint8_t* b, size_t blen) {
  size_t n = a.size() < blen ? a.size() : blen;
  int c = memcmp(a.data(), b, n);
  if (c) return c;
  return a.size() == blen ? 0 : (a.size() < blen ? -1 : 1);
}

// Length of the full encoded DocKey at the head of an internal key
// (hash group + range group, each kGroupEnd-terminated —
// dockv/doc_key.h:40-63). 0 = unparseable. Bounds are DOCKEYS: comparing
// them against the raw internal first key (DocKey || '#' DHT || seq)
// mis-orders exactly when the bound extends the DocKey (e.g. a point
// scan's upper = key + "\x00" sorts BELOW key's internal entries), so
// block selection must compare against this prefix, never the raw key.
size_t dockey_full_len(const uint8_t* k, size_t len) {
  size_t p = 0;
  if (len && k[0] == 0x47) {  // kUInt16Hash
    if (len < 3) return 0;
    p = 3;
    while (p < len && k[p] != 0x21) {  // hashed components
      size_t n = ybg::skip_key_entry(k + p, len - p);
      if (!n) return 0;
      p += n;
    }
    if (p >= len) return 0;
    ++p;  // hashed group end
  }
  while (p < len && k[p] != 0x21) {  // range components
    size_t n = ybg::skip_key_entry(k + p, len - p);
    if (!n) return 0;
    p += n;
  }
  if (p >= len) return 0;
  return p + 1;  // range group end
}

// Returns true (and fills keep) when the spec allows pruning AND at least
// one block can be skipped.
bool compute_block_selection(const ybg_scan_spec_t& spec,
                             const uint8_t* blocks, const uint64_t* offsets,
                             uint64_t n_blocks,
                             std::vector<uint8_t>* keep,
                             bool* by_options = nullptr) {
  if (by_options) *by_options = false;
  std::vector<KeyRange> allowed;
  KeyRange bounds;
  bool have_bounds = false;
  if (spec.lower_bound_len) {
    bounds.lo.assign(spec.lower_bound,
                     spec.lower_bound + spec.lower_bound_len);
    have_bounds = true;
  }
  if (spec.upper_bound_len) {
    bounds.hi.assign(spec.upper_bound,
                     spec.upper_bound + spec.upper_bound_len);
    have_bounds = true;
  }
  // leading-range-key options on range-sharded tables: derive key-prefix
  // ranges from IN / IN_RANGE on key column 0 (a seek plan the reference
  // builds in HybridScanChoices)
  std::vector<KeyRange> opts;
  if (!spec.schema.has_hash &&
      (spec.schema.key_types[0] == YBG_KT_INT64 ||
       spec.schema.key_types[0] == YBG_KT_INT32)) {
    for (int i = 0; i < spec.num_preds; ++i) {
      const ybg_pred_t& p = spec.preds[i];
      if (!p.is_key_col || p.col != 0 || !p.bytes) continue;
      if (p.op == YBG_PRED_IN) {
        for (uint64_t o = 0; o + 8 <= p.bytes_len; o += 8) {
          uint64_t v;
          memcpy(&v, p.bytes + o, 8);
          KeyRange r;
          enc_key_int(spec.schema.key_types[0], v, &r.lo);
          r.hi = prefix_succ(r.lo);
          opts.push_back(std::move(r));
        }
      } else if (p.op == YBG_PRED_IN_RANGE) {
        for (uint64_t o = 0; o + 24 <= p.bytes_len; o += 24) {
          uint64_t lo, hi;
          memcpy(&lo, p.bytes + o, 8);
          memcpy(&hi, p.bytes + o + 8, 8);
          KeyRange r;  // conservative: inclusive both ends as prefixes
          enc_key_int(spec.schema.key_types[0], lo, &r.lo);
          std::vector<uint8_t> h;
          enc_key_int(spec.schema.key_types[0], hi, &h);
          r.hi = prefix_succ(h);
          opts.push_back(std::move(r));
        }
      }
      if (!opts.empty()) break;  // one option pred drives the seek plan
    }
  }
  if (!have_bounds && opts.empty()) return false;
  if (opts.empty()) {
    allowed.push_back(std::move(bounds));
  } else {
    // intersect every option range with the scan bounds
    for (auto& r : opts) {
      KeyRange c = r;
      if (!bounds.lo.empty() &&
          (c.lo.empty() || c.lo < bounds.lo))
        c.lo = bounds.lo;
      if (!bounds.hi.empty() &&
          (c.hi.empty() || bounds.hi < c.hi))
        c.hi = bounds.hi;
      allowed.push_back(std::move(c));
    }
  }

  // block separators: the DOCKEY of each block's first internal key
  // (see dockey_full_len — raw internal-key bytes mis-order vs DocKey
  // bounds)
  std::vector<std::vector<uint8_t>> fk(n_blocks);
  for (uint64_t b = 0; b < n_blocks; ++b) {
    uint8_t buf[256];
    uint64_t len = 0;
    if (ybg_block_first_key(blocks + offsets[b],
                            offsets[b + 1] - offsets[b], spec.kv_format,
                            buf, sizeof(buf), &len))
      return false;  // undecodable: do not prune
    if (len < 8) return false;
    size_t dl = dockey_full_len(buf, len - 8);  // minus the seqno suffix
    if (!dl) return false;  // unknown entry encodings: do not prune
    fk[b].assign(buf, buf + dl);
  }
  keep->assign(n_blocks, 0);
  bool any_skip = false;
  for (uint64_t b = 0; b < n_blocks; ++b) {
    // block b covers DocKeys [fk[b], fk[b+1]] — INCLUSIVE of fk[b+1]:
    // a row whose first entry opens block b+1 may have entries
    // straddling from the tail of block b, so lo uses <= on the next
    // separator (keeps at most one extra block)
    bool hit = false;
    for (const auto& r : allowed) {
      bool lo_ok =
          r.lo.empty() || b + 1 >= n_blocks ||
          pfx_cmp(r.lo, fk[b + 1].data(), fk[b + 1].size()) <= 0;
      bool hi_ok = r.hi.empty() ||
                   pfx_cmp(r.hi, fk[b].data(), fk[b].size()) > 0;
      if (lo_ok && hi_ok) {
        hit = true;
        break;
      }
    }
    (*keep)[b] = hit ? 1 : 0;
    if (!hit) any_skip = true;
  }
  // option ranges (not only the DocKey bounds) shaped the selection
  if (by_options) *by_options = any_skip && !opts.empty();
  return any_skip;
}

}  // namespace

extern "C" {

// Test hook: the block selection feed_blocks applies (1 byte per block;
// returns 1 when pruning engaged). CPU tests feed the kept subset through
// the simulator and compare against unpruned oracle scans.
int ybg_test_block_selection(const ybg_scan_spec_t* spec,
                             const uint8_t* blocks, const uint64_t* offsets,
                             uint64_t n_blocks, uint8_t* keep_out) {
  std::vector<uint8_t> keep;
  if (!compute_block_selection(*spec, blocks, offsets, n_blocks, &keep))
    return 0;
  memcpy(keep_out, keep.data(), n_blocks);
  return 1;
}

/* Bloom-aware feed (BloomFilterAwareIterator role,
 * docdb/docdb_rocksdb_util.cc bloom usage + rocksdb
 * table/fixed_size_filter_block.cc): when the scan's DocKey bounds pin
 * one kUpToHashOrFirstRange prefix (a point read on the hashed
 * components) and the tablet's filter proves that prefix absent, the
 * scan is answered empty WITHOUT uploading or touching any block.
 * filter = ybg_filter_from_sst output for this tablet (may be
 * NULL/empty: never rejects). Results are identical to an unfiltered
 * feed + scan — the filter only skips provably-empty work. */
int yb_gpu_scan_feed_blocks_bloom(ybg_scan_t* s, const uint8_t* blocks,
                                  const uint64_t* offsets,
                                  uint64_t n_blocks, int device,
                                  const uint8_t* filter,
                                  uint64_t filter_len) {
  const ybg_scan_spec_t& sp = s->spec;
  if (filter && filter_len && sp.lower_bound_len && sp.upper_bound_len) {
    size_t pl = ybg::filter_key_prefix_len(sp.lower_bound,
                                           sp.lower_bound_len);
    size_t pu = ybg::filter_key_prefix_len(sp.upper_bound,
                                           sp.upper_bound_len);
    if (pl && pl == pu &&
        memcmp(sp.lower_bound, sp.upper_bound, pl) == 0 &&
        !ybg::bloom_may_match(filter, filter_len, sp.lower_bound,
                              sp.lower_bound_len,
                              (uint32_t)ybg_filter_slice_size())) {
      s->bloom_rejected = true;
      return 0;
    }
  }
  return yb_gpu_scan_feed_blocks(s, blocks, offsets, n_blocks, device);
}

int yb_gpu_scan_feed_blocks(ybg_scan_t* s, const uint8_t* blocks,
                            const uint64_t* offsets, uint64_t n_blocks,
                            int device) {
  // index-guided pruning (host-bytes path): upload only the blocks whose
  // key range intersects the scan's bounds / leading-key option ranges
  std::vector<uint8_t> pruned_blob;
  std::vector<uint64_t> pruned_off;
  bool noprune = false;
  if (const char* e = getenv("YBG_NOPRUNE")) noprune = atoi(e) != 0;
  if (!device && n_blocks && !noprune) {
    std::vector<uint8_t> keep;
    bool by_options = false;
    if (compute_block_selection(s->spec, blocks, offsets, n_blocks,
                                &keep, &by_options)) {
      s->pruned_by_options = by_options;
      pruned_off.push_back(0);
      for (uint64_t b = 0; b < n_blocks; ++b) {
        if (!keep[b]) continue;
        pruned_blob.insert(pruned_blob.end(), blocks + offsets[b],
                           blocks + offsets[b + 1]);
        pruned_off.push_back(pruned_blob.size());
      }
      if (pruned_off.size() <= 1) {
        // nothing selected: feed one empty-ish view is invalid; keep a
        // single block so the scan machinery has a well-formed table
        // (its rows are filtered per-row anyway)
        uint64_t b0 = 0;
        pruned_blob.assign(blocks + offsets[b0], blocks + offsets[b0 + 1]);
        pruned_off.push_back(pruned_blob.size());
      }
      blocks = pruned_blob.data();
      offsets = pruned_off.data();
      n_blocks = pruned_off.size() - 1;
    }
  }
  s->n_blocks = n_blocks;
  s->total_bytes = offsets[n_blocks];
  if (device) {
    s->d_data = const_cast<uint8_t*>(blocks);
    s->d_data_owned = false;
  } else {
    // 256 bytes tail slack: Rdr window init can read up to 32 bytes past
    // the position, load_u64_una up to 11, and the YBG_PF prefetch build
    // up to ~200 (scan_device.h contract)
    HIP_TRY(hipMalloc(&s->d_data, s->total_bytes + 256));
    HIP_TRY(hipMemset(s->d_data + s->total_bytes, 0, 256));
    HIP_TRY(hipMemcpy(s->d_data, blocks, s->total_bytes,
                      hipMemcpyHostToDevice));
    s->d_data_owned = true;
  }
  HIP_TRY(hipMalloc(&s->d_offsets, (n_blocks + 1) * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(s->d_offsets, offsets, (n_blocks + 1) * sizeof(uint64_t),
                    hipMemcpyHostToDevice));

  uint32_t* d_counts;
  int* d_err;
  HIP_TRY(hipMalloc(&d_counts, n_blocks * sizeof(uint32_t)));
  HIP_TRY(hipMalloc(&d_err, sizeof(int)));
  HIP_TRY(hipMemset(d_err, 0, sizeof(int)));
  int blocks_grid = (int)std::min<uint64_t>((n_blocks + 255) / 256, 4096);
  hipLaunchKernelGGL(k_count_restarts, dim3(blocks_grid), dim3(256), 0,
                     s->stream, s->d_data, s->d_offsets, n_blocks, d_counts,
                     d_err);
  std::vector<uint32_t> counts(n_blocks);
  HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, n_blocks * sizeof(uint32_t),
                         hipMemcpyDeviceToHost, s->stream));
  int h_err = 0;
  HIP_TRY(hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (h_err) {
    HIP_WARN(hipFree(d_counts));
    HIP_WARN(hipFree(d_err));
    return set_err(3, "corrupt block trailer");
  }
  std::vector<uint64_t> base(n_blocks + 1);
  uint64_t acc = 0;
  for (uint64_t i = 0; i < n_blocks; ++i) {
    base[i] = acc;
    acc += counts[i];
  }
  base[n_blocks] = acc;
  s->n_ivs = acc;
  uint64_t* d_base;
  HIP_TRY(hipMalloc(&d_base, (n_blocks + 1) * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(d_base, base.data(), (n_blocks + 1) * sizeof(uint64_t),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&s->d_ivs, s->n_ivs * sizeof(Interval)));
  hipLaunchKernelGGL(k_emit_intervals, dim3(blocks_grid), dim3(256), 0,
                     s->stream, s->d_data, s->d_offsets, n_blocks, d_base,
                     s->d_ivs);
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->d_batch_lo = d_base;  // per-block interval base: block-aligned
                           // batches for the scalar dispatch
  HIP_WARN(hipFree(d_counts));
  HIP_WARN(hipFree(d_err));

  // Adaptive batch size: aim for ~2 grid-stride passes over a full launch
  // (span = 8192 workgroups x 256 threads). Reproduces the measured
  // optima — 2 for the 6.5M-interval filtersum tablet (15.6 vs 15.1
  // Grows/s at 1), 8 for the 32M-interval MVCC tablet (3.5 vs 3.2 at 2);
  // larger batches degrade both (tail imbalance + per-wave L2 span).
  {
    const uint64_t span = 8192ull * kThreads;
    uint64_t ivb = (s->n_ivs + span) / (2 * span);
    if (ivb < 1) ivb = 1;
    if (ivb > 64) ivb = 64;
    s->ivb = ivb;
  }
  if (const char* e = getenv("YBG_IVB")) {
    long v = atol(e);
    if (v >= 1 && v <= 4096) s->ivb = (uint64_t)v;
  }
  s->n_batches = (s->n_ivs + s->ivb - 1) / s->ivb;
  uint64_t want = (s->n_batches + kThreads - 1) / kThreads;
  uint64_t cap = 8192;
  if (const char* g = getenv("YBG_GRID")) {
    long v = atol(g);
    if (v > 0) cap = (uint64_t)v;
  }
  s->grid = (int)std::min<uint64_t>(want, cap);
  if (s->grid < 1) s->grid = 1;
  uint64_t span_threads = (uint64_t)s->grid * kThreads;
  s->n_partials = span_threads / 64;
  // head records sized for BOTH batch decompositions (fixed-ivb and
  // block-aligned — execute() picks per dispatch)
  s->n_heads = s->n_batches > s->n_blocks ? s->n_batches : s->n_blocks;
  s->n_gheads = (s->n_batches + kThreads - 1) / kThreads;
  s->na_cap = s->dspec.num_aggs <= 2 ? 2 : (s->dspec.num_aggs <= 4 ? 4 : 8);
  s->hstride = 2 * s->na_cap + 2;
  HIP_TRY(hipMalloc(&s->d_rk_save, span_threads * kKeyCap));
  // three regions: main launch | retry or known-list launch | late launch
  HIP_TRY(hipMalloc(&s->d_partials,
                    3 * s->n_partials * kPartialStride * sizeof(uint64_t)));
  HIP_TRY(hipMalloc(&s->d_heads,
                    s->n_heads * s->hstride * sizeof(uint64_t)));
  // + 8: k_fold reads the state bytes four at a time
  HIP_TRY(hipMalloc(&s->d_walked, s->n_heads + 8));
  HIP_TRY(hipMalloc(&s->d_retry,
                    (s->n_heads ? s->n_heads : 1) * sizeof(uint64_t)));
  HIP_TRY(hipMalloc(&s->d_retry_n, sizeof(unsigned long long)));
  HIP_TRY(hipHostMalloc(&s->h_retry_n, sizeof(unsigned long long)));
  s->known_valid = false;  // a feed drops the known abort set
  HIP_TRY(hipMalloc(&s->d_cont,
                    ((s->n_batches + kThreads - 1) / kThreads) *
                        sizeof(uint32_t)));
  HIP_TRY(hipMalloc(&s->d_result, sizeof(DevResult)));
  HIP_TRY(hipMalloc(&s->d_chunk,
                    kFoldGrid * kPartialStride * sizeof(uint64_t)));
  HIP_TRY(hipMalloc(&s->d_fold_ticket, sizeof(unsigned)));
  HIP_TRY(hipMemset(s->d_fold_ticket, 0, sizeof(unsigned)));
  return 0;
}

// Feed regular blocks together with an intent stream: resolve the
// transaction statuses, merge committed intents into the affected blocks
// (ybg_merge_intents, sstgen.cc) and feed the merged tablet. The scan
// then applies the committed-intent visibility rule on device
// (intent_aware_iterator.cc:1249-1267).
int yb_gpu_scan_feed_blocks_intents(ybg_scan_t* s, const uint8_t* blocks,
                                    const uint64_t* offsets,
                                    uint64_t n_blocks,
                                    const uint8_t* intents,
                                    uint64_t intents_len,
                                    const ybg_txn_status_t* txns,
                                    uint32_t n_txns) {
  uint8_t* mb = nullptr;
  uint64_t* mo = nullptr;
  uint64_t mn = 0, mt = 0;
  int rc = ybg_merge_intents(blocks, offsets, n_blocks, s->spec.kv_format,
                             intents, intents_len, txns, n_txns, &mb, &mo,
                             &mn, &mt);
  if (rc) return set_err(rc, "intent resolve/merge failed");
  rc = yb_gpu_scan_feed_blocks(s, mb, mo, mn, 0);
  ybg_free(mb);
  ybg_free(mo);
  return rc;
}

// Parse an SST file and report the data-block handles (the same parser
// the feed path uses; exposed for CPU-side tests — errors via
// yb_gpu_last_error).
int ybg_sst_index(const uint8_t* file, uint64_t size, int verify,
                  uint64_t* offsets, uint64_t* sizes, uint64_t cap,
                  uint64_t* n_blocks) {
  std::vector<uint64_t> offs, szs;
  std::vector<uint8_t> typs;
  std::string err;
  int rc = ybsst::parse_sst(file, size, verify, &offs, &szs, &typs, &err);
  if (rc) return set_err(rc, err);
  *n_blocks = offs.size();
  for (uint64_t i = 0; i < offs.size() && i < cap; ++i) {
    offsets[i] = offs[i];
    sizes[i] = szs[i];
  }
  return 0;
}

// Feed a complete SST file: parse footer/index (sst_format.cc), verify
// block checksums, strip the per-block trailers into the concatenated
// block layout and hand over to the existing feed path.
// Feed a complete SST file: footer/index parse host-side (tiny), then
// EVERYTHING block-sized runs on device — k_crc32c verifies every data
// block's masked-crc32c trailer, k_snappy decompresses snappy/LZ4 blocks
// (or copies type-0 blocks) into the concatenated layout the scan
// consumes (rocksdb/table/format.cc responsibilities).
int yb_gpu_scan_feed_sst(ybg_scan_t* s, const uint8_t* file, uint64_t size,
                         int verify_checksums) {
  std::vector<uint64_t> offs, szs;
  std::vector<uint8_t> typs;
  std::string err;
  // verify mode 2: footer + index checksums host-side only; the
  // data-block trailers are verified by k_crc32c below
  int rc = ybsst::parse_sst(file, size, verify_checksums ? 2 : 0, &offs,
                            &szs, &typs, &err);
  if (rc) return set_err(rc, err);
  if (offs.empty()) return set_err(3, "SST file holds no data blocks");
  uint64_t n = offs.size();
  std::vector<uint64_t> un_len(n), boff(n + 1);
  boff[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (typs[i] == 1 || typs[i] == 4) {
      // uncompressed length: snappy uvarint preamble / rocksdb LZ4
      // varint32 framing (both LEB128)
      const uint8_t* p = file + offs[i];
      const uint8_t* lim = p + szs[i];
      uint64_t ulen = 0;
      int shift = 0;
      for (;;) {
        if (p >= lim || shift > 28)
          return set_err(3, "corrupt compressed-block length preamble");
        uint8_t b = *p++;
        ulen |= (uint64_t)(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
      }
      if (ulen >> 32)  // a varint32 holds 32 bits, not the 35 of 5 bytes
        return set_err(3, "corrupt compressed-block length preamble");
      un_len[i] = ulen;
    } else {
      un_len[i] = szs[i];
    }
    boff[i + 1] = boff[i] + un_len[i];
  }
  uint64_t total_un = boff[n];
  uint64_t blob_len = 0;  // cover every listed block + its trailer
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t e2 = offs[i] + szs[i] + ybsst::kBlockTrailerSize;
    if (e2 > blob_len) blob_len = e2;
  }
  if (blob_len > size) blob_len = size;
  uint8_t* d_blob = nullptr;
  uint64_t* d_meta = nullptr;  // src_off | src_len | dst_off
  uint8_t* d_types = nullptr;
  uint8_t* d_out = nullptr;
  unsigned long long* d_err = nullptr;
  HIP_TRY(hipMalloc(&d_blob, blob_len));
  HIP_TRY(hipMemcpy(d_blob, file, blob_len, hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&d_meta, (3 * n + 1) * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(d_meta, offs.data(), n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_meta + n, szs.data(), n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_meta + 2 * n, boff.data(), (n + 1) * 8,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&d_types, n));
  HIP_TRY(hipMemcpy(d_types, typs.data(), n, hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&d_err, 8));
  HIP_TRY(hipMemset(d_err, 0, 8));
  int sgrid = (int)std::min<uint64_t>((n + 255) / 256, 4096);
  if (verify_checksums) {
    hipLaunchKernelGGL(k_crc32c, dim3(sgrid), dim3(256), 0, s->stream,
                       d_blob, d_meta, d_meta + n, n, d_err);
    unsigned long long h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost,
                           s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (h_err) {
      HIP_WARN(hipFree(d_blob));
      HIP_WARN(hipFree(d_meta));
      HIP_WARN(hipFree(d_types));
      HIP_WARN(hipFree(d_err));
      return set_err(3, "data block checksum mismatch (device verify)");
    }
  }
  HIP_TRY(hipMalloc(&d_out, total_un + 256));
  HIP_TRY(hipMemset(d_out + total_un, 0, 256));
  hipLaunchKernelGGL(k_snappy, dim3(sgrid), dim3(256), 0, s->stream, d_blob,
                     d_meta, d_meta + n, d_meta + 2 * n, d_types, n, d_out,
                     total_un, d_err);
  unsigned long long h_err = 0;
  HIP_TRY(hipMemcpyAsync(&h_err, d_err, 8, hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_WARN(hipFree(d_blob));
  HIP_WARN(hipFree(d_meta));
  HIP_WARN(hipFree(d_types));
  HIP_WARN(hipFree(d_err));
  if (h_err) {
    HIP_WARN(hipFree(d_out));
    return set_err(3, "block decompression failed");
  }
  rc = yb_gpu_scan_feed_blocks(s, d_out, boff.data(), n, 1);
  if (rc) {
    HIP_WARN(hipFree(d_out));
    return rc;
  }
  s->d_data_owned = true;  // the decompressed copy is ours to free
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------
// Device part of row materialization (declared in snap_internal.h): the
// flags pre-pass and the emit pass, parameterized on the DevSpec and the
// EmitCtx so yb_gpu_scan_next_batch and the columnar-snapshot build share
// one decoder.
// ---------------------------------------------------------------------
namespace ybgint {

ScanView scan_view(ybg_scan_t* s) {
  ScanView v;
  v.spec = &s->spec;
  v.stream = s->stream;
  v.n_ivs = s->n_ivs;
  v.fed = s->d_data != nullptr;
  v.bloom_rejected = s->bloom_rejected;
  v.pruned_by_options = s->pruned_by_options;
  return v;
}

int scan_flags_pass(ybg_scan_t* s, const DevSpec& d, const uint8_t* d_aux) {
  if (!s->d_flags_all)
    HIP_TRY(hipMalloc(&s->d_flags_all, s->n_ivs * sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(s->d_flags_all, 0, s->n_ivs * sizeof(uint32_t),
                         s->stream));
  // flags pre-pass: resolves head-row ownership for EVERY interval
  // (iv_flags written inside the walk; the bheads/walked side effects of
  // this pass are only folded by scan_flags_stats)
  HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_spec), &d, sizeof(DevSpec), 0,
                                 hipMemcpyHostToDevice, s->stream));
  auto flags_kernel = k_scan<2, 3>;
  hipLaunchKernelGGL(flags_kernel, dim3(s->grid), dim3(kThreads), 0,
                     s->stream, s->d_data, s->d_offsets, s->d_ivs,
                     s->n_ivs, d_aux, s->d_rk_save, s->d_partials,
                     s->d_heads, s->d_walked, s->d_flags_all, 1, s->ivb,
                     s->n_batches, (const uint64_t*)nullptr,
                     (const uint64_t*)nullptr,
                     (const unsigned long long*)nullptr);
  return 0;
}

int scan_flags_stats(ybg_scan_t* s, const DevSpec& d, ScanStats* out) {
  // the flags pass is a k_scan<2,3> dispatch over fixed-ivb batches: head
  // record stride 2*2+2, main partials half only. Folded with the
  // aggregate slots off; the result record is a temporary so the handle's
  // last aggregate result stays intact.
  DevSpec rsp = d;
  rsp.num_aggs = 0;
  DevResult* d_res = nullptr;
  HIP_TRY(hipMalloc(&d_res, sizeof(DevResult)));
  hipLaunchKernelGGL(k_fold, dim3(kFoldGrid), dim3(kFoldThreads), 0,
                     s->stream, rsp, s->d_partials, s->n_partials, s->d_heads,
                     s->d_walked, s->n_batches, 6, s->d_chunk,
                     s->d_fold_ticket, d_res);
  DevResult r;
  hipError_t e = hipMemcpyAsync(&r, d_res, sizeof(r), hipMemcpyDeviceToHost,
                                s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  HIP_WARN(hipFree(d_res));
  if (e != hipSuccess) return set_err(10, hipGetErrorString(e));
  memset(out, 0, sizeof(*out));
  out->entries = r.entries;
  out->scanned = r.scanned;
  out->errs = r.errs;
  out->restart_len = unpack_restart_ht(r.restart_hi, r.restart_lo,
                                       r.restart_len, out->restart_ht);
  return 0;
}

int scan_emit_pass(ybg_scan_t* s, const uint8_t* d_aux, EmitCtx ec,
                   unsigned long long* d_counters,
                   unsigned long long ctr[4]) {
  HIP_TRY(hipMemsetAsync(d_counters, 0, 4 * sizeof(unsigned long long),
                         s->stream));
  ec.row_counter = d_counters + 0;
  ec.varlen_counter = d_counters + 1;
  ec.overflow = d_counters + 2;
  ec.head_consumed = s->d_flags_all;
  int egrid = (int)std::min<uint64_t>(
      (s->n_ivs + kEmitThreads - 1) / kEmitThreads, 8192);
  // emit threads use their own rk_save area sized for the emit grid
  uint64_t need_rk = (uint64_t)egrid * kEmitThreads * kKeyCap;
  uint64_t have_rk = (uint64_t)s->grid * kThreads * kKeyCap;
  uint8_t* rk_area = s->d_rk_save;
  uint8_t* rk_extra = nullptr;
  if (need_rk > have_rk) {
    HIP_TRY(hipMalloc(&rk_extra, need_rk));
    rk_area = rk_extra;
  }
  int nc_pad = ec.nc > 0 ? ec.nc : 1;
  size_t emit_dyn_bytes =
      (size_t)kEmitThreads * nc_pad * (sizeof(uint64_t) + sizeof(uint32_t));
  hipLaunchKernelGGL(k_emit, dim3(egrid), dim3(kEmitThreads),
                     emit_dyn_bytes, s->stream, s->d_data, s->d_offsets,
                     s->d_ivs, s->n_ivs, d_aux, rk_area, ec, d_counters + 3,
                     nc_pad);
  hipError_t e = hipMemcpyAsync(ctr, d_counters,
                                4 * sizeof(unsigned long long),
                                hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (rk_extra) HIP_WARN(hipFree(rk_extra));
  if (e != hipSuccess) return set_err(10, hipGetErrorString(e));
  return 0;
}

}  // namespace ybgint

namespace {

// After a fast execute has finished: merge the batches it aborted (n_late
// ids in d_retry) into the handle's known abort set and upload list and
// bitmap. Runs once per change of the set — the list is a few hundred KB at
// most on the headline tablet.
int known_learn(ybg_scan_t* s, uint64_t n_late) {
  if (!s->known_valid || !(s->known_key == s->last_key)) {
    s->known_ids.clear();
    s->known_key = s->last_key;
    s->known_valid = false;
  }
  if (n_late > s->n_heads) return set_err(10, "retry list overran");
  if (n_late) {
    const size_t old = s->known_ids.size();
    s->known_ids.resize(old + n_late);
    HIP_TRY(hipMemcpy(s->known_ids.data() + old, s->d_retry,
                      n_late * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::sort(s->known_ids.begin(), s->known_ids.end());
    s->known_ids.erase(
        std::unique(s->known_ids.begin(), s->known_ids.end()),
        s->known_ids.end());
    const uint64_t words = s->n_heads / 64 + 1;
    if (!s->d_known) {
      HIP_TRY(hipMalloc(&s->d_known, s->n_heads * sizeof(uint64_t)));
      HIP_TRY(hipMalloc(&s->d_known_n, sizeof(unsigned long long)));
      HIP_TRY(hipMalloc(&s->d_known_bits, words * sizeof(uint64_t)));
    }
    std::vector<uint64_t> bits(words, 0);
    for (uint64_t j : s->known_ids) {
      if (j >= s->n_heads) return set_err(10, "retry list holds a bad id");
      bits[j >> 6] |= 1ull << (j & 63);
    }
    const unsigned long long n = s->known_ids.size();
    HIP_TRY(hipMemcpy(s->d_known, s->known_ids.data(), n * sizeof(uint64_t),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_known_n, &n, sizeof(n), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_known_bits, bits.data(), words * sizeof(uint64_t),
                      hipMemcpyHostToDevice));
  }
  s->known_valid = true;
  return 0;
}

}  // namespace

extern "C" {

int yb_gpu_scan_execute(ybg_scan_t* s) {
  if (s->bloom_rejected) {
    s->executed = true;
    return 0;
  }
  if (!s->d_data) return set_err(4, "feed_blocks not called");
  // YBG_STAGE=1: a plain aggregate scan with stageable predicates and
  // aggregates is answered from a columnar snapshot built on the first
  // execute. Anything else — and a failed build — takes the block path.
  s->staged_last = false;
  s->planned_last = false;
  s->last_retry_batches = 0;
  s->retry_pending = false;
  {
    const char* e = getenv("YBG_STAGE");
    if (e && atoi(e) == 1 && !s->stage_failed && !s->spec.emit_rows &&
        s->spec.group_col == 0 && s->spec.row_limit == 0 &&
        ybgint::stage_eligible(s->spec)) {
      // the query is always the handle's own spec, so a block set pruned
      // by that spec's own option predicate still answers it exactly
      if (!s->stage_snap &&
          ybgint::snapshot_build(s, &s->stage_snap, true) != 0) {
        s->stage_snap = nullptr;
        s->stage_failed = true;
      }
      if (s->stage_snap) {
        int rc = ybgint::stage_launch(s->stage_snap, s->spec);
        if (rc) return rc;
        s->staged_last = true;
        s->executed = true;
        return 0;
      }
    }
  }
  HIP_TRY(hipEventRecord(s->ev_start, s->stream));
  HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_spec), &s->dspec,
                                 sizeof(DevSpec), 0, hipMemcpyHostToDevice,
                                 s->stream));
  int na = s->na_cap;
  bool usefast = fast_eligible(s->dspec) && na == 2;
  if (const char* e = getenv("YBG_FAST")) usefast = usefast && atoi(e) != 0;
  // Block-aligned batches keep lanes phase-locked on the restart cadence;
  // they win when the adaptive batch would exceed a block's interval
  // count (measured: MVCC +13%, headline -3%), so auto-enable exactly
  // there. YBG_BB=0/1 overrides.
  bool use_bb = s->n_blocks > 0 &&
                s->ivb * s->n_blocks >= s->n_ivs;  // ivb >= avg ivs/block
  if (const char* e = getenv("YBG_BB")) use_bb = atoi(e) != 0;
  const uint64_t n_bat = use_bb ? s->n_blocks : s->n_batches;
  const uint64_t* bat_lo = use_bb ? s->d_batch_lo : nullptr;
  // partial records the fold reads: the main half, plus exactly the
  // records a retry launch writes (the rest of the retry half is never
  // initialized)
  uint64_t n_fold = s->n_partials;
  if (usefast) {
    HIP_TRY(hipMemsetAsync(s->d_retry_n, 0, sizeof(unsigned long long),
                           s->stream));
    // NC: compile-time column cap for the unrolled load pass (spec is
    // zero-padded up to it; fast_eligible caps num_value_cols at 8).
    // fuse: version-chain decode shape per the spec's expect_versions
    // hint. 3 waves/SIMD is the measured optimum.
    const bool nc4 = s->dspec.num_value_cols <= 4;
    bool fuse = s->dspec.fuse_hint != 0;
    if (const char* e = getenv("YBG_FUSE")) fuse = atoi(e) != 0;
    // a plannable query runs the planned kernel: its packed-row pass is
    // compiled from the spec here, once, instead of interpreted per row
    FastPlan plan;
    s->planned_last = build_fast_plan(s->dspec, &plan) && fast_plan_enabled();
    const int nr = s->planned_last ? fast_plan_nr(plan) : 0;

    // Known abort set. Which batches the fast kernel aborts depends on the
    // entry encodings in the immutable block bytes and on the batch
    // decomposition, not on the query, so the list one execute produced is
    // known before the next one starts: the general kernel then runs it on
    // a second stream NEXT TO the fast kernel instead of after it, and the
    // fast kernel skips those batches by bitmap.
    // INVARIANT: any batch may be run by the general kernel, and a batch
    // the fast kernel aborts that the set did not predict is still
    // appended to the late list and run by the late launch below. A stale
    // or wrong set can therefore cost time and can never change a result.
    // The set is dropped when its key (batch decomposition, kernel
    // variant) changes and at feed; YBG_KNOWN=0 keeps every execute on the
    // serial order.
    ybg_scan::KnownKey key;
    key.n_bat = n_bat;
    key.ivb = s->ivb;
    key.bb = use_bb;
    key.variant = (s->planned_last ? 64 : 0) | (fuse ? 32 : 0) |
                  (s->planned_last ? nr : (nc4 ? 4 : 8));
    bool learn = true;
    if (const char* e = getenv("YBG_KNOWN")) learn = atoi(e) != 0;
    if (s->known_valid && !(s->known_key == key)) s->known_valid = false;
    const bool use_known = learn && s->known_valid && !s->known_ids.empty();
    s->last_key = key;
    s->last_learn = learn;
    s->last_known_n = use_known ? s->known_ids.size() : 0;

    const int rg = std::min(s->grid, 1024);
    auto general_kernel = k_scan<2, 3>;
    // the general kernel over a batch id list, into its own partials region
    auto launch_list = [&](hipStream_t st, int g, uint64_t* region,
                           const uint64_t* ids,
                           const unsigned long long* n_ids) {
      hipLaunchKernelGGL(general_kernel, dim3(g), dim3(kThreads), 0, st,
                         s->d_data, s->d_offsets, s->d_ivs, s->n_ivs,
                         s->d_aux, s->d_rk_save, region, s->d_heads,
                         s->d_walked, nullptr, 0, s->ivb, n_bat, bat_lo, ids,
                         n_ids);
    };
    uint64_t* region1 = s->d_partials + s->n_partials * kPartialStride;
    if (use_known) {
      // fork after the c_spec upload; enqueued before the fast kernel so
      // its workgroups get placed first
      HIP_TRY(hipEventRecord(s->ev_fork, s->stream));
      HIP_TRY(hipStreamWaitEvent(s->stream2, s->ev_fork, 0));
      launch_list(s->stream2, rg, region1, s->d_known, s->d_known_n);
      HIP_TRY(hipEventRecord(s->ev_join, s->stream2));
    }
    const uint64_t* known_bits = use_known ? s->d_known_bits : nullptr;
    auto launchf = [&](auto kern, auto plan) {
      hipLaunchKernelGGL(kern, dim3(s->grid), dim3(kThreads), 0, s->stream,
                         s->d_data, s->d_offsets, s->d_ivs, s->n_ivs,
                         s->d_partials, s->d_heads, s->d_walked, s->ivb,
                         n_bat, bat_lo, s->d_retry, s->d_retry_n, known_bits,
                         plan);
    };
    if (s->planned_last) {
      // compiled per ranged-column count, so the pass has no guards
      auto launchp = [&](auto nr_tag) {
        constexpr int NR = decltype(nr_tag)::value;
        if (fuse) launchf(k_scan_fast<3, NR, true, true>, plan);
        else launchf(k_scan_fast<3, NR, false, true>, plan);
      };
      switch (nr) {
        case 0: launchp(std::integral_constant<int, 0>{}); break;
        case 1: launchp(std::integral_constant<int, 1>{}); break;
        case 2: launchp(std::integral_constant<int, 2>{}); break;
        case 3: launchp(std::integral_constant<int, 3>{}); break;
        case 4: launchp(std::integral_constant<int, 4>{}); break;
        case kPlanShapeP1:
          launchp(std::integral_constant<int, kPlanShapeP1>{});
          break;
        case kPlanShapeP1S1:
          launchp(std::integral_constant<int, kPlanShapeP1S1>{});
          break;
        case kPlanShapeP2:
          launchp(std::integral_constant<int, kPlanShapeP2>{});
          break;
        default: launchp(std::integral_constant<int, 8>{}); break;
      }
    } else if (fuse) {
      if (nc4) launchf(k_scan_fast<3, 4, true>, NoPlan{});
      else launchf(k_scan_fast<3, 8, true>, NoPlan{});
    } else {
      if (nc4) launchf(k_scan_fast<3, 4>, NoPlan{});
      else launchf(k_scan_fast<3, 8>, NoPlan{});
    }
    if (use_known) {
      // join, then a small launch drains the batches the set did not
      // predict (after the join: it shares the per-thread key save area
      // with the known-list launch)
      HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_join, 0));
      const int lg = std::min(rg, 64);
      launch_list(s->stream, lg,
                  region1 + (uint64_t)rg * (kThreads / 64) * kPartialStride,
                  s->d_retry, s->d_retry_n);
      n_fold += (uint64_t)(rg + lg) * (kThreads / 64);
    } else {
      // retry pass: the general kernel over the aborted batch list
      launch_list(s->stream, rg, region1, s->d_retry, s->d_retry_n);
      n_fold += (uint64_t)rg * (kThreads / 64);
    }
  } else {
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(s->grid), dim3(kThreads), 0, s->stream,
                         s->d_data, s->d_offsets, s->d_ivs, s->n_ivs,
                         s->d_aux, s->d_rk_save, s->d_partials, s->d_heads,
                         s->d_walked, nullptr, 0, s->ivb, n_bat, bat_lo,
                         (const uint64_t*)nullptr,
                         (const unsigned long long*)nullptr);
    };
    // dispatch on aggregate-slot capacity (register footprint), each at
    // its measured waves-per-SIMD bound: 3 for the 2-agg shape; the 4-agg
    // kernel at 3 waves carries 240 B/lane of scratch spills vs 0 at 2
    // waves, so it runs at 2; the 8-agg kernel spills either way and
    // keeps 3
    if (na == 2) launch(k_scan<2, 3>);
    else if (na == 4) launch(k_scan<4, 2>);
    else launch(k_scan<8, 3>);
  }
  HIP_TRY(hipEventRecord(s->ev_mid, s->stream));
  hipLaunchKernelGGL(k_fold, dim3(kFoldGrid), dim3(kFoldThreads), 0,
                     s->stream, s->dspec, s->d_partials, n_fold, s->d_heads,
                     s->d_walked, n_bat, s->hstride, s->d_chunk,
                     s->d_fold_ticket, s->d_result);
  HIP_TRY(hipEventRecord(s->ev_end, s->stream));
  if (usefast) {
    // the abort count comes back with the result (pinned, no extra sync)
    HIP_TRY(hipMemcpyAsync(s->h_retry_n, s->d_retry_n,
                           sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           s->stream));
    s->retry_pending = true;
  }
  s->executed = true;
  return 0;
}

int yb_gpu_scan_wait(ybg_scan_t* s) {
  if (!s->executed) return set_err(5, "execute not called");
  if (s->staged_last) {
    double ms = 0;
    int rc = ybgint::stage_finish(s->stage_snap, s->spec, nullptr, &ms);
    if (rc) return rc;
    s->last_decode_ms = s->last_total_ms = ms;
    return 0;
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  float ms1 = 0, ms2 = 0;
  HIP_TRY(hipEventElapsedTime(&ms1, s->ev_start, s->ev_mid));
  HIP_TRY(hipEventElapsedTime(&ms2, s->ev_start, s->ev_end));
  s->last_decode_ms = ms1;
  s->last_total_ms = ms2;
  if (s->retry_pending) {
    s->retry_pending = false;
    const uint64_t n_late = *s->h_retry_n;
    s->last_retry_batches = s->last_known_n + n_late;
    // late aborts are merged into the set; a first execute creates it
    if (s->last_learn && (n_late || !s->known_valid ||
                          !(s->known_key == s->last_key))) {
      int rc = known_learn(s, n_late);
      if (rc) return rc;
    }
  }
  return 0;
}

int yb_gpu_scan_aggregate(ybg_scan_t* s, ybg_scan_result_t* out) {
  if (s->bloom_rejected) {
    memset(out, 0, sizeof(*out));
    for (int g = 0; g < s->spec.num_aggs; ++g) out->aggs[g].is_null = 1;
    return 0;
  }
  int rc = yb_gpu_scan_wait(s);
  if (rc) return rc;
  if (s->staged_last) {
    double ms = 0;
    return ybgint::stage_finish(s->stage_snap, s->spec, out, &ms);
  }
  DevResult r;
  HIP_TRY(hipMemcpy(&r, s->d_result, sizeof(r), hipMemcpyDeviceToHost));
  if (r.errs) return set_err(6, "corrupt entries encountered during scan");
  memset(out, 0, sizeof(*out));
  out->entries_seen = r.entries;
  out->rows_scanned = r.scanned;
  out->rows_matched = r.matched;
  out->restart_ht_len = unpack_restart_ht(r.restart_hi, r.restart_lo,
                                          r.restart_len, out->restart_ht);
  for (int g = 0; g < s->spec.num_aggs; ++g) {
    ybg_agg_result_t& a = out->aggs[g];
    a.is_null = (r.agg_cnt[g] == 0);
    switch (s->spec.aggs[g].op) {
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
  return 0;
}

int yb_gpu_scan_next_batch(ybg_scan_t* s, ybg_row_batch_t* out) {
  if (s->bloom_rejected) {
    memset(out, 0, sizeof(*out));
    return 0;
  }
  if (!s->d_data) return set_err(4, "feed_blocks not called");
  int nk = s->spec.schema.num_hash_cols + s->spec.schema.num_range_cols;
  int nc = s->spec.schema.num_value_cols;
  if (!s->d_em_sort) {
    s->emit_row_cap = std::min<uint64_t>(s->n_ivs * 16ull, 32ull << 20);
    s->em_varlen_cap =
        std::min<uint64_t>(s->total_bytes + (1ull << 20), 1ull << 30);
    HIP_TRY(hipMalloc(&s->d_em_sort, s->emit_row_cap * 8));
    HIP_TRY(hipMalloc(&s->d_em_key, s->emit_row_cap * 8 * (nk ? nk : 1)));
    HIP_TRY(hipMalloc(&s->d_em_dat, s->emit_row_cap * 8 * (nc ? nc : 1)));
    HIP_TRY(hipMalloc(&s->d_em_null, s->emit_row_cap * 4));
    HIP_TRY(hipMalloc(&s->d_em_hash, s->emit_row_cap * 2));
    HIP_TRY(hipMalloc(&s->d_em_varlen, s->em_varlen_cap));
    HIP_TRY(hipMalloc(&s->d_em_counters, 4 * sizeof(unsigned long long)));
  }
  EmitCtx ec;
  ec.sort_key = s->d_em_sort;
  ec.key_datums = s->d_em_key;
  ec.datums = s->d_em_dat;
  ec.null_masks = s->d_em_null;
  ec.hashes = s->d_em_hash;
  ec.varlen = s->d_em_varlen;
  ec.varlen_cap = s->em_varlen_cap;
  ec.row_cap = s->emit_row_cap;
  ec.nk = nk;
  ec.nc = nc;
  unsigned long long ctr[4];
  int rc = ybgint::scan_flags_pass(s, s->dspec, s->d_aux);
  if (rc) return rc;
  rc = ybgint::scan_emit_pass(s, s->d_aux, ec, s->d_em_counters, ctr);
  if (rc) return rc;
  if (ctr[3]) return set_err(6, "corrupt entries encountered during scan");
  if (ctr[2]) return set_err(8, "row batch capacity exceeded");
  uint64_t n_rows = ctr[0];
  uint64_t vl = ctr[1];
  s->h_sort.resize(n_rows);
  s->h_key.resize(n_rows * (nk ? nk : 1));
  s->h_dat.resize(n_rows * (nc ? nc : 1));
  s->h_null.resize(n_rows);
  s->h_hash.resize(n_rows);
  s->h_varlen.resize(vl ? vl : 1);
  if (n_rows) {
    HIP_TRY(hipMemcpy(s->h_sort.data(), s->d_em_sort, n_rows * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s->h_key.data(), s->d_em_key, n_rows * 8 * (nk ? nk : 1),
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s->h_dat.data(), s->d_em_dat, n_rows * 8 * (nc ? nc : 1),
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s->h_null.data(), s->d_em_null, n_rows * 4,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s->h_hash.data(), s->d_em_hash, n_rows * 2,
                      hipMemcpyDeviceToHost));
  }
  if (vl)
    HIP_TRY(hipMemcpy(s->h_varlen.data(), s->d_em_varlen, vl,
                      hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  out->n_rows = n_rows;
  out->n_key_cols = (uint64_t)nk;
  out->n_value_cols = (uint64_t)nc;
  out->sort_key = s->h_sort.data();
  out->key_datums = s->h_key.data();
  out->datums = s->h_dat.data();
  out->null_masks = s->h_null.data();
  out->hashes = s->h_hash.data();
  out->varlen = s->h_varlen.data();
  out->varlen_size = vl;
  return 0;
}

int yb_gpu_scan_group_aggregate(ybg_scan_t* s, uint64_t* keys,
                                int64_t* vals, uint64_t* cnts,
                                uint8_t* key_bytes, uint64_t key_bytes_cap,
                                uint64_t cap, uint64_t* n_groups) {
  if (!s->d_data) return set_err(4, "feed_blocks not called");
  if (s->dspec.group_col < 0)
    return set_err(9, "spec.group_col not set");
  if (!s->gc.gkey) {
    s->group_cap = 1ull << 20;  // 1M groups
    HIP_TRY(hipMalloc(&s->gc.gkey,
                      (s->group_cap + 1) * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&s->gc.state, (s->group_cap + 1) * sizeof(unsigned)));
    HIP_TRY(hipMalloc(&s->gc.vals, (s->group_cap + 1) * YBG_MAX_AGGS * 8));
    HIP_TRY(hipMalloc(&s->gc.cnts, (s->group_cap + 1) * YBG_MAX_AGGS * 8));
    HIP_TRY(hipMalloc(&s->gc.vals_hi,
                      (s->group_cap + 1) * YBG_MAX_AGGS * 8));
    HIP_TRY(hipMalloc(&s->gc.poison,
                      (s->group_cap + 1) * YBG_MAX_AGGS * 4));
    HIP_TRY(hipMalloc(&s->gc.overflow, sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&s->d_g_counters, 4 * sizeof(unsigned long long)));
    s->gc.cap = s->group_cap;
    s->gc.data = s->d_data;
    HIP_TRY(hipMalloc(&s->d_gheads, s->n_gheads * sizeof(GroupHead)));
  }
  HIP_TRY(hipMemsetAsync(s->gc.overflow, 0, 8, s->stream));
  s->group_done = false;
  HIP_TRY(hipMemsetAsync(s->d_g_counters, 0, 32, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_gheads, 0, s->n_gheads * sizeof(GroupHead),
                         s->stream));
  HIP_TRY(hipMemsetAsync(s->d_cont, 0, s->n_gheads * sizeof(uint32_t),
                         s->stream));
  hipLaunchKernelGGL(k_group_init, dim3(512), dim3(256), 0, s->stream,
                     s->dspec, s->gc);
  HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_spec), &s->dspec,
                                 sizeof(DevSpec), 0, hipMemcpyHostToDevice,
                                 s->stream));
  // single fused pass: head-deferral protocol identical to k_scan
  int hgrid = (int)std::min<uint64_t>(
      (s->n_ivs + kThreads - 1) / kThreads, 512);
  if (s->dspec.track_restart) {
    // k_group writes only the restart slots of each wave partial; zero the
    // rest so the k_reduce fold below sees clean records
    HIP_TRY(hipMemsetAsync(s->d_partials, 0,
                           s->n_partials * kPartialStride * sizeof(uint64_t),
                           s->stream));
  }
  auto launch_group = [&](auto kern, auto kern_heads) {
    hipLaunchKernelGGL(kern, dim3(s->grid), dim3(kThreads), 0,
                       s->stream, s->d_data, s->d_offsets, s->d_ivs,
                       s->n_ivs, s->d_aux, s->d_rk_save, s->gc, s->d_gheads,
                       s->d_cont, s->gc.overflow, s->d_partials, s->ivb);
    hipLaunchKernelGGL(kern_heads, dim3(hgrid), dim3(kThreads), 0,
                       s->stream, s->gc, s->d_gheads, s->d_cont,
                       s->n_gheads);
  };
  if (s->dspec.num_aggs <= 4) {
    launch_group(k_group<4, 3>, k_group_heads<4>);
  } else {
    launch_group(k_group<8, 3>, k_group_heads<8>);
  }
  if (s->dspec.track_restart) {
    // fold the wave restart minima into DevResult (num_aggs = 0 spec: only
    // the restart slots matter; n_heads = 0 skips the head records)
    DevSpec rsp = s->dspec;
    rsp.num_aggs = 0;
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s->stream, rsp,
                       s->d_partials, s->n_partials, s->d_heads, s->d_cont,
                       0, s->d_result);
  } else {
    // restart impossible (local_limit == read): restart_data reports none
    HIP_TRY(hipMemsetAsync(s->d_result, 0, sizeof(DevResult), s->stream));
  }
  // export buffers sized to caller caps
  if (!s->d_gk_out) {
    HIP_TRY(hipMalloc(&s->d_gk_out, cap * 8));
    HIP_TRY(hipMalloc(&s->d_gv_out, cap * YBG_MAX_AGGS * 8));
    HIP_TRY(hipMalloc(&s->d_gc_out, cap * YBG_MAX_AGGS * 8));
    HIP_TRY(hipMalloc(&s->d_gb_out, key_bytes_cap ? key_bytes_cap : 1));
  }
  hipLaunchKernelGGL(k_group_export, dim3(512), dim3(256), 0, s->stream,
                     s->dspec, s->gc, s->d_gk_out, s->d_gv_out, s->d_gc_out,
                     s->d_gb_out, key_bytes_cap, cap, s->d_g_counters);
  unsigned long long ctr[4];
  unsigned long long errs = 0;
  HIP_TRY(hipMemcpyAsync(ctr, s->d_g_counters, 32, hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipMemcpyAsync(&errs, s->gc.overflow, 8, hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (errs) return set_err(6, "corrupt entries or group table overflow");
  if (ctr[2]) return set_err(8, "group output capacity exceeded");
  uint64_t ng = ctr[0];
  *n_groups = ng;
  if (ng) {
    HIP_TRY(hipMemcpy(keys, s->d_gk_out, ng * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals, s->d_gv_out, ng * YBG_MAX_AGGS * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cnts, s->d_gc_out, ng * YBG_MAX_AGGS * 8,
                      hipMemcpyDeviceToHost));
  }
  if (ctr[1] && key_bytes)
    HIP_TRY(hipMemcpy(key_bytes, s->d_gb_out,
                      std::min<uint64_t>(ctr[1], key_bytes_cap),
                      hipMemcpyDeviceToHost));
  s->group_null_index = ctr[3] ? (int64_t)ctr[3] - 1 : -1;
  s->group_done = true;
  return 0;
}

int yb_gpu_scan_group_null_index(ybg_scan_t* s, int64_t* index_out) {
  if (!s->group_done)
    return set_err(4, "no successful group_aggregate on this handle");
  *index_out = s->group_null_index;
  return 0;
}

// Read-restart data of the last execute/group_aggregate on this handle
// (GetReadRestartData analog, intent_aware_iterator.cc:1400-1410): the
// encoded DocHybridTime of the smallest-encoded (max commit time) visible
// record past the read time, or len 0 when no restart is needed. The
// aggregate path also surfaces this in ybg_scan_result_t; this entry point
// serves the GROUP BY path, whose result shape has no restart field.
int yb_gpu_scan_restart_data(ybg_scan_t* s, uint8_t* ht_out,
                             uint32_t* len_out) {
  if (s->bloom_rejected) {
    *len_out = 0;
    return 0;
  }
  if (s->staged_last) {  // the snapshot carries its build scan's data
    ybg_scan_result_t res;
    double ms = 0;
    int rc = ybgint::stage_finish(s->stage_snap, s->spec, &res, &ms);
    if (rc) return rc;
    memcpy(ht_out, res.restart_ht, res.restart_ht_len);
    *len_out = res.restart_ht_len;
    return 0;
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  DevResult r;
  HIP_TRY(hipMemcpy(&r, s->d_result, sizeof(r), hipMemcpyDeviceToHost));
  *len_out = unpack_restart_ht(r.restart_hi, r.restart_lo, r.restart_len,
                               ht_out);
  return 0;
}

int yb_gpu_scan_paging_state(ybg_scan_t* s, uint8_t* key_out, size_t cap,
                             size_t* len_out) {
  (void)key_out;
  (void)cap;
  // Paging needs delivered-row ordering, which the batch ABI leaves to the
  // row-at-a-time adapter (GpuDocRowwiseIterator::PagingState — the
  // GetSubDocKey analog, ql_rowwise_iterator_interface.h:32-97). An
  // unlimited scan is simply complete.
  if (s->spec.row_limit != 0)
    return set_err(9,
                   "row_limit paging state is tracked by the iterator "
                   "adapter (yb_host_iter_paging_state)");
  *len_out = 0;
  return 0;
}

int yb_gpu_scan_kernel_ms(ybg_scan_t* s, double* total_ms, double* decode_ms) {
  *total_ms = s->last_total_ms;
  *decode_ms = s->last_decode_ms;
  return 0;
}

int yb_gpu_scan_staged(ybg_scan_t* s) { return s->staged_last ? 1 : 0; }

int yb_gpu_scan_planned(ybg_scan_t* s) { return s->planned_last ? 1 : 0; }

int yb_gpu_scan_retry_batches(ybg_scan_t* s, uint64_t* n_out) {
  *n_out = 0;
  if (s->bloom_rejected || !s->executed) return 0;
  int rc = yb_gpu_scan_wait(s);
  if (rc) return rc;
  *n_out = s->last_retry_batches;
  return 0;
}

int yb_gpu_scan_close(ybg_scan_t* s) {
  if (s->stage_snap) yb_gpu_snapshot_close(s->stage_snap);
  if (s->d_data_owned && s->d_data) HIP_WARN(hipFree(s->d_data));
  if (s->d_offsets) HIP_WARN(hipFree(s->d_offsets));
  if (s->d_ivs) HIP_WARN(hipFree(s->d_ivs));
  if (s->d_batch_lo) HIP_WARN(hipFree(s->d_batch_lo));
  if (s->d_aux) HIP_WARN(hipFree(s->d_aux));
  if (s->d_rk_save) HIP_WARN(hipFree(s->d_rk_save));
  if (s->d_partials) HIP_WARN(hipFree(s->d_partials));
  if (s->d_heads) HIP_WARN(hipFree(s->d_heads));
  if (s->d_cont) HIP_WARN(hipFree(s->d_cont));
  if (s->d_result) HIP_WARN(hipFree(s->d_result));
  if (s->d_chunk) HIP_WARN(hipFree(s->d_chunk));
  if (s->d_fold_ticket) HIP_WARN(hipFree(s->d_fold_ticket));
  if (s->d_walked) HIP_WARN(hipFree(s->d_walked));
  if (s->d_retry) HIP_WARN(hipFree(s->d_retry));
  if (s->d_retry_n) HIP_WARN(hipFree(s->d_retry_n));
  if (s->h_retry_n) HIP_WARN(hipHostFree(s->h_retry_n));
  if (s->d_known) HIP_WARN(hipFree(s->d_known));
  if (s->d_known_n) HIP_WARN(hipFree(s->d_known_n));
  if (s->d_known_bits) HIP_WARN(hipFree(s->d_known_bits));
  if (s->d_flags_all) HIP_WARN(hipFree(s->d_flags_all));
  if (s->d_em_sort) HIP_WARN(hipFree(s->d_em_sort));
  if (s->d_em_key) HIP_WARN(hipFree(s->d_em_key));
  if (s->d_em_dat) HIP_WARN(hipFree(s->d_em_dat));
  if (s->d_em_null) HIP_WARN(hipFree(s->d_em_null));
  if (s->d_em_hash) HIP_WARN(hipFree(s->d_em_hash));
  if (s->d_em_varlen) HIP_WARN(hipFree(s->d_em_varlen));
  if (s->d_em_counters) HIP_WARN(hipFree(s->d_em_counters));
  if (s->gc.gkey) HIP_WARN(hipFree(s->gc.gkey));
  if (s->gc.state) HIP_WARN(hipFree(s->gc.state));
  if (s->gc.vals) HIP_WARN(hipFree(s->gc.vals));
  if (s->gc.cnts) HIP_WARN(hipFree(s->gc.cnts));
  if (s->gc.vals_hi) HIP_WARN(hipFree(s->gc.vals_hi));
  if (s->gc.poison) HIP_WARN(hipFree(s->gc.poison));
  if (s->gc.overflow) HIP_WARN(hipFree(s->gc.overflow));
  if (s->d_gheads) HIP_WARN(hipFree(s->d_gheads));
  if (s->d_g_counters) HIP_WARN(hipFree(s->d_g_counters));
  if (s->d_gk_out) HIP_WARN(hipFree(s->d_gk_out));
  if (s->d_gv_out) HIP_WARN(hipFree(s->d_gv_out));
  if (s->d_gc_out) HIP_WARN(hipFree(s->d_gc_out));
  if (s->d_gb_out) HIP_WARN(hipFree(s->d_gb_out));
  if (s->ev_start) HIP_WARN(hipEventDestroy(s->ev_start));
  if (s->ev_mid) HIP_WARN(hipEventDestroy(s->ev_mid));
  if (s->ev_end) HIP_WARN(hipEventDestroy(s->ev_end));
  if (s->ev_fork) HIP_WARN(hipEventDestroy(s->ev_fork));
  if (s->ev_join) HIP_WARN(hipEventDestroy(s->ev_join));
  if (s->stream2) HIP_WARN(hipStreamDestroy(s->stream2));
  if (s->stream) HIP_WARN(hipStreamDestroy(s->stream));
  delete s;
  return 0;
}

}  // extern "C"
