// The arithmetic of a workspace plan (workspace.hip: ensure_workspace): slab sizes, bytes per slot, rank head-room, slots per chunk, the fit
// into an arena whose growth stopped short, and the engine choice; and of a posterior query's staging (query.h): trials per chunk, columns per block.  Pure functions of the dimensions and of byte counts - standard library only,
// no device call, no context - so that every rule stands once and tests/host/plan_check.cpp can run it without a GPU.  The expressions keep
// the types and the order of operations they had inside ensure_workspace: the integers must not move.
#pragma once
#include <algorithm>
#include <cstddef>

namespace plan {

struct Dims {
  int ld, npad, n, rpad, Tp, T, p;               // of the context (pgpfa_ctx)
  int NB = 128, WIDE_MAX = 32;                   // diagonal block / GEMM tile (types.h); widest latent state of the low-rank engine (model.h) - core.hip checks both
};

struct Slabs { size_t slab, mt; };               // doubles per slot of the factor slabs (H / Yt) and of the L^-T slabs

// per-slot scratch (doubles) the low-rank covariance engine needs inside a factor slab
inline size_t lowrank_slab_elems(const Dims& d) {
  // Yt (ld x rpad), then either the staging of per-trial blocks (Tp x rpad + T^2) or the single-precision correction D of the split
  // accumulation (ld x rpad floats)
  const size_t yt = (size_t)d.ld * d.rpad;
  const size_t need = yt + std::max((size_t)d.Tp * d.rpad + (size_t)d.T * d.T, yt / 2 + 64);
  return std::max(need, (size_t)d.rpad * d.rpad);
}

inline size_t dense_elems(const Dims& d) { return (size_t)d.ld * d.ld; }

// the slabs a plan cannot do with less than
inline Slabs base_slabs(const Dims& d, bool plan_lr) {
  const size_t dense = dense_elems(d);
  // the L^-T slabs only ever hold r x r under the low-rank plan (the big slab is the one that carries Yt)
  return {plan_lr ? (lowrank_slab_elems(d) + 1023) / 1024 * 1024 : dense, plan_lr ? ((size_t)d.rpad * d.rpad + 1023) / 1024 * 1024 : dense};
}

// engine choice: the low-rank form pays when r << n (long timescales); the dense form is the general one
// (round 5: measured at both ends - bench.py --workload floor, tests/test_gpu_round5.py - the low-rank engine is still 9 % faster at a flop
// ratio of 1.6 (100 x 5 x 400, every timescale 3 bins: rank 1520 of 2000) and 23 % at 1.1 (200 x 10 x 500, rank 3856 of 5000: 218 against 284 ms
// per EM iteration of 128 trials): its cubic term runs on r x r systems, its T^2 term mostly on the FP16 / FP32 matrix cores, and the dense engine
// reaches 41 TFLOP/s on 0.72 n^3.  The old rule - ratio below 0.5 and rank at most half of n - sent all of that to the dense engine.)
inline bool lowrank_pays(const Dims& d) {
  const double n = d.n, r = d.rpad, T = d.T, p = d.p;
  if (d.p > d.WIDE_MAX || d.rpad < d.NB || (size_t)d.rpad > (size_t)d.ld) return false;
  const double dense = 0.72 * n * n * n;
  const double lr = 6.0 * T * r * r + 0.7 * r * r * r + p * T * T * r;
  // (small systems - configs 1 and 2 - are launch-bound under either engine and the dense one has fewer launches: there the old rule stands)
  if (d.npad < 1536) return d.rpad * 2 <= d.npad && lr < 0.5 * dense;
  return lr < 1.7 * dense;
}

// (cov_mode 2 forces the low-rank engine at any size it supports - its slabs are sized for what it needs, not by the dense ld x ld; the
// padded rank must fit the n-sized buffers of the shared preconditioner, which near-full-rank priors - timescales of a bin or two,
// every latent's rank rounded up to 16 - can exceed: those run the dense engine)
inline bool want_lowrank(const Dims& d, int cov_mode) {
  return cov_mode == 2 ? (d.p <= d.WIDE_MAX && d.rpad >= d.NB && d.rpad <= d.ld) : (cov_mode == 0 && lowrank_pays(d));
}

inline size_t ld_bytes(const Dims& d) { return (size_t)d.ld * d.ld * sizeof(double); }

inline size_t per_slot_bytes(const Dims& d, size_t slab_elems, size_t mt_elems) {
  const size_t ld = d.ld;
  size_t dbl = slab_elems + mt_elems + 2 * ld * d.NB + 12 * ld + 3 * (size_t)d.T * d.p * d.p + (size_t)d.T * (d.p * (d.p + 1) / 2) / 2 + 3 * ((d.T + 63) / 64) + 32;
  return dbl * sizeof(double);
}

// what a chunk needs whatever its slot count: the shared preconditioner's factor workspace and the slack behind the slot vectors
inline size_t shared_bytes(const Dims& d) { return (3 * ld_bytes(d) + 1024 * (size_t)d.ld * sizeof(double) * 4); }

// the slabs with head-room for the ranks to grow by the factor hh (Yt slab x hh, r x r slab x hh^2), capped at the dense slab
inline Slabs scaled_slabs(const Dims& d, Slabs base, double hh) {
  const size_t dense = dense_elems(d);
  return {std::max(base.slab, std::min(dense, (size_t)((double)base.slab * hh) / 1024 * 1024)),
          std::max(base.mt, std::min(dense, (size_t)((double)base.mt * hh * hh) / 1024 * 1024))};
}
inline size_t list_bytes(const Dims& d, Slabs s, int target) { return per_slot_bytes(d, s.slab, s.mt) * (size_t)std::max(target, 1); }

// (round 6) a RE-plan prefers the largest head-room that fits into the memory the arena already holds - re-partitioning costs nothing, mapping may
// cost seconds (arena_grow) - and otherwise grows for a quarter of head-room only; the first plan of a context takes the full factor
// (headroom: option workspace_headroom; arena_cap: bytes the arena holds, 0 while there is none)
inline double headroom_pick(const Dims& d, Slabs base, double headroom, size_t arena_cap, int target) {
  const double h = std::max(1.0, headroom);
  const size_t shared_b = shared_bytes(d) + ((size_t)64 << 20);
  const size_t mapped = arena_cap > shared_b ? arena_cap - shared_b : 0;
  if (arena_cap > 0)
    for (double hh : {h, 1.75, 1.5, 1.25, 1.1})
      if (hh <= h && list_bytes(d, scaled_slabs(d, base, hh), target) <= mapped) return hh;
  return arena_cap > 0 ? std::min(h, 1.25) : h;
}
// the slabs of a low-rank plan: those of the picked head-room when the whole trial list fits the budget with them, else the bare ones
inline Slabs headroom_slabs(const Dims& d, Slabs base, double headroom, size_t arena_cap, size_t budget, int target) {
  const Slabs want = scaled_slabs(d, base, headroom_pick(d, base, headroom, arena_cap, target));
  return list_bytes(d, want, target) <= budget ? want : base;
}

// the chunks of a list of `target` trials balanced: as many chunks as B slots make necessary, each of the same size rounded up to a group of 8
inline long long balance_slots(long long B, long long target) {
  const long long nchunks = (target + B - 1) / B;
  return std::min(B, ((target + nchunks - 1) / nchunks + 7) / 8 * 8);
}

struct Slots {
  long long B;                                   // slots per chunk; below 1: not one trial fits
  bool capped;                                   // memory (or chunk_trials) bound: asking again would not give more
};
// fit: slots the budget holds (budget / per_slot_bytes); chunk_opt: option chunk_trials (0: not set)
inline Slots slot_count(size_t fit, int chunk_opt, int target) {
  long long B = (long long)fit;
  if (chunk_opt > 0) B = std::min<long long>(B, chunk_opt);
  const bool capped = B < target;
  if (B >= target) B = target;                                   // everything in one chunk
  else if (B >= 16) B = balance_slots(B / 8 * 8, target);        // groups of 8 slots map onto the 8 XCDs
  return {B, capped};
}

struct Fit {
  int B;                                         // slots per chunk
  size_t need;                                   // bytes they measure
  bool capped;                                   // half the list per chunk is good enough to stay with until the ranks ask for a new plan; less than that keeps growing at every call
  bool short_of_floor;                           // not even floor_slots fit arena_cap
};
// The growth's budget ran out (arena_cap < need): the largest balanced chunk that fits what is mapped.  need / must: bytes B_full / floor_slots slots
// measure (must <= arena_cap); bytes_for(n): bytes n slots measure.  The first guess interpolates between the two, then the walk goes down by 8.
template <typename BytesFor>
Fit fit_slots(size_t need, size_t must, size_t arena_cap, int B_full, int floor_slots, int target, BytesFor&& bytes_for) {
  const double per_b = (double)(need - must) / (double)std::max(1, B_full - floor_slots);
  int B_fit = floor_slots + (int)((double)(arena_cap - must) / std::max(per_b, 1.0));
  B_fit = std::max(floor_slots, std::min(B_full, B_fit / 8 * 8));
  B_fit = std::max(floor_slots, (int)balance_slots(B_fit, target));
  for (;;) {
    need = bytes_for(B_fit);
    if (need <= arena_cap || B_fit <= floor_slots) break;
    B_fit = std::max(floor_slots, B_fit - 8);
  }
  return {B_fit, need, 2 * B_fit >= target, need > arena_cap};
}

// ---- the posterior queries (query.h): chunks of a trial list and blocks of columns against stage_bytes of device staging --------------------------
// Trials per chunk of a list of n: the query's *_chunk_trials option when set, else as many as fit stage_bytes at bytes_per_trial of staging
// (0 bytes: the whole list), at least one; never more than cap (0: no cap).
inline int query_chunk(size_t n, int option, size_t bytes_per_trial, size_t cap, size_t stage_bytes) {
  size_t chunk = cap > 0 ? std::min(n, cap) : n;
  if (option > 0) chunk = std::min(chunk, (size_t)option);
  else if (bytes_per_trial > 0) chunk = std::min(chunk, std::max<size_t>(1, stage_bytes / bytes_per_trial));
  return (int)chunk;
}
// Columns (query times, functionals) per block through the root, of padded_width (a multiple of 16): the query's block option rounded up to 16 when set,
// else as many as leave room for eight trials in a chunk at bytes_per_column of staging per trial, a multiple of 16 and at least 16; at most the width.
inline int query_block_cols(int option, int padded_width, size_t bytes_per_column, size_t stage_bytes) {
  if (option > 0) return std::min(padded_width, (option + 15) / 16 * 16);
  const size_t fit = stage_bytes / 8 / bytes_per_column;
  return (int)std::min<size_t>((size_t)padded_width, std::max<size_t>(16, fit / 16 * 16));
}

}  // namespace plan
