// libpgpfa_hip.so - workspace.hip: the chunk workspace - the process-wide arena pool, growth of a context's arena, and the plan that partitions it
// (arithmetic: plan.h).  Host code only: this unit launches no kernel and includes no kernel header.
#include "ctx.h"
#include "plan.h"

using namespace pgpfa;

static plan::Dims plan_dims(const pgpfa_ctx* c) { return {c->ld, c->npad, c->n, c->rpad, c->Tp, c->T, c->p}; }

// engine choice (the rule and its measurements: plan.h)
bool lowrank_pays(const pgpfa_ctx* c) { return plan::lowrank_pays(plan_dims(c)); }
bool want_lowrank(const pgpfa_ctx* c) { return plan::want_lowrank(plan_dims(c), c->cov_mode); }

// allocate a factor workspace: nslots slabs of ld x ld (+ Mt), diagonal inverses, scratch panel
int alloc_cholws(pgpfa_ctx* c, CholWS* w, int nslots, int npad, bool with_mt, size_t slab_elems, bool zero_mt, size_t mt_elems) {
  w->npad = npad;
  w->ld = npad;
  const size_t slab = slab_elems ? slab_elems : (size_t)npad * npad;
  const size_t slab_mt = mt_elems ? mt_elems : slab;
  const size_t slack = (size_t)256 * npad;
  w->sH = slab; w->sM = slab_mt; w->sD = (size_t)npad * NB; w->sP = (size_t)npad * NB;
  CHK(dmalloc(c, &w->H, slab * nslots + slack));
  if (with_mt) CHK(dmalloc(c, &w->Mt, slab_mt * nslots + slack, zero_mt)); else w->Mt = nullptr;
  CHK(dmalloc(c, &w->Dinv, w->sD * nslots + slack));
  CHK(dmalloc(c, &w->P, w->sP * nslots + slack));
  CHK(dmalloc(c, &w->info, nslots, true));
  return 0;
}

// free every workspace allocation (everything allocated after the persistent state)
int free_workspace(pgpfa_ctx* c) {
  if (c->B == 0) return 0;
  HIPC(hipStreamSynchronize(c->st));
  while (c->allocs.size() > c->ws_mark) { hipFree(c->allocs.back()); c->allocs.pop_back(); }
  c->B = 0;
  c->lamd = c->dgrad = c->dpart = c->ldet_buf = c->voff = nullptr;
  c->evid_ld = nullptr;
  c->dual_scr = nullptr;
  c->commbuf = nullptr; c->commbuf_len = 0;
  c->mt_dirty = false;
  return 0;
}

// Grow the arena to at least `need` bytes.  Preferred: map more physical memory behind the reserved address range (the arena does not
// move, the bytes already mapped are not cleared again).  Fallback when the virtual-memory calls are not available: free and
// re-allocate at the size needed.
//
// Arenas of closed contexts stay in a process-wide pool, address range AND mapped memory (round 5).  Two facts of this stack decide that:
// hipMemAddressFree crashed inside the runtime about once in ten runs of a test sequence that opens and closes a few dozen contexts (native
// backtrace: arena_release -> hipMemAddressFree -> libamdhip64; never under a debugger), so ranges were already kept; and memory given back with
// hipMemUnmap + hipMemRelease is NOT returned to the device's free memory while its range lives - tools/leak_probe.py: 308 GB free, a context
// with a 91-GB arena, closed: 217 GB free; the next context's hipMemCreate calls are served from those 91 GB, hipMalloc and hipMemGetInfo never
// see them again.  A plan sized by hipMemGetInfo then shrank with every large context the process had closed before (the config-5 test got 32
// slots per chunk behind the rest of the suite, 128 alone).  Kept mapped, the memory is at least accounted for: the next context starts with
// the pooled arena attached (nothing to map, nothing to clear) and the budget counts it.  When growth fails the other pooled arenas are released.
struct PooledArena { void* va; size_t va_size; std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks; size_t cap; };
std::mutex g_va_mu;
std::vector<PooledArena> g_va_pool;

static void pool_release_chunks(PooledArena& pa) {
  size_t off = 0;
  for (auto& ch : pa.chunks) { hipMemUnmap(reinterpret_cast<char*>(pa.va) + off, ch.second); hipMemRelease(ch.first); off += ch.second; }
  pa.chunks.clear();
  pa.cap = 0;
  (void)hipGetLastError();
}

// bytes of pooled arenas no context holds (device `dev`: ranges are per process, memory per device - contexts of one process on several
// devices are rare enough to ignore the distinction: a range is only re-attached on the device it was mapped for)
static size_t pool_bytes() {
  std::lock_guard<std::mutex> lk(g_va_mu);
  size_t n = 0;
  for (auto& pa : g_va_pool) n += pa.cap;
  return n;
}

// physical memory of the arena: pinned device memory of the context's device
static hipMemAllocationProp arena_mem_prop(const pgpfa_ctx* c) {
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = c->device;
  return prop;
}

// first use of the arena by this context: virtual-memory management available?  reserve a range, or take a pooled one (with its memory)
static void arena_init(pgpfa_ctx* c) {
  if (c->vmm != 0) return;
  const hipMemAllocationProp prop = arena_mem_prop(c);
  size_t gran = 0, free_b = 0, total_b = 0;
  void* va = nullptr;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) == hipSuccess && gran > 0 &&
      hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    const size_t va_size = (total_b + gran - 1) / gran * gran;
    const size_t G = std::max(gran, c->vmm_granule) / gran * gran;
    {
      std::lock_guard<std::mutex> lk(g_va_mu);
      // the pooled arena with the most memory whose chunks have this context's chunk size and device
      int best = -1;
      for (size_t i = 0; c->use_pool && i < g_va_pool.size(); ++i) {
        const PooledArena& pa = g_va_pool[i];
        if (pa.va_size != va_size) continue;
        const bool fits = pa.chunks.empty() || pa.chunks.front().second == G;
        if (fits && (best < 0 || pa.cap > g_va_pool[best].cap)) best = (int)i;
      }
      if (best >= 0) {
        PooledArena pa = std::move(g_va_pool[best]);
        g_va_pool.erase(g_va_pool.begin() + best);
        va = pa.va;
        c->vmm_chunks = std::move(pa.chunks);
        c->arena_cap = pa.cap;
        c->bytes += pa.cap;
      }
    }
    if (va || (hipMemAddressReserve(&va, va_size, gran, nullptr, 0) == hipSuccess && va)) {
      c->arena = reinterpret_cast<char*>(va); c->va_size = va_size; c->vmm_gran = gran; c->vmm = 1;
      c->info["arena_bytes"] = (double)c->arena_cap;
    }
  }
  if (c->vmm != 1) { (void)hipGetLastError(); c->vmm = -1; }
}

// budget_ms > 0: stop mapping once `must` bytes are there and the call has taken that long (returns 0 with arena_cap < need: the caller plans with what
// it has).  Mapping is not a fixed price on this stack: 116 GB in 2 ms in the first process on a box, 4.3 s for the same growth in the next one
// (tools/jump_probe.py, round 6) - pages another process has just given back are cleared before they are handed out again.
int arena_grow(pgpfa_ctx* c, size_t need, double budget_ms, size_t must) {
  g_err.clear();
  arena_init(c);
  const auto t_start = std::chrono::steady_clock::now();
  if (c->vmm == 1) {
    const size_t gran = c->vmm_gran;
    // physical chunks of ONE granule each (one hipMemCreate / hipMemMap / hipMemSetAccess per chunk; 1 GiB by default).  Measured on this
    // stack: hipMemSetAccess returns "invalid argument" for a chunk whose size differs from the first one mapped into the range (13 chunks
    // of 4 GiB, then a 1-GiB remainder: fails; 1 GiB then 4 GiB: fails), so every chunk has the same size.
    const size_t G = std::max(gran, c->vmm_granule) / gran * gran;
    size_t want = need > c->arena_cap ? (need - c->arena_cap + G - 1) / G * G : 0;
    const char* what = "address range exhausted";
    hipError_t err = hipSuccess;
    bool ok = c->arena_cap + want <= c->va_size;
    const hipMemAllocationProp prop = arena_mem_prop(c);
    hipMemAccessDesc desc{};
    desc.location = prop.location;
    desc.flags = hipMemAccessFlagsProtReadWrite;
    bool pool_trimmed = false;
    while (ok && want > 0) {
      const size_t add = std::min(want, std::max(G, gran));
      hipMemGenericAllocationHandle_t h;
      err = hipMemCreate(&h, add, &prop, 0);
      if (err != hipSuccess && !pool_trimmed) {
        // out of memory: the arenas other closed contexts left in the pool give theirs up (the runtime serves later hipMemCreate calls from it)
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(g_va_mu);
        for (auto& pa : g_va_pool) pool_release_chunks(pa);
        pool_trimmed = true;
        continue;
      }
      if (err != hipSuccess) { what = "hipMemCreate"; ok = false; break; }
      err = hipMemMap(c->arena + c->arena_cap, add, 0, h, 0);
      if (err != hipSuccess) { what = "hipMemMap"; hipMemRelease(h); ok = false; break; }
      err = hipMemSetAccess(c->arena + c->arena_cap, add, &desc, 1);
      if (err != hipSuccess) { what = "hipMemSetAccess"; hipMemUnmap(c->arena + c->arena_cap, add); hipMemRelease(h); ok = false; break; }
      c->vmm_chunks.emplace_back(h, add);
      c->arena_cap += add;
      c->bytes += add;
      want -= add;
      if (budget_ms > 0.0 && c->arena_cap >= must &&
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count() > budget_ms) break;
    }
    c->info["arena_bytes"] = (double)c->arena_cap;
    if (ok) return 0;
    (void)hipGetLastError();
    // (the arena only grows between plans, when nothing in it is live: give the range back and carry on with one plain allocation)
    c->info["arena_vmm_failed"] = 1.0;
    std::fprintf(stderr, "pgpfa: workspace arena: %s failed (%s) growing from %zu to %zu bytes; falling back to hipMalloc\n", what,
                 hipGetErrorString(err), c->arena_cap, need);
    c->bytes -= c->arena_cap;
    arena_release(c, true);
    (void)hipGetLastError();
    c->va_size = 0; c->vmm = -1;
  }
  if (c->arena) { hipFree(c->arena); c->bytes -= c->arena_cap; }
  c->arena = nullptr; c->arena_cap = 0;
  if (hipMalloc((void**)&c->arena, need) != hipSuccess) { (void)hipGetLastError(); c->arena = nullptr; return 1; }
  c->arena_cap = need;
  c->bytes += need;
  c->info["arena_bytes"] = (double)c->arena_cap;
  return 0;
}

// (unmap: also release the physical chunks - the fallback path, which is about to try plain allocations; a closing context keeps them mapped
//  in the pool)
void arena_release(pgpfa_ctx* c, bool unmap) {
  if (c->vmm == 1) {
    if (c->arena) {
      PooledArena pa{c->arena, c->va_size, std::move(c->vmm_chunks), c->arena_cap};
      if (unmap) pool_release_chunks(pa);
      std::lock_guard<std::mutex> lk(g_va_mu);
      g_va_pool.push_back(std::move(pa));
    }
    c->vmm_chunks.clear();
  } else if (c->arena) {
    hipFree(c->arena);
  }
  c->arena = nullptr; c->arena_cap = 0;
}

namespace {

// one call of ensure_workspace that makes a new plan
struct WsPlan {
  bool lr;                                       // the low-rank plan (else dense)
  plan::Dims d;
  plan::Slabs base{};                            // the slabs without head-room
  int target = 0;                                // trial-list length planned for
  size_t free_b = 0;                             // free device memory at the start (error texts)
  size_t budget = 0;                             // bytes the slots of a chunk may take
  size_t need = 0;                               // bytes the last measurement gave
  std::chrono::steady_clock::time_point t0{};
};

// accounts the plan's host time on every way out of ensure_workspace, early failures included
struct PlanTimer {
  pgpfa_ctx* c; std::chrono::steady_clock::time_point t0;
  ~PlanTimer() { c->info["plan_ms_total"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); c->info["plans"] += 1.0; }
};

int plan_budget(pgpfa_ctx* c, WsPlan* P) {
  size_t total_b = 0;
  arena_init(c);                                                              // (a pooled arena of a closed context comes with its memory)
  HIPC(hipMemGetInfo(&P->free_b, &total_b));
  // the arena's bytes are ours to re-partition; so are those of pooled arenas nobody holds (arena_grow releases them when it must)
  const size_t avail = (size_t)(0.85 * (double)(P->free_b + c->arena_cap + (c->vmm == 1 ? pool_bytes() : 0)));
  const size_t shared = plan::shared_bytes(P->d);
  P->budget = avail > shared ? avail - shared : 0;
  return 0;
}

// Low-rank plan: the learnt timescales of a fit move, and the ranks with them.  The slabs get head-room for the ranks to grow by
// `arena_headroom` (2: Yt slab x 2, r x r slab x 4) before the plan has to be re-made, when that fits next to the whole
// trial list; a re-plan re-partitions the arena and maps more physical memory into it if it must (only the new bytes cost).
int sizes_and_slots(pgpfa_ctx* c, const WsPlan& P) {
  const plan::Slabs s = P.lr ? plan::headroom_slabs(P.d, P.base, c->arena_headroom, c->arena_cap, P.budget, P.target) : P.base;
  c->slab_elems = s.slab;
  c->mt_elems = s.mt;
  const size_t per = plan::per_slot_bytes(P.d, c->slab_elems, c->mt_elems);
  const plan::Slots slots = plan::slot_count(P.budget / per, c->chunk_opt, P.target);
  c->B_capped = slots.capped;
  if (slots.B < 1) return fail("not enough device memory for one trial slab (%zu bytes needed, %zu free)", per, P.free_b);
  c->B = (int)slots.B;
  return 0;
}

// every allocation of the chunk workspace for c->B slots, through dmalloc in the arena's mode (1 measures, 2 hands out the pointers)
int carve_workspace(pgpfa_ctx* c, bool plan_lr) {
  // (the dense engine needs the strictly lower part of its L^-T slabs zero; the low-rank engine fills its r x r views itself, so under
  // that plan the ~10^11-byte clear is left out and the slabs are marked dirty for a later dense use)
  CHK(alloc_cholws(c, &c->ws, c->B, c->npad, true, c->slab_elems, !plan_lr, c->mt_elems));
  c->ws.nact = round_up(c->n, 64);
  const size_t ld = c->ld, nB = c->B;
  const size_t nBs = nB + 128;                    // slack: multi-RHS GEMM tiles read up to 127 slots past the end
  // all slot vectors: zero-initialised with slack (rows >= n stay zero; GEMM tiles over-read into finite data)
  CHK(dmalloc(c, &c->Xc, ld * nBs, true)); CHK(dmalloc(c, &c->Xt, ld * nBs, true));
  CHK(dmalloc(c, &c->KX, ld * nBs, true)); CHK(dmalloc(c, &c->KD, ld * nBs, true));
  CHK(dmalloc(c, &c->Gl, ld * nBs, true)); CHK(dmalloc(c, &c->Glt, ld * nBs, true));
  CHK(dmalloc(c, &c->Gt, ld * nBs, true)); CHK(dmalloc(c, &c->Dl, ld * nBs, true));
  CHK(dmalloc(c, &c->Rv, ld * nBs, true)); CHK(dmalloc(c, &c->Zv, ld * nBs, true));
  CHK(dmalloc(c, &c->Pv, ld * nBs, true)); CHK(dmalloc(c, &c->Qv, ld * nBs, true));
  CHK(dmalloc(c, &c->Sv, ld * nBs, true)); CHK(dmalloc(c, &c->cg_scal, 4 * nB, true));
  CHK(alloc_cholws(c, &c->sws, 1, c->npad, true));
  c->sws.nact = round_up(c->n, 64);
  CHK(dmalloc(c, &c->sU, ld * ld + 256 * ld, true));
  CHK(dmalloc(c, &c->sDinvT, ld * NB + 256 * ld));
  CHK(dmalloc(c, &c->Wbar, (size_t)c->T * c->p * c->p));
  CHK(dmalloc(c, &c->Gbin, (size_t)c->T * c->p * c->p * nB));
  CHK(dmalloc(c, &c->sc_rz, nB)); CHK(dmalloc(c, &c->sc_pq, nB * (size_t)((c->T + 63) / 64)));
  // per-slot scalars the Newton drivers read back together: one contiguous block, one download
  CHK(dmalloc(c, &c->sc_pack, 7 * nB));
  c->sc_dec = c->sc_pack; c->sc_smax = c->sc_pack + nB; c->sc_qxx = c->sc_pack + 2 * nB; c->sc_qdx = c->sc_pack + 3 * nB;
  c->sc_qdd = c->sc_pack + 4 * nB; c->sc_rr = c->sc_pack + 5 * nB; c->sc_rr0 = c->sc_pack + 6 * nB;
  const size_t wlen = (size_t)c->T * c->p * c->p;
  CHK(dmalloc(c, &c->W, wlen * nB)); CHK(dmalloc(c, &c->Wt, wlen * nB));
  CHK(dmalloc(c, &c->fpart, (size_t)((c->T + 63) / 64) * nB));
  CHK(dmalloc(c, &c->sc_part2, 3 * (size_t)((c->T + 31) / 32) * nB));       // (per (slot, bin tile) partial sums; 32-bin tiles beyond 10 latents)
  // (rows of the component-major form start on 128-byte lines; beyond 10 latents the step's kernels read whole row chunks of the packed triangle at the
  //  template width - up to 210 rows - past a slot's own: one slot's worth of slack behind the last)
  CHK(dmalloc(c, &c->W32, (size_t)round_up(c->T, 32) * (c->p * (c->p + 1) / 2) * nB + (size_t)round_up(c->T, 32) * 210 + 64, true));
  static_assert(sizeof(PcgCtl) <= 64, "the control block is the first 16 words of the solve's upload block");
  CHK(dmalloc(c, &c->pcg_blk, 16 + 4 * nB, true));
  if (c->pcg_blk) {
    c->pcgctl = reinterpret_cast<PcgCtl*>(c->pcg_blk); c->list_a = c->pcg_blk + 16; c->live0 = c->list_a + nB;
    c->pcg_eta = reinterpret_cast<float*>(c->live0 + nB); c->live1 = c->live0 + 2 * nB;
  }
  CHK(dmalloc(c, &c->pcg_ratio, nB, true));
  CHK(dmalloc(c, &c->GbT, (size_t)c->T * (c->p * (c->p + 1) / 2) + 64)); CHK(dmalloc(c, &c->WbT, (size_t)c->T * (c->p * (c->p + 1) / 2) + 64));
  CHK(dmalloc(c, &c->sc_f, nB));
  CHK(dmalloc(c, &c->sc_alpha, nB));
  CHK(dmalloc(c, &c->trial_of_slot, nB)); CHK(dmalloc(c, &c->list_b, nB));
  CHK(dmalloc(c, &c->mask_of_slot, nB));
  CHK(dmalloc(c, &c->ident, nB));
  return 0;
}

// bytes the workspace of `nslots` slots takes (c->B is left at nslots)
int measure(pgpfa_ctx* c, bool plan_lr, int nslots, size_t* bytes) {
  c->B = nslots;
  c->arena_mode = 1; c->arena_off = 0;
  const int rc = carve_workspace(c, plan_lr);
  c->arena_mode = 0;
  *bytes = c->arena_off + ((size_t)1 << 20);
  return rc;
}

// the arena holds less than the plan measures (P->need for c->B slots): grow it, and when the growth stops short fit the chunk into what is there
int grow_and_fit(pgpfa_ctx* c, WsPlan* P) {
  HIPC(hipStreamSynchronize(c->st));
  // (round 6) growth under a time budget (option workspace_grow_budget_ms): whatever it costs the arena gets what `floor_slots` slots need; beyond that
  // mapping stops when the budget is spent and the chunk takes the slots that fit - two chunks of 512 trials cost a few per cent, mapping 100 GB of
  // pages another process has just released costs seconds
  const int B_full = c->B;
  const int floor_slots = std::min(B_full, std::max(8, c->grow_floor_slots));
  size_t must = P->need;
  if (floor_slots < B_full) CHK(measure(c, P->lr, floor_slots, &must));
  const auto t_grow = std::chrono::steady_clock::now();
  const size_t cap_before = c->arena_cap;
  // (not bounded: the first plan of a context - a fit that starts is better off with its whole arena than with a few slow first iterations -
  //  and a plan for a LONGER trial list than the last one: that memory is asked for by the caller, not by ranks that drifted)
  const bool bounded = cap_before > 0 && P->target <= c->plan_target;
  const int rc_grow = arena_grow(c, P->need, bounded ? c->grow_budget_ms : 0.0, must);
  const double grow_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_grow).count();
  c->info["arena_grow_ms_total"] += grow_ms;
  if (std::getenv("PGPFA_PLAN_TRACE"))
    std::fprintf(stderr, "pgpfa: plan %s, %d slots: arena %.1f -> %.1f GB (asked %.1f) in %.0f ms\n", P->lr ? "low-rank" : "dense", B_full, (double)cap_before / 1e9,
                 (double)c->arena_cap / 1e9, (double)P->need / 1e9, grow_ms);
  if (rc_grow) {
    c->B = 0;
    const std::string why = g_err;
    return fail("not enough device memory for the chunk workspace (%zu bytes needed, %zu free)%s%s", P->need, P->free_b, why.empty() ? "" : ": ", why.c_str());
  }
  int B_fit = B_full;
  if (c->arena_cap < P->need) {
    // the budget ran out: the largest balanced chunk that fits what is mapped
    int rc = 0;
    const plan::Fit fit = plan::fit_slots(P->need, must, c->arena_cap, B_full, floor_slots, P->target, [&](int nslots) {
      size_t bytes = 0;
      if (!rc) rc = measure(c, P->lr, nslots, &bytes);
      return bytes;
    });
    CHK(rc);
    P->need = fit.need;
    if (fit.short_of_floor) { c->B = 0; return fail("workspace arena short of its floor (%zu bytes needed, %zu mapped)", P->need, c->arena_cap); }
    c->B_capped = fit.capped;
    B_fit = fit.B;
  }
  c->B = B_fit;
  return 0;
}

}  // namespace

// Workspace plan.  "dense": factor slabs of ld x ld per slot (the general engine, per-trial fallback Newton, post_cov,
// dual variational).  "low-rank": slabs only as large as the r x r systems and their products need, so that ~7x more
// trials fit in one chunk.  Switching plans reallocates the workspace (persistent state is untouched).
int ensure_workspace(pgpfa_ctx* c, bool plan_lr) {
  WsPlan P{plan_lr, plan_dims(c)};
  P.base = plan::base_slabs(P.d, plan_lr);
  // the chunk is sized for the largest trial list seen so far, not for all R resident trials: minibatch EM over a large
  // resident set then keeps one chunk with generous rank head-room instead of re-planning as the ranks grow
  P.target = (c->want_slots > 0) ? std::min(c->want_slots, c->R) : c->R;
  if (c->B > 0 && c->plan_lowrank == plan_lr && P.base.slab <= c->slab_elems && P.base.mt <= c->mt_elems && (c->B >= P.target || c->B_capped)) return 0;
  P.t0 = std::chrono::steady_clock::now();
  PlanTimer plan_timer{c, P.t0};
  CHK(free_workspace(c));
  c->ws_mark = c->allocs.size();
  c->plan_lowrank = plan_lr;
  CHK(plan_budget(c, &P));
  CHK(sizes_and_slots(c, P));
  // pass 1 measures the plan, then the arena is grown if it has to be, pass 2 hands out the pointers
  CHK(measure(c, plan_lr, c->B, &P.need));
  if (P.need > c->arena_cap) CHK(grow_and_fit(c, &P));
  c->arena_mode = 2; c->arena_off = 0;
  const int rc = carve_workspace(c, plan_lr);
  c->arena_mode = 0;
  if (rc) { c->B = 0; return rc; }
  std::vector<int> id(c->B);
  for (int i = 0; i < c->B; ++i) id[i] = i;
  HIPC(hipMemcpyAsync(c->ident, id.data(), sizeof(int) * c->B, hipMemcpyHostToDevice, c->st));
  HIPC(hipStreamSynchronize(c->st));
  if (plan_lr) c->mt_dirty = true;
  c->info["chunk_trials"] = c->B;
  c->info["plan_lowrank"] = c->plan_lowrank ? 1.0 : 0.0;
  c->plan_target = P.target;
  if (std::getenv("PGPFA_PLAN_TRACE"))
    std::fprintf(stderr, "pgpfa: plan %s, %d slots (target %d), slab %zu + %zu elements, %.1f GB carved, %.0f ms\n", plan_lr ? "low-rank" : "dense", c->B, P.target,
                 c->slab_elems, c->mt_elems, (double)P.need / 1e9, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - P.t0).count());
  return 0;
}
