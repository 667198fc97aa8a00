// libpgpfa_hip.so - core.hip (one translation unit of the C-ABI library; shared declarations: ctx.h)
#include "ctx.h"
#include "model.h"
#include "dual.h"
#include "thin.h"
#include "hook.h"
#include "plan.h"

using namespace pgpfa;

static_assert(plan::Dims{}.NB == NB && plan::Dims{}.WIDE_MAX == WIDE_MAX, "plan.h restates two constants of the kernel headers (workspace.hip includes none)");

thread_local std::string g_err;
thread_local unsigned long long g_fail_count = 0;   // failures reported on this thread (queued read-backs of a failed call are void: dl_enqueue / dl_flush)

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  ++g_fail_count;
  return 1;
}

int ensure_hbuf(pgpfa_ctx* c, size_t len) {
  if (len <= c->hbuf_len) return 0;
  if (c->hbuf) hipHostFree(c->hbuf);
  c->hbuf = nullptr;
  HIPC(hipHostMalloc((void**)&c->hbuf, len * sizeof(double)));
  c->hbuf_len = len;
  return 0;
}
int ensure_hibuf(pgpfa_ctx* c, size_t len) {
  if (len <= c->hibuf_len) return 0;
  if (c->hibuf) hipHostFree(c->hibuf);
  c->hibuf = nullptr;
  HIPC(hipHostMalloc((void**)&c->hibuf, len * sizeof(int)));
  c->hibuf_len = len;
  return 0;
}

// ---- profiling (HIP events on the context stream; summed on demand) -------------------------------
// Finished launches are read back (hipEventQuery, no synchronisation) and their events recycled while the run goes on,
// so the number of outstanding events stays bounded however long profiling stays switched on.
void prof_harvest(Prof& P, bool all) {
  while (!P.recs.empty()) {
    Prof::Rec& r = P.recs.front();
    if (!all && hipEventQuery(r.e1) != hipSuccess) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
      P.ms[r.tag] += ms;
      P.flops[r.tag] += r.flops;
      P.count[r.tag] += 1;
      if (ms > P.max_ms[r.tag]) { P.max_ms[r.tag] = ms; P.max_flops[r.tag] = r.flops; }
      if (!r.shape.empty()) { Prof::Shape& sh = P.shapes[r.shape]; sh.ms += ms; sh.flops += r.flops; sh.count += 1; }
    }
    P.idle.push_back(r.e0);
    P.idle.push_back(r.e1);
    P.recs.pop_front();
  }
  (void)hipGetLastError();           // hipEventQuery reports hipErrorNotReady through the sticky error as well
}
hipEvent_t prof_event(Prof& P) {
  if (P.idle.empty()) {
    hipEvent_t e;
    hipEventCreate(&e);
    P.pool.push_back(e);
    return e;
  }
  hipEvent_t e = P.idle.back();
  P.idle.pop_back();
  return e;
}
void prof_begin(pgpfa_ctx* c, int tag, double flops) {
  Prof& P = c->prof;
  if (!P.on || (P.only_tag >= 0 && tag != P.only_tag && tag != TAG_MIX)) return;     // (the one mixing / product-and-mixing launch per E-step rides along)
  if (P.recs.size() >= 256 && (P.recs.size() & 63) == 0) prof_harvest(P, false);
  Prof::Rec r{tag, prof_event(P), prof_event(P), flops, std::string()};
  hipEventRecord(r.e0, c->st);
  P.recs.push_back(r);
  P.open = true;
}
void prof_end(pgpfa_ctx* c) {
  Prof& P = c->prof;
  if (!P.on || !P.open) return;
  hipEventRecord(P.recs.back().e1, c->st);
  P.open = false;
}
void prof_collect(pgpfa_ctx* c) {
  Prof& P = c->prof;
  if (P.recs.empty()) return;
  hipStreamSynchronize(c->st);
  prof_harvest(P, true);
}


int upload_nosync(pgpfa_ctx* c, void* dev, const void* host, size_t bytes);
int upload_list(pgpfa_ctx* c, int* dst, const std::vector<int>& v) {
  if (v.empty()) return 0;
  if (v.size() * sizeof(int) <= (size_t)65536) return upload_nosync(c, dst, v.data(), v.size() * sizeof(int));   // through the pinned ring, no synchronisation
  CHK(ensure_hibuf(c, v.size()));
  // staged through pinned memory; the stream sync in callers orders reuse of the staging buffer
  std::memcpy(c->hibuf, v.data(), v.size() * sizeof(int));
  HIPC(hipMemcpyAsync(dst, c->hibuf, v.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
  HIPC(hipStreamSynchronize(c->st));
  return 0;
}

// Read-backs.  A device-to-host copy into pageable memory makes the runtime drain the stream from the host first and then run a staging
// copy (measured in the kernel trace: 100-280 us of device idle time in front of every such copy); a copy into pinned memory is just
// another stream operation.  Small read-backs therefore land in a pinned staging area and are copied out after ONE synchronisation:
// dl_enqueue queues a copy (several may be queued back to back), dl_flush waits and hands the bytes out.
constexpr size_t DL_STAGE_BYTES = (size_t)4 << 20;
constexpr size_t COPY_KERNEL_MAX = (size_t)256 << 10;        // copies up to this size go through copy_words_kernel when the staging memory is mapped

// dst <- src, bytes a multiple of 4 (every small copy of the library is): one or a few workgroups; either side may be host-mapped memory
__global__ __launch_bounds__(256) void copy_words_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src, size_t nwords) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void copy_vec16_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
// device-to-device copy on the context's stream as a kernel (a runtime copy between two kernels costs hundreds of microseconds of idle time:
// see the note at pgpfa_ctx::copy_kernels); any size, 16-byte vectors when both sides allow
int copy_dev(pgpfa_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  if (c->copy_kernels && (bytes & 3) == 0 && (((size_t)dst | (size_t)src) & 3) == 0) {
    if ((bytes & 15) == 0 && (((size_t)dst | (size_t)src) & 15) == 0) {
      const size_t nv = bytes / 16;
      hipLaunchKernelGGL(copy_vec16_kernel, dim3((unsigned)std::min<size_t>((nv + 255) / 256, 4096)), dim3(256), 0, c->st, reinterpret_cast<uint4*>(dst),
                         reinterpret_cast<const uint4*>(src), nv);
    } else {
      const size_t nw = bytes / 4;
      hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 4096)), dim3(256), 0, c->st, reinterpret_cast<unsigned*>(dst),
                         reinterpret_cast<const unsigned*>(src), nw);
    }
    HIPC(hipGetLastError());
    return 0;
  }
  HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->st));
  return 0;
}
// everything enqueued before this kernel has completed (in-order stream) when the host reads `value` here
__global__ void raise_seq_kernel(volatile unsigned* __restrict__ seq, unsigned value) {
  __threadfence_system();
  *seq = value;
  __threadfence_system();
}

// wait until the stream has drained: by the sequence number in mapped memory when the copies run as kernels, else hipStreamSynchronize
static int stream_drain(pgpfa_ctx* c) {
  if (c->copy_kernels && c->h_seq) {
    const unsigned want = ++c->seq_next;
    hipLaunchKernelGGL(raise_seq_kernel, dim3(1), dim3(1), 0, c->st, (volatile unsigned*)c->d_seq, want);
    if (hipGetLastError() == hipSuccess) {
      const auto t0 = std::chrono::steady_clock::now();
      long spins = 0;
      while (*(volatile unsigned*)c->h_seq != want) {
        if ((++spins & 0xfff) == 0) {
          const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          // a faulted kernel never raises the number: past 50 ms ask the runtime now and then, which also reports the fault
          if (el > 0.05 && hipStreamQuery(c->st) != hipErrorNotReady) break;
        }
      }
      if (*(volatile unsigned*)c->h_seq == want) return 0;
    }
  }
  const hipError_t e_sync = hipStreamSynchronize(c->st);
  if (e_sync != hipSuccess) return fail("%s:%d hipStreamSynchronize -> %s", __FILE__, __LINE__, hipGetErrorString(e_sync));
  return 0;
}
// The queue holds raw host pointers (stack locals, vector buffers, caller arrays) that are only good inside the call that queued them: a
// failure between dl_enqueue and dl_flush - a CHK / HIPC that returned, or the synchronisation below - voids the whole queue, so that no later
// flush copies into memory that call has given back (dl_drop_stale: anything queued before the last fail() of this thread is dropped).
static void dl_drop_stale(pgpfa_ctx* c) {
  if (!c->dl_pending.empty() && c->dl_fail_mark != g_fail_count) { c->dl_pending.clear(); c->dl_used = 0; }
}
int dl_flush(pgpfa_ctx* c) {
  dl_drop_stale(c);
  const int rc_sync = stream_drain(c);
  c->ring_pending = 0;
  if (rc_sync) {
    c->dl_pending.clear();
    c->dl_used = 0;
    return rc_sync;
  }
  for (const auto& e : c->dl_pending) std::memcpy(e.host, c->dl_stage + e.off, e.bytes);
  c->dl_pending.clear();
  c->dl_used = 0;
  return 0;
}
int dl_enqueue(pgpfa_ctx* c, void* host, const void* dev, size_t bytes) {
  if (bytes == 0) return 0;
  if (!c->dl_stage) {
    if (hipHostMalloc((void**)&c->dl_stage, DL_STAGE_BYTES, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); c->dl_stage = nullptr; }
    if (c->dl_stage && hipHostGetDevicePointer((void**)&c->dl_stage_dev, c->dl_stage, 0) != hipSuccess) { (void)hipGetLastError(); c->dl_stage_dev = nullptr; }
    if (!c->h_seq) {
      if (hipHostMalloc((void**)&c->h_seq, 64, hipHostMallocMapped) != hipSuccess ||
          hipHostGetDevicePointer((void**)&c->d_seq, c->h_seq, 0) != hipSuccess) { (void)hipGetLastError(); c->h_seq = nullptr; c->d_seq = nullptr; }
      if (c->h_seq) *c->h_seq = 0u;
    }
  }
  const size_t need = (bytes + 63) / 64 * 64;
  if (!c->dl_stage || need > DL_STAGE_BYTES) {
    // large (or no staging area): straight into the caller's memory; complete when this returns
    CHK(dl_flush(c));
    const hipError_t e_copy = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->st);
    if (e_copy != hipSuccess) return fail("device-to-host copy of %zu bytes: %s", bytes, hipGetErrorString(e_copy));
    return dl_flush(c);
  }
  dl_drop_stale(c);
  if (c->dl_used + need > DL_STAGE_BYTES) CHK(dl_flush(c));
  if (c->copy_kernels && c->dl_stage_dev && c->h_seq && bytes <= COPY_KERNEL_MAX && (bytes & 3) == 0 && (((size_t)dev) & 3) == 0) {
    const size_t nw = bytes / 4;
    hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 64)), dim3(256), 0, c->st,
                       reinterpret_cast<unsigned*>(c->dl_stage_dev + c->dl_used), reinterpret_cast<const unsigned*>(dev), nw);
    HIPC(hipGetLastError());
  } else {
    HIPC(hipMemcpyAsync(c->dl_stage + c->dl_used, dev, bytes, hipMemcpyDeviceToHost, c->st));
  }
  if (c->dl_pending.empty()) c->dl_fail_mark = g_fail_count;
  c->dl_pending.push_back({host, c->dl_used, bytes});
  c->dl_used += need;
  return 0;
}
int download(pgpfa_ctx* c, double* host, const double* dev, size_t n) {
  if (c->hbuf && host >= c->hbuf && host < c->hbuf + c->hbuf_len) {      // already pinned
    // (small: through the staging area like any other read-back - the runtime's copy costs more than the extra memcpy)
    if (c->copy_kernels && n * sizeof(double) <= COPY_KERNEL_MAX) {
      CHK(dl_enqueue(c, host, dev, n * sizeof(double)));
      return dl_flush(c);
    }
    HIPC(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->st));
    return dl_flush(c);
  }
  CHK(dl_enqueue(c, host, dev, n * sizeof(double)));
  return dl_flush(c);
}
int upload(pgpfa_ctx* c, double* dev, const double* host, size_t n) {
  // (small: through the pinned ring - the bytes are out of the caller's buffer when this returns, and nothing waits for the device)
  if (n * sizeof(double) <= (size_t)65536) return upload_nosync(c, dev, host, n * sizeof(double));
  HIPC(hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPC(hipStreamSynchronize(c->st));
  c->ring_pending = 0;
  return 0;
}
// Small upload without a synchronisation: the bytes are copied into the next slot of a ring of pinned buffers and sent asynchronously; a
// slot comes round again after RING_N uploads, and every download / synchronising upload in between (there is at least one per Newton
// outer iteration and per line-search round) has drained the stream by then - enforced by the pending count.
constexpr int RING_N = 16;
int upload_nosync(pgpfa_ctx* c, void* dev, const void* host, size_t bytes) {
  if (bytes == 0) return 0;
  if (bytes > c->ring_slot) {
    HIPC(hipStreamSynchronize(c->st));
    if (c->ring) hipHostFree(c->ring);
    c->ring = nullptr; c->ring_dev = nullptr;
    const size_t slot = (bytes + 4095) / 4096 * 4096;
    HIPC(hipHostMalloc((void**)&c->ring, slot * RING_N, hipHostMallocMapped));
    if (hipHostGetDevicePointer((void**)&c->ring_dev, c->ring, 0) != hipSuccess) { (void)hipGetLastError(); c->ring_dev = nullptr; }
    c->ring_slot = slot; c->ring_cur = 0; c->ring_pending = 0;
  }
  if (c->ring_pending >= RING_N - 1) { HIPC(hipStreamSynchronize(c->st)); c->ring_pending = 0; }
  char* slot = c->ring + (size_t)c->ring_cur * c->ring_slot;
  std::memcpy(slot, host, bytes);
  if (c->copy_kernels && c->ring_dev && bytes <= COPY_KERNEL_MAX && (bytes & 3) == 0 && (((size_t)dev) & 3) == 0) {
    const size_t nw = bytes / 4;
    hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 64)), dim3(256), 0, c->st, reinterpret_cast<unsigned*>(dev),
                       reinterpret_cast<const unsigned*>(c->ring_dev + (size_t)c->ring_cur * c->ring_slot), nw);
    HIPC(hipGetLastError());
  } else {
    HIPC(hipMemcpyAsync(dev, slot, bytes, hipMemcpyHostToDevice, c->st));
  }
  c->ring_cur = (c->ring_cur + 1) % RING_N;
  c->ring_pending += 1;
  return 0;
}


// Kinv (and logdet) of the p Gram slabs currently in Kpad, through the production factor kernels
int build_kinv(pgpfa_ctx* c) {
  c->kinv_serial += 1;
  const size_t slab = (size_t)c->Tp * c->Tp;
  CHK(copy_dev(c, c->kws.H, c->Kpad, slab * c->p * sizeof(double)));
  HIPC(hipMemsetAsync(c->kws.info, 0, sizeof(int) * c->p, c->st));
  CHK(factor(c, c->kws, nullptr, c->p));
  c->logdetK.assign(c->p, 0.0);
  hipLaunchKernelGGL(logdet_batch_kernel, dim3(c->p), dim3(256), 0, c->st, c->kws.H, (long long)c->kws.sH, c->Tp, c->Tp, c->tscal);
  CHK(download(c, c->logdetK.data(), c->tscal, c->p));
  CHK(inverse_t(c, c->kws, nullptr, c->p));
  GemmP g{};
  g.A = c->kws.Mt; g.sA = c->kws.sM; g.lda = c->Tp;
  g.B = c->kws.Mt; g.sB = c->kws.sM; g.ldb = c->Tp;
  g.C = c->Kinv; g.sC = slab; g.ldc = c->Tp;
  g.M = c->Tp; g.N = c->Tp; g.K = c->Tp; g.alpha = 1.0; g.beta = 0.0;
  g.slots = nullptr; g.nbatch = c->p; g.mode = GEMM_FULL; g.kflags = KF_BEGIN_MAXRC;
  CHK(gemm(c, false, g));
  std::vector<int> info(c->p);
  CHK(dl_enqueue(c, info.data(), c->kws.info, sizeof(int) * c->p));
  CHK(dl_flush(c));
  for (int k = 0; k < c->p; ++k)
    if (info[k] != 0) return fail("GP Gram matrix of latent %d is not positive definite (pivot %d)", k, info[k]);
  return 0;
}


// pivoted-Cholesky factors of the RBF part of every Gram matrix and the block tables of the r x r system
// (the pivoted Cholesky itself - p workgroups, a chain of r_k dependent steps each: 1-2 ms with the chip empty - on stream `st`)
// (the three-way choice from explicit arguments: launch_pivchol passes the context's, pgpfa_test_pivchol buffers of its own; lds, optional: the
//  dynamic LDS the form asks for - with run = false nothing is launched, only the form and its LDS are told)
int pivchol_launch(double* F, int Tf, int T, int p, const double* tau, double bin, double eps, double tol, bool pairs, int* rank, hipStream_t st, size_t* lds,
                   bool run) {
  const int rmax = std::min(T, Tf);
  const size_t shm = ((size_t)2 * T + rmax + 16) * sizeof(double) + 16 * sizeof(int);
  const int form = (T > 256 && pairs && Tf % 2 == 0) ? PIVCHOL_PAIRS : T > 256 ? PIVCHOL_512_2 : PIVCHOL_256_1;
  if (lds) *lds = form == PIVCHOL_PAIRS ? pivchol2_lds(T, rmax, 1024, 4) : shm;
  if (!run) return form;
  if (form == PIVCHOL_PAIRS)
    hipLaunchKernelGGL((rbf_pivchol2_kernel<256, 4>), dim3(p), dim3(1024), pivchol2_lds(T, rmax, 1024, 4), st, F, Tf, T, tau, bin, eps, tol, rmax, rank);
  else if (form == PIVCHOL_512_2)
    hipLaunchKernelGGL((rbf_pivchol_kernel<512, 2>), dim3(p), dim3(1024), shm, st, F, Tf, T, tau, bin, eps, tol, rmax, rank);
  else
    hipLaunchKernelGGL((rbf_pivchol_kernel<256, 1>), dim3(p), dim3(256), shm, st, F, Tf, T, tau, bin, eps, tol, rmax, rank);
  return form;
}

int launch_pivchol(pgpfa_ctx* c, hipStream_t st) {
  (void)pivchol_launch(c->Flr, c->Tp, c->T, c->p, c->tau, c->bin, c->eps, c->lr_tol, c->pivchol_pairs != 0, c->d_rank, st);
  HIPC(hipGetLastError());
  return 0;
}

// Work tables of thin.h's kernels from the rank tables (rr: rank rows a latent owns, rk = round_up(rr, 16): the size its products are issued with,
// roff: where its rows start, rtot = roff[p]).
ThinTables thin_tables(int p, int T, const int* rr, const int* rk, const int* roff, int rtot) {
  ThinTables tt;
  std::vector<int>&hft = tt.ft, &hf = tt.f, &hs = tt.s;
  for (int k = 0; k < p; ++k) {
    // (row groups of a latent of equal size up to one 4-row run, multiples of 4 up to 64: 80 rank rows are 40 + 40, not 64 + 16, and 136 are
    //  48 + 44 + 44, not 48 + 48 + 40 - the remainder is dealt out in runs of 4 to the first groups; rr is a multiple of 4)
    // (rr, not rk: these rows are WRITTEN - past the latent's own they are the next latent's)
    const int ngr = (rr[k] + 63) / 64, runs = rr[k] / 4;
    for (int g = 0, m0 = 0; g < ngr; ++g) {
      const int rows = 4 * (runs / ngr + (g < runs % ngr ? 1 : 0));
      hft.push_back(k); hft.push_back(m0); hft.push_back(rows); hft.push_back(roff[k]);
      m0 += rows;
    }
    for (int t0 = 0; t0 < T; t0 += 256) { hf.push_back(k); hf.push_back(t0); hf.push_back(rk[k]); hf.push_back(roff[k]); }
  }
  // Sb u with the same kernel as F^T t: one "latent" of rtot rows and rtot "bins", 64 rows per workgroup
  for (int m0 = 0; m0 < rtot; m0 += 64) { hs.push_back(0); hs.push_back(m0); hs.push_back(std::min(64, rtot - m0)); hs.push_back(0); }
  return tt;
}

// The rank tables of the r x r system (ctx.h; build_lowrank describes the rule and stores what this returns).
RankLayout rank_layout(int p, const int* ranks, int gran, bool thin_all) {
  RankLayout L;
  const int G = ((gran == 4 || gran == 8) && thin_all) ? gran : 16;
  L.rk.assign(p, 0);
  L.roff.assign(p + 1, 0);
  L.rr.assign(p, 0);
  L.roff16.assign(p + 1, 0);
  int extent = 0;
  for (int k = 0; k < p; ++k) {
    L.rr[k] = round_up(std::max(ranks[k], 1), G);
    L.rk[k] = round_up(L.rr[k], 16);
    L.roff[k + 1] = L.roff[k] + L.rr[k];
    L.roff16[k + 1] = L.roff16[k] + L.rk[k];
    extent = std::max(extent, L.roff[k] + L.rk[k]);
  }
  L.rtot = L.roff[p];
  L.rtot16 = L.roff16[p];
  L.rank_compact = (G != 16);
  L.rpad = round_up(std::max(L.rtot, extent), NB);
  const int nblk = round_up(L.rtot16, NB) / 16;
  L.blk_lat.assign(nblk, -1);
  L.blk_col.assign(nblk, 0);
  for (int k = 0; k < p; ++k)
    for (int b = L.roff16[k] / 16; b < L.roff16[k + 1] / 16; ++b) { L.blk_lat[b] = k; L.blk_col[b] = b * 16 - L.roff16[k]; }
  if (L.rank_compact) {
    // padded index -> compact index (-1: a padding row); nrtab[b]: padded rows that can hold something in the 16-column block b of L^-T (it is upper
    // triangular in the compact order: rows up to compact index 16 b + 15), rounded up to a whole 16-row group of the latent that holds the last one
    const int n16 = round_up(L.rtot16, NB);
    std::vector<int> pmap(round_up(L.rtot, 16) + 16, 0);
    L.cmap.assign(n16, -1);
    for (int k = 0; k < p; ++k)
      for (int j = 0; j < L.rr[k]; ++j) { L.cmap[L.roff16[k] + j] = L.roff[k] + j; pmap[L.roff[k] + j] = L.roff16[k] + j; }
    L.nrtab.assign((round_up(L.rtot, 16)) / 16, 0);
    for (size_t b = 0; b < L.nrtab.size(); ++b) {
      const int last = std::min((int)b * 16 + 15, L.rtot - 1);
      L.nrtab[b] = std::min(L.rtot16, round_up(pmap[last] + 1, 16));
    }
    // The DMA form of yt_mix's panel staging (ytmix.h) moves whole row PAIRS, 16 bytes from a 16-byte aligned address: a pair is padding as a
    // whole or two consecutive slab rows from an even one (real rows come in multiples of 4 from a multiple of 4).
    for (int i = 0; i + 1 < n16 && L.bad_pair < 0; i += 2)
      if (L.cmap[i] < 0 ? L.cmap[i + 1] >= 0 : ((L.cmap[i] & 1) != 0 || L.cmap[i + 1] != L.cmap[i] + 1)) L.bad_pair = i;
  }
  return L;
}

// (pivchol_launched: the kernel is already running on the side stream and c->ev_join marks its end)
int build_lowrank(pgpfa_ctx* c, bool pivchol_launched) {
  const int p = c->p, T = c->T, Tp = c->Tp;
  if (pivchol_launched) HIPC(hipStreamWaitEvent(c->st, c->ev_join, 0));
  else CHK(launch_pivchol(c, c->st));
  std::vector<int> r(p);
  CHK(dl_enqueue(c, r.data(), c->d_rank, sizeof(int) * p));
  CHK(dl_flush(c));
  // Rank tables.  rk[k]: the latent's rank rounded up to 16 - the size every product with F_k is issued with (columns of F_k past the rank are zero:
  // the pivoted Cholesky clears its slab first).  roff[k]: where the latent's rows / columns START in the r x r system and in L^-T.
  // rank_gran = 16 (rounds 1-5): roff[k + 1] = roff[k] + rk[k] - every latent owns whole 16-blocks, 7.5 % (late) to 18 % (early iterations of the
  // bench) of the rank total is padding, identity rows that the r x r factorisation, its inverse, the columns of Yt and of the split sums pay for.
  // rank_gran = 4 (round 6): COMPACT offsets roff[k + 1] = roff[k] + round_up(rank, 4).  A product with F_k still takes rk[k] rows from roff[k]
  // on - the last few belong to the next latent and meet zero columns of F_k - so only two kernels need to know: B = I + F^T Wt F is still
  // computed on 16-blocks that never straddle a latent (assemble_b, in the PADDED index space roff16 / blk_lat / blk_col) and stored at its
  // compact place (cmap), and the panel of L^-T that yt_mix stages keeps padded rows (gathered through the same map).
  // (compact offsets need the preconditioner's three products as thin.h's kernels: the general GEMM's row-tile tables start tiles on multiples of 16)
  const bool thin_all = thin_possible(c) && c->thin_products >= 2;
  RankLayout rl = rank_layout(p, r.data(), c->rank_gran, thin_all);
  c->rk = rl.rk;
  c->roff = rl.roff;
  c->rr = rl.rr;
  c->roff16 = rl.roff16;
  c->rtot = rl.rtot;
  c->rtot16 = rl.rtot16;
  c->rank_compact = rl.rank_compact;
  c->rpad = rl.rpad;
  CHK(upload_list(c, c->d_blk_lat, rl.blk_lat));
  CHK(upload_list(c, c->d_blk_col, rl.blk_col));
  CHK(upload_list(c, c->d_roff, c->roff));
  CHK(upload_list(c, c->d_roff16, c->roff16));
  if (c->rank_compact) {
    // A table that breaks the row-pair rule of the panel staging (rank_layout) is an error.
    if (rl.bad_pair >= 0) {
      const int i = rl.bad_pair;
      return fail("rank tables: padded rows %d, %d map to slab rows %d, %d - not a pair the panel staging can move whole", i, i + 1, rl.cmap[i], rl.cmap[i + 1]);
    }
    CHK(upload_list(c, c->d_cmap, rl.cmap));
    CHK(upload_list(c, c->d_nrtab, rl.nrtab));
  }
  {
    // Row-tile tables of the two block-diagonal products of the low-rank preconditioner, 64 rows per tile, one latent per tile:
    // F^T (rpad x n): rank rows [roff[k], roff[k+1]) x the latent's bins [kT, (k+1)T) (rounded out to multiples of 16: the
    //   neighbours' columns in these rows are zero);  F (n x rpad): rows [kT, (k+1)T) x the latent's rank columns.
    std::vector<int> tft, tf;
    c->kr_ft_len = 0; c->kr_f_len = 0;
    for (int k = 0; k < p; ++k) {
      const int kb = (k * T) / 16 * 16, ke = std::min(c->npad, round_up((k + 1) * T, 16));
      for (int r0 = c->roff[k]; r0 < c->roff[k + 1]; r0 += 64) { tft.push_back(r0); tft.push_back(c->roff[k + 1]); tft.push_back(kb); tft.push_back(ke); }
      c->kr_ft_len = std::max(c->kr_ft_len, ke - kb);
      for (int i0 = k * T; i0 < (k + 1) * T; i0 += 64) { tf.push_back(i0); tf.push_back((k + 1) * T); tf.push_back(c->roff[k]); tf.push_back(c->roff[k + 1]); }
      c->kr_f_len = std::max(c->kr_f_len, c->rk[k]);
    }
    c->ntab_ft = (int)tft.size() / 4; c->ntab_f = (int)tf.size() / 4;
    if (tft.size() > c->tab_cap || tf.size() > c->tab_cap) return fail("internal: row-tile table overflow");
    CHK(upload_list(c, c->d_kr_ft, tft));
    CHK(upload_list(c, c->d_kr_f, tf));
    // thin.h: F^T t by (latent, 64 rank rows), F v by (latent, 256 bins), Sb u by 64 rows
    const ThinTables tt = thin_tables(p, T, c->rr.data(), c->rk.data(), c->roff.data(), c->rtot);
    const std::vector<int>&hft = tt.ft, &hf = tt.f, &hs = tt.s;
    c->nthin_s = (int)hs.size() / 4;
    if (hs.size() > c->tab_cap) return fail("internal: thin-product table overflow");
    CHK(upload_list(c, c->d_thin_s, hs));
    c->nthin_ft = (int)hft.size() / 4; c->nthin_f = (int)hf.size() / 4;
    if (hft.size() > c->tab_cap || hf.size() > c->tab_cap) return fail("internal: thin-product table overflow");
    CHK(upload_list(c, c->d_thin_ft, hft));
    CHK(upload_list(c, c->d_thin_f, hf));
  }
  if ((size_t)c->rpad <= (size_t)c->ld) {
    HIPC(hipMemsetAsync(c->Fbig, 0, (size_t)c->ld * c->rpad * sizeof(double), c->st));
    HIPC(hipMemsetAsync(c->FTbig, 0, (size_t)c->rpad * c->ld * sizeof(double), c->st));
    int rkmax = 0;
    for (int k = 0; k < p; ++k) rkmax = std::max(rkmax, c->rk[k]);
    hipLaunchKernelGGL(build_fbig_kernel, dim3(rkmax, p), dim3(128), 0, c->st, c->Flr, Tp, T, c->d_roff, c->Fbig, c->ld, c->FTbig, c->rpad);
    HIPC(hipGetLastError());
  }
  c->info["lowrank_rtot"] = c->rtot;
  c->info["lowrank_rtot16"] = c->rtot16;
  c->info["lowrank_compact"] = c->rank_compact ? 1.0 : 0.0;
  c->flr32_valid = false;
  return 0;
}

// what the kernels that know the compact offsets are told of the tables above (ctx.h)
BLayout b_layout_of(bool compact, int rtot16, int rpad, const int* cmap, const int* roff_padded, const int* nrtab) {
  const int n64 = round_up(rtot16, 64) / 64, d64 = rpad / 64;
  return compact ? BLayout{n64, n64 * (n64 + 1) / 2, cmap, roff_padded, nrtab, round_up(rtot16, (int)NB)}
                 : BLayout{d64, d64 * (d64 + 1) / 2, nullptr, roff_padded, nullptr, 0};
}
BLayout b_layout(const pgpfa_ctx* c) {
  return b_layout_of(c->rank_compact, c->rtot16, c->rpad, c->d_cmap, c->rank_compact ? c->d_roff16 : c->d_roff, c->d_nrtab);
}

// ---- test hook: the three thin products of the low-rank preconditioner on caller data, through thin_tables and the launches of shared_solve ---------
namespace {
int thin_refuse(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  (void)fail("pgpfa_test_thin refuses: %s", buf);
  return code;
}
}  // namespace

int pgpfa_test_thin(pgpfa_ctx* c, int kind, int p, int T, int Tf, const int32_t* ranks, int gran, long long ldx, long long ldy, int Tx, int vec_f32, int nslots,
                    int ncols, const int32_t* cols, int live, int stop, double fill, const double* F, const double* Sb, const void* X, void* Y, int32_t* geom,
                    int tab_cap, int32_t* tab_ft, int32_t* tab_f, int32_t* tab_s, int32_t* ntab) {
  using namespace hook;
  if (!c || !ranks || !X || !Y || !geom || !tab_ft || !tab_f || !tab_s || !ntab) return thin_refuse(PGPFA_THIN_BAD_ARG, "null argument");
  if (kind < PGPFA_THIN_FT || kind > PGPFA_THIN_APPLY) return thin_refuse(PGPFA_THIN_BAD_ARG, "kind %d", kind);
  const bool use_f = kind != PGPFA_THIN_S, use_s = kind == PGPFA_THIN_S || kind == PGPFA_THIN_APPLY;
  if ((use_f && !F) || (use_s && !Sb)) return thin_refuse(PGPFA_THIN_BAD_ARG, "null argument");
  if (p < 1 || nslots < 1 || ncols < 1 || tab_cap < 4) return thin_refuse(PGPFA_THIN_BAD_ARG, "invalid sizes");
  if (gran != 4 && gran != 8 && gran != 16) return thin_refuse(PGPFA_THIN_BAD_ARG, "rank granularity %d (4, 8 or 16)", gran);
  if (vec_f32 && kind == PGPFA_THIN_S) return thin_refuse(PGPFA_THIN_BAD_ARG, "Sb u has no single-precision vectors");
  if (T < 4) return thin_refuse(PGPFA_THIN_REFUSED_T, "T = %d below 4 (the 4-bin runs of the vector loads are clamped to T - 4)", T);
  if (Tf < T || Tf % 4 != 0) return thin_refuse(PGPFA_THIN_BAD_ARG, "slab size Tf = %d below T = %d or no multiple of 4", Tf, T);
  // rank tables by the rule of build_lowrank
  std::vector<int> rr(p), rk(p), roff(p + 1, 0);
  int extent = 0;
  for (int k = 0; k < p; ++k) {
    if (ranks[k] < 1 || ranks[k] % 4 != 0) return thin_refuse(PGPFA_THIN_REFUSED_RANK, "rank %d of latent %d is no positive multiple of 4", ranks[k], k);
    rr[k] = round_up(std::max(ranks[k], 1), gran);
    rk[k] = round_up(rr[k], 16);
    if (rk[k] > Tf) return thin_refuse(PGPFA_THIN_REFUSED_RANK, "latent %d: %d rank columns do not fit a slab of %d", k, rk[k], Tf);
    roff[k + 1] = roff[k] + rr[k];
    extent = std::max(extent, roff[k] + rk[k]);
  }
  const int rtot = roff[p];
  if (rtot % 4 != 0) return thin_refuse(PGPFA_THIN_REFUSED_RANK, "rank total %d is no multiple of 4", rtot);
  const int rpad = round_up(std::max(rtot, extent), NB);
  const bool vec4 = T % 4 == 0;
  if (use_f) {
    if (Tx < T) return thin_refuse(PGPFA_THIN_REFUSED_TX, "latent stride Tx = %d below T = %d", Tx, T);
    if (vec4 && Tx % 4 != 0) return thin_refuse(PGPFA_THIN_REFUSED_TX, "latent stride Tx = %d is no multiple of 4 where T is one (vector loads)", Tx);
  } else {
    Tx = T;
  }
  // leading dimensions: an n-vector holds (p - 1) Tx + T rows, a rank-space vector rtot written rows inside rpad
  const long long nrows = (long long)(p - 1) * Tx + T;
  const long long need_x = kind == PGPFA_THIN_FT || kind == PGPFA_THIN_APPLY ? nrows : rtot;
  const long long need_y = kind == PGPFA_THIN_F || kind == PGPFA_THIN_APPLY ? nrows : rtot;
  if (ldx < need_x || ldy < need_y) return thin_refuse(PGPFA_THIN_REFUSED_LD, "ldx = %lld, ldy = %lld below the rows read / written (%lld, %lld)", ldx, ldy, need_x, need_y);
  if (ldx % 4 != 0 || ldy % 4 != 0) return thin_refuse(PGPFA_THIN_REFUSED_LD, "ldx = %lld, ldy = %lld: no multiples of 4 (vector loads and stores)", ldx, ldy);
  if (ldx > (1ll << 24) || ldy > (1ll << 24)) return thin_refuse(PGPFA_THIN_REFUSED_LD, "leading dimension too large for a test");
  const long long ldr = std::max(ldx, ldy);          // apply: leading dimension of the two rank-space intermediates
  const long long ld_rank = kind == PGPFA_THIN_FT ? ldy : kind == PGPFA_THIN_F ? ldx : kind == PGPFA_THIN_S ? std::min(ldx, ldy) : ldr;
  if (rpad > ld_rank) return thin_refuse(PGPFA_THIN_REFUSED_RPAD, "rpad = %d above the leading dimension %lld of the rank-space vectors", rpad, ld_rank);
  if (cols) {
    std::vector<char> seen(nslots, 0);
    for (int i = 0; i < ncols; ++i) {
      if (cols[i] < 0 || cols[i] >= nslots) return thin_refuse(PGPFA_THIN_REFUSED_COLS, "column list entry %d = %d outside the %d slots", i, cols[i], nslots);
      if (seen[cols[i]]) return thin_refuse(PGPFA_THIN_REFUSED_COLS, "column list names slot %d twice", cols[i]);
      seen[cols[i]] = 1;
    }
  } else if (ncols > nslots) {
    return thin_refuse(PGPFA_THIN_REFUSED_COLS, "%d columns of %d slots", ncols, nslots);
  }
  if (live < -1 || live > ncols) return thin_refuse(PGPFA_THIN_REFUSED_LIVE, "live count %d outside 0..%d", live, ncols);
  if (!c->mfma) return fail("the thin products run on the matrix cores (use_mfma = 1)");
  const ThinTables tt = thin_tables(p, T, rr.data(), rk.data(), roff.data(), rtot);
  if ((int)tt.ft.size() > tab_cap || (int)tt.f.size() > tab_cap || (int)tt.s.size() > tab_cap) return thin_refuse(PGPFA_THIN_BAD_ARG, "tables exceed tab_cap = %d", tab_cap);
  for (int k = 0; k < p; ++k) { geom[k] = rr[k]; geom[p + k] = rk[k]; }
  for (int k = 0; k <= p; ++k) geom[2 * p + k] = roff[k];
  geom[3 * p + 1] = rtot; geom[3 * p + 2] = rpad;
  std::copy(tt.ft.begin(), tt.ft.end(), tab_ft); std::copy(tt.f.begin(), tt.f.end(), tab_f); std::copy(tt.s.begin(), tt.s.end(), tab_s);
  ntab[0] = (int)tt.ft.size() / 4; ntab[1] = (int)tt.f.size() / 4; ntab[2] = (int)tt.s.size() / 4;

  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->st));
  HookBuffers hb;
  // Inputs: the caller's array with SLACK more elements behind it, holding `fill`.  The kernels read whole 64-row tiles: up to 63 rows past the last
  // group of FT and past bin T of the last slab column - values that are never stored.
  constexpr size_t SLACK = 128;
  auto filled = [&](double** dev, size_t count) -> int {
    CHK(hb.get(dev, count + SLACK, 0));
    const std::vector<double> h(count + SLACK, fill);
    HIPC(hipMemcpy(*dev, h.data(), (count + SLACK) * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  };
  auto input = [&](double** dev, const double* host, size_t count) -> int {
    CHK(filled(dev, count));
    HIPC(hipMemcpy(*dev, host, count * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  };
  auto ints = [&](int** dev, const int* host, size_t count) -> int {
    CHK(hb.get(dev, count, 0));
    HIPC(hipMemcpy(*dev, host, count * sizeof(int), hipMemcpyHostToDevice));
    return 0;
  };
  double *dF = nullptr, *dFT = nullptr, *dFbig = nullptr, *dSb = nullptr, *dX = nullptr;
  int *d_ft = nullptr, *d_f = nullptr, *d_s = nullptr, *d_roff = nullptr, *d_cols = nullptr, *d_live = nullptr, *d_stop = nullptr;
  CHK(ints(&d_ft, tt.ft.data(), tt.ft.size()));
  CHK(ints(&d_f, tt.f.data(), tt.f.size()));
  CHK(ints(&d_s, tt.s.data(), tt.s.size()));
  CHK(ints(&d_roff, roff.data(), roff.size()));
  if (cols) CHK(ints(&d_cols, cols, ncols));
  if (live >= 0) CHK(ints(&d_live, &live, 1));
  if (stop >= 0) CHK(ints(&d_stop, &stop, 1));
  const bool x_f32 = vec_f32 && (kind == PGPFA_THIN_FT || kind == PGPFA_THIN_APPLY), y_f32 = vec_f32 && (kind == PGPFA_THIN_F || kind == PGPFA_THIN_APPLY);
  {
    // (floats: ldx is a multiple of 4, two to a double)
    const size_t xd = x_f32 ? (size_t)nslots * ldx / 2 : (size_t)nslots * ldx;
    CHK(input(&dX, static_cast<const double*>(X), xd));
  }
  if (use_f) {
    // slabs, and FT built from them as build_lowrank does - over `fill` where production has zeros: outside the blocks
    CHK(input(&dF, F, (size_t)p * Tf * Tf));
    CHK(filled(&dFT, (size_t)p * T * rpad));
    CHK(hb.get(&dFbig, (size_t)rtot * p * T, 0));
    int rkmax = 0;
    for (int k = 0; k < p; ++k) rkmax = std::max(rkmax, rk[k]);
    HIPC(hipDeviceSynchronize());
    hipLaunchKernelGGL(build_fbig_kernel, dim3(rkmax, p), dim3(128), 0, c->st, dF, Tf, T, d_roff, dFbig, p * T, dFT, rpad);
    HIPC(hipGetLastError());
  }
  if (use_s) CHK(input(&dSb, Sb, (size_t)rpad * rpad));
  void* dY = nullptr;
  const size_t ybytes = (size_t)nslots * ldy * (y_f32 ? sizeof(float) : sizeof(double));
  CHK(hook_output_bytes(hb, &dY, Y, ybytes));
  double *dU = nullptr, *dV = nullptr;
  const size_t mid = (size_t)nslots * ldr;
  if (kind == PGPFA_THIN_APPLY) {
    // the intermediates F^T t and Sb F^T t: `fill` everywhere (rows [rtot, rpad) "may hold anything"), a band behind each
    const std::vector<double> h(mid, fill);
    CHK(hook_output(hb, &dU, h.data(), mid));
    CHK(hook_output(hb, &dV, h.data(), mid));
  }
  HIPC(hipDeviceSynchronize());
  ThinP tp{};
  tp.F = dF; tp.Tf = Tf; tp.T = T; tp.Tx = Tx; tp.FT = dFT; tp.ldft = rpad;
  tp.cols = d_cols; tp.n_dev = d_live; tp.ncols = ncols; tp.skip = d_stop;
  auto run_ft = [&](const double* x, long long lx, double* y, long long ly) {
    tp.tab = d_ft; tp.X = x; tp.ldx = lx; tp.Y = y; tp.ldy = ly;
    thin_launch_ft(tp, ntab[0], ncols, x_f32, c->st);
  };
  auto run_s = [&](const double* x, long long lx, double* y, long long ly) {
    ThinP ts = tp;
    ts.FT = dSb; ts.ldft = rpad; ts.T = rtot; ts.tab = d_s; ts.X = x; ts.ldx = lx; ts.Y = y; ts.ldy = ly;
    thin_launch_s(ts, ntab[2], ncols, c->st);
  };
  auto run_f = [&](const double* x, long long lx, double* y, long long ly) {
    tp.tab = d_f; tp.X = x; tp.ldx = lx; tp.Y = y; tp.ldy = ly;
    thin_launch_f(tp, ntab[1], ncols, y_f32, c->st);
  };
  double* y = static_cast<double*>(dY);
  if (kind == PGPFA_THIN_FT) run_ft(dX, ldx, y, ldy);
  else if (kind == PGPFA_THIN_S) run_s(dX, ldx, y, ldy);
  else if (kind == PGPFA_THIN_F) run_f(dX, ldx, y, ldy);
  else { run_ft(dX, ldx, dU, ldr); run_s(dU, ldr, dV, ldr); run_f(dV, ldr, y, ldy); }
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->st));
  if (kind == PGPFA_THIN_APPLY) {
    CHK(hook_collect("pgpfa_test_thin (F^T t)", dU, nullptr, mid));
    CHK(hook_collect("pgpfa_test_thin (Sb u)", dV, nullptr, mid));
  }
  return hook_collect_bytes("pgpfa_test_thin", dY, Y, ybytes);
}

// ---- test hook: the pivoted Cholesky of the RBF part on caller timescales, through pivchol_launch ----------------------------------------------------
// The kernels read nothing but tau[p] and their own slab; they write all Tf x Tf entries of each slab (zeros first), column j < min(T, Tf) rows t < T -
// the pair form with 16-byte loads and stores of rows (t, t + 1), t even, t + 1 <= round_up(T, 2) - 1 < Tf for an even Tf >= T - and rank[p].
// Dynamic LDS: what pivchol_launch asks for, refused above the 64 KiB a launch may ask for without opting in (production does not opt in).
namespace {
int pivchol_refuse(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  (void)fail("pgpfa_test_pivchol refuses: %s", buf);
  return code;
}
}  // namespace

int pgpfa_test_pivchol(pgpfa_ctx* c, int p, int T, int Tf, const double* tau, double bin, double eps, double tol, int pairs, double fill, double* F,
                       int32_t* rank, int32_t* form) {
  using namespace hook;
  if (!c || !tau || !F || !rank || !form) return pivchol_refuse(PGPFA_PIVCHOL_BAD_ARG, "null argument");
  if (p < 1 || p > 32 || Tf > 4096 || !(bin > 0.0)) return pivchol_refuse(PGPFA_PIVCHOL_BAD_ARG, "invalid sizes");
  for (int k = 0; k < p; ++k)
    if (!(tau[k] > 0.0)) return pivchol_refuse(PGPFA_PIVCHOL_BAD_ARG, "timescale %d is not positive", k);
  if (T < 1) return pivchol_refuse(PGPFA_PIVCHOL_REFUSED_T, "T = %d below 1", T);
  if (Tf < T) return pivchol_refuse(PGPFA_PIVCHOL_REFUSED_TF, "slab size Tf = %d below T = %d", Tf, T);
  if (pairs && Tf % 2 != 0) return pivchol_refuse(PGPFA_PIVCHOL_REFUSED_ODD, "slab size Tf = %d is odd (the pair form moves aligned row pairs)", Tf);
  size_t lds = 0;
  const int f = pivchol_launch(nullptr, Tf, T, p, nullptr, bin, eps, tol, pairs != 0, nullptr, c->st, &lds, false);
  if (lds > (size_t)64 * 1024) return pivchol_refuse(PGPFA_PIVCHOL_REFUSED_LDS, "%zu bytes of dynamic LDS, above the 65536 a launch may ask for", lds);
  HIPC(hipSetDevice(c->device));
  HIPC(hipStreamSynchronize(c->st));
  HookBuffers hb;
  double *dF = nullptr, *dtau = nullptr, *drank = nullptr;
  const size_t nf = (size_t)p * Tf * Tf;
  CHK(hb.get(&dtau, (size_t)p, 0));
  HIPC(hipMemcpy(dtau, tau, p * sizeof(double), hipMemcpyHostToDevice));
  {
    const std::vector<double> h(nf, fill);
    CHK(hook_output(hb, &dF, h.data(), nf));
  }
  // (the ranks: p ints in a buffer of doubles of their own, prefilled with -1, the band behind them)
  const size_t rd = ((size_t)p + 1) / 2;
  {
    std::vector<double> h(rd);
    std::vector<int32_t> m(2 * rd, -1);
    std::memcpy(h.data(), m.data(), rd * sizeof(double));
    CHK(hook_output(hb, &drank, h.data(), rd));
  }
  HIPC(hipDeviceSynchronize());
  const int ran = pivchol_launch(dF, Tf, T, p, dtau, bin, eps, tol, pairs != 0, reinterpret_cast<int*>(drank), c->st);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->st));
  if (ran != f) return fail("internal: the pivoted Cholesky took form %d, not %d", ran, f);
  *form = ran;
  {
    std::vector<double> h(rd);
    CHK(hook_collect("pgpfa_test_pivchol (ranks)", drank, h.data(), rd));
    std::memcpy(rank, h.data(), p * sizeof(int32_t));
  }
  return hook_collect("pgpfa_test_pivchol", dF, F, nf);
}


// distinct = true for every entry point that writes per-trial state (two slots of one chunk scattering to the same
// trial row would race, and the device list of the last E-step holds R entries)
int resolve_trials(pgpfa_ctx* c, int n, const int32_t* idx, Trials* out, bool distinct) {
  if (idx == nullptr) {
    out->v.resize(c->R);
    for (int i = 0; i < c->R; ++i) out->v[i] = i;
    return 0;
  }
  if (n < 1) return fail("empty trial list");
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= c->R) return fail("trial index %d out of range [0,%d)", idx[i], c->R);
  if (distinct) {
    if (n > c->R) return fail("trial list of %d entries for %d resident trials", n, c->R);
    std::vector<char> seen(c->R, 0);
    for (int i = 0; i < n; ++i) {
      if (seen[idx[i]]) return fail("trial %d listed twice", idx[i]);
      seen[idx[i]] = 1;
    }
  }
  out->v.assign(idx, idx + n);
  return 0;
}



const char* pgpfa_last_error(void) { return g_err.c_str(); }
int pgpfa_version(void) { return 100; }

int pgpfa_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail("hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return 0;
}

int pgpfa_create(pgpfa_ctx** out, int device, int q, int p, int T, int R, double bin_ms) {
  if (!out) return fail("null out pointer");
  *out = nullptr;
  if (q < 1 || p < 1 || T < 1 || R < 1) return fail("invalid sizes q=%d p=%d T=%d R=%d", q, p, T, R);
  if (p > 32) return fail("p=%d latents not supported (max 32)", p);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) return fail("no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
  HIPC(hipSetDevice(device));
  pgpfa_ctx* c = new pgpfa_ctx();
  c->device = device; c->q = q; c->p = p; c->T = T; c->R = R; c->bin = bin_ms;
  c->live.q = q; c->live.T = T;
  c->n = p * T;
  c->npad = round_up(c->n, NB);
  c->ld = c->npad;
  c->Tp = round_up(T, NB);
  hipError_t se = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking);
  if (se != hipSuccess) { delete c; return fail("hipStreamCreate: %s", hipGetErrorString(se)); }
  if (hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();                                // (no side stream: everything stays on the one stream)
    if (c->st2) { hipStreamDestroy(c->st2); c->st2 = nullptr; }
  }
  int rc = 0;
  const size_t slab = (size_t)c->Tp * c->Tp;
  rc |= dmalloc(c, &c->Y, (size_t)R * q * T);
  rc |= dmalloc(c, &c->C, (size_t)q * p); rc |= dmalloc(c, &c->d, q); rc |= dmalloc(c, &c->tau, p);
  rc |= dmalloc(c, &c->Kpad, slab * p); rc |= dmalloc(c, &c->Kinv, slab * p);
  rc |= dmalloc(c, &c->Xmode, (size_t)R * c->n + 64, true);
  rc |= dmalloc(c, &c->Xprev, (size_t)R * c->n + 64, true);
  c->mode_serial.assign(R, -10); c->prev_serial.assign(R, -10);
  c->info["last_log_evidence_sum"] = 0.0;
  rc |= dmalloc(c, &c->vsm, (size_t)R * T * p * p + 2048, true);
  // c->vsmgp (R*p blocks of T x T: 20 GB at config 3) is allocated on first use: the low-rank engine's default
  // sum-only output never touches it
  rc |= dmalloc(c, &c->Pauto, slab * p, true);
  rc |= dmalloc(c, &c->Pacc, slab * p, true);
  c->gemm_part_len = (size_t)16 << 20;
  rc |= dmalloc(c, &c->gemm_part, c->gemm_part_len);
  c->qpad = round_up(q, 16);
  c->ccu_cols = round_up(p * (p + 1) / 2, 16);
  if (p <= 16) {
    // widths must match the kernel instantiation dispatch_pw picks for p
    dispatch_pw(p, [&](auto pw) { constexpr int PW = decltype(pw)::value; c->ccu_cols = round_up(PW * (PW + 1) / 2, 16); });
    rc |= dmalloc(c, &c->CCu, (size_t)c->qpad * c->ccu_cols + 64, true);
    rc |= dmalloc(c, &c->C16, (size_t)c->qpad * 16 + 64, true);
  }
  c->dual_npd = round_up(p * (p + 1) / 2, 16);
  c->dual_ncol = c->dual_npd + round_up(p, 16);
  rc |= dmalloc(c, &c->dual_tbl, (size_t)round_up(q, 128) * c->dual_ncol + 4096, true);   // (GEMM tiles read whole 128-row blocks of it)
  rc |= dmalloc(c, &c->ppart, (size_t)p * (PACC_SPLITS + 1) * T * T + 256);
  c->vsmgp_ok.assign(R, 0);
  c->trial_snap.assign(R, -1);
  c->trial_dual.assign(R, 0);
  c->lam_resident.assign(R, 0);
  c->lam_valid.assign(R, 0);
  rc |= dmalloc(c, &c->Flr, slab * p + 256 * (size_t)c->Tp, true);
  rc |= dmalloc(c, &c->d_rank, p); rc |= dmalloc(c, &c->d_roff, p + 1); rc |= dmalloc(c, &c->d_roff16, p + 1);
  rc |= dmalloc(c, &c->d_cmap, (size_t)p * c->Tp + 2 * NB + 64); rc |= dmalloc(c, &c->d_nrtab, (size_t)p * c->Tp / 16 + 64);
  c->tab_cap = 4 * ((size_t)c->ld / 64 + 2 * (size_t)p + 4);
  rc |= dmalloc(c, &c->d_kr_ft, c->tab_cap); rc |= dmalloc(c, &c->d_kr_f, c->tab_cap);
  rc |= dmalloc(c, &c->sink, 128, true);
  rc |= dmalloc(c, &c->zero16, 2, true);
  rc |= dmalloc(c, &c->d_thin_ft, c->tab_cap); rc |= dmalloc(c, &c->d_thin_f, c->tab_cap); rc |= dmalloc(c, &c->d_thin_s, c->tab_cap);
  rc |= dmalloc(c, &c->Fbig, (size_t)c->ld * c->ld + 256 * (size_t)c->ld, true); rc |= dmalloc(c, &c->FTbig, (size_t)c->ld * c->ld + 256 * (size_t)c->ld, true);
  rc |= dmalloc(c, &c->Gbar, (size_t)T * p * p + 64); rc |= dmalloc(c, &c->Wtbar, (size_t)T * p * p + 64); rc |= dmalloc(c, &c->d_blk_lat, (size_t)p * c->Tp / 16 + 64); rc |= dmalloc(c, &c->d_blk_col, (size_t)p * c->Tp / 16 + 64);
  rc |= dmalloc(c, &c->vec, (size_t)q * (p + 1));
  rc |= dmalloc(c, &c->cdpart, (size_t)1024 * (p + 2) * q);
  rc |= dmalloc(c, &c->cdout, (size_t)(p + 2) * q + 8);
  rc |= dmalloc(c, &c->cdym, (size_t)(p + 1) * q + 8);
  rc |= dmalloc(c, &c->cdym_part, (size_t)1024 * (p + 1) * q);
  rc |= dmalloc(c, &c->last_trials, R);
  {
    const size_t NH = 1 + (size_t)(p + 1) + (size_t)(p + 1) * (p + 2) / 2;
    rc |= dmalloc(c, &c->cdhpart, (size_t)128 * NH * q);
    rc |= dmalloc(c, &c->cdhout, NH * q + 8);
    rc |= dmalloc(c, &c->cdcenter, (size_t)q * (p + 1));
    rc |= dmalloc(c, &c->cdpack, (size_t)q * (p + 3) + 8);
  }
  if (hipHostMalloc((void**)&c->h_pcg, 4 * sizeof(int), hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->d_hpcg, c->h_pcg, 0) != hipSuccess) { (void)hipGetLastError(); c->h_pcg = nullptr; c->d_hpcg = nullptr; }
  rc |= alloc_cholws(c, &c->kws, p * TAU_MULTI_MAX, c->Tp, true);
  c->kws.nact = round_up(T, 64);
  {
    const size_t nqmax = (size_t)p * TAU_MULTI_MAX;
    rc |= dmalloc(c, &c->tK, slab * nqmax); rc |= dmalloc(c, &c->tM, slab * nqmax); rc |= dmalloc(c, &c->tA1, slab * nqmax);
    rc |= dmalloc(c, &c->tA2, slab * nqmax);
    rc |= dmalloc(c, &c->tscal, 16 + 8 * nqmax); rc |= dmalloc(c, &c->tpart, 1024 + 64 * nqmax);
  }
  if (rc) { pgpfa_destroy(c); return 1; }
  e = hipStreamSynchronize(c->st);
  if (e != hipSuccess) { pgpfa_destroy(c); return fail("sync: %s", hipGetErrorString(e)); }
  if (const char* g = std::getenv("PGPFA_RANK_GRAN")) { const int v = std::atoi(g); if (v == 4 || v == 8 || v == 16) c->rank_gran = v; }
  c->info["n_pad"] = c->npad;
  c->info["counts_two_bytes"] = 0.0;
  c->info["trial_lengths_set"] = 0.0;
  c->info["observed_set"] = 0.0;
  c->info["observed_bins_set"] = 0.0;
  c->info["last_cd_unobserved_neurons"] = 0.0;
  c->info["arena_bytes"] = 0.0;
  c->info["last_eps_wt_norm"] = 0.0;
  c->info["last_eps_wt_rms"] = 0.0;
  c->info["last_split_cov"] = 0.0;
  c->info["last_syrk_tile"] = 0.0;
  c->info["last_split_sps"] = 0.0;
  c->info["last_cross_kernel"] = 0.0;
  c->info["last_mix_form"] = 0.0;
  c->info["last_yt_mix_fused"] = 0.0;
  c->info["last_cov_f32"] = 0.0;
  c->info["last_cov_f32_fallbacks"] = 0.0;
  for (const char* k : {"plan_ms_total", "plans", "set_params_calls", "last_retry_ms", "last_dense_retries", "last_param_step", "last_param_step_prev",
                        "last_fallback_no_descent", "last_fallback_line_search", "last_fallback_outer_cap", "arena_grow_ms_total", "last_cold_restarts"}) c->info[k] = 0.0;
  *out = c;
  return 0;
}

static void free_tables(LiveTables& L);                    // (the missing-data tables, below)

int pgpfa_destroy(pgpfa_ctx* c) {
  if (!c) return 0;
  hipSetDevice(c->device);
  if (c->st) hipStreamSynchronize(c->st);
  if (c->comm) ncclCommDestroy(c->comm);
  for (void* p : c->allocs) hipFree(p);
  if (c->vsmgp) hipFree(c->vsmgp);
  if (c->Flr32) hipFree(c->Flr32);
  if (c->lam_keep) hipFree(c->lam_keep);
  if (c->split_buf) hipFree(c->split_buf);
  if (c->Yhi) hipFree(c->Yhi);
  free_tables(c->live);
  if (c->trunc_q) hipFree(c->trunc_q);
  arena_release(c);
  if (c->hbuf) hipHostFree(c->hbuf);
  if (c->dl_stage) hipHostFree(c->dl_stage);
  if (c->hibuf) hipHostFree(c->hibuf);
  if (c->ring) hipHostFree(c->ring);
  if (c->h_pcg) hipHostFree(c->h_pcg);
  if (c->h_seq) hipHostFree(c->h_seq);
  for (auto e : c->prof.pool) hipEventDestroy(e);
  if (c->st2) { hipStreamSynchronize(c->st2); hipStreamDestroy(c->st2); }
  if (c->tau_pin) hipHostFree(c->tau_pin);
  if (c->ev_tau_fork) hipEventDestroy(c->ev_tau_fork);
  if (c->ev_tau_done) hipEventDestroy(c->ev_tau_done);
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  if (c->st) hipStreamDestroy(c->st);
  delete c;
  return 0;
}

int pgpfa_set_option(pgpfa_ctx* c, const char* key, double v) {
  if (!c || !key) return fail("null argument");
  const std::string k(key);
  auto chunk_trials = [&](int* field) -> int {              // the *_chunk_trials options of the posterior queries
    if (v < 0.0 || v != std::floor(v)) return fail("%s is a count of trials, or 0", key);
    *field = (int)v;
    return 0;
  };
  if (k == "newton_xtol") c->xtol = v;
  else if (k == "newton_max_iter") c->max_iter = (int)v;
  else if (k == "use_mfma") {
    const bool was = c->mfma;
    c->mfma = (v != 0.0);
    // (compact rank offsets need the thin products, which need the matrix cores: rebuild the rank tables, as for thin_products)
    if (c->have_params && c->rank_gran != 16 && was != c->mfma)
      CHK(pgpfa_set_params(c, std::vector<double>(c->hC).data(), std::vector<double>(c->hd).data(), std::vector<double>(c->htau).data()));
  }
  else if (k == "cd_mfma") c->cd_mfma = (v != 0.0);
  else if (k == "cd_hess_mfma") c->cd_hess_mfma = (v != 0.0);
  else if (k == "cross_kernel") c->cross_kernel = (v != 0.0);
  else if (k == "cd_debug") c->cd_debug = (int)v;
  else if (k == "pcg_fused") c->pcg_fused = (int)v;
  else if (k == "pcg_w32") c->pcg_w32 = (v != 0.0);
  else if (k == "pcg_form") c->pcg_form = (int)v;
  else if (k == "pcg_vec32") c->pcg_vec32 = (int)v;
  else if (k == "pcg_rx32") c->pcg_rx32 = (int)v;
  else if (k == "pcg_adapt") c->pcg_adapt = (int)v;
  else if (k == "pcg_xcd") c->pcg_xcd = (int)v;
  else if (k == "mt_fill") c->mt_fill = (int)v;
  else if (k == "overlap_factors") c->overlap_factors = (int)v;
  else if (k == "mix_slot") c->mix_slot = (int)v;
  else if (k == "yt_mix") c->yt_mix = (v != 0.0);
  else if (k == "pivchol_pairs") c->pivchol_pairs = (v != 0.0);
  else if (k == "vsm_b4") c->vsm_b4 = (int)v;
  else if (k == "poisson_tiles") c->poisson_tiles = (int)v;
  else if (k == "yt_mix_dbg") c->yt_mix_dbg = (int)v;
  else if (k == "yt_mix_dma") c->yt_mix_dma = (v != 0.0);
  else if (k == "syrk_dbg") c->syrk_dbg = (int)v;
  else if (k == "syrk_tile") c->syrk_tile = (int)v;
  else if (k == "mix_wide") c->mix_wide = (int)v;
  else if (k == "thin_products") {
    const bool was = c->thin_products >= 2;
    c->thin_products = (int)v;
    // (the rank tables depend on it under compact offsets: rebuild them)
    if (c->have_params && c->rank_gran != 16 && was != (c->thin_products >= 2))
      CHK(pgpfa_set_params(c, std::vector<double>(c->hC).data(), std::vector<double>(c->hd).data(), std::vector<double>(c->htau).data()));
  }
  else if (k == "copy_kernels") c->copy_kernels = (v != 0.0);
  else if (k == "chord") c->chord = (v != 0.0);
  else if (k == "shared_pcg") c->shared_pcg = (v != 0.0);
  else if (k == "time_newton") c->time_newton = (v != 0.0);
  else if (k == "pcg_trace") c->pcg_trace = (v != 0.0);
  else if (k == "measure_mix") { c->measure_mix = (v != 0.0); c->info["last_eps_wt_norm"] = 0.0; c->info["last_eps_wt_rms"] = 0.0; }
  else if (k == "pcg_retire") c->pcg_retire = (v != 0.0);
  else if (k == "split_cov") c->split_cov = (v != 0.0);
  else if (k == "split_max_norm") c->split_max_norm = v;
  else if (k == "cov_mode") c->cov_mode = (int)v;
  else if (k == "lowrank_tol") {
    const bool changed = c->lr_tol != v;
    c->lr_tol = v;
    // (the low-rank factors are built in pgpfa_set_params)
    if (c->have_params && changed)
      CHK(pgpfa_set_params(c, std::vector<double>(c->hC).data(), std::vector<double>(c->hd).data(), std::vector<double>(c->htau).data()));
  }
  else if (k == "keep_trial_vsmgp") c->keep_trial_vsmgp = (v != 0.0);
  else if (k == "dual_lowrank") c->dual_lowrank = (v != 0.0);
  else if (k == "dual_f32") c->dual_f32 = (int)v;
  else if (k == "laplace_f32") { if (v != 0.0 && v != 1.0 && v != 2.0) return fail("laplace_f32 is 0, 1 or 2"); c->laplace_f32 = (int)v; }
  else if (k == "dual_masked") { if (v != 0.0 && v != 1.0) return fail("dual_masked is 0 or 1"); c->dual_masked = (int)v; }
  else if (k == "laplace_evidence") { if (v != 0.0 && v != 1.0) return fail("laplace_evidence is 0 or 1"); c->laplace_evidence = (int)v; }
  else if (k == "sample_chunk_trials") CHK(chunk_trials(&c->sample_chunk));
  else if (k == "interp_chunk_trials") CHK(chunk_trials(&c->interp_chunk));
  else if (k == "covat_chunk_trials") CHK(chunk_trials(&c->covat_chunk));
  else if (k == "velat_chunk_trials") CHK(chunk_trials(&c->velat_chunk));
  else if (k == "covat_block_times") { if (v < 0.0 || v != std::floor(v)) return fail("covat_block_times is a count of query times, or 0"); c->covat_block = (int)v; }
  else if (k == "func_chunk_trials") CHK(chunk_trials(&c->func_chunk));
  else if (k == "func_block_cols") {
    if (v < 0.0 || v != std::floor(v) || std::fmod(v, 16.0) != 0.0) return fail("func_block_cols is a count of functionals that is a multiple of 16, or 0");
    c->func_block = (int)v;
  }
  else if (k == "rates_chunk_trials") CHK(chunk_trials(&c->rates_chunk));
  else if (k == "counts_chunk_trials") CHK(chunk_trials(&c->counts_chunk));
  else if (k == "counts_nodes") { if (v < 8.0 || v > 64.0 || v != std::floor(v)) return fail("counts_nodes is a node count in 8 .. 64"); c->counts_Q = (int)v; }
  else if (k == "slab_row_align") c->slab_row_align = (v != 0.0);
  else if (k == "vsm_mfma") c->vsm_mfma = (v != 0.0);
  else if (k == "dual_gemm") c->dual_gemm = (v != 0.0);
  else if (k == "extrapolate_start") c->extrapolate = (v != 0.0);
  else if (k == "extrapolate_beta") c->extrapolate_beta = v;
  else if (k == "extrapolate_guard") c->extrapolate_guard = v;
  else if (k == "start_guard") c->start_guard = (v != 0.0);
  else if (k == "shared_min") c->shared_min = (int)v;
  else if (k == "pcg_inner") c->pcg_inner_max = std::max(1, (int)v);
  else if (k == "pcg_eta0") c->pcg_eta0 = v;
  else if (k == "splitk_target") c->splitk_target = std::max(1, (int)v);
  else if (k == "small_tile_below") c->small_tile_below = (int)v;
  else if (k == "f32_tile64") c->f32_tile64 = (int)v;
  else if (k == "splitk_below64") c->splitk_below64 = (int)v;
  else if (k == "pcg_outer_max") c->pcg_outer_max = (int)v;
  else if (k == "chord_xtol") c->chord_xtol = v;
  else if (k == "chord_rho") c->chord_rho = v;
  else if (k == "chord_max_step") c->chord_max_step = v;
  else if (k == "chord_max") c->chord_max = (int)v;
  else if (k == "chunk_trials") { if (c->B > 0) return fail("chunk_trials must be set before the first E-step"); c->chunk_opt = (int)v; }
  else if (k == "workspace_headroom") c->arena_headroom = std::max(1.0, v);
  else if (k == "rank_gran") { if (v != 4.0 && v != 8.0 && v != 16.0) return fail("rank_gran is 4, 8 or 16"); c->rank_gran = (int)v; if (c->have_params) CHK(pgpfa_set_params(c, std::vector<double>(c->hC).data(), std::vector<double>(c->hd).data(), std::vector<double>(c->htau).data())); }
  else if (k == "workspace_pool") { if (c->arena_cap > 0) return fail("workspace_pool must be set before the first E-step"); c->use_pool = (v != 0.0); }
  else if (k == "workspace_grow_budget_ms") c->grow_budget_ms = v;
  else if (k == "workspace_grow_floor_slots") c->grow_floor_slots = std::max(1, (int)v);
  else if (k == "workspace_granule_mb") c->vmm_granule = (size_t)std::max(2.0, v) << 20;
  else if (k == "workspace_vmm") { if (c->arena_cap > 0) return fail("workspace_vmm must be set before the first E-step"); c->vmm = (v != 0.0) ? 0 : -1; }
  else if (k == "eps_noise") {
    const bool changed = c->eps != v;
    c->eps = v;
    // (the Gram matrices, their inverses and the low-rank factors are built from it in pgpfa_set_params; the E-step reads it directly)
    if (c->have_params && changed)
      CHK(pgpfa_set_params(c, std::vector<double>(c->hC).data(), std::vector<double>(c->hd).data(), std::vector<double>(c->htau).data()));
  }
  else if (k == "profile") {
    // 0: off (the accumulated sums stay readable), 1: time every tagged launch, 2: GEMM launches only
    if (v != 0.0) {
      prof_collect(c);
      c->prof.ms.clear(); c->prof.flops.clear(); c->prof.count.clear(); c->prof.max_ms.clear(); c->prof.max_flops.clear(); c->prof.shapes.clear();
      // the events the run will cycle through are created and recorded once NOW: the runtime sets up its signal pools
      // on first use (a one-off ~30 ms that would otherwise land somewhere inside the region being timed)
      HIPC(hipSetDevice(c->device));
      const size_t want = 2 * (256 + 64) + 2;
      while (c->prof.pool.size() < want) {
        hipEvent_t e;
        HIPC(hipEventCreate(&e));
        c->prof.pool.push_back(e);
        c->prof.idle.push_back(e);
      }
      for (int rep = 0; rep < 8; ++rep)            // (the one-off was seen after ~2000 recordings, not at creation)
        for (hipEvent_t e : c->prof.idle) HIPC(hipEventRecord(e, c->st));
      HIPC(hipStreamSynchronize(c->st));
    }
    c->prof.on = (v != 0.0);
    c->prof.configured = c->prof.on;
    c->prof.only_tag = (v == 2.0) ? TAG_GEMM : (v == 3.0) ? TAG_MIX : -1;     // (3: only the product-and-mixing launch of the covariance phase)
  } else if (k == "profile_pause") {
    // 1: stop recording events without touching the sums or waiting for anything; 0: go on (only while "profile" is set).  An event pair
    // around a launch costs ~10 us of device time (two barrier packets): a caller that wants rates over a long region samples it.
    c->prof.on = (v == 0.0) && c->prof.configured;
  } else return fail("unknown option '%s'", key);
  return 0;
}

int pgpfa_get_info(pgpfa_ctx* c, const char* key, double* value) {
  if (!c || !key || !value) return fail("null argument");
  const std::string k(key);
  static const char* tags[TAG_N] = {"gemm", "potrf", "solve", "poisson", "assemble", "vsm", "cd", "mix"};
  if (k.rfind("prof_", 0) == 0) {
    prof_collect(c);
    for (int t = 0; t < TAG_N; ++t) {
      const std::string base = std::string("prof_") + tags[t];
      if (k == base + "_ms") { *value = c->prof.ms[t]; return 0; }
      if (k == base + "_flops") { *value = c->prof.flops[t]; return 0; }
      if (k == base + "_launches") { *value = c->prof.count[t]; return 0; }
      if (k == base + "_max_ms") { *value = c->prof.max_ms[t]; return 0; }
      if (k == base + "_max_flops") { *value = c->prof.max_flops[t]; return 0; }
    }
    return fail("unknown info key '%s'", key);
  }
  if (k == "sample_noise_dim") {                             // normals per draw of the next pgpfa_posterior_sample: p T, + the rank under the low-rank engine
    if (!c->have_params) return fail("set_params has not been called");
    *value = (double)(c->n + (want_lowrank(c) ? c->rtot : 0));
    return 0;
  }
  if (k == "hbm_bytes_allocated") { *value = (double)c->bytes; return 0; }
  if (k == "hbm_bytes_free" || k == "hbm_bytes_total") {
    size_t free_b = 0, total_b = 0;
    HIPC(hipSetDevice(c->device));
    HIPC(hipMemGetInfo(&free_b, &total_b));
    *value = (double)(k == "hbm_bytes_free" ? free_b : total_b);
    return 0;
  }
  if (k == "n_trials_global") { *value = c->n_trials_global; return 0; }
  auto it = c->info.find(k);
  if (it == c->info.end()) return fail("unknown info key '%s'", key);
  *value = it->second;
  return 0;
}

// The resident counts of the listed trials (NULL: all) have been replaced: everything derived from them is stale - the hoisted count
// terms and Hessian sums of the (C,d) M-step, the accumulated covariance sum, and the posterior of those trials.
void counts_changed(pgpfa_ctx* c, const std::vector<int>* trials) {
  c->cdym_valid = false;
  c->cd_hess_valid = false;
  c->pacc_valid = false;
  c->have_precomp = false;
  c->have_post = false;
  if (trials) { for (int t : *trials) { c->vsmgp_ok[t] = 0; c->mode_serial[t] = -10; c->trial_snap[t] = -1; c->trial_dual[t] = 0; c->lam_resident[t] = 0; c->lam_valid[t] = 0; } }
  else {
    std::fill(c->vsmgp_ok.begin(), c->vsmgp_ok.end(), 0); std::fill(c->mode_serial.begin(), c->mode_serial.end(), -10);
    std::fill(c->trial_snap.begin(), c->trial_snap.end(), -1); std::fill(c->trial_dual.begin(), c->trial_dual.end(), 0);
    std::fill(c->lam_resident.begin(), c->lam_resident.end(), 0); std::fill(c->lam_valid.begin(), c->lam_valid.end(), 0);
  }
}

static void drop_high_plane(pgpfa_ctx* c) {
  if (!c->Yhi) return;
  hipStreamSynchronize(c->st);
  hipFree(c->Yhi);
  c->bytes -= (size_t)c->R * c->q * c->T;
  c->Yhi = nullptr;
}
int ensure_high_plane(pgpfa_ctx* c) {
  if (c->Yhi) return 0;
  const size_t n = (size_t)c->R * c->q * c->T;
  if (hipMalloc((void**)&c->Yhi, n) != hipSuccess) { (void)hipGetLastError(); c->Yhi = nullptr; return fail("hipMalloc(%zu bytes) for the high bytes of the counts failed", n); }
  HIPC(hipMemsetAsync(c->Yhi, 0, n, c->st));
  c->bytes += n;
  return 0;
}

// ---- the missing-data tables (LiveTables, live.h): lengths, observation table, per-bin table ---------------------------------------------
static_assert(OBS_NONE == 0 && OBS_ROWS == 1 && OBS_BINS == 2, "dispatch_obs (ctx.h) switches on these values");
int LiveTables::state() const { return binw ? OBS_BINS : (obs ? OBS_ROWS : OBS_NONE); }

static void free_tables(LiveTables& L) {
  if (L.trial_len) hipFree(L.trial_len);
  if (L.obs) hipFree(L.obs);
  if (L.binw) hipFree(L.binw);
  if (L.nlive) hipFree(L.nlive);
}

int refuse_tables(const pgpfa_ctx* c, const char* entry, int allowed, int with_dual_masked) {
  if (!c) return 0;
  const LiveTables& L = c->live;
  const int set = (L.trial_len ? TBL_LEN : 0) | (L.obs ? TBL_ROWS : 0) | (L.binw ? TBL_BINS : 0);
  int bad = set & ~(allowed | with_dual_masked);
  if (!bad && !c->dual_masked) bad = set & ~allowed;
  if (bad & TBL_LEN)
    return fail("%s does not support trials of unequal length yet: per-trial bin counts are set (pgpfa_set_trial_lengths) and the padded bins "
                "would be treated as data", entry);
  if (bad & TBL_ROWS)
    return fail("%s does not support unobserved neurons yet: an observation table is set (pgpfa_set_observed) and the unobserved rows "
                "would be treated as silent neurons", entry);
  if (bad & TBL_BINS)
    return fail("%s does not support a per-bin observation table yet: one is set (pgpfa_set_observed_bins) and the entries it marks as not "
                "recorded would be treated as zero counts", entry);
  return 0;
}

// cnt[r] = number of non-zero counts of trial r (either byte plane) at entries that are not live under the tables given (each may be NULL): bins
// t >= len[r], rows n with obs[r][n] == 0, clear bits of the words [R][q + 1][nw].  grid = R, block = 256 (a wave per neuron row)
static __global__ __launch_bounds__(256) void dead_counts_kernel(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ Yhi, const int* __restrict__ len,
                                                                 const uint8_t* __restrict__ obs, const unsigned long long* __restrict__ words, int q, int T, int nw,
                                                                 int* __restrict__ cnt) {
  __shared__ int red[4];
  const size_t r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = len ? len[r] : T;
  int bad = 0;
  for (int n = wave; n < q; n += 4) {
    const bool row = !obs || obs[r * q + n] != 0;            // (uniform over the wave)
    const size_t base = (r * q + n) * T;
    for (int t = lane; t < T; t += 64) {
      const bool live = row && t < L && (!words || ((words[(r * (q + 1) + n) * nw + (t >> 6)] >> (t & 63)) & 1ull));
      bad += !live && (Y[base + t] != 0 || (Yhi && Yhi[base + t] != 0));
    }
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
  if (lane == 0) red[wave] = bad;
  __syncthreads();
  if (threadIdx.x == 0) cnt[r] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The resident counts against ONE device table (the other two pointers NULL; len_h: host copy of len): fails, naming the first trial, on a non-zero
// count at an entry the table marks dead.
static int check_dead_counts(pgpfa_ctx* c, const char* entry, const int* len, const std::vector<int>* len_h, const uint8_t* obs, const unsigned long long* words) {
  int* dcnt = nullptr;
  if (hipMalloc((void**)&dcnt, (size_t)c->R * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return fail("hipMalloc failed"); }
  std::vector<int> bad(c->R, 0);
  hipLaunchKernelGGL(dead_counts_kernel, dim3(c->R), dim3(256), 0, c->st, c->Y, c->Yhi, len, obs, words, c->q, c->T, (c->T + 63) / 64, dcnt);
  hipMemcpyAsync(bad.data(), dcnt, (size_t)c->R * sizeof(int), hipMemcpyDeviceToHost, c->st);
  const hipError_t e = hipStreamSynchronize(c->st);
  hipFree(dcnt);
  if (e != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: %s", entry, hipGetErrorString(e));
  for (int r = 0; r < c->R; ++r) {
    if (!bad[r]) continue;
    if (len) return fail("trial %d: %d non-zero counts at padded bins (t >= %d): the count tensor must be zero-padded behind a trial's length", r, bad[r], (*len_h)[r]);
    if (obs) return fail("trial %d: %d non-zero counts at unobserved neurons: the count tensor must be zero at the rows the table marks as not recorded", r, bad[r]);
    return fail("trial %d: %d non-zero counts at entries the per-bin table marks as not recorded: the count tensor must be zero there", r, bad[r]);
  }
  return 0;
}

// One word of 64 bins per workgroup (a single wave): bit t & 63 of words[r][n][t >> 6] = entry (r, n, t) is live - marked in raw, inside the trial's
// length (len may be NULL) and the neuron recorded on the trial (obs may be NULL).  Row q of a trial collects the OR over its neurons, nlive[r][n]
// the popcounts.  words and nlive come in zeroed.  grid = R q ceil(T/64), block = 64
static __global__ __launch_bounds__(64) void pack_bins_kernel(const uint8_t* __restrict__ raw, const int* __restrict__ len, const uint8_t* __restrict__ obs,
                                                              int q, int T, int nw, unsigned long long* __restrict__ words, int* __restrict__ nlive) {
  const int lane = threadIdx.x;
  const int w = blockIdx.x % nw, n = (blockIdx.x / nw) % q;
  const size_t r = blockIdx.x / ((unsigned)nw * q);
  const int t = w * 64 + lane;
  const bool live = t < T && raw[(r * q + n) * T + t] != 0 && (!len || t < len[r]) && (!obs || obs[r * q + n] != 0);
  const unsigned long long m = __ballot(live);
  if (lane == 0) {
    words[(r * (q + 1) + n) * nw + w] = m;
    if (m) {
      atomicAdd(&nlive[r * q + n], __popcll(m));
      atomicOr(&words[(r * (q + 1) + q) * nw + w], m);
    }
  }
}

// The device image of a per-bin table from the caller's bytes `raw` and the given length and observation tables (device pointers, either may be
// NULL): built and validated - every trial and every neuron keeps a live entry, counts at dead entries are zero.  The caller owns *dw and *dnl.
static int build_bin_words(pgpfa_ctx* c, const char* entry, const std::vector<uint8_t>& raw, const int* dlen, const uint8_t* dobs, unsigned long long** dw, int** dnl,
                           std::vector<int>* nl) {
  const int R = c->R, q = c->q, T = c->T, nw = (T + 63) / 64;
  const size_t nwords = (size_t)R * (q + 1) * nw, nblocks = (size_t)R * q * nw;
  if (nblocks > 0x7fffffffull) return fail("pgpfa_set_observed_bins: R q ceil(T/64) = %zu exceeds the grid limit", nblocks);
  uint8_t* draw = nullptr;
  *dw = nullptr; *dnl = nullptr;
  auto release = [&]() { if (draw) hipFree(draw); if (*dw) hipFree(*dw); if (*dnl) hipFree(*dnl); draw = nullptr; *dw = nullptr; *dnl = nullptr; };
  if (hipMalloc((void**)&draw, raw.size()) != hipSuccess || hipMalloc((void**)dw, nwords * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)dnl, (size_t)R * q * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    release();
    return fail("hipMalloc for the per-bin observation table failed");
  }
  nl->assign((size_t)R * q, 0);
  hipMemcpyAsync(draw, raw.data(), raw.size(), hipMemcpyHostToDevice, c->st);
  hipMemsetAsync(*dw, 0, nwords * sizeof(unsigned long long), c->st);
  hipMemsetAsync(*dnl, 0, (size_t)R * q * sizeof(int), c->st);
  hipLaunchKernelGGL(pack_bins_kernel, dim3((unsigned)nblocks), dim3(64), 0, c->st, draw, dlen, dobs, q, T, nw, *dw, *dnl);
  hipMemcpyAsync(nl->data(), *dnl, (size_t)R * q * sizeof(int), hipMemcpyDeviceToHost, c->st);
  hipError_t e = hipStreamSynchronize(c->st);            // (the host vectors and the device temporaries outlive every copy and the kernel)
  if (e == hipSuccess) e = hipGetLastError();
  hipFree(draw); draw = nullptr;
  if (e != hipSuccess) { release(); return fail("pgpfa_set_observed_bins: %s", hipGetErrorString(e)); }
  for (int r = 0; r < R; ++r) {
    long long seen = 0;
    for (int n = 0; n < q; ++n) seen += (*nl)[(size_t)r * q + n];
    if (!seen) { release(); return fail("trial %d has no live entry under the per-bin table (with lengths and the observation table folded in)", r); }
  }
  for (int n = 0; n < q; ++n) {
    long long seen = 0;
    for (int r = 0; r < R; ++r) seen += (*nl)[(size_t)r * q + n];
    if (!seen) { release(); return fail("neuron %d has no live entry on any trial under the per-bin table", n); }
  }
  if (check_dead_counts(c, entry, nullptr, nullptr, nullptr, *dw)) { release(); return 1; }
  return 0;
}

// What a setter hands to install_tables: the one table it replaces and the candidate's host copy (an empty vector drops the table).
struct TableEdit {
  int which;                                     // TBL_LEN, TBL_ROWS or TBL_BINS
  std::vector<int> len;                          // TBL_LEN: [R]
  std::vector<uint8_t> bytes;                    // TBL_ROWS: [R][q]; TBL_BINS: [R][q][T]; 0 / 1
};

// The one routine through which a table changes.  The candidate combination - the edited table with the other two as they are - is validated against
// the resident counts (the edited table on its own, then the bin words rebuilt from all three when a per-bin table is part of it) and only then put
// in place, with everything computed under the tables before marked stale.  On failure the context keeps what it had.
static int install_tables(pgpfa_ctx* c, const char* entry, TableEdit& ed) {
  LiveTables& L = c->live;
  const size_t R = c->R, q = c->q;
  const int which = ed.which;
  // device image of a new length / observation table
  void* dnew = nullptr;
  const size_t nbytes = which == TBL_LEN ? R * sizeof(int) : R * q;
  const void* src = which == TBL_LEN ? (const void*)ed.len.data() : (const void*)ed.bytes.data();
  if (which != TBL_BINS && (which == TBL_LEN ? !ed.len.empty() : !ed.bytes.empty())) {
    HIPC(hipMalloc(&dnew, nbytes));
    hipMemcpyAsync(dnew, src, nbytes, hipMemcpyHostToDevice, c->st);
  }
  struct Free { void* p; ~Free() { if (p) hipFree(p); } } guard{dnew};
  const int* dlen = which == TBL_LEN ? (const int*)dnew : L.trial_len;
  const uint8_t* dobs = which == TBL_ROWS ? (const uint8_t*)dnew : L.obs;
  if (dnew) CHK(check_dead_counts(c, entry, which == TBL_LEN ? dlen : nullptr, &ed.len, which == TBL_ROWS ? dobs : nullptr, nullptr));
  // the per-bin words carry the other two tables: built anew from the candidate (a trial it leaves without a live entry fails here)
  const std::vector<uint8_t>& raw = which == TBL_BINS ? ed.bytes : L.bins_h;
  unsigned long long* dw = nullptr;
  int* dnl = nullptr;
  std::vector<int> nl;
  if (!raw.empty()) CHK(build_bin_words(c, entry, raw, dlen, dobs, &dw, &dnl, &nl));
  hipStreamSynchronize(c->st);
  if (which == TBL_LEN) {
    if (L.trial_len) { hipFree(L.trial_len); c->bytes -= nbytes; }
    if (dnew) c->bytes += nbytes;
    L.trial_len = (int*)dnew;
    L.trial_len_h.swap(ed.len);
    c->info["trial_lengths_set"] = dnew ? 1.0 : 0.0;
  } else if (which == TBL_ROWS) {
    if (L.obs) { hipFree(L.obs); c->bytes -= nbytes; }
    if (dnew) c->bytes += nbytes;
    L.obs = (uint8_t*)dnew;
    L.obs_h.swap(ed.bytes);
    c->info["observed_set"] = dnew ? 1.0 : 0.0;
  } else {
    L.bins_h.swap(ed.bytes);
  }
  guard.p = nullptr;
  const size_t wbytes = R * (q + 1) * ((c->T + 63) / 64) * sizeof(unsigned long long) + R * q * sizeof(int);
  if (L.binw) { hipFree(L.binw); hipFree(L.nlive); c->bytes -= wbytes; }
  if (dw) c->bytes += wbytes;
  L.binw = dw;
  L.nlive = dnl;
  L.nlive_h.swap(nl);
  c->info["observed_bins_set"] = dw ? 1.0 : 0.0;
  counts_changed(c, nullptr);                               // sums and posteriors computed under other tables are stale
  return 0;
}

// what the three setters check before they look at their table
static int table_setter_ready(pgpfa_ctx* c, const char* entry) {
  if (!c) return fail("null context");
  if (!c->have_counts) return fail("spike counts have not been uploaded: %s checks them", entry);
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  return 0;
}

int pgpfa_set_trial_lengths(pgpfa_ctx* c, const int32_t* len) {
  CHK(table_setter_ready(c, "pgpfa_set_trial_lengths"));
  TableEdit ed{TBL_LEN};
  if (!len) return c->live.trial_len ? install_tables(c, "pgpfa_set_trial_lengths", ed) : 0;     // back to R trials of T bins
  for (int r = 0; r < c->R; ++r)
    if (len[r] < 1 || len[r] > c->T) return fail("trial %d: length %d is outside 1..T = %d", r, (int)len[r], c->T);
  ed.len.assign(len, len + c->R);
  return install_tables(c, "pgpfa_set_trial_lengths", ed);
}

int pgpfa_set_observed(pgpfa_ctx* c, const uint8_t* obs) {
  CHK(table_setter_ready(c, "pgpfa_set_observed"));
  TableEdit ed{TBL_ROWS};
  if (!obs) return c->live.obs ? install_tables(c, "pgpfa_set_observed", ed) : 0;                 // back to fully observed trials
  const size_t nq = (size_t)c->R * c->q;
  ed.bytes.resize(nq);
  for (size_t i = 0; i < nq; ++i) ed.bytes[i] = obs[i] ? 1 : 0;
  for (int r = 0; r < c->R; ++r) {
    int seen = 0;
    for (int n = 0; n < c->q; ++n) seen += ed.bytes[(size_t)r * c->q + n];
    if (!seen) return fail("trial %d has no observed neuron", r);
  }
  for (int n = 0; n < c->q; ++n) {
    int seen = 0;
    for (int r = 0; r < c->R; ++r) seen += ed.bytes[(size_t)r * c->q + n];
    if (!seen) return fail("neuron %d is observed on no trial", n);
  }
  return install_tables(c, "pgpfa_set_observed", ed);
}

int pgpfa_set_observed_bins(pgpfa_ctx* c, const uint8_t* live) {
  CHK(table_setter_ready(c, "pgpfa_set_observed_bins"));
  TableEdit ed{TBL_BINS};
  if (!live) return c->live.binw ? install_tables(c, "pgpfa_set_observed_bins", ed) : 0;          // back to the length and observation tables alone
  const size_t n = (size_t)c->R * c->q * c->T;
  ed.bytes.resize(n);
  for (size_t i = 0; i < n; ++i) ed.bytes[i] = live[i] ? 1 : 0;
  return install_tables(c, "pgpfa_set_observed_bins", ed);
}

// New counts are resident.  A length table belongs to the counts it was checked against and goes, with the bin words rebuilt without it; the
// observation and per-bin tables stay, and the new counts must be zero at their dead entries.  On failure the context has no counts (the caller
// uploads again).
static int tables_after_upload(pgpfa_ctx* c) {
  LiveTables& L = c->live;
  TableEdit drop_len{TBL_LEN};
  int rc = L.obs ? check_dead_counts(c, "pgpfa_upload_counts", nullptr, nullptr, L.obs, nullptr) : 0;
  if (!rc && L.trial_len) rc = install_tables(c, "pgpfa_upload_counts", drop_len);
  else if (!rc && L.binw) rc = check_dead_counts(c, "pgpfa_upload_counts", nullptr, nullptr, nullptr, L.binw);
  if (rc) c->have_counts = false;
  return rc;
}

int pgpfa_upload_counts_u8(pgpfa_ctx* c, const uint8_t* Y) {
  if (!c || !Y) return fail("null argument");
  HIPC(hipSetDevice(c->device));
  drop_high_plane(c);
  HIPC(hipMemcpyAsync(c->Y, Y, (size_t)c->R * c->q * c->T, hipMemcpyHostToDevice, c->st));
  HIPC(hipStreamSynchronize(c->st));
  c->have_counts = true;
  counts_changed(c, nullptr);
  c->info["counts_two_bytes"] = 0.0;
  return tables_after_upload(c);
}

// counts from a host array of TS (double or uint16): validated and split into byte planes on the device, staged in pieces
template <typename TS>
static int upload_counts_wide(pgpfa_ctx* c, const TS* Y) {
  HIPC(hipSetDevice(c->device));
  const size_t n = (size_t)c->R * c->q * c->T;
  const size_t piece = std::min<size_t>(n, (size_t)1 << 26);
  TS* tmp = nullptr;
  int* flags = nullptr;
  HIPC(hipMalloc((void**)&tmp, piece * sizeof(TS)));
  hipError_t e = hipMalloc((void**)&flags, 2 * sizeof(int));
  if (e != hipSuccess) { hipFree(tmp); return fail("hipMalloc: %s", hipGetErrorString(e)); }
  drop_high_plane(c);
  int hf[2] = {0, 0};
  int rc = 0;
  for (int pass = 0; pass < 2 && !rc; ++pass) {
    // pass 0 writes the low bytes and finds out whether any count needs a second byte; only then is the plane of high bytes
    // allocated and the split repeated (pass 1)
    hipMemsetAsync(flags, 0, 2 * sizeof(int), c->st);
    for (size_t off = 0; off < n; off += piece) {
      const size_t m = std::min(piece, n - off);
      hipMemcpyAsync(tmp, Y + off, m * sizeof(TS), hipMemcpyHostToDevice, c->st);
      hipLaunchKernelGGL(pack_counts_kernel<TS>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->st, tmp, c->Y + off, c->Yhi ? c->Yhi + off : nullptr, m, flags);
      hipStreamSynchronize(c->st);
    }
    hipMemcpy(hf, flags, 2 * sizeof(int), hipMemcpyDeviceToHost);
    if (hf[0] || !hf[1] || pass == 1) break;
    rc = ensure_high_plane(c);
  }
  hipFree(tmp);
  hipFree(flags);
  // from the first piece on, c->Y holds a mixture of old and new (or clamped) counts and the old high plane is gone: on ANY failure the
  // context has no counts and nothing derived from the old ones survives (a caller that catches the error must upload again)
  const hipError_t e_last = hipGetLastError();
  if (rc || e_last != hipSuccess || hf[0]) {
    c->have_counts = false;
    counts_changed(c, nullptr);
    c->info["counts_two_bytes"] = 0.0;
    if (rc) return rc;
    if (e_last != hipSuccess) return fail("count upload: %s", hipGetErrorString(e_last));
    return fail("spike counts must be integers in [0, 65535]");
  }
  c->have_counts = true;
  counts_changed(c, nullptr);
  c->info["counts_two_bytes"] = c->Yhi ? 1.0 : 0.0;
  return tables_after_upload(c);
}

int pgpfa_upload_counts_f64(pgpfa_ctx* c, const double* Y) {
  if (!c || !Y) return fail("null argument");
  return upload_counts_wide<double>(c, Y);
}

int pgpfa_upload_counts_u16(pgpfa_ctx* c, const uint16_t* Y) {
  if (!c || !Y) return fail("null argument");
  return upload_counts_wide<uint16_t>(c, Y);
}

// resident counts of the listed trials as uint16 [n][q][T]
int pgpfa_get_counts_u16(pgpfa_ctx* c, int n, const int32_t* idx, uint16_t* out) {
  if (!c || !out) return fail("null argument");
  if (!c->have_counts) return fail("spike counts have not been uploaded");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr));
  const size_t m = (size_t)c->q * c->T;
  std::vector<uint8_t> lo(m), hi(m, 0);
  for (size_t i = 0; i < tr.v.size(); ++i) {
    HIPC(hipMemcpyAsync(lo.data(), c->Y + (size_t)tr.v[i] * m, m, hipMemcpyDeviceToHost, c->st));
    if (c->Yhi) CHK(dl_enqueue(c, hi.data(), c->Yhi + (size_t)tr.v[i] * m, m));
    CHK(dl_flush(c));
    for (size_t e = 0; e < m; ++e) out[i * m + e] = (uint16_t)(lo[e] | (hi[e] << 8));
  }
  return 0;
}

int pgpfa_set_params(pgpfa_ctx* c, const double* C, const double* d, const double* tau_s) {
  PhaseRange range_phase("pgpfa.set_params");
  if (!c || !C || !d || !tau_s) return fail("null argument");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  for (int k = 0; k < c->p; ++k)
    if (!(tau_s[k] > 0.0) || !std::isfinite(tau_s[k])) return fail("tau[%d] = %g must be positive and finite", k, tau_s[k]);
  CHK(upload(c, c->C, C, (size_t)c->q * c->p));
  CHK(upload(c, c->d, d, c->q));
  CHK(upload(c, c->tau, tau_s, c->p));
  {
    // (the arguments may alias the stored copies: pgpfa_set_params(c, c->eC.data(), ...) restores a snapshot)
    std::vector<double> nC(C, C + (size_t)c->q * c->p), nd(d, d + c->q), nt(tau_s, tau_s + c->p);
    c->hC.swap(nC); c->hd.swap(nd); c->htau.swap(nt);
  }
  hipLaunchKernelGGL(gram_tau_kernel, dim3(c->Tp, c->p), dim3(256), 0, c->st, c->Kpad, c->Tp, c->T, c->tau, c->bin, c->eps);
  if (c->CCu)
    hipLaunchKernelGGL(poisson_tables_kernel, dim3(c->qpad), dim3(64), 0, c->st, c->C, c->q, c->p, c->qpad, c->ccu_cols, c->CCu, c->C16);
  hipLaunchKernelGGL(dual_table_kernel, dim3(c->qpad), dim3(64), 0, c->st, c->C, c->q, c->p, c->dual_ncol, c->dual_npd, c->dual_tbl);
  HIPC(hipGetLastError());
  // The two things built from the timescales do not depend on each other: the Gram inverses (p slots through the batched factor kernels: ~40 small
  // launches, two host read-backs) and the pivoted Cholesky factors (one kernel of p workgroups).  The latter goes to the side stream first.
  bool side = false;
  if (c->overlap_factors && c->st2) {
    if (hipEventRecord(c->ev_fork, c->st) == hipSuccess && hipStreamWaitEvent(c->st2, c->ev_fork, 0) == hipSuccess) {
      CHK(launch_pivchol(c, c->st2));
      HIPC(hipEventRecord(c->ev_join, c->st2));
      side = true;
    } else {
      (void)hipGetLastError();
    }
  }
  const int rc_kinv = build_kinv(c);
  if (rc_kinv) {                                            // (never leave the side stream running into buffers a failed call may free)
    if (side) (void)hipStreamSynchronize(c->st2);
    return rc_kinv;
  }
  CHK(build_lowrank(c, side));
  c->have_params = true;
  c->info["set_params_calls"] += 1.0;
  return 0;
}

int get_slabs(pgpfa_ctx* c, const double* src, double* out) {
  for (int k = 0; k < c->p; ++k) {
    HIPC(hipMemcpy2DAsync(out + (size_t)k * c->T * c->T, (size_t)c->T * sizeof(double), src + (size_t)k * c->Tp * c->Tp,
                          (size_t)c->Tp * sizeof(double), (size_t)c->T * sizeof(double), c->T, hipMemcpyDeviceToHost, c->st));
  }
  HIPC(hipStreamSynchronize(c->st));
  return 0;
}
int pgpfa_get_gram(pgpfa_ctx* c, double* K) {
  if (!c || !K) return fail("null argument");
  if (!c->have_params) return fail("set_params has not been called");
  HIPC(hipSetDevice(c->device));
  return get_slabs(c, c->Kpad, K);
}
int pgpfa_get_gram_inverse(pgpfa_ctx* c, double* Kinv) {
  if (!c || !Kinv) return fail("null argument");
  if (!c->have_params) return fail("set_params has not been called");
  HIPC(hipSetDevice(c->device));
  return get_slabs(c, c->Kinv, Kinv);
}

int ready(pgpfa_ctx* c) {
  if (!c) return fail("null context");
  if (!c->have_counts) return fail("spike counts have not been uploaded");
  if (!c->have_params) return fail("set_params has not been called");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  return ensure_workspace(c, false);
}

int ready_estep(pgpfa_ctx* c, bool allow_lowrank) {
  if (!c) return fail("null context");
  if (!c->have_counts) return fail("spike counts have not been uploaded");
  if (!c->have_params) return fail("set_params has not been called");
  if (c->tau_inflight) return fail("a timescale pass is in flight (pgpfa_mstep_tau_costgrad_multi_begin): collect it first");
  HIPC(hipSetDevice(c->device));
  return ensure_workspace(c, allow_lowrank && want_lowrank(c));
}


int pgpfa_set_modes(pgpfa_ctx* c, int n, const int32_t* idx, const double* X) {
  if (!c || !X) return fail("null argument");
  HIPC(hipSetDevice(c->device));
  Trials tr;
  CHK(resolve_trials(c, n, idx, &tr, true));
  for (size_t i = 0; i < tr.v.size(); ++i)
    HIPC(hipMemcpyAsync(c->Xmode + (size_t)tr.v[i] * c->n, X + i * c->n, c->n * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPC(hipStreamSynchronize(c->st));
  c->pacc_valid = false;          // the accumulated covariance sum belonged to the modes just overwritten
  c->cdym_valid = false;          // ... and so do the hoisted count terms sum_t y m_t and the per-neuron Hessian sums of the (C,d) M-step
  c->cd_hess_valid = false;
  for (int t_ : tr.v) c->mode_serial[t_] = -10;
  return 0;
}

// The posterior of the listed trials has just been computed under the current parameters: snapshot them once, point the trials at
// the snapshot, drop snapshots no trial refers to any more.
void snapshot_params(pgpfa_ctx* c, const std::vector<int>& trials) {
  const int id = ++c->snap_serial;
  c->snaps[id] = pgpfa_ctx::ParamSnap{c->hC, c->hd, c->htau};
  for (int t : trials) c->trial_snap[t] = id;
  std::vector<char> used(c->snaps.size() + 1, 0);
  std::map<int, int> pos;
  int i = 0;
  for (auto& kv : c->snaps) pos[kv.first] = i++;
  for (int s : c->trial_snap) if (s >= 0) used[pos[s]] = 1;
  for (auto it = c->snaps.begin(); it != c->snaps.end();) {
    if (!used[pos[it->first]]) it = c->snaps.erase(it); else ++it;
  }
}

// Run fn under the parameters of snapshot `id` (no-op switch when they are the current ones), then put the current ones back.
int with_snapshot(pgpfa_ctx* c, int id, const std::function<int()>& fn) {
  auto it = c->snaps.find(id);
  if (it == c->snaps.end()) return fn();
  const pgpfa_ctx::ParamSnap snap = it->second;              // (copy: pgpfa_set_params rewrites hC..., never the snapshots, but keep it simple)
  const bool moved = (c->hC != snap.C || c->hd != snap.d || c->htau != snap.tau);
  if (!moved) return fn();
  const std::vector<double> curC = c->hC, curd = c->hd, curtau = c->htau;
  CHK(pgpfa_set_params(c, snap.C.data(), snap.d.data(), snap.tau.data()));
  int rc = fn();
  const std::string err = g_err;
  const int rc2 = pgpfa_set_params(c, curC.data(), curd.data(), curtau.data());
  if (rc) { g_err = err; return rc; }
  return rc2;
}

int remember_trials(pgpfa_ctx* c, const std::vector<int>& v) {
  c->last_trials_h = v;
  CHK(upload_list(c, c->last_trials, v));
  c->have_post = true;
  c->have_precomp = false;
  c->pacc_valid = false;
  c->cdym_valid = false;
  return 0;
}



