// What the posterior queries share, host side (definitions: query.hip unless another unit is named): the gate of the entry points, device scratch, chunks
// and blocks of a trial list, snapshot groups, time grids and their weight slabs, and the stage that carries columns through the square root of a
// resident posterior.  Included by rates.hip, psample.hip, interp.hip, covat.hip, velat.hip and pfunc.hip, and by cov.hip for for_snapshot_groups.
#pragma once
#include "ctx.h"
#include "plan.h"

struct DevBufs {                                              // device scratch of one call of `entry`: freed on every way out
  const char* entry;
  std::vector<void*> v;
  explicit DevBufs(const char* entry_point) : entry(entry_point) {}
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() { for (void* p : v) hipFree(p); }
  template <typename T> int get(T** out, size_t count) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail("%s: hipMalloc(%zu bytes) failed: %s", entry, count * sizeof(T), hipGetErrorString(e)); }
    v.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return 0;
  }
};
constexpr size_t QUERY_STAGE_BYTES = (size_t)256 << 20;      // bound on the device staging of one chunk of a query's trial list
constexpr int GEMM_ROW_SLACK = 128;                          // the GEMM stages whole row tiles of its first operand: rows past M are read, never used
constexpr size_t QUERY_LDS_MAX = (size_t)160 << 10;          // LDS of a CU: what a query kernel stages per workgroup has to fit
// While it lives the library's GEMM launcher never cuts k (pgpfa_ctx::no_splitk; linalg.hip: gemm).  The number of k parts there follows the number of
// tiles of a launch, i.e. - in the Poisson pass, the factorisation and the triangular inverse - the number of slots of the chunk: the bits of a trial's
// square root would follow the chunk it is factored in (RootStage::factor).
struct NoSplitK {
  pgpfa_ctx* c;
  bool was;
  explicit NoSplitK(pgpfa_ctx* ctx) : c(ctx), was(ctx->no_splitk) { c->no_splitk = true; }
  ~NoSplitK() { c->no_splitk = was; }
  NoSplitK(const NoSplitK&) = delete;
  NoSplitK& operator=(const NoSplitK&) = delete;
};
// Trials per chunk of a list of n: the query's *_chunk_trials option when set, else as many as fit that bound at bytes_per_trial of staging
// (0 bytes: the whole list), at least one; never more than cap (0: no cap).
inline int query_chunk(size_t n, int option, size_t bytes_per_trial, size_t cap = 0) { return plan::query_chunk(n, option, bytes_per_trial, cap, QUERY_STAGE_BYTES); }
// A posterior is resident for a trial once a Laplace E-step (mode_serial), pgpfa_dual_finalize (its parameter snapshot) or pgpfa_set_posterior (which
// marks the blocks it uploaded, or left, as the resident ones) has written it; new counts or lengths clear all three: RESIDENT_BLOCKS.  One that can
// be sampled is one an E-step or pgpfa_dual_finalize of this context wrote - of an uploaded one only blocks are known -, with the kept lambda if it is
// variational: RESIDENT_SAMPLABLE.  Fails naming the first listed trial that has none.
enum ResidentKind { RESIDENT_BLOCKS, RESIDENT_SAMPLABLE };
int require_resident(const pgpfa_ctx* c, const std::vector<int>& trials, ResidentKind kind);
// fn(positions, dual) for the positions of `trials` that share a (parameter snapshot, Laplace / variational) pair, in the order of the pairs, under that
// snapshot's parameters (with_snapshot): blocks rebuilt on demand and queries are those of every trial's OWN E-step
int for_snapshot_groups(pgpfa_ctx* c, const std::vector<int>& trials, const std::function<int(const std::vector<int>& positions, bool dual)>& fn);

// The gate of the entry points that take a trial list and a grid or weights, behind their own argument checks: parameters set, no timescale pass in
// flight, the device; a resident posterior for every listed trial - RESIDENT_BLOCKS, or with `root_need` (what of the call needs the square root, for
// the text) the sampler's predicate RESIDENT_SAMPLABLE, with texts of the call's own for the two ways a trial misses it -; no truncated variational one.
int query_gate(pgpfa_ctx* c, const char* entry, const std::vector<int>& trials, const char* root_need = nullptr);
// every query time finite: S shared ones, or S per list entry
int check_query_times(const char* entry, const double* times, int S, bool per_trial, const std::vector<int>& trials);
// the trial of every position of a group
std::vector<int> group_trials(const std::vector<int>& trials, const std::vector<int>& pos);
// ready_estep under the engine a resident posterior of this kind takes, and the kept lambda of a variational one: before anything goes through the root
int ready_root(pgpfa_ctx* c, bool dual);
// a kernel about to be launched with `lds` bytes of dynamic LDS: opted in above the 48 KiB every kernel may have
int lds_opt_in(const void* kernel, size_t lds);
// a staged plane [rows][Spad] to the caller's [rows][S], on the context's stream
int download_plane(pgpfa_ctx* c, double* host, const double* dev, int rows, int S, int Spad);

// The query times of a call on the device: `grids` grids of S times - the shared one, or those of a chunk's list positions.
struct TimeGrids {
  pgpfa_ctx* c; const double* times; int S;                   // the caller's: [S], or [list position][S]
  double* d = nullptr;
  std::vector<double> h;                                      // the gathered grids of a chunk: alive until the stream has taken them
  int alloc(DevBufs& dev, int grids) { return dev.get(&d, (size_t)grids * S); }
  int upload_shared();
  int upload_listed(const int* pos, int nc);                  // the grids of the list positions pos[0 .. nc)
};
// a kx / A-shaped pair of weight slabs of `len` doubles each (the grids' slabs and GEMM_ROW_SLACK), zeroed: the rows t >= T stay zero for the whole call
int weight_slabs(pgpfa_ctx* c, DevBufs& dev, size_t len, double** kx, double** A);

// Columns through the square root of the resident posteriors of a chunk: Q^T = U^T L^-T per slot, U the caller's columns, column-major with the column
// stride CW.  Low-rank engine: the caller's expand kernel writes V (p T16 rows), then W^T = V_k^T F_k and Q^T = W^T L^-T (products).  Dense engine: the
// caller's own product into Q, from a GemmP of batch().
struct RootStage {
  pgpfa_ctx* c; bool lr;
  size_t q_rows;                                              // rows of a slot's Q: rpad, or npad
  int rows;                                                   // those that can hold something, a multiple of 8
  size_t CW = 0;
  double *V = nullptr, *W = nullptr, *Q = nullptr;
  RootStage(pgpfa_ctx* ctx, bool lowrank) : c(ctx), lr(lowrank), q_rows(lowrank ? (size_t)ctx->rpad : (size_t)ctx->npad), rows(round_up(lowrank ? ctx->rtot : ctx->n, 8)) {}
  long long sQ() const { return (long long)(q_rows * CW); }
  int alloc(DevBufs& dev, size_t col_stride, int chunk);      // Q, and V and W under the low-rank engine, for `chunk` slots of CW = col_stride columns, zeroed
  // curvature blocks and the factor of the slots of tos[c0 .. c0 + nc), as the joint sampler forms them (psample.hip) - with every product on one k loop
  int factor(const std::vector<int>& tos, int c0, int nc, bool dual);
  // What every product of a query sets alike, for nc slots.  They stay off the split-K path - a fixed 64-tile and a one-level batch declared as the low half
  // of a two-level one -: the number of k parts there follows the number of tiles, i.e. the chunk and the block, and the bits of a trial's covariance must not.
  pgpfa::GemmP batch(int nc) const;
  int products(int nc, size_t col0, int ncols);               // V -> W -> Q of the columns col0 .. col0 + ncols
};

// interp.hip: kx and A = Kinv kx of `grids` time grids whose times are on the device ([grid][p][T16][Spad], interp.h), as pgpfa_posterior_at forms them
int interp_weights(pgpfa_ctx* c, const double* d_times, int grids, int S, int Spad, int T16, double* kx, double* A);
// the GEMM half of interp_weights: A = Kinv rhs for `grids` right-hand sides in the layout of kx (two-level batch, fixed 64-tile, off split-K)
int interp_solve(pgpfa_ctx* c, const double* rhs, int grids, int Spad, int T16, double* A);
struct MarkKeeper {                                           // the resident marks of post_vsmGP are what they were when the call returns
  pgpfa_ctx* c;
  std::vector<std::pair<int, char>> saved;
  ~MarkKeeper() { for (auto& kv : saved) c->vsmgp_ok[kv.first] = kv.second; }
};
// the T x T blocks of the trials `tos` (one snapshot) made resident for a query: the buffer, blocks rebuilt on demand under the sum-only plan with
// post_vsm of the rebuilt trials set aside (scratch from `dev`) and put back, the marks restored when `keep` goes out of scope
int interp_blocks_resident(pgpfa_ctx* c, DevBufs& dev, MarkKeeper& keep, const std::vector<int>& tos);
// rates.hip: rates_kernel on staged planes (pgpfa_posterior_cov_at)
int rates_staged_planes(pgpfa_ctx* c, const char* entry, const double* mean, const double* cov, int Tplane, int nslots, double* eta, double* var);
