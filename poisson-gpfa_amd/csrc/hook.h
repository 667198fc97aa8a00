// hook.h - device buffers of the test hooks (pgpfa_test_split_*, pgpfa_test_assemble_b: cov.hip; pgpfa_test_thin, pgpfa_test_pivchol: core.hip;
// pgpfa_test_bin_blocks: estep.hip): allocations of one call, output buffers that
// hold the caller's prefill in front of a band no kernel may touch.
#pragma once
#include "ctx.h"

namespace hook {
constexpr size_t HOOK_BAND = 1024;                      // doubles behind every output buffer of a hook that no kernel may touch
constexpr double HOOK_BAND_VALUE = -12345.6789;

struct HookBuffers {                                    // device allocations of one hook call, freed when it returns
  std::vector<void*> ptrs;
  ~HookBuffers() { for (void* q : ptrs) (void)hipFree(q); }
  // `count` elements + `slack` zeroed ones behind them (the general GEMM reads whole 64-row tiles: rows past M of the last column of the last slot)
  template <typename T>
  int get(T** out, size_t count, size_t slack) {
    void* q = nullptr;
    const size_t bytes = (count + slack) * sizeof(T);
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return fail("out of device memory in a test hook (%zu bytes)", bytes); }
    ptrs.push_back(q);
    if (hipMemset(q, 0, bytes) != hipSuccess) return fail("hipMemset failed in a test hook");
    *out = reinterpret_cast<T*>(q);
    return 0;
  }
};

// output buffer of `bytes` bytes (a multiple of 8) holding the caller's prefill, with the band behind it
inline int hook_output_bytes(HookBuffers& hb, void** dev, const void* host, size_t bytes) {
  char* q = nullptr;
  CHK(hb.get(&q, bytes + HOOK_BAND * sizeof(double), 0));
  HIPC(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice));
  const std::vector<double> band(HOOK_BAND, HOOK_BAND_VALUE);
  HIPC(hipMemcpy(q + bytes, band.data(), HOOK_BAND * sizeof(double), hipMemcpyHostToDevice));
  *dev = q;
  return 0;
}
// host (may be null: only the band is read) <- the buffer; fails if the band changed
inline int hook_collect_bytes(const char* what, const void* dev, void* host, size_t bytes) {
  std::vector<double> band(HOOK_BAND);
  if (host) HIPC(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(band.data(), static_cast<const char*>(dev) + bytes, HOOK_BAND * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < HOOK_BAND; ++i)
    if (band[i] != HOOK_BAND_VALUE) return fail("%s: a kernel wrote %zu doubles past the end of its output", what, i + 1);
  return 0;
}
// the same for `count` doubles
inline int hook_output(HookBuffers& hb, double** dev, const double* host, size_t count) {
  void* q = nullptr;
  CHK(hook_output_bytes(hb, &q, host, count * sizeof(double)));
  *dev = static_cast<double*>(q);
  return 0;
}
inline int hook_collect(const char* what, const double* dev, double* host, size_t count) { return hook_collect_bytes(what, dev, host, count * sizeof(double)); }
}  // namespace hook
