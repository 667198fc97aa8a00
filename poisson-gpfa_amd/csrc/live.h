// Which entries (trial, neuron, bin) carry a likelihood term: the three missing-data tables of a context and the one place that knows their formats.
//   lengths  (pgpfa_set_trial_lengths)  bins t >= length(r) of trial r are padding
//   rows     (pgpfa_set_observed)       neurons not recorded on a trial
//   bins     (pgpfa_set_observed_bins)  single entries not recorded
// An entry that is not live has a zero count (checked against the resident counts whenever a table or the counts change) and no rate in the Poisson
// pass, the cold objective and the (C,d) passes; the GP prior, the solvers and the covariance engines still span all T bins.  Callers ask the
// questions below; the fields change only through install_tables (core.hip), which keeps the bin words in step with the other two tables.
#pragma once
#include <stdint.h>
#include <vector>

enum { TBL_LEN = 1, TBL_ROWS = 2, TBL_BINS = 4 };              // a table each (refuse_tables, install_tables)

struct LiveTables {
  int q = 0, T = 0;                              // of the context
  int* trial_len = nullptr;                      // device [R]; NULL: every trial has T bins
  std::vector<int> trial_len_h;                  // host copy; empty while trial_len is NULL
  uint8_t* obs = nullptr;                        // device [R][q], 0 = not recorded; NULL: every neuron is observed on every trial
  std::vector<uint8_t> obs_h;                    // host copy; empty while obs is NULL
  // The caller's per-bin table stays on the host (bins_h, one byte per entry); the device holds it as bit words of 64 bins with lengths and obs
  // folded in, [R][q + 1][ceil(T/64)] (row q of a trial: OR over its neurons - bin_words, model.h), and the live entries per (trial, neuron)
  unsigned long long* binw = nullptr;            // device; NULL: no per-bin table
  int* nlive = nullptr;                          // device [R][q]
  std::vector<int> nlive_h;                      // host copy
  std::vector<uint8_t> bins_h;                   // the caller's table [R][q][T], 0 / 1; empty while binw is NULL

  // template state OBS of the kernels that read a table: OBS_NONE / OBS_ROWS / OBS_BINS (model.h; defined in core.hip)
  int state() const;
  // `len` and `obs` of a kernel's argument struct (PoissonArgs, CdArgs): under a per-bin table `obs` carries the words (template state OBS_BINS)
  template <typename Args>
  void fill(Args& a) const {
    a.len = trial_len;
    a.obs = binw ? reinterpret_cast<const uint8_t*>(binw) : obs;
  }
  // device tables of the kernels that take them as plain arguments (NULL: not set - which is also how a caller asks whether one is)
  const int* lengths() const { return trial_len; }
  const uint8_t* rows() const { return obs; }
  const unsigned long long* words() const { return binw; }
  const int* live_counts() const { return nlive; }
  // host look-ups
  int length(int trial) const { return trial_len ? trial_len_h[trial] : T; }
  bool seen(int trial, int neuron) const {                     // the neuron has a live entry on the trial (under a per-bin table: lengths and rows folded in)
    if (binw) return nlive_h[(size_t)trial * q + neuron] != 0;
    return !obs || obs_h[(size_t)trial * q + neuron] != 0;
  }
  bool entry_live(int trial, size_t e) const {                 // entry e = n T + t of the trial, by lengths and rows (the dual path, which refuses a per-bin table)
    return (int)(e % T) < length(trial) && (!obs || obs_h[(size_t)trial * q + e / T] != 0);
  }
};
