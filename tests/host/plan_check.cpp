// Runs the plan arithmetic of csrc/plan.h on the cases tests/test_cpu_workspace_plan.py writes to standard input: one case per line in, one
// line of integers out.  Built by that test with the address and undefined-behaviour sanitizers; needs nothing but the standard library.
//   slots fit chunk_opt target                                            -> B capped
//   fit need must arena_cap B_full floor_slots target b0 b1 step_at step  -> B need capped short_of_floor     (bytes(n) = b0 + b1 n, + step from step_at slots on)
//   base ld npad n rpad Tp T p plan_lr                                    -> slab mt dense
//   bytes ld npad n rpad Tp T p slab mt                                   -> per_slot_bytes shared_bytes
//   headroom ld npad n rpad Tp T p factor arena_cap budget target         -> pick slab mt                      (low-rank plan)
//   engine ld npad n rpad Tp T p cov_mode                                 -> lowrank_pays want_lowrank
//   qchunk n option bytes_per_trial cap stage_bytes                       -> trials per chunk of a posterior query
//   qblock option padded_width bytes_per_column stage_bytes               -> columns per block of a posterior query
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "plan.h"

static plan::Dims read_dims(std::istream& in) {
  plan::Dims d{};
  in >> d.ld >> d.npad >> d.n >> d.rpad >> d.Tp >> d.T >> d.p;
  return d;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "slots") {
      size_t fit; int chunk_opt, target;
      in >> fit >> chunk_opt >> target;
      const plan::Slots s = plan::slot_count(fit, chunk_opt, target);
      std::printf("%lld %d\n", s.B, (int)s.capped);
    } else if (what == "fit") {
      size_t need, must, cap, b0, b1, step; int B_full, floor_slots, target, step_at;
      in >> need >> must >> cap >> B_full >> floor_slots >> target >> b0 >> b1 >> step_at >> step;
      const plan::Fit f = plan::fit_slots(need, must, cap, B_full, floor_slots, target, [&](int n) { return b0 + b1 * (size_t)n + (n >= step_at ? step : 0); });
      std::printf("%d %zu %d %d\n", f.B, f.need, (int)f.capped, (int)f.short_of_floor);
    } else if (what == "base") {
      const plan::Dims d = read_dims(in);
      int lr;
      in >> lr;
      const plan::Slabs s = plan::base_slabs(d, lr != 0);
      std::printf("%zu %zu %zu\n", s.slab, s.mt, plan::dense_elems(d));
    } else if (what == "bytes") {
      const plan::Dims d = read_dims(in);
      size_t slab, mt;
      in >> slab >> mt;
      std::printf("%zu %zu\n", plan::per_slot_bytes(d, slab, mt), plan::shared_bytes(d));
    } else if (what == "headroom") {
      const plan::Dims d = read_dims(in);
      double factor; size_t cap, budget; int target;
      in >> factor >> cap >> budget >> target;
      const plan::Slabs base = plan::base_slabs(d, true);
      const plan::Slabs s = plan::headroom_slabs(d, base, factor, cap, budget, target);
      std::printf("%.17g %zu %zu\n", plan::headroom_pick(d, base, factor, cap, target), s.slab, s.mt);
    } else if (what == "engine") {
      const plan::Dims d = read_dims(in);
      int cov_mode;
      in >> cov_mode;
      std::printf("%d %d\n", (int)plan::lowrank_pays(d), (int)plan::want_lowrank(d, cov_mode));
    } else if (what == "qchunk") {
      size_t n, bytes, cap, stage; int option;
      in >> n >> option >> bytes >> cap >> stage;
      std::printf("%d\n", plan::query_chunk(n, option, bytes, cap, stage));
    } else if (what == "qblock") {
      int option, width; size_t bytes, stage;
      in >> option >> width >> bytes >> stage;
      std::printf("%d\n", plan::query_block_cols(option, width, bytes, stage));
    } else {
      std::fprintf(stderr, "plan_check: unknown case '%s'\n", line.c_str());
      return 2;
    }
    if (!in) { std::fprintf(stderr, "plan_check: short case '%s'\n", line.c_str()); return 2; }
  }
  return 0;
}
