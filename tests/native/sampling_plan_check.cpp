// Host check (test infrastructure): the sampling plan's device functions of mppi_detmath.h
// (plan_source, plan_ar1, plan_apply over noise_block_pk), walked as the generator's serial form
// walks them: the ceil(H/2) Philox blocks of a trajectory in order, e[t-1] carried per channel.
// Prints, per requested global trajectory k, the 2H sampling normals as hex words; tests/
// test_sampling_native.py compares them with mppi_amd.sampling.apply_plan.  Built with
// -ffp-contract=off, as the library.
//   usage: sampling_plan_check seed step H beta antithetic nominal k...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mppi_detmath.h"

using namespace mppi;

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const uint64_t seed = strtoull(argv[1], nullptr, 10), step = strtoull(argv[2], nullptr, 10);
  const int H = atoi(argv[3]);
  const float beta = strtof(argv[4], nullptr);
  const int anti = atoi(argv[5]), nominal = atoi(argv[6]);
  const float g = (float)std::sqrt(1.0 - (double)beta * (double)beta);
  const int NB = (H + 1) / 2;
  for (int i = 7; i < argc; ++i) {
    const uint64_t k = strtoull(argv[i], nullptr, 10), ks = plan_source(k, anti);
    std::vector<float> o1(2 * NB), o2(2 * NB);
    float e1 = 0.0f, e2 = 0.0f;
    for (int n = 0; n < NB; ++n) {
      float a1, a2, b1, b2;
      noise_block_pk(seed, step * (uint64_t)NB + (uint64_t)n, ks, &a1, &a2, &b1, &b2);
      if (beta > 0.0f) {
        e1 = n == 0 ? a1 : plan_ar1(e1, a1, beta, g);
        e2 = n == 0 ? a2 : plan_ar1(e2, a2, beta, g);
        o1[2 * n] = e1;
        o2[2 * n] = e2;
        e1 = plan_ar1(e1, b1, beta, g);
        e2 = plan_ar1(e2, b2, beta, g);
        o1[2 * n + 1] = e1;
        o2[2 * n + 1] = e2;
      } else {
        o1[2 * n] = a1;
        o2[2 * n] = a2;
        o1[2 * n + 1] = b1;
        o2[2 * n + 1] = b2;
      }
    }
    printf("%llu", (unsigned long long)k);
    for (int t = 0; t < H; ++t) printf(" %08x", f_bits(plan_apply(o1[t], k, anti, nominal)));
    for (int t = 0; t < H; ++t) printf(" %08x", f_bits(plan_apply(o2[t], k, anti, nominal)));
    printf("\n");
  }
  return 0;
}
