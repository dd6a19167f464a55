// Host check (test infrastructure): the rollout chain's reciprocal for near-unit norms (mppi_detmath.h
// recip_near1: b = RN(sqrt(n)) from the bit pattern, y = fma(1 - b, 1 + 2^-13, 1) written as one fma on b, no transcendental) and
// the chain's quotient sequence on it (recip_div), against the IEEE operators, bit for bit.  Built and
// run by tests/test_near1_recip.py with -ffp-contract=off, as the library.
//
// usage: near1_recip_check [full|quick] [threads]
//   full (default)  every divisor b with |bits(b) - bits(1)| <= 1024
//   quick           |bits(b) - bits(1)| <= 128 and every 8th divisor beyond
// For every squared norm n that gives one of those divisors (the guard's kNear1 = 2047 ulps and a little
// beyond): b == sqrtf(n) and y == 1.0f / b.  For every
// divisor of the mode and EVERY significand a in [1, 2), both signs: recip_div(a, r) == a / b; and +-0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "mppi_detmath.h"

using namespace mppi;

static const int32_t kOne = 0x3F800000;

// quotient mismatches over every significand of a (both signs) and +-0 for the divisor r.b
static long sweep(const Recip& r) {
  long bad = 0;
  for (uint32_t m = 0; m < (1u << 23); ++m) {
    const float a = bits_f(0x3F800000u | m);
    bad += f_bits(recip_div(a, r)) != f_bits(a / r.b);
    bad += f_bits(recip_div(-a, r)) != f_bits(-a / r.b);
  }
  bad += f_bits(recip_div(0.0f, r)) != f_bits(0.0f / r.b);
  bad += f_bits(recip_div(-0.0f, r)) != f_bits(-0.0f / r.b);
  return bad;
}

// the helper's Recip for the divisor kOne + kb (through the smallest-magnitude norm that gives it)
static Recip recip_for(int kb) {
  const Recip r = recip_near1(bits_f((uint32_t)(kOne + 2 * kb)));
  if ((int32_t)f_bits(r.b) != kOne + kb) {
    printf("internal: norm %d ulps does not give divisor %d ulps\n", 2 * kb, kb);
    exit(2);
  }
  return r;
}

int main(int argc, char** argv) {
  const bool quick = argc > 1 && !strcmp(argv[1], "quick");
  unsigned nt = argc > 2 ? (unsigned)atoi(argv[2]) : std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > 16) nt = 16;

  // 1. square root and reciprocal for every norm that gives a divisor within 1024 ulps of 1: the norms the
  // guard admits (kNear1) and the three beyond that still round into the range
  long bad_b = 0, bad_y = 0, norms = 0;
  int kb_lo = 0, kb_hi = 0;
  for (int k = -(kNear1 + 1); k <= kNear1 + 2; ++k, ++norms) {
    const float n = bits_f((uint32_t)(kOne + k));
    const Recip r = recip_near1(n);
    const int kb = (int32_t)f_bits(r.b) - kOne;
    kb_lo = kb < kb_lo ? kb : kb_lo;
    kb_hi = kb > kb_hi ? kb : kb_hi;
    if (f_bits(r.b) != f_bits(sqrtf(n)) && bad_b++ < 5) printf("sqrt mismatch: norm %d ulps\n", k);
    if (f_bits(r.y) != f_bits(1.0f / r.b) && bad_y++ < 5) printf("reciprocal mismatch: norm %d ulps, divisor %d ulps\n", k, kb);
  }
  printf("norms %d .. %d ulps from 1: %ld, divisors %d .. %d ulps: %ld sqrt mismatches, %ld reciprocal mismatches\n",
         -(kNear1 + 1), kNear1 + 2, norms, kb_lo, kb_hi, bad_b, bad_y);
  if (kb_lo != -1024 || kb_hi != 1024) {
    printf("internal: divisor range\n");
    return 2;
  }

  // 2. the quotients
  std::vector<int> ks;
  for (int kb = -1024; kb <= 1024; ++kb)
    if (!quick || abs(kb) <= 128 || kb % 8 == 0) ks.push_back(kb);
  std::vector<long> bad(nt, 0);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (size_t i = t; i < ks.size(); i += nt) {
        const long b = sweep(recip_for(ks[i]));
        if (b) printf("divisor %d ulps: %ld quotient mismatches\n", ks[i], b);
        bad[t] += b;
      }
    });
  for (auto& x : th) x.join();
  long bad_q = 0;
  for (long b : bad) bad_q += b;
  const double nq = (double)ks.size() * ((double)(1u << 24) + 2.0);
  printf("%s: %zu divisors within 1024 ulps of 1, %.4g quotients (every significand, both signs, +-0): %ld quotient mismatches\n",
         quick ? "quick" : "full", ks.size(), nq, bad_q);

  // 3. the four divisors just outside the range: informative only.  The guard (squared norm within kNear1
  // ulps of 1, checked on the device by lean_bad) is what keeps them from the helper, whatever they give.
  for (int kb : {-1026, -1025, 1025, 1026}) {
    const Recip r = recip_for(kb);
    const int kn = 2 * kb;
    printf("outside: divisor %d ulps (norm %d ulps, guard %s): reciprocal %s, %ld quotient mismatches\n", kb, kn,
           (kn < -kNear1 || kn > kNear1) ? "excludes it" : "ADMITS IT",
           f_bits(r.y) == f_bits(1.0f / r.b) ? "equal" : "differs", sweep(r));
    if (kn >= -kNear1 && kn <= kNear1) return 2;
  }
  const long total = bad_b + bad_y + bad_q;
  printf("near1 reciprocal: %ld mismatches\n", total);
  return total != 0;
}
