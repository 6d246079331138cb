// verify.hpp — the tree verifier's state (verify.hip); the C ABI's opaque sheep_verify.
#pragma once
#include "tree_tour.hpp"

struct sheep_verify {
  sheep::Ctx *ctx = nullptr;
  uint64_t n = 0;
  const sheep_jnode *tree = nullptr;
  bool toured = false;      // structure held: the arrays below are built
  bool failed = false;      // an add met a range error: there is no verdict
  uint64_t bad_parent = 0, first_bad_parent = ~0ull;
  sheep_kids k;
  char *buf = nullptr;      // one allocation: the counters, then the six arrays
  unsigned long long *ctr = nullptr;
  uint32_t *tD = nullptr, *ilo = nullptr, *ihi = nullptr, *kd = nullptr, *sup = nullptr, *cnt = nullptr;
};

namespace sheep {
void verify_begin(Ctx &c, const sheep_jnode *tree, uint64_t n, sheep_verify *h);
void verify_add(sheep_verify *h, const sheep_xs1 *rec, uint64_t nrec, const uint32_t *pos, uint64_t pos_size);
void verify_finish(sheep_verify *h, sheep_verify_t *out);
void verify_free(sheep_verify *h);   // the handle's device memory (never throws)
}  // namespace sheep
