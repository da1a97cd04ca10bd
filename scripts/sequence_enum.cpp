// sequence_enum.cpp — the FULL product of the facts step_shape() depends on (tests/test_sequence_cpu.py covers it in two
// products), with the same assertions, as a stand-alone host program: slq_sequence.hpp has no HIP dependency.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/sequence_enum.cpp -o sequence_enum && ./sequence_enum
#include <cstdio>
#include <cstdlib>

#include "../primate_amd/csrc/slq_sequence.hpp"

using namespace slq::seq;

static long g_cases = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) {                                                                                           \
      fprintf(stderr, "case %ld, j = %d: %s fails (line %d)\n", g_cases, j, #cond, __LINE__);                \
      for (int i = 0; i < kNumFacts; ++i) fprintf(stderr, "%d ", a[i]);                                      \
      fprintf(stderr, "\n");                                                                                 \
      exit(1);                                                                                               \
    }                                                                                                        \
  } while (0)

static int describe_today(const int *a) {  // the parent's plan_create flags and plan_sequence(), restated on the raw facts
  const int csr = a[0], far_le4 = a[1], tiles = a[2], upper = a[3], ringR = a[4], orth = a[8], nstale = a[9], fused = a[14], merged = a[15], mgs = a[16],
            stored_u = a[17], nt = a[18], gram_sw = a[20], gram_csr_sw = a[21], ring_gen_sw = a[22], ring_deep_sw = a[23];
  const bool ringed = tiles == 2 && ringR > 0;
  const bool ring_gen = ringed && (ringR > 1 || (nt && ring_gen_sw));
  const bool ring_deep = ringed && (ringR > 1 || nt) && ring_deep_sw;
  const bool gram = ring_gen && ring_deep && merged && !mgs && upper && gram_sw;
  const bool gram_csr = csr && ringR == 0 && upper && merged && !mgs && nt && gram_sw && gram_csr_sw;
  if (!csr || fused == 0 || mgs || nstale > 0) return 0;
  if (fused == 2 || far_le4) return (((gram && ringR > 0) || gram_csr) && orth >= 1) ? 4 : 1;
  return (orth >= 1 && stored_u && merged && ringR == 0) ? 2 : 0;
}

static void check(const int *a, int j, bool prev_xt) {
  const SequenceFacts f = facts_from_array(a);
  const StepShape s = step_shape(f, j, prev_xt);
  int out[kNumShape];
  shape_to_array(s, out);
  const int deg = f.deg, r = s.r, tiles = a[2];
  const bool mgs = f.mgs || f.nstale > 0;
  const bool sweeps = s.seq >= SEQ_SWEEPS_CGS;
  const bool gram = s.seq == SEQ_GRAM_RING || s.seq == SEQ_GRAM_CSR;
  CHECK(s.seq >= 0 && s.seq <= 7);
  CHECK(r == (f.orth > 0 ? std::min(j + 1 + f.nstale, f.orth) : 0));
  if (gram) CHECK(r >= 1 && f.nstale == 0 && !mgs && f.upper && f.sw_gram);
  if (s.seq == SEQ_GRAM_RING) CHECK(s.gen && s.tiled);
  if (s.seq == SEQ_GRAM_CSR) CHECK(!s.tiled);
  if (s.seq == SEQ_STORED_U) CHECK(f.csr && !s.tiled && r >= 1 && r <= kMaxFusedR && f.merged && f.stored_u && (s.xt_dots & 2) && (s.xt_update & 2));
  else CHECK(!(s.xt_dots & 2) && !(s.xt_update & 2));
  if (r > kMaxFusedR || mgs || !f.csr || f.fused == 0) CHECK(sweeps);
  if (sweeps) CHECK(s.seq == (r == 0 ? SEQ_SWEEPS_PLAIN : mgs ? SEQ_SWEEPS_MGS : SEQ_SWEEPS_CGS) && s.xt_update == 0 && s.xt_alpha == 0);
  if (s.gen || s.alpha_upper) CHECK(tiles == 2 && f.ringR > 0);
  if (s.alpha_tiled) CHECK(s.tiled);
  const bool last = j == deg - 1 && f.basis_mode != 1 && f.last_store == 0;
  if (s.xt_update & 16) CHECK(last && s.seq != SEQ_STORED_U && !sweeps && !(s.tiled && !s.gen) && !(s.tiled && tiles != 2));
  else if (!sweeps && s.seq != SEQ_STORED_U && last) CHECK(s.tiled && !s.gen);
  if (s.xt_update & 4) CHECK(s.tiled && tiles == 2 && f.ring_rev);
  if (s.xt_alpha & 8) CHECK(s.gen && s.alpha_upper && f.rs_u_padded);
  if (s.omega) CHECK(r == 3 && f.orth == 3 && s.seq == SEQ_GRAM_RING && f.omega_on && s.est_prev == (j >= 3));
  else CHECK(!s.est_prev);
  if (s.prev_xt) CHECK(s.seq == SEQ_SEPARATE && f.cross && (s.xt_update & 1));
  else CHECK(!(s.xt_update & 1));
  if (s.seq == SEQ_SEPARATE) CHECK((s.xt_alpha & 1) == (prev_xt && j > 0 ? 1 : 0));
  const int today = describe_today(a), now = plan_sequence_of(f);
  CHECK(now == today);
  if (r <= kMaxFusedR) CHECK((gram ? 4 : s.seq == SEQ_STORED_U ? 2 : sweeps ? 0 : 1) == now);
  ++g_cases;
}

int main() {
  const int deg = 20, orths[6] = {0, 1, 3, 8, 9, 20}, steps[7] = {0, 1, 2, 8, 9, deg - 2, deg - 1};
  for (int csr = 0; csr < 2; ++csr)
  for (int far = 0; far < 2; ++far)
  for (int tiles = 0; tiles < 3; ++tiles)
  for (int ringR = 0; ringR < 3; ++ringR)
  for (int upper = 0; upper < 2; ++upper)
  for (int orth : orths)
  for (int nstale = 0; nstale <= 2; nstale += 2)
  for (int basis = 0; basis < 3; ++basis)
  for (int fused = 0; fused < 3; ++fused)
  for (int bits = 0; bits < 512; ++bits) {  // merged, mgs, stored_u, nt, gram, gram_csr, ring_gen, ring_deep, last_store
    const int ru = upper && tiles == 2 && ringR > 0;
    for (int extra = 0; extra < 4; ++extra) {  // (and, beyond the test's product: cross, prev_xt)
      const int a[kNumFacts] = {csr, far, tiles, upper, ringR, ru, ru, deg, orth, nstale, basis, csr ? 0 : 4, 0, 1, fused, bits & 1, (bits >> 1) & 1,
                                (bits >> 2) & 1, (bits >> 3) & 1, extra & 1, (bits >> 4) & 1, (bits >> 5) & 1, (bits >> 6) & 1, (bits >> 7) & 1,
                                (bits >> 8) & 1, 2, 1};
      for (int j : steps) check(a, j, (extra & 2) != 0);
    }
  }
  printf("sequence_enum: %ld cases, every assertion holds\n", g_cases);
  return 0;
}
