// Zero-knowledge proofs in a batch (ProverKey::prove_batch_zk, pm_plonk_prove_batch_zk) from C++ -- no Python in the
// process: with zero blinders a batch of four reproduces prove_batch, every member of a blinded batch equals prove_zk of the
// same witness and blinders, and two sets of blinders give different proofs.
//   g++ -std=c++17 -O2 examples/zk_batch_demo.cpp -Iinclude -Lplonk-prototype_amd/lib -lplonk_mi355x
#include <cstdio>
#include <cstring>

#include "plonk_mi355x.hpp"

using namespace plonk_mi355x;

static uint64_t rng_state = 0x13198A2E03707344ULL;
static uint64_t next_u64() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
// demo randomness only: a real prover draws its blinders from a cryptographic generator
static Fr random_fr() {
  Fr r{next_u64(), next_u64(), next_u64(), next_u64() & ((1ULL << 62) - 1)};   // < 2^254 < r
  return r;
}
static const G1Affine G1_GEN = {0x5cb38790fd530c16ULL, 0x7817fc679976fff5ULL, 0x154f95c7143ba1c1ULL,
                                0xf0ae6acdf3d0e747ULL, 0xedce6ecc21dbf440ULL, 0x120177419e0bfb75ULL,
                                0xbaac93d50ce72271ULL, 0x8c22631a7918fd8eULL, 0xdd595f13570725ceULL,
                                0x51ac582950405194ULL, 0x0e1c8c3fad0059c0ULL, 0x0bbc3efc5008a26aULL};
#define REQUIRE(cond)                                                \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "zk_batch_demo: failed: %s\n", #cond);    \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  try {
    Context ctx(0);
    // a 256-gate circuit  a - c = 0  (q_l = 1, q_o = -1), no copy constraints; four witnesses of it
    const size_t gn = 256;
    const uint32_t B = 4;
    const Fr zero{0, 0, 0, 0}, one = EvaluationDomain::one();
    const Fr minus_one = DevicePolynomial(ctx, std::vector<Fr>{zero}).sub(DevicePolynomial(ctx, std::vector<Fr>{one})).to_host()[0];
    std::array<std::vector<Fr>, PM_PLONK_SELECTORS> sel;
    for (int s = 0; s < 7; ++s) sel[s].assign(gn, zero);
    sel[1].assign(gn, one);        // q_l
    sel[3].assign(gn, minus_one);  // q_o
    sel[6].assign(gn, one);        // q_arith
    std::vector<int64_t> sigma(4 * gn);
    for (size_t p = 0; p < 4 * gn; ++p) sigma[p] = (int64_t)p;
    std::vector<Fr> wits(B * 4 * gn);
    for (uint32_t b = 0; b < B; ++b) {
      Fr* w = &wits[(size_t)b * 4 * gn];
      for (size_t i = 0; i < gn; ++i) {
        w[i] = w[2 * gn + i] = random_fr();   // a = c
        w[gn + i] = random_fr();
        w[3 * gn + i] = random_fr();
      }
    }
    CommitKey ck(ctx, std::vector<G1Affine>(gn + PM_PLONK_ZK_EXTRA_BASES, G1_GEN), /*precompute=*/true);
    ProverKey pk(ctx, sel, sigma, ck);
    pk.enable_zk();
    BatchWorkspace ws = pk.batch(B);
    const size_t plain_bytes = ws.device_bytes(), added = ws.enable_zk();
    REQUIRE(added > 0 && ws.enable_zk() == added && ws.device_bytes() == plain_bytes);
    DevicePolynomial dwits(ctx, wits);
    std::vector<DevicePolynomial> single;
    for (uint32_t b = 0; b < B; ++b)
      single.emplace_back(ctx, std::vector<Fr>(wits.begin() + (size_t)b * 4 * gn, wits.begin() + (size_t)(b + 1) * 4 * gn));
    std::array<Fr, PM_PLONK_ZK_BLINDERS> none;
    none.fill(zero);
    std::vector<std::array<Fr, PM_PLONK_ZK_BLINDERS>> zeros(B, none), b1(B), b2(B);
    for (uint32_t b = 0; b < B; ++b)
      for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i) {
        b1[b][i] = random_fr();   // every proof has its own set
        b2[b][i] = random_fr();
      }
    for (bool bind : {true, false}) {
      const std::vector<Proof> plain = pk.prove_batch(ck, ws, dwits, {}, bind);
      const std::vector<Proof> z0 = pk.prove_batch_zk(ck, ws, dwits, zeros, {}, bind);
      const std::vector<Proof> p1 = pk.prove_batch_zk(ck, ws, dwits, b1, {}, bind), p2 = pk.prove_batch_zk(ck, ws, dwits, b2, {}, bind);
      REQUIRE(plain.size() == B && z0.size() == B && p1.size() == B && p2.size() == B);
      for (uint32_t b = 0; b < B; ++b) {
        REQUIRE(z0[b].bytes == plain[b].bytes);                                            // zero blinders: the plain batch
        REQUIRE(p1[b].bytes == pk.prove_zk(ck, single[b], b1[b], {}, bind).bytes);         // = the single prover
        REQUIRE(p1[b].challenges == pk.prove_zk(ck, single[b], b1[b], {}, bind).challenges);
        REQUIRE(p2[b].bytes == pk.prove_zk(ck, single[b], b2[b], {}, bind).bytes);
        REQUIRE(p1[b].bytes != plain[b].bytes && p1[b].bytes != p2[b].bytes);
        for (uint32_t c = 0; c < b; ++c) REQUIRE(p1[b].bytes != p1[c].bytes);
      }
      REQUIRE(pk.prove_batch(ck, ws, dwits, {}, bind)[B - 1].bytes == plain[B - 1].bytes);   // the plain batch is unchanged
    }
    std::printf("zk_batch_demo OK (%u proofs of a %zu-gate circuit; %zu + %zu workspace bytes)\n", B, gn, plain_bytes, added);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "zk_batch_demo: Error %d: %s\n", e.code, e.what());
    return 1;
  }
}
