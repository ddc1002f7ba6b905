// Many proofs of one circuit in one call (ProverKey::prove_batch, pm_plonk_prove_batch) from C++ -- no Python in the process:
// a batch of distinct witnesses of one circuit, each proof compared byte for byte with the single-proof path.
//   g++ -std=c++17 -O2 examples/batch_demo.cpp -Iinclude -Lplonk-prototype_amd/lib -lplonk_mi355x
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
static Fr random_fr() {
  Fr r{next_u64(), next_u64(), next_u64(), next_u64() & ((1ULL << 62) - 1)};   // < 2^254 < r
  return r;
}
static const G1Affine G1_GEN = {0x5cb38790fd530c16ULL, 0x7817fc679976fff5ULL, 0x154f95c7143ba1c1ULL,
                                0xf0ae6acdf3d0e747ULL, 0xedce6ecc21dbf440ULL, 0x120177419e0bfb75ULL,
                                0xbaac93d50ce72271ULL, 0x8c22631a7918fd8eULL, 0xdd595f13570725ceULL,
                                0x51ac582950405194ULL, 0x0e1c8c3fad0059c0ULL, 0x0bbc3efc5008a26aULL};
#define REQUIRE(cond)                                              \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "batch_demo: failed: %s\n", #cond);     \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main() {
  try {
    Context ctx(0);
    // a 256-gate circuit  a - c + PI = 0  (q_l = 1, q_o = -1), no copy constraints; B witnesses with their own public inputs
    const size_t gn = 256;
    const uint32_t B = 6;
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
    std::vector<std::vector<PublicInput>> pis(B);
    for (uint32_t b = 0; b < B; ++b) {
      Fr* w = &wits[b * 4 * gn];
      for (size_t i = 0; i < gn; ++i) {
        w[i] = w[2 * gn + i] = random_fr();   // a = c
        w[gn + i] = random_fr();
        w[3 * gn + i] = random_fr();
      }
      // proof b: b public inputs of value 0 (the gate stays satisfied), b = 5 through the staged scatter (> 16 after b = 5 x 4)
      for (uint32_t k = 0; k < (b == 5 ? 20u : b); ++k) pis[b].push_back(PublicInput{(uint64_t)(7 * k + b) % gn, zero});
    }
    CommitKey ck(ctx, std::vector<G1Affine>(gn, G1_GEN), /*precompute=*/true);
    ProverKey pk(ctx, sel, sigma, ck);
    BatchWorkspace ws = pk.batch(8);
    REQUIRE(ws.device_bytes() >= (size_t)42 * 8 * gn * 32);
    DevicePolynomial dwits(ctx, wits);
    for (bool bind : {true, false}) {
      std::vector<Proof> proofs = pk.prove_batch(ck, ws, dwits, pis, bind);
      REQUIRE(proofs.size() == B);
      for (uint32_t b = 0; b < B; ++b) {
        DevicePolynomial one_wit(ctx, std::vector<Fr>(wits.begin() + b * 4 * gn, wits.begin() + (b + 1) * 4 * gn));
        const Proof single = pk.prove(ck, one_wit, pis[b], bind);
        REQUIRE(proofs[b].bytes == single.bytes && proofs[b].challenges == single.challenges);
      }
    }
    // refusals: a batch above the workspace's max_batch
    bool threw = false;
    try {
      DevicePolynomial big(ctx, 9 * 4 * gn);
      pk.prove_batch(ck, ws, big);
    } catch (const Error& e) {
      threw = e.code == PM_ERR_BAD_ARG;
    }
    REQUIRE(threw);
    std::printf("batch_demo OK (%u proofs of a %zu-gate circuit in one call, byte-identical to single proofs; %zu workspace bytes)\n",
                B, gn, ws.device_bytes());
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "batch_demo: Error %d: %s\n", e.code, e.what());
    return 1;
  }
}
