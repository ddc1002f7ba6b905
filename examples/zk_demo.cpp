// Zero-knowledge proofs (ProverKey::prove_zk, pm_plonk_prove_zk) from C++ -- no Python in the process: zero blinders give the
// plain proof byte for byte, two blinder sets give two different proofs of one witness, and a short commit key is refused.
//   g++ -std=c++17 -O2 examples/zk_demo.cpp -Iinclude -Lplonk-prototype_amd/lib -lplonk_mi355x
#include <cstdio>
#include <cstring>

#include "plonk_mi355x.hpp"

using namespace plonk_mi355x;

static uint64_t rng_state = 0x243F6A8885A308D3ULL;
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
#define REQUIRE(cond)                                          \
  do {                                                         \
    if (!(cond)) {                                             \
      std::fprintf(stderr, "zk_demo: failed: %s\n", #cond);    \
      return 1;                                                \
    }                                                          \
  } while (0)

int main() {
  try {
    Context ctx(0);
    // a 256-gate circuit  a - c = 0  (q_l = 1, q_o = -1), no copy constraints
    const size_t gn = 256;
    const Fr zero{0, 0, 0, 0}, one = EvaluationDomain::one();
    const Fr minus_one = DevicePolynomial(ctx, std::vector<Fr>{zero}).sub(DevicePolynomial(ctx, std::vector<Fr>{one})).to_host()[0];
    std::array<std::vector<Fr>, PM_PLONK_SELECTORS> sel;
    for (int s = 0; s < 7; ++s) sel[s].assign(gn, zero);
    sel[1].assign(gn, one);        // q_l
    sel[3].assign(gn, minus_one);  // q_o
    sel[6].assign(gn, one);        // q_arith
    std::vector<int64_t> sigma(4 * gn);
    for (size_t p = 0; p < 4 * gn; ++p) sigma[p] = (int64_t)p;
    std::vector<Fr> wit(4 * gn);
    for (size_t i = 0; i < gn; ++i) {
      wit[i] = wit[2 * gn + i] = random_fr();   // a = c
      wit[gn + i] = random_fr();
      wit[3 * gn + i] = random_fr();
    }
    // the commit key needs n + PM_PLONK_ZK_EXTRA_BASES points (the blinded quotient's last piece has n + 10 coefficients)
    CommitKey ck(ctx, std::vector<G1Affine>(gn + PM_PLONK_ZK_EXTRA_BASES, G1_GEN), /*precompute=*/true);
    ProverKey pk(ctx, sel, sigma, ck);
    const size_t added = pk.enable_zk();
    REQUIRE(added > 0 && pk.enable_zk() == added);
    DevicePolynomial dwit(ctx, wit);
    std::array<Fr, PM_PLONK_ZK_BLINDERS> none, b1, b2;
    none.fill(zero);
    for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i) {
      b1[i] = random_fr();
      b2[i] = random_fr();
    }
    for (bool bind : {true, false}) {
      const Proof plain = pk.prove(ck, dwit, {}, bind);
      REQUIRE(pk.prove_zk(ck, dwit, none, {}, bind).bytes == plain.bytes);
      const Proof p1 = pk.prove_zk(ck, dwit, b1, {}, bind), p2 = pk.prove_zk(ck, dwit, b2, {}, bind);
      REQUIRE(p1.bytes.size() == PM_PLONK_PROOF_BYTES && p1.bytes != plain.bytes && p1.bytes != p2.bytes);
      REQUIRE(pk.prove(ck, dwit, {}, bind).bytes == plain.bytes);   // the plain path is unchanged
    }
    // refusal: a commit key without the extra points
    CommitKey short_ck(ctx, std::vector<G1Affine>(gn + PM_PLONK_ZK_EXTRA_BASES - 1, G1_GEN), false);
    bool threw = false;
    try {
      pk.prove_zk(short_ck, dwit, b1);
    } catch (const Error& e) {
      threw = e.code == PM_ERR_LENGTH;
    }
    REQUIRE(threw);
    std::printf("zk_demo OK (%zu-gate circuit; zero blinders = the plain proof, random blinders hide it; %zu key bytes added)\n",
                gn, added);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "zk_demo: Error %d: %s\n", e.code, e.what());
    return 1;
  }
}
