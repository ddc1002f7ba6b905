"""MI355X (gfx950) backend for the PLONK prover hot path of Manta-Network/Plonk-Prototype:
BLS12-381 Fr NTT (``EvaluationDomain``) and G1 MSM (``msm_variable_base`` / ``CommitKey``).

Host-side mirror of the dusk-plonk / dusk-bls12_381 interfaces the reference depends on
(ref:Cargo.toml:19-20), sitting on the C ABI of ``include/plonk_mi355x.h``.  All compute
runs in hand-written HIP kernels; importing works without a GPU, but creating a
:class:`Context` raises unless a gfx950 device and the built library are present.
"""
from ._lib import (BackendMissing, NTT_COSET, NTT_INVERSE, NTT_TRANSPOSED, SCALAR_CANONICAL,  # noqa: F401
                   SCALAR_MONTGOMERY, load, LIB_PATH)
from .host import (CommitKey, Context, DeviceVector, Error, EvaluationDomain, LagrangeCommitKey, Polynomial,  # noqa: F401
                   msm_variable_base, g1_scalar_mul,
                   g1_fold, g1_to_affine, g1_compress, g1_decompress, domain_info, ntt_plan)
from . import cipher, field, jubjub, poseidon, prover, schnorr, srs, synthetic, transcript  # noqa: F401,E402
from .cipher import (CIPHER_REASONS, CIPHER_SCAN_MAX_KEYS, PoseidonCipher, poseidon_cipher_decrypt_host,  # noqa: F401,E402
                     poseidon_cipher_encrypt_host)
from .jubjub import (JUBJUB_CODEC_REASONS, JUBJUB_GENERATOR, JubJubBase, fr_sqrt, fr_sqrt_dev, fr_sqrt_host,  # noqa: F401,E402
                     jubjub_add_host, jubjub_check, jubjub_commit, jubjub_commit_dev, jubjub_compress, jubjub_compress_dev,
                     jubjub_compress_host, jubjub_decompress, jubjub_decompress_dev, jubjub_decompress_host, jubjub_msm,
                     jubjub_msm_dev, jubjub_msm_host, jubjub_mul, jubjub_mul_dev, jubjub_mul_host)
from .poseidon import Hades, LedgerTree, MerkleTree, hades_permute_host, poseidon_hash_host  # noqa: F401,E402
from .prover import (BatchWorkspace, Circuit, Gadget, GadgetInputError, GadgetReport, Proof, ProverKey,  # noqa: F401,E402
                     UnsatisfiedWitness, WitnessReport, preprocess, prove, prove_batch, random_blinders, sigma_from_wires)
from .schnorr import SCHNORR_REASONS, Schnorr, schnorr_sign_host, schnorr_verify_host  # noqa: F401,E402
from .transcript import Transcript  # noqa: F401,E402
