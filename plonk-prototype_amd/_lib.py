"""ctypes declarations of the C ABI in ``include/plonk_mi355x.h`` (one entry per export)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PM_LIB_PATH: load another build of the same library (A/B runs of compiler flags)
LIB_PATH = os.environ.get("PM_LIB_PATH") or os.path.join(_HERE, "lib", "libplonk_mi355x.so")

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)



class PermArgs(C.Structure):
    """``pm_plonk_perm_args``"""
    _fields_ = [("wires", C.c_void_p * 4), ("sigmas", C.c_void_p * 4), ("roots", C.c_void_p),
                ("beta", C.c_uint64 * 4), ("gamma", C.c_uint64 * 4), ("k", (C.c_uint64 * 4) * 3)]


class QuotientArgs(C.Structure):
    """``pm_plonk_quotient_args``"""
    _fields_ = [("wires", C.c_void_p * 4), ("z", C.c_void_p), ("q_m", C.c_void_p), ("q_l", C.c_void_p),
                ("q_r", C.c_void_p), ("q_o", C.c_void_p), ("q_4", C.c_void_p), ("q_c", C.c_void_p),
                ("pi", C.c_void_p), ("sigmas", C.c_void_p * 4), ("l1", C.c_void_p), ("x", C.c_void_p),
                ("alpha", C.c_uint64 * 4), ("beta", C.c_uint64 * 4), ("gamma", C.c_uint64 * 4),
                ("k", (C.c_uint64 * 4) * 3), ("zh_inv", (C.c_uint64 * 4) * 4),
                ("q_arith", C.c_void_p), ("q_range", C.c_void_p), ("q_logic", C.c_void_p),
                ("q_fixed_group_add", C.c_void_p), ("q_variable_group_add", C.c_void_p),
                ("range_sep", C.c_uint64 * 4), ("logic_sep", C.c_uint64 * 4), ("fixed_sep", C.c_uint64 * 4),
                ("var_sep", C.c_uint64 * 4)]


class PlonkProof(C.Structure):
    """``pm_plonk_proof``"""
    _fields_ = [("commitments", (C.c_uint64 * 12) * 11), ("evaluations", (C.c_uint64 * 4) * 17),
                ("challenges", (C.c_uint64 * 4) * 10)]


class WitnessReport(C.Structure):
    """``pm_plonk_witness_report``"""
    _fields_ = [("failed_rows", C.c_uint64), ("first_row", C.c_uint64), ("first_mask", C.c_uint32),
                ("reserved", C.c_uint32), ("count", C.c_uint64 * 6)]


class Gadget(C.Structure):
    """``pm_plonk_gadget``"""
    _fields_ = [("kind", C.c_uint32), ("level", C.c_uint32), ("first_row", C.c_uint64), ("count", C.c_uint32),
                ("param", C.c_uint32), ("in_var", C.c_uint32 * 2)]


class GadgetReport(C.Structure):
    """``pm_plonk_gadget_report``"""
    _fields_ = [("failed", C.c_uint64), ("first_gadget", C.c_uint64), ("first_reason", C.c_uint32), ("reserved", C.c_uint32)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, C.c_uint32)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, u64p)
COMM_MSG_WORDS = 289


class Dist(C.Structure):
    """``pm_dist``"""
    _fields_ = [("world", C.c_uint32), ("rank", C.c_uint32), ("allgather", C.c_void_p), ("alltoall", C.c_void_p),
                ("user", C.c_void_p)]


ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
VK_POINTS = (C.c_uint64 * 12) * 15
PLONK_SELECTORS, PLONK_PROOF_BYTES, PLONK_BIND_PUBLIC_INPUTS, PLONK_UPSTREAM_TRANSCRIPT = 11, 1040, 1, 2
COMM_ID_BYTES, COMM_MAX_POINTS = 128, 16
LINCOMB_MAX = 16
PLONK_MAX_BATCH = 64
PLONK_NO_VAR = 0xffffffff     # PM_PLONK_NO_VAR: a wire position that belongs to no variable (value 0, sigma fixes it)
WIRE_SORT_TILE = 4096         # pairs per workgroup and pass of pm_plonk_sigma_from_wires (csrc/wire_perm.hip)

# name -> (restype, argtypes); must list every function the header declares
SIGNATURES = {
    "pm_version": (C.c_char_p, []),
    "pm_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "pm_shutdown": (None, [C.c_void_p]),
    "pm_last_error": (C.c_char_p, [C.c_void_p]),
    "pm_sync": (C.c_int, [C.c_void_p]),
    "pm_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "pm_trim": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_domain_info": (C.c_int, [C.c_uint32, u64p, u64p, u64p]),
    "pm_domain_prepare": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pm_domain_evaluate_vanishing_polynomial": (C.c_int, [C.c_uint32, u64p, u64p]),
    "pm_domain_vanishing_poly_over_coset": (C.c_int, [C.c_uint32, C.c_uint64, u64p]),
    "pm_domain_vanishing_poly_over_coset_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "pm_domain_evaluate_all_lagrange_coefficients": (C.c_int, [C.c_uint32, u64p, u64p]),
    "pm_domain_evaluate_all_lagrange_coefficients_dev": (C.c_int, [C.c_void_p, C.c_uint32, u64p, C.c_void_p, C.c_void_p]),
    "pm_fr_ntt": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, C.c_uint32, C.c_uint32]),
    "pm_fr_ntt_batch": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p, C.c_size_t,
                                  C.c_uint32, C.c_uint32, C.c_uint32]),
    "pm_fr_ntt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "pm_fr_ntt_fourstep_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_fr_ntt_fourstep_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_comm_stats": (C.c_int, [C.c_void_p, u64p, C.c_int]),
    "pm_test_host_field_op": (C.c_int, [C.c_int, u64p, u64p, u64p, C.c_size_t]),
    "pm_g1_bases_upload": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "pm_g1_bases_from_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "pm_g1_fixed_base_mul_dev": (C.c_int, [C.c_void_p, u64p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                           C.c_void_p]),
    "pm_g1_compress": (C.c_int, [u64p, C.POINTER(C.c_uint8)]),
    "pm_g1_decompress": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, u64p, u32p]),
    "pm_g1_decompress_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, u64p, u32p,
                                       C.c_void_p]),
    "pm_g1_check_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, u64p, u32p, C.c_void_p]),
    "pm_g1_compress_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_g1_bases_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u64p, u32p]),
    "pm_g1_bases_from_compressed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p),
                                              u64p, u32p]),
    "pm_g1_bases_to_compressed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pm_g1_bases_lagrange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_g1_bases_lagrange_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_g1_scalar_mul_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                       C.c_void_p]),
    "pm_g1_bases_to_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pm_g1_bases_precompute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "pm_g1_bases_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_g1_bases_len": (C.c_size_t, [C.c_void_p]),
    "pm_g1_msm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, u64p, C.c_uint32, u64p]),
    "pm_g1_msm_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                C.c_uint32, u64p, C.c_void_p]),
    "pm_g1_msm_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_uint32, C.c_uint32, u64p, C.c_void_p]),
    "pm_g1_fold": (C.c_int, [u64p, C.c_size_t, u64p]),
    "pm_g1_to_affine": (C.c_int, [u64p, u64p, C.POINTER(C.c_int)]),
    "pm_g1_to_affine_batch": (C.c_int, [u64p, C.c_size_t, u64p, C.POINTER(C.c_int)]),
    "pm_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "pm_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pm_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pm_fr_vec_op_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "pm_fr_poly_evaluate_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, u64p, u64p, C.c_void_p]),
    "pm_fr_poly_ruffini_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, u64p, C.c_void_p, C.c_void_p]),
    "pm_fr_prefix_product_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_fr_batch_inverse_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pm_fr_powers_dev": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_fr_lincomb_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), u64p, C.c_size_t, C.c_void_p,
                                    C.c_void_p]),
    "pm_plonk_perm_terms_dev": (C.c_int, [C.c_void_p, C.POINTER(PermArgs), C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "pm_plonk_quotient_dev": (C.c_int, [C.c_void_p, C.POINTER(QuotientArgs), C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_plonk_preprocess": (C.c_int, [C.c_void_p, C.POINTER(u64p), C.POINTER(C.c_int64), C.c_size_t,
                                      C.POINTER(C.c_void_p)]),
    "pm_plonk_key_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_plonk_key_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]),
    "pm_plonk_key_set_lagrange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pm_plonk_key_commit_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_char_p, C.c_void_p]),
    "pm_plonk_verifier_key": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_plonk_prove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p, C.c_size_t, C.c_uint32,
                                 C.POINTER(PlonkProof)]),
    "pm_plonk_key_enable_zk": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_plonk_prove_zk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p, C.c_size_t, C.c_uint32,
                                    u64p, C.POINTER(PlonkProof)]),
    "pm_plonk_prove_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, u64p, u64p,
                                         C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(PlonkProof)]),
    "pm_plonk_transcript_labels": (C.c_char_p, []),
    "pm_plonk_preprocess_dist": (C.c_int, [C.c_void_p, C.POINTER(Dist), C.POINTER(u64p), C.POINTER(C.c_int64), C.c_size_t,
                                           C.POINTER(C.c_void_p)]),
    "pm_plonk_dist_key_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_plonk_dist_key_bytes": (C.c_size_t, [C.c_void_p]),
    "pm_plonk_key_commit_dist": (C.c_int, [C.c_void_p, C.POINTER(Dist), C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]),
    "pm_plonk_prove_dist": (C.c_int, [C.c_void_p, C.POINTER(Dist), C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p, C.c_size_t,
                                      C.c_uint32, C.POINTER(PlonkProof)]),
    "pm_plonk_key_enable_check": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
    "pm_plonk_check_witness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p, C.c_size_t,
                                         C.POINTER(WitnessReport), C.POINTER(C.c_uint8)]),
    "pm_plonk_check_witness_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(u64p),
                                               C.POINTER(u64p), C.POINTER(C.c_size_t), C.POINTER(WitnessReport),
                                               C.POINTER(C.c_uint8)]),
    "pm_plonk_sigma_from_wires": (C.c_int, [C.c_void_p, u32p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64)]),
    "pm_plonk_sigma_from_wires_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_plonk_preprocess_wires": (C.c_int, [C.c_void_p, C.POINTER(u64p), u32p, C.c_size_t, C.c_size_t,
                                            C.POINTER(C.c_void_p)]),
    "pm_plonk_key_num_vars": (C.c_size_t, [C.c_void_p]),
    "pm_plonk_witness_from_vars_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                                 C.c_void_p]),
    "pm_plonk_key_set_gadgets": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Gadget), C.c_size_t, C.POINTER(C.c_size_t)]),
    "pm_plonk_fill_gadgets_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                            C.POINTER(GadgetReport), C.c_void_p]),
    "pm_plonk_gadget_rows": (C.c_uint64, [C.POINTER(Gadget)]),
    "pm_hades_params_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "pm_hades_params_from_key": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "pm_hades_params_info": (C.c_int, [C.c_void_p, u32p, u32p, u32p]),
    "pm_hades_params_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_hades_permute_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "pm_poseidon_hash_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_uint32, C.c_void_p]),
    "pm_poseidon_merkle_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                         C.c_void_p]),
    "pm_poseidon_merkle_paths_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p]),
    "pm_poseidon_merkle_update_work_bytes": (C.c_size_t, [C.c_size_t]),
    "pm_poseidon_merkle_update_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, u64p, C.c_void_p]),
    "pm_poseidon_merkle_verify_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pm_poseidon_ledger_create": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_uint32, u64p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "pm_poseidon_ledger_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_poseidon_ledger_info": (C.c_int, [C.c_void_p, u32p, u64p, u64p, C.POINTER(C.c_size_t)]),
    "pm_poseidon_ledger_bytes": (C.c_size_t, [C.c_uint32, C.c_uint64]),
    "pm_poseidon_ledger_empty_roots": (C.c_int, [C.c_void_p, u64p]),
    "pm_poseidon_ledger_append_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, u64p, C.c_void_p]),
    "pm_poseidon_ledger_truncate_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u64p, C.c_void_p]),
    "pm_poseidon_ledger_root_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pm_poseidon_ledger_root": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p]),
    "pm_poseidon_ledger_level": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), u64p]),
    "pm_poseidon_ledger_paths_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_poseidon_ledger_verify_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pm_hades_permute_host": (C.c_int, [C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p]),
    "pm_poseidon_hash_host": (C.c_int, [C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, C.c_size_t, u64p]),
    "pm_jubjub_base_create": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_void_p)]),
    "pm_jubjub_base_from_key": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "pm_jubjub_base_point": (C.c_int, [C.c_void_p, u64p]),
    "pm_jubjub_base_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_jubjub_fixed_mul_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_jubjub_commit_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                       C.c_void_p, C.c_void_p]),
    "pm_jubjub_mul_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_jubjub_check_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_jubjub_mul_host": (C.c_int, [u64p, u64p, C.c_uint32, u64p]),
    "pm_jubjub_add_host": (C.c_int, [u64p, u64p, u64p]),
    "pm_jubjub_msm_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p]),
    "pm_jubjub_msm_host": (C.c_int, [u64p, u64p, C.c_size_t, C.c_uint32, u64p]),
    "pm_schnorr_sign_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_uint32, C.c_void_p, C.c_void_p]),
    "pm_schnorr_verify_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_uint32, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_schnorr_sign_host": (C.c_int, [u64p, C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, u64p, u64p, C.c_uint32,
                                       u64p]),
    "pm_schnorr_verify_host": (C.c_int, [u64p, C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, u64p, u64p, C.c_uint32,
                                         u32p]),
    "pm_schnorr_verify_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_uint32, C.c_void_p, u32p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_poseidon_cipher_encrypt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t,
                                                 C.c_void_p, C.c_void_p]),
    "pm_poseidon_cipher_decrypt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_poseidon_cipher_scan_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_poseidon_cipher_scan_keys_dev": (C.c_int, [C.c_void_p, C.c_void_p, u64p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_poseidon_cipher_scan_keys_work_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t]),
    "pm_poseidon_cipher_encrypt_host": (C.c_int, [C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, u64p, C.c_uint32,
                                                  u64p]),
    "pm_poseidon_cipher_decrypt_host": (C.c_int, [C.c_uint32, C.c_uint32, u64p, u64p, C.c_uint32, u64p, u64p, u64p, C.c_uint32,
                                                  u64p, u32p]),
    "pm_fr_sqrt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_fr_sqrt_host": (C.c_int, [u64p, u64p, u32p]),
    "pm_jubjub_compress": (C.c_int, [u64p, C.POINTER(C.c_uint8)]),
    "pm_jubjub_decompress": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, u64p, u32p]),
    "pm_jubjub_compress_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pm_jubjub_decompress_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]),
    "pm_dev_copy_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]),
    "pm_plonk_proof_to_bytes": (C.c_int, [C.POINTER(PlonkProof), C.POINTER(C.c_uint8)]),
    "pm_plonk_batch_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "pm_plonk_batch_free": (None, [C.c_void_p, C.c_void_p]),
    "pm_plonk_batch_bytes": (C.c_size_t, [C.c_void_p]),
    "pm_plonk_prove_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.POINTER(u64p), C.POINTER(u64p), C.POINTER(C.c_size_t), C.c_uint32,
                                       C.POINTER(PlonkProof)]),
    "pm_plonk_batch_enable_zk": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_plonk_batch_zk_bytes": (C.c_size_t, [C.c_void_p]),
    "pm_plonk_prove_batch_zk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.POINTER(u64p), C.POINTER(u64p), C.POINTER(C.c_size_t), C.c_uint32, u64p,
                                          C.POINTER(PlonkProof)]),
    "pm_fr_poly_evaluate_many_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_size_t, u64p, u64p,
                                               C.c_void_p]),
    "pm_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "pm_comm_init": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "pm_comm_destroy": (C.c_int, [C.c_void_p]),
    "pm_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pm_g1_allgather_fold": (C.c_int, [C.c_void_p, u64p, C.c_uint32]),
    "pm_test_fold_gathered": (C.c_int, [u64p, C.c_int, C.c_uint32, u64p]),
    "pm_test_comm_deadline": (C.c_int, [C.c_long, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "pm_keccak_f1600": (None, [C.c_char_p]),
    "pm_ntt_plan": (C.c_int, [C.c_uint32, u32p, u32p]),
    "pm_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_long]),
    "pm_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "pm_profile_select": (C.c_int, [C.c_void_p, C.c_char_p]),
    "pm_profile_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "pm_test_field_op": (C.c_int, [C.c_void_p, C.c_int, u64p, u64p, u64p, C.c_size_t]),
    "pm_test_field_raw_op": (C.c_int, [C.c_void_p, C.c_int, C.c_int, u32p, u32p, C.c_size_t]),
    "pm_test_g1_raw_op": (C.c_int, [C.c_void_p, C.c_int, u32p, u32p, u32p, C.c_size_t]),
    "pm_test_glv_split": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_uint32, u64p]),
    "pm_test_host_glv_split": (C.c_int, [u64p, u64p]),
    "pm_test_jubjub_scalar_op": (C.c_int, [C.c_void_p, C.c_int, u64p, u64p, u64p, u64p, C.c_size_t]),
    "pm_test_host_jubjub_scalar_op": (C.c_int, [C.c_int, u64p, u64p, u64p, u64p, C.c_size_t]),
    "pm_test_schnorr_stride": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_test_cipher_stride": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_test_cipher_digits": (C.c_int, [u64p, C.c_uint32, C.POINTER(C.c_int8)]),
    "pm_test_cipher_scan_keys_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_long, C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_size_t)]),
    "pm_test_jubjub_msm_plan":(C.c_int, [C.c_size_t, C.c_uint32, C.c_long, C.c_uint32, u64p]),
    "pm_test_jubjub_msm_digits": (C.c_int, [u64p, C.c_uint32, C.POINTER(C.c_int32), u32p]),
    "pm_test_ledger_plan": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u32p, u64p]),
    "pm_test_ntt_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_long, C.c_long, C.c_long, C.c_uint32, C.POINTER(C.c_uint32)]),
    "pm_test_ntt_exchange_map": (C.c_int, [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)]),
    "pm_test_ntt_fixed_match": (C.c_int, [C.c_uint32] * 7 + [C.c_uint64, C.c_uint32, C.c_uint32]),
    "pm_test_ntt_last_variants": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "pm_test_ntt_launches": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_long), C.c_uint32,
                                       C.POINTER(C.c_int32)]),
    "pm_test_ntt_table_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "pm_test_ntt_step4_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "pm_test_ntt_step4_lazy_table": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_size_t,
                                               C.POINTER(C.c_size_t)]),
    "pm_test_wire_sort_plan": (C.c_int, [C.c_size_t, C.c_size_t, u32p, u32p, C.POINTER(C.c_size_t)]),
    "pm_test_host_naf": (C.c_int, [u64p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_int)]),
    "pm_test_msm_sizing": (C.c_int, [C.c_size_t, C.c_uint32, C.c_long, C.c_uint32, C.c_uint32, u64p]),
    "pm_test_msm_plan": (C.c_int, [C.c_size_t, C.c_uint32, C.c_long, C.c_uint32, C.c_uint32, C.c_long, C.c_long,
                                   u32p, u32p]),
    "pm_test_msm_geometry": (C.c_int, [C.c_size_t, C.c_long, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pm_test_plonk_linearise": (C.c_int, [C.c_size_t, u64p, u64p, u64p, C.c_uint32, u64p, u32p, u32p, u64p]),
}

PM_OK = 0
PM_ERR_BAD_ARG = -1
PM_ERR_DOMAIN_TOO_LARGE = -2
PM_ERR_OOM = -3
PM_ERR_HIP = -4
PM_ERR_NO_DEVICE = -5
PM_ERR_LENGTH = -6
PM_ERR_EXCHANGE = -7
PM_ERR_BUSY = -8
PM_ERR_POINT = -9

G1_CHECK_SUBGROUP = 1         # pm_g1_decompress* / pm_g1_check_dev / pm_g1_bases_check flag
G1_POINTS_IN_SUBGROUP = 1     # pm_g1_scalar_mul_dev / pm_g1_bases_lagrange_ex flag: the caller asserts membership
GLV_Z2 = 0xac45a4010001a4020000000100000000   # z^2: k = k1 + k2 z^2 is the split behind that flag (csrc/ec_mul.hip.h)
G1_BAD_ENCODING, G1_BAD_NOT_ON_CURVE, G1_BAD_NOT_IN_SUBGROUP = 1, 2, 3
G1_BAD_REASONS = {1: "malformed encoding or non-canonical coordinate", 2: "not on the curve", 3: "not in the subgroup"}

PLONK_ZK_BLINDERS = 17        # pm_plonk_prove_zk: blinding scalars per proof
PLONK_ZK_EXTRA_BASES = 10     # ... and commit-key points it needs beyond n

# pm_plonk_check_witness: bit k of a row's mask, and count[k] of the report
PLONK_FAIL_ARITH, PLONK_FAIL_RANGE, PLONK_FAIL_LOGIC = 1, 2, 4
PLONK_FAIL_FIXED_BASE, PLONK_FAIL_VAR_BASE, PLONK_FAIL_COPY = 8, 16, 32
PLONK_FAIL_NAMES = ("arith", "range", "logic", "fixed_base", "var_base", "copy")

# pm_plonk_key_set_gadgets / pm_plonk_fill_gadgets_dev: gadget kinds and the reasons of a report
PLONK_GADGET_RANGE, PLONK_GADGET_LOGIC, PLONK_GADGET_FIXED_BASE, PLONK_GADGET_CURVE_ADD = 0, 1, 2, 3
PLONK_GADGET_MAX_ROUNDS = 256
PLONK_GADGET_TOO_WIDE, PLONK_GADGET_SCALAR_TOO_LONG, PLONK_GADGET_DEGENERATE = 1, 2, 3
PLONK_GADGET_KINDS = ("range", "logic", "fixed_base", "curve_add")
PLONK_GADGET_REASONS = {1: "too_wide", 2: "scalar_too_long", 3: "degenerate"}
# the composed kinds of the same table (arithmetic rows only; they never fail a fill)
PLONK_COMPOSED_ARITH, PLONK_COMPOSED_BITS, PLONK_COMPOSED_MAYBE_EQUAL = 4, 5, 6
PLONK_COMPOSED_MAX_BITS = 256
PLONK_COMPOSED_KINDS = {4: "arith", 5: "bits", 6: "maybe_equal"}
# ... and a whole permutation (include/plonk_mi355x.h, PM_PLONK_PERMUTATION_HADES: count = rounds, param = full rounds)
PLONK_PERMUTATION_HADES = 7
PLONK_PERMUTATION_KINDS = {7: "hades"}
PLONK_HADES_WIDTH = 5
# ... and a variable-base scalar multiplication (PM_PLONK_GADGET_VAR_BASE: count = rounds; 8 and 9 are no kinds)
PLONK_GADGET_VAR_BASE = 10
PLONK_CHAIN_KINDS = {10: "variable_base"}
# pm_hades_permute_dev / pm_poseidon_*_dev: which kernel form runs (the bytes do not depend on it)
HADES_FORM_AUTO, HADES_FORM_THREAD, HADES_FORM_WAVE = 0, 1, 2
POSEIDON_MERKLE_MAX_HEIGHT = 15
POSEIDON_LEDGER_MAX_HEIGHT = 31   # pm_poseidon_ledger_*: the append-only tree
# pm_poseidon_merkle_verify_dev: the status of a path; LINK + l = the hash of level l is not its successor
MERKLE_PATH_OK, MERKLE_PATH_INDEX, MERKLE_PATH_LINK = 0, 1, 2
# pm_schnorr_verify_*: why a signature is not valid, the lowest that applies
SCHNORR_OK, SCHNORR_U_RANGE, SCHNORR_R_POINT, SCHNORR_PK_POINT, SCHNORR_EQUATION = 0, 1, 2, 3, 4
SCHNORR_REASONS = {1: "u_range", 2: "r_point", 3: "pk_point", 4: "equation"}
# pm_poseidon_cipher_decrypt_* / _scan_dev: the status of a decryption, the lowest that applies
CIPHER_OK, CIPHER_POINT, CIPHER_RANGE, CIPHER_TAG = 0, 1, 2, 3
CIPHER_REASONS = {1: "point", 2: "range", 3: "tag"}
CIPHER_MAX_LEN = 4            # message words of a cipher: the rate of the width-5 permutation
CIPHER_SCAN_MAX_KEYS = 64     # PM_CIPHER_SCAN_MAX_KEYS: viewing keys of one pm_poseidon_cipher_scan_keys_dev, a bit of the mask each
# pm_jubjub_decompress*: the flag, and the status of a point, the lowest that applies
JUBJUB_CHECK_SUBGROUP = 1
JUBJUB_OK, JUBJUB_BAD_RANGE, JUBJUB_BAD_NOT_ON_CURVE, JUBJUB_BAD_SIGN, JUBJUB_BAD_NOT_IN_SUBGROUP = 0, 1, 2, 3, 4
JUBJUB_CODEC_REASONS = {1: "range", 2: "not_on_curve", 3: "sign", 4: "not_in_subgroup"}

# pm_jubjub_msm_dev: the window widths the option "jubjub_msm_window_bits" may force
JUBJUB_MSM_MIN_WINDOW_BITS, JUBJUB_MSM_MAX_WINDOW_BITS = 4, 16

NTT_INVERSE = 1
NTT_COSET = 2
NTT_TRANSPOSED = 4   # pm_fr_ntt_fourstep_dev: block-transposed order between a forward and an inverse transform
SCALAR_MONTGOMERY = 0
SCALAR_CANONICAL = 1

_lib = None


class BackendMissing(RuntimeError):
    """The HIP extension is not built / not loadable.  There is no CPU fallback."""


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so with
    the same SONAME (libamdhip64.so.7) as /opt/rocm's.  Whichever loads first serves both, but
    if the system copy wins, torch later loads its bundled copy *as well* (it asks for it by
    file name) and that second runtime finds no GPU.  So when torch is installed, load its
    copy first; our library's DT_NEEDED then resolves to it and torch tensors, streams and
    our kernels share one runtime.  Without torch the library uses /opt/rocm via its RUNPATH."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load() -> C.CDLL:
    """dlopen the in-tree HIP library and bind every symbol.  Fails loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C plonk-prototype_amd/csrc`).  This package has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared export
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
