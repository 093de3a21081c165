"""ctypes binding of libhalo_hip.so (include/halo_accumulation.h) and its build recipe."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB_PATH = os.path.join(PKG, "libhalo_hip.so")
DEV_LIB_PATH = os.path.join(PKG, "libhalo_hip_dev.so")

HALO_OK, HALO_E_ASSERT, HALO_E_REJECT, HALO_E_ARG, HALO_E_DEVICE = 0, -1, -2, -3, -4

u64p = C.POINTER(C.c_uint64)


class HaloError(RuntimeError):
    """Raised for HALO_E_ARG / HALO_E_DEVICE (library-level failures)."""


class HaloReject(ValueError):
    """The reference's `ensure!` -> Err (verifier-side rejection)."""


def build(force: bool = False, jobs: int = 4) -> str:
    """Compile every HIP translation unit for gfx950 into libhalo_hip.so (in-tree)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".cpp", ".map"))]
    srcs.append(os.path.join(PKG, "..", "include", "halo_accumulation.h"))
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", CSRC, "-j", str(jobs), "-s"])
    return LIB_PATH


_lib = None

_SIGS = {
    "halo_last_error": (C.c_char_p, []),
    "halo_device_count": (C.c_int, []),
    "halo_ctx_create": (C.c_int, [C.c_int, u64p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "halo_ctx_create_urs": (C.c_int, [C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_void_p)]),
    "halo_ctx_create_urs_strided": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_size_t, C.POINTER(C.c_void_p)]),
    "halo_ctx_create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, u64p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "halo_ctx_create_urs_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_void_p)]),
    "halo_ctx_devices": (C.c_int, [C.c_void_p]),
    "halo_ctx_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "halo_ctx_destroy": (None, [C.c_void_p]),
    "halo_ctx_size": (C.c_size_t, [C.c_void_p]),
    "halo_ctx_read_bases": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, u64p]),
    "halo_ctx_bases_dev": (C.c_void_p, [C.c_void_p]),
    "halo_ctx_stream": (C.c_void_p, [C.c_void_p]),
    "halo_public_points": (C.c_int, [u64p, u64p]),
    "halo_msm": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, u64p, C.c_int, u64p]),
    "halo_msm_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, u64p, C.c_int]),
    "halo_msm_end": (C.c_int, [C.c_void_p, C.c_int, u64p]),
    "halo_msm_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, u64p]),
    "halo_msm_dev_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int]),
    "halo_msm_dev_end": (C.c_int, [C.c_void_p, C.c_int, u64p]),
    "halo_msm_points": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p]),
    "halo_msm_affine": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, C.c_int, u64p]),
    "halo_scalar_dot": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p]),
    "halo_powers": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p]),
    "halo_poly_eval": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, u64p]),
    "halo_h_coeffs": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p]),
    "halo_h_commit": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p]),
    "halo_h_eval_batch": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p, u64p]),
    "halo_h_accumulate": (C.c_int, [C.c_void_p, u64p, u64p, u64p, C.c_size_t, C.c_size_t, u64p]),
    "halo_ipa_begin": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p, C.POINTER(C.c_void_p)]),
    "halo_ipa_begin_strided": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]),
    "halo_ipa_begin_vectors": (C.c_int, [C.c_void_p, C.c_size_t, u64p, u64p, C.POINTER(C.c_void_p)]),
    "halo_ipa_dot_cz": (C.c_int, [C.c_void_p, u64p]),
    "halo_ipa_round_lr_partial": (C.c_int, [C.c_void_p, u64p, u64p, u64p]),
    "halo_ipa_finish_z": (C.c_int, [C.c_void_p, u64p, u64p, u64p]),
    "halo_ipa_hiding_partial": (C.c_int, [C.c_void_p, C.c_uint64, C.c_size_t, u64p, C.c_uint64, C.c_uint64, u64p]),
    "halo_ipa_apply_hiding": (C.c_int, [C.c_void_p, u64p]),
    "halo_open_hiding_combine": (C.c_int, [u64p, u64p, u64p, u64p, C.c_size_t, u64p, C.POINTER(C.c_uint64), C.c_size_t, u64p, u64p, u64p, u64p]),
    "halo_open_start": (C.c_int, [u64p, u64p, u64p, C.c_size_t, u64p, u64p, u64p]),
    "halo_open_combine": (C.c_int, [u64p, C.c_size_t, u64p, u64p, u64p, u64p, u64p, u64p]),
    "halo_open_tail": (C.c_int, [u64p, C.c_size_t, u64p, u64p, u64p, u64p, u64p, u64p]),
    "halo_ipa_round_lr": (C.c_int, [C.c_void_p, u64p, u64p, u64p]),
    "halo_ipa_round_fold": (C.c_int, [C.c_void_p, u64p, u64p]),
    "halo_ipa_finish": (C.c_int, [C.c_void_p, u64p, u64p]),
    "halo_ipa_destroy": (None, [C.c_void_p]),
    "halo_ipa_len": (C.c_size_t, [C.c_void_p]),
    "halo_proof_words": (C.c_size_t, [C.c_size_t]),
    "halo_instance_words": (C.c_size_t, [C.c_size_t]),
    "halo_accumulator_words": (C.c_size_t, [C.c_size_t]),
    "halo_pedersen_commit": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t, u64p]),
    "halo_pedersen_commit_affine": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p]),
    "halo_pcdl_commit": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p, u64p]),
    "halo_pcdl_open": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), u64p, C.c_size_t, u64p, C.c_size_t, u64p, u64p, u64p]),
    "halo_pcdl_open_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p, u64p, u64p]),
    "halo_pcdl_commit_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, u64p, u64p]),
    "halo_pcdl_succinct_check": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, u64p, u64p, u64p, u64p]),
    "halo_pcdl_succinct_check_batch": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_pcdl_check": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, u64p, u64p]),
    "halo_pcdl_check_batch": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_int)]),
    "halo_pcdl_check_batch_combined": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_acc_decider_batch_combined": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_pcdl_check_batch_fused": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_acc_decider_batch_fused": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_pcdl_check_batch_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_int)]),
    "halo_pcdl_check_batch_mixed_combined": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_acc_decider_batch_mixed": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_int)]),
    "halo_acc_decider_batch_mixed_combined": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_pcdl_check_batch_mixed_fused": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_acc_decider_batch_mixed_fused": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.c_size_t, C.c_char_p, C.POINTER(C.c_int)]),
    "halo_pcdl_check_partial": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, u64p, u64p, C.c_uint64, C.c_uint64, u64p, u64p]),
    "halo_pcdl_open_sharded": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), u64p, C.c_size_t, C.c_size_t, u64p, C.c_size_t,
                                         u64p, u64p, C.c_void_p, C.c_void_p, u64p, u64p]),
    "halo_pcdl_check_sharded": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u64p, C.c_size_t, u64p, u64p, u64p, C.c_void_p, C.c_void_p]),
    "halo_msm_sharded": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_size_t, u64p, C.c_int, C.c_void_p, C.c_void_p, u64p]),
    "halo_msm_dev_sharded": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, u64p]),
    "halo_msm_end_sharded": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, u64p]),
    "halo_acc_prover": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, u64p, C.c_size_t, u64p]),
    "halo_acc_verifier": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p]),
    "halo_acc_decider": (C.c_int, [C.c_void_p, u64p]),
    "halo_acc_decider_batch": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_int)]),
    "halo_acc_verifier_batch": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.POINTER(C.c_int)]),
    "halo_acc_prover_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, u64p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.POINTER(C.c_int)]),
    "halo_random_instance": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, u64p]),
    "halo_pcdl_open_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, u64p, C.c_size_t, u64p, u64p, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_random_instance_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_size_t, u64p]),
    "halo_pcdl_commit_batch": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, u64p, u64p]),
    "halo_pcdl_commit_dev_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_instance_from_poly": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), u64p, C.c_size_t, C.c_size_t, u64p, u64p, u64p]),
    "halo_instance_from_poly_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, u64p, C.c_size_t, u64p, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_poly_degrees_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_poly_eval_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, u64p, u64p]),
    "halo_instance_from_poly_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, C.c_size_t, u64p, u64p, u64p]),
    "halo_pcdl_open_dev_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, u64p, u64p,
                                           u64p, u64p, C.POINTER(C.c_int)]),
    "halo_instance_from_poly_dev_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                    u64p, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_proof_encoded_size": (C.c_size_t, [C.c_size_t, C.c_int]),
    "halo_instance_encoded_size": (C.c_size_t, [C.c_size_t, C.c_int]),
    "halo_accumulator_encoded_size": (C.c_size_t, [C.c_size_t]),
    "halo_proof_encode": (C.c_int, [u64p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_proof_decode": (C.c_int, [C.c_char_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_instance_encode": (C.c_int, [u64p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_instance_decode": (C.c_int, [C.c_char_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_accumulator_encode": (C.c_int, [u64p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_accumulator_decode": (C.c_int, [C.c_char_p, C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_proof_decode_batch": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "halo_instance_decode_batch": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "halo_accumulator_decode_batch": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "halo_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_prof_reset": (C.c_int, [C.c_void_p]),
    "halo_prof_count": (C.c_int, [C.c_void_p]),
    "halo_prof_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "halo_msm_dev_begin_part": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "halo_msm_dev_batch_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "halo_msm_dev_batch_end": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, u64p]),
    "halo_set_table_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_fold_table": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_ctx_info": (C.c_size_t, [C.c_void_p, C.c_int]),
    "halo_set_memory_budget": (C.c_int, [C.c_void_p, C.c_size_t]),
    "halo_point_sum": (C.c_int, [u64p, C.c_size_t, u64p]),
    "halo_rng_scalars_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_void_p]),
}

u32p = C.POINTER(C.c_uint32)

# libhalo_hip_dev.so (include/halo_accumulation_dev.h): experiment knobs, primitive test hooks, fault injectors.  Loaded only
# when one of these is called -- tests and tools/; the product path (pcdl.py, acc.py, sharded.py, bench.py's timed legs) never does.
_DEV_SIGS = {
    "halo_dev_hook": (C.c_int, [C.c_char_p, C.c_long]),
    "halo_dev_tuning": (C.c_long, [C.c_char_p]),
    "halo_set_batch_verify": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_bench_fr_kernel": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_int]),
    "halo_set_window_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_reduce_span": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_task_len": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_sort_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_small_path": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_fold_levels": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_fold_async": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_set_ipa_switch": (C.c_int, [C.c_void_p, C.c_size_t]),
    "halo_set_graphs": (C.c_int, [C.c_void_p, C.c_int]),
    "halo_test_glv_digits": (C.c_int, [u64p, C.POINTER(C.c_uint8), C.POINTER(C.c_int)]),
    "halo_test_fold_digits": (C.c_int, [u64p, C.POINTER(C.c_int8)]),
    "halo_test_field_op": (C.c_int, [C.c_void_p, C.c_int, C.c_int, u64p, u64p, C.c_size_t, u64p]),
    "halo_test_point_op": (C.c_int, [C.c_void_p, C.c_int, u64p, u64p, C.c_size_t, u64p]),
    "halo_dev_fr_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_long)]),
    "halo_dev_dot2_cross": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, u64p]),
    "halo_dev_h_coeffs_batch": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p]),
    "halo_dev_h_accumulate_batch": (C.c_int, [C.c_void_p, u64p, u64p, u64p, C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_size_t, u64p]),
    "halo_dev_check_weights": (C.c_int, [u64p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_char_p, u64p]),
    "halo_dev_check_combined_scalars": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, C.c_size_t, u64p]),
    "halo_dev_check_mixed_weights": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, C.c_char_p, u64p]),
    "halo_dev_check_mixed_scalars": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_size_t), u64p, C.c_size_t, u64p]),
    "halo_dev_check_fused_weights": (C.c_int, [u64p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_char_p, u64p]),
    "halo_dev_check_fused_terms": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_size_t, u64p, u64p]),
    "halo_dev_check_mixed_fused_weights": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, C.c_char_p, u64p]),
    "halo_dev_check_mixed_terms": (C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_size_t), C.c_size_t, u64p, u64p]),
    "halo_dev_small_msm_seg": (C.c_int, [C.c_void_p, u64p, u64p, C.POINTER(C.c_size_t), C.c_size_t, u64p]),
    "halo_dev_batch_small_msm": (C.c_int, [C.c_void_p, u64p, u64p, C.c_size_t, C.c_size_t, u64p]),
    "halo_dev_batch_to_affine": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p]),
    "halo_dev_transcripts": (C.c_int, [C.c_void_p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p, u64p, C.POINTER(C.c_int)]),
    "halo_dev_fq_sqrt": (C.c_int, [C.c_void_p, u64p, C.c_size_t, u64p, u32p]),
    "halo_dev_fold_points": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_int, u64p, C.c_int, C.c_int, u64p]),
    "halo_dev_fold_points_batch": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_int, u64p, C.c_int, C.c_int, C.c_int, u64p]),
    "halo_dev_msm_offsets": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t, u64p, C.c_int, C.c_int, u64p]),
    "halo_dev_msm_tagged": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, u64p, u64p]),
    "halo_dev_sqrt_tables": (C.c_int, [u32p, C.c_size_t]),
    "halo_dev_table_read": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, u64p]),
    "halo_dev_msm_last_plan": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_long)]),
    "halo_dev_msm_window_sums": (C.c_int, [C.c_void_p, C.c_int, u64p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "halo_test_lazy_field_op": (C.c_int, [C.c_void_p, C.c_int, u32p, C.c_size_t, u32p]),
    "halo_test_lazy_point_op": (C.c_int, [C.c_void_p, C.c_int, C.c_int, u32p, u32p, C.c_size_t, u32p]),
}


def dev_rows(dptrs, lens, who):
    """m device addresses and lengths as the C arrays of the entry points over device rows (0 / None: a null pointer)"""
    m = len(dptrs)
    if len(lens) != m:
        raise ValueError("%s: %d lengths for %d pointers" % (who, len(lens), m))
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(int(p or 0)) for p in dptrs])
    ln = (C.c_size_t * max(m, 1))(*[int(k) for k in lens])
    return ptrs, ln


def declared_symbols():
    return sorted(_SIGS)


def declared_dev_symbols():
    return sorted(_DEV_SIGS)


def load():
    """dlopen libhalo_hip.so; fails loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HaloError("libhalo_hip.so is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # One HIP runtime per process: PyTorch bundles its own libamdhip64.  If this library pulled in the
        # system copy first, torch would later load a second runtime and find no device ("No HIP GPUs are
        # available").  Importing torch first makes both resolve to the copy torch loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)  # (global: the development library resolves its internals against THIS copy)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = _Lib(lib)
    return _lib


class _Lib:
    """The product library; names of the development interface resolve to libhalo_hip_dev.so, loaded at their first use."""

    def __init__(self, product):
        self._product = product
        self._dev = None

    def dev(self):
        if self._dev is None:
            if not os.path.exists(DEV_LIB_PATH):
                raise HaloError("libhalo_hip_dev.so is missing: run __graft_entry__.build()")
            dev = C.CDLL(DEV_LIB_PATH)
            for name, (res, args) in _DEV_SIGS.items():
                fn = getattr(dev, name)
                fn.restype = res
                fn.argtypes = args
            self._dev = dev
        return self._dev

    def __getattr__(self, name):
        if name in _DEV_SIGS:
            return getattr(self.dev(), name)
        return getattr(self._product, name)


def dev_hook(name: str, value: int) -> None:
    """fault injectors / forced test paths of the development library (csrc/tuning.hpp DevHooks); "reset" switches all off"""
    check(load().halo_dev_hook(name.encode(), int(value)))


FR_PLAN_KERNELS = {"powers": 0, "poly_eval": 1, "dot": 2, "h_coeffs": 3, "poly_eval_batch": 4}


def fr_plan(which: str, n: int, ctx=None) -> dict:
    """The launch plan of one Fr kernel family at size n as its launcher computes it now (development hooks, environment, defaults;
    csrc/fr_plan.hpp): {"E", "nwin", "blocks", "trips"}.  which: powers / poly_eval / dot / h_coeffs (n = 2^lg_n) /
    poly_eval_batch (the p(z) of halo_pcdl_open_batch: at most 256 blocks per member).  Host only."""
    out = (C.c_long * 4)()
    check(load().halo_dev_fr_plan(None if ctx is None else ctx.h, FR_PLAN_KERNELS[which], int(n), out))
    return dict(zip(("E", "nwin", "blocks", "trips"), [int(v) for v in out]))


def ptr(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need contiguous uint64 array"
    return a.ctypes.data_as(u64p)


def check(rc: int) -> None:
    if rc == HALO_OK:
        return
    msg = load().halo_last_error().decode()
    if rc == HALO_E_ASSERT:
        raise AssertionError(msg)
    if rc == HALO_E_REJECT:
        raise HaloReject(msg)
    raise HaloError("%s (code %d)" % (msg, rc))


class Context:
    """A commitment key resident on one GPU (consts.rs: N, GS)."""

    def __init__(self, bases=None, *, urs_n: int | None = None, first_index: int = 2, stride: int = 1, device: int = 0, devices=None):
        """devices=[d0, d1, ...]: a multi-device context (halo_ctx_create_multi): full context on d0, one index-block shard per entry"""
        lib = load()
        h = C.c_void_p()
        if devices is not None:
            assert stride == 1, "multi-device contexts hold index blocks"
            if len(devices) == 0:
                raise HaloError("ctx_create_multi: 1..64 device ids")
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            device = int(devices[0])
            if bases is not None:
                bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
                check(lib.halo_ctx_create_multi(devs, len(devices), ptr(bases), bases.shape[0], C.byref(h)))
            else:
                check(lib.halo_ctx_create_urs_multi(devs, len(devices), first_index, int(urs_n), C.byref(h)))
        elif bases is not None:
            bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
            check(lib.halo_ctx_create(device, ptr(bases), bases.shape[0], C.byref(h)))
        elif stride != 1:
            check(lib.halo_ctx_create_urs_strided(device, first_index, stride, int(urs_n), C.byref(h)))
        else:
            check(lib.halo_ctx_create_urs(device, first_index, int(urs_n), C.byref(h)))
        self.h = h
        self.lib = lib
        self.device = device
        self._children = []  # weak references to the Ipa states of this context: they must go before it

    def clone(self):
        """a second context over the same resident key and tables (halo_ctx_clone): one per host thread"""
        h = C.c_void_p()
        check(self.lib.halo_ctx_clone(self.h, C.byref(h)))
        other = Context.__new__(Context)
        other.h, other.lib, other.device, other._children = h, self.lib, self.device, []
        return other

    def close(self):
        if getattr(self, "h", None):
            for ref in self._children:
                child = ref()
                if child is not None:
                    child.close()
            self._children = []
            self.lib.halo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        return self.lib.halo_ctx_size(self.h)

    @property
    def n_devices(self) -> int:
        return self.lib.halo_ctx_devices(self.h)

    def read_bases(self, off=0, n=None):
        n = self.size - off if n is None else n
        out = np.zeros((n, 8), dtype=np.uint64)
        check(self.lib.halo_ctx_read_bases(self.h, off, n, ptr(out)))
        return out

    # ---- group.rs
    def msm(self, scalars, off=0, mont=True):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm(self.h, off, scalars.shape[0], ptr(scalars), int(mont), ptr(out)))
        return out

    def msm_begin(self, slot: int, scalars, off=0, mont=True):
        """host scalars, asynchronous: copy + launch on `slot`; msm_end(slot) collects"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        check(self.lib.halo_msm_begin(self.h, slot, off, scalars.shape[0], ptr(scalars), int(mont)))

    def msm_end(self, slot: int):
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm_end(self.h, slot, ptr(out)))
        return out

    def msm_dev(self, dptr: int, n: int, off=0, mont=True):
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm_dev(self.h, off, n, C.c_void_p(dptr), int(mont), ptr(out)))
        return out

    def msm_dev_begin(self, slot: int, dptr: int, n: int, off=0, mont=True, part=0, parts=1):
        """parts > 1: only window shard `part` of `parts` (the partial results of all parts sum to the MSM)"""
        if parts == 1:
            check(self.lib.halo_msm_dev_begin(self.h, slot, off, n, C.c_void_p(dptr), int(mont)))
        else:
            check(self.lib.halo_msm_dev_begin_part(self.h, slot, off, n, C.c_void_p(dptr), int(mont), part, parts))

    def msm_dev_end(self, slot: int):
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm_dev_end(self.h, slot, ptr(out)))
        return out

    def msm_dev_batch_begin(self, slot: int, dptrs, n: int, off=0, mont=True, part=0, parts=1):
        """len(dptrs) (1..8) MSMs over the same bases, one resident scalar array each, as one launch sequence;
        parts > 1: window shard `part` of each"""
        arr = (C.c_void_p * len(dptrs))(*[C.c_void_p(int(p)) for p in dptrs])
        check(self.lib.halo_msm_dev_batch_begin(self.h, slot, off, n, arr, len(dptrs), int(mont), part, parts))

    def msm_dev_batch_end(self, slot: int, batch: int):
        out = np.zeros((batch, 12), dtype=np.uint64)
        check(self.lib.halo_msm_dev_batch_end(self.h, slot, batch, ptr(out)))
        return out

    # ---- group.rs sharded over one process per GPU: this rank's share, one all-gather (halo_msm_sharded and its forms).
    # allgather: None (world 1, no collective), an object with .fn / .user (rccl.RcclGather: passed as it is) or a Python
    # callable arr -> (world, len) uint64, whose exception is raised here after the call.
    def msm_sharded(self, scalars, world: int, rank: int, allgather, off=0, mont=True):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(12, dtype=np.uint64)
        cb, fn, user = allgather_args(allgather, world)
        rc = self.lib.halo_msm_sharded(self.h, world, rank, off, scalars.shape[0], ptr(scalars), int(mont), fn, user, ptr(out))
        _raise_callback(cb)
        check(rc)
        return out

    def msm_dev_sharded(self, dptr: int, n: int, world: int, rank: int, allgather, off=0, mont=True):
        out = np.zeros(12, dtype=np.uint64)
        cb, fn, user = allgather_args(allgather, world)
        rc = self.lib.halo_msm_dev_sharded(self.h, world, rank, off, n, C.c_void_p(dptr), int(mont), fn, user, ptr(out))
        _raise_callback(cb)
        check(rc)
        return out

    def msm_end_sharded(self, slot: int, batch: int, world: int, rank: int, allgather):
        """collect what `slot` holds (any msm*_begin; batch = its member count) and sum it across ranks -> (batch, 12)"""
        out = np.zeros((batch, 12), dtype=np.uint64)
        cb, fn, user = allgather_args(allgather, world)
        rc = self.lib.halo_msm_end_sharded(self.h, slot, batch, world, rank, fn, user, ptr(out))
        _raise_callback(cb)
        check(rc)
        return out

    def msm_points(self, pts_jac, scalars):
        pts_jac = np.ascontiguousarray(pts_jac, dtype=np.uint64).reshape(-1, 12)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        m = min(len(pts_jac), len(scalars))  # msm_unchecked zips to the shorter input
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm_points(self.h, ptr(pts_jac), ptr(scalars), m, ptr(out)))
        return out

    def msm_affine(self, bases_affine, scalars, mont=True):
        """point_dot_affine over bases that are not part of the context's key (uploaded for this call)"""
        bases_affine = np.ascontiguousarray(bases_affine, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        m = min(len(bases_affine), len(scalars))  # msm_unchecked zips to the shorter input
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_msm_affine(self.h, ptr(bases_affine), ptr(scalars), m, int(mont), ptr(out)))
        return out

    def scalar_dot(self, xs, ys):
        xs = np.ascontiguousarray(xs, dtype=np.uint64).reshape(-1, 4)
        ys = np.ascontiguousarray(ys, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(4, dtype=np.uint64)
        check(self.lib.halo_scalar_dot(self.h, ptr(xs), ptr(ys), min(len(xs), len(ys)), ptr(out)))
        return out

    def powers(self, z, n):
        out = np.zeros((n, 4), dtype=np.uint64)
        check(self.lib.halo_powers(self.h, ptr(np.ascontiguousarray(z, dtype=np.uint64)), n, ptr(out)))
        return out

    def poly_eval(self, coeffs, z):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(4, dtype=np.uint64)
        check(self.lib.halo_poly_eval(self.h, ptr(coeffs), coeffs.shape[0], ptr(np.ascontiguousarray(z, dtype=np.uint64)), ptr(out)))
        return out

    def poly_eval_dev(self, dptr, length, z):
        """p(z) for `length` coefficients resident in device memory (halo_poly_eval_dev)"""
        out = np.zeros(4, dtype=np.uint64)
        check(self.lib.halo_poly_eval_dev(self.h, C.c_void_p(int(dptr)), length, ptr(np.ascontiguousarray(z, dtype=np.uint64)), ptr(out)))
        return out

    def poly_degrees_dev(self, dptrs, lens):
        """the degrees of m device-resident rows, found on the device (halo_poly_degrees_dev) -> list of m ints"""
        ptrs, ln = dev_rows(dptrs, lens, "poly_degrees_dev")
        m = len(dptrs)
        out = (C.c_size_t * max(m, 1))()
        check(self.lib.halo_poly_degrees_dev(self.h, ptrs, ln, m, out))
        return [int(out[i]) for i in range(m)]

    # ---- h(X)
    def h_coeffs(self, xis):
        xis = np.ascontiguousarray(xis, dtype=np.uint64).reshape(-1, 4)
        lg = xis.shape[0] - 1
        out = np.zeros((1 << lg, 4), dtype=np.uint64)
        check(self.lib.halo_h_coeffs(self.h, ptr(xis), lg, ptr(out)))
        return out

    def h_commit(self, xis):
        xis = np.ascontiguousarray(xis, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(12, dtype=np.uint64)
        check(self.lib.halo_h_commit(self.h, ptr(xis), xis.shape[0] - 1, ptr(out)))
        return out

    def h_eval_batch(self, xis, z):
        xis = np.ascontiguousarray(xis, dtype=np.uint64)
        m, lg1 = xis.shape[0], xis.shape[1]
        out = np.zeros((m, 4), dtype=np.uint64)
        check(self.lib.halo_h_eval_batch(self.h, ptr(xis), m, lg1 - 1, ptr(np.ascontiguousarray(z, dtype=np.uint64)), ptr(out)))
        return out

    def h_accumulate(self, h0, xis, alphas, out=None):
        """out: an (n, 4) uint64 array to write into (a caller that keeps its buffer: no fresh pages for the driver to pin)"""
        xis = np.ascontiguousarray(xis, dtype=np.uint64)
        m, lg1 = xis.shape[0], xis.shape[1]
        if out is None:
            out = np.empty((1 << (lg1 - 1), 4), dtype=np.uint64)
        assert out.shape == (1 << (lg1 - 1), 4) and out.dtype == np.uint64 and out.flags["C_CONTIGUOUS"]
        h0 = None if h0 is None else np.ascontiguousarray(h0, dtype=np.uint64)
        check(self.lib.halo_h_accumulate(self.h, ptr(h0), ptr(xis), ptr(np.ascontiguousarray(alphas, dtype=np.uint64)), m, lg1 - 1, ptr(out)))
        return out

    # ---- measurement
    def prof_enable(self, on=1):
        """1: every launch; 2: dominant kernels only; 0: off"""
        check(self.lib.halo_prof_enable(self.h, int(on)))

    def prof_reset(self):
        check(self.lib.halo_prof_reset(self.h))

    def prof(self):
        out = {}
        for i in range(self.lib.halo_prof_count(self.h)):
            name, ms, cnt = C.c_char_p(), C.c_double(), C.c_long()
            check(self.lib.halo_prof_get(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt)))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

    def bench_fr_kernel(self, which: int, n: int, reps: int):
        """reps back-to-back launches of one Fr kernel (0 powers, 1 poly_eval, 2 dot, 3 dot2 of a round, 4 h_coeffs, 5 fold_scalars, 6 axpy)"""
        check(self.lib.halo_bench_fr_kernel(self.h, which, n, reps))

    def rng_scalars_dev(self, state: int, n: int, dptr: int) -> int:
        """Fill device memory with n scalars of the SplitMix64 stream; returns the advanced state."""
        st = C.c_uint64(state)
        check(self.lib.halo_rng_scalars_dev(self.h, C.byref(st), n, C.c_void_p(dptr)))
        return st.value

    def set_graphs(self, on: bool):
        check(self.lib.halo_set_graphs(self.h, int(on)))

    def set_ipa_switch(self, size):
        check(self.lib.halo_set_ipa_switch(self.h, size))

    def set_window_bits(self, c):
        check(self.lib.halo_set_window_bits(self.h, c))

    def set_reduce_span(self, span):
        check(self.lib.halo_set_reduce_span(self.h, span))

    def set_sort_mode(self, mode):
        check(self.lib.halo_set_sort_mode(self.h, mode))

    def set_batch_verify(self, on):
        check(self.lib.halo_set_batch_verify(self.h, int(on)))

    def set_fold_levels(self, levels):
        check(self.lib.halo_set_fold_levels(self.h, levels))

    def set_fold_async(self, mode):
        """-1 automatic (opens of <= 2^18 points), 0 never, 1 wherever possible"""
        check(self.lib.halo_set_fold_async(self.h, int(mode)))

    def set_fold_table(self, mode):
        check(self.lib.halo_set_fold_table(self.h, mode))

    def info(self, what: int) -> int:
        """0: MSM table bytes, 1: fold table bytes, 2: fold table build time in microseconds, ..., 10: members of the last open-type
        batch call that ran through member-batched launches (halo_ctx_info)"""
        return self.lib.halo_ctx_info(self.h, what)

    def set_memory_budget(self, nbytes: int):
        """budget for optional table memory on this context's device, process-wide (halo_set_memory_budget)"""
        check(self.lib.halo_set_memory_budget(self.h, int(nbytes)))

    def set_table_mode(self, mode):
        check(self.lib.halo_set_table_mode(self.h, mode))

    def set_small_path(self, mode):
        check(self.lib.halo_set_small_path(self.h, mode))

    def set_task_len(self, n):
        check(self.lib.halo_set_task_len(self.h, n))

    # ---- primitive hooks
    def field_op(self, field, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros_like(a)
        check(self.lib.halo_test_field_op(self.h, field, op, ptr(a), ptr(b), a.shape[0], ptr(out)))
        return out

    def point_op(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 12)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros_like(a)
        check(self.lib.halo_test_point_op(self.h, op, ptr(a), ptr(b), a.shape[0], ptr(out)))
        return out

    # ---- raw-limb hooks (csrc/dev_lazy_ops.hpp): native operands whose limbs the caller chooses
    def fold_points(self, key, levels, scalars, form=0, in_place=False, n=None):
        """halo_dev_fold_points: one point fold over `key` (n x 8 words; None: the first n points of the context's own key) in the
        kernel form `form` -> m x 8 affine words"""
        if key is not None:
            key = np.ascontiguousarray(key, dtype=np.uint64).reshape(-1, 8)
            n = key.shape[0]
        n = self.size if n is None else int(n)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert scalars.shape[0] == (3 if levels == 2 else 1)
        out = np.zeros((max(n // (4 if levels == 2 else 2), 1), 8), dtype=np.uint64)
        check(self.lib.halo_dev_fold_points(self.h, ptr(key), n, int(levels), ptr(scalars), int(form), int(bool(in_place)), ptr(out)))
        return out

    def fold_points_batch(self, key, levels, scalars, members, shared=True, form=0, n=None):
        """halo_dev_fold_points_batch: `members` folds in one launch.  key: None (the first n points of the context's key, shared), n x 8
        words (one key for all, shared) or members x n x 8 words (shared=False: folded in place); scalars: members x (1 | 3) x 4 words
        -> members x m x 8 affine words"""
        if key is not None:
            key = np.ascontiguousarray(key, dtype=np.uint64).reshape(-1, 8)
            n = key.shape[0] // (1 if shared else members)
        n = self.size if n is None else int(n)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert scalars.shape[0] == members * (3 if levels == 2 else 1)
        out = np.zeros((members, max(n // (4 if levels == 2 else 2), 1), 8), dtype=np.uint64)
        check(self.lib.halo_dev_fold_points_batch(self.h, ptr(key), n, int(levels), ptr(scalars), int(members), int(bool(shared)), int(form), ptr(out)))
        return out

    def msm_offsets(self, offs, n, scalars, mont=False):
        """halo_dev_msm_offsets: len(offs) MSMs of n points as ONE batched launch sequence, member b over the key's points
        [offs[b], offs[b] + n) with scalars[b] -> len(offs) x 12 Jacobian words (normalised, as halo_msm's)"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(len(offs), int(n), 4)
        co = (C.c_size_t * len(offs))(*[int(o) for o in offs])
        out = np.zeros((len(offs), 12), dtype=np.uint64)
        check(self.lib.halo_dev_msm_offsets(self.h, co, int(n), ptr(scalars), len(offs), int(bool(mont)), ptr(out)))
        return out

    def msm_tagged(self, scalars, off=0):
        """halo_dev_msm_tagged: ONE tagged launch over the key's points [off, off + len(scalars)): scalars = n x 4 canonical words,
        bit 255 of scalar i names its bucket set -> 2 x 12 Jacobian words (normalised), the sum of each set"""
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((2, 12), dtype=np.uint64)
        check(self.lib.halo_dev_msm_tagged(self.h, int(off), scalars.shape[0], ptr(scalars), ptr(out)))
        return out

    def table_read(self, row, off=0, n=None):
        """halo_dev_table_read: entries [off, off + n) of row `row` of the MSM table -> n x 8 affine words, as read_bases gives the key"""
        n = self.size - off if n is None else n
        out = np.zeros((n, 8), dtype=np.uint64)
        check(self.lib.halo_dev_table_read(self.h, int(row), int(off), int(n), ptr(out)))
        return out

    MSM_PLAN_FIELDS = ("pipeline", "c", "W", "B", "members", "sets", "pieces", "kmax", "form", "L", "logL", "nseg", "live_seg")

    def msm_last_plan(self, slot=0) -> dict:
        """halo_dev_msm_last_plan: the plan of the launch enqueued last on `slot`, as its launch sequence noted it.  pipeline: 0 general,
        1 small, 2 table with fixed windows, 3 table sliding; form: 0 k_msm_reduce1 + k_smsm_final, 1 k_smsm_reduce, 2 k_msm_reduce_rc +
        k_rc_mid (then lg_rows, lg_cols, per; else 0).  Host only."""
        out = (C.c_long * 16)()
        check(self.lib.halo_dev_msm_last_plan(self.h, int(slot), out))
        d = dict(zip(self.MSM_PLAN_FIELDS, [int(v) for v in out]))
        rc = int(out[13])
        d.update(lg_rows=rc & 255, lg_cols=(rc >> 8) & 255, per=rc >> 16)
        return d

    def msm_window_sums(self, slot=0, cap=None):
        """halo_dev_msm_window_sums: the records the slot's last finished launch left for the host's combination -> (count, 12)
        Jacobian words (layout per form: include/halo_accumulation_dev.h).  cap: room offered, in points (None: what it takes)."""
        cnt = C.c_size_t(0)
        if cap is None:
            rc = self.lib.halo_dev_msm_window_sums(self.h, int(slot), None, 0, C.byref(cnt))  # (refused for its room: tells the count)
            if rc != HALO_E_ARG or (cnt.value == 0 and b"null pointer" not in self.lib.halo_last_error()):
                check(rc)  # (a bad slot, a slot in flight, no launch: that message, at once)
            cap = cnt.value
        out = np.zeros((max(int(cap), 1), 12), dtype=np.uint64)
        check(self.lib.halo_dev_msm_window_sums(self.h, int(slot), ptr(out), int(cap), C.byref(cnt)))
        return out[:cnt.value]

    def batch_to_affine(self, pts_jac):
        """halo_dev_batch_to_affine: m x 12 Jacobian words through the product's batch_to_affine -> m x 8 affine words"""
        pts_jac = np.ascontiguousarray(pts_jac, dtype=np.uint64).reshape(-1, 12)
        out = np.zeros((pts_jac.shape[0], 8), dtype=np.uint64)
        check(self.lib.halo_dev_batch_to_affine(self.h, ptr(pts_jac), pts_jac.shape[0], ptr(out)))
        return out

    def transcripts(self, d, instances, on_device):
        """halo_dev_transcripts: the succinct check's transcripts of m Instance blobs of degree bound d on the host pool or through
        the device route -> (xis m x (lg + 1) x 4, C' m x 12 normalised, status m: 0 ok, 1 instance, 2 proof, 3 zero challenge,
        4 header)"""
        lg = (int(d) + 1).bit_length() - 1
        instances = np.ascontiguousarray(instances, dtype=np.uint64).reshape(-1, 21 + 2 + 24 * lg + 32)
        m = instances.shape[0]
        xis, cp = np.zeros((m, lg + 1, 4), dtype=np.uint64), np.zeros((m, 12), dtype=np.uint64)
        st = (C.c_int * max(m, 1))()
        check(self.lib.halo_dev_transcripts(self.h, int(d), ptr(instances), m, int(bool(on_device)), ptr(xis), ptr(cp), st))
        return xis, cp, np.array(list(st)[:m], dtype=np.int64)

    def batch_small_msm(self, points, scalars, K):
        """halo_dev_batch_small_msm: m sums of K terms (m K x 8 affine words, m K x 4 canonical scalar words) in one
        k_batch_small_msm launch -> m x 12 Jacobian words"""
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert points.shape[0] == scalars.shape[0] and points.shape[0] % K == 0
        m = points.shape[0] // K
        out = np.zeros((m, 12), dtype=np.uint64)
        check(self.lib.halo_dev_batch_small_msm(self.h, ptr(points), ptr(scalars), m, int(K), ptr(out)))
        return out

    def dot2_cross(self, c, z):
        """the two dot products of an IPA round over c, z of 2 m elements, any m (halo_dev_dot2_cross): <c_hi, z_lo>, <c_lo, z_hi>"""
        c = np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4)
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        assert len(c) == len(z) and len(c) % 2 == 0
        out = np.zeros((2, 4), dtype=np.uint64)
        check(self.lib.halo_dev_dot2_cross(self.h, ptr(c), ptr(z), len(c) // 2, ptr(out)))
        return out[0], out[1]

    def small_msm_seg(self, points, scalars, lens):
        """halo_dev_small_msm_seg: sums of lens[s] terms each, the terms sum after sum, in one k_small_msm_seg launch -> len(lens) x 12"""
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        assert points.shape[0] == scalars.shape[0] == sum(lens)
        out = np.zeros((len(lens), 12), dtype=np.uint64)
        cl = (C.c_size_t * len(lens))(*[int(x) for x in lens])
        check(self.lib.halo_dev_small_msm_seg(self.h, ptr(points), ptr(scalars), cl, len(lens), ptr(out)))
        return out

    def lazy_field_op(self, op, a):
        """a: (n, 40) uint32, four operands of 9 limbs + pad -> (n, 10) uint32"""
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 40)
        out = np.zeros((a.shape[0], 10), dtype=np.uint32)
        check(self.lib.halo_test_lazy_field_op(self.h, op, a.ctypes.data_as(u32p), a.shape[0], out.ctypes.data_as(u32p)))
        return out

    def lazy_point_op(self, op, a, b, quad=False):
        """a, b: (n, 40) uint32 native points -> (n, 40) uint32; quad: the quad-parallel form of curve_quad.hpp"""
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 40)
        b = np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, 40)
        assert a.shape == b.shape
        out = np.zeros_like(a)
        check(self.lib.halo_test_lazy_point_op(self.h, op, int(quad), a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), a.shape[0], out.ctypes.data_as(u32p)))
        return out


class Ipa:
    """Device-resident state of pcdl::open's halving loop (pcdl.rs:183-231)."""

    def __init__(self, ctx: Context, n: int, coeffs, z, *, stride: int = 1, offset: int = 0, z_vec=None):
        """Default: c = coeffs zero-padded, z-vector = powers of z.  stride/offset: the cyclic shard
        z^(offset + j*stride).  z_vec: explicit vectors (coeffs and z_vec both of length n)."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        h = C.c_void_p()
        if z_vec is not None:
            z_vec = np.ascontiguousarray(z_vec, dtype=np.uint64).reshape(-1, 4)
            assert coeffs.shape[0] == n == z_vec.shape[0]
            check(ctx.lib.halo_ipa_begin_vectors(ctx.h, n, ptr(coeffs), ptr(z_vec), C.byref(h)))
        elif stride != 1 or offset != 0:
            check(ctx.lib.halo_ipa_begin_strided(ctx.h, n, ptr(coeffs), coeffs.shape[0], ptr(np.ascontiguousarray(z, dtype=np.uint64)),
                                                 stride, offset, C.byref(h)))
        else:
            check(ctx.lib.halo_ipa_begin(ctx.h, n, ptr(coeffs), coeffs.shape[0], ptr(np.ascontiguousarray(z, dtype=np.uint64)), C.byref(h)))
        self.h, self.ctx = h, ctx
        import weakref
        ctx._children.append(weakref.ref(self))

    def dot_cz(self):
        out = np.zeros(4, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_dot_cz(self.h, ptr(out)))
        return out

    def round_lr_partial(self):
        """-> one record L 12 | R 12 | dot_l 4 | dot_r 4 (no H' terms)"""
        rec = np.zeros(32, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_round_lr_partial(self.h, ptr(rec[:12]), ptr(rec[12:24]), ptr(rec[24:])))
        return rec

    def hiding_partial(self, rng_state: int, deg: int, z, stride: int, offset: int):
        out = np.zeros(12, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_hiding_partial(self.h, rng_state, deg, ptr(np.ascontiguousarray(z, dtype=np.uint64)), stride, offset, ptr(out)))
        return out

    def apply_hiding(self, alpha):
        check(self.ctx.lib.halo_ipa_apply_hiding(self.h, ptr(np.ascontiguousarray(alpha, dtype=np.uint64))))

    def finish_z(self):
        U, c, z0 = np.zeros(12, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_finish_z(self.h, ptr(U), ptr(c), ptr(z0)))
        return U, c, z0

    def round_lr(self, H_prime):
        L, R = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_round_lr(self.h, ptr(np.ascontiguousarray(H_prime, dtype=np.uint64)), ptr(L), ptr(R)))
        return L, R

    def round_fold(self, xi, xi_inv):
        check(self.ctx.lib.halo_ipa_round_fold(self.h, ptr(np.ascontiguousarray(xi, dtype=np.uint64)), ptr(np.ascontiguousarray(xi_inv, dtype=np.uint64))))

    def finish(self):
        U, c = np.zeros(12, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        check(self.ctx.lib.halo_ipa_finish(self.h, ptr(U), ptr(c)))
        return U, c

    def __len__(self):
        return self.ctx.lib.halo_ipa_len(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.halo_ipa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def open_start(Cm, z, v_parts):
    """v = sum of the shards' <c, z>; xi_0 = rho_0(C, z, v); H' = xi_0 H"""
    v_parts = np.ascontiguousarray(v_parts, dtype=np.uint64).reshape(-1, 4)
    v, xi, Hp = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    check(load().halo_open_start(ptr(np.ascontiguousarray(Cm, dtype=np.uint64)), ptr(np.ascontiguousarray(z, dtype=np.uint64)), ptr(v_parts),
                                 v_parts.shape[0], ptr(v), ptr(xi), ptr(Hp)))
    return v, xi, Hp


def open_hiding_combine(Cm, z, v_parts, cbar_parts, w, rng_state: int, deg: int):
    """-> C_bar, alpha, w', C', advanced rng state"""
    v_parts = np.ascontiguousarray(v_parts, dtype=np.uint64).reshape(-1, 4)
    cbar_parts = np.ascontiguousarray(cbar_parts, dtype=np.uint64).reshape(-1, 12)
    st = C.c_uint64(rng_state)
    Cbar, alpha, wp, Cp = (np.zeros(12, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64),
                           np.zeros(12, dtype=np.uint64))
    check(load().halo_open_hiding_combine(ptr(np.ascontiguousarray(Cm, dtype=np.uint64)), ptr(np.ascontiguousarray(z, dtype=np.uint64)),
                                          ptr(v_parts), ptr(cbar_parts), v_parts.shape[0], ptr(np.ascontiguousarray(w, dtype=np.uint64)),
                                          C.byref(st), deg, ptr(Cbar), ptr(alpha), ptr(wp), ptr(Cp)))
    return Cbar, alpha, wp, Cp, st.value


def open_combine(parts, Hp, xi_prev):
    """parts (P, 32) in rank order -> L, R, xi_next, xi_next^-1"""
    parts = np.ascontiguousarray(parts, dtype=np.uint64).reshape(-1, 32)
    L, R = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    xi, xi_inv = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    check(load().halo_open_combine(ptr(parts), parts.shape[0], ptr(np.ascontiguousarray(Hp, dtype=np.uint64)),
                                   ptr(np.ascontiguousarray(xi_prev, dtype=np.uint64)), ptr(L), ptr(R), ptr(xi), ptr(xi_inv)))
    return L, R, xi, xi_inv


# the caller's all-gather as the library calls it (include/halo_accumulation.h halo_allgather_fn)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64))


def make_allgather_callback(allgather, world: int):
    """allgather(arr) -> (P, len) uint64 wrapped for halo_pcdl_open_sharded / _check_sharded; keep the returned object alive
    for the duration of the call.  An exception inside the collective is kept in cb.error and reported as a failure."""
    def _cb(_user, send, words, recv):
        try:
            a = np.ctypeslib.as_array(send, shape=(words,)).copy()
            out = np.ascontiguousarray(allgather(a), dtype=np.uint64).reshape(-1)
            assert out.size == world * words
            np.ctypeslib.as_array(recv, shape=(world * words,))[:] = out
            return 0
        except Exception as e:  # noqa: BLE001 -- must not unwind through the C frame
            cb.error = e
            return 1
    cb = ALLGATHER_FN(_cb)
    cb.error = None
    return cb


def allgather_args(allgather, world: int):
    """-> (object to keep alive, function pointer, user pointer) for the sharded entry points.  An all-gather that brings its own
    C entry point (rccl.RcclGather: .fn = halo_allgather_rccl, .user = its handle) is passed as it is -- no Python frame in the
    collective path; a Python callable is wrapped (make_allgather_callback); None stays None (one rank, no collective)."""
    if allgather is None:
        return None, None, None
    if hasattr(allgather, "fn") and hasattr(allgather, "user"):
        return None, allgather.fn, allgather.user
    cb = make_allgather_callback(allgather, world)
    return cb, C.cast(cb, C.c_void_p), None


def _raise_callback(cb):
    if cb is not None and cb.error is not None:
        raise cb.error


def open_tail(recs, Hp, xi_prev):
    """recs (P, 20): the gathered (G_i | c_i | z_i) in index order -> (Ls (lg P, 12), Rs (lg P, 12), U, c): the last lg P rounds on the host"""
    recs = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 20)
    P = recs.shape[0]
    lg = max(P.bit_length() - 1, 0)
    Ls, Rs = np.zeros((max(lg, 1), 12), dtype=np.uint64), np.zeros((max(lg, 1), 12), dtype=np.uint64)
    U, c = np.zeros(12, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    check(load().halo_open_tail(ptr(recs), P, ptr(np.ascontiguousarray(Hp, dtype=np.uint64)), ptr(np.ascontiguousarray(xi_prev, dtype=np.uint64)),
                                ptr(Ls), ptr(Rs), ptr(U), ptr(c)))
    return Ls[:lg], Rs[:lg], U, c


def _encode(fn, blob, cap):
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    buf = C.create_string_buffer(cap)
    n = C.c_size_t()
    check(fn(ptr(blob), buf, cap, C.byref(n)))
    return buf.raw[: n.value]


def _decode(fn, data, words_of_lg):
    data = bytes(data)
    out = np.zeros(words_of_lg(40), dtype=np.uint64)
    lg = C.c_size_t()
    check(fn(data, len(data), ptr(out), out.shape[0], C.byref(lg)))
    return out[: words_of_lg(lg.value)].copy()


def proof_encode(proof):
    """EvalProof blob -> bytes (ark-serialize compressed layout of pcdl.rs:22-30)"""
    lib = load()
    return _encode(lib.halo_proof_encode, proof, lib.halo_proof_encoded_size(int(proof[1]), 1))


def proof_decode(data):
    lib = load()
    return _decode(lib.halo_proof_decode, data, lib.halo_proof_words)


def instance_encode(inst):
    lib = load()
    return _encode(lib.halo_instance_encode, inst, lib.halo_instance_encoded_size(int(inst[22]), 1))


def instance_decode(data):
    lib = load()
    return _decode(lib.halo_instance_decode, data, lib.halo_instance_words)


def accumulator_encode(acc):
    lib = load()
    return _encode(lib.halo_accumulator_encode, acc, lib.halo_accumulator_encoded_size(int(acc[22])))


def accumulator_decode(data):
    lib = load()
    return _decode(lib.halo_accumulator_decode, data, lib.halo_accumulator_words)


def _decode_batch(name, datas, words_of_lg, ctx, stride_words):
    """m byte strings -> (blobs (m, stride), lgs, statuses); a member that fails has its code in statuses and a zero row"""
    lib = load()
    datas = [bytes(d) for d in datas]
    m = len(datas)
    offs = (C.c_size_t * (m + 1))()
    for i, d in enumerate(datas):
        offs[i + 1] = offs[i] + len(d)
    if stride_words is None:  # the largest lg any member's length allows (33 bytes per L and per R)
        stride_words = words_of_lg(min(40, max([len(d) // 66 for d in datas], default=0)))
    out = np.zeros((m, int(stride_words)), dtype=np.uint64)
    lgs, st = (C.c_size_t * max(m, 1))(), (C.c_int * max(m, 1))()
    rc = getattr(lib, name)(ctx.h if ctx is not None else None, b"".join(datas), offs, m, ptr(out), int(stride_words), lgs, st)
    if rc != HALO_OK and not any(st[i] for i in range(m)):
        check(rc)  # a whole-call error
    return out, np.array(lgs[:m], dtype=np.int64), np.array(st[:m], dtype=np.int32)


def proof_decode_batch(datas, ctx=None, stride_words=None):
    """halo_proof_decode_batch: (blobs[m, stride], lgs, statuses); member failures are reported in statuses, not raised"""
    return _decode_batch("halo_proof_decode_batch", datas, load().halo_proof_words, ctx, stride_words)


def instance_decode_batch(datas, ctx=None, stride_words=None):
    return _decode_batch("halo_instance_decode_batch", datas, load().halo_instance_words, ctx, stride_words)


def accumulator_decode_batch(datas, ctx=None, stride_words=None):
    return _decode_batch("halo_accumulator_decode_batch", datas, load().halo_accumulator_words, ctx, stride_words)


def point_sum(pts_jac):
    """Sum of Jacobian points in index order (host): the combine step of the sharded MSM."""
    pts_jac = np.ascontiguousarray(pts_jac, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    check(load().halo_point_sum(ptr(pts_jac), pts_jac.shape[0], ptr(out)))
    return out


def public_points():
    S, H = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    check(load().halo_public_points(ptr(S), ptr(H)))
    return S, H
