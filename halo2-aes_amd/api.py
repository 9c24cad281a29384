"""ctypes binding of include/aesw.h plus a thin tensor-level wrapper.

PyTorch is plumbing only: device memory (``torch.empty(..., device="cuda")``),
the current HIP stream and ``torch.distributed``.  All compute happens in
``libaesw.so`` (hand-written gfx950 kernels) through the C ABI; if the library
is missing or no gfx950 device is usable this module raises -- there is no
fallback path.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from pathlib import Path

import numpy as np

from . import constants as K

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libaesw.so"            # HIP kernels + the C ABI of include/aesw.h
HOST_LIB_PATH = _PKG / "libaesw_host.so"  # C++ mirror of the reference's host interface (include/aesw_host.h), above the C ABI
CIRC_LIB_PATH = _PKG / "libaesw_circ.so"  # the many-circuit witness checker (include/aesw_circ.h): one more kernel, next to libaesw.so
COLS_LIB_PATH = _PKG / "libaesw_cols.so"  # the checker of the assembled advice columns (include/aesw_cols.h), next to libaesw.so
VALS_LIB_PATH = _PKG / "libaesw_vals.so"  # the checker of a VALUES witness (include/aesw_vals.h), next to libaesw.so
ACC_LIB_PATH = _PKG / "libaesw_acc.so"    # the lookup multiplicities of one circuit, accumulated chunk by chunk (include/aesw_acc.h)
PERM_LIB_PATH = _PKG / "libaesw_perm.so"  # plookup's permuted columns arranged from the multiplicities (include/aesw_perm.h)
VACC_LIB_PATH = _PKG / "libaesw_vacc.so"  # the same accumulated from a VALUES witness (include/aesw_vacc.h)
MULT_LIB_PATH = _PKG / "libaesw_mult.so"  # the lookup multiplicities of a many-circuit batch (include/aesw_mult.h), next to libaesw.so
THETA_LIB_PATH = _PKG / "libaesw_theta.so"  # the lookup arguments compressed under theta (include/aesw_theta.h)
GRAND_LIB_PATH = _PKG / "libaesw_grand.so"  # the grand product Z of every lookup argument from beta and gamma (include/aesw_grand.h)
SIGMA_LIB_PATH = _PKG / "libaesw_sigma.so"  # the grand products of the permutation argument from beta and gamma (include/aesw_sigma.h)
NTT_LIB_PATH = _PKG / "libaesw_ntt.so"  # columns of Fr cells between Lagrange, coefficient and extended-coset form (include/aesw_ntt.h)
QUOT_LIB_PATH = _PKG / "libaesw_quot.so"  # sigma of the permutation argument as Fr columns, for the quotient h(X) (include/aesw_quot.h)
OPEN_LIB_PATH = _PKG / "libaesw_open.so"  # coefficient columns evaluated at points, folded under v and divided by (X - z) (include/aesw_open.h)
MSM_LIB_PATH = _PKG / "libaesw_msm.so"  # columns of cells or bytes committed against a basis of points of bn256's G1 (include/aesw_msm.h)
TRANSCRIPT_LIB_PATH = _PKG / "libaesw_transcript.so"  # the Blake2b transcript: challenges from commitments, and the proof bytes (include/aesw_transcript.h)
SHPLONK_LIB_PATH = _PKG / "libaesw_shplonk.so"  # SHPLONK's two quotients over every queried column (include/aesw_shplonk.h)
VANISH_LIB_PATH = _PKG / "libaesw_vanish.so"  # the quotient h(X) folded one constraint segment per call (include/aesw_vanish.h)
BLIND_LIB_PATH = _PKG / "libaesw_blind.so"  # the blinding rows of a column from a seed, and the commitment of a blinded tail (include/aesw_blind.h)

STATUS = {
    0: "AESW_OK", 1: "AESW_ERR_INVALID_ARG", 2: "AESW_ERR_NO_DEVICE", 3: "AESW_ERR_HIP", 4: "AESW_ERR_NOMEM",
    5: "AESW_ERR_CAPACITY", 6: "AESW_ERR_NO_KEY", 7: "AESW_ERR_MISMATCH", 8: "AESW_ERR_UNSATISFIED", 9: "AESW_ERR_COMM",
}
OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_CAPACITY, ERR_NO_KEY, ERR_MISMATCH = range(8)


class AeswError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        msg = "%s (%d): %s" % (STATUS.get(status, "?"), status, _strerror(status))
        if detail:
            msg += " -- " + detail
        super().__init__(msg)


class StreamStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("chunks", "bytes_to_host", "kernel_ns", "d2h_ns", "consumer_ns", "wait_ns", "wall_ns")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class KeySlab(C.Structure):
    _fields_ = [("w", C.c_void_p), ("kx", C.c_void_p), ("ky", C.c_void_p), ("kz", C.c_void_p)]


class Columns(C.Structure):
    """aesw_columns: one device allocation holding every output column of a batch (aesw_columns_alloc)."""
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_uint64), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p),
                ("ct", C.c_void_p), ("key", KeySlab), ("candidates", C.c_uint32), ("chosen", C.c_uint32),
                ("probe_us", C.c_float), ("fill_us", C.c_float)]


class Batch(C.Structure):
    """aesw_batch: one batch of aesw_encrypt_witness_batches_device."""
    _fields_ = [("d_pt", C.c_void_p), ("d_keys", C.c_void_p), ("n", C.c_uint64), ("d_x", C.c_void_p), ("d_y", C.c_void_p),
                ("d_z", C.c_void_p), ("d_ct", C.c_void_p), ("d_key_slab", C.POINTER(KeySlab))]


class CheckReport(C.Structure):
    """aesw_check_report: what aesw_check_witness_device found."""
    _fields_ = [("blocks", C.c_uint64), ("keys", C.c_uint64), ("lookup_failures", C.c_uint64), ("copy_failures", C.c_uint64),
                ("gate_failures", C.c_uint64), ("input_failures", C.c_uint64), ("first", C.c_uint64)]


class CircCheckReport(C.Structure):
    """aesw_circ_check_report: what aesw_circ_check_witness_device found."""
    _fields_ = CheckReport._fields_ + [("offset_failures", C.c_uint64)]


class MultReport(C.Structure):
    """aesw_mult_report: what aesw_mult_count_device saw next to the histograms."""
    _fields_ = [("lookups", C.c_uint64), ("misses", C.c_uint64), ("first_miss", C.c_uint64)]


class _DevView:
    """A raw device range as a __cuda_array_interface__ object, so torch can wrap it without owning it."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 3, "strides": None}


# every symbol include/aesw.h declares: (restype, argtypes)
_P, _I, _U64, _U32, _I64 = C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_int64
SYMBOLS = {
    "aesw_version": (_I, []),
    "aesw_strerror": (C.c_char_p, [_I]),
    "aesw_last_error": (C.c_char_p, [_P]),
    "aesw_device_count": (_I, [C.POINTER(_I)]),
    "aesw_create": (_I, [C.POINTER(_P), _I, _P, _P, _P]),
    "aesw_destroy": (None, [_P]),
    "aesw_device": (_I, [_P]),
    "aesw_create_group": (_I, [C.POINTER(_P), _P, _U32, _P, _P, _P]),
    "aesw_group_size": (_I, [_P]),
    "aesw_group_member": (_P, [_P, _U32]),
    "aesw_group_shard": (_I, [_U32, _U64, _U32, C.POINTER(_U64), C.POINTER(_U64)]),
    "aesw_column_stride": (_U32, [_I, _I]),
    "aesw_key_column_stride": (_U32, [_I, _I]),
    "aesw_packed_index": (_I, [_I, _P]),
    "aesw_layout_index": (_I, [_I, _I, _P]),
    "aesw_key_packed_index": (_I, [_I, _P]),
    "aesw_block_placement": (_I, [_U32, _U32, _U64, C.POINTER(_U32), C.POINTER(_U64)]),
    "aesw_block_capacity": (_U64, [_U32, _U32]),
    "aesw_selector_tags": (_I, [_P, _P, _P, _P]),
    "aesw_block_copy_graph": (_I, [_P]),
    "aesw_key_copy_graph": (_I, [_P]),
    "aesw_assemble_selectors": (_I, [_U32, _U32, _U64, _P, _P]),
    "aesw_schedule_key_device": (_I, [_P, _P, _I, C.POINTER(KeySlab), _P]),
    "aesw_schedule_key": (_I, [_P, _P, _I, C.POINTER(KeySlab)]),
    "aesw_encrypt_witness_device": (_I, [_P, _P, _P, _I, _U64, _I, _P, _P, _P, _P, C.POINTER(KeySlab), _P]),
    "aesw_encrypt_witness_batches_device": (_I, [_P, C.POINTER(Batch), _U32, _I, _I, _P]),
    "aesw_key_schedule_witness_device": (_I, [_P, _P, _U64, _I, _P, _P, _P, _P, _P, _P]),
    "aesw_lookup_table_device": (_I, [_P, _P, _P, _P, _P, _P]),
    "aesw_expand_fr_device": (_I, [_P, _P, _U64, _P, _P]),
    "aesw_check_witness_device": (_I, [_P, _P, _P, _I, _U64, _I, _P, _P, _P, _P, C.POINTER(KeySlab), _P, _P]),
    "aesw_check_witness": (_I, [_P, _P, _P, _I, _U64, _I, _P, _P, _P, _P, C.POINTER(KeySlab), C.POINTER(CheckReport)]),
    "aesw_last_stream_check": (_I, [_P, C.POINTER(CheckReport)]),
    "aesw_assemble_advice_device": (_I, [_P, _U32, _U32, _U64, _I, _P, _P, _P, C.POINTER(KeySlab), _I, _P, _P]),
    "aesw_assemble_advice_circuits_device": (_I, [_P, _U32, _U32, _U32, _P, _I, _P, _P, _P, C.POINTER(KeySlab), _I, _P, _P]),
    "aesw_columns_alloc": (_I, [_P, _U64, _I, _I, _I, C.POINTER(Columns)]),
    "aesw_columns_free": (_I, [_P, C.POINTER(Columns)]),
    "aesw_encrypt_witness": (_I, [_P, _P, _P, _I, _U64, _I, _P, _P, _P, _P, C.POINTER(KeySlab)]),
    "aesw_key_schedule_witness": (_I, [_P, _P, _U64, _I, _P, _P, _P, _P, _P]),
    "aesw_encrypt_witness_stream": (_I, [_P, _P, _P, _I, _U64, _I, _P, _P]),
    "aesw_lookup_table": (_I, [_P, _P, _P, _P, _P]),
    "aesw_last_stream_stats": (_I, [_P, _P]),
    "aesw_assemble_advice_host": (_I, [_P, _U32, _U32, _U64, _I, _P, _P, _P, C.POINTER(KeySlab), _I, _P]),
    "aesw_host_register": (_I, [_P, C.c_size_t]),
    "aesw_host_unregister": (_I, [_P]),
    "aesw_assemble_advice_stream": (_I, [_P, _U32, _U32, _U64, _I, _P, _P, _P, C.POINTER(KeySlab), _I, _P, _P]),
    "aesw_host_alloc": (_P, [C.c_size_t]),
    "aesw_host_free": (None, [_P]),
    "aesw_comm_unique_id": (_I, [_P]),
    "aesw_comm_create": (_I, [_P, _I, _I, _P, C.POINTER(_P)]),
    "aesw_comm_destroy": (None, [_P]),
    "aesw_comm_set_max_message": (_I, [_P, _U64]),
    "aesw_comm_last_error": (C.c_char_p, []),
    "aesw_gather_offsets": (_I, [_I, _P, _P, C.POINTER(_U64)]),
    "aesw_gather_columns_device": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "aesw_set_option": (_I, [_P, C.c_char_p, _I64]),
    "aesw_get_option": (_I, [_P, C.c_char_p, C.POINTER(_I64)]),
    "aesw_uses_xtime_path": (_I, [_P]),
}

# include/aesw_host.h: the host-side mirror of the reference's circuits
HOST_SYMBOLS = {
    "aesw_host_aes_circuit_run": (_I, [_P, _U32, _U32, _P, _P, _U64, _I, _I, _I, C.POINTER(_P)]),
    "aesw_host_circuit_copies": (_I, [_P, _P]),
    "aesw_host_aes_circuit_columns": (_I, [_P, _U32, _U32, _P, _P, _U64, C.POINTER(_P)]),
    "aesw_host_key_circuit_run": (_I, [_P, _U32, _P, C.POINTER(_P)]),
    "aesw_host_circuit_free": (None, [_P]),
    "aesw_host_circuit_verify": (_I, [_P, C.c_char_p, C.c_size_t]),
    "aesw_host_circuit_num_advice": (_U32, [_P]),
    "aesw_host_circuit_num_selectors": (_U32, [_P]),
    "aesw_host_circuit_num_rows": (_U64, [_P]),
    "aesw_host_circuit_num_regions": (_U64, [_P]),
    "aesw_host_circuit_num_copies": (_U64, [_P]),
    "aesw_host_circuit_closure_calls": (_U64, [_P]),
    "aesw_host_circuit_advice": (C.POINTER(C.c_uint8), [_P, _U32]),
    "aesw_host_circuit_advice_assigned": (C.POINTER(C.c_uint8), [_P, _U32]),
    "aesw_host_circuit_selector": (C.POINTER(C.c_uint8), [_P, _U32]),
    "aesw_host_circuit_fixed": (C.POINTER(C.c_uint8), [_P]),
    "aesw_host_circuit_table": (C.POINTER(C.c_uint8), [_P, _U32, C.POINTER(_U64)]),
    "aesw_host_circuit_ciphertext": (_I, [_P, _U64, _P]),
    "aesw_host_circuit_poke": (_I, [_P, _U32, _U64, C.c_uint8]),
    "aesw_host_last_error": (C.c_char_p, []),
}

# include/aesw_circ.h
CIRC_SYMBOLS = {
    "aesw_circ_check_witness_device": (_I, [_P, _U32, _U32, _U32, _P, _U64, _P, _P, _I, _P, _P, _P, _P, C.POINTER(KeySlab), _P, _P]),
    "aesw_circ_circuit_of_block": (_U32, [_P, _U32, _U64]),
}

# include/aesw_cols.h
COLS_SYMBOLS = {
    "aesw_cols_check_device": (_I, [_P, _U32, _U32, _U32, _P, _U64, _P, _P, _P, _I, _P, _P, _P]),
    "aesw_cols_cell_index": (_U64, [_U32, _U32, _U32, _U32, _U64]),
    "aesw_cols_fr_table": (None, [_P]),
    "aesw_cols_hash_search": (_I, [_P, C.POINTER(_U32), C.POINTER(_U32), _P]),
    "aesw_cols_hash_invert": (_I, [_P, _U32, _U32, _P, _P]),
}

# include/aesw_vals.h
VALS_SYMBOLS = {
    "aesw_vals_check_device": (_I, [_P, _P, _P, _I, _U64, _P, _P, _P, C.POINTER(KeySlab), _P, _P]),
    "aesw_vals_prepare": (_I, [_P]),
    "aesw_vals_check_rows": (_U32, []),
    "aesw_vals_check_table": (_I, [_P, _P]),
    "aesw_vals_image_bytes": (_U32, []),
}

# include/aesw_mult.h
_MULT_ARGS = [_P, _U32, _U32, _U32, _P, _I, _P, _P, _P, C.POINTER(KeySlab), _P, _P, _P]
MULT_SYMBOLS = {
    "aesw_mult_count_device": (_I, _MULT_ARGS),
    "aesw_mult_count_device_form": (_I, _MULT_ARGS + [_I]),
    "aesw_mult_default_form": (_I, [_U32, _U32, _U32]),
    "aesw_mult_bin": (_U32, [_U32, _U32, _U32]),
}
MULT_FORM_AUTO, MULT_FORM_DIRECT, MULT_FORM_PRIVATE = 0, 1, 2

# include/aesw_acc.h
_ACC_ADD_ARGS = [_P, _U32, _U32, _U64, _U64, _I, _P, _P, _P, _P, _P, _P]
ACC_SYMBOLS = {
    "aesw_acc_reset_device": (_I, [_P, _U32, _P, _P, _P]),
    "aesw_acc_add_device": (_I, _ACC_ADD_ARGS),
    "aesw_acc_add_device_chunk": (_I, _ACC_ADD_ARGS + [_U32]),
    "aesw_acc_add_key_device": (_I, [_P, _U32, _I, C.POINTER(KeySlab), _P, _P, _P]),
    "aesw_acc_default_chunk": (_U32, [_U32, _U32, _U64, _U64]),
}

# include/aesw_vacc.h
_VACC_ADD_ARGS = [_P, _U32, _U32, _U64, _U64, _P, _P, _P, C.POINTER(KeySlab), _P, _P, _P]
VACC_SYMBOLS = {
    "aesw_vacc_add_device": (_I, _VACC_ADD_ARGS),
    "aesw_vacc_add_device_chunk": (_I, _VACC_ADD_ARGS + [_U32]),
    "aesw_vacc_default_chunk": (_U32, [_U32, _U32, _U64, _U64]),
    "aesw_vacc_prepare": (_I, [_P]),
}

# include/aesw_perm.h
PERM_SYMBOLS = {
    "aesw_perm_workspace_bytes": (C.c_size_t, [_U32]),
    "aesw_perm_build_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P, _P]),
    "aesw_perm_gather_fr_device": (_I, [_P, _U64, _P, _P, _P, _P]),
}

# include/aesw_theta.h
THETA_SYMBOLS = {
    "aesw_theta_compress_table_device": (_I, [_P, _P, _P, _P, _P]),
    "aesw_theta_inputs_device": (_I, [_P, _U32, _U32, _U64, _I, _P, _P, _P, C.POINTER(KeySlab), _P, _P, _P]),
    "aesw_theta_prepare": (_I, [_P, _U32, _U32, _P]),
    "aesw_theta_columns_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P, _P]),
}

# include/aesw_grand.h
GRAND_SYMBOLS = {
    "aesw_grand_invert_table_device": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "aesw_grand_workspace_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_grand_product_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}
# include/aesw_sigma.h
SIGMA_SYMBOLS = {
    "aesw_sigma_columns": (_U32, [_U32]),
    "aesw_sigma_sources_host": (_I, [_U32, _P]),
    "aesw_sigma_mapping_host": (_I, [_U32, _U32, _U32, _P]),
    "aesw_sigma_tables_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_sigma_workspace_bytes": (C.c_size_t, [_U32, _U32, _U32]),
    "aesw_sigma_tables_device": (_I, [_P, _U32, _U32, _P, _P]),
    "aesw_sigma_product_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _U32, _P, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}
# include/aesw_ntt.h
NTT_SYMBOLS = {
    "aesw_ntt_tables_bytes": (C.c_size_t, [_U32]),
    "aesw_ntt_workspace_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_ntt_tables_device": (_I, [_P, _U32, _P, _P]),
    "aesw_ntt_lagrange_to_coeff_device": (_I, [_P, _U32, _U32, _P, _P, _P, _U32, _P, _P]),
    "aesw_ntt_coeff_to_lagrange_device": (_I, [_P, _U32, _U32, _P, _P, _P, _U32, _P, _P]),
    "aesw_ntt_coeff_to_extended_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P, _U32, _P, _P]),
    "aesw_ntt_extended_to_coeff_device": (_I, [_P, _U32, _U32, _U32, _P, _P, _P, _U32, _P, _P]),
}
# include/aesw_quot.h
QUOT_SYMBOLS = {
    "aesw_quot_sigma_fr_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P]),
}
# include/aesw_open.h
OPEN_SYMBOLS = {
    "aesw_open_workspace_bytes": (C.c_size_t, [_U32, _U32, _U32]),
    "aesw_open_evaluate_device": (_I, [_P, _U32, _U32, _U32, _P, _P, _P, _P, _P]),
    "aesw_open_fold_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P, _P]),
    "aesw_open_divide_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P, _P, _P]),
}
# include/aesw_msm.h
MSM_SYMBOLS = {
    "aesw_msm_chunk_rows": (_U32, []),
    "aesw_msm_slices": (_U32, [_U32, _U32, _U32, _U32]),
    "aesw_msm_workspace_bytes": (C.c_size_t, [_U32, _U32, _U32, _U32]),
    "aesw_msm_basis_device": (_I, [_P, _U32, _P, _P, _P, _P]),
    "aesw_msm_commit_device": (_I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P]),
}
MSM_FR, MSM_BYTES = 0, 1  # AESW_MSM_FR, AESW_MSM_BYTES
# include/aesw_transcript.h
TRANSCRIPT_SYMBOLS = {
    "aesw_transcript_chunk_points": (_U32, []),
    "aesw_transcript_chunk_scalars": (_U32, []),
    "aesw_transcript_init_device": (_I, [_P, _P, _P]),
    "aesw_transcript_points_device": (_I, [_P, _P, _U32, _P, _P, C.c_uint64, _P]),
    "aesw_transcript_scalars_device": (_I, [_P, _P, _U32, _P, _P, C.c_uint64, _P]),
    "aesw_transcript_squeeze_device": (_I, [_P, _P, _P, _P]),
}
TRANSCRIPT_STATE_BYTES = 256  # AESW_TRANSCRIPT_STATE_BYTES
# include/aesw_shplonk.h
SHPLONK_SYMBOLS = {
    "aesw_shplonk_scalars_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_shplonk_scalars_offset": (C.c_size_t, [_U32, _U32]),
    "aesw_shplonk_workspace_bytes": (C.c_size_t, [_U32]),
    "aesw_shplonk_report_bytes": (C.c_size_t, []),
    "aesw_shplonk_prepare_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aesw_shplonk_finish_device": (_I, [_P, _P, _P, _P, _P, _P]),
    "aesw_shplonk_combine_device": (_I, [_P, _U32, _U32, _P, _P, _P, _U32, _P, _P, _P]),
    "aesw_shplonk_quotient_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}
# include/aesw_vanish.h
VANISH_SYMBOLS = {
    "aesw_vanish_shape_ok": (_I, [_U32, _U32, _U32, _U32, _U32, _U32]),
    "aesw_vanish_tables_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_vanish_tables_device": (_I, [_P, _U32, _U32, _U32, _P, _P]),
    "aesw_vanish_scalars_bytes": (C.c_size_t, [_U32, _U32]),
    "aesw_vanish_scalars_offset": (C.c_size_t, [_U32, _U32]),
    "aesw_vanish_scalars_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P, _P, _P]),
    "aesw_vanish_head_device": (_I, [_P, _U32, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P, _P, _P]),
    "aesw_vanish_perm_device": (_I, [_P, _U32, _U32, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aesw_vanish_lookup_device": (_I, [_P, _U32, _U32, _U32, _U32, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aesw_vanish_divide_device": (_I, [_P, _U32, _U32, _P, _P, _P, _P]),
}
# include/aesw_blind.h
BLIND_SYMBOLS = {
    "aesw_blind_tail_rows": (_U64, [_U32, _U64]),
    "aesw_blind_max_tail": (_U32, []),
    "aesw_blind_rows_device": (_I, [_P, _U32, _U32, _U64, _U64, _U64, _P, _P, _P]),
    "aesw_blind_tail_device": (_I, [_P, _U32, _U32, _U64, _U64, _U64, _P, _P, _P]),
    "aesw_blind_commit_tail_device": (_I, [_P, _U32, _U32, _U64, _P, _P, _P, _P]),
}
BLIND_SEED_BYTES = 32  # AESW_BLIND_SEED_BYTES
# the entries of the scalars block (AESW_VANISH_THETA ... AESW_VANISH_BETA_DELTA), for vanishing_scalar
VANISH_TABLES = ("theta", "beta", "gamma", "y", "y_pow", "theta_pow", "tag", "delta", "beta_delta")
# the column groups of the quotient, in the order Context.quotient_extended takes them
QUOTIENT_GROUPS = ("advice", "rcon", "selectors", "table", "sigma", "zperm", "a", "s", "zlookup", "l")
# the tables of the scalars block (AESW_SHPLONK_PLAN ... AESW_SHPLONK_Y_POW), for shplonk_table
SHPLONK_TABLES = ("plan", "v_pow", "ebar", "w", "vw", "neg_r", "z", "z_t", "z0_inv", "l_coef", "l_const", "l_low", "y_pow")
SHPLONK_REPORT_LAST_REM = 32  # AESW_SHPLONK_REPORT_LAST_REM
FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001  # the order of bn256's scalar field
FQ_MODULUS = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47  # bn256's base field: the coordinates of G1

_BUILD_IT = "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
_NO_FALLBACK = " (hipcc --offload-arch=gfx950). There is no fallback implementation."
# the in-tree libraries: name -> (path, symbols, what the FileNotFoundError adds to _BUILD_IT); behind libaesw.so and the host
# mirror, one entry per library of _build.library_names(), in its order (tests/test_build_table.py holds the two together)
_LIBRARIES = {
    "aesw": (LIB_PATH, SYMBOLS, _NO_FALLBACK),
    "host": (HOST_LIB_PATH, HOST_SYMBOLS, ""),
    "circ": (CIRC_LIB_PATH, CIRC_SYMBOLS, _NO_FALLBACK),
    "cols": (COLS_LIB_PATH, COLS_SYMBOLS, _NO_FALLBACK),
    "vals": (VALS_LIB_PATH, VALS_SYMBOLS, _NO_FALLBACK),
    "acc": (ACC_LIB_PATH, ACC_SYMBOLS, _NO_FALLBACK),
    "perm": (PERM_LIB_PATH, PERM_SYMBOLS, _NO_FALLBACK),
    "vacc": (VACC_LIB_PATH, VACC_SYMBOLS, _NO_FALLBACK),
    "mult": (MULT_LIB_PATH, MULT_SYMBOLS, _NO_FALLBACK),
    "theta": (THETA_LIB_PATH, THETA_SYMBOLS, _NO_FALLBACK),
    "grand": (GRAND_LIB_PATH, GRAND_SYMBOLS, _NO_FALLBACK),
    "sigma": (SIGMA_LIB_PATH, SIGMA_SYMBOLS, _NO_FALLBACK),
    "ntt": (NTT_LIB_PATH, NTT_SYMBOLS, _NO_FALLBACK),
    "quot": (QUOT_LIB_PATH, QUOT_SYMBOLS, _NO_FALLBACK),
    "open": (OPEN_LIB_PATH, OPEN_SYMBOLS, _NO_FALLBACK),
}
# the libraries of _build.curve_library_names(), in its order: the same entry shape, consulted after _LIBRARIES
_CURVE_LIBRARIES = {
    "msm": (MSM_LIB_PATH, MSM_SYMBOLS, _NO_FALLBACK),
}
# the libraries of _build.proof_library_names(), in its order: the same entry shape, consulted after _CURVE_LIBRARIES
_PROOF_LIBRARIES = {
    "transcript": (TRANSCRIPT_LIB_PATH, TRANSCRIPT_SYMBOLS, _NO_FALLBACK),
}
# the libraries of _build.multiopen_library_names(), in its order: the same entry shape, consulted after _PROOF_LIBRARIES
_MULTIOPEN_LIBRARIES = {
    "shplonk": (SHPLONK_LIB_PATH, SHPLONK_SYMBOLS, _NO_FALLBACK),
}
# the libraries of _build.vanishing_library_names(), in its order: the same entry shape, consulted after _MULTIOPEN_LIBRARIES
_VANISHING_LIBRARIES = {
    "vanish": (VANISH_LIB_PATH, VANISH_SYMBOLS, _NO_FALLBACK),
}
# the libraries of _build.blinding_library_names(), in its order: the same entry shape, consulted after _VANISHING_LIBRARIES
_BLINDING_LIBRARIES = {
    "blind": (BLIND_LIB_PATH, BLIND_SYMBOLS, _NO_FALLBACK),
}
_loaded = {}  # name -> the CDLL of the default path


def _load(name: str, path) -> C.CDLL:
    """The library `name` with every declared symbol bound (AttributeError if its ABI is incomplete).  The default path is
    loaded once; an explicit path is loaded anew and never cached.  A missing library is an error: there is no fallback."""
    if path is None and name in _loaded:
        return _loaded[name]
    default, symbols, hint = next(table[name] for table in (_LIBRARIES, _CURVE_LIBRARIES, _PROOF_LIBRARIES, _MULTIOPEN_LIBRARIES, _VANISHING_LIBRARIES, _BLINDING_LIBRARIES)
                                 if name in table)
    if name == "aesw":
        # torch ships its own libamdhip64.so.7 and dlopen()s it by path.  Import it
        # FIRST so libaesw.so's NEEDED libamdhip64.so.7 binds to that copy: two HIP
        # runtimes in one process do not share the device (hipGetDeviceCount fails
        # in the second one).  A host without torch (the Rust caller) uses /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    else:
        _load("aesw", None)  # libaesw.so first: the NEEDED entry resolves to the copy already mapped
    p = Path(path) if path else default
    if not p.exists():
        raise FileNotFoundError((_BUILD_IT + hint) % p)
    lib = C.CDLL(str(p))  # RTLD_LOCAL: two builds of a library can sit in one process (tools/ab_lib.py)
    for sym, (res, args) in symbols.items():
        fn = getattr(lib, sym)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _loaded[name] = lib
    return lib


def load_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw.so (in-tree).  Raises if it has not been built."""
    return _load("aesw", path)


def load_host_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_host.so (in-tree): the host-side mirror.  It links against libaesw.so and holds no device code."""
    return _load("host", path)


def load_circ_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_circ.so (in-tree): the many-circuit checker behind Context.check_circuits.  It links against libaesw.so,
    whose contexts it takes."""
    return _load("circ", path)


def load_cols_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_cols.so (in-tree): the checker of the assembled advice columns behind Context.check_columns."""
    return _load("cols", path)


def load_vals_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_vals.so (in-tree): the checker of a VALUES witness behind Context.check_values."""
    return _load("vals", path)


def load_mult_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_mult.so (in-tree): the lookup multiplicities behind Context.lookup_multiplicities."""
    return _load("mult", path)


def load_acc_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_acc.so (in-tree): the chunk-by-chunk lookup multiplicities behind Context.multiplicity_accumulator."""
    return _load("acc", path)


def load_vacc_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_vacc.so (in-tree): the lookup multiplicities of a VALUES witness behind MultiplicityAccumulator.add_values."""
    return _load("vacc", path)


def load_perm_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_perm.so (in-tree): plookup's permuted columns behind Context.permuted_columns and Context.gather_fr."""
    return _load("perm", path)


def load_theta_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_theta.so (in-tree): the compression under theta behind Context.compress_table, Context.lookup_inputs and
    Context.argument_columns."""
    return _load("theta", path)


def load_grand_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_grand.so (in-tree): the lookup grand product behind Context.invert_table and Context.grand_product."""
    return _load("grand", path)


def load_sigma_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_sigma.so (in-tree): the permutation argument's grand products behind Context.permutation_tables and
    Context.permutation_product, and the host functions behind permutation_columns, permutation_sources and permutation_mapping."""
    return _load("sigma", path)


def load_ntt_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_ntt.so (in-tree): the transforms behind Context.ntt_tables, lagrange_to_coeff, coeff_to_lagrange,
    coeff_to_extended and extended_to_coeff."""
    return _load("ntt", path)


def load_quot_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_quot.so (in-tree): sigma as Fr columns behind Context.permutation_columns_fr."""
    return _load("quot", path)


def load_open_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_open.so (in-tree): coefficient columns at points behind Context.evaluate_columns, fold_columns and
    divide_columns."""
    return _load("open", path)


def load_msm_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_msm.so (in-tree): the commitments behind Context.msm_basis and Context.commit_columns."""
    return _load("msm", path)


def load_transcript_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_transcript.so (in-tree): the Blake2b transcript behind Context.transcript."""
    return _load("transcript", path)


def load_shplonk_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_shplonk.so (in-tree): SHPLONK's multi-opening argument behind Context.shplonk_prepare, shplonk_finish,
    combine_columns, set_quotient and open_shplonk."""
    return _load("shplonk", path)


def load_vanish_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_vanish.so (in-tree): the quotient h(X) behind Context.vanishing_tables, vanishing_scalars,
    quotient_accumulator and quotient_extended."""
    return _load("vanish", path)


def load_blind_library(path: Path | None = None) -> C.CDLL:
    """Load libaesw_blind.so (in-tree): the blinding cells behind Context.blind_rows and blinding_tail, and the tail commitment
    behind Context.commit_tail and commit_blinded_bytes."""
    return _load("blind", path)


def permutation_sets(n_sets: int, chunk_len: int) -> int:
    """The sets the permutation's 3 n_sets + 2 columns are cut into."""
    return -(-(3 * n_sets + 2) // chunk_len)


def permutation_source(n_sets: int, c: int):
    """Where column c of the permutation (x0 y0 z0 words rcon x1 y1 z1 ...) lies: ("advice", its column) or ("rcon", 0)."""
    return ("advice", c) if c < 3 else ("advice", 3 * n_sets) if c == 3 else ("rcon", 0) if c == 4 else ("advice", c - 2)


def quotient_pieces(h_coeff, k: int, ext_k: int):
    """The m = 2^(ext_k - k) pieces h_0 ... h_(m-1) of the quotient, h(X) = sum_i X^(n i) h_i(X): views of 2^k coefficients each of
    what extended_to_coeff returns for the quotient, a [2^ext_k, 32] tensor (or numpy array) of cells.  No copy and no kernel."""
    k, ext_k = int(k), int(ext_k)
    if not 0 <= k <= ext_k <= 28 or tuple(h_coeff.shape) != (1 << ext_k, 32):
        raise ValueError("h_coeff must have shape [2^ext_k, 32] and k must be at most ext_k")
    return [h_coeff[i << k:(i + 1) << k] for i in range(1 << (ext_k - k))]


class MultiopenPlan:
    """What multiopen_plan returns: the static part of a multi-opening.  rotations: the super set, in order of first appearance.
    sets: a list of (point indices, column ids) -- the indices strictly increasing into rotations, the columns in order of first
    appearance.  set_points, set_cols and point_index are the three host arrays of aesw_shplonk_prepare_device; eval_order() is the
    (column id, rotation) of every cell of d_evals: set by set, column by column, point by point."""

    def __init__(self, rotations, sets):
        self.rotations, self.sets = list(rotations), [(tuple(idx), list(cols)) for idx, cols in sets]
        self.set_points = [len(idx) for idx, _cols in self.sets]
        self.set_cols = [len(cols) for _idx, cols in self.sets]
        self.point_index = [p for idx, _cols in self.sets for p in idx]

    def eval_order(self) -> list:
        return [(c, self.rotations[p]) for idx, cols in self.sets for c in cols for p in idx]


def multiopen_plan(queries) -> MultiopenPlan:
    """The plan of SHPLONK's multi-opening from (column id, rotation) queries, pure Python: the super set is the rotations in
    order of first appearance; a column's point set is the indices of its rotations, ascending; columns with the same point set
    form a set, the sets and the columns within one in order of first appearance.  halo2 orders the point sets by the value of
    their points, which needs x; this order does not, and differs from halo2's."""
    rotations, of_column = [], {}
    for column, rotation in queries:
        if rotation not in rotations:
            rotations.append(rotation)
        of_column.setdefault(column, set()).add(rotations.index(rotation))
    sets = {}
    for column, indices in of_column.items():  # a dict keeps the order of first appearance
        sets.setdefault(tuple(sorted(indices)), []).append(column)
    return MultiopenPlan(rotations, list(sets.items()))


def shplonk_report_dict(rep) -> dict:
    """The report words of include/aesw_shplonk.h; last_remainder: the four words of the last division's remainder, all 0 for 0."""
    v = _words(rep)
    return {"bad_sets": v[0], "first_bad_set": None if v[1] == _NONE else v[1], "zero_differences": v[2], "z0_zero": v[3], "last_remainder": v[4:8]}


def permutation_columns(n_sets: int) -> int:
    """aesw_sigma_columns: the columns of the permutation argument of a FixedAes128Config<k, n_sets> circuit, 3 * n_sets + 2."""
    return int(load_sigma_library().aesw_sigma_columns(int(n_sets)))


def permutation_sources(n_sets: int) -> np.ndarray:
    """aesw_sigma_sources_host: uint32[3 * n_sets + 2] -- for each permutation column in halo2's order (x0 y0 z0 words rcon x1 ...)
    the assembled advice column it is, or 3 * n_sets + 1 for the fixed round_constants column."""
    out = np.zeros(3 * int(n_sets) + 2, np.uint32)
    rc = load_sigma_library().aesw_sigma_sources_host(int(n_sets), _np_ptr(out))
    if rc:
        raise AeswError(rc, "aesw_sigma_sources_host")
    return out


def permutation_mapping(k: int, n_sets: int, n_blocks: int) -> np.ndarray:
    """aesw_sigma_mapping_host: uint32[3 * n_sets + 2, 2^k] -- sigma of a circuit with one schedule_key and n_blocks encrypt calls
    as cell indices, map[c][i] = c' * 2^k + i' (halo2's Assembly::copy over the copy graphs, include/aesw_sigma.h)."""
    k, n_sets = int(k), int(n_sets)
    if not (10 <= k <= 28 and 1 <= n_sets <= 1024 and (3 * n_sets + 2) << k <= 1 << 32):
        raise AeswError(ERR_INVALID_ARG, "aesw_sigma_mapping_host")
    out = np.zeros((3 * n_sets + 2, 1 << k), np.uint32)
    rc = load_sigma_library().aesw_sigma_mapping_host(k, n_sets, int(n_blocks), _np_ptr(out))
    if rc:
        raise AeswError(rc, "aesw_sigma_mapping_host")
    return out


def fr_cell(value: int) -> np.ndarray:
    """uint8[32]: the Fr cell of `value` (any int, reduced mod r) -- value * 2^256 mod r, little-endian."""
    return np.frombuffer(((int(value) % FR_MODULUS << 256) % FR_MODULUS).to_bytes(32, "little"), np.uint8).copy()


def fq_cell(value: int) -> np.ndarray:
    """uint8[32]: the Fq coordinate of `value` (any int, reduced mod q) -- value * 2^256 mod q, little-endian."""
    return np.frombuffer(((int(value) % FQ_MODULUS << 256) % FQ_MODULUS).to_bytes(32, "little"), np.uint8).copy()


def g1_from_cells(cells) -> list:
    """The points of uint8 [..., 64] cells (what Context.commit_columns returns, copied to the host) as plain integers: (x, y) a
    point, None for the identity, 64 zero bytes."""
    unmont = pow(1 << 256, -1, FQ_MODULUS)
    rows = np.ascontiguousarray(cells, np.uint8).reshape(-1, 64)
    return [tuple(int.from_bytes(row[i:i + 32].tobytes(), "little") * unmont % FQ_MODULUS for i in (0, 32)) if row.any() else None for row in rows]


def g1_generator() -> np.ndarray:
    """uint8[64]: the generator (1, 2) of bn256's G1 as a point of a basis, x then y in Montgomery form."""
    return np.concatenate([fq_cell(1), fq_cell(2)])


def rotated_points(x: int, k: int, rotations) -> np.ndarray:
    """uint8 [len(rotations), 32]: the Fr cells of x * omega_k^r for every signed rotation r -- the points halo2 opens a column at
    for a challenge x --, omega_k = 7^((r - 1) / 2^k) the generator of the 2^k rows (k at most 28).  Pure Python, through fr_cell."""
    k = int(k)
    if not 0 <= k <= 28:
        raise ValueError("k must be 0 ... 28 (the field's 2-adicity)")
    omega = pow(7, (FR_MODULUS - 1) >> k, FR_MODULUS)
    return np.array([fr_cell(int(x) * pow(omega, int(r) % (1 << k), FR_MODULUS)) for r in rotations], np.uint8).reshape(-1, 32)


def mult_bin(tag: int, x: int, y: int = 0):
    """aesw_mult_bin: the table row the input operands of a lookup name (None for tag 0 and for anything that is no tag)."""
    b = int(load_mult_library().aesw_mult_bin(tag, x, y))
    return None if b == 0xFFFFFFFF else b


def vals_check_table():
    """aesw_vals_check_table: (words uint32[1056, 2], rows uint16[1056]) -- the resolved lookups of a VALUES block; the image
    order and the offset encoding are in include/aesw_vals.h."""
    lib = load_vals_library()
    n = int(lib.aesw_vals_check_rows())
    words, rows = np.zeros((n, 2), np.uint32), np.zeros(n, np.uint16)
    rc = lib.aesw_vals_check_table(_np_ptr(words), _np_ptr(rows))
    if rc:
        raise AeswError(rc, "aesw_vals_check_table")
    return words, rows


_NONE = 0xFFFFFFFFFFFFFFFF  # `first` / `first_cell` of a report that found nothing (-1 as int64)


def _words(rep) -> list:
    """A report tensor (int64 on any device) read back as unsigned 64-bit words."""
    return [int(x) & _NONE for x in rep.cpu().tolist()]


def _decode(v) -> dict:
    """The seven words every report starts with (the fields of CheckReport, in order) as the dict of Context.check_witness."""
    first = None if v[6] == _NONE else (v[6] >> 20, bool((v[6] >> 19) & 1), (v[6] >> 16) & 7, v[6] & 0xFFFF)
    return {"blocks": v[0], "keys": v[1], "lookup_failures": v[2], "copy_failures": v[3], "gate_failures": v[4], "input_failures": v[5],
            "first": first, "satisfied": not any(v[2:6])}


def _decode_struct(rep: CheckReport) -> dict:
    return _decode([int(getattr(rep, f)) for f, _ in CheckReport._fields_])


def check_report_dict(rep) -> dict:
    """The uint64[7] report tensor of Context.check_witness / check_values (sync=False), read back, as the dict sync=True returns."""
    return _decode(_words(rep))


def circ_report_dict(rep) -> dict:
    """The uint64[8] report tensor of Context.check_circuits(sync=False), read back, as the dict sync=True returns."""
    v = _words(rep)
    out = _decode(v)
    out.update(offset_failures=v[7], satisfied=out["satisfied"] and v[7] == 0)
    return out


def cols_report_dict(rep) -> dict:
    """The uint64[12] report tensor of Context.check_columns(sync=False), read back, as the dict sync=True returns."""
    v = _words(rep)
    out = circ_report_dict(rep[:8])
    out.update(cell_failures=v[8], unassigned_failures=v[9], first_cell=None if v[10] == _NONE else v[10], cells=v[11],
               satisfied=out["satisfied"] and v[8] == 0 and v[9] == 0)
    return out


def mult_report_dict(rep) -> dict:
    """The uint64[3] report tensor of Context.lookup_multiplicities(sync=False), read back, as the dict sync=True returns:
    lookups, misses and first_miss = None or (unit, is_key_slab, row) -- the unit is the batch-wide block index, or the circuit
    for a key slab."""
    v = _words(rep)
    first = None if v[2] == _NONE else (v[2] >> 20, bool((v[2] >> 19) & 1), v[2] & 0xFFFF)
    return {"lookups": v[0], "misses": v[1], "first_miss": first}


def theta_report_dict(rep) -> dict:
    """The uint64[2] report tensor of Context.compress_table(sync=False), read back, as the dict sync=True returns."""
    v = _words(rep)
    return {"cells": v[0], "noncanonical": bool(v[1])}


def grand_invert_report_dict(rep) -> dict:
    """The uint64[3] report tensor of Context.invert_table(sync=False), read back, as the dict sync=True returns."""
    v = _words(rep)
    return {"cells": v[0], "noncanonical": bool(v[1]), "zero_terms": v[2]}


def grand_report_dict(rep) -> dict:
    """The uint64[3] report tensor of Context.grand_product(sync=False), read back, as the dict sync=True returns: arguments,
    open and first_open = None or (set, tag)."""
    v = _words(rep)
    return {"arguments": v[0], "open": v[1], "first_open": None if v[2] == _NONE else (v[2] >> 3, v[2] & 7)}


def sigma_report_dict(rep) -> dict:
    """The uint64[6] report tensor of Context.permutation_product(sync=False), read back, as the dict sync=True returns: sets,
    open, zero_terms, first_zero = None or (set, row), out_of_range, noncanonical.  (set, row) needs k: first_zero is left as the
    word set * 2^k + row."""
    v = _words(rep)
    return {"sets": v[0], "open": bool(v[1]), "zero_terms": v[2], "first_zero": None if v[3] == _NONE else v[3], "out_of_range": v[4],
            "noncanonical": bool(v[5])}


def perm_report_dict(rep) -> dict:
    """The uint64[3] report tensor of Context.permuted_columns(sync=False), read back, as the dict sync=True returns: arguments,
    overflowed and first_overflow = None or (set, tag)."""
    v = _words(rep)
    return {"arguments": v[0], "overflowed": v[1], "first_overflow": None if v[2] == _NONE else (v[2] >> 3, v[2] & 7)}


def _ptr(x):
    """An optional argument as ctypes takes it: None, a reference to a structure, a numpy array's or a tensor's address."""
    if x is None:
        return None
    if isinstance(x, C.Structure):
        return C.byref(x)
    return _np_ptr(x) if isinstance(x, np.ndarray) else x.data_ptr()


def _strerror(status: int) -> str:
    try:
        return load_library().aesw_strerror(status).decode()
    except Exception:  # library not built yet
        return ""


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


# ---- pure-host geometry -----------------------------------------------------------

def column_stride(layout: int, col: int) -> int:
    return int(load_library().aesw_column_stride(layout, col))


def key_column_stride(layout: int, col: int) -> int:
    return int(load_library().aesw_key_column_stride(layout, col))


def packed_index(col: int) -> np.ndarray:
    idx = np.zeros(K.AES_ROWS, dtype=np.int32)
    rc = load_library().aesw_packed_index(col, _np_ptr(idx))
    if rc:
        raise AeswError(rc)
    return idx


def layout_index(layout: int, col: int) -> np.ndarray:
    """dense row -> index in column `col` of `layout` (-1: the layout leaves the cell out)."""
    idx = np.zeros(K.AES_ROWS, dtype=np.int32)
    rc = load_library().aesw_layout_index(layout, col, _np_ptr(idx))
    if rc:
        raise AeswError(rc)
    return idx


def key_packed_index(col: int) -> np.ndarray:
    idx = np.zeros(K.KEY_ROWS, dtype=np.int32)
    rc = load_library().aesw_key_packed_index(col, _np_ptr(idx))
    if rc:
        raise AeswError(rc)
    return idx


def block_placement(k: int, n_sets: int, b: int):
    """(set, first row) of the b-th encrypt() call; raises AeswError(CAPACITY) where the reference panics."""
    s, r = C.c_uint32(), C.c_uint64()
    rc = load_library().aesw_block_placement(k, n_sets, b, C.byref(s), C.byref(r))
    if rc:
        raise AeswError(rc)
    return int(s.value), int(r.value)


def block_capacity(k: int, n_sets: int) -> int:
    return int(load_library().aesw_block_capacity(k, n_sets))


def circuit_offsets(k: int, n_sets: int, counts, n: int) -> np.ndarray:
    """uint64[C+1] block offsets of C FixedAes128Config<k, n_sets> circuits (circuit c owns blocks [offsets[c], offsets[c+1]))
    from their block counts; ValueError unless there is at least one circuit, every count is 0 ... block_capacity(k, n_sets)
    (the reference panics "AES calls too many") and the counts sum to n."""
    counts = [int(c) for c in counts]
    if not counts:
        raise ValueError("at least one circuit is needed")
    cap = block_capacity(k, n_sets)
    for i, c in enumerate(counts):
        if c < 0 or c > cap:
            raise ValueError("circuit %d: %d blocks, a FixedAes128Config<%d, %d> holds 0 ... %d" % (i, c, k, n_sets, cap))
    if sum(counts) != n:
        raise ValueError("the circuits' counts sum to %d, the batch has %d blocks" % (sum(counts), n))
    offs = np.zeros(len(counts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts, dtype=np.uint64)
    return offs


def circuit_of_block(offsets, b: int) -> int:
    """aesw_circ_circuit_of_block: the circuit the many-circuit checker holds block b against (the kernel's own search, run on
    the host); offsets: C+1 block offsets.  In [0, C) whatever the offsets hold."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    if offs.ndim != 1 or offs.size < 2:
        raise ValueError("offsets must hold C + 1 entries for C >= 1 circuits")
    return int(load_circ_library().aesw_circ_circuit_of_block(_np_ptr(offs), offs.size - 1, int(b)))


def selector_tags():
    """(enc_tag[1360], key_tag[400], q_eq_rcon[96], rcon_fixed[96]): fixed selector data for keygen."""
    e, k = np.zeros(K.AES_ROWS, np.uint8), np.zeros(K.KEY_ROWS, np.uint8)
    q, c = np.zeros(K.WORDS_ROWS, np.uint8), np.zeros(K.WORDS_ROWS, np.uint8)
    rc = load_library().aesw_selector_tags(_np_ptr(e), _np_ptr(k), _np_ptr(q), _np_ptr(c))
    if rc:
        raise AeswError(rc)
    return e, k, q, c


COPY_EDGE = np.dtype([("dst_space", np.uint8), ("dst_col", np.uint8), ("dst_row", np.uint16),
                      ("src_space", np.uint8), ("src_col", np.uint8), ("src_row", np.uint16)])


def block_copy_graph() -> np.ndarray:
    """The 1 952 copy_advice() edges of one encrypt() call (structured array, see aesw_copy_edge)."""
    e = np.zeros(1952, dtype=COPY_EDGE)
    rc = load_library().aesw_block_copy_graph(_np_ptr(e))
    if rc:
        raise AeswError(rc)
    return e


def key_copy_graph() -> np.ndarray:
    """The 640 copy_advice() edges of schedule_keys()."""
    e = np.zeros(640, dtype=COPY_EDGE)
    rc = load_library().aesw_key_copy_graph(_np_ptr(e))
    if rc:
        raise AeswError(rc)
    return e


def assemble_selectors(k: int, n_sets: int, n_blocks: int):
    """(selectors[(5*n_sets+1), 2^k], fixed[2^k]) of a whole circuit, as keygen lays them out."""
    sel = np.zeros((5 * n_sets + 1, 1 << k), np.uint8)
    fixed = np.zeros(1 << k, np.uint8)
    rc = load_library().aesw_assemble_selectors(k, n_sets, n_blocks, _np_ptr(sel), _np_ptr(fixed))
    if rc:
        raise AeswError(rc)
    return sel, fixed


def device_count() -> int:
    n = C.c_int(0)
    load_library().aesw_device_count(C.byref(n))
    return int(n.value)


def host_alloc(nbytes: int) -> np.ndarray:
    """Page-locked uint8 host buffer (aesw_host_alloc): D2H lands in it without a bounce copy."""
    lib = load_library()
    p = lib.aesw_host_alloc(nbytes)
    if not p:
        raise MemoryError("aesw_host_alloc(%d) failed" % nbytes)
    buf = (C.c_uint8 * nbytes).from_address(p)
    arr = np.frombuffer(buf, dtype=np.uint8)
    _pinned[arr.ctypes.data] = p
    return arr


def host_register(arr: np.ndarray):
    """Page-lock memory the caller already owns (hipHostRegister); pair with host_unregister."""
    rc = load_library().aesw_host_register(_np_ptr(arr), arr.nbytes)
    if rc:
        raise AeswError(rc, "aesw_host_register")


def host_unregister(arr: np.ndarray):
    rc = load_library().aesw_host_unregister(_np_ptr(arr))
    if rc:
        raise AeswError(rc, "aesw_host_unregister")


def host_free(arr: np.ndarray):
    p = _pinned.pop(arr.ctypes.data, None)
    if p:
        load_library().aesw_host_free(p)


_pinned = {}


Witness = namedtuple("Witness", "x y z ct key")
KeyWitness = namedtuple("KeyWitness", "w kx ky kz rk")


class ArenaWitness(Witness):
    """A Witness whose tensors are views of an arena of aesw_columns_alloc; `.columns` is the aesw_columns handle it is
    freed by (Context.free_columns), so slicing or replacing a member tensor cannot orphan the arena."""


# ---- marshalling of the prover-side tensor arguments: every rule once -------------

TABLE_FR_SHAPE = (3, K.TABLE_ROWS, 32)  # table_fr, what compress_table returns
INV_FR_SHAPE = (2,) + TABLE_FR_SHAPE    # inv_fr, what invert_table returns


def argument_shape(k: int, n_sets: int) -> tuple:
    """(n_sets, 5, 2^k), a column of table-row indices for every lookup argument of a circuit; (0,) outside 0 <= k <= 30 and
    1 <= n_sets <= 1024, where the library refuses the call and nothing may be sized by k."""
    return (n_sets, 5, 1 << k) if 0 <= k <= 30 and 0 < n_sets <= 1024 else (0,)


def check_tensor(t, name: str, device: int, dtype: str = "uint8", shape=None, min_bytes: int | None = None, nbytes: int | None = None, alt: str = ""):
    """`t` as a library call takes it: a torch tensor of `dtype` ("uint8" or "int32") on cuda:`device`, else TypeError (`alt`
    names what else the caller accepts); contiguous, else ValueError; and of `shape` -- a tuple whose first entry may be None, any
    number of columns, or a list of such tuples --, of at least `min_bytes` or of exactly `nbytes`, where given, else ValueError."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != getattr(torch, dtype) or not t.is_cuda or t.device.index != device:
        raise TypeError("%s must be a tensor of %s on cuda:%d%s" % (name, dtype, device, alt))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != shape:
        shapes, has = shape if isinstance(shape, list) else [shape], tuple(t.shape)
        for s in shapes:
            if has == s or (s[:1] == (None,) and len(has) == len(s) and has[1:] == s[1:]):
                break
        else:
            raise ValueError("%s must have shape %s" % (name, " or ".join("[%s]" % ", ".join("n" if a is None else str(a) for a in s) for s in shapes)))
    held = t.numel() * t.element_size() if min_bytes is not None or nbytes is not None else 0
    if (min_bytes is not None and held < min_bytes) or (nbytes is not None and held != nbytes):
        raise ValueError("%s must hold %s%d bytes" % (name, "at least " if nbytes is None else "", min_bytes if nbytes is None else nbytes))
    return t


def cells_of(value, name: str = "value") -> np.ndarray:
    """The numpy half of Context._cells: an int (Python's or numpy's) or a sequence of ints becomes uint8 [n, 32], each reduced mod
    r and put into Montgomery form (fr_cell); a numpy array must already be uint8 cells, [..., 32], and is returned as it is."""
    if isinstance(value, (int, np.integer)):
        value = [value]
    if not isinstance(value, np.ndarray):
        try:
            value = np.array([fr_cell(v) for v in value], np.uint8).reshape(-1, 32)
        except TypeError:  # no sequence, or not of ints: as before, under the argument's name
            raise TypeError("%s must be ints, or uint8 cells of shape [n, 32]" % name) from None
    if value.dtype != np.uint8 or value.shape[-1:] != (32,):
        raise ValueError("%s must be ints, or uint8 cells of shape [n, 32]" % name)
    return value


class Context:
    """One aesw_ctx: a device plus the host's three byte tables."""

    def __init__(self, device: int = 0, tables=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        sbox, mul2, mul3 = tables if tables is not None else K.reference_tables()
        self._tables = tuple(np.ascontiguousarray(t, dtype=np.uint8) for t in (sbox, mul2, mul3))
        for t in self._tables:
            if t.shape != (256,):
                raise ValueError("tables must be three uint8[256] arrays")
        rc = self._lib.aesw_create(C.byref(self._h), device, *[_np_ptr(t) for t in self._tables])
        if rc:
            self._h = C.c_void_p()
            raise AeswError(rc, "aesw_create(device=%d)" % device)
        self.device = device
        self._arenas = {}  # y pointer -> Columns of alloc_columns()

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for _group, comm in list(getattr(self, "_sharding_comms", {}).values()):  # communicators sharding.gather_columns made for this context
                comm.close()
            self.__dict__.pop("_sharding_comms", None)
            for cols in list(getattr(self, "_arenas", {}).values()):
                self._lib.aesw_columns_free(self._h, C.byref(cols))
            self._arenas = {}
            self._lib.aesw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str = ""):
        if rc:
            raise AeswError(rc, (what + " " + self._lib.aesw_last_error(self._h).decode()).strip())

    # -- options
    def set_option(self, name: str, value: int):
        self._check(self._lib.aesw_set_option(self._h, name.encode(), int(value)), "set_option(%s)" % name)

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        self._check(self._lib.aesw_get_option(self._h, name.encode(), C.byref(v)), "get_option(%s)" % name)
        return int(v.value)

    @property
    def uses_xtime_path(self) -> bool:
        return bool(self._lib.aesw_uses_xtime_path(self._h))

    # -- tensor plumbing
    def _torch(self):
        import torch
        return torch

    def _dev(self):
        return self._torch().device("cuda", self.device)

    def _stream(self):
        return C.c_void_p(self._torch().cuda.current_stream(self.device).cuda_stream)

    def _u8(self, t, what):
        torch = self._torch()
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.device.index != self.device:
            raise TypeError("%s must be a uint8 tensor on cuda:%d" % (what, self.device))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        return t

    # the prover-side arguments (lookup_multiplicities ... divide_columns): check_tensor on this context's device
    def _tensor(self, t, name, dtype="uint8", shape=None, **size):
        return check_tensor(t, name, self.device, dtype, shape, **size)

    def _output(self, t, name, shape, dtype="uint8", **size):
        """An output: None allocates `shape`; a tensor handed in must have that shape -- or the byte count of `size` instead."""
        if t is None:
            return self._torch().empty(shape, dtype=getattr(self._torch(), dtype), device=self._dev())
        return check_tensor(t, name, self.device, dtype, None if size else shape, **size)

    def _workspace(self, t, need: int):
        """A workspace of `need` bytes: the caller's, or one that lives for the call."""
        if t is None:
            # freed on return, while the kernels may still run: the caching allocator hands it out again in stream order only
            return self._torch().empty(max(need, 16), dtype=self._torch().uint8, device=self._dev())
        return check_tensor(t, "_workspace", self.device, min_bytes=need)

    def _index_words(self, t, name, shape):
        """uint32 words the kernels index by (source, mapping): a numpy array is uploaded as int32, an int32 device tensor stays."""
        if isinstance(t, np.ndarray):
            t = self._torch().from_numpy(np.ascontiguousarray(t, np.uint32).view(np.int32)).to(self._dev())
        return check_tensor(t, name, self.device, "int32", shape, alt=", or a numpy array")

    def _columns(self, t, name, k):
        """n_cols of `t`, a uint8 [n_cols, 2^k, 32] tensor of columns of cells (or [2^k, 32], one column)."""
        check_tensor(t, name, self.device, shape=[(None, 1 << k, 32), (1 << k, 32)])
        return t.shape[0] if t.dim() == 3 else 1

    def _point_rows(self, t, name):
        """Points as they lie in memory, a uint8 [n, 64] tensor on the device (what commit_columns returns): a numpy array is
        uploaded, a device tensor stays."""
        if isinstance(t, np.ndarray):
            t = self._torch().from_numpy(np.ascontiguousarray(t, np.uint8)).to(self._dev())
        return check_tensor(t, name, self.device, shape=(None, 64), alt=", or a numpy array")

    def _points(self, t, name):
        """Points as the calls of libaesw_msm.so read them, a uint8 [2^k, 64] tensor on the device, and k: a numpy array is uploaded,
        a device tensor stays.  A row count that is no power of two in 2^10 ... 2^28 is refused."""
        t = self._point_rows(t, name)
        k = t.shape[0].bit_length() - 1
        if t.shape[0] != 1 << k or not 10 <= k <= 28:
            raise AeswError(ERR_INVALID_ARG, "%s must hold 2^k points, k = 10 ... 28" % name)
        return t, k

    def _cells(self, value, name, one=False):
        """Points (or v) as the calls of libaesw_open.so read them, a uint8 [n, 32] tensor of cells on the device: an int or a
        sequence of ints (reduced mod r and put into Montgomery form) and a numpy uint8 [n, 32] array of cells (rotated_points) are
        uploaded, a uint8 [n, 32] or [32] tensor stays and is read when the kernels run.  one: n must be 1."""
        if not isinstance(value, self._torch().Tensor):
            value = self._torch().from_numpy(np.ascontiguousarray(cells_of(value, name))).to(self._dev())
        value = check_tensor(value, name, self.device, shape=[(None, 32), (32,)], alt=", or ints or numpy cells").view(-1, 32)
        if one and value.shape[0] != 1:
            raise ValueError("%s must be one int or one cell" % name)
        return value

    def _challenge(self, value, name):
        """theta, beta or gamma as the calls that read a challenge take it: an int (Python's or numpy's; reduced mod r and put into
        Montgomery form, one 32-byte upload per call) becomes its cell on the device, a uint8[32] tensor stays."""
        if isinstance(value, (int, np.integer)):
            value = self._torch().from_numpy(fr_cell(value)).to(self._dev())
        return check_tensor(value, name, self.device, shape=(32,), alt=", or an int")

    def alloc_witness(self, n: int, layout: int = K.LAYOUT_PACKED, want_ct: bool = False, key_slab: bool = False,
                      n_keys: int | None = None):
        torch = self._torch()
        dev = self._dev()
        cols = [torch.empty(n * column_stride(layout, c), dtype=torch.uint8, device=dev) for c in range(3)]
        ct = torch.empty((n, 16), dtype=torch.uint8, device=dev) if want_ct else None
        key = None
        if key_slab:
            m = n if n_keys is None else n_keys
            key = KeyWitness(torch.empty(m * K.WORDS_ROWS, dtype=torch.uint8, device=dev),
                             *[torch.empty(m * key_column_stride(layout, c), dtype=torch.uint8, device=dev)
                               for c in range(3)], None)
        return Witness(cols[0], cols[1], cols[2], ct, key)

    def alloc_columns(self, n: int, layout: int = K.LAYOUT_PACKED, want_ct: bool = False, key_slab: bool = False, key_only: bool = False):
        """alloc_witness through the C ABI's arena (aesw_columns_alloc): every column of the batch placed together, each on
        a 2 MiB boundary.  From 2^16 blocks on the physical backing is chosen by measurement (option "arena_probe"; a shape
        this context has placed and freed before comes out of its placement cache without a search, last_arena["candidates"]
        == 0); with "arena_probe" 0 it is one hipMalloc with columns on 2^"arena_align_log2"-byte boundaries (that option is
        ignored on the probed path).  The returned ArenaWitness's tensors are views of the arena, which lives until
        free_columns(witness) or the Context is closed."""
        torch = self._torch()
        cols = Columns()
        if key_only:
            key_slab = True
        self._check(self._lib.aesw_columns_alloc(self._h, n, layout, 2 if key_only else (1 if key_slab else 0), 1 if want_ct else 0, C.byref(cols)),
                    "aesw_columns_alloc")
        dev = self._dev()

        def view(ptr, nbytes):
            if not ptr or not nbytes:
                return torch.empty(0, dtype=torch.uint8, device=dev)
            return torch.as_tensor(_DevView(ptr, nbytes), device=dev)

        x, y, z = (view(getattr(cols, c), n * column_stride(layout, i) if not key_only else 0) for i, c in enumerate("xyz"))
        ct = view(cols.ct, n * 16).view(n, 16) if want_ct else None
        key = None
        if key_slab:
            key = KeyWitness(view(cols.key.w, n * K.WORDS_ROWS), *[view(getattr(cols.key, c), n * key_column_stride(layout, i))
                                                                   for i, c in enumerate(("kx", "ky", "kz"))], None)
        wit = ArenaWitness(x, y, z, ct, key)
        wit.columns = cols
        self._arenas[id(cols)] = cols
        self.last_arena = {"candidates": int(cols.candidates), "chosen": int(cols.chosen), "probe_us": float(cols.probe_us),
                           "fill_us": float(cols.fill_us), "bytes": int(cols.bytes)}
        return wit

    def free_columns(self, wit) -> None:
        """Release the arena behind a Witness from alloc_columns (its tensors must not be used afterwards)."""
        cols = getattr(wit, "columns", None)
        if cols is None or self._arenas.pop(id(cols), None) is None:
            raise ValueError("not a witness of alloc_columns (or already freed)")
        wit.columns = None
        self._check(self._lib.aesw_columns_free(self._h, C.byref(cols)), "aesw_columns_free")

    # -- device entry points
    def schedule_key(self, key, layout: int = K.LAYOUT_PACKED, key_slab: bool = True):
        """FixedAes128Config::schedule_key (src/aes128.rs:143-152): expand `key`
        (uint8[16] on the device) once; later encrypt_witness(pt, None) calls use it.
        Returns its key-schedule witness (KeyWitness, rk=None) when key_slab."""
        torch = self._torch()
        key = self._u8(key, "key")
        if key.numel() != 16:
            raise ValueError("key must be uint8[16]")
        out = ks = None
        if key_slab:
            dev = self._dev()
            out = KeyWitness(torch.empty(K.WORDS_ROWS, dtype=torch.uint8, device=dev),
                             *[torch.empty(key_column_stride(layout, c), dtype=torch.uint8, device=dev) for c in range(3)],
                             None)
            ks = KeySlab(*[t.data_ptr() for t in out[:4]])
        rc = self._lib.aesw_schedule_key_device(self._h, key.data_ptr(), layout, _ptr(ks),
                                                self._stream())
        self._check(rc, "aesw_schedule_key_device")
        return out

    def encrypt_witness(self, pt, keys, layout: int = K.LAYOUT_PACKED, out: Witness | None = None,
                        want_ct: bool = False, key_slab: bool = False) -> Witness:
        """Batched FixedAes128Config::encrypt witness (src/aes128.rs:154-265).

        pt: uint8[n,16] on the device.  keys: None (the key given to
        schedule_key(): the reference's schedule_key once + encrypt n times),
        uint8[16] (one shared key expanded inside the call) or uint8[n,16]
        (per-block keys).  Asynchronous on torch's current stream.
        """
        pt = self._u8(pt, "pt")
        if pt.dim() != 2 or pt.shape[1] != 16:
            raise ValueError("pt must be [n,16]")
        n = pt.shape[0]
        if keys is None:
            pbk = 0
            if key_slab:
                raise ValueError("the key slab of a scheduled key is returned by schedule_key()")
        else:
            keys = self._u8(keys, "keys")
        if keys is None:
            pass
        elif keys.numel() == 16 and keys.dim() == 1:
            pbk = 0
        elif keys.dim() == 2 and tuple(keys.shape) == (n, 16):
            pbk = 1
        else:
            raise ValueError("keys must be [16] (shared) or [n,16] (per block)")
        if out is None:
            out = self.alloc_witness(n, layout, want_ct, key_slab, n_keys=n if pbk else 1)
        for c, name in enumerate("xyz"):
            self._u8(out[c], name)
            if out[c].numel() < n * column_stride(layout, c):
                raise ValueError("column %s too small" % name)
        ks = None
        if out.key is not None:
            ks = KeySlab(*[_ptr(t) for t in out.key[:4]])
        rc = self._lib.aesw_encrypt_witness_device(
            self._h, pt.data_ptr(), _ptr(keys), pbk, n, layout,
            out.x.data_ptr() if out.x.numel() else None, out.y.data_ptr(),
            out.z.data_ptr(), _ptr(out.ct),
            _ptr(ks), self._stream())
        self._check(rc, "aesw_encrypt_witness_device")
        return out

    def encrypt_witness_batches(self, batches, per_block_keys: bool, layout: int = K.LAYOUT_PACKED):
        """aesw_encrypt_witness_batches_device: `batches` is a list of (pt, keys, out) with pt uint8[n,16], keys None /
        uint8[16] / uint8[n,16] (all batches in the same key mode) and out a Witness whose columns hold n blocks (its .ct and
        .key are written when present).  The batches are dealt round-robin onto the context's internal streams behind torch's
        current stream and joined back into it: ramp and tail of one launch overlap its neighbours."""
        arr = (Batch * len(batches))()
        keep = []
        for i, (pt, keys, out) in enumerate(batches):
            pt = self._u8(pt, "pt")
            n = pt.shape[0]
            if pt.dim() != 2 or pt.shape[1] != 16:
                raise ValueError("pt must be [n,16]")
            if keys is not None:
                keys = self._u8(keys, "keys")
                if keys.numel() != (n * 16 if per_block_keys else 16):
                    raise ValueError("keys must hold 16 bytes, or n*16 with per_block_keys")
            elif per_block_keys:
                raise ValueError("per_block_keys needs keys")
            for c, name in enumerate("xyz"):
                if out[c].numel() < n * column_stride(layout, c):
                    raise ValueError("column %s of batch %d too small" % (name, i))
            ks = None
            if out.key is not None:
                ks = KeySlab(*[_ptr(t) for t in out.key[:4]])
                keep.append(ks)
            arr[i] = Batch(pt.data_ptr(), _ptr(keys), n,
                           out.x.data_ptr() if out.x.numel() else None, out.y.data_ptr(), out.z.data_ptr(),
                           _ptr(out.ct), C.pointer(ks) if ks is not None else None)
            keep.append((pt, keys))
        rc = self._lib.aesw_encrypt_witness_batches_device(self._h, arr, len(batches), 1 if per_block_keys else 0, layout, self._stream())
        self._check(rc, "aesw_encrypt_witness_batches_device")

    def key_schedule_witness(self, keys, layout: int = K.LAYOUT_PACKED, want_rk: bool = True, out: KeyWitness | None = None) -> KeyWitness:
        """Aes128KeyScheduleConfig::schedule_keys witness for n keys (src/key_schedule.rs:80-224); into `out`
        (e.g. alloc_columns(n, layout, key_only=True).key) when given."""
        torch = self._torch()
        keys = self._u8(keys, "keys")
        if keys.dim() == 1:
            keys = keys.reshape(1, 16)
        if keys.dim() != 2 or keys.shape[1] != 16:
            raise ValueError("keys must be [n,16]")
        n = keys.shape[0]
        dev = self._dev()
        if out is not None:
            w, kx, ky, kz = out[:4]
            for t, need in ((w, n * K.WORDS_ROWS), (kx, n * key_column_stride(layout, 0)), (ky, n * key_column_stride(layout, 1)),
                            (kz, n * key_column_stride(layout, 2))):
                if self._u8(t, "out").numel() < need:
                    raise ValueError("out column too small")
        else:
            w = torch.empty(n * K.WORDS_ROWS, dtype=torch.uint8, device=dev)
            kx, ky, kz = [torch.empty(n * key_column_stride(layout, c), dtype=torch.uint8, device=dev) for c in range(3)]
        rk = torch.empty((n, 176), dtype=torch.uint8, device=dev) if want_rk else None
        rc = self._lib.aesw_key_schedule_witness_device(
            self._h, keys.data_ptr(), n, layout, w.data_ptr(), kx.data_ptr(), ky.data_ptr(), kz.data_ptr(),
            _ptr(rk), self._stream())
        self._check(rc, "aesw_key_schedule_witness_device")
        return KeyWitness(w, kx, ky, kz, rk)

    def lookup_table(self):
        """load_enc_full_table (src/table.rs:18-192): four uint8[66561] columns on the device."""
        torch = self._torch()
        t = torch.empty((4, K.TABLE_ROWS), dtype=torch.uint8, device=self._dev())
        rc = self._lib.aesw_lookup_table_device(self._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                t[3].data_ptr(), self._stream())
        self._check(rc, "aesw_lookup_table_device")
        return t

    def expand_fr(self, cells, out=None):
        """uint8 cells -> [n,32] uint8 bn256::Fr Montgomery cells (Fp::from(u64), src/utils.rs:23)."""
        torch = self._torch()
        cells = self._u8(cells, "cells")
        n = cells.numel()
        if out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device=self._dev())
        rc = self._lib.aesw_expand_fr_device(self._h, cells.data_ptr(), n, out.data_ptr(), self._stream())
        self._check(rc, "aesw_expand_fr_device")
        return out

    def _report(self, rep, sync: bool, decode):
        """The end of every check_*: the report tensor as it is, or synchronise the stream and decode it."""
        if not sync:
            return rep
        self._torch().cuda.current_stream().synchronize()
        return decode(rep)

    def check_witness(self, pt, keys, witness: Witness, key_witness: KeyWitness, layout: int = K.LAYOUT_PACKED, ct=None, sync: bool = True):
        """MockProver::assert_satisfied over a batch on the device (aesw_check_witness_device; src/aes128.rs:409-418): every
        enabled lookup, every copy_advice() pair, the round-constant gate and the literal rows of n blocks and their key slab(s).
        keys: None, uint8[16] or uint8[n,16] (per-block keys: key_witness then holds n key slabs).  Returns a dict (counts,
        `satisfied`, `first` = None or (unit, is_key_slab, kind, index)) after synchronising the stream; with sync=False the
        uint64[7] device tensor the report was written to."""
        torch = self._torch()
        pt = self._u8(pt, "pt")
        n = pt.shape[0]
        pbk = keys is not None and self._u8(keys, "keys").numel() != 16
        ks = KeySlab(*[t.data_ptr() for t in key_witness[:4]])
        rep = torch.empty(7, dtype=torch.int64, device=self._dev())
        rc = self._lib.aesw_check_witness_device(
            self._h, pt.data_ptr(), _ptr(keys), 1 if pbk else 0, n, layout, witness.x.data_ptr(),
            witness.y.data_ptr(), witness.z.data_ptr(), _ptr(ct), C.byref(ks), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_check_witness_device")
        return self._report(rep, sync, check_report_dict)

    def check_values(self, pt, keys, witness: Witness, key_witness: KeyWitness, ct=None, sync: bool = True):
        """MockProver::assert_satisfied over a VALUES witness on the device (aesw_vals_check_device, libaesw_vals.so): the 1 056
        enabled lookups of every block, each x (and the y of an xor row) resolved through the copy graph to the VALUES cell, plaintext
        byte or round-key cell it copies from, and the packed key slab(s) as check_witness checks them.  witness: the y / z of
        encrypt_witness(layout=LAYOUT_VALUES) (x is ignored); keys: None, uint8[16] or uint8[n,16] (per-block keys: key_witness
        then holds n key slabs).  Returns the dict of check_witness after synchronising the stream; with sync=False the uint64[7]
        device tensor the report was written to."""
        lib = load_vals_library()
        torch = self._torch()
        pt = self._u8(pt, "pt")
        n = int(pt.shape[0])
        pbk = keys is not None and self._u8(keys, "keys").numel() != 16
        ks = KeySlab(*[t.data_ptr() for t in key_witness[:4]]) if key_witness is not None else None
        rep = torch.empty(7, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_vals_check_device(
            self._h, pt.data_ptr() if n else None, _ptr(keys), 1 if pbk else 0, n, _ptr(witness.y), _ptr(witness.z),
            ct.data_ptr() if ct is not None and n else None, _ptr(ks), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_vals_check_device")
        return self._report(rep, sync, check_report_dict)

    def last_stream_check(self):
        """aesw_last_stream_check: what option "stream_check" found over the chunks of the last encrypt_witness_stream call."""
        rep = CheckReport()
        self._check(self._lib.aesw_last_stream_check(self._h, C.byref(rep)), "aesw_last_stream_check")
        return _decode_struct(rep)

    def check_witness_host(self, pt, keys, cols, key_cols, layout: int = K.LAYOUT_PACKED, ct=None):
        """aesw_check_witness: the same check for a witness in HOST memory (numpy uint8 arrays: cols = (x, y, z), key_cols =
        (w, kx, ky, kz)); uploaded and checked in stages of "chunk_blocks" blocks."""
        import numpy as np
        pt = np.ascontiguousarray(pt, np.uint8).reshape(-1, 16)
        n = pt.shape[0]
        keys = None if keys is None else np.ascontiguousarray(keys, np.uint8)
        pbk = keys is not None and keys.size != 16
        keep = [np.ascontiguousarray(a, np.uint8) for a in (*cols, *key_cols)] + ([np.ascontiguousarray(ct, np.uint8)] if ct is not None else [])
        ks = KeySlab(*[a.ctypes.data for a in keep[3:7]])
        rep = CheckReport()
        rc = self._lib.aesw_check_witness(self._h, _np_ptr(pt), _ptr(keys), 1 if pbk else 0, n, layout, *[_np_ptr(a) for a in keep[:3]],
                                          _np_ptr(keep[7]) if ct is not None else None, C.byref(ks), C.byref(rep))
        self._check(rc, "aesw_check_witness")
        return _decode_struct(rep)

    def assemble_advice(self, k: int, n_sets: int, witness: Witness, key_witness: KeyWitness | None, n_blocks: int,
                        layout: int = K.LAYOUT_PACKED, as_fr: bool = False, out=None):
        """All advice columns of a FixedAes128Config<K, n_sets> circuit as the prover holds them:
        [(3*n_sets+1), 2^k] bytes, or [(3*n_sets+1), 2^k, 32] Fr cells with as_fr (into `out` when given)."""
        torch = self._torch()
        ncol = 3 * n_sets + 1
        shape = (ncol, 1 << k, 32) if as_fr else (ncol, 1 << k)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self._dev())
        elif tuple(out.shape) != shape:
            raise ValueError("out must have shape %r" % (shape,))
        self._u8(out, "out")
        ks = KeySlab(*[t.data_ptr() for t in key_witness[:4]]) if key_witness is not None else None
        rc = self._lib.aesw_assemble_advice_device(
            self._h, k, n_sets, n_blocks, layout, witness.x.data_ptr(), witness.y.data_ptr(), witness.z.data_ptr(),
            _ptr(ks), 1 if as_fr else 0, out.data_ptr(), self._stream())
        self._check(rc, "aesw_assemble_advice_device")
        return out

    # -- many circuits per launch
    def _offsets_tensor(self, offs: np.ndarray):
        return self._torch().from_numpy(offs.view(np.int64)).to(self._dev())

    def _circuit_args(self, k: int, n_sets: int, n: int, counts, keys, _offsets=None):
        """What the many-circuit entry points share: (C, the device int64[C+1] block offsets) of `counts` over n blocks,
        validated on the host unless `_offsets` is handed in, and keys checked to be None or uint8[C,16]."""
        nc = len(counts)
        if _offsets is None:
            _offsets = self._offsets_tensor(circuit_offsets(k, n_sets, counts, n))
        elif int(_offsets.numel()) != nc + 1:
            raise ValueError("_offsets must hold len(counts) + 1 entries")
        if keys is not None and tuple(self._u8(keys, "keys").shape) != (nc, 16):
            raise ValueError("keys must be [C,16] for C = len(counts)")
        return nc, _offsets

    def _key_slabs(self, key_witness, nc: int) -> KeySlab:
        """The aesw_key_slab of a key_witness that holds (at least) nc key slabs."""
        if key_witness is None or int(key_witness.w.numel()) < nc * K.WORDS_ROWS:
            raise ValueError("key_witness must hold one key slab per circuit")
        return KeySlab(*[self._u8(t, "key_witness").data_ptr() for t in key_witness[:4]])

    def assemble_advice_circuits(self, k: int, n_sets: int, witness: Witness, key_witness: KeyWitness, counts, as_fr: bool = False,
                                 layout: int = K.LAYOUT_PACKED, n_blocks: int | None = None, out=None, _offsets=None):
        """aesw_assemble_advice_circuits_device: the advice columns of C FixedAes128Config<k, n_sets> circuits as
        [C, 3*n_sets+1, 2^k] bytes, or [C, 3*n_sets+1, 2^k, 32] Fr cells with as_fr; circuit c is counts[c] blocks of
        `witness` (in order) and key slab c of `key_witness`.  n_blocks (default: the blocks `witness` holds) must equal
        sum(counts); the counts are checked before anything is launched."""
        if n_blocks is None:
            n_blocks = int(witness.y.numel()) // column_stride(layout, 1)
        offs = circuit_offsets(k, n_sets, counts, n_blocks)
        nc = len(offs) - 1
        ks = self._key_slabs(key_witness, nc)
        torch = self._torch()
        shape = (nc, 3 * n_sets + 1, 1 << k) + ((32,) if as_fr else ())
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self._dev())
        elif tuple(out.shape) != shape:
            raise ValueError("out must have shape %r" % (shape,))
        self._u8(out, "out")
        d_offs = self._offsets_tensor(offs) if _offsets is None else _offsets
        rc = self._lib.aesw_assemble_advice_circuits_device(
            self._h, k, n_sets, nc, d_offs.data_ptr(), layout, witness.x.data_ptr(), witness.y.data_ptr(), witness.z.data_ptr(),
            C.byref(ks), 1 if as_fr else 0, out.data_ptr(), self._stream())
        self._check(rc, "aesw_assemble_advice_circuits_device")
        return out

    def check_circuits(self, k: int, n_sets: int, pt, keys, witness: Witness, key_witness: KeyWitness, counts, layout: int = K.LAYOUT_PACKED,
                       ct=None, sync: bool = True, _offsets=None):
        """MockProver::assert_satisfied over C FixedAes128Config<k, n_sets> circuits in one launch (aesw_circ_check_witness_device,
        libaesw_circ.so): block b of `witness` against the lookups, its copies resolved in key slab circuit(b) of `key_witness`, its
        literal rows against pt (uint8[n,16]) and ct (uint8[n,16] or None); every one of the C key slabs, and its key bytes when
        keys (uint8[C,16] or None) is given; and the offsets themselves.  counts: blocks per circuit, validated on the host like
        assemble_advice_circuits; _offsets: a device int64[C+1] tensor passed through unvalidated instead (counts then only gives C).
        Returns the dict of check_witness plus `offset_failures` (`satisfied` also needs that to be 0; a key slab's unit is its
        circuit) after synchronising the stream; with sync=False the uint64[8] device tensor the report was written to."""
        lib = load_circ_library()
        torch = self._torch()
        pt = self._u8(pt, "pt")
        n = int(pt.shape[0])
        nc, d_offs = self._circuit_args(k, n_sets, n, counts, keys, _offsets)
        ks = self._key_slabs(key_witness, nc)
        rep = torch.empty(8, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_circ_check_witness_device(
            self._h, k, n_sets, nc, d_offs.data_ptr(), n, pt.data_ptr() if n else None, _ptr(keys), layout,
            witness.x.data_ptr() if n else None, witness.y.data_ptr() if n else None, witness.z.data_ptr() if n else None,
            ct.data_ptr() if ct is not None and n else None, C.byref(ks), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_circ_check_witness_device")
        return self._report(rep, sync, circ_report_dict)

    def lookup_multiplicities(self, k: int, n_sets: int, witness: Witness, key_witness: KeyWitness | None, counts,
                              layout: int = K.LAYOUT_PACKED, sync: bool = True, _offsets=None, _form: int = MULT_FORM_AUTO, _out=None):
        """How often every row of the lookup table is looked up, per circuit and column set (aesw_mult_count_device,
        libaesw_mult.so): (mult, report) with mult an int32 [C, n_sets, 66561] tensor in the row order of lookup_table() --
        histogram (c, s) counts the blocks of set s of circuit c, (c, 0) also the rows of key slab c of `key_witness` (None: no
        key lookups) -- and report the dict of mult_report_dict after synchronising the stream, or with sync=False the uint64[3]
        device tensor.  The all-zero row stays 0: for the argument (set s, tag t) its multiplicity is 2^k minus the sum of section
        t of histogram (c, s).  counts / _offsets as for check_circuits; _form forces one of the two forms (MULT_FORM_*) and
        _out is an int32 [C, n_sets, 66561] tensor to count into (tests, tools)."""
        lib = load_mult_library()
        torch = self._torch()
        n = sum(int(c) for c in counts)
        for i, t in enumerate(witness[:3]):
            if int(self._u8(t, "witness").numel()) < n * column_stride(layout, i):
                raise ValueError("witness holds fewer blocks than the counts sum to")
        nc, d_offs = self._circuit_args(k, n_sets, n, counts, None, _offsets)
        ks = self._key_slabs(key_witness, nc) if key_witness is not None else None
        _out = self._output(_out, "_out", (nc, n_sets, K.TABLE_ROWS), "int32")
        rep = torch.empty(3, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_mult_count_device_form(
            self._h, k, n_sets, nc, d_offs.data_ptr(), layout, witness.x.data_ptr(), witness.y.data_ptr(), witness.z.data_ptr(),
            _ptr(ks), _out.data_ptr(), rep.data_ptr(), self._stream(), _form)
        self._check(rc, "aesw_mult_count_device")
        return _out, self._report(rep, sync, mult_report_dict)

    def permuted_columns(self, k: int, n_sets: int, mult, n_rows: int | None = None, pad_row: int = 0, sync: bool = True, _out=None):
        """plookup's permuted columns of the 5 * n_sets lookup arguments of one circuit, arranged from its lookup multiplicities
        (aesw_perm_build_device, libaesw_perm.so): (a, s, report) with a and s int32 [n_sets, 5, 2^k] tensors of table-row
        indices in the row order of lookup_table() -- argument (set, tag) at [set, tag - 1], A' and S' -- of which rows
        0 ... n_rows - 1 are written (n_rows: the usable rows, default 2^k; the rest is the host's blinding rows).  mult: the
        int32 [n_sets, 66561] histograms of lookup_multiplicities (one circuit) or MultiplicityAccumulator.histograms();
        pad_row: the table row the table columns hold below row 66 560.  report: the dict of perm_report_dict after synchronising
        the stream, or with sync=False the uint64[3] device tensor.  The call owns its workspace; _out is an (a, s) pair of
        such tensors to write into (tests, tools)."""
        lib = load_perm_library()
        torch = self._torch()
        k, n_sets = int(k), int(n_sets)
        if isinstance(mult, torch.Tensor) and tuple(mult.shape) == (1, n_sets, K.TABLE_ROWS):
            mult = mult[0]
        mult = self._tensor(mult, "mult", "int32", (n_sets, K.TABLE_ROWS))
        _out = [self._output(t, "_out", argument_shape(k, n_sets), "int32") for t in ((None, None) if _out is None else _out)]
        ws = self._workspace(None, int(lib.aesw_perm_workspace_bytes(n_sets)))
        rep = torch.empty(3, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_perm_build_device(self._h, k, n_sets, (1 << k) if n_rows is None else int(n_rows), int(pad_row), mult.data_ptr(),
                                        _out[0].data_ptr(), _out[1].data_ptr(), ws.data_ptr(), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_perm_build_device")
        return _out[0], _out[1], self._report(rep, sync, perm_report_dict)

    def gather_fr(self, index, table_fr, out=None):
        """int32 table-row indices (any shape; a column of permuted_columns) -> [..., 32] uint8 cells: table_fr[index]
        (aesw_perm_gather_fr_device).  table_fr: uint8 [66561, 32], the host's compressed table; an index outside the table gives
        a cell of zeros."""
        lib = load_perm_library()
        index = self._tensor(index, "index", "int32")
        table_fr = self._tensor(table_fr, "table_fr", shape=TABLE_FR_SHAPE[1:])
        n = index.numel()
        out = self._output(out, "out", tuple(index.shape) + (32,), nbytes=n * 32)
        rc = lib.aesw_perm_gather_fr_device(self._h, n, index.data_ptr(), table_fr.data_ptr(), out.data_ptr(), self._stream())
        self._check(rc, "aesw_perm_gather_fr_device")
        return out

    def compress_table(self, theta, sync: bool = True, _out=None):
        """The three compressed tables under theta (aesw_theta_compress_table_device, libaesw_theta.so): (table_fr, report) with
        table_fr a uint8 [3, 66561, 32] tensor -- table j compresses the first j + 2 of (tag, a, b, c) of every row of
        lookup_table(), acc = acc * theta + e -- and report the dict of theta_report_dict after synchronising the stream, or with
        sync=False the uint64[2] device tensor.  theta: an int (reduced mod r and put into Montgomery form here), or a uint8[32]
        tensor on the device holding the cell as it lies, which is read when the kernel runs; if it is not canonical every cell
        is zero and the report says so.  _out is a tensor to write into (tests, tools)."""
        lib = load_theta_library()
        torch = self._torch()
        theta = self._challenge(theta, "theta")
        _out = self._output(_out, "_out", TABLE_FR_SHAPE)
        rep = torch.empty(2, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_theta_compress_table_device(self._h, theta.data_ptr(), _out.data_ptr(), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_theta_compress_table_device")
        return _out, self._report(rep, sync, theta_report_dict)

    def lookup_inputs(self, k: int, n_sets: int, witness: Witness, key_witness: KeyWitness | None, n_blocks: int | None = None,
                      layout: int = K.LAYOUT_PACKED, sync: bool = True, _out=None):
        """The compressed input columns of one circuit in row order, as table-row indices (aesw_theta_inputs_device): (index,
        report) with index an int32 [n_sets, 5, 2^k] tensor -- argument (set, tag) at [set, tag - 1]; the bin of the row's lookup,
        -1 (0xffffffff) for a miss, 66560 (the all-zero row) wherever the argument's selector is off -- and report the dict of
        mult_report_dict after synchronising the stream, or with sync=False the uint64[3] device tensor.  The circuit is the first
        n_blocks blocks of `witness` (default: all it holds) and the key slab `key_witness` (None: no key lookups).  _out is a
        tensor to write into (tests, tools).  Under torch.cuda.graph the library cannot allocate the report's workspace: call
        prepare_lookup_inputs(k, n_sets, stream) with the capturing stream first."""
        lib = load_theta_library()
        torch = self._torch()
        k, n_sets = int(k), int(n_sets)
        stride = column_stride(layout, 1)
        if n_blocks is None:
            n_blocks = int(witness.y.numel()) // stride if stride else 0
        for i, t in enumerate(witness[:3]):
            if int(self._u8(t, "witness").numel()) < n_blocks * column_stride(layout, i):
                raise ValueError("witness holds fewer than n_blocks blocks")
        ks = self._key_slabs(key_witness, 1) if key_witness is not None else None
        _out = self._output(_out, "_out", argument_shape(k, n_sets), "int32")
        if not torch.cuda.is_current_stream_capturing():  # the report's workspace: a capture needs it in place already
            self._check(lib.aesw_theta_prepare(self._h, k, n_sets, self._stream()), "aesw_theta_prepare")
        rep = torch.empty(3, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_theta_inputs_device(self._h, k, n_sets, int(n_blocks), layout, *[t.data_ptr() if n_blocks else None for t in witness[:3]],
                                          _ptr(ks), _out.data_ptr(), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_theta_inputs_device")
        return _out, self._report(rep, sync, mult_report_dict)

    def prepare_lookup_inputs(self, k: int, n_sets: int, stream=None):
        """aesw_theta_prepare: the workspace lookup_inputs needs for a circuit of (k, n_sets) on `stream` (a torch stream; default
        the current one), made ahead of a capture on that stream.  It is never freed or moved afterwards."""
        handle = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        self._check(load_theta_library().aesw_theta_prepare(self._h, int(k), int(n_sets), handle), "aesw_theta_prepare")

    def argument_columns(self, index, table_fr, k: int, n_sets: int, n_rows: int | None = None, pad_row: int = 0, out=None):
        """A column of all 5 * n_sets lookup arguments as Fr cells (aesw_theta_columns_device): uint8 [n_sets, 5, 2^k, 32] with
        out[s, t - 1, i] = table_fr[j(t)][index[s, t - 1, i]] for i < n_rows (default 2^k; the rest is not written), j the table
        of the argument's arity.  index: an int32 [n_sets, 5, 2^k] tensor -- lookup_inputs, or a or s of permuted_columns; an
        index outside the table gives a cell of zeros -- or None for the table column in row order: row i for i < 66561, pad_row
        behind it.  table_fr: what compress_table returns."""
        lib = load_theta_library()
        k, n_sets = int(k), int(n_sets)
        shape = argument_shape(k, n_sets)
        if index is not None:
            self._tensor(index, "index", "int32", shape, alt=", or None")
        self._tensor(table_fr, "table_fr", shape=TABLE_FR_SHAPE)
        out = self._output(out, "out", shape + (32,))
        rc = lib.aesw_theta_columns_device(self._h, k, n_sets, (1 << k) if n_rows is None else int(n_rows), int(pad_row),
                                           None if index is None else index.data_ptr(), table_fr.data_ptr(), out.data_ptr(), self._stream())
        self._check(rc, "aesw_theta_columns_device")
        return out

    def invert_table(self, table_fr, beta, gamma, sync: bool = True, _out=None):
        """The inverse table of the lookup grand product (aesw_grand_invert_table_device, libaesw_grand.so): (inv_fr, report) with
        inv_fr a uint8 [2, 3, 66561, 32] tensor -- plane 0 inv(table_fr[j][r] + beta), plane 1 inv(table_fr[j][r] + gamma), inv(0)
        = 0 -- and report the dict of grand_invert_report_dict after synchronising the stream, or with sync=False the uint64[3]
        device tensor.  table_fr: what compress_table returns.  beta, gamma: ints (reduced mod r and put into Montgomery form
        here), or uint8[32] tensors on the device holding the cells as they lie, read when the kernel runs; if one is not
        canonical every cell is zero and the report says so.  _out is a tensor to write into (tests, tools)."""
        lib = load_grand_library()
        torch = self._torch()
        self._tensor(table_fr, "table_fr", shape=TABLE_FR_SHAPE)
        beta, gamma = self._challenge(beta, "beta"), self._challenge(gamma, "gamma")
        _out = self._output(_out, "_out", INV_FR_SHAPE)
        rep = torch.empty(3, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_grand_invert_table_device(self._h, table_fr.data_ptr(), beta.data_ptr(), gamma.data_ptr(), _out.data_ptr(), rep.data_ptr(),
                                                self._stream())
        self._check(rc, "aesw_grand_invert_table_device")
        return _out, self._report(rep, sync, grand_invert_report_dict)

    def grand_product(self, k: int, n_sets: int, inputs, a, s, table_fr, inv_fr, beta, gamma, n_rows: int | None = None, pad_row: int = 0,
                      sync: bool = True, _out=None, _workspace=None):
        """The grand product Z of all 5 * n_sets lookup arguments of one circuit (aesw_grand_product_device): (z, closing, report)
        with z a uint8 [n_sets, 5, 2^k, 32] tensor of which rows 0 ... min(n_rows, 2^k - 1) are written (n_rows: the usable rows,
        default 2^k; row n_rows holds the closing product, the rest is the host's blinding rows), closing the uint8 [n_sets, 5, 32]
        closing products and report the dict of grand_report_dict after synchronising the stream, or with sync=False the
        uint64[3] device tensor.  inputs: the int32 [n_sets, 5, 2^k] index column of lookup_inputs; a, s: those of
        permuted_columns; table_fr: what compress_table returns; inv_fr: what invert_table returns for the same beta and gamma
        (ints, or uint8[32] device tensors read when the kernels run).  The workspace is allocated per call and handed back to
        the caching allocator in stream order; _workspace is a uint8 tensor of workspace_bytes to use instead (a capture that
        prepares it beforehand), _out a (z, closing) pair to write into (tests, tools)."""
        lib = load_grand_library()
        torch = self._torch()
        k, n_sets = int(k), int(n_sets)
        shape = argument_shape(k, n_sets)
        for name, t in (("inputs", inputs), ("a", a), ("s", s)):
            self._tensor(t, name, "int32", shape)
        self._tensor(table_fr, "table_fr", shape=TABLE_FR_SHAPE)
        self._tensor(inv_fr, "inv_fr", shape=INV_FR_SHAPE)
        beta, gamma = self._challenge(beta, "beta"), self._challenge(gamma, "gamma")
        z, closing = (None, None) if _out is None else _out[:2]
        _out = (self._output(z, "_out", shape + (32,)), self._output(closing, "_out", shape[:2] + (32,)))
        _workspace = self._workspace(_workspace, int(lib.aesw_grand_workspace_bytes(k, n_sets)))
        rep = torch.empty(3, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_grand_product_device(self._h, k, n_sets, (1 << k) if n_rows is None else int(n_rows), int(pad_row), inputs.data_ptr(), a.data_ptr(),
                                           s.data_ptr(), table_fr.data_ptr(), inv_fr.data_ptr(), beta.data_ptr(), gamma.data_ptr(), _out[0].data_ptr(),
                                           _out[1].data_ptr(), _workspace.data_ptr(), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_grand_product_device")
        return _out[0], _out[1], self._report(rep, sync, grand_report_dict)

    def permutation_tables(self, k: int, n_cols: int, _out=None):
        """The power tables of the permutation argument (aesw_sigma_tables_device, libaesw_sigma.so), challenge free, once per
        (k, n_cols): a uint8 [2^min(k, 14) + 2^max(k - 14, 0) + n_cols, 32] tensor -- omega^j, omega^(j * 2^14), delta^c."""
        lib = load_sigma_library()
        k, n_cols = int(k), int(n_cols)
        need = int(lib.aesw_sigma_tables_bytes(k, n_cols)) if 0 <= k < 2 ** 32 and 0 <= n_cols < 2 ** 32 else 0
        _out = self._output(_out, "_out", (max(need, 32) // 32, 32), min_bytes=need)
        rc = lib.aesw_sigma_tables_device(self._h, k, n_cols, _out.data_ptr(), self._stream())
        self._check(rc, "aesw_sigma_tables_device")
        return _out

    def permutation_product(self, k: int, n_cols: int, chunk_len: int, advice_bytes, fixed_bytes, source, mapping, tables, beta, gamma,
                            n_rows: int | None = None, sync: bool = True, _out=None, _workspace=None):
        """The grand products Z of the permutation argument (aesw_sigma_product_device): (z, closing, report) with z a uint8
        [S, 2^k, 32] tensor, S = ceil(n_cols / chunk_len), of which rows 0 ... min(n_rows, 2^k - 1) are written (n_rows: the usable
        rows, default 2^k), closing the uint8 [S, 32] cells Z_s[n_rows] and report the dict of sigma_report_dict after
        synchronising the stream, or with sync=False the uint64[6] device tensor.  advice_bytes: uint8 [n_advice, 2^k], what
        assemble_advice gives with as_fr=False; fixed_bytes: uint8 [n_fixed, 2^k] or None; source: the uint32 [n_cols] column
        choice (permutation_sources; a numpy array or an int32 device tensor); mapping: the [n_cols, 2^k] cell indices
        (permutation_mapping; a numpy array is uploaded, an int32 device tensor stays); tables: what permutation_tables returns;
        beta, gamma: ints, or uint8[32] device tensors read when the kernels run.  _workspace: a uint8 tensor of
        aesw_sigma_workspace_bytes to use (a capture), _out a (z, closing) pair to write into (tests, tools)."""
        lib = load_sigma_library()
        torch = self._torch()
        k, n_cols, chunk_len = int(k), int(n_cols), int(chunk_len)
        rows = 1 << k if 0 <= k <= 28 else 0
        source, mapping = self._index_words(source, "source", (n_cols,)), self._index_words(mapping, "mapping", (n_cols, rows))
        n_advice = n_fixed = 0
        if advice_bytes is not None:
            n_advice = self._tensor(advice_bytes, "advice_bytes", shape=(None, rows)).shape[0]
        if fixed_bytes is not None:
            n_fixed = self._tensor(fixed_bytes, "fixed_bytes", shape=(None, rows)).shape[0]
        self._tensor(tables, "tables", min_bytes=int(lib.aesw_sigma_tables_bytes(k, n_cols)) if k >= 0 and n_cols >= 0 else 0)
        beta, gamma = self._challenge(beta, "beta"), self._challenge(gamma, "gamma")
        sets = -(-n_cols // chunk_len) if 1 <= chunk_len <= 8 and n_cols > 0 else 0
        z, closing = (None, None) if _out is None else _out[:2]
        _out = (self._output(z, "_out", (sets, rows, 32)), self._output(closing, "_out", (sets, 32)))
        need = int(lib.aesw_sigma_workspace_bytes(k, n_cols, chunk_len)) if k >= 0 and n_cols >= 0 and chunk_len >= 0 else 0
        _workspace = self._workspace(_workspace, need)
        rep = torch.empty(6, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_sigma_product_device(self._h, k, n_cols, chunk_len, rows if n_rows is None else int(n_rows),
                                           None if advice_bytes is None else advice_bytes.data_ptr(), n_advice,
                                           None if fixed_bytes is None else fixed_bytes.data_ptr(), n_fixed, source.data_ptr(), mapping.data_ptr(),
                                           tables.data_ptr(), beta.data_ptr(), gamma.data_ptr(), _out[0].data_ptr(), _out[1].data_ptr(), _workspace.data_ptr(),
                                           rep.data_ptr(), self._stream())
        self._check(rc, "aesw_sigma_product_device")
        return _out[0], _out[1], self._report(rep, sync, sigma_report_dict)

    def ntt_tables(self, max_k: int, _out=None):
        """The twiddle tables of the transforms below (aesw_ntt_tables_device, libaesw_ntt.so), once per max_k (10 ... 28): a uint8
        [cells, 32] tensor that serves every transform of size up to 2^max_k."""
        lib = load_ntt_library()
        max_k = int(max_k)
        need = int(lib.aesw_ntt_tables_bytes(max_k)) if 0 <= max_k < 2 ** 32 else 0
        if not need:
            raise AeswError(ERR_INVALID_ARG, "aesw_ntt_tables_device: max_k must be 10 ... 28")
        _out = self._output(_out, "_out", (need // 32, 32), nbytes=need)
        rc = lib.aesw_ntt_tables_device(self._h, max_k, _out.data_ptr(), self._stream())
        self._check(rc, "aesw_ntt_tables_device")
        return _out

    def _ntt(self, call, leading, cells, k_in, k_out, tables, out, _workspace=None):
        """One transform, `leading` the call's arguments in front of n_cols: `cells` a uint8 [n_cols, 2^k_in, 32] tensor (or [2^k_in, 32], one column), the result of the same rank with
        2^k_out rows.  out: the tensor to write into -- `cells` itself for a call in place --, default a new one.  max_k is what
        `tables` was built for (its size says which).  The workspace of a call in place is allocated here and handed back to the
        caching allocator in stream order; _workspace is a uint8 tensor to use instead (a capture)."""
        lib = load_ntt_library()
        k_in, k_out = int(k_in), int(k_out)
        if not 10 <= k_in <= k_out <= 28:
            raise AeswError(ERR_INVALID_ARG, call + ": k (and ext_k, no smaller) must be 10 ... 28")
        n_cols = self._columns(cells, "cells", k_in)
        tables_bytes = self._tensor(tables, "tables").numel()
        max_k = next((m for m in range(k_out, 29) if int(lib.aesw_ntt_tables_bytes(m)) == tables_bytes), None)
        if max_k is None:
            raise ValueError("tables must be what ntt_tables(max_k) returns for a max_k of at least %d" % k_out)
        out = self._output(out, "out", tuple(cells.shape[:-2]) + (1 << k_out, 32))
        need = int(lib.aesw_ntt_workspace_bytes(k_out, n_cols)) if out.data_ptr() == cells.data_ptr() else 0
        if need:
            _workspace = self._workspace(_workspace, need)
        rc = getattr(lib, call)(self._h, *[int(v) for v in leading], n_cols, cells.data_ptr(), out.data_ptr(), tables.data_ptr(), max_k,
                                None if _workspace is None else _workspace.data_ptr(), self._stream())
        self._check(rc, call)
        return out

    def lagrange_to_coeff(self, cells, k: int, tables, out=None, _workspace=None):
        """aesw_ntt_lagrange_to_coeff_device: the evaluations of a column on {omega_k^i} -> its 2^k coefficients (halo2's
        lagrange_to_coeff, the 1/2^k included).  cells: uint8 [n_cols, 2^k, 32] or [2^k, 32] Montgomery cells, canonical; tables:
        what ntt_tables returns; out=cells transforms in place."""
        return self._ntt("aesw_ntt_lagrange_to_coeff_device", (k,), cells, k, k, tables, out, _workspace)

    def coeff_to_lagrange(self, coeff, k: int, tables, out=None, _workspace=None):
        """aesw_ntt_coeff_to_lagrange_device: the inverse of lagrange_to_coeff."""
        return self._ntt("aesw_ntt_coeff_to_lagrange_device", (k,), coeff, k, k, tables, out, _workspace)

    def coeff_to_extended(self, coeff, k: int, ext_k: int, tables, zeta_sel: int = 1, out=None):
        """aesw_ntt_coeff_to_extended_device: 2^k coefficients -> the 2^ext_k evaluations on zeta * {omega_ext^i} (halo2's
        coeff_to_extended).  zeta_sel 0: g^((r - 1) / 3), 1: its square -- which of them halo2 uses is not pinned (include/aesw_ntt.h)."""
        return self._ntt("aesw_ntt_coeff_to_extended_device", (k, ext_k, zeta_sel), coeff, k, ext_k, tables, out)

    def extended_to_coeff(self, ext, ext_k: int, tables, zeta_sel: int = 1, out=None, _workspace=None):
        """aesw_ntt_extended_to_coeff_device: 2^ext_k evaluations on the coset -> 2^ext_k coefficients (halo2's extended_to_coeff
        without the truncation); out=ext transforms in place."""
        return self._ntt("aesw_ntt_extended_to_coeff_device", (ext_k, zeta_sel), ext, ext_k, ext_k, tables, out, _workspace)

    def permutation_columns_fr(self, k: int, n_cols: int, mapping, sigma_tables, _out=None):
        """Sigma as Fr cells (aesw_quot_sigma_fr_device): a uint8 [n_cols, 2^k, 32] tensor, cell [c][i] the label delta^c' * omega^i'
        of mapping[c][i] = c' * 2^k + i' -- the Lagrange form of halo2's permutation polynomials; an entry out of range reads as the
        cell itself.  mapping: the [n_cols, 2^k] cell indices (permutation_mapping; a numpy array is uploaded, an int32 device
        tensor stays); sigma_tables: what permutation_tables returns for the same (k, n_cols)."""
        lib = load_quot_library()
        k, n_cols = int(k), int(n_cols)
        need = int(load_sigma_library().aesw_sigma_tables_bytes(k, n_cols)) if 0 <= k < 2 ** 32 and 0 <= n_cols < 2 ** 32 else 0
        if not need:
            raise AeswError(ERR_INVALID_ARG, "aesw_quot_sigma_fr_device: k must be 10 ... 28, n_cols 1 ... 3074 and n_cols * 2^k at most 2^32")
        mapping = self._index_words(mapping, "mapping", (n_cols, 1 << k))
        self._tensor(sigma_tables, "sigma_tables", min_bytes=need)
        _out = self._output(_out, "_out", (n_cols, 1 << k, 32))
        rc = lib.aesw_quot_sigma_fr_device(self._h, k, n_cols, mapping.data_ptr(), sigma_tables.data_ptr(), _out.data_ptr(), self._stream())
        self._check(rc, "aesw_quot_sigma_fr_device")
        return _out

    def _open_columns(self, call, coeff, k):
        """(k, n_cols) of `coeff`, a uint8 [n_cols, 2^k, 32] tensor of coefficient columns (or [2^k, 32], one column)"""
        k = int(k)
        if not 10 <= k <= 28:
            raise AeswError(ERR_INVALID_ARG, call + ": k must be 10 ... 28")
        return k, self._columns(coeff, "coeff", k)

    def _open_workspace(self, k, n_cols, n_points, _workspace):
        return self._workspace(_workspace, int(load_open_library().aesw_open_workspace_bytes(k, n_cols, n_points)) if n_cols < 2 ** 32 else 0)

    def evaluate_columns(self, coeff, k: int, points, out=None, _workspace=None):
        """aesw_open_evaluate_device (libaesw_open.so): every coefficient column at every point, halo2's eval_polynomial -- a uint8
        [n_cols, n_points, 32] tensor of cells ([n_points, 32] for a coeff of one column, [2^k, 32]), cell [c][p] = sum_i
        coeff[c][i] * z_p^i.  coeff: uint8 [n_cols, 2^k, 32] Montgomery cells (what lagrange_to_coeff returns); points: 1 ... 16 of
        them -- ints, the cells rotated_points returns, or a uint8 [n_points, 32] tensor on the device, read when the kernels run.
        out: the tensor to write into; _workspace: a uint8 tensor to use instead of a fresh one (a capture)."""
        call = "aesw_open_evaluate_device"
        lib = load_open_library()
        k, n_cols = self._open_columns(call, coeff, k)
        points = self._cells(points, "points")
        n_points = points.shape[0]
        out = self._output(out, "out", tuple(coeff.shape[:-2]) + (n_points, 32))
        _workspace = self._open_workspace(k, n_cols, n_points, _workspace)
        rc = lib.aesw_open_evaluate_device(self._h, k, n_cols, n_points, coeff.data_ptr(), points.data_ptr(), out.data_ptr(), _workspace.data_ptr(), self._stream())
        self._check(rc, call)
        return out

    def fold_columns(self, coeff, k: int, v, acc=None, out=None):
        """aesw_open_fold_device: the columns of coeff folded under v, cell by cell -- a uint8 [2^k, 32] tensor, cell i =
        (...((acc[i] * v + coeff[0][i]) * v + coeff[1][i])...) * v + coeff[n_cols - 1][i]; acc: a uint8 [2^k, 32] tensor, or None
        for zero; out=acc folds into acc itself, so columns of separate tensors are folded by successive calls.  v: an int or a
        uint8 [32] tensor on the device, read when the kernel runs.  The order is not pinned against halo2 (include/aesw_open.h)."""
        call = "aesw_open_fold_device"
        lib = load_open_library()
        k, n_cols = self._open_columns(call, coeff, k)
        v = self._cells(v, "v", one=True)
        if acc is not None:
            self._tensor(acc, "acc", shape=(1 << k, 32))
        out = self._output(out, "out", (1 << k, 32))
        rc = lib.aesw_open_fold_device(self._h, k, n_cols, coeff.data_ptr(), v.data_ptr(), None if acc is None else acc.data_ptr(), out.data_ptr(), self._stream())
        self._check(rc, call)
        return out

    def divide_columns(self, coeff, k: int, point, out=None, _rem=None, _workspace=None):
        """aesw_open_divide_device: (quot, rem) -- quot of coeff's shape, the coefficients of (p_c(X) - p_c(z)) / (X - z) for every
        column c (halo2's kate_division of poly - eval; the last coefficient is 0), and rem a uint8 [n_cols, 32] tensor ([32] for
        one column), p_c(z).  point: one int or a uint8 [32] tensor on the device.  out=coeff divides in place."""
        call = "aesw_open_divide_device"
        lib = load_open_library()
        k, n_cols = self._open_columns(call, coeff, k)
        point = self._cells(point, "point", one=True)
        out = self._output(out, "out", tuple(coeff.shape))
        _rem = self._output(_rem, "_rem", tuple(coeff.shape[:-2]) + (32,))
        _workspace = self._open_workspace(k, n_cols, 1, _workspace)
        rc = lib.aesw_open_divide_device(self._h, k, n_cols, coeff.data_ptr(), point.data_ptr(), out.data_ptr(), _rem.data_ptr(), _workspace.data_ptr(), self._stream())
        self._check(rc, call)
        return out, _rem

    def msm_basis(self, points, out=None, _report=None):
        """aesw_msm_basis_device (libaesw_msm.so): the basis a commitment is taken against -- a uint8 [2^k, 64] tensor of points in
        Montgomery form -- from the plain little-endian coordinates a params file holds, uint8 [2^k, 64], x then y: a numpy array
        or a tensor on the device.  Every point is checked (both coordinates below q, on the curve); a bad one raises AeswError
        with their count and the index of the first.  out=points converts a device tensor in place.  Waits for the stream."""
        call = "aesw_msm_basis_device"
        lib = load_msm_library()
        points, k = self._points(points, "points")
        out = self._output(out, "out", (1 << k, 64))
        _report = self._output(_report, "_report", (16,))
        rc = lib.aesw_msm_basis_device(self._h, k, points.data_ptr(), out.data_ptr(), _report.data_ptr(), self._stream())
        self._check(rc, call)
        bad, first = self._report(_report, True, lambda rep: _words(rep.view(self._torch().int64)))
        if bad:
            raise AeswError(ERR_INVALID_ARG, "%s: %d of the 2^%d points are not on the curve or not below q, the first at index %d" % (call, bad, k, first))
        return out

    def commit_columns(self, scalars, basis, *, out=None, slices: int = 0, _workspace=None):
        """aesw_msm_commit_device: the commitments of columns against a basis, C_j = sum_i scalars[j][i] * basis[i] over bn256's G1 --
        a uint8 [n_cols, 64] tensor of affine points in Montgomery form, 64 zero bytes for the identity (g1_from_cells reads
        them).  scalars: uint8 [n_cols, 2^k, 32], columns of Fr cells, or uint8 [n_cols, 2^k], columns of bytes (an assembled advice
        column as it lies: one window of the method).  basis: uint8 [2^k, 64], what msm_basis returns.  slices: 0 for the
        library's own count, else how many runs the rows are cut into -- the time changes, never the result.  out: the tensor to
        write into; _workspace: a uint8 tensor to use instead of a fresh one (a capture)."""
        call = "aesw_msm_commit_device"
        lib = load_msm_library()
        basis, k = self._points(basis, "basis")
        self._tensor(scalars, "scalars", shape=[(None, 1 << k, 32), (None, 1 << k)])
        kind, n_cols, slices = MSM_FR if scalars.dim() == 3 else MSM_BYTES, scalars.shape[0], int(slices)
        need = int(lib.aesw_msm_workspace_bytes(k, n_cols, kind, slices)) if 0 <= slices < 2 ** 32 and 0 < n_cols < 2 ** 32 else 0
        if not need:
            raise AeswError(ERR_INVALID_ARG, call + ": n_cols must be 1 ... 65535 and slices 0 ... 2^k / 16, at most 65535")
        out = self._output(out, "out", (n_cols, 64))
        _workspace = self._workspace(_workspace, need)
        rc = lib.aesw_msm_commit_device(self._h, k, n_cols, kind, slices, scalars.data_ptr(), basis.data_ptr(), out.data_ptr(), _workspace.data_ptr(), self._stream())
        self._check(rc, call)
        return out

    def shplonk_table(self, scalars, table: str, set: int = 0, cells: int = 1):
        """The `cells` cells of `table` (a name of SHPLONK_TABLES) that belong to set `set` in the scalars block shplonk_prepare
        returns, as a uint8 [cells, 32] view: aesw_shplonk_scalars_offset says where they lie."""
        at = int(load_shplonk_library().aesw_shplonk_scalars_offset(SHPLONK_TABLES.index(table), int(set)))
        if at == C.c_size_t(-1).value:
            raise AeswError(ERR_INVALID_ARG, "shplonk_table: no set %d in table %s" % (set, table))
        return self._tensor(scalars, "scalars", min_bytes=at + 32 * cells).view(-1)[at:at + 32 * cells].view(cells, 32)

    def shplonk_prepare(self, plan, points, evals, y, v, _scalars=None, _report=None):
        """aesw_shplonk_prepare_device (libaesw_shplonk.so): the small phase of SHPLONK's multi-opening after y and v -- (scalars,
        report), a uint8 block that holds the plan and the tables y^j, v^i, e_is, w_is, v^i w_is and -R_i (shplonk_table reads
        them) and an int64 [8] report, reset (shplonk_report_dict reads it).  plan: what multiopen_plan returns.  points: the
        super set, len(plan.rotations) cells -- ints, the cells rotated_points returns, or a uint8 [n, 32] tensor on the device;
        evals: the evaluations in plan.eval_order(), likewise; y, v: ints or uint8 [32] tensors on the device (what
        Transcript.squeeze returns).  All are read when the kernel runs.  Parity with halo2 is not pinned (include/aesw_shplonk.h)."""
        call = "aesw_shplonk_prepare_device"
        lib = load_shplonk_library()
        points = self._tensor(self._cells(points, "points"), "points", shape=(len(plan.rotations), 32))
        evals = self._tensor(self._cells(evals, "evals"), "evals", shape=(len(plan.eval_order()), 32))
        y, v = self._challenge(y, "y"), self._challenge(v, "v")
        n_sets, max_cols = len(plan.sets), max(plan.set_cols, default=0)
        need = int(lib.aesw_shplonk_scalars_bytes(n_sets, max_cols)) if n_sets < 2 ** 32 and max_cols < 2 ** 32 else 0
        if not need:
            raise AeswError(ERR_INVALID_ARG, call + ": a plan has 1 ... 16 sets of 1 ... 65535 columns")
        _scalars = self._output(_scalars, "_scalars", (need,), min_bytes=need)
        _report = self._output(_report, "_report", (8,), "int64")
        words = [(C.c_uint32 * max(len(a), 1))(*a) for a in (plan.set_points, plan.set_cols, plan.point_index)]
        rc = lib.aesw_shplonk_prepare_device(self._h, len(plan.rotations), n_sets, *words, points.data_ptr(), evals.data_ptr(), y.data_ptr(), v.data_ptr(),
                                             _scalars.data_ptr(), _report.data_ptr(), self._stream())
        self._check(rc, call)
        return _scalars, _report

    def shplonk_finish(self, points, u, scalars, report):
        """aesw_shplonk_finish_device: the small phase after u -- z_i, z_T, z_0^-1, the coefficients of L' = z_0^-1 L, its constant
        and its low cells written into the `scalars` shplonk_prepare returned; word 3 of `report` set.  Returns scalars."""
        call = "aesw_shplonk_finish_device"
        lib = load_shplonk_library()
        points, u = self._cells(points, "points"), self._challenge(u, "u")
        self._tensor(scalars, "scalars", min_bytes=int(lib.aesw_shplonk_scalars_bytes(1, 1)))
        self._tensor(report, "report", "int64", (8,))
        self._check(lib.aesw_shplonk_finish_device(self._h, points.data_ptr(), u.data_ptr(), scalars.data_ptr(), report.data_ptr(), self._stream()), call)
        return scalars

    def combine_columns(self, coeff, k: int, coefs, low=None, acc=None, out=None):
        """aesw_shplonk_combine_device: a uint8 [2^k, 32] tensor, cell r = acc[r] + sum_j coefs[j] * coeff[j][r], plus low[r] for
        r < len(low) <= 8.  coefs: one cell per column, low: the low cells or None -- ints, numpy cells or uint8 [n, 32] tensors on
        the device (shplonk_table's views), read when the kernel runs; acc: a uint8 [2^k, 32] tensor, or None for zero; out=acc
        adds into acc itself, so columns of separate tensors take successive calls."""
        call = "aesw_shplonk_combine_device"
        lib = load_shplonk_library()
        k, n_cols = self._open_columns(call, coeff, k)
        coefs = self._tensor(self._cells(coefs, "coefs"), "coefs", shape=(n_cols, 32))
        low = None if low is None else self._cells(low, "low")
        if acc is not None:
            self._tensor(acc, "acc", shape=(1 << k, 32))
        out = self._output(out, "out", (1 << k, 32))
        rc = lib.aesw_shplonk_combine_device(self._h, k, n_cols, coeff.data_ptr(), coefs.data_ptr(), None if low is None else low.data_ptr(),
                                             0 if low is None else low.shape[0], None if acc is None else acc.data_ptr(), out.data_ptr(), self._stream())
        self._check(rc, call)
        return out

    def set_quotient(self, numer, k: int, set: int, points, scalars, report, acc=None, out=None, _rem=None, _workspace=None):
        """aesw_shplonk_quotient_device: (out, rem) -- out a uint8 [2^k, 32] tensor, acc + v^i Q_i for set i = `set` of the plan in
        `scalars`, Q_i the partial-fraction sum over the set's points of the quotients of numer = N_i (a uint8 [2^k, 32] tensor);
        rem a uint8 [8, 32] tensor whose first t_i cells are N_i at the set's points.  out=acc accumulates h over the sets,
        out=numer divides in place.  A remainder that is not 0 adds the set to `report`."""
        call = "aesw_shplonk_quotient_device"
        lib = load_shplonk_library()
        k, _one = self._open_columns(call, numer, k)
        self._tensor(numer, "numer", shape=(1 << k, 32))
        points = self._cells(points, "points")
        self._tensor(scalars, "scalars", min_bytes=int(lib.aesw_shplonk_scalars_bytes(1, 1)))
        self._tensor(report, "report", "int64", (8,))
        if acc is not None:
            self._tensor(acc, "acc", shape=(1 << k, 32))
        out = self._output(out, "out", (1 << k, 32))
        _rem = self._output(_rem, "_rem", (8, 32))
        _workspace = self._workspace(_workspace, int(lib.aesw_shplonk_workspace_bytes(k)))
        rc = lib.aesw_shplonk_quotient_device(self._h, k, int(set), numer.data_ptr(), points.data_ptr(), scalars.data_ptr(), None if acc is None else acc.data_ptr(),
                                              out.data_ptr(), _rem.data_ptr(), _workspace.data_ptr(), report.data_ptr(), self._stream())
        self._check(rc, call)
        return out, _rem

    def open_shplonk(self, plan, columns, evals, points, transcript, basis, out=None, _report=None):
        """SHPLONK's multi-opening, the whole stage on the current stream with no host wait: (points, report) -- a uint8 [2, 64]
        tensor, the commitments [h] and [W] (what commit_columns returns), and the int64 [8] report (shplonk_report_dict reads it
        after a synchronise).  Squeezes y and v from `transcript`, prepares, makes N_i (combine_columns) and adds v^i Q_i to h
        (set_quotient) set by set, commits h, writes [h], squeezes u, finishes, combines L', divides it by (X - u) in place
        (divide_columns, the remainder into the report), commits W and writes [W]: 64 more proof bytes.  plan: multiopen_plan's;
        columns: one uint8 [m_i, 2^k, 32] tensor of coefficient columns per set, in the plan's order; evals and points as
        shplonk_prepare takes them; basis: uint8 [2^k, 64], what msm_basis returns.  It allocates (S + 2) columns of its own."""
        basis, k = self._points(basis, "basis")
        n_sets = len(plan.sets)
        if len(columns) != n_sets:
            raise ValueError("columns must hold one tensor per set of the plan")
        out = self._output(out, "out", (2, 64))
        points = self._cells(points, "points")
        y, v = transcript.squeeze(), transcript.squeeze()
        scalars, report = self.shplonk_prepare(plan, points, evals, y, v, _report=_report)
        work = self._output(None, "work", (n_sets + 1, 1 << k, 32))  # N_0 ... N_(S-1), then h
        for i, cols in enumerate(columns):
            self.combine_columns(cols, k, self.shplonk_table(scalars, "y_pow", cells=plan.set_cols[i]), low=self.shplonk_table(scalars, "neg_r", i, plan.set_points[i]),
                                 out=work[i])
            self.set_quotient(work[i], k, i, points, scalars, report, acc=work[n_sets] if i else None, out=work[n_sets])
        self.commit_columns(work[n_sets:], basis, out=out[:1])
        transcript.write_points(out[:1])
        u = transcript.squeeze()
        self.shplonk_finish(points, u, scalars, report)
        line = self.combine_columns(work, k, self.shplonk_table(scalars, "l_coef", cells=n_sets + 1), low=self.shplonk_table(scalars, "l_low", cells=8))
        self.divide_columns(line, k, u, out=line, _rem=report.view(self._torch().uint8)[SHPLONK_REPORT_LAST_REM:SHPLONK_REPORT_LAST_REM + 32])
        self.commit_columns(line.view(1, 1 << k, 32), basis, out=out[1:])
        transcript.write_points(out[1:])
        return out, report

    def vanishing_tables(self, k: int, ext_k: int, zeta_sel: int = 1, _out=None):
        """aesw_vanish_tables_device (libaesw_vanish.so): the tables of the quotient on the coset of (k, ext_k, zeta_sel), free of the
        challenges -- inv(x^n - 1) for the m values of x^n and the powers x_j is one product of -- as a uint8 tensor."""
        call = "aesw_vanish_tables_device"
        lib = load_vanish_library()
        k, ext_k, zeta_sel = int(k), int(ext_k), int(zeta_sel)
        need = int(lib.aesw_vanish_tables_bytes(k, ext_k)) if 0 <= k < 2 ** 32 and 0 <= ext_k < 2 ** 32 else 0
        if not need or not 0 <= zeta_sel <= 1:
            raise AeswError(ERR_INVALID_ARG, call + ": k must be 10 ... 28, ext_k k + 2 ... 28 and zeta_sel 0 or 1")
        _out = self._output(_out, "_out", (need,), min_bytes=need)
        self._check(lib.aesw_vanish_tables_device(self._h, k, ext_k, zeta_sel, _out.data_ptr(), self._stream()), call)
        return _out

    def vanishing_scalars(self, n_sets: int, chunk_len: int, theta, beta, gamma, y, _out=None):
        """aesw_vanish_scalars_device: the scalars block of the quotient's segments -- the challenges, y^len per segment kind, theta^2,
        theta^3, t * theta^(arity - 1) per tag, delta^first(s) and beta * delta^first(s) per permutation set -- as a uint8 tensor
        (vanishing_scalar reads it).  theta, beta, gamma, y: ints or uint8 [32] tensors on the device (what Transcript.squeeze
        returns), read when the kernel runs: a captured call follows new challenges."""
        call = "aesw_vanish_scalars_device"
        lib = load_vanish_library()
        n_sets, chunk_len = int(n_sets), int(chunk_len)
        need = int(lib.aesw_vanish_scalars_bytes(n_sets, chunk_len)) if 0 <= n_sets < 2 ** 32 and 0 <= chunk_len < 2 ** 32 else 0
        if not need:
            raise AeswError(ERR_INVALID_ARG, call + ": n_sets must be 1 ... 1024 and chunk_len 1 ... 8")
        theta, beta, gamma, y = (self._challenge(v, name) for v, name in ((theta, "theta"), (beta, "beta"), (gamma, "gamma"), (y, "y")))
        _out = self._output(_out, "_out", (need,), min_bytes=need)
        rc = lib.aesw_vanish_scalars_device(self._h, n_sets, chunk_len, theta.data_ptr(), beta.data_ptr(), gamma.data_ptr(), y.data_ptr(), _out.data_ptr(), self._stream())
        self._check(rc, call)
        return _out

    def vanishing_scalar(self, scalars, table: str, index: int = 0, cells: int = 1):
        """The `cells` cells from entry `index` of `table` (a name of VANISH_TABLES) in the block vanishing_scalars returns, as a
        uint8 [cells, 32] view: aesw_vanish_scalars_offset says where they lie (the entries of delta and beta_delta lie 64 bytes apart)."""
        at = int(load_vanish_library().aesw_vanish_scalars_offset(VANISH_TABLES.index(table), int(index)))
        if at == C.c_size_t(-1).value:
            raise AeswError(ERR_INVALID_ARG, "vanishing_scalar: no entry %d in table %s" % (index, table))
        return self._tensor(scalars, "scalars", min_bytes=at + 32 * cells).view(-1)[at:at + 32 * cells].view(cells, 32)

    def quotient_accumulator(self, k: int, ext_k: int, zeta_sel: int, n_sets: int, chunk_len: int, n_rows: int, tables, scalars, _acc=None) -> "QuotientAccumulator":
        """The quotient h(X) on the extended coset, one constraint segment per call (libaesw_vanish.so): an accumulator that owns the
        acc column and takes head(...), permutation_set(s, ...) for every permutation set, lookup_set(s, ...) for every column set
        and divide(), in that order -- each reads only its own extended columns, so a caller extends a group, folds it and uses
        the buffer again.  tables: what vanishing_tables returns for (k, ext_k, zeta_sel); scalars: what vanishing_scalars returns
        for (n_sets, chunk_len).  Neither the order of the constraints nor zeta is pinned against halo2 (include/aesw_vanish.h)."""
        return QuotientAccumulator(self, k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, tables, scalars, _acc)

    def quotient_extended(self, groups, k: int, ext_k: int, zeta_sel: int, n_sets: int, chunk_len: int, n_rows: int, theta, beta, gamma, y, tables=None, out=None):
        """The quotient over the ten column groups at once, for a caller that has every extended column resident: a uint8
        [2^ext_k, 32] tensor, halo2's evaluate_h.  groups: a dict by the names of QUOTIENT_GROUPS, or a sequence in their order, of
        uint8 [columns, 2^ext_k, 32] tensors (what coeff_to_extended returns).  Written on top of quotient_accumulator; the
        columns of a permutation set are gathered into a buffer of chunk_len columns, since they do not lie next to each other.
        It allocates that buffer, the scalars block and, without `tables`, the tables inside the call: capture the accumulator's own
        calls instead (quotient_accumulator with tensors made beforehand), as tests/test_gpu_vanish_calls.py does."""
        if not isinstance(groups, dict):
            groups = dict(zip(QUOTIENT_GROUPS, groups))
        if sorted(groups) != sorted(QUOTIENT_GROUPS):
            raise ValueError("groups must hold %s" % ", ".join(QUOTIENT_GROUPS))
        tables = self.vanishing_tables(k, ext_k, zeta_sel) if tables is None else tables
        acc = self.quotient_accumulator(k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, tables, self.vanishing_scalars(n_sets, chunk_len, theta, beta, gamma, y), _acc=out)
        n_sets, chunk_len, rows = acc.n_sets, acc.chunk_len, 1 << acc.ext_k
        count = {"advice": 3 * n_sets + 1, "rcon": 2, "selectors": 5 * n_sets, "table": 4, "sigma": 3 * n_sets + 2, "zperm": acc.perm_sets, "a": 5 * n_sets, "s": 5 * n_sets,
                 "zlookup": 5 * n_sets, "l": 3}
        for name in QUOTIENT_GROUPS:
            self._tensor(groups[name], name, shape=(count[name], rows, 32))
        acc.head(groups["advice"][3 * n_sets], groups["rcon"], groups["zperm"], groups["l"])
        values = self._output(None, "values", (chunk_len, rows, 32))
        for s in range(acc.perm_sets):
            first, end = s * chunk_len, min((s + 1) * chunk_len, 3 * n_sets + 2)
            for c in range(first, end):
                group, column = permutation_source(n_sets, c)
                values[c - first].copy_(groups[group][column])
            acc.permutation_set(s, values[:end - first], groups["sigma"][first:end], groups["zperm"][s], groups["l"])
        for s in range(n_sets):
            five = slice(5 * s, 5 * s + 5)
            acc.lookup_set(s, groups["advice"][3 * s:3 * s + 3], groups["selectors"][five], groups["table"], groups["a"][five], groups["s"][five], groups["zlookup"][five],
                           groups["l"])
        return acc.divide()

    def blinding_seed(self, seed: bytes | None = None):
        """The 32-byte seed of the blinding cells as the calls of libaesw_blind.so read it: a uint8 [32] tensor on the device, read
        when a kernel runs, so a captured graph follows a seed copied into it.  seed None: secrets.token_bytes(32), the operating
        system's randomness -- what a prover that wants zero knowledge passes.  A proof is reproducible from its seed."""
        if seed is None:
            import secrets
            seed = secrets.token_bytes(BLIND_SEED_BYTES)
        seed = bytes(seed)
        if len(seed) != BLIND_SEED_BYTES:
            raise ValueError("seed must be %d bytes" % BLIND_SEED_BYTES)
        return self._torch().from_numpy(np.frombuffer(seed, np.uint8).copy()).to(self._dev())

    def _blind_tail(self, call, k, n_cols, first_row, domain=0, first_column=0):
        """The arguments of a call of libaesw_blind.so as ints, and the rows of the tail; what the library would refuse of a size is
        an AeswError before anything is sized by it."""
        lib = load_blind_library()
        k, n_cols, first_row, domain, first_column = int(k), int(n_cols), int(first_row), int(domain), int(first_column)
        tail = int(lib.aesw_blind_tail_rows(k, first_row)) if 0 <= k < 2 ** 32 and 0 <= first_row < 2 ** 64 else 0
        if not tail or not 1 <= n_cols <= 65535 or not 0 <= domain < 2 ** 64 or not 0 <= first_column < 2 ** 64:
            raise AeswError(ERR_INVALID_ARG, call + ": k must be 10 ... 28, n_cols 1 ... 65535, first_row below 2^k, domain and first_column below 2^64")
        return lib, k, n_cols, first_row, domain, first_column, tail

    def blind_rows(self, cells, k: int, first_row: int, seed, domain: int, first_column: int = 0):
        """aesw_blind_rows_device (libaesw_blind.so): rows first_row ... 2^k - 1 of every column of `cells`, a uint8 [n_cols, 2^k, 32]
        (or [2^k, 32]) tensor of Fr cells, filled in place with blinding cells, and no other byte touched; returns `cells`.  A cell is
        BLAKE2b-512 keyed by `seed` (what blinding_seed returns) over (domain, first_column + j, row), reduced mod r
        (include/aesw_blind.h): `domain` is the caller's tag of this group of columns, so that groups under one seed share no cell."""
        call = "aesw_blind_rows_device"
        lib, k, _one, first_row, domain, first_column, _tail = self._blind_tail(call, k, 1, first_row, domain, first_column)
        n_cols = self._columns(cells, "cells", k)
        seed = self._tensor(seed, "seed", shape=(BLIND_SEED_BYTES,))
        self._check(lib.aesw_blind_rows_device(self._h, k, n_cols, first_row, domain, first_column, seed.data_ptr(), cells.data_ptr(), self._stream()), call)
        return cells

    def blinding_tail(self, k: int, n_cols: int, first_row: int, seed, domain: int, first_column: int = 0, out=None):
        """aesw_blind_tail_device: the same cells compactly, a uint8 [n_cols, 2^k - first_row, 32] tensor -- the tail of columns whose
        body is bytes (commit_blinded_bytes takes it)."""
        call = "aesw_blind_tail_device"
        lib, k, n_cols, first_row, domain, first_column, tail = self._blind_tail(call, k, n_cols, first_row, domain, first_column)
        seed = self._tensor(seed, "seed", shape=(BLIND_SEED_BYTES,))
        out = self._output(out, "out", (n_cols, tail, 32))
        self._check(lib.aesw_blind_tail_device(self._h, k, n_cols, first_row, domain, first_column, seed.data_ptr(), out.data_ptr(), self._stream()), call)
        return out

    def commit_tail(self, tail, k: int, first_row: int, basis, commitments):
        """aesw_blind_commit_tail_device: commitments[j] += sum_i tail[j][i] * basis[first_row + i], in place; returns `commitments`.
        tail: uint8 [n_cols, 2^k - first_row, 32], any canonical cells, at most 64 rows; basis: uint8 [2^k, 64], what msm_basis
        returns; commitments: uint8 [n_cols, 64], what commit_columns returns.  The scalars are secret: the kernel's double-and-add
        runs the same steps whatever they are."""
        call = "aesw_blind_commit_tail_device"
        n_cols = tail.shape[0] if hasattr(tail, "shape") and len(tail.shape) == 3 else 0
        lib, k, n_cols, first_row, _domain, _column, rows = self._blind_tail(call, k, n_cols, first_row)
        if rows > int(lib.aesw_blind_max_tail()):
            raise AeswError(ERR_INVALID_ARG, call + ": the tail, 2^k - first_row rows, must be at most %d" % int(lib.aesw_blind_max_tail()))
        basis = self._tensor(basis, "basis", shape=(1 << k, 64))
        tail = self._tensor(tail, "tail", shape=(n_cols, rows, 32))
        commitments = self._tensor(commitments, "commitments", shape=(n_cols, 64))
        self._check(lib.aesw_blind_commit_tail_device(self._h, k, n_cols, first_row, tail.data_ptr(), basis.data_ptr(), commitments.data_ptr(), self._stream()), call)
        return commitments

    def commit_blinded_bytes(self, byte_columns, tail, k: int, first_row: int, basis, out=None, _workspace=None):
        """The commitments of columns of bytes whose rows from first_row on are the cells of `tail`: commit_columns over the bytes --
        one 8-bit window, a thirty-second of the work of a column of cells -- then commit_tail in place: two enqueues and no wait.
        byte_columns: uint8 [n_cols, 2^k], the rows from first_row on zero (a byte left there is added to its tail cell); tail: uint8
        [n_cols, 2^k - first_row, 32] (blinding_tail).  Returns a uint8 [n_cols, 64] tensor: byte for byte what commit_columns gives
        for the same columns expanded to cells with blind_rows applied."""
        self._tensor(byte_columns, "byte_columns", shape=(None, 1 << int(k)) if 0 <= int(k) <= 28 else None)
        out = self.commit_columns(byte_columns, basis, out=out, _workspace=_workspace)
        return self.commit_tail(tail, k, first_row, basis, out)

    def transcript(self, proof_capacity: int = 0, _state=None, _proof=None) -> "Transcript":
        """A fresh Blake2b transcript on the device (libaesw_transcript.so): commitments and scalars go in where they lie,
        challenges come out as uint8 [32] device tensors that compress_table, invert_table, grand_product, permutation_product
        and fold_columns take as they are, and the write_ forms append the proof's bytes to a device buffer of proof_capacity
        bytes (0: none; the transcript then only derives challenges).  _state is a uint8 [256] tensor and _proof a uint8
        [proof_capacity] tensor to use instead of fresh ones (tests, a capture)."""
        return Transcript(self, proof_capacity, _state, _proof)

    def multiplicity_accumulator(self, k: int, n_sets: int, layout: int = K.LAYOUT_PACKED, _out=None) -> "MultiplicityAccumulator":
        """The lookup multiplicities of ONE FixedAes128Config<k, n_sets> circuit whose blocks arrive piece by piece
        (libaesw_acc.so): reset() once, then add() any contiguous run of the circuit's blocks, in any number of calls and in any
        order, and add_key() its key slab; histograms() is then what lookup_multiplicities gives over the whole circuit.  `layout`
        is the layout of every witness handed in; _out is an int32 [n_sets, 66561] tensor to count into (tests, tools)."""
        return MultiplicityAccumulator(self, k, n_sets, layout, _out)

    def check_columns(self, k: int, n_sets: int, pt, keys, advice, counts, ct=None, sync: bool = True, _offsets=None):
        """MockProver::assert_satisfied over the ASSEMBLED advice columns of C FixedAes128Config<k, n_sets> circuits in one launch
        (aesw_cols_check_device, libaesw_cols.so).  advice: what assemble_advice_circuits returns, [C, 3*n_sets+1, 2^k] bytes or
        [C, 3*n_sets+1, 2^k, 32] Fr cells (for C = 1 also assemble_advice's [3*n_sets+1, 2^k] / [..., 32]); pt uint8[n,16], keys
        uint8[C,16] or None, ct uint8[n,16] or None, counts / _offsets as for check_circuits.  Returns the dict of check_circuits
        plus cell_failures, unassigned_failures, first_cell (None or the absolute cell index) and cells; `satisfied` needs every
        failure count to be 0.  With sync=False the uint64[12] device tensor the report was written to."""
        lib = load_cols_library()
        torch = self._torch()
        pt = self._u8(pt, "pt")
        n = int(pt.shape[0])
        nc = len(counts)
        advice = self._u8(advice, "advice")
        ncol, rows = 3 * n_sets + 1, 1 << k
        shape = tuple(advice.shape)
        if shape in ((nc, ncol, rows), (nc, ncol, rows, 32)):
            as_fr = len(shape) == 4
        elif nc == 1 and shape in ((ncol, rows), (ncol, rows, 32)):
            as_fr = len(shape) == 3
        else:
            raise ValueError("advice must be [C, 3*n_sets+1, 2^k] bytes or [C, 3*n_sets+1, 2^k, 32] Fr cells")
        nc, d_offs = self._circuit_args(k, n_sets, n, counts, keys, _offsets)
        if ct is not None and tuple(self._u8(ct, "ct").shape) != (n, 16):
            raise ValueError("ct must be [n,16]")
        rep = torch.empty(12, dtype=torch.int64, device=self._dev())
        rc = lib.aesw_cols_check_device(
            self._h, k, n_sets, nc, d_offs.data_ptr(), n, pt.data_ptr() if n else None, _ptr(keys),
            ct.data_ptr() if ct is not None and n else None, 1 if as_fr else 0, advice.data_ptr(), rep.data_ptr(), self._stream())
        self._check(rc, "aesw_cols_check_device")
        return self._report(rep, sync, cols_report_dict)

    def circuits(self, k: int, n_sets: int, keys, pt, counts, as_fr: bool = True):
        """C FixedAes128Config<k, n_sets> circuits on torch's current stream: the key schedule of keys (uint8[C,16]), the
        witness of pt (uint8[n,16]; circuit c takes the next counts[c] blocks) with each block under its circuit's key, and
        the advice columns of every circuit in one launch.  Returns (witness, key_witness, advice): the PACKED block slabs and
        ciphertexts, the C key slabs and advice [C, 3*n_sets+1, 2^k] (bytes) or [..., 32] (Fr)."""
        n = int(pt.shape[0])
        _nc, d_offs = self._circuit_args(k, n_sets, n, counts, keys)  # counts first, then keys (uint8[C,16])
        torch = self._torch()
        kw = self.key_schedule_witness(keys, K.LAYOUT_PACKED, want_rk=False)
        # every block under its circuit's key: the per-block-key launch on the keys gathered by circuit (16 B per block)
        per_block = torch.repeat_interleave(keys, torch.as_tensor(counts, dtype=torch.int64, device=keys.device), dim=0)
        wit = self.encrypt_witness(pt, per_block, K.LAYOUT_PACKED, want_ct=True) if n else \
            self.alloc_witness(1, K.LAYOUT_PACKED, want_ct=True)  # no block: key rows only (the slabs are never read)
        adv = self.assemble_advice_circuits(k, n_sets, wit, kw, counts, as_fr=as_fr, n_blocks=n, _offsets=d_offs)
        return wit, kw, adv

    # -- host entry points (numpy in, numpy out)
    def encrypt_witness_host(self, pt: np.ndarray, keys: np.ndarray, layout: int = K.LAYOUT_PACKED,
                             want_ct: bool = False, key_slab: bool = False, out_cols=None):
        pt = np.ascontiguousarray(pt, dtype=np.uint8).reshape(-1, 16)
        n = pt.shape[0]
        if keys is None:  # the key given to schedule_key()
            pbk = 0
            if key_slab:
                raise ValueError("the key slab of a scheduled key is returned by schedule_key()")
        else:
            keys = np.ascontiguousarray(keys, dtype=np.uint8)
            pbk = 0 if keys.size == 16 else 1
            if pbk and keys.size != n * 16:
                raise ValueError("keys must hold 16 or n*16 bytes")
        cols = list(out_cols) if out_cols is not None else [np.empty(n * column_stride(layout, c), dtype=np.uint8)
                                                            for c in range(3)]
        ct = np.empty((n, 16), dtype=np.uint8) if want_ct else None
        key = ks = None
        if key_slab:
            m = n if pbk else 1
            key = KeyWitness(np.empty(m * K.WORDS_ROWS, np.uint8),
                             *[np.empty(m * key_column_stride(layout, c), np.uint8) for c in range(3)], None)
            ks = KeySlab(*[a.ctypes.data for a in key[:4]])
        rc = self._lib.aesw_encrypt_witness(self._h, _np_ptr(pt), _ptr(keys), pbk, n, layout,
                                            *[_np_ptr(c) for c in cols],
                                            _ptr(ct), _ptr(ks))
        self._check(rc, "aesw_encrypt_witness")
        return Witness(cols[0], cols[1], cols[2], ct, key)

    def encrypt_witness_stream(self, pt: np.ndarray, keys, consume, layout: int = K.LAYOUT_PACKED):
        """aesw_encrypt_witness_stream: consume(first_block, n_blocks, x, y, z) is called per chunk with
        numpy views of page-locked buffers (valid only during the call) while the next chunk is in flight."""
        pt = np.ascontiguousarray(pt, dtype=np.uint8).reshape(-1, 16)
        n = pt.shape[0]
        pbk = 0
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint8)
            pbk = 0 if keys.size == 16 else 1
        strides = [column_stride(layout, c) for c in range(3)]
        err = []

        @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))
        def cb(_user, first, count, x, y, z):
            try:
                cols = [np.ctypeslib.as_array(p, shape=(count * s,)) if s else np.empty(0, np.uint8)  # VALUES: no x
                        for p, s in zip((x, y, z), strides)]
                r = consume(int(first), int(count), *cols)
                return int(r or 0)
            except Exception as e:  # never let an exception cross the C boundary
                err.append(e)
                return 1

        rc = self._lib.aesw_encrypt_witness_stream(self._h, _np_ptr(pt), _ptr(keys), pbk, n,
                                                   layout, C.cast(cb, C.c_void_p), None)
        if err:
            raise err[0]
        self._check(rc, "aesw_encrypt_witness_stream")

    def last_stream_stats(self) -> dict:
        """Where the time of the last streaming call went (aesw_last_stream_stats)."""
        st = StreamStats()
        self._check(self._lib.aesw_last_stream_stats(self._h, C.byref(st)), "aesw_last_stream_stats")
        return st.as_dict()

    def assemble_advice_stream(self, k: int, n_sets: int, witness: "Witness", key_witness, n_blocks: int, consume,
                               layout: int = K.LAYOUT_PACKED, as_fr: bool = True):
        """aesw_assemble_advice_stream: consume(column, cells) per advice column with a numpy view of the page-locked
        buffer (2^k bytes, or [2^k, 32] Fr cells), valid only during the call, while the next column is in flight."""
        self._torch().cuda.current_stream(self.device).synchronize()  # the slabs must be complete
        err = []

        @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint64)
        def cb(_user, col, cells, n_cells):
            try:
                a = np.ctypeslib.as_array(cells, shape=(n_cells * (32 if as_fr else 1),))
                r = consume(int(col), a.reshape(n_cells, 32) if as_fr else a)
                return int(r or 0)
            except Exception as e:  # never let an exception cross the C boundary
                err.append(e)
                return 1

        ks = KeySlab(*[t.data_ptr() for t in key_witness[:4]]) if key_witness is not None else None
        rc = self._lib.aesw_assemble_advice_stream(
            self._h, k, n_sets, n_blocks, layout, witness.x.data_ptr(), witness.y.data_ptr(), witness.z.data_ptr(),
            _ptr(ks), 1 if as_fr else 0, C.cast(cb, C.c_void_p), None)
        if err:
            raise err[0]
        self._check(rc, "aesw_assemble_advice_stream")

    def assemble_advice_host(self, k: int, n_sets: int, witness: "Witness", key_witness, n_blocks: int, out: np.ndarray,
                             layout: int = K.LAYOUT_PACKED, as_fr: bool = True):
        """aesw_assemble_advice_host: all advice columns into the host array `out` ((3*n_sets+1) << k cells of 1 or 32 bytes);
        direct DMA when `out` is page-locked (api.host_alloc / host_register)."""
        self._torch().cuda.current_stream(self.device).synchronize()  # the slabs must be complete
        need = ((3 * n_sets + 1) << k) * (32 if as_fr else 1)
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.size < need:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % need)
        ks = KeySlab(*[t.data_ptr() for t in key_witness[:4]]) if key_witness is not None else None
        rc = self._lib.aesw_assemble_advice_host(
            self._h, k, n_sets, n_blocks, layout, witness.x.data_ptr(), witness.y.data_ptr(), witness.z.data_ptr(),
            _ptr(ks), 1 if as_fr else 0, _np_ptr(out))
        self._check(rc, "aesw_assemble_advice_host")
        return out

    def key_schedule_witness_host(self, keys: np.ndarray, layout: int = K.LAYOUT_PACKED) -> KeyWitness:
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
        n = keys.shape[0]
        w = np.empty(n * K.WORDS_ROWS, np.uint8)
        kx, ky, kz = [np.empty(n * key_column_stride(layout, c), np.uint8) for c in range(3)]
        rk = np.empty((n, 176), np.uint8)
        rc = self._lib.aesw_key_schedule_witness(self._h, _np_ptr(keys), n, layout, _np_ptr(w), _np_ptr(kx), _np_ptr(ky),
                                                 _np_ptr(kz), _np_ptr(rk))
        self._check(rc, "aesw_key_schedule_witness")
        return KeyWitness(w, kx, ky, kz, rk)

    def schedule_key_host(self, key, layout: int = K.LAYOUT_PACKED, key_slab: bool = True):
        """aesw_schedule_key: FixedAes128Config::schedule_key from 16 host bytes; later encrypt_witness_host(pt, None) calls use
        the key.  Returns its key slab (numpy KeyWitness, rk None) when key_slab."""
        key = np.ascontiguousarray(key, dtype=np.uint8).reshape(-1)
        if key.size != 16:
            raise ValueError("key must be 16 bytes")
        kw = ks = None
        if key_slab:
            kw = KeyWitness(np.empty(K.WORDS_ROWS, np.uint8), *[np.empty(key_column_stride(layout, c), np.uint8) for c in range(3)], None)
            ks = KeySlab(*[a.ctypes.data for a in kw[:4]])
        rc = self._lib.aesw_schedule_key(self._h, _np_ptr(key), layout, _ptr(ks))
        self._check(rc, "aesw_schedule_key")
        return kw

    def lookup_table_host(self) -> np.ndarray:
        t = np.empty((4, K.TABLE_ROWS), dtype=np.uint8)
        rc = self._lib.aesw_lookup_table(self._h, *[_np_ptr(t[i]) for i in range(4)])
        self._check(rc, "aesw_lookup_table")
        return t


def group_shard(members: int, n: int, i: int):
    """aesw_group_shard: (first, count) of member i's blocks in a batch of n (the ranges of sharding.shard_range)."""
    first, count = C.c_uint64(), C.c_uint64()
    rc = load_library().aesw_group_shard(members, n, i, C.byref(first), C.byref(count))
    if rc:
        raise AeswError(rc, "aesw_group_shard(%d, %d, %d)" % (members, n, i))
    return int(first.value), int(count.value)


def transcript_status_dict(rep) -> dict:
    """The report words of a transcript's state (include/aesw_transcript.h, words 26 ... 29)."""
    v = _words(rep)
    return {"proof_bytes": v[26], "proof_missed": v[27], "identities": v[28], "first_identity": None if v[29] == _NONE else v[29]}


class QuotientAccumulator:
    """What Context.quotient_accumulator returns: the fold of the quotient's constraints, cut into segments (include/aesw_vanish.h).
    It owns acc, a uint8 [2^ext_k, 32] tensor every segment folds into in place.  The segments come in the fold's order -- head,
    permutation_set(0) ... (S - 1), lookup_set(0) ... (n_sets - 1), divide -- and each once: another order is another
    polynomial, so it is refused (AeswError, nothing enqueued).  Every method is asynchronous on the current stream and
    allocates nothing, so the whole fold can be captured into one graph; restart() opens the next fold over the same acc."""

    def __init__(self, ctx: "Context", k, ext_k, zeta_sel, n_sets, chunk_len, n_rows, tables, scalars, _acc=None):
        self._lib = load_vanish_library()
        self.ctx = ctx
        self.k, self.ext_k, self.zeta_sel, self.n_sets, self.chunk_len, self.n_rows = (int(v) for v in (k, ext_k, zeta_sel, n_sets, chunk_len, n_rows))
        shape = (self.k, self.ext_k, self.zeta_sel, self.n_sets, self.chunk_len, self.n_rows)  # the bounds are the library's: csrc/aesw_quot.h's quot_shape_ok
        if not all(0 <= v < 2 ** 32 for v in shape) or not self._lib.aesw_vanish_shape_ok(*shape):
            raise AeswError(ERR_INVALID_ARG, "quotient_accumulator: k must be 10 ... 28 and ext_k k + 2 ... 28, zeta_sel 0 or 1, n_sets 1 ... 1024, chunk_len 1 ... 8 with "
                            "chunk_len + 2 <= 2^(ext_k - k) + 1, n_rows 1 ... 2^k - 1")
        self.perm_sets = permutation_sets(self.n_sets, self.chunk_len)
        self.tables = ctx._tensor(tables, "tables", min_bytes=int(self._lib.aesw_vanish_tables_bytes(self.k, self.ext_k)))
        self.scalars = ctx._tensor(scalars, "scalars", min_bytes=int(self._lib.aesw_vanish_scalars_bytes(self.n_sets, self.chunk_len)))
        self.acc = ctx._output(_acc, "_acc", (1 << self.ext_k, 32))
        self._order = [("head", 0)] + [("permutation_set", s) for s in range(self.perm_sets)] + [("lookup_set", s) for s in range(self.n_sets)] + [("divide", 0)]
        self._done = 0

    def restart(self):
        """The next fold over the same acc: head comes next again."""
        self._done = 0
        return self

    def _turn(self, segment, s=0):
        s = int(s)
        want = self._order[self._done] if self._done < len(self._order) else None
        if want != (segment, s):
            raise AeswError(ERR_INVALID_ARG, "quotient_accumulator: %s(%d) is out of order or given twice: %s" %
                            (segment, s, "the fold is complete" if want is None else "%s(%d) comes next" % want))
        return s

    def _group(self, t, name, columns):
        rows = 1 << self.ext_k
        return self.ctx._tensor(t, name, shape=[(columns, rows, 32), (rows, 32)] if columns == 1 else (columns, rows, 32))

    def _shape(self):
        return (self.k, self.ext_k, self.n_sets, self.chunk_len, self.n_rows)

    def head(self, words, rcon, zperm, l):
        """HEAD: the gate and the constraints that tie the permutation's grand products together.  words: the round-constant advice
        column, advice[3 n_sets]; rcon [2], zperm [S], l [3]: those groups extended.  It opens the fold: acc is written, not read."""
        call = "aesw_vanish_head_device"
        self._turn("head")
        words, rcon, zperm, l = self._group(words, "words", 1), self._group(rcon, "rcon", 2), self._group(zperm, "zperm", self.perm_sets), self._group(l, "l", 3)
        rc = self._lib.aesw_vanish_head_device(self.ctx._h, *self._shape(), words.data_ptr(), rcon.data_ptr(), zperm.data_ptr(), l.data_ptr(), self.scalars.data_ptr(),
                                               self.acc.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, call)
        self._done += 1
        return self

    def permutation_set(self, s: int, values, sigma, z, l):
        """PERM(s): the product constraint of permutation set s.  values, sigma: only the columns of that set, in the permutation's
        order (permutation_source says where column c lies), extended; z: Zp_s; l [3]."""
        call = "aesw_vanish_perm_device"
        s = self._turn("permutation_set", s)
        columns = min((s + 1) * self.chunk_len, 3 * self.n_sets + 2) - s * self.chunk_len
        values, sigma, z, l = self._group(values, "values", columns), self._group(sigma, "sigma", columns), self._group(z, "z", 1), self._group(l, "l", 3)
        rc = self._lib.aesw_vanish_perm_device(self.ctx._h, *self._shape(), s, values.data_ptr(), sigma.data_ptr(), z.data_ptr(), l.data_ptr(), self.tables.data_ptr(),
                                               self.scalars.data_ptr(), self.acc.data_ptr(), self.acc.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, call)
        self._done += 1
        return self

    def lookup_set(self, s: int, advice3, selectors5, table4, a5, s5, z5, l):
        """LOOKUP(s): the 25 constraints of column set s.  advice3: the set's columns x, y, z; selectors5, a5, s5, z5: the selector,
        A', S' and Z of its five arguments; table4: the table; l [3]; all extended."""
        call = "aesw_vanish_lookup_device"
        s = self._turn("lookup_set", s)
        advice3, table4, l = self._group(advice3, "advice3", 3), self._group(table4, "table4", 4), self._group(l, "l", 3)
        selectors5, a5, s5, z5 = (self._group(t, name, 5) for t, name in ((selectors5, "selectors5"), (a5, "a5"), (s5, "s5"), (z5, "z5")))
        rc = self._lib.aesw_vanish_lookup_device(self.ctx._h, *self._shape(), s, advice3.data_ptr(), selectors5.data_ptr(), table4.data_ptr(), a5.data_ptr(), s5.data_ptr(),
                                                 z5.data_ptr(), l.data_ptr(), self.scalars.data_ptr(), self.acc.data_ptr(), self.acc.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, call)
        self._done += 1
        return self

    def divide(self):
        """DIVIDE: acc * inv(x_j^n - 1) in place; returns acc, the quotient on the extended coset (extended_to_coeff takes it)."""
        call = "aesw_vanish_divide_device"
        self._turn("divide")
        rc = self._lib.aesw_vanish_divide_device(self.ctx._h, self.k, self.ext_k, self.tables.data_ptr(), self.acc.data_ptr(), self.acc.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, call)
        self._done += 1
        return self.acc


class Transcript:
    """What Context.transcript returns: halo2's Blake2bWrite<_, G1Affine, Challenge255<_>> on the device (include/aesw_transcript.h
    states the rule; parity with halo2 itself is not pinned).  Every method but proof() and status() is asynchronous on the
    current stream and allocates only the tensors it returns, so reset() ... squeeze(out=...) can be captured into one graph."""

    def __init__(self, ctx: "Context", proof_capacity: int = 0, _state=None, _proof=None):
        self._lib = load_transcript_library()
        self.ctx, self.proof_capacity = ctx, int(proof_capacity)
        self._state = ctx._output(_state, "_state", (TRANSCRIPT_STATE_BYTES,))
        self._proof = ctx._output(_proof, "_proof", (self.proof_capacity,)) if self.proof_capacity > 0 else None
        self.reset()

    def reset(self):
        """aesw_transcript_init_device: nothing absorbed, the proof's cursor at 0."""
        self.ctx._check(self._lib.aesw_transcript_init_device(self.ctx._h, self._state.data_ptr(), self.ctx._stream()), "aesw_transcript_init_device")
        return self

    def _absorb(self, call, items, write):
        if write and self._proof is None:
            raise AeswError(ERR_INVALID_ARG, call + ": the transcript was made with proof_capacity=0 and has no proof to write to")
        rc = getattr(self._lib, call)(self.ctx._h, self._state.data_ptr(), items.shape[0], items.data_ptr(), self._proof.data_ptr() if write else None,
                                      self.proof_capacity if write else 0, self.ctx._stream())
        self.ctx._check(rc, call)
        return self

    def common_points(self, points):
        """common_point for every row of points, in order: a uint8 [n, 64] tensor of affine points in Montgomery form (what
        commit_columns returns), or a numpy array of that shape, which is uploaded.  1 <= n <= 65535."""
        return self._absorb("aesw_transcript_points_device", self.ctx._point_rows(points, "points"), False)

    def write_points(self, points):
        """write_point for every row of points: absorbed as common_points absorbs them, and 32 compressed bytes each appended to
        the proof."""
        return self._absorb("aesw_transcript_points_device", self.ctx._point_rows(points, "points"), True)

    def common_scalars(self, cells):
        """common_scalar for every cell, in order.  cells: ints, numpy cells or a uint8 [n, 32] (or [32]) tensor on the device."""
        return self._absorb("aesw_transcript_scalars_device", self.ctx._cells(cells, "cells"), False)

    def write_scalars(self, cells):
        """write_scalar for every cell: absorbed, and its 32 plain little-endian bytes appended to the proof."""
        return self._absorb("aesw_transcript_scalars_device", self.ctx._cells(cells, "cells"), True)

    def squeeze(self, out=None):
        """squeeze_challenge: a uint8 [32] device tensor holding the challenge as an Fr cell in Montgomery form, written when the
        kernel runs.  out: the tensor to write into (a capture)."""
        out = self.ctx._output(out, "out", (32,))
        rc = self._lib.aesw_transcript_squeeze_device(self.ctx._h, self._state.data_ptr(), out.data_ptr(), self.ctx._stream())
        self.ctx._check(rc, "aesw_transcript_squeeze_device")
        return out

    def status(self) -> dict:
        """The state's report words after synchronising the stream: proof_bytes (produced so far, the cursor), proof_missed (of
        those, the bytes that did not fit), identities (identity points seen) and first_identity (the index of the first among
        the points absorbed, or None)."""
        return self.ctx._report(self._state.view(self.ctx._torch().int64), True, transcript_status_dict)

    def proof(self) -> bytes:
        """The proof bytes produced so far, after synchronising the stream.  AeswError if any did not fit: the text names the
        capacity the proof needs."""
        st = self.status()
        if st["proof_missed"]:
            raise AeswError(ERR_CAPACITY, "Transcript.proof: %d of the %d proof bytes did not fit into proof_capacity=%d; the proof needs %d" % (
                st["proof_missed"], st["proof_bytes"], self.proof_capacity, st["proof_bytes"]))
        return self._proof[:st["proof_bytes"]].cpu().numpy().tobytes() if st["proof_bytes"] else b""


class MultiplicityAccumulator:
    """What Context.multiplicity_accumulator returns.  Nothing here waits on the host or allocates after the constructor, so a
    reset() and its add()s can be captured into one graph; a replay of captured add()s adds again."""

    def __init__(self, ctx: "Context", k: int, n_sets: int, layout: int, _out=None):
        torch = ctx._torch()
        self._lib = load_acc_library()
        self.ctx, self.k, self.n_sets, self.layout = ctx, int(k), int(n_sets), int(layout)
        self._mult = ctx._output(_out, "_out", (self.n_sets, K.TABLE_ROWS), "int32")
        self._rep = torch.empty(3, dtype=torch.int64, device=ctx._dev())

    def _stream(self, stream):
        return self.ctx._stream() if stream is None else C.c_void_p(stream.cuda_stream)

    def reset(self, stream=None):
        """Histograms to zero, the report to (0 lookups, 0 misses, no miss).  The first call of every count."""
        rc = self._lib.aesw_acc_reset_device(self.ctx._h, self.n_sets, self._mult.data_ptr(), self._rep.data_ptr(), self._stream(stream))
        self.ctx._check(rc, "aesw_acc_reset_device")
        return self

    def add(self, first_block: int, witness: Witness, stream=None, n_blocks: int | None = None, _chunk: int = 0):
        """Adds circuit blocks [first_block, first_block + n_blocks): slab i of `witness` (x, y, z) is block first_block + i.
        n_blocks: default every block `witness` holds; fewer when a reused buffer is only partly filled.  _chunk forces the
        blocks a pair of workgroups takes (tests, tools)."""
        x, y, z = [self.ctx._u8(t, "witness") for t in witness[:3]]
        held = int(y.numel()) // column_stride(self.layout, 1) if self.layout in (K.LAYOUT_DENSE, K.LAYOUT_PACKED) else 0
        n = held if n_blocks is None else int(n_blocks)
        for i, t in enumerate((x, y, z)):
            if n and int(t.numel()) < n * column_stride(self.layout, i):
                raise ValueError("witness holds fewer than n_blocks blocks")
        rc = self._lib.aesw_acc_add_device_chunk(self.ctx._h, self.k, self.n_sets, int(first_block), n, self.layout, x.data_ptr(), y.data_ptr(),
                                                 z.data_ptr(), self._mult.data_ptr(), self._rep.data_ptr(), self._stream(stream), int(_chunk))
        self.ctx._check(rc, "aesw_acc_add_device")
        return self

    def add_values(self, first_block: int, pt, witness: Witness, key_witness: KeyWitness, stream=None, n_blocks: int | None = None, _chunk: int = 0):
        """Adds circuit blocks [first_block, first_block + n_blocks) given as a VALUES witness (libaesw_vacc.so, loaded on the
        first call): `witness` is what encrypt_witness(layout=LAYOUT_VALUES) returns (its y and z are read, x is ignored), pt
        uint8[n,16] the plaintext of the same blocks, key_witness the circuit's packed key slab, of which the round-key cells are
        read -- its own 400 rows are add_key()'s.  Whatever `layout` the accumulator was made with: the histograms do not depend
        on it.  n_blocks and _chunk as for add()."""
        lib = load_vacc_library()
        pt, y, z = self.ctx._u8(pt, "pt"), self.ctx._u8(witness.y, "witness"), self.ctx._u8(witness.z, "witness")
        w, kz = self.ctx._u8(key_witness[0], "key_witness"), self.ctx._u8(key_witness[3], "key_witness")
        n = int(y.numel()) // column_stride(K.LAYOUT_VALUES, 1) if n_blocks is None else int(n_blocks)
        for t, per in ((pt, 16), (y, column_stride(K.LAYOUT_VALUES, 1)), (z, column_stride(K.LAYOUT_VALUES, 2))):
            if int(t.numel()) < n * per:
                raise ValueError("pt or witness holds fewer than n_blocks blocks")
        if int(w.numel()) < K.WORDS_ROWS or int(kz.numel()) < key_column_stride(K.LAYOUT_PACKED, 2):
            raise ValueError("key_witness must hold one packed key slab")
        ks = KeySlab(w.data_ptr(), None, None, kz.data_ptr())
        rc = lib.aesw_vacc_add_device_chunk(self.ctx._h, self.k, self.n_sets, int(first_block), n, pt.data_ptr(), y.data_ptr(), z.data_ptr(),
                                            C.byref(ks), self._mult.data_ptr(), self._rep.data_ptr(), self._stream(stream), int(_chunk))
        self.ctx._check(rc, "aesw_vacc_add_device")
        return self

    def add_key(self, key_witness: KeyWitness, stream=None):
        """Adds the 400 rows of the circuit's key slab (the first one `key_witness` holds) to set 0; nothing for k < 9."""
        kx, ky, kz = [self.ctx._u8(t, "key_witness") for t in key_witness[1:4]]
        ks = KeySlab(None, kx.data_ptr(), ky.data_ptr(), kz.data_ptr())
        rc = self._lib.aesw_acc_add_key_device(self.ctx._h, self.k, self.layout, C.byref(ks), self._mult.data_ptr(), self._rep.data_ptr(),
                                               self._stream(stream))
        self.ctx._check(rc, "aesw_acc_add_key_device")
        return self

    def histograms(self):
        """The int32 [n_sets, 66561] device tensor every call adds to (not a copy; nothing is synchronised)."""
        return self._mult

    def permuted_columns(self, n_rows: int | None = None, pad_row: int = 0, sync: bool = True):
        """Context.permuted_columns over these histograms as they stand on the current stream."""
        return self.ctx.permuted_columns(self.k, self.n_sets, self._mult, n_rows, pad_row, sync)

    def report(self, sync: bool = True):
        """The dict of mult_report_dict over everything added since reset() -- a block's unit is its index in the circuit, the
        key slab's 0 -- after synchronising the stream; with sync=False the uint64[3] device tensor."""
        return self.ctx._report(self._rep, sync, mult_report_dict)


def _group_refuses(name):
    def refuse(self, *args, **kwargs):
        raise AeswError(ERR_INVALID_ARG, "Group.%s: device pointers belong to one GPU; use a member (Group.member_handle(i) is its aesw_ctx*)" % name)
    refuse.__name__ = name
    return refuse


class Group(Context):
    """A group context (aesw_create_group): one member context per listed device, driven from this one process.  The host-pointer
    methods of Context split a batch into contiguous block shards, one member (and host thread) each, every GPU copying its shard
    over its own link into the caller's arrays.  Methods that take device tensors raise: device memory belongs to one GPU."""

    def __init__(self, devices=None, tables=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        sbox, mul2, mul3 = tables if tables is not None else K.reference_tables()
        self._tables = tuple(np.ascontiguousarray(t, dtype=np.uint8) for t in (sbox, mul2, mul3))
        for t in self._tables:
            if t.shape != (256,):
                raise ValueError("tables must be three uint8[256] arrays")
        devs = None if devices is None else np.ascontiguousarray(list(devices), dtype=np.intc)
        rc = self._lib.aesw_create_group(C.byref(self._h), _ptr(devs),
                                         0 if devs is None else devs.size, *[_np_ptr(t) for t in self._tables])
        if rc:
            self._h = C.c_void_p()
            raise AeswError(rc, "aesw_create_group(devices=%r)" % (devices,))
        self.device = int(self._lib.aesw_device(self._h))
        self._arenas = {}

    @property
    def size(self) -> int:
        return int(self._lib.aesw_group_size(self._h))

    def shard(self, n: int, i: int):
        """(first, count) of member i's blocks in a batch of n."""
        return group_shard(self.size, n, i)

    def member_handle(self, i: int) -> int:
        """aesw_group_member: the borrowed aesw_ctx* of member i (an int; valid while the group lives)."""
        h = self._lib.aesw_group_member(self._h, i)
        if not h:
            raise IndexError("member %d of a group of %d" % (i, self.size))
        return int(h)


# the device-tensor methods of Context (the C ABI refuses them on a group as well)
for _name in ("alloc_witness", "alloc_columns", "free_columns", "schedule_key", "encrypt_witness", "encrypt_witness_batches",
              "key_schedule_witness", "lookup_table", "expand_fr", "check_witness", "assemble_advice", "assemble_advice_stream",
              "assemble_advice_host", "assemble_advice_circuits", "circuits", "check_circuits", "check_columns", "check_values",
              "lookup_multiplicities", "multiplicity_accumulator", "permuted_columns", "gather_fr",
              "compress_table", "lookup_inputs", "prepare_lookup_inputs", "argument_columns", "invert_table", "grand_product",
              "permutation_tables", "permutation_product", "ntt_tables", "lagrange_to_coeff", "coeff_to_lagrange", "coeff_to_extended",
              "extended_to_coeff", "permutation_columns_fr", "evaluate_columns", "fold_columns", "divide_columns", "msm_basis",
              "commit_columns", "transcript", "shplonk_table", "shplonk_prepare", "shplonk_finish", "combine_columns", "set_quotient", "open_shplonk",
              "vanishing_tables", "vanishing_scalars", "vanishing_scalar", "quotient_accumulator", "quotient_extended",
              "blinding_seed", "blind_rows", "blinding_tail", "commit_tail", "commit_blinded_bytes"):
    setattr(Group, _name, _group_refuses(_name))
del _name


class Comm:
    """aesw_comm: the RCCL communicator of the C ABI (one process per GPU).  `unique_id()` on one rank, carried to
    the others by the host's own means, then Comm(ctx, nranks, rank, id) on every rank (collective)."""

    def __init__(self, ctx: "Context", nranks: int, rank: int, uid: bytes | None = None):
        self._lib = ctx._lib
        self._h = C.c_void_p()
        self.nranks, self.rank, self.ctx = nranks, rank, ctx
        buf = (C.c_uint8 * 128).from_buffer_copy(uid) if uid is not None else None
        rc = self._lib.aesw_comm_create(ctx._h, nranks, rank, buf, C.byref(self._h))
        if rc:
            raise AeswError(rc, self._lib.aesw_comm_last_error().decode())

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        rc = lib.aesw_comm_unique_id(buf)
        if rc:
            raise AeswError(rc, lib.aesw_comm_last_error().decode())
        return bytes(buf)

    def close(self):
        if self._h:
            self._lib.aesw_comm_destroy(self._h)
            self._h = C.c_void_p()

    def set_max_message(self, nbytes: int):
        rc = self._lib.aesw_comm_set_max_message(self._h, nbytes)
        if rc:
            raise AeswError(rc)

    def gather_columns(self, columns, counts, strides, root: int = 0, out=None):
        """aesw_gather_columns_device on torch's current stream.  columns: this rank's flat uint8 device tensors;
        returns the gathered tensors on `root` (allocated unless `out` is given), None elsewhere."""
        import torch
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        strides_a = np.ascontiguousarray(strides, dtype=np.uint32)
        if counts.size != self.nranks or len(columns) != strides_a.size:
            raise ValueError("counts/strides do not match ranks / columns")
        total = int(counts.sum())
        n = len(columns)
        send = (C.c_void_p * n)(*[c.data_ptr() if c.numel() else None for c in columns])
        recv = None
        if self.rank == root:
            if out is None:
                out = [torch.empty(total * int(s), dtype=torch.uint8, device=c.device) for c, s in zip(columns, strides_a)]
            recv = (C.c_void_p * n)(*[o.data_ptr() if o.numel() else None for o in out])
        stream = C.c_void_p(torch.cuda.current_stream(self.ctx.device).cuda_stream)
        rc = self._lib.aesw_gather_columns_device(self._h, root, n, send, recv, _np_ptr(counts), _np_ptr(strides_a), stream)
        if rc:
            raise AeswError(rc, self._lib.aesw_comm_last_error().decode())
        return out if self.rank == root else None


class HostCircuit:
    """What the C++ host mirror's synthesize() assigned (include/aesw_host.h):
    MockProver::run of the reference's circuits with device-fed value closures."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, C.c_void_p(handle)

    @staticmethod
    def _host():
        return load_host_library()

    @classmethod
    def aes(cls, ctx: "Context", k: int, n_sets: int, key, pts, with_witnesses: bool = True,
            skip_schedule_key: bool = False, bulk_assign: bool = False, values_only: bool = False,
            streaming: bool = False, dense: bool = False) -> "HostCircuit":
        """load_enc_full_table, schedule_key(key), encrypt(pts[b]) for every block: TestAesCircuit /
        Aes128BenchCircuit (src/aes128.rs:376-407, benches/aes128.rs:30-61).  The device witness travels in the
        PACKED layout (assigned cells only) unless values_only / streaming (VALUES) or dense is asked for."""
        key = np.ascontiguousarray(key, np.uint8).reshape(16)
        pts = np.ascontiguousarray(pts, np.uint8).reshape(-1, 16)
        h = C.c_void_p()
        lib = cls._host()
        mode = 3 if streaming else (2 if values_only else (1 if bulk_assign else (4 if dense else 0)))
        rc = lib.aesw_host_aes_circuit_run(ctx._h, k, n_sets, _np_ptr(key), _np_ptr(pts), pts.shape[0],
                                           1 if with_witnesses else 0, 1 if skip_schedule_key else 0, mode, C.byref(h))
        if rc:
            raise AeswError(rc, lib.aesw_host_last_error().decode())
        return cls(lib, h.value)

    @classmethod
    def aes_columns(cls, ctx: "Context", k: int, n_sets: int, key, pts) -> "HostCircuit":
        """The same circuit without running a region: whole advice columns from the device witness, selectors, fixed
        column, table and equality constraints from the library's keygen data (aesw_host_aes_circuit_columns)."""
        key = np.ascontiguousarray(key, np.uint8).reshape(16)
        pts = np.ascontiguousarray(pts, np.uint8).reshape(-1, 16)
        h = C.c_void_p()
        lib = cls._host()
        rc = lib.aesw_host_aes_circuit_columns(ctx._h, k, n_sets, _np_ptr(key), _np_ptr(pts), pts.shape[0], C.byref(h))
        if rc:
            raise AeswError(rc, lib.aesw_host_last_error().decode())
        return cls(lib, h.value)

    @classmethod
    def key_schedule(cls, ctx: "Context", k: int, key) -> "HostCircuit":
        """key_schedule.rs TestCircuit (src/key_schedule.rs:245-320)."""
        key = np.ascontiguousarray(key, np.uint8).reshape(16)
        h = C.c_void_p()
        lib = cls._host()
        rc = lib.aesw_host_key_circuit_run(ctx._h, k, _np_ptr(key), C.byref(h))
        if rc:
            raise AeswError(rc, lib.aesw_host_last_error().decode())
        return cls(lib, h.value)

    def close(self):
        if self._h:
            self._lib.aesw_host_circuit_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def verify(self):
        """mock.assert_satisfied(): (0, "") or (AESW_ERR_UNSATISFIED, first failure)."""
        buf = C.create_string_buffer(256)
        rc = self._lib.aesw_host_circuit_verify(self._h, buf, 256)
        return rc, buf.value.decode()

    num_advice = property(lambda self: self._lib.aesw_host_circuit_num_advice(self._h))
    num_selectors = property(lambda self: self._lib.aesw_host_circuit_num_selectors(self._h))
    num_rows = property(lambda self: self._lib.aesw_host_circuit_num_rows(self._h))
    num_regions = property(lambda self: self._lib.aesw_host_circuit_num_regions(self._h))
    num_copies = property(lambda self: self._lib.aesw_host_circuit_num_copies(self._h))
    closure_calls = property(lambda self: self._lib.aesw_host_circuit_closure_calls(self._h))

    def _arr(self, p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    def advice(self, col):
        return self._arr(self._lib.aesw_host_circuit_advice(self._h, col), self.num_rows)

    def advice_assigned(self, col):
        return self._arr(self._lib.aesw_host_circuit_advice_assigned(self._h, col), self.num_rows)

    def selector(self, s):
        return self._arr(self._lib.aesw_host_circuit_selector(self._h, s), self.num_rows)

    def fixed(self):
        return self._arr(self._lib.aesw_host_circuit_fixed(self._h), self.num_rows)

    def table(self, col):
        n = C.c_uint64()
        p = self._lib.aesw_host_circuit_table(self._h, col, C.byref(n))
        return self._arr(p, n.value)

    def copies(self) -> np.ndarray:
        """[num_copies, 4] = (copy column, copy row, original column, original row)."""
        out = np.zeros((self.num_copies, 4), np.uint64)
        rc = self._lib.aesw_host_circuit_copies(self._h, _np_ptr(out))
        if rc:
            raise AeswError(rc)
        return out

    def ciphertext(self, b):
        ct = np.zeros(16, np.uint8)
        rc = self._lib.aesw_host_circuit_ciphertext(self._h, b, _np_ptr(ct))
        if rc:
            raise AeswError(rc)
        return ct

    def poke(self, col, row, value):
        rc = self._lib.aesw_host_circuit_poke(self._h, col, row, value)
        if rc:
            raise AeswError(rc)
