"""ctypes binding of libmi_gp.so (include/mi_gp.h).  There is no CPU fallback: if the HIP library
is missing the import of the product path fails loudly."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi_gp.so")
SPARSE_LIB_PATH = os.path.join(_HERE, "libmi_gp_sparse.so")  # the sparse inducing-point bound (include/mi_gp_sparse.h)
# the same entry points and the data-side gradients (include/mi_gp_sparse_data.h)
SPARSE_DATA_LIB_PATH = os.path.join(_HERE, "libmi_gp_sparse_data.so")
# the entry points of include/mi_gp.h and the gradient binding (include/mi_gp_deriv.h)
DERIV_LIB_PATH = os.path.join(_HERE, "libmi_gp_deriv.so")

MAX_KERN = 8
KERNEL_IDS = {"RBF": 0, "Matern52": 1, "Matern32": 2, "Exponential": 3, "RatQuad": 4}
OP_IDS = {"+": 0, "*": 1}


class MiGpConfig(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int),
        ("d", ctypes.c_int),
        ("nkern", ctypes.c_int),
        ("kernel_ids", ctypes.c_int * MAX_KERN),
        ("ops", ctypes.c_int * MAX_KERN),
        ("device", ctypes.c_int),
        ("panel_tiles", ctypes.c_int),
    ]


class MiGpBuffers(ctypes.Structure):
    _fields_ = [
        ("X_dev", ctypes.c_void_p),
        ("y_dev", ctypes.c_void_p),
        ("K_dev", ctypes.c_void_p),
        ("lda", ctypes.c_long),
        ("Z_dev", ctypes.c_void_p),
        ("W_dev", ctypes.c_void_p),
    ]


class MiGpBatchBuffers(ctypes.Structure):
    _fields_ = [
        ("K_dev", ctypes.c_void_p),
        ("Z_dev", ctypes.c_void_p),
        ("W_dev", ctypes.c_void_p),
        ("stride_k", ctypes.c_long),
        ("stride_zw", ctypes.c_long),
        ("count", ctypes.c_int),
    ]


class MiGpShardConfig(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int),
        ("d", ctypes.c_int),
        ("nkern", ctypes.c_int),
        ("kernel_ids", ctypes.c_int * MAX_KERN),
        ("ops", ctypes.c_int * MAX_KERN),
        ("panel_tiles", ctypes.c_int),
        ("world", ctypes.c_int),
        ("rank", ctypes.c_int),
        ("device", ctypes.c_int),
        ("X_dev", ctypes.c_void_p),
        ("y_dev", ctypes.c_void_p),
        ("K_dev", ctypes.c_void_p),
        ("ldk", ctypes.c_long),
        ("P_dev", ctypes.c_void_p * 2),
        ("ldp", ctypes.c_long),
        ("theta_dev", ctypes.c_void_p),
        ("info_dev", ctypes.c_void_p),
        ("out_dev", ctypes.c_void_p),
    ]


class MiGpSparseConfig(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int),
        ("m", ctypes.c_int),
        ("d", ctypes.c_int),
        ("nkern", ctypes.c_int),
        ("kernel_ids", ctypes.c_int * MAX_KERN),
        ("ops", ctypes.c_int * MAX_KERN),
        ("device", ctypes.c_int),
        ("chunk", ctypes.c_int),
        ("zgrad_slabs", ctypes.c_int),  # 0: no dF/dZ; s >= 1: dF/dZ behind dF/dtheta, at most s slabs per chunk
    ]


_lib = None
_deriv = None


def load():
    """Load libmi_gp.so and declare every entry point of include/mi_gp.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C andvaranaut_amd/csrc` (there is no CPU fallback for the GP hot path)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    _declare(lib)
    _lib = lib
    return lib


def load_deriv():
    """Load libmi_gp_deriv.so and declare every entry point of include/mi_gp_deriv.h (those of include/mi_gp.h, the same code,
    and the gradient binding's three)."""
    global _deriv
    if _deriv is not None:
        return _deriv
    if not os.path.exists(DERIV_LIB_PATH):
        raise RuntimeError(f"{DERIV_LIB_PATH} not found: build it with `make -C andvaranaut_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(DERIV_LIB_PATH)
    _declare(lib)
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.mi_gp_deriv_bind.argtypes = [vp, ci]
    lib.mi_gp_deriv_assemble.argtypes = [ci, ci, vp, vp, ci, ci, vp, ci, ci, vp, cl, ci, ci, ci, ci, vp, vp]
    lib.mi_gp_deriv_contract.argtypes = [ci, ci, vp, vp, ci, vp, cl, vp, vp, cl, vp, vp]
    for name in DERIV_EXPORTS:
        getattr(lib, name)  # raises AttributeError if a declared symbol is missing
    _deriv = lib
    return lib


def _declare(lib):
    """the argument types of the entry points of include/mi_gp.h"""
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.mi_gp_last_global_error.restype = ctypes.c_char_p
    lib.mi_gp_last_error.restype = ctypes.c_char_p
    lib.mi_gp_last_error.argtypes = [vp]
    lib.mi_gp_create.argtypes = [ctypes.POINTER(MiGpConfig), ctypes.POINTER(vp)]
    lib.mi_gp_destroy.argtypes = [vp]
    lib.mi_gp_padded_n.argtypes = [vp]
    lib.mi_gp_padded_n.restype = cl
    lib.mi_gp_num_theta.argtypes = [vp]
    lib.mi_gp_stream.argtypes = [vp]
    lib.mi_gp_stream.restype = vp
    lib.mi_gp_set_data.argtypes = [vp, ctypes.POINTER(MiGpBuffers)]
    lib.mi_gp_lml.argtypes = [vp, dp, dp]
    lib.mi_gp_lml_parts.argtypes = [vp, dp, dp]
    lib.mi_gp_lml_grad.argtypes = [vp, dp, dp, dp]
    lib.mi_gp_set_batch.argtypes = [vp, ctypes.POINTER(MiGpBatchBuffers)]
    lib.mi_gp_lml_batch.argtypes = [vp, ci, dp, dp, ip]
    lib.mi_gp_lml_grad_batch.argtypes = [vp, ci, dp, dp, dp, ip]
    lib.mi_gp_alpha.argtypes = [vp, dp]
    lib.mi_gp_grad_x.argtypes = [vp, vp]
    lib.mi_gp_set_diag.argtypes = [vp, vp]
    lib.mi_gp_factor.argtypes = [vp, dp]
    lib.mi_gp_predict.argtypes = [vp, vp, ci, vp, cl, vp, vp, ci]
    lib.mi_gp_predict_u.argtypes = [vp, vp, ci, vp, cl, vp, vp, ci]
    lib.mi_gp_predict_grad.argtypes = [vp, vp, ci, vp, cl, vp, vp, ci, vp, vp]
    lib.mi_gp_factor_batch.argtypes = [vp, ci, dp, ip]
    lib.mi_gp_reserve.argtypes = [vp, ci]
    lib.mi_gp_append.argtypes = [vp, vp, vp, vp, ci, vp, cl]
    lib.mi_gp_logpdf_work.argtypes = [cl]
    lib.mi_gp_logpdf_work.restype = cl
    lib.mi_gp_logpdf.argtypes = [vp, vp, vp, vp, ci, vp, cl, dp, vp, vp]
    lib.mi_gp_kfold_work.argtypes = [ci, cl]
    lib.mi_gp_kfold_work.restype = cl
    lib.mi_gp_kfold.argtypes = [vp, ci, ip, ip, vp, cl, vp, vp, vp, ip]
    lib.mi_gp_predict_batch.argtypes = [vp, ci, vp, ci, vp, cl, cl, vp, vp, ci, vp, vp]
    lib.mi_gp_predict_cov.argtypes = [vp, vp, ci, vp, cl, vp, vp, cl, ci]
    lib.mi_gp_sample_cov_work.argtypes = [ci, ci]
    lib.mi_gp_sample_cov_work.restype = cl
    u64 = ctypes.c_uint64
    lib.mi_gp_sample_cov.argtypes = [vp, vp, cl, ci, vp, cd, ci, u64, u64, vp, cl, vp, cl]
    lib.mi_gp_set_option.argtypes = [vp, ci, ci]
    lib.mi_gp_get_option.argtypes = [vp, ci, ip]
    lib.mi_gp_set_profiling.argtypes = [vp, ci]
    lib.mi_gp_timers.argtypes = [vp, dp, ci]
    lib.mi_gp_assemble_block.argtypes = [ci, ci, ip, ip, vp, vp, ci, vp, ci, ci, ci, vp, cl, ci, ci, ci, vp]
    lib.mi_gp_chol_panel.argtypes = [vp, cl, ci, ci, vp, vp, ci, vp]
    lib.mi_gp_lml_partial.argtypes = [vp, cl, vp, ci, vp, vp]
    lib.mi_gp_gemm_f64.argtypes = [ci, ci, ci, ci, ci, cd, vp, cl, vp, cl, cd, vp, cl, ci, ci, ci, cl, cl, cl, vp]
    lib.mi_gp_gemm_f64_tuned.argtypes = [ci, ci, ci, ci, ci, cd, vp, cl, vp, cl, cd, vp, cl, ci, ci, ci, ci, ci, ci, vp]
    lib.mi_gp_gemm_nt_kseg.argtypes = [ci, ci, ci, cd, vp, cl, vp, cl, ci, cl, cd, vp, cl, ci, ci, vp]
    lib.mi_gp_trsm_block.argtypes = [vp, cl, vp, ci, ci, vp, cl, ci, vp]
    lib.mi_gp_trmv_upper.argtypes = [vp, cl, vp, ci, vp, vp]
    lib.mi_gp_grad_contract_block_scratch.argtypes = [ci, ci, ci, ci]
    lib.mi_gp_grad_contract_block_scratch.restype = cl
    lib.mi_gp_grad_contract_block.argtypes = [ci, ci, ip, ip, vp, vp, ci, vp, cl, ci, ci, ci, vp, vp, cl, vp, vp]
    lib.mi_gp_shard_create.argtypes = [ctypes.POINTER(MiGpShardConfig), ctypes.POINTER(vp)]
    lib.mi_gp_shard_destroy.argtypes = [vp]
    lib.mi_gp_shard_begin.argtypes = [vp, ci, vp, vp]
    lib.mi_gp_shard_step.argtypes = [vp, ci, vp, vp]
    lib.mi_gp_shard_finish.argtypes = [vp, vp, vp]
    lib.mi_gp_shard_wait_piece.argtypes = [vp, ci, vp]
    lib.mi_gp_shard_set_option.argtypes = [vp, ci, ci]
    lib.mi_gp_shard_times.argtypes = [vp, dp, ci]
    lib.mi_gp_shard_piece_times.argtypes = [vp, dp, ci]
    lib.mi_gp_shard_chain_stream.argtypes = [vp]
    lib.mi_gp_shard_last_error.argtypes = [vp]
    lib.mi_gp_shard_last_error.restype = ctypes.c_char_p
    for name in EXPORTS:
        getattr(lib, name)  # raises AttributeError if a declared symbol is missing


# every symbol include/mi_gp.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = [
    "mi_gp_reserve",
    "mi_gp_append",
    "mi_gp_logpdf_work",
    "mi_gp_logpdf",
    "mi_gp_kfold_work",
    "mi_gp_kfold",
    "mi_gp_last_global_error",
    "mi_gp_last_error",
    "mi_gp_create",
    "mi_gp_destroy",
    "mi_gp_padded_n",
    "mi_gp_num_theta",
    "mi_gp_stream",
    "mi_gp_set_data",
    "mi_gp_lml",
    "mi_gp_lml_parts",
    "mi_gp_lml_grad",
    "mi_gp_set_batch",
    "mi_gp_lml_batch",
    "mi_gp_lml_grad_batch",
    "mi_gp_alpha",
    "mi_gp_grad_x",
    "mi_gp_set_diag",
    "mi_gp_factor",
    "mi_gp_predict",
    "mi_gp_predict_u",
    "mi_gp_predict_grad",
    "mi_gp_factor_batch",
    "mi_gp_predict_batch",
    "mi_gp_predict_cov",
    "mi_gp_sample_cov_work",
    "mi_gp_sample_cov",
    "mi_gp_set_option",
    "mi_gp_get_option",
    "mi_gp_set_profiling",
    "mi_gp_timers",
    "mi_gp_gemm_f64",
    "mi_gp_gemm_f64_tuned",
    "mi_gp_gemm_nt_kseg",
    "mi_gp_assemble_block",
    "mi_gp_chol_panel",
    "mi_gp_lml_partial",
    "mi_gp_trsm_block",
    "mi_gp_trmv_upper",
    "mi_gp_grad_contract_block_scratch",
    "mi_gp_grad_contract_block",
    "mi_gp_shard_create",
    "mi_gp_shard_destroy",
    "mi_gp_shard_begin",
    "mi_gp_shard_step",
    "mi_gp_shard_finish",
    "mi_gp_shard_wait_piece",
    "mi_gp_shard_set_option",
    "mi_gp_shard_times",
    "mi_gp_shard_piece_times",
    "mi_gp_shard_chain_stream",
    "mi_gp_shard_last_error",
]

# every symbol include/mi_gp_deriv.h declares, with those of the header it includes (checked by tests/test_deriv_host.py against
# the library's dynamic symbols)
DERIV_EXPORTS = EXPORTS + ["mi_gp_deriv_bind", "mi_gp_deriv_assemble", "mi_gp_deriv_contract"]


_sparse = None
_sparse_data = None


def _declare_sparse(lib):
    """the argument types of the eight entry points of include/mi_gp_sparse.h"""
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    dp = ctypes.POINTER(ctypes.c_double)
    lib.mi_gp_sparse_create.argtypes = [ctypes.POINTER(MiGpSparseConfig), ctypes.POINTER(vp)]
    lib.mi_gp_sparse_destroy.argtypes = [vp]
    lib.mi_gp_sparse_last_error.argtypes = [vp]
    lib.mi_gp_sparse_last_error.restype = ctypes.c_char_p
    lib.mi_gp_sparse_work.argtypes = [ci, ci]
    lib.mi_gp_sparse_work.restype = cl
    lib.mi_gp_sparse_set_data.argtypes = [vp, vp, vp, ci, vp, vp, cl]
    lib.mi_gp_sparse_bound_grad.argtypes = [vp, dp, dp, dp]
    lib.mi_gp_sparse_factor.argtypes = [vp, dp]
    lib.mi_gp_sparse_predict.argtypes = [vp, vp, ci, vp, vp, ci]


def load_sparse():
    """Load libmi_gp_sparse.so and declare every entry point of include/mi_gp_sparse.h."""
    global _sparse
    if _sparse is not None:
        return _sparse
    if not os.path.exists(SPARSE_LIB_PATH):
        raise RuntimeError(f"{SPARSE_LIB_PATH} not found: build it with `make -C andvaranaut_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(SPARSE_LIB_PATH)
    _declare_sparse(lib)
    for name in SPARSE_EXPORTS:
        getattr(lib, name)  # raises AttributeError if a declared symbol is missing
    _sparse = lib
    return lib


def load_sparse_data():
    """Load libmi_gp_sparse_data.so and declare every entry point of include/mi_gp_sparse_data.h (those of
    include/mi_gp_sparse.h, the same code, and mi_gp_sparse_bind_data_grad)."""
    global _sparse_data
    if _sparse_data is not None:
        return _sparse_data
    if not os.path.exists(SPARSE_DATA_LIB_PATH):
        raise RuntimeError(f"{SPARSE_DATA_LIB_PATH} not found: build it with `make -C andvaranaut_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(SPARSE_DATA_LIB_PATH)
    _declare_sparse(lib)
    lib.mi_gp_sparse_bind_data_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    for name in SPARSE_DATA_EXPORTS:
        getattr(lib, name)  # raises AttributeError if a declared symbol is missing
    _sparse_data = lib
    return lib


# every symbol include/mi_gp_sparse.h declares (checked by tests/test_sparse_abi_host.py against the header text)
SPARSE_EXPORTS = [
    "mi_gp_sparse_create",
    "mi_gp_sparse_destroy",
    "mi_gp_sparse_last_error",
    "mi_gp_sparse_work",
    "mi_gp_sparse_set_data",
    "mi_gp_sparse_bound_grad",
    "mi_gp_sparse_factor",
    "mi_gp_sparse_predict",
]

# every symbol include/mi_gp_sparse_data.h declares, with those of the header it includes (checked by
# tests/test_sgpr_data_grad_host.py against the library's dynamic symbols)
SPARSE_DATA_EXPORTS = SPARSE_EXPORTS + ["mi_gp_sparse_bind_data_grad"]
