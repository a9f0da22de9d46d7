"""ctypes binding of the C ABI in include/llmqat_fakequant.h.

There is no fallback: if the HIP library is missing or fails to load, every op raises.
"""
import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# LLMQAT_AMD_LIB points the loader at another build of the library (A/B runs of kernel variants: tools/ab_bench.sh) -- the product
# file is never overwritten; fq_build_info() / LIB_PATH say which one is loaded
LIB_PATH = os.environ.get("LLMQAT_AMD_LIB") or os.path.join(HERE, "libllmqat_fakequant.so")
ABI_VERSION = 7   # fq_mx_gemm, the rotated MX entry points and the *_ex / fq_mx_ste_bwd ones are additions within 7 (the header says why)

DTYPE_F32, DTYPE_BF16, DTYPE_F16, DTYPE_F64 = 0, 1, 2, 3
SEM_CPU_EAGER, SEM_DEVICE_EAGER = 0, 1

# every symbol include/llmqat_fakequant.h declares (tests check the .so exports them all)
EXPORTS = (
    "fq_version", "fq_build_info", "fq_last_error", "fq_rowwise_workspace_bytes",
    "fq_sym_fwd", "fq_asym_fwd", "fq_sym_fwd_debug", "fq_asym_fwd_debug",
    "fq_ste_bwd", "fq_ste_bwd_rows",
    "fq_ste_mask_bytes", "fq_sym_fwd_train", "fq_asym_fwd_train", "fq_ste_bwd_mask",
    "fq_w12_fwd", "fq_sym_fwd_autocast", "fq_sym_fwd_pair", "fq_ste_bwd_mask_pair", "fq_ste_bwd_mask_wide",
    "fq_export_bins_bytes", "fq_sym_export", "fq_asym_export", "fq_sym_row_scales", "fq_sym_fwd_multi", "fq_ste_bwd_mask_multi", "fq_w12_fwd_rows",
    "fq_rowwise_fwd_v", "fq_sym_fwd_multi_v", "fq_ste_bwd_mask_multi_v", "fq_ste_bwd_v",
    "fq_group_fwd",
    "fq_mx_fwd", "fq_mx_export",
    "fq_mx_gemm",
    "fq_mx_fwd_rot", "fq_mx_export_rot", "fq_block_rotate",
    "fq_mx_fwd_ex", "fq_mx_export_ex", "fq_mx_ste_bwd",
)
# every symbol include/llmqat_fakequant_train.h declares (the fqt_ family: the training-side entry points, outside the recorded set above)
TRAIN_EXPORTS = ("fqt_mx_fwd_cols",)
# every symbol include/llmqat_fakequant_sr.h declares (the fqs_ family: MX fake quantization with stochastic rounding)
SR_EXPORTS = ("fqs_mx_fwd", "fqs_mx_fwd_cols", "fqs_mx_noise")
# every symbol include/llmqat_fakequant_infer.h declares (the fqi_ family: the inference-side entry points)
INFER_EXPORTS = ("fqi_mx_dequant",)
# every symbol include/llmqat_fakequant_loss.h declares (the fql_ family: the distillation loss)
LOSS_EXPORTS = ("fql_kd_kl_fwd", "fql_kd_kl_bwd")
# every symbol include/llmqat_fakequant_ce.h declares (the fqc_ family: the language-model cross-entropy loss)
CE_EXPORTS = ("fqc_ce_fwd", "fqc_ce_bwd")
CE_MEAN, CE_SUM = 0, 1   # FQC_REDUCTION_*
# every symbol include/llmqat_fakequant_norm.h declares (the fqn_ family: the RMSNorm in front of the quantized projections)
NORM_EXPORTS = ("fqn_rms_norm_fwd", "fqn_rms_norm_bwd", "fqn_rms_norm_bwd_parts", "fqn_rms_norm_bwd_workspace_bytes")
# every symbol include/llmqat_fakequant_act.h declares (the fqa_ family: the gated activation of the MLP)
ACT_EXPORTS = ("fqa_swiglu_fwd", "fqa_swiglu_bwd")
# every symbol include/llmqat_fakequant_rope.h declares (the fqr_ family: the rotary position embedding of q and k)
ROPE_EXPORTS = ("fqr_rope_dense_strides", "fqr_rope_fwd", "fqr_rope_bwd")
# every symbol include/llmqat_fakequant_attn.h declares (the fqs2_ family: the softmax chain between the two attention products)
ATTN_EXPORTS = ("fqs2_attn_softmax_fwd", "fqs2_attn_softmax_bwd")
MAX_TENSORS = 4  # tensors per multi-tensor launch


class FwdTensor(ctypes.Structure):  # fq_fwd_tensor
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("rows", ctypes.c_int64), ("bits", ctypes.c_int), ("row_bounds", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("mask_bytes", ctypes.c_size_t)]


class BwdTensor(ctypes.Structure):  # fq_bwd_tensor
    _fields_ = [("g", ctypes.c_void_p), ("gx", ctypes.c_void_p), ("rows", ctypes.c_int64), ("row_bounds", ctypes.c_void_p), ("mask", ctypes.c_void_p)]



class RowsView(ctypes.Structure):  # fq_rows_view: rows that do not follow one another in memory (strides in elements; n_inner = 0: contiguous)
    _fields_ = [("n_inner", ctypes.c_int64), ("stride_outer", ctypes.c_int64), ("stride_inner", ctypes.c_int64)]


class FwdTensorV(ctypes.Structure):  # fq_fwd_tensor_v
    _fields_ = FwdTensor._fields_ + [("xv", RowsView), ("yv", RowsView)]


class BwdTensorV(ctypes.Structure):  # fq_bwd_tensor_v
    _fields_ = BwdTensor._fields_ + [("gv", RowsView), ("gxv", RowsView)]


MX_FP4_E2M1, MX_FP6_E2M3, MX_FP6_E3M2, MX_FP8_E4M3, MX_FP8_E5M2 = 0, 1, 2, 3, 4
MX_FLAG_ROTATE, MX_FLAG_CEIL = 1, 2   # flags of fq_mx_fwd_ex / fq_mx_export_ex (fq_mx_ste_bwd: the first only)
BINS_NONE, BINS_INT4, BINS_INT8, BINS_INT16 = 0, 1, 2, 3
ERR_UNSUPPORTED = -8

_lock = threading.Lock()
_lib = None


class FakeQuantLibraryError(RuntimeError):
    pass


def _bind(L):
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.fq_version.argtypes = []
    L.fq_version.restype = i32
    L.fq_build_info.argtypes = []
    L.fq_build_info.restype = ctypes.c_char_p
    L.fq_last_error.argtypes = []
    L.fq_last_error.restype = ctypes.c_char_p
    L.fq_rowwise_workspace_bytes.argtypes = [i64, i64, i32]
    L.fq_rowwise_workspace_bytes.restype = sz
    for name in ("fq_sym_fwd", "fq_asym_fwd"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp, vp, sz, vp]
        f.restype = i32
    for name in ("fq_sym_fwd_debug", "fq_asym_fwd_debug"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, sz, vp]
        f.restype = i32
    L.fq_ste_bwd.argtypes = [vp, vp, vp, i64, f32, f32, i32, vp]
    L.fq_ste_bwd.restype = i32
    L.fq_ste_bwd_rows.argtypes = [vp, vp, vp, i64, i64, f32, f32, vp, i32, vp]
    L.fq_ste_bwd_rows.restype = i32
    L.fq_ste_mask_bytes.argtypes = [i64, i64, i32]
    L.fq_ste_mask_bytes.restype = sz
    for name in ("fq_sym_fwd_train", "fq_asym_fwd_train"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, i64, i64, i32, i32, i32, f32, f32, vp, vp, sz, vp]
        f.restype = i32
    L.fq_ste_bwd_mask.argtypes = [vp, vp, i64, i64, f32, f32, vp, vp, sz, i32, vp]
    L.fq_ste_bwd_mask.restype = i32
    L.fq_w12_fwd.argtypes = [vp, vp, vp, i64, i64, i32, i32, i32, vp]
    L.fq_w12_fwd.restype = i32
    L.fq_sym_fwd_autocast.argtypes = [vp, vp, i64, i64, i32, i32, i32, i32, f32, f32, vp, vp, sz, vp, sz, vp]
    L.fq_sym_fwd_autocast.restype = i32
    L.fq_sym_fwd_pair.argtypes = [vp, vp, i64, i32, vp, vp, sz, vp, vp, i64, i32, vp, vp, sz, i64, i32, i32, i32, f32, f32, vp]
    L.fq_sym_fwd_pair.restype = i32
    L.fq_ste_bwd_mask_pair.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, f32, f32, i32, vp]
    L.fq_ste_bwd_mask_pair.restype = i32
    L.fq_ste_bwd_mask_wide.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, f32, f32, i32, vp]
    L.fq_ste_bwd_mask_wide.restype = i32
    L.fq_export_bins_bytes.argtypes = [i64, i64, i32]
    L.fq_export_bins_bytes.restype = sz
    L.fq_sym_export.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, i32, vp]
    L.fq_sym_export.restype = i32
    L.fq_asym_export.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, vp]
    L.fq_asym_export.restype = i32
    L.fq_sym_row_scales.argtypes = [vp, vp, i64, i64, i32, i32, i32, i32, f32, f32, vp, vp, sz, vp]
    L.fq_sym_row_scales.restype = i32
    L.fq_w12_fwd_rows.argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    L.fq_w12_fwd_rows.restype = i32
    L.fq_sym_fwd_multi.argtypes = [i32, ctypes.POINTER(FwdTensor), i64, i32, i32, i32, f32, f32, vp]
    L.fq_sym_fwd_multi.restype = i32
    L.fq_ste_bwd_mask_multi.argtypes = [i32, ctypes.POINTER(BwdTensor), i64, f32, f32, i32, i32, vp]
    L.fq_ste_bwd_mask_multi.restype = i32
    rv = ctypes.POINTER(RowsView)
    L.fq_rowwise_fwd_v.argtypes = [i32, vp, rv, vp, rv, i64, i64, i32, i32, i32, f32, f32, vp, vp, sz, vp]
    L.fq_rowwise_fwd_v.restype = i32
    L.fq_sym_fwd_multi_v.argtypes = [i32, ctypes.POINTER(FwdTensorV), i64, i32, i32, i32, f32, f32, vp]
    L.fq_sym_fwd_multi_v.restype = i32
    L.fq_ste_bwd_mask_multi_v.argtypes = [i32, ctypes.POINTER(BwdTensorV), i64, f32, f32, i32, i32, vp]
    L.fq_ste_bwd_mask_multi_v.restype = i32
    L.fq_ste_bwd_v.argtypes = [vp, rv, vp, rv, vp, rv, i64, i64, f32, f32, vp, i32, vp]
    L.fq_ste_bwd_v.restype = i32
    L.fq_group_fwd.argtypes = [i32, vp, vp, i64, i64, i64, i32, i32, i32, i32, f32, f32, vp, vp, sz, vp]
    L.fq_group_fwd.restype = i32
    L.fq_mx_fwd.argtypes = [vp, vp, i64, i64, i32, i32, vp]
    L.fq_mx_fwd.restype = i32
    L.fq_mx_export.argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    L.fq_mx_export.restype = i32
    L.fq_mx_fwd_rot.argtypes = [vp, vp, i64, i64, i32, i32, vp]
    L.fq_mx_fwd_rot.restype = i32
    L.fq_mx_export_rot.argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    L.fq_mx_export_rot.restype = i32
    L.fq_block_rotate.argtypes = [vp, vp, i64, i64, i32, vp]
    L.fq_block_rotate.restype = i32
    L.fq_mx_fwd_ex.argtypes = [vp, vp, vp, i64, i64, i32, i32, i32, vp]
    L.fq_mx_fwd_ex.restype = i32
    L.fq_mx_export_ex.argtypes = [vp, vp, vp, i64, i64, i32, i32, i32, vp]
    L.fq_mx_export_ex.restype = i32
    L.fq_mx_ste_bwd.argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    L.fq_mx_ste_bwd.restype = i32
    L.fq_mx_gemm.argtypes = [vp, vp, i32, vp, vp, i32, vp, i64, i64, i64, i32, vp]
    L.fq_mx_gemm.restype = i32
    L.fqt_mx_fwd_cols.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp]
    L.fqt_mx_fwd_cols.restype = i32
    u64 = ctypes.c_uint64
    for name in ("fqs_mx_fwd", "fqs_mx_fwd_cols"):
        f = getattr(L, name)
        f.argtypes = [vp, vp, i64, i64, i32, i32, i32, u64, u64, vp]
        f.restype = i32
    L.fqs_mx_noise.argtypes = [u64, u64, i64, i64, i32, vp]
    L.fqs_mx_noise.restype = i32
    L.fqi_mx_dequant.argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    L.fqi_mx_dequant.restype = i32
    L.fql_kd_kl_fwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]
    L.fql_kd_kl_fwd.restype = i32
    L.fql_kd_kl_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]
    L.fql_kd_kl_bwd.restype = i32
    L.fqc_ce_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i32, i32, vp]
    L.fqc_ce_fwd.restype = i32
    L.fqc_ce_bwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i32, i32, vp]
    L.fqc_ce_bwd.restype = i32
    L.fqn_rms_norm_fwd.argtypes = [vp, vp, vp, vp, i64, i64, f32, i32, i32, vp]
    L.fqn_rms_norm_fwd.restype = i32
    L.fqn_rms_norm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i32, i32, vp]
    L.fqn_rms_norm_bwd.restype = i32
    L.fqn_rms_norm_bwd_parts.argtypes = [i64, i64]
    L.fqn_rms_norm_bwd_parts.restype = i64
    L.fqn_rms_norm_bwd_workspace_bytes.argtypes = [i64, i64]
    L.fqn_rms_norm_bwd_workspace_bytes.restype = sz
    L.fqa_swiglu_fwd.argtypes = [vp, vp, vp, i64, i64, i64, i64, i32, vp]
    L.fqa_swiglu_fwd.restype = i32
    L.fqa_swiglu_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, vp]
    L.fqa_swiglu_bwd.restype = i32
    L.fqr_rope_dense_strides.argtypes = [i64] * 7 + [ctypes.POINTER(i64)]
    L.fqr_rope_dense_strides.restype = i32
    L.fqr_rope_fwd.argtypes = [vp] * 7 + [i64] * 13 + [i32, i32, i32, vp]
    L.fqr_rope_fwd.restype = i32
    L.fqr_rope_bwd.argtypes = [vp] * 7 + [i64] * 19 + [i32, i32, i32, vp]
    L.fqr_rope_bwd.restype = i32
    L.fqs2_attn_softmax_fwd.argtypes = [vp] * 4 + [i64] * 7 + [f32, i32, i32, vp]
    L.fqs2_attn_softmax_fwd.restype = i32
    L.fqs2_attn_softmax_bwd.argtypes = [vp] * 5 + [i64] * 7 + [f32, i32, i32, vp]
    L.fqs2_attn_softmax_bwd.restype = i32
    return L


def lib():
    """The loaded library; raises FakeQuantLibraryError (never falls back) if unavailable."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise FakeQuantLibraryError(
                        f"{LIB_PATH} not found: build it with `python llm-qat_amd/build.py` "
                        "(or __graft_entry__.build()). There is no CPU/eager fallback.")
                try:
                    L = ctypes.CDLL(LIB_PATH)
                except OSError as e:  # e.g. libamdhip64 missing
                    raise FakeQuantLibraryError(f"cannot load {LIB_PATH}: {e}") from e
                _bind(L)
                v = L.fq_version()
                if v != ABI_VERSION:
                    raise FakeQuantLibraryError(f"ABI mismatch: library {v}, binding {ABI_VERSION}")
                _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().fq_last_error().decode(errors="replace")
        if rc in (-2,):  # FQ_ERR_BITS
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")
