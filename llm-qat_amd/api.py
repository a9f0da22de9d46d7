"""Public surface of the package."""
from . import ops
from . import distill   # llm_qat_amd.distill: kd_kl_loss, install (its names stay in the submodule)
from . import lm_loss   # llm_qat_amd.lm_loss: cross_entropy, causal_lm_loss, CrossEntropyLoss, install (likewise)
from . import norm      # llm_qat_amd.norm: rms_norm, RMSNorm, install, convert (likewise)
from . import mlp       # llm_qat_amd.mlp: swiglu, SwiGLUMLP, install, convert (likewise)
from . import rope      # llm_qat_amd.rope: apply_rotary_pos_emb, rotary, install (likewise)
from . import attention  # llm_qat_amd.attention: attn_softmax, install, convert (likewise)
from .cpu_tensors import allow_cpu_tensors
from ._lib import FakeQuantLibraryError
from .ops import get_semantics, set_semantics
from .mx_inference import MXLinear, convert_to_mx_inference
from .utils_quant import (AsymQuantizer, QuantizeLinear, SymQuantizer, conservative, cpp_node, default_group_sizes, default_mx_formats, default_mx_rotate, default_mx_scale_rule, default_mx_ste, default_mx_backward_format, enable_weight_quant_cache, fuse_low_bit_mean,
                          get_backward_mode, block_rotate, group_quantize, host_node, mx_quantize, mx_quantize_axis, mx_quantize_sr, mx_sr_seed, default_mx_backward_rounding,
                          inplace_weight_grad, pair_kv_hooks, pair_operands, quantize_kv, reset_learned_state, set_backward_mode, share_activation_quant, stats)

__version__ = "0.5.0"
__all__ = ["SymQuantizer", "AsymQuantizer", "QuantizeLinear", "ops", "set_semantics", "get_semantics", "set_backward_mode", "get_backward_mode",
           "share_activation_quant", "enable_weight_quant_cache", "pair_operands", "quantize_kv", "fuse_low_bit_mean", "inplace_weight_grad", "pair_kv_hooks",
           "conservative", "cpp_node", "host_node", "stats", "reset_learned_state", "allow_cpu_tensors", "FakeQuantLibraryError",
           "group_quantize", "default_group_sizes", "mx_quantize", "default_mx_formats", "block_rotate", "default_mx_rotate", "default_mx_scale_rule", "default_mx_ste",
           "default_mx_backward_format", "mx_quantize_axis", "mx_quantize_sr", "mx_sr_seed", "default_mx_backward_rounding",
           "MXLinear", "convert_to_mx_inference"]
