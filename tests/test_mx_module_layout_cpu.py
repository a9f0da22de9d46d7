"""Where the MX training front-end lives: mx_quant holds it, utils_quant re-imports every name as the same object, the public surface and
what a constructed QuantizeLinear carries are what they were before the move.  No launch."""
import ast

import llm_qat_amd
from llm_qat_amd import mx_quant, utils_quant

MOVED = ("_BlockRotate", "_MXQuantizer", "_MXQuantizerSR",
         "MX_STE_MODES", "_check_mx_ste", "_check_mx_format", "_mx_check", "_mx_apply",
         "block_rotate", "mx_quantize", "mx_quantize_axis", "mx_quantize_sr",
         "_sr_lock", "_sr_state", "mx_sr_seed", "_sr_next",
         "MX_BACKWARD_ROUNDINGS", "_check_mx_backward_rounding", "_mx_backward_refusal", "_MXLinearBackward",
         "default_mx_formats", "default_mx_rotate", "default_mx_scale_rule", "default_mx_ste", "default_mx_backward_format",
         "default_mx_backward_rounding")
REGISTRY = ("_DEFAULTS", "_set_default", "_explicit_else")

MX_ATTRIBUTES = ("weight_format", "act_format", "mx_rotate", "mx_scale_rule", "mx_ste", "mx_backward_format", "mx_backward_rounding")

PUBLIC = ["SymQuantizer", "AsymQuantizer", "QuantizeLinear", "ops", "set_semantics", "get_semantics", "set_backward_mode", "get_backward_mode",
          "share_activation_quant", "enable_weight_quant_cache", "pair_operands", "quantize_kv", "fuse_low_bit_mean", "inplace_weight_grad", "pair_kv_hooks",
          "conservative", "cpp_node", "host_node", "stats", "reset_learned_state", "allow_cpu_tensors", "FakeQuantLibraryError",
          "group_quantize", "default_group_sizes", "mx_quantize", "default_mx_formats", "block_rotate", "default_mx_rotate", "default_mx_scale_rule", "default_mx_ste",
          "default_mx_backward_format", "mx_quantize_axis", "mx_quantize_sr", "mx_sr_seed", "default_mx_backward_rounding",
          "MXLinear", "convert_to_mx_inference"]


def test_every_moved_name_is_one_object_in_both_modules():
    for name in MOVED + REGISTRY:
        assert getattr(utils_quant, name) is getattr(mx_quant, name), name
    for name in MOVED + REGISTRY:
        obj = getattr(mx_quant, name)
        if hasattr(obj, "__module__") and callable(obj):
            assert obj.__module__ == mx_quant.__name__, name      # (defined there, not re-imported the other way round)


def test_mx_quant_does_not_import_utils_quant():
    with open(mx_quant.__file__) as f:
        tree = ast.parse(f.read())
    imported = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            imported.add(node.module or "")
            imported.update(a.name for a in node.names)
    assert imported, "the walk found no import at all"
    assert not [name for name in imported if "utils_quant" in name], imported


def test_the_public_surface_is_unchanged():
    assert llm_qat_amd.__all__ == PUBLIC
    for name in PUBLIC:
        assert hasattr(llm_qat_amd, name), name


def test_a_layer_without_an_mx_setting_carries_none_of_the_names():
    layer = utils_quant.QuantizeLinear(64, 8)
    assert not [name for name in MX_ATTRIBUTES if name in vars(layer)]
    assert [getattr(layer, name) for name in MX_ATTRIBUTES] == [None, None, False, "floor", "identity", None, None]   # the class attributes


def test_a_layer_with_explicit_settings_carries_those_and_no_others():
    layer = utils_quant.QuantizeLinear(64, 32, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3",
                                       mx_backward_format="mxfp8_e4m3", mx_backward_rounding="stochastic")
    assert {name: vars(layer)[name] for name in MX_ATTRIBUTES if name in vars(layer)} == {
        "weight_format": "mxfp4", "act_format": "mxfp8_e4m3", "mx_scale_rule": "floor", "mx_ste": "identity",    # (a layer with an MX operand
        "mx_backward_format": "mxfp8_e4m3", "mx_backward_rounding": "stochastic"}                                 # is assigned rule and gradient)
    assert "mx_rotate" not in vars(layer) and layer.mx_rotate is False
