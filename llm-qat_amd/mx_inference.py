"""Inference in the arithmetic MX fake quantization simulates: a linear layer whose weight is kept as MX codes (4.25 bits per element for
mxfp4) and whose product runs on gfx950's block-scaled matrix instruction (ops.mx_matmul)."""
import torch
from torch import nn

from . import compiled, ops
from .utils_quant import QuantizeLinear

# The recommended dequant_above of MXLinear, from the layer timings of DESIGN.md section 21 (tools/mx_dequant_bench.py on one MI355X, the
# three LLaMA-7B projections, W mxfp4 / A mxfp8_e4m3, bf16): the smallest measured token count above which the dequantized route beats the
# GEMM route on all three shapes by more than the runs' spread; None would say there is no such count.  At 64 tokens the GEMM route still
# wins on 4096 -> 11008 (47 against 57 us); from 128 tokens on the dequantized route wins everywhere (62 / 87 / 47 against 81 / 158 / 77 us).
# Offered, not applied: MXLinear's own default is dequant_above=None.
DEQUANT_ABOVE_DEFAULT = 64


def _check_dequant_above(n):
    """-> n, None or a Python int >= 0; ValueError for anything else (bools and strings included)"""
    if n is None or (isinstance(n, int) and not isinstance(n, bool) and n >= 0):
        return n
    raise ValueError(f"MXLinear: dequant_above={n!r}: None (every call runs the MX GEMM) or an int >= 0 (calls with more rows than that "
                     "run the dequantized route)")


def _exportable(fmt):
    """whether the MX GEMM reads this format's export (mxfp4 / mxfp8_*: FP6 has no packing)"""
    return fmt in ops.MX_GEMM_FORMATS


def _k_refusal(in_features):
    """why the MX GEMM kernel does not serve this K, or None"""
    if in_features <= 0 or in_features % ops.MX_GEMM_KSTEP:
        return f"in_features={in_features} is not a positive multiple of {ops.MX_GEMM_KSTEP}, the K step of the MX GEMM kernel"
    return None


def _why_not(layer):
    """None if `layer` can become an MXLinear, else the reason."""
    if not isinstance(layer, QuantizeLinear):
        return f"expected a QuantizeLinear, got {type(layer).__name__}"
    for what, fmt in (("weight_format", layer.weight_format), ("act_format", layer.act_format)):
        if fmt is None:
            return f"{what} is not set: the layer does not quantize that operand to an MX format"
        if not _exportable(fmt):
            return f"{what}={fmt!r} has no export packing (one of {', '.join(ops.MX_GEMM_FORMATS)})"
    return _k_refusal(layer.in_features)


class MXLinear(nn.Module):
    """y = mx_matmul(mx_export(x, act_format), W) (+ bias): two launches, W held as `weight_elements` / `weight_scales` buffers (the
    ops.MXExport of the trained weight), no bf16 weight.  Inference only: not differentiable.  The output has x's dtype; the bias is added
    in that dtype (cast to it when the module's dtype differs).
    rotate=True: the buffers hold the export of W R and the activation's export launch rotates x, so the product
    is (x R)(W R)^T -- still two launches, the same GEMM.  A constructor attribute like the formats: it is not in the state_dict.
    scale_rule: the shared-exponent rule of the activation's export launch ("floor" / "ceil"); the weight buffers
    carry whatever rule exported them, and the GEMM reads the scale bytes as they are.  A constructor attribute too.
    dequant_above: None -- every call runs as above.  An int n >= 0: a call whose x has more than n rows (the
    product of its leading dimensions) runs F.linear(mx_quantize(x, act_format, rotate, scale_rule), mx_dequantize(W, x.dtype)) (+ bias)
    instead -- the fake-quantize launch, one dequantize launch, the library GEMM: the arithmetic of QuantizeLinear.eval(), bit for bit,
    with W still read from its codes; a call with n rows or fewer runs the MX GEMM.  0 sends every call there.  That route allocates a
    transient [out_features, in_features] tensor in x's dtype per call (90 MB for a bf16 4096 x 11008 projection), freed when the call
    returns; the weight stays compressed between calls.  DEQUANT_ABOVE_DEFAULT is the measured recommendation.  A constructor attribute
    like rotate: not in the state_dict."""

    def __init__(self, in_features, out_features, weight_format="mxfp4", act_format="mxfp8_e4m3", bias=False, device=None, dtype=None,
                 rotate=False, scale_rule="floor", dequant_above=None):
        super().__init__()
        for what, fmt in (("weight_format", weight_format), ("act_format", act_format)):
            if not _exportable(fmt):
                raise ValueError(f"{what}={fmt!r}: one of {', '.join(ops.MX_GEMM_FORMATS)}")
        why = _k_refusal(in_features)
        if why is not None:
            raise ValueError(why)
        self.in_features, self.out_features = in_features, out_features
        self.weight_format, self.act_format = weight_format, act_format
        self.rotate = bool(rotate)   # (in_features % 128 == 0 holds whole 64-element rotation runs)
        ops.check_mx_scale_rule(scale_rule, "MXLinear")
        self.scale_rule = scale_rule
        self.dequant_above = _check_dequant_above(dequant_above)
        ebytes = in_features // 2 if weight_format == "mxfp4" else in_features
        self.register_buffer("weight_elements", torch.zeros(out_features, ebytes, dtype=torch.uint8, device=device))
        self.register_buffer("weight_scales", torch.zeros(out_features, in_features // ops.MX_BLOCK, dtype=torch.uint8, device=device))
        self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device) if bias else None)

    @classmethod
    def from_quantize_linear(cls, layer, dequant_above=None):
        """The inference form of a QuantizeLinear whose weight and activations both resolve to mxfp4 / mxfp8_* (explicitly or through
        default_mx_formats) and whose in_features the kernel serves; ValueError names what is missing otherwise.  The weight is exported
        once (one launch), on the device it lives on.  dequant_above: the new module's (MXLinear's argument)."""
        why = _why_not(layer)
        if why is not None:
            raise ValueError(f"MXLinear.from_quantize_linear: {why}")
        has_bias = getattr(layer, "bias", None) is not None
        m = cls(layer.in_features, layer.out_features, layer.weight_format, layer.act_format, bias=has_bias, device=layer.weight.device,
                dtype=layer.weight.dtype, rotate=layer.mx_rotate, scale_rule=layer.mx_scale_rule, dequant_above=dequant_above)
        e = layer.export_weight()
        m.weight_elements.copy_(e.elements)
        m.weight_scales.copy_(e.scales)
        if has_bias:
            m.bias.copy_(layer.bias.detach())
        return m

    def weight_export(self):
        """the weight as an ops.MXExport (shares the buffers)"""
        return ops.MXExport(self.weight_elements, self.weight_scales, self.weight_format, (self.out_features, self.in_features),
                            torch.float32 if self.bias is None else self.bias.dtype, self.rotate)

    def forward(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXLinear is an inference module and is not differentiable: call it under torch.no_grad() or on a detached input")
        if self.dequant_above is not None and x.numel() // self.in_features > self.dequant_above:
            return self._forward_dequant(x)
        if torch.compiler.is_compiling():
            ae, asc = compiled.mx_export(x, self.act_format, self.rotate, self.scale_rule)
            y = compiled.mx_matmul_op(ae, asc, self.act_format, self.weight_elements, self.weight_scales, self.weight_format, list(x.shape), x.dtype)
        else:
            a = ops.mx_export(x, self.act_format, rotate=self.rotate, scale_rule=self.scale_rule)
            y = ops.mx_matmul_tensors(a.elements, a.scales, a.fmt, self.weight_elements, self.weight_scales, self.weight_format, a.shape, x.dtype)
        return self._add_bias(y)

    def _forward_dequant(self, x):
        """the dequantized route: x fake-quantized (one launch), W expanded to x's dtype (one launch), the library GEMM"""
        shape = (self.out_features, self.in_features)
        if torch.compiler.is_compiling():
            xq = compiled.mx_fake_quant(x, self.act_format, self.rotate, self.scale_rule, False)
            w = compiled.mx_dequant_op(self.weight_elements, self.weight_scales, self.weight_format, list(shape), x.dtype)
        else:
            xq = ops.mx_quantize(x, self.act_format, rotate=self.rotate, scale_rule=self.scale_rule)
            w = ops.mx_dequantize_tensors(self.weight_elements, self.weight_scales, self.weight_format, shape, x.dtype)
        return self._add_bias(nn.functional.linear(xq, w))

    def _add_bias(self, y):
        # the bias in x's dtype: the output dtype follows x (fp16 + bf16 would promote the sum to fp32)
        return y if self.bias is None else y + self.bias.to(y.dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, weight_format={self.weight_format!r}, "
                f"act_format={self.act_format!r}, bias={self.bias is not None}" + (", rotate=True" if self.rotate else "")
                + (f", scale_rule={self.scale_rule!r}" if self.scale_rule != "floor" else "")
                + (f", dequant_above={self.dequant_above}" if self.dequant_above is not None else ""))


def convert_to_mx_inference(model, dequant_above=None):
    """Replace, in place, every QuantizeLinear of `model` that MXLinear.from_quantize_linear accepts; integer-quantized, group-wise, FP6
    layers and those whose in_features the kernel does not serve stay as they are.  dequant_above: what every new MXLinear gets.  -> the number of layers replaced."""
    _check_dequant_above(dequant_above)
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, QuantizeLinear) and _why_not(child) is None:
                setattr(parent, name, MXLinear.from_quantize_linear(child, dequant_above=dequant_above))
                n += 1
    return n
