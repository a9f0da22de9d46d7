"""The MX training front-end: the block rotation and the MX quantizers as autograd Functions, the public mx_quantize family, the MX linear
backward, the process defaults of QuantizeLinear's settings and the resolver of a layer's MX settings.  Stateless apart from those
defaults and the stochastic-rounding counter; utils_quant re-imports every name (import order: ops, compiled, mx_quant, utils_quant)."""
import threading

import torch
import torch.nn as nn

from . import compiled, ops

# what the QuantizeLinears constructed from now on take for the settings they are not given explicitly (the default_* setters below and
# utils_quant.default_group_sizes): (weight, activation) group sizes, (weight, activation) MX formats, and the MX operands' rotation,
# scale rule and gradient
_DEFAULTS = {"groups": (None, None), "mx": (None, None), "mx_rotate": False, "mx_scale_rule": "floor", "mx_ste": "identity", "mx_backward": None,
             "mx_backward_rounding": None}


def _set_default(name, value):
    prev, _DEFAULTS[name] = _DEFAULTS[name], value
    return prev


def _explicit_else(explicit, default, applies):
    """QuantizeLinear's rule for a setting it was not given: the explicit argument, else the process default where it applies to the layer"""
    return explicit if explicit is not None else (default if applies else None)


class _BlockRotate(torch.autograd.Function):
    """x R (ops.mx_rotate): R is symmetric and its own inverse, so the backward is the forward on the gradient.  Nothing is saved."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        return ops.mx_rotate(x)

    @staticmethod
    def backward(ctx, grad_output):
        return None if grad_output is None else _BlockRotate.apply(grad_output)


class _MXQuantizer(torch.autograd.Function):
    """MX block-scaled fake quantization (ops.mx_quantize_axis; DESIGN.md sections 13, 15, 16, 17), straight-through over the quantizer only.
    Without clip nothing is saved and the gradient is the incoming one itself (as the 1-/2-bit weight branches, _LowBitWeight; the saturated
    elements are not masked), times R under rotate -- the rotation is a linear map with its own gradient: one rotate launch.  clip: the
    forward launch also writes the saturation bitmap, the only tensor saved, and the backward is one launch: grad_x = grad_y where the bit
    is 1, +0.0 elsewhere (times R under rotate, in that launch).  axis -2 (the blocks run down the columns) serves neither rotate nor clip."""

    @staticmethod
    def forward(ctx, x, fmt, rotate, scale_rule, clip, axis):
        ctx.set_materialize_grads(False)
        ctx.rotate, ctx.clip = rotate, clip
        if not clip:
            return ops.mx_quantize_axis(x, fmt, rotate, scale_rule, False, axis)
        y, mask = ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=scale_rule, return_mask=True)
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        g, rotate = grad_output, ctx.rotate
        if g is not None and ctx.clip:
            mask, = ctx.saved_tensors
            if torch.is_grad_enabled():   # create_graph: the mask does not depend on the gradient (as _graph_aware) -- learn it on ones
                with torch.no_grad():
                    keep = ops.mx_ste_backward(torch.ones_like(g), mask)
                g = torch.where(keep != 0, g, torch.zeros((), dtype=g.dtype, device=g.device))
            else:
                g, rotate = ops.mx_ste_backward(g, mask, rotate), False   # (the rotation rides in that launch)
        if g is not None and rotate:
            g = _BlockRotate.apply(g)
        return g, None, None, None, None, None


MX_STE_MODES = ("identity", "clip")


def _check_mx_ste(ste, what="mx_quantize"):
    if not isinstance(ste, str) or ste not in MX_STE_MODES:
        raise ValueError(f"{what}: unknown ste {ste!r}: one of {', '.join(MX_STE_MODES)}")
    return ste


def _check_mx_format(fmt):
    """a setting that holds an MX format name or None"""
    if fmt is not None:
        ops._mx_format(fmt)


def _mx_check(x, fmt, rotate, scale_rule, ste, axis):
    """The argument checks of mx_quantize / mx_quantize_axis, in their order: tensor, axis, format, shape, rule, ste, what the column axis
    does not serve, the rotation's shape -> -1 | -2.  (Dynamo traces this: plain branches and lookups.)"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"mx_quantize: expected a torch.Tensor, got {type(x).__name__}")
    axis = ops.check_mx_axis(x.dim(), axis)
    if axis == -2:
        ops.check_mx_cols(tuple(x.shape), fmt)
    else:
        ops.check_mx(tuple(x.shape), fmt)
    ops.check_mx_scale_rule(scale_rule)
    _check_mx_ste(ste)
    if axis == -2 and (rotate or ste == "clip"):
        raise ValueError(f"mx_quantize: the column axis (axis=-2) does not serve {'rotate=True' if rotate else 'ste=clip'} yet")
    if rotate:
        ops.check_mx_rotate(tuple(x.shape), "mx_quantize")
    return axis


def _mx_apply(x, fmt, rotate, scale_rule, ste, axis=-1):
    """the MX quantizer of (rotate, scale_rule, ste, axis) on x, eager or while compiling; the arguments are checked by the callers"""
    clip = ste == "clip" and torch.is_grad_enabled() and x.requires_grad   # no backward will come: no bitmap is written
    if torch.compiler.is_compiling():
        return compiled.mx_fake_quant(x, fmt, rotate, scale_rule, clip, axis)
    return _MXQuantizer.apply(x, fmt, rotate, scale_rule, clip, axis)


def block_rotate(x):
    """x R: every run of 64 consecutive elements of the last dimension (a multiple of 64) times H64 / 8, the normalised 64 x 64 Sylvester
    Hadamard matrix; fp32 arithmetic, rounded once to x's dtype.  Differentiable; its backward is itself."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"block_rotate: expected a torch.Tensor, got {type(x).__name__}")
    ops.check_mx_rotate(tuple(x.shape), "block_rotate")
    if torch.compiler.is_compiling():
        return compiled.mx_block_rotate_op(x)
    return _BlockRotate.apply(x)


def mx_quantize(x, fmt, rotate=False, scale_rule="floor", ste="identity"):
    """OCP MX fake quantization ("mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e4m3", "mxfp8_e5m2"): every 32 consecutive elements of the
    last dimension share one power-of-two scale.  Same shape and dtype as x; the gradient is the identity (straight-through).
    rotate=True quantizes x R (block_rotate) in the same launch; the result is in the rotated basis and the gradient is grad R.
    scale_rule="ceil" takes the shared exponent under which no element saturates ("floor": OCP's round-down rule, under which the top
    binade of a block may).  ste="clip" zeroes the gradient of the elements that saturation changed: the forward launch also writes a
    bitmap (numel / 8 bytes, all that is saved) and the backward is one launch, with or without the rotation."""
    return _mx_apply(x, fmt, bool(rotate), scale_rule, ste, _mx_check(x, fmt, rotate, scale_rule, ste, -1))


def mx_quantize_axis(x, fmt, rotate=False, scale_rule="floor", ste="identity", axis=-1):
    """mx_quantize with a choice of the axis the blocks run along: -1 (or ndim - 1) is mx_quantize itself.  -2 (or ndim - 2): the blocks
    run down the columns -- 32 consecutive elements of the second-to-last dimension (a multiple of 32; the last one is free) share a
    scale, which is what a product that contracts over that axis needs (the backward GEMMs of a linear layer).  One launch, a contiguous
    result, the identity gradient; the rotation and ste="clip" are not served along that axis (ValueError).  (The same checks and
    quantizer as mx_quantize, whose own parameter list is pinned by tests/test_mx_rules_cpu.py.)"""
    return _mx_apply(x, fmt, bool(rotate), scale_rule, ste, _mx_check(x, fmt, rotate, scale_rule, ste, axis))


class _MXQuantizerSR(torch.autograd.Function):
    """ops.mx_quantize_sr, straight-through: nothing is saved and the gradient is the incoming one itself (no launch backward)."""

    @staticmethod
    def forward(ctx, x, fmt, seed, stream, scale_rule, axis):
        ctx.set_materialize_grads(False)
        return ops.mx_quantize_sr(x, fmt, seed, stream, scale_rule, axis)

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output, None, None, None, None, None


def mx_quantize_sr(x, fmt, seed, stream=0, scale_rule="floor", axis=-1):
    """MX fake quantization with stochastic rounding: as mx_quantize_axis, but every element goes to one of its two
    grid neighbours with the probabilities that make the result unbiased (E[y] = x; exactly so under scale_rule="ceil", under "floor" the
    top binade of a block still clips) -- the rounding for a gradient operand.  The noise is Philox4x32-10 on (seed, stream, flat element
    index): Python ints in [0, 2^64); the same pair reproduces the result bit for bit.  Same shape and dtype as x, contiguous; the gradient
    is the identity and costs no launch.  Along axis=-2 the last dimension must be whole 16-byte vectors.  Not served while torch.compile
    traces (NotImplementedError).  A launch captured into a hipGraph carries its seed and stream, so every replay repeats its noise."""
    if torch.compiler.is_compiling():
        raise NotImplementedError("mx_quantize_sr is not served while torch.compile traces (seed and stream would be baked into the graph): "
                                  "call it eagerly")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"mx_quantize_sr: expected a torch.Tensor, got {type(x).__name__}")
    return _MXQuantizerSR.apply(x, fmt, seed, stream, scale_rule, axis)


# The noise of the module path (QuantizeLinear(mx_backward_rounding="stochastic")): one process seed and one process-wide stream counter.
# Every stochastic launch of a module backward takes the counter's next value under the lock, Qr(g) before Qc(g) within a backward, so a
# fixed program with a fixed seed reproduces bit for bit.  Data-parallel ranks should be given different seeds by the caller.
_sr_lock = threading.Lock()
_sr_state = {"seed": None, "next": 0}


def mx_sr_seed(seed):
    """Set the seed of the stochastic backward roundings of this process and reset their stream counter to 0.  -> the previous seed (None
    if none was set; then the first stochastic backward would have taken torch.initial_seed() & (2^64 - 1))."""
    ops.check_mx_sr_word(seed, "seed", "mx_sr_seed")
    with _sr_lock:
        prev, _sr_state["seed"], _sr_state["next"] = _sr_state["seed"], seed, 0
    return prev


def _sr_next():
    """-> (seed, stream id) of the next stochastic launch of a module backward"""
    with _sr_lock:
        if _sr_state["seed"] is None:
            _sr_state["seed"] = torch.initial_seed() & ((1 << 64) - 1)
        stream = _sr_state["next"]
        _sr_state["next"] = (stream + 1) & ((1 << 64) - 1)
        return _sr_state["seed"], stream


MX_BACKWARD_ROUNDINGS = ("nearest", "stochastic")


def _check_mx_backward_rounding(mode, what="mx_backward_rounding"):
    if mode is not None and (not isinstance(mode, str) or mode not in MX_BACKWARD_ROUNDINGS):
        raise ValueError(f"{what}: unknown rounding {mode!r}: one of {', '.join(MX_BACKWARD_ROUNDINGS)} (or None)")


def default_mx_backward_rounding(mode):
    """The rounding ("nearest" / "stochastic", None: nearest) the QuantizeLinears constructed from now on take for the gradient operand of
    their MX backward GEMMs when their own mx_backward_rounding is not given.  Applies only to layers that have a backward format
    (mx_backward_format or its process default).  -> the previous mode."""
    _check_mx_backward_rounding(mode, "default_mx_backward_rounding")
    return _set_default("mx_backward_rounding", mode)


def default_mx_formats(weight=None, act=None):
    """MX formats the QuantizeLinears constructed from now on take for the operands they quantize (w_bits < 32 / a_bits < 32, not
    layerwise, no explicit group size) when their own weight_format / act_format are not given (None: the integer quantizers).  Lets
    unchanged model code (LLM-QAT's train.py) train for MXFP4.  -> the previous pair."""
    _check_mx_format(weight)
    _check_mx_format(act)
    return _set_default("mx", (weight, act))


def default_mx_rotate(flag):
    """Whether the QuantizeLinears constructed from now on whose two operands both resolve to an MX format, and whose in_features is a
    multiple of 64, rotate their operands (mx_rotate=True) when their own mx_rotate is not given.  Layers the rotation does not apply to
    stay unrotated.  Lets unchanged model code train with the rotation.  -> the previous flag."""
    return _set_default("mx_rotate", bool(flag))


def default_mx_scale_rule(rule):
    """The scale rule ("floor" / "ceil") the QuantizeLinears constructed from now on take for their MX operands when their own
    mx_scale_rule is not given.  Layers without an MX operand are not affected.  -> the previous rule."""
    ops.check_mx_scale_rule(rule, "default_mx_scale_rule")
    return _set_default("mx_scale_rule", rule)


def default_mx_ste(mode):
    """The gradient ("identity" / "clip") the QuantizeLinears constructed from now on take for their MX operands when their own mx_ste
    is not given.  Layers without an MX operand are not affected.  -> the previous mode."""
    _check_mx_ste(mode, "default_mx_ste")
    return _set_default("mx_ste", mode)


def default_mx_backward_format(fmt):
    """The MX format the QuantizeLinears constructed from now on run their backward GEMMs in (mx_backward_format) when their own is not
    given; None: the backward GEMMs stay in the tensors' dtype.  Applies only to layers that qualify: both operands in an MX format, no
    rotation, the identity gradient, out_features a multiple of 32.  -> the previous format."""
    _check_mx_format(fmt)
    return _set_default("mx_backward", fmt)


def _mx_backward_refusal(layer):
    """why `layer` cannot run its backward GEMMs on MX operands, or None"""
    if layer.weight_format is None or layer.act_format is None:
        return "it needs both operands in an MX format (weight_format and act_format)"
    if layer.mx_rotate:
        return "the column axis does not serve the rotation yet (mx_rotate must be False)"
    if layer.mx_ste != "identity":
        return 'the column axis does not serve the clip gradient yet (mx_ste must be "identity")'
    if layer.out_features % ops.MX_BLOCK:
        return f"dX = dY W contracts over out_features, which must be a multiple of {ops.MX_BLOCK}, got {layer.out_features}"
    return None


def _mx_resolve(layer, weight_format, act_format, mx_rotate, mx_scale_rule, mx_ste, mx_backward_format, mx_backward_rounding,
                w_bits, a_bits, weight_layerwise, act_layerwise, weight_group_size, act_group_size):
    """The MX settings of a QuantizeLinear under construction, from its seven explicit arguments and the process defaults: an explicit
    argument is checked and must apply to the layer (ValueError), a process default applies only where it means something.  Each setting
    that resolves becomes a plain instance attribute of `layer`; the others stay the class attributes."""
    # MX formats: an explicit argument always applies (and excludes that operand's group size and layerwise flag); the process default
    # (default_mx_formats) applies to the operands this layer quantizes, and then no default group size does
    for (name, given, default, bits, layerwise, group, shape) in (
            ("weight", weight_format, _DEFAULTS["mx"][0], w_bits, weight_layerwise, weight_group_size, tuple(layer.weight.shape)),
            ("act", act_format, _DEFAULTS["mx"][1], a_bits, act_layerwise, act_group_size, (layer.in_features,))):
        if given is not None and (group is not None or layerwise):
            raise ValueError(f"{name}_format cannot be combined with {name}_group_size or {name}_layerwise")
        fmt = _explicit_else(given, default, bits < 32 and group is None and not layerwise)
        if fmt is not None:
            ops.check_mx(shape, fmt)
            setattr(layer, name + "_format", fmt)
    # the rotation: an explicit True needs both operands in an MX format (rotating one alone changes the product) and whole 64-runs;
    # the process default (default_mx_rotate) applies to the layers that meet both
    both_mx = layer.weight_format is not None and layer.act_format is not None
    if mx_rotate:
        if not both_mx:
            raise ValueError("mx_rotate needs both operands in an MX format (weight_format and act_format): (x R)(W R)^T = x W^T only "
                             "when both are rotated")
        ops.check_mx_rotate((layer.in_features,), "mx_rotate")
        layer.mx_rotate = True
    elif mx_rotate is None and _DEFAULTS["mx_rotate"] and both_mx and layer.in_features % ops.MX_ROTATE == 0:
        layer.mx_rotate = True
    # scale rule and gradient of the MX operands: an explicit argument needs one; the process defaults apply to the layers that have one
    any_mx = layer.weight_format is not None or layer.act_format is not None
    for name, given, check in (("mx_scale_rule", mx_scale_rule, ops.check_mx_scale_rule), ("mx_ste", mx_ste, _check_mx_ste)):
        if given is not None:
            check(given, name)
            if not any_mx:
                raise ValueError(f"{name} applies to MX operands: this layer has neither weight_format nor act_format")
        if any_mx:
            setattr(layer, name, _explicit_else(given, _DEFAULTS[name], True))
    # the backward GEMMs in an MX format: an explicit format needs a layer that qualifies (_mx_backward_refusal); the process default
    # (default_mx_backward_format) applies to the layers that do
    why = _mx_backward_refusal(layer)
    if mx_backward_format is not None:
        _check_mx_format(mx_backward_format)
        if why is not None:
            raise ValueError(f"mx_backward_format: {why}")
        layer.mx_backward_format = mx_backward_format
    elif _DEFAULTS["mx_backward"] is not None and why is None:
        layer.mx_backward_format = _DEFAULTS["mx_backward"]
    # the rounding of the gradient operand: an explicit value needs a backward format in force; the process default
    # (default_mx_backward_rounding) applies to the layers that have one
    _check_mx_backward_rounding(mx_backward_rounding)
    if mx_backward_rounding is not None and layer.mx_backward_format is None:
        raise ValueError("mx_backward_rounding applies to the MX backward GEMMs: this layer has no mx_backward_format in force")
    mode = _explicit_else(mx_backward_rounding, _DEFAULTS["mx_backward_rounding"], layer.mx_backward_format is not None)
    if mode is not None:
        layer.mx_backward_rounding = mode


class _MXLinearBackward(torch.autograd.Function):
    """F.linear(Qr(x), Qr(W)) whose two backward GEMMs run on MX-quantized operands, each blocked along its contraction axis (DESIGN.md
    section 17; Qr / Qc: ops.mx_quantize / ops.mx_quantize_axis(axis=-2), format fb, the layer's scale rule):
        dX = Qr(g) Qc(W)         both blocked along `out`
        dW = Qc(g)^T Qc(x)       both blocked along the tokens (zero rows pad them to a multiple of 32: no amax and no sum changes)
    The operands quantized backward are the ORIGINAL x and W cast to the output's dtype, as the microscaling emulation libraries do, so x
    and W themselves are what is saved.  An operand of a gradient nobody needs is not quantized.
    stochastic: the two quantizations of the gradient operand, Qr(g) and then Qc(g) (after the zero-row padding),
    round stochastically (ops.mx_quantize_sr), each on the process seed and the next stream id (_sr_next); Qc(W) and Qc(x) stay nearest.
    The launches stay one row-kernel and three column-kernel launches and two GEMMs."""

    @staticmethod
    def forward(ctx, x, w, weight_format, act_format, scale_rule, fb, stochastic):
        ctx.cfg = (fb, scale_rule)
        ctx.stochastic = stochastic
        ctx.save_for_backward(x, w)
        wq = ops.mx_quantize(w, weight_format, scale_rule=scale_rule)
        return nn.functional.linear(ops.mx_quantize(x, act_format, scale_rule=scale_rule), wq)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        fb, rule = ctx.cfg
        need_x, need_w = ctx.needs_input_grad[:2]
        gx = gw = None
        with torch.autocast("cuda", enabled=False):   # every operand is cast to d explicitly
            d = g.dtype
            g2 = g.reshape(-1, w.shape[0]).contiguous()
            if ctx.stochastic:
                def qg(t, axis):
                    return ops.mx_quantize_sr(t, fb, *_sr_next(), scale_rule=rule, axis=axis)
            else:
                def qg(t, axis):
                    return ops.mx_quantize_axis(t, fb, scale_rule=rule, axis=axis)
            if need_x:
                gx2 = torch.matmul(qg(g2, -1), ops.mx_quantize_axis(w.to(d), fb, scale_rule=rule, axis=-2))
                gx = gx2.reshape(x.shape).to(x.dtype)
            if need_w:
                x2 = x.reshape(-1, w.shape[1]).to(d)
                pad = -g2.shape[0] % ops.MX_BLOCK
                if pad:
                    ops.mx_counts["mx_copy_route"] += 1
                    g2, x2 = nn.functional.pad(g2, (0, 0, 0, pad)), nn.functional.pad(x2, (0, 0, 0, pad))
                gw = torch.matmul(qg(g2, -2).t(), ops.mx_quantize_axis(x2, fb, scale_rule=rule, axis=-2)).to(w.dtype)
        return gx, gw, None, None, None, None, None
