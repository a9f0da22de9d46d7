"""GPU tier of the fused attention softmax (llm_qat_amd.attention): the kernels against float64 under the caps that the
eager chain set (tests/attn_softmax_reference.py), ten launch shapes (the whole ladder: tests/test_gpu_attn_softmax_shapes.py), the device's
scalar rule and the roundings in front of the softmax bit for bit, masked rows, special values, memory, counters, torch.compile and a tiny
LLaMA through install."""
import types

import numpy as np
import pytest
import torch

import attn_softmax_reference as R

pytestmark = pytest.mark.gpu

BF, H, F = torch.bfloat16, torch.float16, torch.float32
PAIRS = [(BF, BF), (BF, F), (H, H), (H, F), (F, F), (BF, None), (H, None), (F, None)]
HD = R.HEAD_DIM


def _mods():
    from llm_qat_amd import attention, ops
    return attention, ops


def fused(x, mask, g, hd=HD):
    _, ops = _mods()
    y, stats = ops.attn_softmax_forward(x, mask, hd)
    return y, ops.attn_softmax_backward(g, x, mask, stats, hd), stats


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- error caps ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_live_chain_sits_where_the_caps_were_measured():
    """the eager fp32 chain on this device: within a quarter of each cap (the caps are 4 x its largest measure) and above a sixteenth"""
    m = R.eager_measures("cuda")
    cy, cdx = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print("eager fp32 chain on the device: C_y", cy, "C_dx", cdx, "caps", R.Y_CAP, R.DX_CAP)
    assert R.Y_CAP / 16 < cy <= R.Y_CAP / 4 and R.DX_CAP / 16 < cdx <= R.DX_CAP / 4


@pytest.mark.parametrize("ds,dm", PAIRS, ids=lambda d: str(d).replace("torch.", ""))
def test_y_and_dx_are_within_the_caps_over_the_case_list(ds, dm):
    worst = [0.0, 0.0]
    for name, (x, pat, g) in R.CASES().items():
        if (dm is None) != (pat is None):
            continue
        x, g, mask = x.cuda().to(ds), g.cuda().to(ds), (R.mask_of(pat, dm, "cuda") if dm is not None else None)
        ref = R.ref64(x, mask, g)
        y, dx, _ = fused(x, mask, g)
        cy, cdx = R.c_y(y, ref), R.c_dx(dx, ref)
        worst = [max(worst[0], cy), max(worst[1], cdx)]
        assert cy <= R.Y_CAP and cdx <= R.DX_CAP, (name, cy, cdx)
    print(ds, dm, "C_y", worst[0], "C_dx", worst[1])


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------------------
def _shape_case(B, Hh, T, S, ds, dm, seed, expand=False, offset=0):
    gen = torch.Generator().manual_seed(seed)
    n = B * Hh * T * S

    def make(dt):
        flat = torch.empty(n + 8, dtype=dt, device="cuda")
        return flat[offset:offset + n].view(B, Hh, T, S)          # offset 1: storage that is not 16-byte aligned
    x, g = make(ds), make(ds)
    x.copy_((torch.randn(B, Hh, T, S, generator=gen) * 20).to(ds))
    g.copy_(torch.randn(B, Hh, T, S, generator=gen).to(ds))
    mask = None
    if dm is not None:
        keep = torch.rand(B, 1, T, S, generator=gen) < 0.7
        keep[..., 0] = True
        m = torch.where(keep, 0.0, torch.finfo(dm).min).to(dm)
        mask = m[:1].cuda().expand(B, 1, T, S) if expand else m.cuda()
    return x, mask, g


def _check(x, mask, g, what):
    ref = R.ref64(x, mask, g)
    y, dx, stats = fused(x, mask, g)
    cy, cdx = R.c_y(y, ref), R.c_dx(dx, ref)
    assert cy <= R.Y_CAP and cdx <= R.DX_CAP, (what, cy, cdx)
    assert y.is_contiguous() and dx.is_contiguous() and y.dtype == x.dtype and dx.dtype == x.dtype
    assert torch.isfinite(stats).all()


@pytest.mark.parametrize("S", [1, 7, 33, 64, 255, 2047, 2048, 2049, 4099, 8200])
def test_every_launch_shape_alignment_and_pair(S):
    """(the full ladder, every register rung and every boundary of it: tests/test_gpu_attn_softmax_shapes.py)"""
    for ds, dm in PAIRS:
        for offset in (0, 1):
            _check(*_shape_case(1, 1, 5, S, ds, dm, S + offset, offset=offset), what=(S, ds, dm, offset))


@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_the_wave_paths_row_counts(rows):
    for ds, dm in ((BF, F), (F, None), (H, H)):
        _check(*_shape_case(1, 1, rows, 264, ds, dm, rows), what=(rows, ds, dm))


@pytest.mark.parametrize("S", [33, 264, 2056])
def test_mask_batch_strides_heads_and_decode(S):
    for ds, dm in ((BF, F), (BF, BF), (F, F)):
        _check(*_shape_case(2, 3, 4, S, ds, dm, S, expand=True), what=("expanded", S, ds, dm))      # batch stride 0
        _check(*_shape_case(2, 3, 4, S, ds, dm, S + 1), what=("batched", S, ds, dm))                # a real batch stride
    _check(*_shape_case(2, 3, 1, 33, BF, F, 5), what="decode")                                      # T = 1


def test_a_mask_row_is_the_tokens_own_in_every_head_and_batch():
    """distinct masks per (batch, token): a wrong row or batch index shows against the chain's NaN-free zero pattern"""
    x, mask, g = _shape_case(2, 3, 4, 40, BF, F, 11)
    y, _, _ = fused(x, mask, g)
    assert torch.equal(y == 0, (mask < 0).expand_as(y))


# ---- the scalar rule and the roundings in front of the softmax ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,dm", [(BF, BF), (BF, F), (H, H), (H, F)], ids=lambda d: str(d).replace("torch.", ""))
def test_two_unmasked_columns_give_the_sigmoid_of_z_of_bit_for_bit(ds, dm):
    """rows with exactly two unmasked columns: y is a function of z1 - z0 alone, so the kernel's y must be rb(sigmoid64(+-(z1 - z0))) of
    z_of on the device.  Elements whose float64 value lies within Y_CAP 2^-24 (relative) of a rounding boundary are excepted and counted:
    below 1 %, with the chain held to the same check.  A wrong inv, a missing rounding or a wrong P moves z by 2^-9 relative.
    The excepted share is a property of the format and the cap, not of the kernel: the band 2 Y_CAP 2^-24 p over fp16's spacing of
    2^-11 .. 2^-10 p is 0.9 .. 1.8 % of the values in fp16's normal range (an eighth of that for bf16), so the scores are spread
    (sigma 120) until half of the rows saturate to 0 and 1, where no boundary is near: measured at sigma 60, fp16: 1.11 %."""
    gen = torch.Generator().manual_seed(7)
    T, S = 4096, 40
    x = (torch.randn(1, 1, T, S, generator=gen) * 120).to(ds).cuda()
    cols = torch.stack([torch.randperm(S, generator=gen)[:2] for _ in range(T)])
    keep = torch.zeros(T, S, dtype=torch.bool)
    keep[torch.arange(T).unsqueeze(1), cols] = True
    mask = torch.where(keep, 0.0, torch.finfo(dm).min).to(dm).reshape(1, 1, T, S).cuda()
    _, z = R.z_of(x, mask)
    zz = z.double()[0, 0][keep.cuda()].reshape(T, 2)
    p64 = torch.sigmoid(torch.stack([zz[:, 0] - zz[:, 1], zz[:, 1] - zz[:, 0]], 1))
    want = p64.to(ds)
    # distance of p64 to the nearest rounding boundary of ds, relative: the midpoint between want and its neighbour on p64's side
    w64 = want.double()
    m, e = torch.frexp(w64)                                          # w = m 2^e, m in [0.5, 1)
    sb = 8 if ds == BF else 11                                       # significant bits
    ulp = torch.ldexp(torch.ones_like(w64), e - sb)
    if ds == H:
        ulp = torch.where(w64 < 2.0 ** -14, torch.full_like(ulp, 2.0 ** -24), ulp)      # fp16's subnormals, zero included
    down = torch.where((m == 0.5) & (ulp > 2.0 ** -24), ulp / 2, ulp)      # below a power of two the spacing halves
    nxt = torch.where(p64 > w64, w64 + ulp, w64 - down)
    near = ((p64 - (w64 + nxt) / 2).abs() <= R.Y_CAP * R.UNIT * p64)
    assert near.float().mean() < 0.01, near.float().mean()
    attention, _ = _mods()
    for name, y in (("kernel", attention.attn_softmax(x, mask, HD)), ("chain", R.chain(x, mask))):
        got = y[0, 0][keep.cuda()].reshape(T, 2)
        bad = (bits(got) != bits(want)) & ~near
        print(name, ds, dm, "differ:", int((bits(got) != bits(want)).sum()), "near a boundary:", int(near.sum()), "of", near.numel())
        assert not bad.any(), (name, int(bad.sum()))
        assert (y[0, 0][~keep.cuda()] == 0).all()


# ---- mask rows ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,dm", PAIRS[:5], ids=lambda d: str(d).replace("torch.", ""))
def test_fully_masked_and_minus_inf_rows(ds, dm):
    S = 33                                                           # padding slots: a row whose real maximum is the clamp value sums to 1
    x, _, g = _shape_case(1, 2, 4, S, ds, None, 3)
    x = x / 8                                                        # small scores: min + x rounds to min in every P
    mask = torch.zeros(1, 1, 4, S, dtype=dm, device="cuda")
    mask[0, 0, 1] = torch.finfo(dm).min                              # a fully masked row: every element a tie
    mask[0, 0, 2] = float("-inf")                                    # a row of -inf: below the clamp
    y, dx, stats = fused(x, mask, g)
    assert (y[:, :, 1:3].float() == torch.tensor(1.0 / S).to(ds).float()).all()          # uniform
    assert abs(float(y[0, 0, 1].float().sum()) - 1) < 2e-2 and (stats[:, 1].reshape(2, 4)[:, 1:3] == S).all()
    assert (dx[:, :, 2] == 0).all()
    ye, dxe = R.eager32(x, mask, g)
    ref = R.ref64(x, mask, g)
    assert torch.equal(y[:, :, 1:3], ye[:, :, 1:3])
    assert R.c_dx(dx, ref) <= R.DX_CAP and R.c_dx(dxe, ref) <= R.DX_CAP
    d = (ref["g"] - (ref["g"] * ref["p"]).sum(-1, keepdim=True)) * ref["p"] * ref["inv"]
    half = (d / 2)[:, :, 1]
    assert (dx[:, :, 1].double() - half).abs().max() <= 2 * (2.0 ** -8 if ds != F else 1e-6) * half.abs().max()     # d / 2, not d and not 0
    assert dx[:, :, 1].abs().max() > 0


# ---- special values, determinism, canaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds,dm", [(BF, F), (F, F), (H, None)], ids=lambda d: str(d).replace("torch.", ""))
def test_nan_and_inf_rows_agree_with_the_chain_by_nan_position(ds, dm):
    x, mask, g = _shape_case(1, 1, 6, 264, ds, dm, 9)
    x[0, 0, 1, 5] = float("nan")
    x[0, 0, 3, 200] = float("inf")
    x[0, 0, 4, 7] = float("-inf")
    y, dx, _ = fused(x, mask, g)
    ye, dxe = R.eager32(x, mask, g)
    assert torch.equal(torch.isnan(y), torch.isnan(ye)) and torch.equal(torch.isnan(dx), torch.isnan(dxe))
    assert torch.isnan(y[0, 0, 1]).all() and torch.isnan(y[0, 0, 3]).all() and not torch.isnan(y[0, 0, [0, 2, 4, 5]]).any()


def test_two_runs_give_equal_bits_and_nothing_is_written_outside_the_results():
    _, ops = _mods()
    from llm_qat_amd import _lib
    B, Hh, T, S = 1, 2, 3, 2049
    x, mask, g = _shape_case(B, Hh, T, S, BF, F, 13)
    y1, dx1, st1 = fused(x, mask, g)
    y2, dx2, st2 = fused(x, mask, g)
    assert torch.equal(bits(y1), bits(y2)) and torch.equal(bits(dx1), bits(dx2)) and torch.equal(st1, st2)
    rows, pad = B * Hh * T, 64
    buf = {k: torch.full((n + 2 * pad,), 7.0, dtype=dt, device="cuda") for k, (n, dt) in dict(y=(rows * S, BF), st=(rows * 2, F), dx=(rows * S, BF)).items()}
    inner = {k: v[pad:-pad] for k, v in buf.items()}
    L, inv = _lib.lib(), ops.attn_inv(HD)
    tail = (rows, S, B, Hh, T, mask.stride(0), mask.stride(2), inv, 1, 0, None)
    assert L.fqs2_attn_softmax_fwd(x.data_ptr(), mask.data_ptr(), inner["y"].data_ptr(), inner["st"].data_ptr(), *tail) == 0
    assert L.fqs2_attn_softmax_bwd(g.data_ptr(), x.data_ptr(), mask.data_ptr(), inner["st"].data_ptr(), inner["dx"].data_ptr(), *tail) == 0
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert (v[:pad] == 7).all() and (v[-pad:] == 7).all(), k
    assert torch.equal(bits(inner["y"]), bits(y1).reshape(-1)) and torch.equal(bits(inner["dx"]), bits(dx1).reshape(-1))


# ---- memory -------------------------------------------------------------------------------------------------------------------------------------------
def test_saved_tensors_are_the_scores_the_mask_and_the_stats_and_nothing_under_no_grad():
    attention, ops = _mods()
    x, mask, g = _shape_case(1, 2, 8, 64, BF, F, 17)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = attention.attn_softmax(x.requires_grad_(True), mask, HD)
    assert len(saved) == 3 and saved[0].data_ptr() == x.data_ptr() and saved[2].data_ptr() == mask.data_ptr()
    assert saved[1].dtype == F and tuple(saved[1].shape) == (16, 2)
    saved.clear()
    before = dict(ops.attn_counts)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        with torch.no_grad():
            attention.attn_softmax(x, mask, HD)
        y2 = attention.attn_softmax(x.detach(), mask, HD)            # a frozen input
    assert saved == [] and not y2.requires_grad
    assert ops.attn_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.attn_counts["bwd_launch"] == before["bwd_launch"]
    y.backward(g)
    assert ops.attn_counts["bwd_launch"] == before["bwd_launch"] + 1


def test_the_forwards_peak_is_y_and_the_stats_and_the_chains_is_four_times_that():
    attention, _ = _mods()
    x, mask, _ = _shape_case(1, 2, 512, 512, BF, F, 19)
    x.requires_grad_(True)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out
        return p
    rows = 2 * 512
    want = x.numel() * 2 + 8 * rows
    got, eager = peak(lambda: attention.attn_softmax(x, mask, HD)), peak(lambda: R.chain(x, mask))
    print("forward peak over the inputs: fused", got, "bytes (y + stats:", want, "), eager chain", eager)
    assert want <= got <= want + 2 * 512                             # the allocator's granularity: 512 bytes a block
    assert eager >= 4 * got


# ---- counters and compile -----------------------------------------------------------------------------------------------------------------------------
def test_counters_per_call_and_a_transposed_scores_is_copied_once():
    attention, ops = _mods()
    x, mask, g = _shape_case(1, 2, 8, 8, BF, F, 23)
    c0 = dict(ops.attn_counts)
    y = attention.attn_softmax(x.requires_grad_(True), mask, HD)
    y.backward(g)
    c1 = dict(ops.attn_counts)
    assert (c1["fwd_launch"], c1["bwd_launch"], c1["copy_route"]) == (c0["fwd_launch"] + 1, c0["bwd_launch"] + 1, c0["copy_route"])
    xt = x.detach().transpose(2, 3).requires_grad_(True)
    yt = attention.attn_softmax(xt, mask.transpose(2, 3).contiguous(), HD)
    yt.backward(g)
    c2 = dict(ops.attn_counts)
    assert c2["copy_route"] == c1["copy_route"] + 1 and c2["fwd_launch"] == c1["fwd_launch"] + 1 and c2["bwd_launch"] == c1["bwd_launch"] + 1
    assert torch.equal(yt, attention.attn_softmax(xt.detach().contiguous(), mask.transpose(2, 3).contiguous(), HD))
    attention.attn_softmax(x, mask, HD).backward(g.transpose(2, 3).contiguous().transpose(2, 3))      # a gradient whose last stride is not 1: copied once, too
    assert ops.attn_counts["copy_route"] == c2["copy_route"] + 1 and ops.attn_counts["bwd_launch"] == c2["bwd_launch"] + 1


def test_torch_compile_fullgraph_equals_eager():
    attention, _ = _mods()
    x, mask, g = _shape_case(2, 2, 8, 72, BF, F, 29)

    def f(x, mask):
        return attention.attn_softmax(x * 1.0, mask, HD) * 2.0
    xe, xc = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ye = f(xe, mask)
    yc = torch.compile(f, backend="aot_eager", fullgraph=True)(xc, mask)
    ye.backward(g)
    yc.backward(g)
    assert torch.equal(bits(ye), bits(yc)) and torch.equal(bits(xe.grad), bits(xc.grad))


# ---- the tiny LLaMA -----------------------------------------------------------------------------------------------------------------------------------
def test_one_step_of_the_tiny_llama_through_install():
    """bf16 autocast, w4 a8 kv4, causal plus left-padding fp32 mask, through attention.install on a namespace whose LlamaAttention wears the
    reference's attribute names over the harness model's modules.  One forward and one backward launch per layer; loss and logits within
    the tolerance test_tiny_llama.py uses against the CPU fixture on the device (loss 5e-3, logits rtol 0.1 atol 0.02); every parameter
    gradient within 5 % of the eager step's in relative L2 distance, the same file's tolerance for values that cross a quantizer's bin
    edge: y differs from the chain's by one bf16 ulp (2^-8) on the few elements near a rounding boundary, an 8-bit activation bin is 2^-7
    of its row's range, so what follows the softmax moves by bins, not by more.  Measured on the MI355X: loss and logits equal the
    eager step's bits, the largest relative L2 distance of a parameter gradient is 1.0e-3."""
    import math

    import tiny_llama as TL
    from llm_qat_amd import utils_quant as UQ
    attention, ops = _mods()
    B, T = 2, 32
    neg = torch.finfo(F).min
    mask = torch.full((T, T), neg).triu(1).expand(B, 1, T, T).clone()
    mask[1, :, :, :3] = neg                                          # batch element 1 is left-padded: its rows 0..2 are fully masked
    mask = mask.cuda()
    pos = torch.arange(T, device="cuda").expand(B, T)
    ns = types.ModuleType("tiny_modeling")

    def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
        return q * cos + TL.rotate_half(q) * sin, k * cos + TL.rotate_half(k) * sin
    ns.apply_rotary_pos_emb = apply_rotary_pos_emb

    class Rotary(torch.nn.Module):
        def __init__(self, hd):
            super().__init__()
            self.hd = hd

        def forward(self, x, seq_len):
            return TL.rope_tables(self.hd, seq_len, x.device, x.dtype)

    class LlamaAttention(TL.Attention):
        """the harness attention under the reference's names, its forward the eager chain with the reference's signature"""

        def __init__(self, *a):
            super().__init__(*a)
            self.num_heads, self.head_dim, self.hidden_size = self.nh, self.hd, self.nh * self.hd
            self.act_quantizer_k = self.act_quantizer_v = self.kv_quant
            self.act_clip_val_k = self.act_clip_val_v = self.clip
            self.rotary_emb = Rotary(self.hd)
            self.register_forward_pre_hook(lambda m, a, kw: (a, dict(attention_mask=mask, position_ids=pos)), with_kwargs=True)
            self.register_forward_hook(lambda m, a, out: out[0])

        def forward(self, h, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False):
            b, t, d = h.shape
            q = self.q_proj(h).view(b, t, self.nh, self.hd).transpose(1, 2)
            k = self.kv_quant.apply(self.k_proj(h), self.clip, self.kv_bits, False).view(b, t, self.nh, self.hd).transpose(1, 2)
            v = self.kv_quant.apply(self.v_proj(h), self.clip, self.kv_bits, False).view(b, t, self.nh, self.hd).transpose(1, 2)
            cos, sin = self.rotary_emb(v, seq_len=t)
            q, k = ns.apply_rotary_pos_emb(q, k, cos, sin, position_ids)
            y = R.chain(torch.matmul(q, k.transpose(2, 3)), attention_mask, self.hd).to(q.dtype)
            return self.o_proj(torch.matmul(y, v).transpose(1, 2).reshape(b, t, d)), None, None
    ns.LlamaAttention = LlamaAttention

    def step(cls):
        old, TL.Attention = TL.Attention, cls
        try:
            model = TL.load_deterministic(TL.TinyLlama(UQ, w_bits=4, a_bits=8, kv_bits=4)).cuda()
        finally:
            TL.Attention = old
        ids = TL.deterministic_batch(B, T).cuda()
        with torch.autocast("cuda", dtype=BF):
            loss, logits = model(ids, labels=ids)
        loss.backward()
        return loss.detach(), logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    eager = step(LlamaAttention)
    assert attention.install(ns) is LlamaAttention
    before = dict(ops.attn_counts)
    got = step(ns.LlamaAttention)
    layers = TL.TINY["num_hidden_layers"]
    assert ops.attn_counts["fwd_launch"] == before["fwd_launch"] + layers and ops.attn_counts["bwd_launch"] == before["bwd_launch"] + layers
    print("loss", float(eager[0]), float(got[0]), "max logit distance", float((eager[1] - got[1]).abs().max()))
    assert abs(float(eager[0]) - float(got[0])) < 5e-3
    np.testing.assert_allclose(got[1].float().cpu().numpy(), eager[1].float().cpu().numpy(), rtol=0.1, atol=0.02)
    worst = 0.0
    for n in eager[2]:
        rel = float((eager[2][n].double() - got[2][n].double()).norm() / eager[2][n].double().norm().clamp_min(1e-30))
        worst = max(worst, rel)
        assert rel <= 0.05, (n, rel)
    print("largest relative L2 distance of a parameter gradient:", worst)
