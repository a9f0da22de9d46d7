"""CPU tier of the fused rotary embedding: the fqr_ header and its binding, every refusal of the entry points in the
order the header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers below are never dereferenced), the
formula model against the reference's own vectors (tests/golden/rope.npz) and against the chain, the layout rule of the results against
the chain's strides, the CPU-tensor route, install(), the compiled ops' fake implementations and the Python argument refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, compiled, ops, rope

import rope_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, K, QO, KO, COS, SIN, POS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000      # never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rope.npz"))


def fwd(ptrs, pbs, dims, qs, ks, dt, tdt):
    L = _lib.lib()
    rc = L.fqr_rope_fwd(*ptrs, pbs, *dims, *qs, *ks, *(dt if isinstance(dt, tuple) else (dt, dt)), tdt, None)
    return rc, L.fq_last_error().decode()


def bwd(ptrs, pbs, dims, gqs, gks, qs, ks, dt, tdt):
    L = _lib.lib()
    rc = L.fqr_rope_bwd(*ptrs, pbs, *dims, *gqs, *gks, *qs, *ks, *(dt if isinstance(dt, tuple) else (dt, dt)), tdt, None)
    return rc, L.fq_last_error().decode()


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_rope_header_names_equal_rope_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_rope.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqr_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.ROPE_EXPORTS) == {"fqr_rope_fwd", "fqr_rope_bwd", "fqr_rope_dense_strides"}
    assert not re.findall(r"\bfq[tsilcna]?_[a-z0-9_]+\s*\(", src)     # nothing of the eight other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    others = (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS) | set(_lib.INFER_EXPORTS) | set(_lib.LOSS_EXPORTS)
              | set(_lib.CE_EXPORTS) | set(_lib.NORM_EXPORTS) | set(_lib.ACT_EXPORTS))
    assert not set(_lib.ROPE_EXPORTS) & others
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.fqr_rope_fwd.argtypes == [vp] * 7 + [i64] * 13 + [i32, i32, i32, vp] and L.fqr_rope_fwd.restype is i32
    assert L.fqr_rope_bwd.argtypes == [vp] * 7 + [i64] * 19 + [i32, i32, i32, vp] and L.fqr_rope_bwd.restype is i32


def test_the_build_lists_the_new_unit_header_and_node():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_rope.hip", "fq_rope.h", "llmqat_fakequant_rope.h", "fq_rope_node.cpp"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

N7 = (None,) * 7
DIMS = (2, 8, 2, 5, 64, 16)                       # B, Hq, Hk, T, D, P
QS, KS = (5 * 8 * 64, 64, 8 * 64), (5 * 2 * 64, 64, 2 * 64)
BAD3 = (-1, -1, -1)
FP = (Q, K, QO, KO, COS, SIN, POS)
FWD_REFUSALS = [
    # (pointers, pos_batch_stride, dims, q strides, k strides, dtype or (q dtype, k dtype), table dtype), code, part of the message
    ((N7, 3, (0,) * 6, BAD3, BAD3, 9, F32), DTYPE, "unknown dtype"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, (BF16, 7), F32), DTYPE, "unknown dtype"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, (BF16, F64), F32), DTYPE, "float64"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, (BF16, F16), F32), DTYPE, "one of them is float32"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, (BF16, F32), BF16), DTYPE, "take float32 tables"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, (F32, F16), F16), DTYPE, "take float32 tables"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BF16, -1), DTYPE, "unknown dtype"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, F64, F32), DTYPE, "float64"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, F32, F64), DTYPE, "float64"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BF16, F16), DTYPE, "tensors' dtype or in float32"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, F32, BF16), DTYPE, "tensors' dtype or in float32"),
    ((N7, 3, (0, 8, 2, 5, 63, 0), BAD3, BAD3, BF16, F32), SHAPE, "non-positive shape"),
    ((N7, 3, (2, 8, -2, 5, 63, 0), BAD3, BAD3, BF16, BF16), SHAPE, "non-positive shape"),
    ((N7, 3, (2, 8, 2, 5, 0, 0), BAD3, BAD3, F16, F16), SHAPE, "non-positive shape"),
    ((N7, 3, (2, 8, 2, 5, 63, 0), BAD3, BAD3, F32, F32), SHAPE, "odd head size"),
    ((N7, 3, (2, 8, 2, 5, 64, 0), BAD3, BAD3, BF16, F32), SHAPE, "non-positive table rows"),
    ((N7, 3, (2, 8, 2, 5, 64, -16), BAD3, BAD3, BF16, F32), SHAPE, "non-positive table rows"),
    ((N7, 3, (2, 8, 2, 5, 64, 2 ** 58), BAD3, BAD3, BF16, F32), SHAPE, "P * D overflows"),
    ((N7, 3, DIMS, BAD3, BAD3, BF16, F32), SHAPE, "neither 0 nor T"),
    ((N7, 5, DIMS, (QS[0], -64, QS[2]), KS, BF16, F32), SHAPE, "negative stride"),
    ((N7, 0, DIMS, QS, (KS[0], KS[1], -1), BF16, F32), SHAPE, "negative stride"),
    ((N7, 0, (2 ** 20, 2 ** 20, 2, 2 ** 20, 64, 16), QS, KS, BF16, F32), SHAPE, "element count of q overflows"),
    ((N7, 0, DIMS, (2 ** 61, 64, 512), KS, BF16, F32), SHAPE, "extent of q overflows"),
    ((N7, 0, DIMS, QS, (640, 2 ** 61, 128), BF16, F32), SHAPE, "extent of k overflows"),
    ((N7, 5, DIMS, QS, KS, BF16, F32), NULL, "NULL"),
    (((None, K, QO, KO, COS, SIN, POS), 5, DIMS, QS, KS, BF16, F32), NULL, "NULL"),
    (((Q, K, QO, None, COS, SIN, None), 0, DIMS, QS, KS, BF16, F32), NULL, "NULL"),
    (((Q, K, QO, KO, None, SIN, None), 0, DIMS, QS, KS, F32, F32), NULL, "NULL"),
    (((Q, K, Q, None, COS, SIN, None), 0, (2 ** 20, 8, 2, 2 ** 20, 64, 16), (0, 0, 0), (0, 0, 0), BF16, F32), NULL, "NULL"),     # the pointers come before the aliasing and the grid
    (((Q, K, Q, KO, COS, SIN, POS), 5, DIMS, QS, KS, BF16, F32), ARG, "in-place"),
    (((Q, K, QO, K, COS, SIN, POS), 5, DIMS, QS, KS, BF16, F32), ARG, "in-place"),
    (((Q, K, K, KO, COS, SIN, POS), 5, DIMS, QS, KS, BF16, F32), ARG, "in-place"),
    (((Q, K, QO, SIN, COS, SIN, POS), 5, DIMS, QS, KS, BF16, BF16), ARG, "in-place"),
    (((Q, K, QO, QO, COS, SIN, POS), 5, DIMS, QS, KS, BF16, F32), ARG, "same buffer"),
    (((Q, K, QO, QO, COS, SIN, None), 0, (2 ** 20, 8, 2, 2 ** 20, 64, 16), (0, 0, 0), (0, 0, 0), BF16, F32), ARG, "same buffer"),   # the aliasing comes before the grid
    (((Q, K, QO, KO, COS, SIN, None), 0, (2 ** 20, 8, 2, 2 ** 20, 64, 16), (0, 0, 0), (0, 0, 0), BF16, F32), UNSUPPORTED, "exceed one launch's grid"),
    (((Q, K, QO, KO, COS, SIN, None), 0, (1, 2 ** 25, 2, 1, 64, 16), (0, 0, 0), (0, 0, 0), BF16, F32), UNSUPPORTED, "exceeds 2^30"),
]
BP = (Q, K, QO, KO, COS, SIN, POS)                # dq_out, dk_out, dq, dk, cos, sin, positions
BWD_REFUSALS = [
    # (pointers, pos_batch_stride, dims, gq strides, gk strides, q strides, k strides, dtype, table dtype), code, part of the message
    ((N7, 3, (0,) * 6, BAD3, BAD3, BAD3, BAD3, 9, F32), DTYPE, "unknown dtype"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BAD3, BAD3, F64, F32), DTYPE, "float64"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BAD3, BAD3, F16, BF16), DTYPE, "tensors' dtype or in float32"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BAD3, BAD3, (F16, BF16), F32), DTYPE, "one of them is float32"),
    ((N7, 3, (0,) * 6, BAD3, BAD3, BAD3, BAD3, (F32, BF16), BF16), DTYPE, "take float32 tables"),
    ((N7, 3, (2, 0, 2, 5, 63, 0), BAD3, BAD3, BAD3, BAD3, BF16, F32), SHAPE, "non-positive shape"),
    ((N7, 3, (2, 8, 2, 5, 63, 0), BAD3, BAD3, BAD3, BAD3, BF16, F32), SHAPE, "odd head size"),
    ((N7, 3, (2, 8, 2, 5, 64, 0), BAD3, BAD3, BAD3, BAD3, BF16, F32), SHAPE, "non-positive table rows"),
    ((N7, 3, DIMS, BAD3, BAD3, BAD3, BAD3, BF16, F32), SHAPE, "neither 0 nor T"),
    ((N7, 5, DIMS, QS, (640, -64, 128), QS, KS, BF16, F32), SHAPE, "negative stride -64 of dk_out"),
    ((N7, 5, DIMS, QS, KS, QS, (-640, 64, 128), BF16, F32), SHAPE, "negative stride -640 of k"),
    ((N7, 5, DIMS, (2 ** 61, 64, 512), KS, QS, KS, BF16, F32), SHAPE, "extent of dq_out overflows"),
    ((N7, 5, DIMS, QS, KS, QS, KS, BF16, F32), NULL, "cos / sin"),
    (((Q, K, QO, KO, COS, None, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), NULL, "cos / sin"),
    (((Q, K, None, None, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), NULL, "both"),
    (((None, K, QO, KO, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), NULL, "incoming gradient"),
    (((Q, None, None, KO, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), NULL, "incoming gradient"),
    (((Q, K, Q, KO, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), ARG, "in-place"),
    (((Q, K, QO, K, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), ARG, "in-place"),
    (((Q, K, QO, COS, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, F32, F32), ARG, "in-place"),
    (((Q, K, QO, QO, COS, SIN, POS), 5, DIMS, QS, KS, QS, KS, BF16, F32), ARG, "same buffer"),
    (((Q, K, QO, QO, COS, SIN, None), 0, (2 ** 20, 8, 2, 2 ** 20, 64, 16), (0,) * 3, (0,) * 3, (0,) * 3, (0,) * 3, BF16, F32), ARG, "same buffer"),
    (((Q, K, QO, KO, COS, SIN, None), 0, (2 ** 20, 8, 2, 2 ** 20, 64, 16), (0,) * 3, (0,) * 3, (0,) * 3, (0,) * 3, BF16, F32), UNSUPPORTED, "exceed one launch's grid"),
    (((None, K, None, KO, COS, SIN, None), 0, (1, 2 ** 25, 2, 1, 64, 16), (0,) * 3, (0,) * 3, (0,) * 3, (0,) * 3, F16, F16), UNSUPPORTED, "exceeds 2^30"),
]


@pytest.mark.parametrize("args, code, text", FWD_REFUSALS)
def test_every_forward_refusal_comes_back_with_its_code_in_the_stated_order(args, code, text):
    rc, msg = fwd(*args)
    assert rc == code, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("args, code, text", BWD_REFUSALS)
def test_every_backward_refusal_comes_back_with_its_code_in_the_stated_order(args, code, text):
    rc, msg = bwd(*args)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_every_served_dtype_pair_passes_the_first_checks():
    for dt, tdt in ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), ((BF16, F32), F32), ((F32, F16), F32)):
        assert fwd(N7, 5, DIMS, QS, KS, dt, tdt)[0] == NULL and bwd(N7, 0, DIMS, QS, KS, QS, KS, dt, tdt)[0] == NULL


def test_a_frozen_side_may_leave_its_incoming_gradient_out():
    """dq NULL: dq_out may be NULL too; the call then stops at nothing before the launch, which this tier does not make -- so the
    last refusal it can show is the grid's"""
    big = (2 ** 20, 8, 2, 2 ** 20, 64, 16)
    z = (0,) * 3
    assert bwd((None, K, None, KO, COS, SIN, None), 0, big, z, z, z, z, BF16, F32)[0] == UNSUPPORTED
    assert bwd((Q, None, QO, None, COS, SIN, None), 0, big, z, z, z, z, BF16, F32)[0] == UNSUPPORTED


# ---- the layout of the results ---------------------------------------------------------------------------------------------------------------

def layouts(B, H, T, D, dtype=torch.float32):
    return {
        "transposed": torch.randn(B, T, H * D).to(dtype).view(B, T, H, D).transpose(1, 2),
        "contiguous": torch.randn(B, H, T, D).to(dtype),
        "qkv_chunk": torch.randn(B, T, 3 * H * D).to(dtype).chunk(3, -1)[1].view(B, T, H, D).transpose(1, 2),
        "offset_base": torch.randn(B * T * H * D + 1).to(dtype)[1:].view(B, T, H, D).transpose(1, 2),
        "odd_token_stride": torch.randn(B, H, T, D + 1).to(dtype)[..., :D],
        "expanded_heads": torch.randn(B, 1, T, D).to(dtype).expand(B, H, T, D),
    }


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 3, 5, 6), (1, 3, 33, 16), (2, 1, 5, 64), (1, 32, 1, 128), (2, 8, 33, 64)])
def test_the_dense_rule_gives_the_chains_own_strides(shape):
    B, H, T, D = shape
    cos, sin = R.tables(64, D)
    for name, q in layouts(B, H, T, D).items():
        for pos in (None, torch.arange(T).unsqueeze(0), torch.arange(T).unsqueeze(0).expand(B, T).contiguous()):
            qe, _ = R.chain(q, q, cos, sin, pos)
            assert ops.rope_dense_like(q.shape, q.stride()) == tuple(qe.stride()), (name, q.stride(), qe.stride())


def test_the_reference_layout_keeps_its_strides():
    q = torch.randn(2, 33, 32 * 128).view(2, 33, 32, 128).transpose(1, 2)
    assert ops.rope_dense_like(q.shape, q.stride()) == tuple(q.stride())


# ---- the formula model, the golden vectors and the chain ----------------------------------------------------------------------------------------

def gold(key, dtype):
    a = GOLD[key]
    return torch.from_numpy(a.view(np.int16)).view(dtype) if a.dtype == np.uint16 else torch.from_numpy(a)


def gold_cases():
    for name in GOLD["dtypes"]:
        for case in [f"s{i}" for i in range(len(GOLD["shapes"]))] + ["special"]:
            yield str(name), case


@pytest.mark.parametrize("name, case", list(gold_cases()))
def test_the_formula_model_equals_the_references_own_bits(name, case):
    dt = R.DTYPES[name]
    g = {k: gold(f"{name}_{case}_{k}", dt) for k in ("q", "k", "gq", "gk", "qe", "ke", "dq", "dk")}
    pos = torch.from_numpy(GOLD[f"{name}_{case}_pos"])
    D = g["q"].shape[-1]
    cos, sin = torch.from_numpy(GOLD[f"cos_d{D}"]), torch.from_numpy(GOLD[f"sin_d{D}"])
    assert cos.dtype == torch.float32 and cos.shape == (int(GOLD["P"]), D)
    assert torch.equal(R.bits(R.model_fwd(g["q"], cos, sin, pos)), R.bits(g["qe"]))
    assert torch.equal(R.bits(R.model_fwd(g["k"], cos, sin, pos)), R.bits(g["ke"]))
    assert torch.equal(R.bits(R.model_bwd(g["gq"], cos, sin, pos)), R.bits(g["dq"]))
    assert torch.equal(R.bits(R.model_bwd(g["gk"], cos, sin, pos)), R.bits(g["dk"]))
    qe, ke, dq, dk = R.chain_grads(g["q"], g["k"], cos, sin, pos, g["gq"], g["gk"])           # this project's wording of the chain: the same bits
    for got, want in ((qe, g["qe"]), (ke, g["ke"]), (dq, g["dq"]), (dk, g["dk"])):
        assert torch.equal(R.bits(got), R.bits(want))


def test_the_special_case_holds_zeros_of_either_sign_and_the_gradient_of_a_zero_row_is_plus_zero():
    for name, dt in R.DTYPES.items():
        gq, dq, dk = gold(f"{name}_special_gq", dt), gold(f"{name}_special_dq", dt), gold(f"{name}_special_dk", dt)
        assert not gq[0, 0, 0].signbit().any() and gq[0, 1, 1].signbit().all() and (gq[0, :2, :2] == 0).any()
        for row in (dq[0, 0, 0], dq[0, 1, 1], dk[0, 0, 0]):
            assert (row == 0).all() and not row.signbit().any()


def test_a_single_rounding_rope_is_another_function():
    """fp32 tables and one rounding (the 'better' RoPE) differ from the chain in a large share of the outputs: the model must not be that"""
    gen = torch.Generator().manual_seed(3)
    cos, sin = R.tables(64, 64)
    for dt, least in ((torch.bfloat16, 0.15), (torch.float16, 0.15)):
        q = torch.randn(2, 4, 33, 64, generator=gen).to(dt)
        want = R.model_fwd(q, cos, sin)
        once = (q.float() * cos[:33] + R.rotate_half(q.float()) * sin[:33]).to(dt)
        assert (R.bits(once).view(torch.int16) != R.bits(want).view(torch.int16)).float().mean() > least


@pytest.mark.parametrize("name", list(R.DTYPES))
def test_the_model_equals_the_chain_with_unequal_halves_table_dtypes_and_every_position_form(name):
    dt = R.DTYPES[name]
    gen = torch.Generator().manual_seed(11)
    B, Hq, Hk, T, D, P = 2, 3, 2, 7, 16, 24
    q, k = R.transposed(B, Hq, T, D, dt, "cpu", gen), R.transposed(B, Hk, T, D, dt, "cpu", gen)
    gq, gk = R.transposed(B, Hq, T, D, dt, "cpu", gen), R.transposed(B, Hk, T, D, dt, "cpu", gen)
    cos, sin = R.tables(P, D, equal_halves=False)
    assert not torch.equal(cos[:, : D // 2], cos[:, D // 2:])
    for tables in ((cos, sin), (cos.to(dt), sin.to(dt)), (cos.view(1, 1, P, D), sin.view(1, 1, P, D))):
        for pos in (None, torch.randint(0, P, (B, T), generator=gen), torch.randint(0, P, (1, T), generator=gen), torch.randint(-P, 0, (B, T), generator=gen)):
            qe, ke, dq, dk = R.chain_grads(q, k, *tables, pos, gq, gk)
            assert torch.equal(R.bits(R.model_fwd(q, *tables, pos)), R.bits(qe)) and torch.equal(R.bits(R.model_fwd(k, *tables, pos)), R.bits(ke))
            assert torch.equal(R.bits(R.model_bwd(gq, *tables, pos)), R.bits(dq)) and torch.equal(R.bits(R.model_bwd(gk, *tables, pos)), R.bits(dk))


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_two_dtypes_the_chain_promotes_and_the_cpu_route_follows_it(name):
    """q 16-bit beside an fp32 k and fp32 tables (the reference under autocast behind its fp32 K quantizer), and the other way round: both
    results fp32 = the fp32 formulas on the exact values; the 16-bit side's gradient = the backward formulas with that dtype's roundings on
    fp32 gradients and unrounded tables"""
    dt = R.DTYPES[name]
    gen = torch.Generator().manual_seed(13)
    B, Hq, Hk, T, D, P = 2, 3, 2, 7, 16, 24
    cos, sin = R.tables(P, D, equal_halves=False)
    pos = torch.randint(0, P, (B, T), generator=gen)
    gq, gk = R.transposed(B, Hq, T, D, torch.float32, "cpu", gen), R.transposed(B, Hk, T, D, torch.float32, "cpu", gen)
    gq[0, 0, 0], gq[0, 1, 1] = 0.0, -0.0
    was = llm_qat_amd.cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(True)
        for qdt, kdt in ((dt, torch.float32), (torch.float32, dt)):
            q, k = R.transposed(B, Hq, T, D, qdt, "cpu", gen), R.transposed(B, Hk, T, D, kdt, "cpu", gen)
            qe, ke, dq, dk = R.chain_grads(q, k, cos, sin, pos, gq, gk)
            assert qe.dtype is ke.dtype is torch.float32 and dq.dtype is qdt and dk.dtype is kdt
            assert torch.equal(R.bits(R.model_fwd(q.float(), cos, sin, pos)), R.bits(qe)) and torch.equal(R.bits(R.model_fwd(k.float(), cos, sin, pos)), R.bits(ke))
            for g, d, ddt in ((gq, dq, qdt), (gk, dk, kdt)):
                assert torch.equal(R.bits(R.model_bwd(g, cos, sin, pos, ddt)), R.bits(d)), (qdt, kdt, ddt)
            qr, kr = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
            got = rope.rotary(qr, kr, cos, sin, pos)
            grads = torch.autograd.grad(got, (qr, kr), (gq, gk))
            for a, b in zip((*got, *grads), (qe, ke, dq, dk)):
                assert a.dtype is b.dtype and torch.equal(R.bits(a), R.bits(b))
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


def test_the_model_gives_nan_for_a_position_outside_the_table_and_leaves_the_other_tokens():
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(1, 2, 4, 8, generator=gen)
    cos, sin = R.tables(6, 8)
    pos = torch.tensor([[0, 7, -7, 5]])
    y = R.model_fwd(q, cos, sin, pos)
    assert y[:, :, 1:3].isnan().all() and not y[:, :, (0, 3)].isnan().any()
    assert torch.equal(y[:, :, (0, 3)], R.model_fwd(q[:, :, (0, 3)], cos, sin, torch.tensor([[0, 5]])))


# ---- the CPU-tensor route -------------------------------------------------------------------------------------------------------------------

def test_cpu_tensors_are_refused_by_default_and_served_bit_for_bit_after_the_opt_in():
    was = llm_qat_amd.cpu_tensors.ENABLED
    dt = torch.bfloat16
    q, k, pos = gold("bf16_s0_q", dt), gold("bf16_s0_k", dt), torch.from_numpy(GOLD["bf16_s0_pos"])
    cos, sin = torch.from_numpy(GOLD["cos_d8"]), torch.from_numpy(GOLD["sin_d8"])
    try:
        llm_qat_amd.allow_cpu_tensors(False)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rope.rotary(q, k, cos, sin, pos)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rope.apply_rotary_pos_emb(q, k, cos.view(1, 1, 16, 8), sin.view(1, 1, 16, 8), pos)
        with pytest.raises(RuntimeError, match="MI355X"):
            ops.rope_forward(q, k, cos, sin, pos)
        llm_qat_amd.allow_cpu_tensors(True)
        for name, dtype in R.DTYPES.items():
            q, k = (gold(f"{name}_s0_{t}", dtype).requires_grad_(True) for t in "qk")
            pos = torch.from_numpy(GOLD[f"{name}_s0_pos"])
            qe, ke = rope.apply_rotary_pos_emb(q, k, cos.view(1, 1, 16, 8), sin.view(1, 1, 16, 8), pos)
            dq, dk = torch.autograd.grad((qe, ke), (q, k), (gold(f"{name}_s0_gq", dtype), gold(f"{name}_s0_gk", dtype)))
            for got, key in ((qe, "qe"), (ke, "ke"), (dq, "dq"), (dk, "dk")):
                assert torch.equal(R.bits(got), R.bits(gold(f"{name}_s0_{key}", dtype))), (name, key)
        qe, _ = rope.rotary(q.detach()[:, :, :5], k.detach()[:, :, :5], cos, sin)                 # no positions: the token index
        assert torch.equal(R.bits(qe), R.bits(R.chain(q.detach()[:, :, :5], k.detach()[:, :, :5], cos, sin, None)[0]))
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


# ---- install() ---------------------------------------------------------------------------------------------------------------------------------

def test_install_replaces_the_modules_function_returns_the_old_one_and_is_undone_by_assignment():
    ns = types.ModuleType("stand_in_modeling")

    def chain_style(q, k, cos, sin, position_ids):
        return R.chain(q, k, cos, sin, position_ids)
    ns.apply_rotary_pos_emb = chain_style
    ns.caller = lambda *a: ns.apply_rotary_pos_emb(*a)       # looks the function up at call time, as LlamaAttention.forward does
    previous = rope.install(ns)
    assert previous is chain_style and ns.apply_rotary_pos_emb is rope.apply_rotary_pos_emb
    was = llm_qat_amd.cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(True)
        q, k = torch.randn(1, 2, 3, 4), torch.randn(1, 1, 3, 4)
        cos, sin = R.tables(8, 4)
        pos = torch.tensor([[2, 0, 7]])
        got, want = ns.caller(q, k, cos, sin, pos), chain_style(q, k, cos, sin, pos)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        llm_qat_amd.allow_cpu_tensors(was)
    ns.apply_rotary_pos_emb = previous
    assert ns.apply_rotary_pos_emb is chain_style
    with pytest.raises(TypeError, match="module object"):
        rope.install(types.SimpleNamespace(apply_rotary_pos_emb=chain_style))
    with pytest.raises(AttributeError):
        rope.install(types.ModuleType("empty"))


def test_the_public_names_live_in_the_submodule():
    assert llm_qat_amd.rope is rope and set(rope.__all__) == {"apply_rotary_pos_emb", "rotary", "install"}
    assert not hasattr(llm_qat_amd, "rotary")
    assert set(ops.rope_counts.keys()) == {"fwd_launch", "bwd_launch", "copy_route"}


# ---- the compiled ops' fake implementations --------------------------------------------------------------------------------------------------

def test_fake_ops_shapes_dtypes_and_strides_on_meta_tensors():
    for dtype in R.DTYPES.values():
        q = torch.empty(2, 5, 8 * 64, dtype=dtype, device="meta").view(2, 5, 8, 64).transpose(1, 2)
        k = torch.empty(2, 2, 5, 64, dtype=dtype, device="meta")
        cos, sin = torch.empty(16, 64, device="meta"), torch.empty(16, 64, device="meta")
        pos = torch.empty(1, 5, dtype=torch.int64, device="meta")
        for p in (pos, None):
            qe, ke = torch.ops.llmqat_amd.rope_fwd(q, k, cos, sin, p)
            assert qe.device.type == "meta" and qe.shape == q.shape and qe.dtype is dtype and qe.stride() == q.stride()
            assert ke.shape == k.shape and ke.is_contiguous()
        dq, dk = torch.ops.llmqat_amd.rope_bwd(qe, ke, cos, sin, pos, list(q.shape), list(q.stride()), dtype, list(k.shape), list(k.stride()), dtype, True, False)
        assert dq.shape == q.shape and dq.stride() == q.stride() and dq.dtype is dtype and dk.numel() == 0
        if dtype is not torch.float32:                       # q 16-bit beside an fp32 k: fp32 results, gradients in their tensor's dtype
            qe, ke = torch.ops.llmqat_amd.rope_fwd(q, k.float(), cos, sin, pos)
            assert qe.dtype is ke.dtype is torch.float32 and qe.stride() == q.stride()
            dq, dk = torch.ops.llmqat_amd.rope_bwd(qe, ke, cos, sin, pos, list(q.shape), list(q.stride()), dtype, list(k.shape), list(k.stride()), torch.float32, True, True)
            assert dq.dtype is dtype and dk.dtype is torch.float32
    with pytest.raises(ValueError, match="odd head size"):
        torch.ops.llmqat_amd.rope_fwd(torch.empty(1, 1, 2, 3, device="meta"), torch.empty(1, 1, 2, 3, device="meta"), torch.empty(4, 3, device="meta"),
                                      torch.empty(4, 3, device="meta"), None)
    assert compiled.rope_fwd_op is not None and compiled.rope_bwd_op is not None


# ---- the Python argument refusals ----------------------------------------------------------------------------------------------------------------

def test_python_argument_refusals():
    q, k = torch.randn(2, 3, 5, 8), torch.randn(2, 1, 5, 8)
    cos, sin = R.tables(16, 8)
    pos = torch.zeros(2, 5, dtype=torch.int64)
    for f in (rope.rotary, ops.rope_forward, ops.check_rope):
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(q, None, cos, sin, pos)
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(q, k, cos, 1.0, pos)
        with pytest.raises(TypeError, match="not served"):
            f(q.double(), k.double(), cos, sin, pos)
        with pytest.raises(TypeError, match="not served"):
            f(q.long(), k.long(), cos, sin, pos)
        with pytest.raises(TypeError, match="one of them is float32"):
            f(q.half(), k.bfloat16(), cos, sin, pos)
        with pytest.raises(TypeError, match="float32"):
            f(q.bfloat16(), k, cos.bfloat16(), sin.bfloat16(), pos)          # two dtypes: the tables are float32
        with pytest.raises(TypeError, match="float32"):
            f(q, k, cos.bfloat16(), sin.bfloat16(), pos)                     # fp32 tensors with 16-bit tables
        with pytest.raises(TypeError, match="float32"):
            f(q.bfloat16(), k.bfloat16(), cos.half(), sin.half(), pos)
        with pytest.raises(TypeError, match="float32"):
            f(q.bfloat16(), k.bfloat16(), cos, sin.bfloat16(), pos)          # one dtype for both tables
        with pytest.raises(TypeError, match="int64"):
            f(q, k, cos, sin, pos.int())
        with pytest.raises(ValueError, match=r"\[B, H, T, D\]"):
            f(q[0], k[0], cos, sin, pos)
        with pytest.raises(ValueError, match="differ in batch, tokens or head size"):
            f(q, k[:, :, :4], cos, sin, pos)
        with pytest.raises(ValueError, match="empty"):
            f(q[:0], k[:0], cos, sin, pos[:0])
        with pytest.raises(ValueError, match="odd head size"):
            f(q[..., :7], k[..., :7], cos[:, :7], sin[:, :7], pos)
        with pytest.raises(ValueError, match="tables are"):
            f(q, k, cos[:, :6], sin[:, :6], pos)
        with pytest.raises(ValueError, match="tables are"):
            f(q, k, cos.view(1, 16, 8), sin.view(1, 16, 8), pos)
        with pytest.raises(ValueError, match="tables are"):
            f(q, k, cos, sin[:8], pos)
        with pytest.raises(ValueError, match="position_ids are"):
            f(q, k, cos, sin, pos[:, :4])
        with pytest.raises(ValueError, match="position_ids are"):
            f(q, k, cos, sin, pos[0])
        with pytest.raises(ValueError, match="on meta"):
            f(q, k, cos.to("meta"), sin.to("meta"), pos)
        with pytest.raises(ValueError, match="k on meta"):
            f(q, k.to("meta"), cos, sin, pos)
    with pytest.raises(ValueError, match="neither dq nor dk"):
        ops.rope_backward(q, k, cos, sin, pos, q, k, False, False)
    with pytest.raises(ValueError, match="gradient of a result"):
        ops.rope_backward(q[:, :2], k, cos, sin, pos, q, k)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.rope_backward(q, k, cos, sin, pos, q, k)
    assert ops.check_rope(q, k, cos.view(1, 1, 16, 8), sin.view(1, 1, 16, 8), pos[:1]) == (2, 3, 1, 5, 8, 16)


def test_the_front_ends_layout_helpers_copy_only_what_the_kernels_cannot_read():
    before = dict(ops.rope_counts)
    q = torch.randn(2, 5, 3 * 8).view(2, 5, 3, 8).transpose(1, 2)
    cos, _ = R.tables(16, 8)
    assert ops._rope_served(q) is q and ops._rope_table(cos, 8) is cos
    assert ops._rope_table(cos.view(1, 1, 16, 8), 8).data_ptr() == cos.data_ptr()
    big = torch.randn(32, 8)
    assert ops._rope_table(big[:16], 8).data_ptr() == big.data_ptr()          # a slice of a larger table is read where it lies
    pos = torch.zeros(2, 5, dtype=torch.int64)
    assert ops._rope_positions(pos, 2) == (pos, 5) and ops._rope_positions(pos[:1], 2)[1] == 0 and ops._rope_positions(None, 2) == (None, 0)
    assert dict(ops.rope_counts) == before
    t = torch.randn(2, 3, 8, 5).transpose(2, 3)                              # a last stride of 5: the one copy
    c = ops._rope_served(t)
    assert c.is_contiguous() and torch.equal(c, t)
    assert ops._rope_table(torch.randn(16, 16)[:, ::2], 8).is_contiguous()
    assert ops.rope_counts["copy_route"] == before["copy_route"] + 2
