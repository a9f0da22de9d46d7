"""CPU tier: a DIFFERENTIAL run of the oracle against what the REAL reference code computed on inputs no other fixture holds.

The reference's own `SymQuantizer` / `AsymQuantizer` (models/utils_quant.py:31-162) were executed on freshly drawn tensors
(3 dtypes, bits 2..16, 1-D .. 4-D, layerwise, rows scaled from 1e-30 to 1e30 for fp32 / bf16 and across fp16's range, signed zeros,
NaN / Inf, all-zero rows, rows at and around the STE clip) and their results recorded in tests/golden/live_reference.json by
tests/golden/make_golden_live_reference.py: a digest of every input, forward value and STE gradient (bits, any NaN equal to any NaN).
The tests below draw the same inputs from the same seeds, check them against the recorded digests, and require the oracle
(oracle/fq_oracle.c) to reproduce the reference's results bit for bit.  And the autocast arithmetic: the real `SymQuantizer.apply`
under CUDA autocast's cast policy (tests/autocast_policy.py, both scalar policies) against `fqo_sym_fwd_autocast` / `fqo_ste_bwd_wide`.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, nan_mask
from oracle import oracle as O

sys.path.insert(0, os.path.join(ROOT, "tests"))

RECORD = os.path.join(GOLDEN, "live_reference.json")
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def rec():
    """the reference's recorded results (tests/golden/make_golden_live_reference.py)"""
    with open(RECORD) as f:
        return json.load(f)


def digest(a, dtype):
    """digest of raw storage (uint16 bits / float32) that two arrays share iff they are bit-equal with any NaN equal to any NaN
    (conftest.bits_equal)"""
    a = np.ascontiguousarray(a)
    na = nan_mask(a, dtype)
    v = a.view(np.uint32) if a.dtype == np.float32 else a
    h = hashlib.sha256(f"{dtype}{a.shape}".encode())
    h.update(na.tobytes())
    h.update(np.where(na, 0, v).astype(v.dtype).tobytes())
    return h.hexdigest()[:32]


def to_np(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16).copy() if t.dtype in (torch.bfloat16, torch.float16) else t.numpy().copy()


def draw(rng, dtype, trial):
    """a tensor with adversarial rows; -> torch tensor of `dtype` (CPU)"""
    nd = int(rng.integers(1, 5))
    shape = tuple(int(rng.integers(1, 7)) for _ in range(nd - 1)) + (int(rng.choice([1, 2, 5, 8, 17, 64, 100, 257])),)
    scales = {"fp32": [1e-30, 1e-12, 1e-6, 1e-4, 0.02, 1.0, 2.0, 40.0, 1e6, 1e30], "bf16": [1e-30, 1e-12, 1e-6, 1e-4, 3e-4, 0.02, 1.0, 2.0, 40.0, 1e6, 1e30],
              "fp16": [1e-7, 1e-5, 1.2e-4, 2.4e-4, 1e-3, 0.02, 1.0, 2.0, 40.0, 3e3, 3e4]}[dtype]
    rows = int(np.prod(shape[:-1])) if nd > 1 else 1
    with np.errstate(over="ignore", invalid="ignore"):
        x = rng.standard_normal(shape).astype(np.float32) * rng.choice(scales, size=shape[:-1] + (1,)).astype(np.float32)
        flat = x.reshape(rows, shape[-1])
        for _ in range(int(rng.integers(0, 4))):
            r, c = int(rng.integers(0, rows)), int(rng.integers(0, shape[-1]))
            flat[r, c] = np.float32(rng.choice([0.0, -0.0, 2.0, -2.0, 1.9921875, -2.015625, np.nan, np.inf, -np.inf, 6e4, 1e-40]))
        if rng.random() < 0.2:
            flat[int(rng.integers(0, rows))] = 0.0
    return torch.from_numpy(x).to(TD[dtype])


FRESH_TRIALS, AUTOCAST_TRIALS, LOWBIT_TRIALS = 150, 75, 50


def fresh_cases(dtype, n=FRESH_TRIALS):
    """-> (trial, x, kind, bits, layerwise, lo, hi, g) as the reference saw them"""
    rng = np.random.default_rng({"bf16": 101, "fp16": 102, "fp32": 103}[dtype])
    for trial in range(n):
        x = draw(rng, dtype, trial)
        kind = "sym" if trial % 3 else "asym"
        bits = int(rng.choice([1, 2, 3, 4, 6, 8, 12, 16, 31])) if kind == "sym" else int(rng.choice([1, 2, 4, 8, 16, 24]))
        layerwise = bool(rng.random() < 0.2) and x.dim() <= 3
        lo, hi = [(-2.0, 2.0), (-0.5, 0.75), (-1.0, 1.0)][int(rng.integers(0, 3))]
        g = (torch.randn(x.shape, generator=torch.Generator().manual_seed(trial)) * 0.1).to(TD[dtype])
        yield trial, x, kind, bits, layerwise, lo, hi, g


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_oracle_equals_the_live_reference_on_fresh_inputs(rec, dtype):
    want_all = rec["fresh"][dtype]
    assert len(want_all) == FRESH_TRIALS
    for (trial, x, kind, bits, layerwise, lo, hi, g), want in zip(fresh_cases(dtype), want_all):
        r, c = O.rows_cols(tuple(x.shape), layerwise)
        x_np = to_np(x)
        tag = f"trial {trial}: {kind} {dtype} {tuple(x.shape)} b{bits} lw={layerwise} clip=({lo},{hi})"
        assert (digest(x_np, dtype), digest(to_np(g), dtype)) == (want["x"], want["g"]), f"{tag}: not the inputs the reference saw"
        y = (O.sym_fwd(x_np, r, c, bits, dtype)[0] if kind == "sym" else O.asym_fwd(x_np, r, c, bits, dtype)[0])
        assert digest(y.reshape(x_np.shape), dtype) == want["y"], f"{tag} forward differs from the reference's"
        gx = O.ste_bwd(to_np(g), x_np, lo, hi, dtype)
        assert digest(gx.reshape(x_np.shape), dtype) == want["gx"], f"{tag} gradient differs from the reference's"


def autocast_cases(dtype, device_scalars, n=AUTOCAST_TRIALS):
    """-> (trial, x, bits, lo, hi, g) as the reference saw them"""
    rng = np.random.default_rng({"bf16": 201, "fp16": 202}[dtype] + (10 if device_scalars else 0))
    for trial in range(n):
        x = draw(rng, dtype, trial)
        if x.dim() > 3 and trial % 2:
            x = x.reshape(-1, x.shape[-1])
        bits = int(rng.choice([1, 2, 3, 4, 8, 12, 16, 31]))
        lo, hi = [(-2.0, 2.0), (-0.5, 0.75)][trial % 2]
        g = torch.randn(x.shape, generator=torch.Generator().manual_seed(trial)) * 0.1
        yield trial, x, bits, lo, hi, g


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("device_scalars", [False, True])
def test_oracle_equals_the_live_reference_under_the_autocast_policy(rec, dtype, device_scalars):
    """SymQuantizer.apply of the real reference under CUDA autocast's casts (fp32 behind the reciprocal, fp32 result) on fresh tensors;
    the recorded gradient is the engine's cast of the fp32 gradient to the input's dtype (zeroing commutes with that cast)"""
    sem = O.SEM_DEVICE if device_scalars else O.SEM_CPU
    want_all = rec["autocast"][f"{dtype}/{int(device_scalars)}"]
    assert len(want_all) == AUTOCAST_TRIALS
    for (trial, x, bits, lo, hi, g), want in zip(autocast_cases(dtype, device_scalars), want_all):
        tag = f"trial {trial}: {dtype} {tuple(x.shape)} b{bits} device_scalars={device_scalars}"
        x_np = to_np(x)
        assert (digest(x_np, dtype), digest(g.numpy(), "fp32")) == (want["x"], want["g"]), f"{tag}: not the inputs the reference saw"
        r, c = O.rows_cols(tuple(x.shape), False)
        y, _ = O.sym_fwd_autocast(x_np, r, c, bits, dtype, wide=True, sem=sem)
        assert digest(y.reshape(x_np.shape), "fp32") == want["y"], f"{tag}: forward differs from the reference's"
        gx = O.ste_bwd_wide(g.numpy().copy(), x_np, lo, hi, dtype)
        assert digest(gx.reshape(x_np.shape), dtype) == want["gx"], f"{tag} gradient differs from the reference's"


def lowbit_cases(dtype, n=LOWBIT_TRIALS):
    """-> (trial, out_f, in_f, w_bits, layerwise, weight) with the weight as the reference's QuantizeLinear held it"""
    rng = np.random.default_rng({"bf16": 301, "fp16": 302, "fp32": 303}[dtype])
    for trial in range(n):
        out_f, in_f = int(rng.integers(1, 12)), int(rng.choice([1, 3, 8, 33, 128]))
        w_bits, layerwise = 1 + trial % 2, bool(rng.random() < 0.3)
        w = rng.standard_normal((out_f, in_f)).astype(np.float32) * rng.choice([1e-3, 0.02, 1.0, 30.0], size=(out_f, 1)).astype(np.float32)
        if rng.random() < 0.5:
            w[int(rng.integers(0, out_f)), int(rng.integers(0, in_f))] = np.float32(rng.choice([0.0, -0.0, 1e-30]))
        yield trial, out_f, in_f, w_bits, layerwise, torch.from_numpy(w).to(TD[dtype])


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_low_bit_weight_branches_equal_the_live_reference(rec, dtype):
    """QuantizeLinear's 1-/2-bit weight branches (:202-242): the weight the REAL module handed to F.linear (recorded) against the
    oracle's elementwise chain given the module's own mean-|w| scale (a float sum is order dependent: the scale is ATen's, as in w12.npz)."""
    want_all = rec["lowbit"][dtype]
    assert len(want_all) == LOWBIT_TRIALS
    for (trial, out_f, in_f, w_bits, layerwise, weight), want in zip(lowbit_cases(dtype), want_all):
        tag = f"trial {trial}: {dtype} [{out_f},{in_f}] w_bits={w_bits} lw={layerwise}"
        w_np = to_np(weight)
        assert digest(w_np, dtype) == want["w"], f"{tag}: not the weight the reference held"
        absmean = weight.abs().mean() if layerwise else weight.abs().mean(dim=1)
        sc = (absmean if w_bits == 1 else 2 * absmean).float().reshape(-1).numpy()
        if layerwise:
            got, _ = O.w12_fwd(w_np.reshape(1, -1), 1, out_f * in_f, w_bits, dtype, scale_in=sc)
        else:
            got, _ = O.w12_fwd(w_np, out_f, in_f, w_bits, dtype, scale_in=sc)
        assert digest(got.reshape(w_np.shape), dtype) == want["linear_weight"], f"{tag}: the oracle differs from the weight the reference handed to F.linear"


DEGENERATE_SHAPES = [(0, 8), (3, 0), (0,), (2, 0, 8), (2, 3, 0), (0, 0), (0, 3, 4, 8), (2, 3, 0, 8), (2, 0, 4, 8), (2, 3, 4, 0), (0, 0, 4, 8),
                     (1, 1), (1,), (5, 1), (), (1, 1, 1, 1), (1, 1, 1, 1, 2)]


def run_degenerate(q, shape, layerwise):
    """-> the exception type's name, or {"y": .., "grad": ..} as (shape, float32 bit patterns)"""
    x = torch.full(shape, 0.75).requires_grad_(True)
    try:
        y = q.apply(x, torch.tensor([-2.0, 2.0]), 8, layerwise)
        y.sum().backward()
    except Exception as e:  # noqa: BLE001
        return type(e).__name__
    return {k: [list(t.shape), t.detach().contiguous().numpy().view(np.uint32).reshape(-1).tolist()] for k, t in (("y", y), ("grad", x.grad))}


def test_degenerate_shapes_cpu_tensor_path_vs_the_live_reference(rec):
    """the drop-in's opt-in CPU-tensor path (llm_qat_amd.allow_cpu_tensors) on tensors without elements / with one element: the
    reference's recorded result, or the reference's exception type (tests/test_gpu_parity.py checks the same list on the GPU kernels'
    host path against the eager chain)"""
    import llm_qat_amd
    from llm_qat_amd.utils_quant import AsymQuantizer, SymQuantizer
    want_all = rec["degenerate"]
    llm_qat_amd.allow_cpu_tensors(True)
    try:
        for shape in DEGENERATE_SHAPES:
            for layerwise in (False, True):
                for q in (SymQuantizer, AsymQuantizer):
                    key = f"{q.__name__} {shape} layerwise={layerwise}"
                    want, got = want_all[key], run_degenerate(q, shape, layerwise)
                    if isinstance(want, str):
                        assert got == want, f"{key}: reference raises {want}, drop-in gave {got}"
                    else:
                        assert not isinstance(got, str), f"{key}: drop-in raised {got}"
                        assert got == want, key
    finally:
        llm_qat_amd.allow_cpu_tensors(False)
