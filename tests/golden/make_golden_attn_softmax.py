#!/usr/bin/env python3
"""Golden vectors of the lines between the two attention products of the reference's own LlamaAttention.forward
(models/modeling_llama_quant.py:352-375) on CPU tensors -> attn_softmax.npz.

    LLMQAT_REFERENCE=<checkout of the reference> python tests/golden/make_golden_attn_softmax.py

A tiny LlamaAttention (hidden 64, 4 heads of 16, unquantized) runs with output_attentions=True under a function mode that keeps the first
torch.matmul result (the scores) and calls retain_grad() on it.  Recorded per case: the scores, the mask, the returned attn_weights, an
upstream gradient of them and the scores' gradient.  Cases: bf16 / fp16 / fp32 modules with the mask in the module's dtype, the 16-bit
ones with an fp32 mask too; a causal mask, a causal mask plus left padding (fully masked rows, elements of -inf where both masks add
up, and one row of -inf only), and T != S behind a past.  16-bit values are stored as bit patterns (uint16).  Only the generator reads the
reference; the tests read the .npz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if "LLMQAT_REFERENCE" not in os.environ:
    raise SystemExit("set LLMQAT_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["LLMQAT_REFERENCE"])

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.overrides import TorchFunctionMode  # noqa: E402

from models.configuration_llama import LlamaConfig  # noqa: E402
from models.modeling_llama_quant import LlamaAttention  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
HIDDEN, HEADS, B, T, PAST = 64, 4, 2, 8, 5
KINDS = ("causal", "padded", "past")


class KeepScores(TorchFunctionMode):
    """keeps the first torch.matmul result, with its gradient retained"""
    scores = None

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func is torch.matmul and self.scores is None:
            out.retain_grad()
            self.scores = out
        return out


def store(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy()


def mask_of(kind, dt):
    neg = torch.finfo(dt).min
    S = T + PAST if kind == "past" else T
    col = torch.arange(S).unsqueeze(0)
    causal = torch.where(col > (S - T + torch.arange(T)).unsqueeze(1), neg, 0.0).to(dt).expand(B, 1, T, S).clone()
    if kind != "padded":
        return causal
    pad = torch.zeros(B, 1, T, S, dtype=dt)
    pad[1, :, :, :3] = neg                      # batch element 1 is left-padded by three tokens: its rows 0..2 are fully masked
    m = causal + pad                            # both masks: -inf
    m[1, :, 1, :] = float("-inf")               # and one row of -inf only
    return m


def main():
    out = {"dtypes": np.array(list(DT)), "kinds": np.array(KINDS), "head_dim": np.array(HIDDEN // HEADS)}
    cfg = LlamaConfig(vocab_size=32, hidden_size=HIDDEN, intermediate_size=128, num_hidden_layers=1, num_attention_heads=HEADS,
                      max_position_embeddings=32, w_bits=32, a_bits=32, kv_bits=32, hidden_act="silu")
    for di, (name, dt) in enumerate(DT.items()):
        for mname, mdt in ((name, dt),) + ((("f32", torch.float32),) if dt != torch.float32 else ()):
            for ki, kind in enumerate(KINDS):
                torch.manual_seed(1000 * di + 10 * ki + (mdt != dt))
                attn = LlamaAttention(cfg).to(dt)
                for p in attn.parameters():
                    p.data.mul_(6.0)           # scores of a few units, so that the softmax is not flat
                h = torch.randn(B, T, HIDDEN).to(dt)
                past = None
                pos = torch.arange(T).unsqueeze(0).expand(B, T)
                if kind == "past":
                    past = tuple(torch.randn(B, HEADS, PAST, HIDDEN // HEADS).to(dt) for _ in range(2))
                    pos = pos + PAST
                mask = mask_of(kind, mdt)
                # (a 16-bit module beside an fp32 mask: the sum promotes, and the reference's cast to q's dtype brings the probabilities back)
                with KeepScores() as keep:
                    _, y, _ = attn(h, attention_mask=mask, position_ids=pos, past_key_value=past, output_attentions=True)
                scores = keep.scores
                gy = torch.randn(y.shape).to(y.dtype)
                y.backward(gy)
                assert scores.grad is not None and scores.dtype == dt and y.dtype == dt, (scores.dtype, y.dtype)
                key = f"{name}_{mname}_{kind}_"
                out.update({key + "scores": store(scores), key + "mask": store(mask), key + "y": store(y), key + "gy": store(gy),
                            key + "dscores": store(scores.grad)})
    path = os.path.join(HERE, "attn_softmax.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
