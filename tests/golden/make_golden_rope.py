#!/usr/bin/env python3
"""Golden vectors of the reference's own LlamaRotaryEmbedding and apply_rotary_pos_emb (models/modeling_llama_quant.py:132-196) on CPU
tensors -> rope.npz.

    LLMQAT_REFERENCE=<checkout of the reference> python tests/golden/make_golden_rope.py

For bf16, fp16 and fp32 and the shapes of SHAPES: q and k (the reference's transposed views over [B, T, H * D] memory, randn), shuffled
and repeated position_ids, the gradients gq and gk of the results -> q_embed, k_embed, dq, dk, with the cached fp32 tables of the
rotary module (cos_cached, sin_cached) that its forward casts to the tensors' dtype.  Per dtype one special case: zeros of either sign
planted in q, k and in whole rows of the gradients.  16-bit values are stored as bit patterns (uint16), every tensor contiguous in
[B, H, T, D] order.  Only the generator reads the reference; the tests read the .npz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if "LLMQAT_REFERENCE" not in os.environ:
    raise SystemExit("set LLMQAT_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["LLMQAT_REFERENCE"])

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.modeling_llama_quant import LlamaRotaryEmbedding, apply_rotary_pos_emb  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SHAPES = ((2, 3, 3, 5, 8), (1, 4, 2, 7, 64), (2, 2, 1, 3, 2))      # B, Hq, Hk, T, D
P = 16


def store(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy()


def view(B, H, T, D, dt, gen):
    return torch.randn(B, T, H * D, generator=gen).to(dt).view(B, T, H, D).transpose(1, 2)


def reference(q, k, pos, gq, gk):
    rot = LlamaRotaryEmbedding(q.shape[-1], max_position_embeddings=P)
    qr, kr = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
    cos, sin = rot(qr, seq_len=P)
    qe, ke = apply_rotary_pos_emb(qr, kr, cos, sin, pos)
    dq, dk = torch.autograd.grad((qe, ke), (qr, kr), (gq, gk))
    assert qe.dtype == dq.dtype == q.dtype and qe.stride() == q.stride()
    return qe, ke, dq, dk, rot.cos_cached[0, 0], rot.sin_cached[0, 0]


def main():
    out = {"dtypes": np.array(list(DT)), "shapes": np.array(SHAPES), "P": np.array(P)}
    for di, (name, dt) in enumerate(DT.items()):
        for si, (B, Hq, Hk, T, D) in enumerate(SHAPES + (SHAPES[0],)):
            special = si == len(SHAPES)
            gen = torch.Generator().manual_seed(100 * di + si)
            q, k = view(B, Hq, T, D, dt, gen), view(B, Hk, T, D, dt, gen)
            gq, gk = view(B, Hq, T, D, dt, gen), view(B, Hk, T, D, dt, gen)
            pos = torch.randint(0, P, (B, T), generator=gen)
            if special:                       # zeros of either sign in the inputs, and whole gradient rows of +0 and of -0
                q, k, gq, gk = q.clone(), k.clone(), gq.clone(), gk.clone()
                q[0, 0, 0, :] = 0.0
                q[0, 1, 1, :] = -0.0
                k[0, 0, 2, : D // 2] = -0.0
                gq[0, 0, 0, :] = 0.0
                gq[0, 1, 1, :] = -0.0
                gk[0, 0, 0, :] = -0.0
                gk[0, 2, 3, D // 2:] = 0.0
            qe, ke, dq, dk, cos, sin = reference(q, k, pos, gq, gk)
            key = f"{name}_{'special' if special else 's%d' % si}_"
            out.update({key + "q": store(q), key + "k": store(k), key + "gq": store(gq), key + "gk": store(gk), key + "pos": pos.numpy(),
                        key + "qe": store(qe), key + "ke": store(ke), key + "dq": store(dq), key + "dk": store(dk)})
            out[f"cos_d{D}"], out[f"sin_d{D}"] = cos.numpy(), sin.numpy()
    path = os.path.join(HERE, "rope.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
