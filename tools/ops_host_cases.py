"""Host time of ops.py's masked STE backwards and pair forward on tensors small enough to be host-bound, one process's figures as one JSON
line: HIP events around 200 calls, 7 rounds, the median of the rounds (group_bench.time_rounds).  Run it in fresh processes of two
trees in turn to compare them (profiles/ops_fold_host_ab.txt).

    python tools/ops_host_cases.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from group_bench import time_rounds  # noqa: E402

LO, HI = -2.0, 2.0


def main():
    import llm_qat_amd
    from llm_qat_amd import ops
    from llm_qat_amd.utils_quant import QuantizeLinear
    gen = torch.Generator(device="cpu").manual_seed(11)

    def t(rows, cols=256, dtype=torch.bfloat16, scale=1.0):
        return (torch.randn(rows, cols, generator=gen) * scale).to(dtype).cuda()
    x, w, w2 = t(32, scale=1.5), t(8, scale=1.5), t(8, scale=1.5)
    gx, gw, gw2, gx32 = t(32), t(8), t(8), t(32, dtype=torch.float32)
    _, side_x, _, cols = ops.train_forward("sym", x, 8, False, LO, HI)
    _, side_w, _, _ = ops.train_forward("sym", w, 4, False, LO, HI)
    _, side_w2, _, _ = ops.train_forward("sym", w2, 4, False, LO, HI)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, side_wide, _, _, got = ops.sym_forward_autocast(x, 8, False, wide=True, lo=LO, hi=HI, train="mask")
    assert got == "mask"
    lin = QuantizeLinear(128, 96, w_bits=4, a_bits=8).cuda().bfloat16()
    tokens, go = t(32, 128).requires_grad_(True), t(32, 96)

    def step(i):
        lin(tokens).backward(go)

    variants = {
        "train_backward": lambda i: ops.train_backward(gx, side_x, 32, cols, LO, HI),
        "train_backward in place": lambda i: ops.train_backward(gx, side_x, 32, cols, LO, HI, inplace=True),
        "train_backward_wide": lambda i: ops.train_backward_wide(gx32, side_wide, 32, cols, LO, HI, torch.bfloat16),
        "pair_backward": lambda i: ops.pair_backward(gw, gx, side_w, side_x, 8, 32, cols, LO, HI),
        "multi_backward 3": lambda i: ops.multi_backward([gx, gw, gw2], [side_x, side_w, side_w2], [32, 8, 8], cols, LO, HI),
        "pair_forward": lambda i: ops.pair_forward(w, x, 4, 8, LO, HI, True, True),
        "QuantizeLinear 128->96 step, C++ node": step,
    }
    res = time_rounds(variants, 200, 7, warmup=20)
    node = llm_qat_amd.host_node()
    llm_qat_amd.cpp_node(False)     # the Python nodes: the route that runs pair_forward / pair_backward
    res.update(time_rounds({"QuantizeLinear 128->96 step, Python node": step}, 200, 7, warmup=20))
    print(json.dumps({"host_node": node, "us_per_call": {k: v["median"] for k, v in res.items()}}))


if __name__ == "__main__":
    main()
