"""The calls of the ABI-refusal transcript (tests/golden/abi_refusals.json), shared by the script that records it from the parent
commit's library (tests/golden/make_abi_refusals.py) and the test that replays it (tests/test_abi_refusals_cpu.py).

Two parts.  `seeded(L)`: the 400 seeded calls per launching entry point of
test_abi_and_host.py::test_abi_rejects_null_pointers_and_hostile_sizes_before_any_launch -- same seed, same argument lists, NULL pointers
only.  `HAND`: calls that reach the later checks with non-NULL pointers that are never dereferenced (0x1000, 0x2000, ...): every one is
refused before any launch, so nothing reaches HIP and no GPU is needed.  ctypes only, no kernel runs."""
import ctypes
import hashlib
import random

ERR_LAUNCH = -6
NOT_LAUNCHING = ("fq_version", "fq_build_info", "fq_last_error", "fq_rowwise_workspace_bytes", "fq_ste_mask_bytes", "fq_export_bins_bytes")
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 11008, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]
FLOATS = [0.0, -0.0, 1.0, -2.0, 2.0, float("inf"), float("-inf"), float("nan"), 1e-45, 3e38]


def launching(_lib):
    return [n for n in _lib.EXPORTS if n not in NOT_LAUNCHING]


def seeded(_lib, L):
    """-> (entry point, args) in the order the fuzz test makes its calls"""
    rng = random.Random(0)
    for name in launching(_lib):
        f = getattr(L, name)
        for _ in range(400):
            args = []
            for t in f.argtypes:
                if t is ctypes.c_void_p:
                    args.append(None)
                elif t is ctypes.c_float:
                    args.append(rng.choice(FLOATS))
                elif t is ctypes.c_int64:
                    args.append(rng.choice(INTS))
                elif t is ctypes.c_size_t:
                    args.append(rng.choice([v for v in INTS if v >= 0]))
                elif t is ctypes.c_int:
                    args.append(max(-(2 ** 31), min(2 ** 31 - 1, rng.choice(INTS))))
                else:   # POINTER(struct) of the multi-tensor entry points: NULL, or a table of zeroed slots
                    args.append(None if rng.random() < 0.5 else (t._type_ * _lib.MAX_TENSORS)())
            yield name, args


def call(L, name, args):
    rc = getattr(L, name)(*args)
    return rc, L.fq_last_error().decode(errors="replace")


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def seeded_lines(_lib, L):
    """-> {entry point: the ordered "rc|message" lines of its 400 seeded calls}"""
    lines = {}
    for name, args in seeded(_lib, L):
        rc, msg = call(L, name, args)
        lines.setdefault(name, []).append(f"{rc}|{msg}")
    return lines


def pairs_of(lines):
    """the distinct (rc, message) pairs of a list of "rc|message" lines"""
    return {(int(rc), msg) for rc, msg in (ln.split("|", 1) for ln in lines)}


# ---- the hand-written list ---------------------------------------------------------------------------------------------------------------
A, B, C, D, E_ = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000       # 16-byte aligned, never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
LO, HI = -2.0, 2.0
N = None


def _fwd(_lib, *slots):
    t = (_lib.FwdTensor * _lib.MAX_TENSORS)()
    for i, s in enumerate(slots):
        t[i] = _lib.FwdTensor(*s)
    return t


def _bwd_v(_lib, slot, gv, gxv):
    t = (_lib.BwdTensorV * _lib.MAX_TENSORS)()
    t[0] = _lib.BwdTensorV(*slot, _lib.RowsView(*gv), _lib.RowsView(*gxv))
    return t


def hand(_lib):
    """-> (id, entry point, args): [4, 64] bf16 tensors (one 64-bit mask word per row: 32 mask bytes) unless the check needs another shape"""
    view = ctypes.pointer(_lib.RowsView(2, 256, 128))           # rows that do not follow one another
    long_view = ctypes.pointer(_lib.RowsView(1, 140000, 140000))
    bad_view = ctypes.pointer(_lib.RowsView(2, -256, 128))
    H = [
        # y == x
        ("inplace sym_fwd", "fq_sym_fwd", [A, A, 4, 64, 4, BF16, 0, N, N, 0, N]),
        ("inplace asym_fwd", "fq_asym_fwd", [A, A, 4, 64, 4, F32, 0, N, N, 0, N]),
        ("inplace debug", "fq_sym_fwd_debug", [A, A, B, C, 4, 64, 4, BF16, 0, N, 0, N]),
        ("inplace train", "fq_sym_fwd_train", [A, A, 4, 64, 4, BF16, 0, LO, HI, B, C, 32, N]),
        ("inplace autocast", "fq_sym_fwd_autocast", [A, A, 4, 64, 8, BF16, 0, 1, LO, HI, N, N, 0, N, 0, N]),
        ("inplace rowwise_v", "fq_rowwise_fwd_v", [0, A, N, A, N, 4, 64, 4, BF16, 0, LO, HI, N, N, 0, N]),
        ("inplace group", "fq_group_fwd", [0, A, A, 4, 64, 32, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("inplace mx_fwd", "fq_mx_fwd", [A, A, 4, 64, 0, BF16, N]),
        ("inplace block_rotate", "fq_block_rotate", [A, A, 4, 64, BF16, N]),
        # the head checks of the forwards, each site's own wording
        ("y NULL sym_fwd", "fq_sym_fwd", [A, N, 4, 64, 4, BF16, 0, N, N, 0, N]),
        ("y NULL autocast", "fq_sym_fwd_autocast", [A, N, 4, 64, 8, F16, 0, 0, LO, HI, N, N, 0, N, 0, N]),
        ("negative sym_fwd", "fq_sym_fwd", [A, B, -4, 64, 4, BF16, 0, N, N, 0, N]),
        ("negative autocast", "fq_sym_fwd_autocast", [A, B, 4, -64, 8, BF16, 0, 0, LO, HI, N, N, 0, N, 0, N]),
        ("bits autocast", "fq_sym_fwd_autocast", [A, B, 4, 64, 32, BF16, 0, 0, LO, HI, N, N, 0, N, 0, N]),
        ("sem autocast", "fq_sym_fwd_autocast", [A, B, 4, 64, 8, BF16, 2, 0, LO, HI, N, N, 0, N, 0, N]),
        ("f64 bounds", "fq_sym_fwd", [A, B, 4, 64, 4, F64, 0, C, N, 0, N]),
        ("f64 train", "fq_asym_fwd_train", [A, B, 4, 64, 4, F64, 0, LO, HI, C, D, 32, N]),
        ("f64 view", "fq_rowwise_fwd_v", [1, A, view, B, N, 4, 64, 4, F64, 0, LO, HI, N, N, 0, N]),
        ("f64 unaligned", "fq_sym_fwd", [A + 4, B, 4, 64, 4, F64, 0, N, N, 0, N]),
        ("negative stride", "fq_rowwise_fwd_v", [0, A, bad_view, B, N, 4, 64, 4, BF16, 0, LO, HI, N, N, 0, N]),
        # a mask without bounds
        ("mask no bounds train", "fq_sym_fwd_train", [A, B, 4, 64, 4, BF16, 0, LO, HI, N, C, 32, N]),
        ("bounds no mask train", "fq_asym_fwd_train", [A, B, 4, 64, 4, BF16, 0, LO, HI, C, N, 32, N]),
        ("mask no bounds autocast", "fq_sym_fwd_autocast", [A, B, 4, 64, 8, BF16, 0, 1, LO, HI, N, C, 32, N, 0, N]),
        ("mask no bounds rowwise_v", "fq_rowwise_fwd_v", [1, A, N, B, N, 4, 64, 4, BF16, 0, LO, HI, N, C, 32, N]),
        ("mask no bounds row_scales", "fq_sym_row_scales", [A, N, 4, 64, 8, BF16, 0, 0, LO, HI, N, C, 32, N]),
        ("mask no bounds group", "fq_group_fwd", [0, A, B, 4, 64, 32, 4, BF16, 0, 0, LO, HI, N, C, 32, N]),
        ("mask no bounds multi", "fq_sym_fwd_multi", [1, _fwd(_lib, (A, B, 4, 4, N, C, 32)), 64, BF16, 0, 0, LO, HI, N]),
        # the mask buffer one byte short, and a shape the mask path does not serve
        ("mask short train", "fq_sym_fwd_train", [A, B, 4, 64, 4, BF16, 0, LO, HI, C, D, 31, N]),
        ("mask short asym train", "fq_asym_fwd_train", [A, B, 4, 64, 4, F32, 0, LO, HI, C, D, 31, N]),
        ("mask short autocast", "fq_sym_fwd_autocast", [A, B, 4, 64, 8, F16, 0, 0, LO, HI, C, D, 31, N, 0, N]),
        ("mask short rowwise_v", "fq_rowwise_fwd_v", [0, A, N, B, N, 4, 64, 4, BF16, 0, LO, HI, C, D, 31, N]),
        ("mask short row_scales", "fq_sym_row_scales", [A, N, 4, 64, 8, BF16, 0, 0, LO, HI, C, D, 31, N]),
        ("mask short group", "fq_group_fwd", [0, A, B, 4, 64, 32, 4, BF16, 0, 0, LO, HI, C, D, 31, N]),
        ("mask short bwd", "fq_ste_bwd_mask", [A, B, 4, 64, LO, HI, C, D, 31, BF16, N]),
        ("mask short multi", "fq_sym_fwd_multi", [1, _fwd(_lib, (A, B, 4, 4, C, D, 31)), 64, BF16, 0, 0, LO, HI, N]),
        ("mask shape train", "fq_sym_fwd_train", [A, B, 4, 100, 4, BF16, 0, LO, HI, C, D, 4096, N]),
        ("mask shape autocast", "fq_sym_fwd_autocast", [A, B, 4, 100, 8, BF16, 0, 0, LO, HI, C, D, 4096, N, 0, N]),
        ("mask shape row_scales", "fq_sym_row_scales", [A, N, 4, 100, 8, BF16, 0, 0, LO, HI, C, D, 4096, N]),
        ("mask shape bwd", "fq_ste_bwd_mask", [A, B, 4, 100, LO, HI, C, D, 4096, BF16, N]),
        ("mask unaligned train", "fq_sym_fwd_train", [A + 2, B, 4, 64, 4, BF16, 0, LO, HI, C, D, 32, N]),
        ("mask unaligned autocast", "fq_sym_fwd_autocast", [A + 2, B, 4, 64, 8, BF16, 0, 0, LO, HI, C, D, 32, N, 0, N]),
        ("mask unaligned wide", "fq_sym_fwd_autocast", [A + 4, B, 4, 64, 8, BF16, 0, 1, LO, HI, C, D, 32, N, 0, N]),
        ("mask unaligned row_scales", "fq_sym_row_scales", [A + 2, N, 4, 64, 8, BF16, 0, 0, LO, HI, C, D, 32, N]),
        # export: containers, autocast, what to produce, the grid
        ("container sym", "fq_sym_export", [A, B, N, N, 4, 64, 8, 7, BF16, 0, 0, N]),
        ("container asym", "fq_asym_export", [A, B, N, N, 4, 64, 8, -1, BF16, 0, N]),
        ("container none sym", "fq_sym_export", [A, B, N, N, 4, 64, 8, 0, BF16, 0, 0, N]),
        ("container none asym", "fq_asym_export", [A, B, N, N, 4, 64, 8, 0, BF16, 0, N]),
        ("autocast fp32 export", "fq_sym_export", [A, B, N, N, 4, 64, 8, 2, F32, 0, 1, N]),
        ("autocast fp32 row_scales", "fq_sym_row_scales", [A, B, 4, 64, 8, F32, 0, 1, LO, HI, N, N, 0, N]),
        ("bins NULL", "fq_asym_export", [A, N, B, N, 4, 64, 8, 2, BF16, 0, N]),
        ("nothing to produce", "fq_sym_row_scales", [A, N, 4, 64, 8, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("export dtype f64", "fq_sym_export", [A, B, N, N, 4, 64, 8, 2, F64, 0, 0, N]),
        ("export rows grid", "fq_sym_export", [A, B, N, N, 2 ** 31, 64, 8, 2, BF16, 0, 0, N]),
        # autocast on fp32 or Asym
        ("autocast fp32", "fq_sym_fwd_autocast", [A, B, 4, 64, 8, F32, 0, 1, LO, HI, N, N, 0, N, 0, N]),
        ("autocast f64", "fq_sym_fwd_autocast", [A, B, 4, 64, 8, F64, 0, 1, LO, HI, N, N, 0, N, 0, N]),
        ("autocast asym group", "fq_group_fwd", [1, A, B, 4, 64, 32, 4, BF16, 0, 1, LO, HI, N, N, 0, N]),
        ("autocast fp32 group", "fq_group_fwd", [0, A, B, 4, 64, 16, 4, F32, 0, 1, LO, HI, N, N, 0, N]),
        ("autocast 2 group", "fq_group_fwd", [0, A, B, 4, 64, 32, 4, BF16, 0, 2, LO, HI, N, N, 0, N]),
        ("autocast fp32 multi", "fq_sym_fwd_multi", [1, _fwd(_lib, (A, B, 4, 4, N, N, 0)), 64, F32, 0, 1, LO, HI, N]),
        ("autocast 3 multi", "fq_sym_fwd_multi", [1, _fwd(_lib, (A, B, 4, 4, N, N, 0)), 64, BF16, 0, 3, LO, HI, N]),
        ("autocast fp32 pair", "fq_sym_fwd_pair", [A, B, 4, 4, N, N, 0, C, D, 4, 8, N, N, 0, 64, F32, 0, 2, LO, HI, N]),
        # group-wise: the group, the row length, the grid, alignment
        ("group not dividing", "fq_group_fwd", [0, A, B, 4, 64, 48, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group of 3 vectors", "fq_group_fwd", [0, A, B, 4, 48, 24, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group of 2 vectors", "fq_group_fwd", [1, A, B, 4, 64, 8, 4, F32, 0, 0, LO, HI, N, N, 0, N]),
        ("group half vectors", "fq_group_fwd", [0, A, B, 4, 60, 20, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group zero", "fq_group_fwd", [0, A, B, 4, 64, 0, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group asym code", "fq_group_fwd", [2, A, B, 4, 64, 32, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group f64", "fq_group_fwd", [0, A, B, 4, 64, 32, 4, F64, 0, 0, LO, HI, N, N, 0, N]),
        ("group long rows", "fq_group_fwd", [0, A, B, 4, 8 * 8192 + 64, 64, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group rows grid", "fq_group_fwd", [0, A, B, 2 ** 31, 64, 32, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group unaligned", "fq_group_fwd", [0, A + 8, B, 4, 64, 32, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        ("group overflow", "fq_group_fwd", [0, A, B, 2 ** 62, 64, 32, 4, BF16, 0, 0, LO, HI, N, N, 0, N]),
        # MX: formats, flags, shapes, aliasing, alignment, the grid
        ("mx fmt unknown fwd", "fq_mx_fwd", [A, B, 4, 64, -1, BF16, N]),
        ("mx fmt unknown export", "fq_mx_export", [A, B, C, 4, 64, 9, BF16, N]),
        ("mx fp6 export", "fq_mx_export", [A, B, C, 4, 64, 1, BF16, N]),
        ("mx fp6 export_rot", "fq_mx_export_rot", [A, B, C, 4, 64, 2, F16, N]),
        ("mx fp6 export_ex", "fq_mx_export_ex", [A, B, C, 4, 64, 2, F32, 2, N]),
        ("mx f64", "fq_mx_fwd", [A, B, 4, 64, 0, F64, N]),
        ("mx f64 bwd", "fq_mx_ste_bwd", [A, B, C, 4, 64, F64, 0, N]),
        ("mx dtype", "fq_block_rotate", [A, B, 4, 64, 4, N]),
        ("mx flags fwd_ex", "fq_mx_fwd_ex", [A, B, N, 4, 64, 0, BF16, 4, N]),
        ("mx flags export_ex", "fq_mx_export_ex", [A, B, C, 4, 64, 0, BF16, 8, N]),
        ("mx flags bwd", "fq_mx_ste_bwd", [A, B, C, 4, 64, BF16, 2, N]),
        ("mx flags before dtype", "fq_mx_fwd_ex", [A, B, N, 4, 64, 0, 9, 4, N]),
        ("mx dtype before flags bwd", "fq_mx_ste_bwd", [A, B, C, 4, 64, 9, 2, N]),
        ("mx rot cols fwd_rot", "fq_mx_fwd_rot", [A, B, 4, 96, 0, BF16, N]),
        ("mx rot cols export_rot", "fq_mx_export_rot", [A, B, C, 4, 96, 3, BF16, N]),
        ("mx rot cols block_rotate", "fq_block_rotate", [A, B, 4, 32, BF16, N]),
        ("mx rot cols fwd_ex", "fq_mx_fwd_ex", [A, B, N, 4, 96, 0, BF16, 1, N]),
        ("mx rot cols bwd", "fq_mx_ste_bwd", [A, B, C, 4, 96, BF16, 1, N]),
        ("mx block cols fwd", "fq_mx_fwd", [A, B, 4, 48, 0, BF16, N]),
        ("mx block cols bwd", "fq_mx_ste_bwd", [A, B, C, 4, 48, BF16, 0, N]),
        ("mx negative", "fq_mx_export", [A, B, C, -4, 64, 0, BF16, N]),
        ("mx negative bwd", "fq_mx_ste_bwd", [A, B, C, 4, -64, BF16, 0, N]),
        ("mx overflow", "fq_mx_fwd", [A, B, 2 ** 56, 64, 0, BF16, N]),
        ("mx overflow bwd", "fq_mx_ste_bwd", [A, B, C, 2 ** 56, 64, BF16, 1, N]),
        ("mx NULL fwd", "fq_mx_fwd", [A, N, 4, 64, 0, BF16, N]),
        ("mx NULL export", "fq_mx_export", [A, B, N, 4, 64, 0, BF16, N]),
        ("mx NULL bwd", "fq_mx_ste_bwd", [A, N, C, 4, 64, BF16, 0, N]),
        ("mx mask is x", "fq_mx_fwd_ex", [A, B, A, 4, 64, 0, BF16, 0, N]),
        ("mx mask is y", "fq_mx_fwd_ex", [A, B, B, 4, 64, 3, BF16, 3, N]),
        ("mx mask is g", "fq_mx_ste_bwd", [A, A, C, 4, 64, BF16, 0, N]),
        ("mx mask is gx", "fq_mx_ste_bwd", [A, C, C, 4, 64, BF16, 0, N]),
        ("mx gx is g rotated", "fq_mx_ste_bwd", [A, B, A, 4, 64, BF16, 1, N]),
        ("mx unaligned fwd", "fq_mx_fwd", [A, B + 8, 4, 64, 0, BF16, N]),
        ("mx unaligned export", "fq_mx_export", [A, B, C + 4, 4, 64, 0, BF16, N]),
        ("mx unaligned mask", "fq_mx_fwd_ex", [A, B, C + 8, 4, 64, 0, BF16, 0, N]),
        ("mx unaligned bwd", "fq_mx_ste_bwd", [A, B + 4, C, 4, 64, BF16, 0, N]),
        ("mx grid fwd", "fq_mx_fwd", [A, B, 2 ** 30, 2 ** 14, 0, BF16, N]),
        ("mx grid export", "fq_mx_export", [A, B, C, 2 ** 30, 2 ** 14, 0, BF16, N]),
        ("mx grid bwd", "fq_mx_ste_bwd", [A, B, C, 2 ** 30, 2 ** 14, BF16, 0, N]),
        # the MX GEMM
        ("gemm K 64", "fq_mx_gemm", [A, B, 0, C, D, 0, E_, 16, 16, 64, BF16, N]),
        ("gemm K 0", "fq_mx_gemm", [A, B, 0, C, D, 0, E_, 16, 16, 0, BF16, N]),
        ("gemm K 192", "fq_mx_gemm", [A, B, 3, C, D, 4, E_, 16, 16, 192, F32, N]),
        ("gemm fp6", "fq_mx_gemm", [A, B, 1, C, D, 0, E_, 16, 16, 128, BF16, N]),
        ("gemm fmt", "fq_mx_gemm", [A, B, 0, C, D, 5, E_, 16, 16, 128, BF16, N]),
        ("gemm f64", "fq_mx_gemm", [A, B, 0, C, D, 0, E_, 16, 16, 128, F64, N]),
        ("gemm M", "fq_mx_gemm", [A, B, 0, C, D, 0, E_, 2 ** 31, 16, 128, BF16, N]),
        ("gemm NULL", "fq_mx_gemm", [A, N, 0, C, D, 0, E_, 16, 16, 128, BF16, N]),
        ("gemm unaligned", "fq_mx_gemm", [A, B, 0, C, D, 0, E_ + 8, 16, 16, 128, BF16, N]),
        ("gemm N grid", "fq_mx_gemm", [A, B, 0, C, D, 0, E_, 64, 2 ** 23, 128, BF16, N]),
        # the mask backwards
        ("wide rows0 zero", "fq_ste_bwd_mask_wide", [A, B, 0, C, D, A, B, 4, C, D, 64, LO, HI, BF16, N]),
        ("wide fp32", "fq_ste_bwd_mask_wide", [A, B, 4, C, D, N, N, 0, N, N, 64, LO, HI, F32, N]),
        ("wide shape", "fq_ste_bwd_mask_wide", [A, B, 4, C, D, N, N, 0, N, N, 100, LO, HI, BF16, N]),
        ("wide unaligned", "fq_ste_bwd_mask_wide", [A + 8, B, 4, C, D, N, N, 0, N, N, 64, LO, HI, BF16, N]),
        ("pair bwd NULL mask", "fq_ste_bwd_mask_pair", [A, B, 4, C, D, A, B, 4, C, N, 64, LO, HI, BF16, N]),
        ("bwd mask unaligned", "fq_ste_bwd_mask", [A + 8, B, 4, 64, LO, HI, C, D, 32, BF16, N]),
        ("in-place unequal views", "fq_ste_bwd_mask_multi_v", [1, _bwd_v(_lib, (A, A, 4, B, C), (2, 256, 128), (0, 0, 0)), 64, LO, HI, BF16, 0, N]),
        ("multi_v negative stride", "fq_ste_bwd_mask_multi_v", [1, _bwd_v(_lib, (A, B, 4, C, D), (2, -256, 128), (0, 0, 0)), 64, LO, HI, BF16, 0, N]),
        ("multi wide fp32", "fq_ste_bwd_mask_multi_v", [1, _bwd_v(_lib, (A, B, 4, C, D), (0, 0, 0), (0, 0, 0)), 64, LO, HI, F32, 1, N]),
        # launchers that refuse before their first launch
        ("pair unaligned", "fq_sym_fwd_pair", [A, B, 4, 4, N, N, 0, C + 8, D, 4, 8, N, N, 0, 64, BF16, 0, 0, LO, HI, N]),
        ("pair autocast unaligned", "fq_sym_fwd_pair", [A, B, 4, 4, N, N, 0, C + 8, D, 4, 8, N, N, 0, 64, BF16, 0, 1, LO, HI, N]),
        ("pair wide unaligned", "fq_sym_fwd_pair", [A, B, 4, 4, N, N, 0, C + 4, D, 4, 8, N, N, 0, 64, BF16, 0, 2, LO, HI, N]),
        ("two-pass no workspace", "fq_sym_fwd", [A, B, 2, 70000, 4, BF16, 0, N, N, 0, N]),
        ("two-pass small workspace", "fq_asym_fwd", [A, B, 2, 70000, 4, BF16, 0, N, C, 15, N]),
        ("two-pass odd no workspace", "fq_sym_fwd", [A, B, 2, 70001, 4, F32, 0, N, N, 0, N]),
        ("two-pass grid", "fq_sym_fwd", [A, B, 2 ** 20, 2 ** 24, 4, BF16, 0, N, C, 2 ** 23, N]),
        ("two-pass view", "fq_rowwise_fwd_v", [0, A, long_view, B, N, 2, 70000, 4, BF16, 0, LO, HI, N, N, 0, N]),
        ("two-pass autocast no workspace", "fq_sym_fwd_autocast", [A, B, 2, 70000, 8, BF16, 0, 0, LO, HI, N, N, 0, N, 0, N]),
        ("two-pass wide small workspace", "fq_sym_fwd_autocast", [A, B, 2, 70000, 8, F16, 0, 1, LO, HI, N, N, 0, C, 15, N]),
        ("rows grid sym_fwd", "fq_sym_fwd", [A, B, 2 ** 31, 64, 4, BF16, 0, N, N, 0, N]),
        ("rows grid autocast", "fq_sym_fwd_autocast", [A, B, 2 ** 31, 64, 8, BF16, 0, 0, LO, HI, N, N, 0, N, 0, N]),
        ("ste n too large", "fq_ste_bwd", [A, B, C, 2 ** 50, LO, HI, BF16, N]),
        ("ste_v unaligned view", "fq_ste_bwd_v", [A + 8, view, B, N, C, N, 4, 64, LO, HI, N, BF16, N]),
        ("w12 too large", "fq_w12_fwd", [A, B, C, 2 ** 22, 2 ** 22, 1, 1, BF16, N]),
        ("w12 bits", "fq_w12_fwd", [A, B, C, 4, 64, 3, 1, BF16, N]),
        ("w12_rows small", "fq_w12_fwd_rows", [A, B, N, 4, 64, 1, BF16, N]),
        ("w12_rows long", "fq_w12_fwd_rows", [A, B, N, 8, 2 ** 20, 2, BF16, N]),
        ("w12_rows f64", "fq_w12_fwd_rows", [A, B, N, 8, 256, 1, F64, N]),
    ]
    assert len({h[0] for h in H}) == len(H)
    return H
