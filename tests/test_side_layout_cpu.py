"""The side buffer of a training forward (ops.split_side): float32 [rows, 2] row bounds followed by the STE row bitmap, both views of the
one uint8 allocation.  Host logic only: CPU tensors, no kernel."""
import numpy as np
import pytest
import torch

from llm_qat_amd import ops


def test_the_bounds_of_one_row_are_two_floats():
    assert ops.SIDE_ROW_BYTES == 2 * torch.finfo(torch.float32).bits // 8


@pytest.mark.parametrize("m", [8, 40])
@pytest.mark.parametrize("rows", [1, 5])
def test_split_side_gives_views_of_the_buffer(rows, m):
    nb = rows * 8
    raw = (np.arange(nb + m) * 7 + 3).astype(np.uint8)
    side = torch.from_numpy(raw.copy())
    bounds, mask = ops.split_side(side, rows)
    assert bounds.dtype is torch.float32 and tuple(bounds.shape) == (rows, 2) and bounds.is_contiguous()
    assert mask.dtype is torch.uint8 and tuple(mask.shape) == (m,)
    assert bounds.data_ptr() == side.data_ptr() and mask.data_ptr() == side.data_ptr() + nb
    assert bounds.untyped_storage().data_ptr() == side.untyped_storage().data_ptr() == mask.untyped_storage().data_ptr()
    assert bounds.storage_offset() == 0 and mask.storage_offset() == nb
    assert np.array_equal(bounds.numpy().view(np.uint8).reshape(-1), raw[:nb]) and np.array_equal(mask.numpy(), raw[nb:])
    # a write through either view lands in the buffer, at its place and nowhere else
    bounds[rows - 1, 1] = 1.5
    mask[m - 1] = 0xA5
    want = raw.copy()
    want[nb - 4: nb] = np.frombuffer(np.float32(1.5).tobytes(), np.uint8)
    want[-1] = 0xA5
    assert np.array_equal(side.numpy(), want)
