"""Host-side checks of the object tables (iodine_amd.objects, iodine_slot_table / iodine_seg_overlap): the float64 reference the GPU
tests compare against on a hand-computed case, the exports, the argument checks the entry points make before they touch a device, and
the host math of slot_iou.  No GPU."""
import ctypes as C
import os

import pytest
import torch

import objects_reference as R
from iodine_amd import _lib, objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID


def test_reference_on_a_hand_computed_case():
    """S = 8, K = 2: slot 0 holds 0.75 on the left half (cols 0..3) and 0.25 on the right, slot 1 the rest.
    soft_area_0 = 32 * 0.75 + 32 * 0.25 = 32.  sum m col for slot 0 = 8 rows * (0.75 * (0+1+2+3) + 0.25 * (4+5+6+7)) = 8 * (4.5 + 5.5) = 80,
    so soft_cx_0 = 80 / 32 = 2.5; slot 1 mirrors it: 8 * (0.25 * 6 + 0.75 * 22) = 144, soft_cx_1 = 4.5.  Rows are symmetric: soft_cy = 3.5."""
    S = 8
    mask = torch.empty(1, 2, 1, S, S)
    mask[0, 0, 0, :, :4], mask[0, 0, 0, :, 4:] = 0.75, 0.25
    mask[0, 1] = 1.0 - mask[0, 0]
    mean = torch.zeros(1, 2, 3, S, S)
    mean[0, 0, 0], mean[0, 0, 1, :, :4], mean[0, 1, 2] = 1.0, 1.0, 0.5
    t, seg = R.slot_table(mask, mean)
    assert seg.dtype == torch.uint8 and torch.equal(seg[0, :, :4], torch.zeros(S, 4, dtype=torch.uint8))
    assert torch.equal(seg[0, :, 4:], torch.ones(S, 4, dtype=torch.uint8))
    col = {n: i for i, n in enumerate(R.COLUMNS)}
    assert t[0, :, col['hard_area']].tolist() == [32.0, 32.0]
    assert t[0, 0, 6:10].tolist() == [0.0, 0.0, 3.0, 7.0] and t[0, 1, 6:10].tolist() == [4.0, 0.0, 7.0, 7.0]
    assert t[0, :, col['hard_cx']].tolist() == [1.5, 5.5] and t[0, :, col['hard_cy']].tolist() == [3.5, 3.5]
    assert t[0, :, col['soft_area']].tolist() == [32.0, 32.0]
    assert t[0, :, col['soft_cx']].tolist() == [2.5, 4.5] and t[0, :, col['soft_cy']].tolist() == [3.5, 3.5]
    # colours: slot 0 red everywhere -> r = 1; green on the left half only -> g = 32 * 0.75 / 32 = 0.75; slot 1 blue 0.5 everywhere
    assert t[0, 0, 10:13].tolist() == [1.0, 0.75, 0.0] and t[0, 1, 10:13].tolist() == [0.0, 0.0, 0.5]
    assert t[0, :, col['peak']].tolist() == [0.75, 0.75]
    # ties go to the lowest index, an all-zero slot is empty, and without mean the colours are 0
    tie = torch.full((1, 3, 1, 4, 4), 0.5)
    tie[0, 2] = 0.0
    t2, seg2 = R.slot_table(tie)
    assert int(seg2.max()) == 0 and t2[0, :, 1].tolist() == [16.0, 0.0, 0.0]
    assert t2[0, 1, 4:10].tolist() == [-1.0] * 6 and t2[0, 2, [0, 2, 3, 10, 11, 12]].tolist() == [0.0] * 6
    ov = R.overlap_table(seg, seg2.new_zeros(1, S, S), 2, 3)
    assert ov[0].tolist() == [[32, 0, 0], [32, 0, 0]]


def test_columns_and_exports():
    assert len(objects.SLOT_COLUMNS) == 14 and tuple(objects.SLOT_COLUMNS) == R.COLUMNS
    import iodine_amd
    assert iodine_amd.slot_table is objects.slot_table and iodine_amd.SLOT_COLUMNS is objects.SLOT_COLUMNS
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in ('iodine_slot_table', 'iodine_seg_overlap'):
        assert name in _lib.EXPORTS and hasattr(L, name) and f'int {name}(' in header, name
    assert L.iodine_abi_version() == 3


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every one of these returns IODINE_ERR_INVALID before a launch: the pointers are never dereferenced on the host, so dummy non-null
    addresses stand in for device memory."""
    L = _lib.lib()
    p, null = C.c_void_p(4096), None
    st = C.c_void_p(0)
    assert L.iodine_slot_table(st, null, p, 1, 2, 8, p, p) == INVALID            # mask
    assert L.iodine_slot_table(st, p, p, 1, 2, 8, null, p) == INVALID            # table
    assert b'iodine_slot_table' in L.iodine_last_error(None)
    for slots in (0, 17, -1):
        assert L.iodine_slot_table(st, p, null, 1, slots, 8, p, null) == INVALID
    for size in (0, 1025, -3):
        assert L.iodine_slot_table(st, p, null, 1, 2, size, p, null) == INVALID
    assert L.iodine_slot_table(st, p, null, 0, 2, 8, p, null) == INVALID         # batch
    for args in ((null, p, p), (p, null, p), (p, p, null)):                      # seg_a, seg_b, table
        assert L.iodine_seg_overlap(st, args[0], args[1], 1, 2, 2, 64, args[2]) == INVALID
    assert b'iodine_seg_overlap' in L.iodine_last_error(None)
    for ka, kb in ((0, 2), (17, 2), (2, 0), (2, 17)):
        assert L.iodine_seg_overlap(st, p, p, 1, ka, kb, 64, p) == INVALID
    for pixels in (0, -1, 1025 * 1025):                                          # size 0 and 1025 as pixel counts
        assert L.iodine_seg_overlap(st, p, p, 1, 2, 2, pixels, p) == INVALID
    assert L.iodine_seg_overlap(st, p, p, 0, 2, 2, 64, p) == INVALID             # batch


def test_python_layer_refuses_cpu_tensors_and_wrong_shapes():
    mask = torch.rand(2, 3, 1, 8, 8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        objects.slot_table(mask)
    with pytest.raises(RuntimeError, match='ROCm device'):
        objects.slot_table(mask, torch.rand(2, 3, 3, 8, 8), segmentation=True)
    seg = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        objects.overlap_table(seg, seg, 3, 3)


def test_slot_iou_on_hand_numbers():
    """rows 4 / 6 / 0, columns 5 / 5: iou[i][j] = t / (row_i + col_j - t); the empty third segment has union col_j > 0 and iou 0, and an
    all-zero table (union 0 everywhere) gives 0, not NaN."""
    t = torch.tensor([[3, 1], [2, 4], [0, 0]], dtype=torch.int32)
    iou = objects.slot_iou(t)
    assert iou.dtype == torch.float64 and iou.shape == (3, 2)
    want = torch.tensor([[3 / 6, 1 / 8], [2 / 9, 4 / 7], [0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(iou, want)
    z = objects.slot_iou(torch.zeros(2, 2, 3, dtype=torch.int32))
    assert z.shape == (2, 2, 3) and float(z.abs().max()) == 0.0 and not torch.isnan(z).any()
    batched = objects.slot_iou(torch.stack([t, t.flip(0)]))
    assert torch.equal(batched[0], want) and torch.equal(batched[1], want.flip(0))


def test_model_starts_without_objects():
    from util import golden_setup, hip_arch, load_golden
    from iodine_amd import IODINE
    arch = golden_setup(load_golden('tiny'))[0]
    assert IODINE(hip_arch(arch)).objects is None
