"""Host-side checks of the decomposition sheets (iodine_amd.figures, iodine_render_sheet / iodine_sheet_size): the numpy reference the GPU
tests compare against on a hand-computed case, the layout arithmetic, the palette, the PNG encoder, the argument checks the entry points
make before they touch a device, and the refusals of the Python layer.  No GPU."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import sheet_reference as R
from iodine_amd import _lib, figures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID


def test_reference_on_a_hand_computed_case():
    """S = 2, K = 2, pad = 1 of (9, 9, 9), panels seg and slot_masked 0: a 4 x 7 sheet.
    m_0 = [[0.75, 0.25], [0.5, 0.5]], m_1 = 1 - m_0: labels [[0, 1], [0, 0]] (the tie goes to slot 0), so seg is palette 0 = (230, 25, 75)
    except palette 1 = (60, 180, 75) at the top right.  mean_0 = (1, 0, 0.5), background 1:  r = m + (1 - m) = 1 -> 255;
    g = 1 - m: 0.25 -> int(64.25) = 64, 0.75 -> int(191.75) = 191, 0.5 -> int(128.0) = 128;
    b = 0.5 m + (1 - m): 0.625 -> int(159.875) = 159, 0.875 -> int(223.625) = 223, 0.75 -> int(191.75) = 191."""
    mask = np.array([[[[0.75, 0.25], [0.5, 0.5]], [[0.25, 0.75], [0.5, 0.5]]]], dtype=np.float32)
    mean = np.zeros((1, 2, 3, 2, 2), dtype=np.float32)
    mean[0, 0, 0], mean[0, 0, 2] = 1.0, 0.5
    got = R.sheet([('seg', 0), ('slot_masked', 0)], figures.PALETTE, mask, scale=1, pad=1, pad_value=(9, 9, 9), mean=mean)
    P, A, B = [9, 9, 9], [230, 25, 75], [60, 180, 75]
    want = np.array([[P, P, P, P, P, P, P],
                     [P, A, B, P, [255, 64, 159], [255, 191, 223], P],
                     [P, A, A, P, [255, 128, 191], [255, 128, 191], P],
                     [P, P, P, P, P, P, P]], dtype=np.uint8)
    assert got.dtype == np.uint8 and got.shape == (4, 7, 3)
    assert np.array_equal(got, want)
    # replication: every source pixel becomes a 2 x 2 square, the padding keeps its width
    big = R.sheet([('seg', 0)], figures.PALETTE, mask, scale=2, pad=1, pad_value=(9, 9, 9))
    assert big.shape == (6, 6, 3) and np.array_equal(big[1:5, 1:5], np.repeat(np.repeat(want[1:3, 1:3], 2, 0), 2, 1))


def test_reference_special_values():
    """The rules the GPU cases rely on: NaN never wins the argmax and quantises to 0, a tie goes to the lowest index, values outside
    [0, 1] clamp, the lowest ground-truth row wins and an uncovered pixel is "none"."""
    assert R.quantise(np.array([np.nan, -1.0, 0.0, 0.5, 1.0, 7.0, np.inf, -np.inf], dtype=np.float32)).tolist() == [0, 0, 0, 128, 255, 255, 255, 0]
    assert R.quantise(np.float32(0.001)).tolist() == 0 and R.quantise(np.float32(0.002)).tolist() == 1      # 0.255 + 0.5, 0.51 + 0.5
    m = np.full((3, 2, 2), 0.25, dtype=np.float32)
    assert R.argmax_labels(m).tolist() == [[0, 0], [0, 0]]
    m[0] = np.nan
    assert R.argmax_labels(m).tolist() == [[1, 1], [1, 1]]
    m[:] = np.nan
    assert R.argmax_labels(m).tolist() == [[0, 0], [0, 0]]
    gt = np.zeros((3, 1, 2), dtype=np.uint8)
    gt[1, 0, 0], gt[2, 0, 0] = 1, 7
    assert R.gt_labels(gt).tolist() == [[1, -1]]
    pal = np.asarray(figures.PALETTE, dtype=np.uint8)
    assert np.array_equal(R.panel('gt', 0, 0, pal, gt=gt[None]), pal[[[1, 16]]])
    assert np.array_equal(R.panel('gt', 0, 0, pal, gt=gt[None], gt_colors=np.array([[5, 16, 3]], dtype=np.uint8)), pal[[[16, 16]]])
    # error: gain (|dx0| + |dx1| + |dx2|) / 3 = 4 * 0.3 / 3 = 0.4 -> 102; overlay edges: right / lower neighbour with another label
    x = np.zeros((1, 3, 1, 2), dtype=np.float32)
    p = np.full((1, 3, 1, 2), 0.1, dtype=np.float32)
    assert R.panel('error', 0, 0, pal, x=x, pred=p)[0, 0].tolist() == [102, 102, 102]
    mk = np.zeros((1, 2, 2, 2), dtype=np.float32)
    mk[0, 1, 1, 1] = 1.0                                                          # labels [[0, 0], [0, 1]]
    ov = R.panel('overlay', 0, 0, pal, x=np.ones((1, 3, 2, 2), dtype=np.float32), mask=mk, edge=(1, 2, 3), alpha=1.0)
    assert ov[0, 1].tolist() == [1, 2, 3] and ov[1, 0].tolist() == [1, 2, 3]
    assert ov[0, 0].tolist() == list(pal[0]) and ov[1, 1].tolist() == list(pal[1])         # alpha = 1: 0 * x + c / 255 -> c
    ov = R.panel('overlay', 0, 0, pal, x=np.ones((1, 3, 2, 2), dtype=np.float32), mask=mk, edges=False, alpha=0.0)
    assert ov.reshape(-1).tolist() == [255] * 12                                            # alpha = 0: the image


def test_layout_on_hand_numbers():
    H, W, boxes = figures.layout(2, ('image', 'pred', 'seg', 'slots'), K=3, S=8, scale=2, pad=2)
    assert (H, W) == (2 + 2 * 18, 2 + 6 * 18) and len(boxes) == 2 and len(boxes[0]) == 6
    assert boxes[0][0] == (2, 2, 16) and boxes[1][5] == (20, 92, 16)
    H, W, boxes = figures.layout(3, [('slot_mask', 1), 'error'], K=2, S=5, scale=1, pad=0)
    assert (H, W) == (15, 10) and boxes[2][1] == (10, 5, 5) and boxes[0][0] == (0, 0, 5)
    with pytest.raises(ValueError, match='unknown panel'):
        figures.layout(1, ('image', 'nonsense'), K=2, S=4)
    with pytest.raises(ValueError, match='slot index'):
        figures.layout(1, (('slot_mean', 2),), K=2, S=4)
    assert figures.expand_panels('slots', 2, 'mask') == [('slot_mask', 0), ('slot_mask', 1)]


def test_palette_invariants():
    assert len(figures.PALETTE) == 17 and all(len(c) == 3 and all(isinstance(v, int) and 0 <= v <= 255 for v in c) for c in figures.PALETTE)
    assert len(set(figures.PALETTE[:16])) == 16 and figures.PALETTE[16] not in figures.PALETTE[:16]
    r, g, b = figures.PALETTE[figures.NONE_COLOR]
    assert r == g == b and r < 96                                                 # a dark grey
    import iodine_amd
    assert iodine_amd.sheet is figures.sheet and iodine_amd.PALETTE is figures.PALETTE and iodine_amd.write_png is figures.write_png


def _chunks(png):
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    out, i = [], 8
    while i < len(png):
        n, = struct.unpack('>I', png[i:i + 4])
        tag, data = png[i + 4:i + 8], png[i + 8:i + 8 + n]
        crc, = struct.unpack('>I', png[i + 8 + n:i + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        out.append((tag, data))
        i += 12 + n
    assert i == len(png)
    return out


@pytest.mark.parametrize('shape', [(5, 7), (1, 1)])
def test_encode_png(shape, tmp_path):
    H, W = shape
    a = np.random.RandomState(3).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    png = figures.encode_png(a)
    chunks = _chunks(png)
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND'] and chunks[2][1] == b''
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)       # width, height, 8 bit, RGB, deflate, filter 0, no interlace
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(H, W, 3), a)
    assert figures.encode_png(torch.from_numpy(a)) == png                          # a tensor goes the same way
    path = tmp_path / 's.png'
    figures.write_png(str(path), a)
    assert path.read_bytes() == png
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(str(path)) as im:
            assert im.mode == 'RGB' and np.array_equal(np.asarray(im), a)
    with pytest.raises(ValueError, match='uint8'):
        figures.encode_png(a.astype(np.float32))


def _spec(**kw):
    sp = _lib.SheetSpec(rows=2, slots=3, n_gt=2, size=8, scale=2, pad=2, n_panels=3, draw_edges=1, alpha=0.5, error_gain=4.0)
    sp.panel_kind[0], sp.panel_kind[1], sp.panel_kind[2] = 0, 2, 6
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every one of these returns IODINE_ERR_INVALID before a launch: the pointers are never dereferenced on the host, so dummy non-null
    addresses stand in for device memory."""
    L = _lib.lib()
    p, null, st = C.c_void_p(4096), None, C.c_void_p(0)
    h, w = C.c_int(), C.c_int()

    def render(sp, x=p, pred=p, mask=p, mean=p, gt=p, sheet=p):
        return L.iodine_render_sheet(st, C.byref(sp) if sp is not None else None, x, pred, mask, mean, gt, null, null, sheet)

    assert L.iodine_sheet_size(C.byref(_spec()), C.byref(h), C.byref(w)) == 0
    assert (h.value, w.value) == figures.layout(2, ('image', 'seg', ('slot_masked', 0)), K=3, S=8, scale=2, pad=2)[:2] == (38, 56)
    bad = [dict(rows=0), dict(rows=-1), dict(slots=0), dict(slots=17), dict(n_gt=-1), dict(n_gt=17), dict(size=0), dict(size=1025),
           dict(scale=0), dict(scale=9), dict(pad=-1), dict(pad=17), dict(n_panels=0), dict(n_panels=65)]
    for kw in bad:
        assert render(_spec(**kw)) == INVALID, kw
        assert b'iodine_render_sheet' in L.iodine_last_error(None)
        assert L.iodine_sheet_size(C.byref(_spec(**kw)), C.byref(h), C.byref(w)) == INVALID, kw
        assert b'iodine_sheet_size' in L.iodine_last_error(None)
    sp = _spec()
    sp.panel_kind[1] = 9                                                          # unknown kind
    assert render(sp) == INVALID and b'unknown kind' in L.iodine_last_error(None)
    sp = _spec()
    sp.panel_slot[2] = 3                                                          # slot index K
    assert render(sp) == INVALID and b'slot 3' in L.iodine_last_error(None)
    sp.panel_slot[2] = 2
    sp.panel_slot[0] = 200                                                        # ignored by a kind that reads no slot
    assert L.iodine_sheet_size(C.byref(sp), C.byref(h), C.byref(w)) == 0
    assert render(None) == INVALID
    assert render(_spec(), mask=null) == INVALID and b'mask' in L.iodine_last_error(None)
    assert render(_spec(), sheet=null) == INVALID and b'sheet' in L.iodine_last_error(None)
    assert render(_spec(), x=null) == INVALID and b'needs x' in L.iodine_last_error(None)         # panel 0 = image
    assert render(_spec(), mean=null) == INVALID and b'needs mean' in L.iodine_last_error(None)   # panel 2 = slot_masked
    # every kind against its missing input: (kind, the pointer it needs)
    for kind, miss in ((1, 'pred'), (3, 'x'), (4, 'gt'), (5, 'x'), (5, 'pred'), (7, 'mean')):
        sp = _spec(n_panels=1)
        sp.panel_kind[0] = kind
        assert render(sp, **{miss: null}) == INVALID, (kind, miss)
    sp = _spec(n_panels=1, n_gt=0)
    sp.panel_kind[0] = 4                                                          # a gt panel without ground-truth rows
    assert render(sp) == INVALID
    assert L.iodine_sheet_size(None, C.byref(h), C.byref(w)) == INVALID and L.iodine_sheet_size(C.byref(_spec()), None, C.byref(w)) == INVALID
    # 32-bit indexing: 8192 x 8192 x 3 bytes per row of one panel; 10 rows fit below 2^31, 11 do not, nor does one row of 64 panels
    big = dict(size=1024, scale=8, pad=0, n_panels=1)
    assert L.iodine_sheet_size(C.byref(_spec(rows=10, **big)), C.byref(h), C.byref(w)) == 0 and (h.value, w.value) == (81920, 8192)
    assert L.iodine_sheet_size(C.byref(_spec(rows=11, **big)), C.byref(h), C.byref(w)) == INVALID
    assert render(_spec(rows=11, **big)) == INVALID and b'2^31' in L.iodine_last_error(None)
    sp = _spec(rows=1, size=1024, scale=8, pad=0, n_panels=64)
    assert render(sp) == INVALID
    assert L.iodine_sheet_form(C.byref(_spec(rows=0)), p, p, p, p, p, p) == -1
    # the form query is host arithmetic on the addresses: S = 8 and 16-byte aligned planes -> vector loads; W = 56 -> word stores
    assert L.iodine_sheet_form(C.byref(_spec()), p, p, p, p, p, p) == 3
    assert L.iodine_sheet_form(C.byref(_spec()), C.c_void_p(4100), p, p, p, p, p) == 2
    assert L.iodine_sheet_form(C.byref(_spec(n_panels=2)), p, p, p, p, p, p) == 1  # W = 2 + 2 * 18 = 38
    assert L.iodine_sheet_form(C.byref(_spec(size=5)), p, p, p, p, p, C.c_void_p(4097)) == 0


def test_python_layer_refuses_cpu_tensors_and_wrong_shapes():
    mask, mean, pred, x = torch.rand(2, 3, 1, 8, 8), torch.rand(2, 3, 3, 8, 8), torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        figures.sheet(mask, mean, pred, x)
    with pytest.raises(RuntimeError, match='ROCm device'):
        figures.sheet(mask, panels=('seg',))
    with pytest.raises(ValueError, match=r'mask must be \(\*, K, 1, S, S\)'):
        figures.sheet(mask[:, :, 0], mean, pred, x)
    with pytest.raises(ValueError, match='mean must be'):
        figures.sheet(mask, mean[:, :2], pred, x)
    with pytest.raises(ValueError, match='pred must be'):
        figures.sheet(mask, mean, pred[:1], x)
    with pytest.raises(ValueError, match='x must be'):
        figures.sheet(mask, mean, pred, x[:, :, :4])
    with pytest.raises(ValueError, match='gt must be uint8'):
        figures.sheet(mask, mean, pred, x, gt=torch.zeros(2, 2, 8, 8))
    with pytest.raises(ValueError, match='gt must be'):
        figures.sheet(mask, mean, pred, x, gt=torch.zeros(2, 2, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='needs mean'):
        figures.sheet(mask, None, pred, x)
    with pytest.raises(ValueError, match='needs gt'):
        figures.sheet(mask, mean, pred, x, panels=('gt',))
    with pytest.raises(ValueError, match='scale'):
        figures.sheet(mask, mean, pred, x, scale=9)
    with pytest.raises(ValueError, match='colors must be uint8'):
        figures.sheet(mask, mean, pred, x, colors=torch.zeros(2, 3))
    with pytest.raises(ValueError, match='K must be in'):
        figures.sheet(torch.rand(1, 17, 1, 4, 4), panels=('seg',))
    with pytest.raises(ValueError, match='torch tensor'):
        figures.sheet(np.zeros((1, 2, 1, 4, 4), dtype=np.float32))


def test_spec_struct_matches_header_and_abi_version():
    """_lib.SheetSpec declares the fields of iodine_sheet_spec in the header's order, the kind numbers are the header's, the three entries
    are exported and the ABI version is still 3 (the additions are additive)."""
    import re
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    body = header[header.index('typedef struct iodine_sheet_spec {'):header.index('} iodine_sheet_spec;')]
    fields = re.findall(r'^\s*(?:int|float|unsigned char)\s+([a-z_]+)(?:\[[A-Z_0-9]+\])?;', body, flags=re.M)
    assert fields == [f[0] for f in _lib.SheetSpec._fields_]
    for name, v in figures.KINDS.items():
        assert re.search(rf'#define IODINE_SHEET_{name.upper()} {v}\b', header), name
    assert C.sizeof(_lib.SheetSpec) == 8 * 4 + 5 * 4 + 6 + 128 + 51 + 3          # 237 bytes of fields, padded to the int alignment
    L = _lib.lib()
    for name in ('iodine_sheet_size', 'iodine_render_sheet', 'iodine_sheet_form'):
        assert name in _lib.EXPORTS and hasattr(L, name) and f'int {name}(' in header, name
    assert L.iodine_abi_version() == 3
    from iodine_amd import build
    assert 'kernels_sheet.hip' in build.SOURCES and 'iodine_sheet.cpp' in build.SOURCES
