"""Host-side checks of connected components (iodine_amd.objects.components, iodine_seg_components / iodine_seg_components_host): the numpy
reference against scipy, the serial host entry against the reference with exact equality of all six outputs over the pattern list, the
refusals the entry points make before they touch a device, the Python wrapper on CPU tensors, and properties of the rule.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import components_reference as R
from iodine_amd import _lib, objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID
SIZES = (1, 2, 3, 7, 16, 33, 64)
OUTPUTS = ('labels', 'area_map', 'count', 'per_slot', 'table', 'clean')


def host_components(seg, slots, connectivity, min_area, max_components):
    """iodine_seg_components_host on one numpy map -> dict of numpy outputs"""
    S = seg.shape[0]
    seg = np.ascontiguousarray(seg)
    out = dict(labels=np.full((S, S), 7, np.int32), area_map=np.full((S, S), 7, np.int32), count=np.full(4, 7, np.int32),
               per_slot=np.full((slots, 4), 7, np.int32), table=np.full((max_components, 8), 7, np.int32), clean=np.full((S, S), 7, np.uint8))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().iodine_seg_components_host(ptr(seg), slots, S, connectivity, min_area, max_components, ptr(out['labels']),
                                               ptr(out['area_map']), ptr(out['count']), ptr(out['per_slot']), ptr(out['table']),
                                               ptr(out['clean']))
    assert rc == 0, _lib.lib().iodine_last_error(None)
    return out


def assert_same(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        assert np.array_equal(g, want[k]), (what, k)


@pytest.mark.parametrize('connectivity', [4, 8])
def test_reference_numbers_like_scipy(connectivity):
    """scipy.ndimage.label per slot, an independent implementation: the same partition, the same numbering order within a slot (scipy
    numbers in raster order of the first pixel, the order the rule fixes), the same areas."""
    ndimage = pytest.importorskip('scipy.ndimage')
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    rng = np.random.default_rng(11)
    for S, K, smooth in ((9, 3, 0), (24, 4, 0), (40, 6, 3), (33, 16, 0)):
        seg = rng.integers(0, K, (S, S)).astype(np.uint8)
        for _ in range(smooth):                          # larger regions: each pixel takes the label above or to the left at random
            seg = np.where(rng.random((S, S)) < 0.5, np.roll(seg, 1, 0), np.roll(seg, 1, 1))
        seg[rng.random((S, S)) < 0.05] = R.INVALID
        comp, first, area, slot = R.partition(seg, K, connectivity)
        assert np.array_equal(comp < 0, seg >= K)
        assert np.all(np.diff(first) > 0) and int(area.sum()) == int((seg < K).sum())
        for k in range(K):
            lab, n = ndimage.label(seg == k, structure=structure)
            mine = np.flatnonzero(slot == k)             # this slot's components, in the reference's (global) order
            assert n == len(mine)
            for j, c in enumerate(mine):                 # scipy's j + 1 is the reference's j-th component of the slot
                assert np.array_equal(lab == j + 1, comp == c), (S, k, j)
                assert int((lab == j + 1).sum()) == int(area[c])


def test_reference_on_a_hand_computed_case():
    """4 x 4, two slots:   0 0 1 1      label 0 is one component of area 12 under both connectivities (everything joins through row 2).
                           0 1 0 0      4: label 1 is {2, 3}, {5} and {15}, numbered 1, 2, 3 after label 0's first pixel 0.
                           0 0 0 0      8: pixel 5 joins {2, 3} over the diagonal (area 3); pixel 15 stays alone, its three upper / left
                           0 0 0 1         neighbours are 0."""
    seg = np.array([[0, 0, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], np.uint8)
    r = R.components(seg, 2, 4, 1, 8)
    assert r['labels'].tolist() == [[0, 0, 1, 1], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 3]]
    assert r['count'].tolist() == [4, 0, 0, 0]
    # label 0: columns by row 0+1, 0+2+3, 0+1+2+3, 0+1+2 = 15; rows 2 * 0 + 3 * 1 + 4 * 2 + 3 * 3 = 20
    assert r['table'][0].tolist() == [0, 12, 15, 20, 0, 0, 3, 3]
    assert r['table'][1].tolist() == [1, 2, 5, 0, 2, 0, 3, 0] and r['table'][4].tolist() == [-1] * 8
    r = R.components(seg, 2, 8, 2, 8)
    assert r['count'].tolist() == [2, 1, 1, 0] and r['per_slot'].tolist() == [[1, 0, 12, 0], [1, 1, 3, 1]]
    assert r['labels'].tolist() == [[0, 0, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, -1]]
    assert r['clean'][3, 3] == 0 and r['area_map'][3, 3] == 1 and r['area_map'][1, 1] == 3
    r = R.components(seg, 1, 4, 1, 2)                                                                # label 1 is now invalid
    assert r['count'].tolist() == [1, 0, 0, 4] and r['labels'][0, 2] == -1 and r['area_map'][0, 2] == 0 and r['clean'][0, 2] == 1


def test_tie_speck_pattern_has_a_tie():
    """the pattern the tie rule is tested on: the speck's kept neighbours at min_area 9 are the two blocks of area 9, and the upper wins"""
    S = 16
    seg = R.pattern('specks', S)
    (r, c), = np.argwhere(seg == 12)
    e = R.expected('specks', S, 4, 9, 64)
    assert e['area_map'][r - 1, c] == 9 and e['area_map'][r + 1, c] == 9 and e['labels'][r - 1, c] >= 0 and e['labels'][r + 1, c] >= 0
    assert e['labels'][r, c - 1] == -1 and e['labels'][r, c + 1] == -1 and e['clean'][r, c] == 10
    (r, c), = np.argwhere(seg == 9)                      # enclosed by the ring of area 8: stays
    assert e['clean'][r, c] == 9 and e['clean'][r, c - 1] == 0


@pytest.mark.parametrize('S', SIZES)
@pytest.mark.parametrize('name', sorted(R.PATTERNS))
def test_host_entry_is_the_reference(name, S):
    seg = R.pattern(name, S)
    for connectivity in (4, 8):
        n_comp = len(R._partition_cached(name, S, connectivity)[1])
        for min_area in (1, 2, 9):
            for M in sorted({64, max(1, n_comp - 1), max(1, n_comp // 2)}):       # one of them below the component count
                got = host_components(seg, R.SLOTS, connectivity, min_area, M)
                assert_same(got, R.expected(name, S, connectivity, min_area, M), (name, S, connectivity, min_area, M))


def test_exports_and_constants():
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in ('iodine_seg_components', 'iodine_seg_components_host'):
        assert name in _lib.EXPORTS and hasattr(L, name) and f'int {name}(' in header, name
    assert 'iodine_seg_components_scratch_bytes' in _lib.EXPORTS and 'size_t iodine_seg_components_scratch_bytes(' in header
    assert L.iodine_abi_version() == 3
    assert int(re.search(r'#define IODINE_COMPONENTS_LDS_MAX_SIZE (\d+)', header).group(1)) == objects.COMPONENTS_LDS_MAX_SIZE >= 128
    assert len(objects.COMPONENT_COLUMNS) == 8 and len(objects.COUNT_COLUMNS) == 4 and len(objects.PER_SLOT_COLUMNS) == 4
    assert objects.Components._fields == ('labels', 'count', 'per_slot', 'table', 'area_map', 'clean')
    import iodine_amd
    assert iodine_amd.components is objects.components and iodine_amd.seg_to_mask is objects.seg_to_mask


def test_scratch_query_is_host_only():
    L = _lib.lib()
    q = L.iodine_seg_components_scratch_bytes
    assert q(0, 64) == 0 and q(1, 0) == 0 and q(1, 1025) == 0
    assert 0 < q(1, 1) < q(1, 64) < q(2, 64) < q(1, 1024) <= 32 << 20
    assert q(4, 128) >= 4 * 128 * 128 * 4                # at least the area of every pixel


def test_entry_points_refuse_bad_arguments_without_a_device():
    """IODINE_ERR_INVALID before a launch: dummy non-null addresses stand in for device memory and are never dereferenced."""
    L = _lib.lib()
    p, null, st = C.c_void_p(4096), None, C.c_void_p(0)
    big = 1 << 40

    def dev(seg=p, batch=1, slots=2, size=8, conn=4, min_area=1, M=4, labels=p, count=p, table=p, scratch=p, nbytes=big):
        return L.iodine_seg_components(st, seg, batch, slots, size, conn, min_area, M, labels, p, count, p, table, p, scratch, nbytes)

    def host(seg=p, slots=2, size=8, conn=4, min_area=1, M=4, labels=p, count=p, table=p):
        return L.iodine_seg_components_host(seg, slots, size, conn, min_area, M, labels, p, count, p, table, p)

    for f, who in ((dev, b'iodine_seg_components:'), (host, b'iodine_seg_components_host:')):
        for bad in (dict(seg=null), dict(labels=null), dict(count=null), dict(slots=0), dict(slots=17), dict(size=0), dict(size=1025),
                    dict(conn=6), dict(conn=0), dict(min_area=0), dict(min_area=-2), dict(M=0), dict(M=-1, table=null)):
            assert f(**bad) == INVALID, (who, bad)
            assert L.iodine_last_error(None).startswith(who), (who, bad, L.iodine_last_error(None))
    for bad in (dict(batch=0), dict(batch=-1), dict(scratch=null), dict(nbytes=L.iodine_seg_components_scratch_bytes(1, 8) - 1),
                dict(batch=2, nbytes=L.iodine_seg_components_scratch_bytes(1, 8))):
        assert dev(**bad) == INVALID, bad
        assert L.iodine_last_error(None).startswith(b'iodine_seg_components:'), bad
    assert b'scratch' in L.iodine_last_error(None)


def test_wrapper_refuses_bad_arguments():
    seg = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for bad in (dict(slots=0), dict(slots=17), dict(slots=2.5), dict(connectivity=6), dict(min_area=0), dict(max_components=-1),
                dict(slots=True)):
        kw = dict(slots=2)
        kw.update(bad)
        with pytest.raises(ValueError, match='components:'):
            objects.components(seg, **kw)
    for t in (seg.float(), torch.zeros(8, dtype=torch.uint8), torch.zeros(2, 8, 7, dtype=torch.uint8), torch.zeros(0, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='components:'):
            objects.components(t, 2)
    with pytest.raises(ValueError, match='components:'):
        objects.components(seg.numpy(), 2)
    with pytest.raises(ValueError, match='components:'):
        objects.clean_segmentation(seg, 2, 0)
    with pytest.raises(ValueError, match='seg_to_mask:'):
        objects.seg_to_mask(seg.float(), 2)
    with pytest.raises(ValueError, match='seg_to_mask:'):
        objects.seg_to_mask(seg, 17)


def test_wrapper_on_cpu_tensors_runs_the_host_entry_over_leading_dimensions():
    """(2, 3, S, S) on the CPU: every image equals the reference; a non-contiguous view gives the same; the optional outputs are None
    unless asked for."""
    S, names = 16, ('specks', 'random16_invalid', 'rings', 'checkerboard', 'corner_blocks', 'serpentine')
    seg = torch.from_numpy(np.stack([R.pattern(n, S) for n in names])).view(2, 3, S, S)
    got = objects.components(seg, R.SLOTS, connectivity=8, min_area=2, max_components=5, area_map=True, clean=True)
    assert isinstance(got, objects.Components) and got.labels.shape == (2, 3, S, S) and got.table.shape == (2, 3, 5, 8)
    assert got.count.shape == (2, 3, 4) and got.per_slot.shape == (2, 3, R.SLOTS, 4) and got.clean.dtype == torch.uint8
    for i, n in enumerate(names):
        assert_same({k: getattr(got, k)[i // 3, i % 3] for k in OUTPUTS}, R.expected(n, S, 8, 2, 5), n)
    plain = objects.components(seg, R.SLOTS, connectivity=8, min_area=2)
    assert plain.area_map is None and plain.clean is None and plain.table.shape == (2, 3, 64, 8) and torch.equal(plain.labels, got.labels)
    assert objects.components(seg, R.SLOTS, max_components=0).table is None
    wide = torch.zeros(2, 3, S, 2 * S, dtype=torch.uint8)
    wide[..., ::2] = seg
    again = objects.components(wide[..., ::2], R.SLOTS, connectivity=8, min_area=2, max_components=5, area_map=True, clean=True)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    assert torch.equal(objects.clean_segmentation(seg, R.SLOTS, 2, connectivity=8), got.clean)


def test_seg_to_mask_is_one_hot():
    seg = torch.from_numpy(np.stack([R.pattern('random16_invalid', 7), R.pattern('rings', 7)])).view(2, 1, 7, 7)
    m = objects.seg_to_mask(seg, 3)
    assert m.shape == (2, 1, 3, 1, 7, 7) and m.dtype == torch.float32
    for k in range(3):
        assert torch.equal(m[:, :, k, 0], (seg == k).float())
    assert torch.equal(m.sum(2)[:, :, 0], (seg < 3).float())


@pytest.mark.parametrize('connectivity', [4, 8])
def test_properties_of_the_rule(connectivity):
    """areas of all components sum to the valid pixel count; per_slot sums agree with count; after cleaning, every formerly kept region
    is still in one piece (its pixels keep their label and share one component of the cleaned map)."""
    S, slots, min_area = 33, 5, 4
    rng = np.random.default_rng(3)
    maps = []
    for i in range(4):
        seg = rng.integers(0, slots, (S, S)).astype(np.uint8)
        for _ in range(2 + i):
            seg = np.where(rng.random((S, S)) < 0.5, np.roll(seg, 1, 0), np.roll(seg, 1, 1))
        seg[rng.random((S, S)) < 0.03] = R.INVALID
        maps.append(seg)
    seg = torch.from_numpy(np.stack(maps))
    c = objects.components(seg, slots, connectivity=connectivity, min_area=min_area, max_components=2048, area_map=True, clean=True)
    valid = seg < slots
    assert torch.equal(c.count[:, 3], (~valid).sum((1, 2)).int())
    for b in range(len(maps)):
        kept = int(c.count[b, 0])
        assert kept <= 2048 and int(c.table[b, :kept, 1].sum()) + int(c.count[b, 2]) == int(valid[b].sum())
        assert int(c.labels[b].max()) == kept - 1
        firsts = [int(torch.nonzero(c.labels[b].reshape(-1) == i)[0]) for i in range(kept)]
        assert firsts == sorted(firsts)                                                  # numbered in raster order of the first pixel
    assert torch.equal(c.per_slot[..., 0].sum(1), c.count[:, 0]) and torch.equal(c.per_slot[..., 1].sum(1), c.count[:, 1])
    assert torch.equal(c.per_slot[..., 3].sum(1), c.count[:, 2])
    assert torch.equal((c.area_map >= min_area) & valid, c.labels >= 0) and torch.equal(c.area_map == 0, ~valid)
    again = objects.components(c.clean, slots, connectivity=connectivity, min_area=1, max_components=0)
    assert torch.equal(c.clean[c.labels >= 0], seg[c.labels >= 0]) and torch.equal(c.clean[~valid], seg[~valid])
    for b in range(len(maps)):
        for i in range(int(c.count[b, 0])):
            assert again.labels[b][c.labels[b] == i].unique().numel() == 1, (b, i)
    assert int(again.count[:, 2].sum()) == 0 and int(c.count[:, 2].sum()) > 0           # min_area 1: nothing is small; the maps had specks


def test_engine_flag():
    from iodine_amd import engine
    args = engine.make_parser().parse_args(['--metrics', '--min-component-area', '9'])
    assert args.min_component_area == 9 and engine.make_parser().parse_args([]).min_component_area == 0
    with pytest.raises(SystemExit, match='--metrics'):
        engine.main(['--min-component-area', '9'])
    with pytest.raises(ValueError, match='min_component_area'):
        engine.evaluate(None, [], 'cpu', min_component_area=-1)


def test_model_refuses_components_without_objects():
    from util import golden_setup, hip_arch, load_golden
    from iodine_amd import IODINE
    arch = golden_setup(load_golden('tiny'))[0]
    model = IODINE(hip_arch(arch))
    x = torch.zeros(1, 3, arch.img_size, arch.img_size)
    with pytest.raises(ValueError, match='objects=True'):
        model.reconstruct(x, components=True)
    with pytest.raises(ValueError, match='components= takes'):
        model.reconstruct(x, objects=True, components=dict(area=3))
