"""iodine_seg_components on the device: exact equality of all six outputs with the numpy reference (components_reference.py) and with the
serial host entry, over the pattern list, on both sides of the LDS form's size limit; determinism, input layouts, and the model's
``reconstruct(objects=True, components=...)``.  Everything is integer: every comparison is ``==``."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_reference as R
from iodine_amd import _lib, objects
from util import golden_setup, load_golden, make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LDS = objects.COMPONENTS_LDS_MAX_SIZE
SIZES = (1, 2, 3, 7, 16, 33, 64, 128, LDS, LDS + 1, 256)
OUTPUTS = ('labels', 'area_map', 'count', 'per_slot', 'table', 'clean')
NAMES = sorted(R.PATTERNS)


def host_components(seg, connectivity, min_area, M):
    """iodine_seg_components_host on one numpy map -> dict of numpy outputs"""
    S = seg.shape[0]
    seg = np.ascontiguousarray(seg)
    out = dict(labels=np.empty((S, S), np.int32), area_map=np.empty((S, S), np.int32), count=np.empty(4, np.int32),
               per_slot=np.empty((R.SLOTS, 4), np.int32), table=np.empty((M, 8), np.int32), clean=np.empty((S, S), np.uint8))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().iodine_seg_components_host(ptr(seg), R.SLOTS, S, connectivity, min_area, M, ptr(out['labels']), ptr(out['area_map']),
                                               ptr(out['count']), ptr(out['per_slot']), ptr(out['table']), ptr(out['clean']))
    assert rc == 0
    return out


def device_components(maps, connectivity, min_area, M):
    """``objects.components`` on the stacked numpy maps -> list of dicts of numpy outputs, one per map"""
    got = objects.components(torch.from_numpy(np.stack(maps)).to(DEV), R.SLOTS, connectivity=connectivity, min_area=min_area,
                             max_components=M, area_map=True, clean=True)
    assert all(t.device.type == 'cuda' for t in got)
    host = {k: getattr(got, k).cpu().numpy() for k in OUTPUTS}
    return [{k: host[k][i] for k in OUTPUTS} for i in range(len(maps))]


def assert_same(got, want, what):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('S', sorted(set(SIZES)))
def test_device_is_the_reference_and_the_host_entry(S, connectivity):
    """every pattern at this size, three maps a call; min_area 1 runs with a table of 5 rows (fewer than most patterns have components)"""
    for min_area, M in ((1, 5), (2, 64), (9, 64)):
        for i in range(0, len(NAMES), 3):
            names = NAMES[i:i + 3]
            got = device_components([R.pattern(n, S) for n in names], connectivity, min_area, M)
            for n, g in zip(names, got):
                what = (n, S, connectivity, min_area, M)
                assert_same(g, R.expected(n, S, connectivity, min_area, M), what)
                assert_same(g, host_components(R.pattern(n, S), connectivity, min_area, M), what + ('host',))


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name', ['one_label', 'serpentine'])
def test_largest_size(name, connectivity):
    """S = 1024, one map: the longest unions and the longest path the global form meets (256 tiles, indices up to 2^20)"""
    S = 1024
    for min_area, M in ((1, 5), (2, 64), (9, 64)):
        got, = device_components([R.pattern(name, S)], connectivity, min_area, M)
        assert_same(got, R.expected(name, S, connectivity, min_area, M), (name, connectivity, min_area))
    assert_same(got, host_components(R.pattern(name, S), connectivity, 9, 64), (name, connectivity, 'host'))


def _all_equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('S', [33, LDS, LDS + 1])
def test_two_calls_and_a_side_stream_give_the_same_bits(S):
    seg = torch.from_numpy(np.stack([R.pattern(n, S) for n in ('random16_invalid', 'specks', 'tile_crosser', 'checkerboard')])).to(DEV)
    kw = dict(connectivity=8, min_area=3, max_components=40, area_map=True, clean=True)
    first = objects.components(seg, R.SLOTS, **kw)
    assert _all_equal(objects.components(seg, R.SLOTS, **kw), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = objects.components(seg, R.SLOTS, **kw)
    side.synchronize()
    assert _all_equal(other, first)
    # without the optional outputs: the same labels, counts and table
    plain = objects.components(seg, R.SLOTS, connectivity=8, min_area=3, max_components=40)
    assert plain.area_map is None and plain.clean is None and _all_equal(plain[:4], first[:4])
    bare = objects.components(seg, R.SLOTS, connectivity=8, min_area=3, max_components=0)
    assert bare.table is None and _all_equal(bare[:3], first[:3])
    assert torch.equal(objects.clean_segmentation(seg, R.SLOTS, 3, connectivity=8), first.clean)


def test_input_layouts():
    """a non-contiguous seg and leading dimensions (T + 1, B, ...): the results of the plain batch, reshaped; a CPU tensor gives the same"""
    S = 33
    maps = np.stack([R.pattern(n, S) for n in ('random16_invalid', 'specks', 'rings', 'corner_blocks', 'serpentine', 'random16')])
    seg = torch.from_numpy(maps).to(DEV)
    kw = dict(connectivity=4, min_area=2, max_components=16, area_map=True, clean=True)
    flat = objects.components(seg, R.SLOTS, **kw)
    lead = objects.components(seg.view(3, 2, S, S), R.SLOTS, **kw)
    assert lead.labels.shape == (3, 2, S, S) and lead.table.shape == (3, 2, 16, 8) and lead.count.shape == (3, 2, 4)
    assert lead.per_slot.shape == (3, 2, R.SLOTS, 4) and lead.clean.shape == (3, 2, S, S)
    assert all(torch.equal(a.reshape(b.shape), b) for a, b in zip(lead, flat))
    wide = torch.zeros(6, S, 2 * S, dtype=torch.uint8, device=DEV)
    wide[..., ::2] = seg
    assert not wide[..., ::2].is_contiguous() and _all_equal(objects.components(wide[..., ::2], R.SLOTS, **kw), flat)
    on_cpu = objects.components(seg.cpu(), R.SLOTS, **kw)
    assert all(t.device.type == 'cpu' for t in on_cpu) and all(torch.equal(a, b.cpu()) for a, b in zip(on_cpu, flat))
    with pytest.raises(ValueError, match='components:'):
        objects.components(seg, 17)


# ---- the module: reconstruct(objects=True, components=...) ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny():
    g = load_golden('tiny')
    arch, params, x, eps, _ = golden_setup(g)
    assert x.shape[0] >= 2
    return arch, make_hip_model(arch, params), x[:2].to(DEV), eps[:, :2].contiguous().to(DEV)


OPTIONS = dict(connectivity=8, min_area=3, max_components=12, clean=True)


def test_reconstruct_components(tiny):
    arch, m, x, eps = tiny
    K = arch.slots
    plain = m.reconstruct(x, eps, False, None, False, None, True)          # the signature before the keyword, objects=True
    before = {k: v.clone() for k, v in m.objects.items()}
    assert set(before) == {'table', 'segmentation', 'kl'}
    outs = m.reconstruct(x, eps, objects=True, components=OPTIONS)
    assert all(torch.equal(a, b) for a, b in zip(plain, outs))
    assert set(m.objects) == {'table', 'segmentation', 'kl', 'components'}
    assert all(torch.equal(before[k], m.objects[k]) for k in before)
    got = m.objects['components']
    assert isinstance(got, objects.Components) and got.area_map is None and got.clean is not None and got.table.shape == (2, 12, 8)
    assert _all_equal(got, objects.components(m.objects['segmentation'], K, **OPTIONS))
    ref = R.components(m.objects['segmentation'][0].cpu().numpy(), K, 8, 3, 12)
    assert np.array_equal(got.labels[0].cpu().numpy(), ref['labels']) and np.array_equal(got.clean[0].cpu().numpy(), ref['clean'])
    assert np.array_equal(got.table[0].cpu().numpy(), ref['table']) and np.array_equal(got.count[0].cpu().numpy(), ref['count'])
    m.reconstruct(x, eps, objects=True, components=True)                     # the defaults
    assert _all_equal(m.objects['components'], objects.components(m.objects['segmentation'], K))
    # without the keyword: the bits and the keys of before
    again = m.reconstruct(x, eps, objects=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)) and set(m.objects) == {'table', 'segmentation', 'kl'}
    assert all(torch.equal(before[k], m.objects[k]) for k in before)
    m.reconstruct(x, eps)
    assert m.objects is None
    with pytest.raises(ValueError, match='objects=True'):
        m.reconstruct(x, eps, components=True)


def test_reconstruct_components_with_trajectory(tiny):
    arch, m, x, eps = tiny
    K, S, T = arch.slots, arch.img_size, arch.iters
    m.reconstruct(x, eps, trajectory=True, objects=True, components=OPTIONS)
    tr, ob = m.trajectory['components'], m.objects['components']
    assert tr.labels.shape == (T + 1, 2, S, S) and tr.table.shape == (T + 1, 2, 12, 8) and tr.count.shape == (T + 1, 2, 4)
    assert _all_equal(tr, objects.components(m.trajectory['segmentation'], K, **OPTIONS))
    assert _all_equal(type(tr)(*(None if t is None else t[T] for t in tr)), ob)
    assert _all_equal(ob, objects.components(m.objects['segmentation'], K, **OPTIONS))
    m.reconstruct(x, eps, trajectory=True, objects=True)
    assert 'components' not in m.trajectory and 'components' not in m.objects


def test_reconstruct_components_chunked(tiny):
    arch, m, x, eps = tiny
    m.reconstruct(x, eps, objects=True, components=OPTIONS)
    whole = m.objects['components']
    m.set_option('batch_cap', 1)
    try:
        m.reconstruct(x, eps, objects=True, components=OPTIONS)
        chunked = m.objects['components']
    finally:
        m.set_option('batch_cap', 0)
    assert _all_equal(chunked, whole)


def test_evaluate_with_min_component_area():
    """engine.evaluate(min_component_area=N): the raw scores are those of an evaluation without it; at N = 1 nothing is small, so the cleaned
    maps are the argmax maps and score exactly like them; at N = 4 the extra means are in range"""
    from iodine_amd import IODINE, engine, matching
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    dl = make_dataloader(engine.SyntheticScenes(8, 16), batch_size=4, shuffle=False)
    runs = []
    for kw in ({}, dict(min_component_area=1), dict(min_component_area=4)):
        m.manual_seed(3)
        runs.append(engine.evaluate(m, dl, torch.device(DEV), evaluator=matching.SegmentationEvaluator(), **kw))
    plain, one, four = runs
    assert not hasattr(plain, 'cleaned')
    for ev in (one, four):
        assert ev.aris == plain.aris and ev.mious == plain.mious and ev.global_means == plain.global_means
        assert set(ev.cleaned) == {'components_per_slot', 'small_pixel_share', 'aris', 'mious', 'scs', 'mscs'}
        assert ev.cleaned['components_per_slot'] >= 1.0 and 0.0 <= ev.cleaned['small_pixel_share'] <= 1.0
    assert one.cleaned['small_pixel_share'] == 0.0
    assert all(one.cleaned[k] == plain.global_means[k] for k in ('aris', 'mious', 'scs', 'mscs'))
    assert all(0.0 <= four.cleaned[k] <= 1.0 for k in ('mious', 'scs', 'mscs'))
    with pytest.raises(ValueError, match='min_component_area'):
        engine.evaluate(m, dl, torch.device(DEV), min_component_area=-1)


def test_cleaned_map_goes_where_a_mask_goes(tiny):
    """seg_to_mask(clean) through slot_table and segmentation_scores: hard areas are the cleaned map's pixel counts, and the scores against
    the cleaned map itself as ground truth are perfect"""
    from iodine_amd import matching
    arch, m, x, eps = tiny
    K, S = arch.slots, arch.img_size
    m.reconstruct(x, eps, objects=True, components=dict(min_area=4, clean=True))
    clean = m.objects['components'].clean
    mask = objects.seg_to_mask(clean, K)
    assert mask.shape == (2, K, 1, S, S) and mask.dtype == torch.float32
    table, seg = objects.slot_table(mask, segmentation=True)
    assert torch.equal(seg, clean)
    counts = torch.stack([(clean == k).sum((1, 2)) for k in range(K)], 1)
    assert torch.equal(table[..., objects.SLOT_COLUMNS.index('hard_area')].long(), counts)
    gt = mask[:, :, 0].to(torch.uint8)                                     # (B, K, S, S); a slot without pixels is a padding row
    s = matching.segmentation_scores(mask, gt)
    assert s.miou.tolist() == [1.0, 1.0] and s.sc.tolist() == [1.0, 1.0] and s.msc.tolist() == [1.0, 1.0]
