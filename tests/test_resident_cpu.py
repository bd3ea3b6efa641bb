"""Host side of the device-resident datasets (iodine_amd.resident): ingestion against data.CLEVR + pack_gt, the bit-word masks, the cache
file, the epoch order's sharding, and the two C-ABI entries in header and library.  No GPU: a store may live on the CPU for all of this."""
import os
import re
import subprocess
import shutil

import numpy as np
import pytest
import torch

from iodine_amd import _lib, data, engine, resident
from iodine_amd.matching import pack_gt
from iodine_amd.resident import ResidentDataset
from oracle import philox_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 56
COLOURS = [(200, 10, 10), (10, 200, 10), (10, 10, 200)]                     # sorted order: blue, green, red
N_IMAGES = 3


def _mask_frame(i):
    """background + three colours; the red rectangle sits in the top-left corner, outside the 24-pixel centre crop (rows 8..31, columns
    16..39); blue and green lie inside and move with i"""
    m = np.empty((H, W, 3), dtype=np.uint8)
    m[:] = data.CLEVR_BACKGROUND
    m[0:5, 0:9] = COLOURS[0]
    m[10 + i:20 + i, 18:27] = COLOURS[1]
    m[15:28, 25 + i:37 + i] = COLOURS[2]
    return m


@pytest.fixture(scope='module')
def clevr_root(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp('clevr')
    os.makedirs(root / 'images'), os.makedirs(root / 'masks')
    rng = np.random.default_rng(0)
    for i in range(N_IMAGES):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / 'images' / f'{i}.png')
        if i != 1:                                                           # image 1 has no mask file
            Image.fromarray(_mask_frame(i)).save(root / 'masks' / f'{i}.png')
    return str(root)


class _Plain(torch.utils.data.Dataset):
    """the same items through the generic ingestion path (not an instance of data.CLEVR)"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        return self.ds[i]


def _check_against_items(arrays, items, size):
    assert arrays['images'].dtype == np.uint8 and arrays['images'].shape == (len(items), size, size, 3)
    assert arrays['masks'].dtype == np.uint16 and arrays['n_gt'].dtype == np.uint8
    for i, (img, mask) in enumerate(items):
        x = torch.from_numpy(arrays['images'][i]).permute(2, 0, 1).float().div_(255.0)
        assert torch.equal(x.view(torch.int32), img.view(torch.int32)), i
        assert arrays['n_gt'][i] == (0 if mask is None else mask.shape[0])
    gt = pack_gt([m for _, m in items], size)
    planes = max(1, int(arrays['n_gt'].max()))
    assert gt.shape[1] == planes
    assert np.array_equal(resident.unpack_words(arrays['masks'], planes), gt.numpy())


def test_clevr_ingestion_equals_the_loader_items(clevr_root):
    ds = data.CLEVR(clevr_root)
    items = [ds[i] for i in range(len(ds))]
    assert [None if m is None else m.shape[0] for _, m in items] == [3, None, 3]
    fast = resident.ingest(ds)
    _check_against_items(fast, items, 128)
    plain = resident.ingest(_Plain(ds))                                      # the generic path gives the same arrays
    for k in fast:
        assert np.array_equal(fast[k], plain[k]) and fast[k].dtype == plain[k].dtype, k
    two = resident.ingest(ds, workers=2)                                     # ... and so do worker processes
    for k in fast:
        assert np.array_equal(fast[k], two[k]), k


def test_a_colour_outside_the_centre_crop_keeps_its_row(clevr_root):
    """crop 24 -> 16: the red plane is empty after the crop but still counts (data.clevr_masks keeps it), in clevr_separate_masks' order"""
    from PIL import Image
    ds = data.CLEVR(clevr_root)
    items = []
    for path in ds.img_paths:
        img = data.clevr_image(np.asarray(Image.open(path).convert('RGB')), 24, 16)
        mp = os.path.join(clevr_root, 'masks', os.path.basename(path))
        items.append((img, data.clevr_masks(np.asarray(Image.open(mp).convert('RGB')), 24, 16) if os.path.exists(mp) else None))
    assert items[0][1].shape == (3, 16, 16) and items[0][1][2].sum() == 0 and items[0][1][0].sum() > 0 and items[0][1][1].sum() > 0
    arrays = resident.ingest(ds, crop=24, size=16)
    _check_against_items(arrays, items, 16)
    assert arrays['n_gt'].tolist() == [3, 0, 3] and not (arrays['masks'] & 4).any() and not arrays['masks'][1].any()


def test_fast_colour_separation_equals_clevr_separate_masks():
    rng = np.random.default_rng(1)
    palette = np.array([data.CLEVR_BACKGROUND, (0, 0, 1), (0, 1, 0), (1, 0, 0), (255, 255, 255), (64, 64, 65), (63, 255, 0), (64, 0, 255)],
                       dtype=np.uint8)
    frames = [_mask_frame(0), palette[rng.integers(0, len(palette), (H, W))], np.full((5, 7, 3), 64, dtype=np.uint8),
              palette[rng.integers(1, 4, (6, 6))]]                           # the last one has no background pixel
    for m in frames:
        ref = data.clevr_separate_masks(m)
        labels, count = resident.separate_masks_fast(m)
        got = resident.planes_from_labels(labels, count)
        assert count == ref.shape[0] and got.shape == ref.shape and np.array_equal(got, ref)


def test_bit_words_unpack_to_the_planes_and_overlaps_are_exact():
    a = np.zeros((8, 8), dtype=np.float32); a[1:6, 1:6] = 1
    b = np.zeros((8, 8), dtype=np.float32); b[4:8, 3:8] = 0.5              # overlaps a; non-zero = inside
    planes = np.stack([a, b])
    words = resident.pack_words(planes)
    assert words.dtype == np.uint16 and set(np.unique(words)) == {0, 1, 2, 3}
    assert np.array_equal(resident.unpack_words(words, 2), (planes != 0).astype(np.uint8))
    assert np.array_equal(resident.unpack_words(words, 3)[2], np.zeros((8, 8), dtype=np.uint8))
    full = np.ones((16, 4, 4), dtype=np.uint8)
    assert (resident.pack_words(full) == 0xFFFF).all()

    class Two(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return torch.zeros(3, 8, 8), torch.from_numpy(planes)
    arrays = resident.ingest(Two())
    assert np.array_equal(resident.unpack_words(arrays['masks'], 2)[0], pack_gt([planes]).numpy()[0]) and arrays['n_gt'].tolist() == [2]


def test_seventeen_masks_are_refused():
    with pytest.raises(ValueError, match='at most 16 masks'):
        resident.pack_words(np.ones((17, 4, 4), dtype=np.uint8))

    class Many(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return torch.zeros(3, 4, 4), torch.ones(17, 4, 4)
    with pytest.raises(ValueError, match='at most 16 masks'):
        ResidentDataset.from_dataset(Many(), 'cpu')
    with pytest.raises(ValueError, match='at most 16 masks'):
        ResidentDataset(np.zeros((1, 4, 4, 3), dtype=np.uint8), np.zeros((1, 4, 4), dtype=np.uint16), np.array([17], dtype=np.uint8))


def test_save_load_round_trips_bitwise(clevr_root, tmp_path):
    for name, ds in (('u8', data.CLEVR(clevr_root)), ('f32', engine.SyntheticScenes(3, 16)), ('clips', engine.SyntheticClips(2, 16, 3))):
        store = ResidentDataset.from_dataset(ds, 'cpu')
        path = str(tmp_path / f'{name}.npz')
        store.save(path)
        with np.load(path, allow_pickle=False) as z:                         # plain arrays, readable without pickle
            assert set(z.files) == {'images', 'masks', 'n_gt'}
        back = ResidentDataset.load(path, 'cpu')
        assert back.images.dtype == store.images.dtype and torch.equal(back.images, store.images)
        assert torch.equal(back.masks.view(torch.int16), store.masks.view(torch.int16)) and torch.equal(back.n_gt, store.n_gt)
        assert (back.planes, back.frames, back.size, back.image_kind) == (store.planes, store.frames, store.size, store.image_kind)
    assert (store.frames, store.image_kind) == (3, 1) and tuple(store.images.shape) == (2, 3, 3, 16, 16) and tuple(store.masks.shape) == (2, 3, 16, 16)
    unlabelled = ResidentDataset(np.zeros((2, 4, 4, 3), dtype=np.uint8), None, np.zeros(2, dtype=np.uint8))
    unlabelled.save(str(tmp_path / 'none.npz'))
    assert ResidentDataset.load(str(tmp_path / 'none.npz'), 'cpu').masks is None and unlabelled.planes == 1


def test_a_float_image_that_is_not_eight_bit_turns_the_store_float32():
    k255 = torch.arange(48, dtype=torch.float32).reshape(3, 4, 4).div_(255.0)
    other = k255.clone(); other[0, 0, 0] = 0.3                               # 0.3 * 255 = 76.5: no k / 255

    class Items(torch.utils.data.Dataset):
        def __init__(self, items):
            self.items = items

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i], None
    a = resident.ingest(Items([k255, k255 * 0 + 1.0]))
    assert a['images'].dtype == np.uint8 and a['masks'] is None and a['n_gt'].tolist() == [0, 0]
    assert np.array_equal(a['images'][0], np.arange(48, dtype=np.uint8).reshape(3, 4, 4).transpose(1, 2, 0))
    b = resident.ingest(Items([k255, other, k255]))
    assert b['images'].dtype == np.float32 and b['images'].shape == (3, 3, 4, 4)
    for got, ref in zip(b['images'], (k255, other, k255)):
        assert np.array_equal(got.view(np.int32), ref.numpy().view(np.int32))
    c = resident.ingest(engine.SyntheticScenes(2, 16))                       # the synthetic scenes are not 8-bit (background 0.25)
    assert c['images'].dtype == np.float32 and c['masks'].dtype == np.uint16
    imgs, masks = zip(*[engine.SyntheticScenes(2, 16)[i] for i in range(2)])
    assert np.array_equal(c['images'], torch.stack(imgs).numpy())
    assert np.array_equal(resident.unpack_words(c['masks'], int(c['n_gt'].max())), pack_gt(masks).numpy())


def test_gather_and_generation_need_a_rocm_device():
    store = ResidentDataset(np.zeros((2, 4, 4, 3), dtype=np.uint8), None, np.zeros(2, dtype=np.uint8))
    with pytest.raises(RuntimeError, match='ROCm device'):
        store.gather([0])
    with pytest.raises(RuntimeError, match='ROCm device'):
        resident.synth_scenes(1, 8, device='cpu')
    with pytest.raises(RuntimeError, match='ROCm device'):
        resident.epoch_order(4, 0, 0, 'cpu')


# ---- epoch order --------------------------------------------------------------------------------------------------------------------
def _order(n, seed, epoch):
    """numpy restatement of resident.epoch_order on the Philox oracle: the stable argsort of the epoch's normals"""
    return np.argsort(P.randn(n, seed, epoch), kind='stable')


def test_shards_cover_the_wrapped_epoch_order_once():
    n, world = 10, 3
    order = _order(n, seed=4, epoch=2)
    assert sorted(order.tolist()) == list(range(n))
    shards = [resident.shard_order(order, r, world).tolist() for r in range(world)]
    assert [len(s) for s in shards] == [4, 4, 4]
    wrapped = order.tolist() + order.tolist()[:2]                            # padded by wrapping round to a multiple of 3
    assert [shards[i % world][i // world] for i in range(12)] == wrapped
    assert sorted(sum(shards, [])) == sorted(wrapped)
    assert np.array_equal(_order(n, 4, 2), order)                            # the same (seed, epoch): the same order
    assert not np.array_equal(_order(n, 4, 3), order) and not np.array_equal(_order(n, 5, 2), order)
    assert resident.shard_order(order, 0, 1).tolist() == order.tolist()
    assert resident.shard_order([0, 1], 2, 5).tolist() == [0] and resident.shard_order([0, 1], 1, 5).tolist() == [1]   # wraps more than once
    with pytest.raises(ValueError):
        resident.shard_order(order, 3, 3)


def test_batches_object_has_the_loader_attributes_the_engine_reads():
    store = ResidentDataset(np.zeros((10, 4, 4, 3), dtype=np.uint8), None, np.zeros(10, dtype=np.uint8))
    b = store.batches(4, shuffle=False, rank=1, world_size=3)
    assert b.dataset is store and len(b.dataset) == 10 and b.sampler is b and len(b) == 1
    assert b.order().tolist() == [1, 4, 7, 0]
    b.set_epoch(5)
    assert b.epoch == 5 and len(store.batches(4, shuffle=False)) == 3 and len(store.batches(4, shuffle=False, drop_last=True)) == 2
    with pytest.raises(ValueError):
        store.batches(0)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_entries_and_the_library_exports_them():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    L = _lib.lib()
    for name in ('iodine_batch_gather', 'iodine_synth_scenes'):
        assert re.search(r'\bint ' + name + r'\(void\* stream,', header), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    nm = shutil.which('nm')
    if nm:
        out = subprocess.run([nm, '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert ' T iodine_batch_gather' in out and ' T iodine_synth_scenes' in out
    # bad arguments are refused in words before anything touches a device
    assert L.iodine_batch_gather(None, None, 1, None, 0, None, 16, 1, None, None) == 1
    assert b'iodine_batch_gather' in L.iodine_last_error(None)
    assert L.iodine_synth_scenes(None, 1, 16, 0, 1, 0, 0, 1, 17, 0, None, None, None) == 1
    assert b'iodine_synth_scenes' in L.iodine_last_error(None)
