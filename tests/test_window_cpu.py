"""Host side of windowed batches (iodine_amd.windows, tests/window_reference.py): the resampling rule against PIL, the window policies, the
--augment spec, the frame store's file and CLEVR ingestion.  No GPU: a store may live on the CPU for all of this."""
import os

import numpy as np
import pytest
import torch

import window_reference as R
from iodine_amd import _lib, data, engine, resident, synth, windows
from iodine_amd.windows import Augment, Center, FrameStore

H, W = 240, 320
PALETTE = np.array([data.CLEVR_BACKGROUND, (200, 10, 10), (10, 200, 10), (10, 10, 200), (250, 250, 0)], dtype=np.uint8)


def _frames():
    """a noise frame and an 8 x 8-blocky one, 240 x 320 uint8"""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    blocky = np.repeat(np.repeat(rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8), 8, axis=0), 8, axis=1)
    return {'noise': noise, 'blocky': blocky}


# ---- the rule against PIL -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [128, 64])
@pytest.mark.parametrize('kind', ['noise', 'blocky'])
def test_centre_crop_192_is_within_one_grey_level_of_pil(kind, size):
    """PIL rounds to 8 bits after each pass (1/2 + 1/2 level) and its coefficients are 22-bit fixed point: the 0.001"""
    pytest.importorskip('PIL')
    frame = _frames()[kind]
    row = Center(192).rows([0], H, W, size)[0]
    assert row.tolist() == [24, 64, 192, 192, 0, 1, 1, 1]
    got = R.window_image(frame, row, size)
    ref = data.clevr_image(frame, 192, size).numpy().astype(np.float64)
    err = np.abs(got - ref).max() * 255.0
    print(f'{kind} 192 -> {size}: max |delta| = {err:.6f} grey levels, mean {np.abs(got - ref).mean() * 255.0:.4f}')
    assert err <= 1.001


def test_centre_crop_at_scale_one_is_pil_bitwise():
    pytest.importorskip('PIL')
    for frame in _frames().values():
        got = R.window_image(frame, Center(128).rows([0], H, W, 128)[0], 128).astype(np.float32)
        ref = data.clevr_image(frame, 128, 128).numpy()
        assert np.array_equal(got.view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize('crop,size', [(192, 128), (192, 64), (96, 128), (240, 64)])
def test_nearest_rule_is_pil_nearest_on_a_label_image(crop, size):
    pytest.importorskip('PIL')
    rng = np.random.default_rng(3)
    labels = np.repeat(np.repeat(rng.integers(0, len(PALETTE), (H // 4, W // 4)), 4, axis=0), 4, axis=1)
    labels[::7, ::5] = rng.integers(0, len(PALETTE), labels[::7, ::5].shape)            # single pixels too
    mask_img = PALETTE[labels]
    ref = data.clevr_masks(mask_img, crop, size).numpy()
    lab, count = resident.separate_masks_fast(mask_img)
    assert count == ref.shape[0] == len(PALETTE) - 1
    words = resident.pack_words(resident.planes_from_labels(lab, count))
    got = R.unpack(R.window_words(words, Center(crop).rows([0], H, W, size)[0], size), count)
    assert np.array_equal(got, ref.astype(np.uint8))


def test_reference_properties_at_scale_one():
    """whole-pixel windows at scale 1 weigh {1, 0}: slices and mirrors, bit for bit; the flip mirrors image and words alike"""
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, (13, 22, 3), dtype=np.uint8)
    words = rng.integers(0, 1 << 16, (13, 22)).astype(np.uint16)
    full = (frame.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
    for flip in (0, 1):
        row = np.array([3, 5, 8, 8, flip, 1, 1, 1], dtype=np.float32)
        x = R.window_image(frame, row, 8).astype(np.float32)
        w = R.window_words(words, row, 8)
        ref_x, ref_w = full[:, 3:11, 5:13], words[3:11, 5:13]
        if flip:
            ref_x, ref_w = ref_x[:, :, ::-1], ref_w[:, ::-1]
        assert np.array_equal(x.view(np.int32), np.ascontiguousarray(ref_x).view(np.int32)) and np.array_equal(w, ref_w)
    first, count, weights, _ = R.axis_taps(0.25, 32.0, 40, 8)                  # scale 4, the widest: int(c + 4.5) - int(c - 3.5) = 8 taps
    assert count.tolist() == [6] + [8] * 6 + [7] and count.max() <= R.MAX_TAPS and np.allclose(weights.sum(axis=1), 1.0)


# ---- window policies ----------------------------------------------------------------------------------------------------------------
def test_vectorised_uniforms_equal_the_per_item_call():
    idx = [0, 1, 5, 123456, 2 ** 31 + 7]
    for seed, epoch in ((0, 0), (3, 2), (11, 40)):
        got = windows.item_uniforms(idx, seed, epoch)
        ref = np.stack([synth.uniform01(8, seed + 1000003 * epoch, stream=i) for i in idx])
        assert got.dtype == np.float64 and np.array_equal(got, ref)


def test_augment_rows_depend_on_seed_epoch_and_index_alone():
    aug = Augment(crop=192, scale=(0.7, 1), ratio=(0.8, 1.25), translate=8, flip=True, gain=0.1)
    idx = np.array([9, 2, 7, 2, 0, 31, 4, 18])
    rows = aug.rows(idx, H, W, 128, seed=5, epoch=3)
    assert rows.dtype == np.float32 and rows.shape == (8, 8)
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    assert np.array_equal(aug.rows(idx[perm], H, W, 128, seed=5, epoch=3), rows[perm])               # order
    assert np.array_equal(rows[1], rows[3])                                                          # the same item twice
    for r in (0, 1):                                                                                 # a split into two ranks
        assert np.array_equal(aug.rows(idx[r::2], H, W, 128, seed=5, epoch=3), rows[r::2])
    assert np.array_equal(aug.rows(idx[:3], H, W, 128, seed=5, epoch=3), rows[:3])                   # batch size
    assert not np.array_equal(aug.rows(idx, H, W, 128, seed=5, epoch=4), rows)
    assert not np.array_equal(aug.rows(idx, H, W, 128, seed=6, epoch=3), rows)
    assert set(rows[:, 4].tolist()) <= {0.0, 1.0} and (np.abs(rows[:, 5:8] - 1) <= 0.1 + 1e-6).all()
    ident = Augment().rows(idx, 16, 16, 16, seed=1, epoch=2)                                         # the defaults: the identity
    assert np.array_equal(ident, np.tile(np.array([0, 0, 16, 16, 0, 1, 1, 1], dtype=np.float32), (8, 1)))


@pytest.mark.parametrize('aug,size', [
    (Augment(crop=240, scale=(0.05, 1.0), ratio=(0.25, 4.0), translate='full', flip=True, gain=0.999), 128),
    (Augment(crop=240, scale=(1.0, 1.06), ratio=(1.0, 1.0), translate=1000.0), 64),
    (Augment(scale=(0.3, 1.0), ratio=(0.5, 2.0), translate=0.3), 120),
])
def test_every_window_lies_inside_the_frame(aug, size):
    rows = aug.rows(np.arange(1000), H, W, size, seed=2, epoch=1)
    d = rows.astype(np.float64)
    assert (d[:, 0] >= 0).all() and (d[:, 1] >= 0).all() and (d[:, 2] > 0).all() and (d[:, 3] > 0).all()
    assert (d[:, 0] + d[:, 2] <= H).all() and (d[:, 1] + d[:, 3] <= W).all()
    assert (d[:, 2] / size <= 4).all() and (d[:, 3] / size <= 4).all() and (d[:, 5:8] >= 0).all()
    windows.check_rows(rows, H, W, size)
    if aug.translate == 'full':
        assert d[:, 0].max() > 100 and d[:, 1].max() > 150                   # ... and they do move


def test_argument_refusals():
    with pytest.raises(ValueError, match='exceeds 4'):
        Augment(crop=240, scale=(1, 1.1)).rows([0], H, W, 64)                # 240 * 1.1 / 64 > 4
    with pytest.raises(ValueError, match='exceeds 4'):
        Center(240).rows([0], H, W, 32)
    Augment(crop=240).rows([0], H, W, 60)                                    # exactly 4 is allowed
    with pytest.raises(ValueError, match='larger than the 240 x 320 frame'):
        Augment(crop=241).rows([0], H, W, 128)
    with pytest.raises(ValueError, match='larger than'):
        Center(300).rows([0], H, W, 128)
    for bad in ((0, 1), (-1, 1), (1, 0.5)):
        with pytest.raises(ValueError, match='scale'):
            Augment(scale=bad)
    for bad in ((0, 1), (1, -2)):
        with pytest.raises(ValueError, match='ratio'):
            Augment(ratio=bad)
    for bad in (-0.1, 1.0, 2):
        with pytest.raises(ValueError, match=r'gain must be in \[0, 1\)'):
            Augment(gain=bad)
    with pytest.raises(ValueError, match='translate'):
        Augment(translate=-1)
    for bad in (0, 513, 2.5):
        with pytest.raises(ValueError, match=r'size must be an integer in 1\.\.512'):
            Augment().rows([0], H, W, bad)
        with pytest.raises(ValueError, match=r'size must be an integer in 1\.\.512'):
            Center().rows([0], H, W, bad)
    good = np.array([[0, 0, 16, 16, 0, 1, 1, 1]], dtype=np.float32)
    windows.check_rows(good, 16, 16, 16)
    for col, value in ((0, 0.5), (1, -1), (2, 0), (3, 17), (4, 0.5), (5, -0.1), (6, np.nan), (7, np.inf), (2, 65)):
        row = good.copy()
        row[0, col] = value
        with pytest.raises(ValueError, match='row 0'):
            windows.check_rows(row, 16 if col != 2 or value != 65 else 80, 16, 16)
    with pytest.raises(ValueError, match=r'float32 \(n, 8\)'):
        windows.check_rows(good.astype(np.float64), 16, 16, 16)


def test_augment_spec_parsing():
    assert engine.parse_augment('flip,scale=0.7:1,ratio=0.8:1.25,translate=8,gain=0.1') == {
        'flip': True, 'scale': (0.7, 1.0), 'ratio': (0.8, 1.25), 'translate': 8.0, 'gain': 0.1}
    assert engine.parse_augment('translate=full') == {'translate': 'full'}
    assert engine.parse_augment(' scale=0.5 , flip ') == {'scale': (0.5, 0.5), 'flip': True}
    Augment(**engine.parse_augment('flip,scale=0.7:1,gain=0.1'))
    for bad, word in (('rotate=3', 'unknown entry'), ('scale=a:b', 'cannot read'), ('flip=1', 'takes no value'), ('gain=0.1,gain=0.2', 'twice'),
                      ('scale=1:2:3', 'cannot read')):
        with pytest.raises(ValueError, match=word):
            engine.parse_augment(bad)
    args = engine.make_parser().parse_args(['--resident', '--augment', 'flip', '--native-frames', '--crop', '96'])
    assert args.augment == 'flip' and args.native_frames and args.crop == 96
    with pytest.raises(SystemExit, match='--resident'):
        engine.main(['--augment', 'flip'])


# ---- the frame store ----------------------------------------------------------------------------------------------------------------
def test_save_load_round_trips_bitwise(tmp_path):
    rng = np.random.default_rng(4)
    u8 = FrameStore(rng.integers(0, 256, (3, 6, 10, 3), dtype=np.uint8), rng.integers(0, 8, (3, 6, 10)).astype(np.uint16),
                    np.array([3, 0, 2], dtype=np.uint8))
    clips = FrameStore(rng.random((2, 4, 3, 5, 7), dtype=np.float32), None, np.zeros(2, dtype=np.uint8))
    assert (u8.image_kind, u8.frames, u8.height, u8.width, u8.planes, len(u8)) == (0, 0, 6, 10, 3, 3)
    assert (clips.image_kind, clips.frames, clips.height, clips.width, clips.planes) == (1, 4, 5, 7, 1)
    for name, store in (('u8', u8), ('clips', clips)):
        path = str(tmp_path / f'{name}.npz')
        store.save(path)
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == ({'images', 'masks', 'n_gt'} if store.masks is not None else {'images', 'n_gt'})
        back = FrameStore.load(path, 'cpu')
        assert back.images.dtype == store.images.dtype and torch.equal(back.images, store.images) and torch.equal(back.n_gt, store.n_gt)
        assert (back.masks is None) == (store.masks is None)
        if store.masks is not None:
            assert torch.equal(back.masks.view(torch.int16), store.masks.view(torch.int16))
        assert (back.planes, back.frames, back.height, back.width, back.image_kind) == (store.planes, store.frames, store.height,
                                                                                        store.width, store.image_kind)
    with pytest.raises(ValueError, match='uint16'):
        FrameStore(np.zeros((1, 4, 6, 3), dtype=np.uint8), np.zeros((1, 6, 4), dtype=np.uint16), np.zeros(1, dtype=np.uint8))
    with pytest.raises(ValueError, match='at most 16 masks'):
        FrameStore(np.zeros((1, 4, 6, 3), dtype=np.uint8), np.zeros((1, 4, 6), dtype=np.uint16), np.array([17], dtype=np.uint8))


def test_from_resident_wraps_without_copying():
    store = resident.ResidentDataset(np.zeros((4, 8, 8, 3), dtype=np.uint8), np.ones((4, 8, 8), dtype=np.uint16), np.ones(4, dtype=np.uint8))
    frames = FrameStore.from_resident(store)
    assert frames.images.data_ptr() == store.images.data_ptr() and frames.masks.data_ptr() == store.masks.data_ptr()
    assert (frames.height, frames.width, frames.planes, len(frames)) == (8, 8, 1, 4)
    b = frames.batches(3, 8, Center(), shuffle=False, rank=1, world_size=2)
    assert b.dataset is frames and b.sampler is b and len(b) == 1 and b.order().tolist() == [1, 3]
    b.set_epoch(4)
    assert b.epoch == 4
    with pytest.raises(ValueError, match='exceeds 4'):
        frames.batches(2, 1, Center())                                       # 8 / 1 > 4: refused when the iterator is made


def test_from_clevr_keeps_native_frames_and_packs_the_masks(tmp_path):
    pytest.importorskip('PIL')
    from PIL import Image
    root = tmp_path / 'clevr'
    os.makedirs(root / 'images'), os.makedirs(root / 'masks')
    rng = np.random.default_rng(0)
    imgs, mask_imgs = [], []
    for i in range(3):
        imgs.append(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8))
        Image.fromarray(imgs[-1]).save(root / 'images' / f'{i}.png')
        m = np.empty((24, 32, 3), dtype=np.uint8)
        m[:] = data.CLEVR_BACKGROUND
        m[2:10, 3 + i:12] = (200, 10, 10)
        m[8:20, 10:30 - i] = (10, 10, 200)
        mask_imgs.append(m)
        if i != 1:                                                           # frame 1 has no mask file
            Image.fromarray(m).save(root / 'masks' / f'{i}.png')
    store = FrameStore.from_clevr(data.CLEVR(str(root)), 'cpu')
    assert store.images.dtype == torch.uint8 and tuple(store.images.shape) == (3, 24, 32, 3) and tuple(store.masks.shape) == (3, 24, 32)
    assert store.n_gt_host.tolist() == [2, 0, 2] and store.planes == 2 and (store.height, store.width) == (24, 32)
    assert np.array_equal(store.images.numpy(), np.stack(imgs))
    for i in (0, 2):
        ref = data.clevr_separate_masks(mask_imgs[i]).astype(np.uint8)       # (2, 24, 32), sorted by colour
        assert np.array_equal(resident.unpack_words(store.masks[i].numpy(), 2), ref)
    assert not store.masks[1].numpy().any()
    m = np.zeros((24, 32, 3), dtype=np.uint8)
    m[0, :17, 0] = np.arange(1, 18)                                          # 17 colours + background (0, 0, 0) ... which is a colour too
    Image.fromarray(m).save(root / 'masks' / '1.png')
    with pytest.raises(ValueError, match='at most 16 masks'):
        FrameStore.from_clevr(data.CLEVR(str(root)), 'cpu')


def test_window_needs_a_rocm_device():
    store = FrameStore(np.zeros((2, 4, 4, 3), dtype=np.uint8), None, np.zeros(2, dtype=np.uint8))
    with pytest.raises(RuntimeError, match='ROCm device'):
        store.window([0], 4, Center())


def test_entry_is_declared_exported_and_refuses_bad_arguments_before_the_device():
    L = _lib.lib()
    assert 'iodine_batch_window' in _lib.EXPORTS and hasattr(L, 'iodine_batch_window')
    assert L.iodine_batch_window(None, None, 1, None, 0, None, 16, 16, None, 16, 1, None, None) == 1
    assert b'iodine_batch_window' in L.iodine_last_error(None)
