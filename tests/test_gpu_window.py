"""Windowed batches on the GPU (iodine_amd.windows; iodine_batch_window) against tests/window_reference.py, the rule in fp64.

Bitwise cases: at scale 1 with whole y0, x0 the taps weigh {1, 0}, so identity windows are ``ResidentDataset.gather`` and crops, shifts and
mirrors its slices, bit for bit (N = 5 frames of 16 x 16, both image kinds, overlapping mask bits, planes 1 / 3 / 16).

General cases: frames 13 x 22 (odd, W % 4 != 0: the byte path; the float32 store too), S = 7 and 8, 1 and 33 items, every window of
``_general_rows`` that fits - upsampling (h / S = 0.4), fractional origins, windows flush with each edge, unequal h / S and w / S, gains 0.5 /
1 / 1.5 on frames that hold 255 (the clamp).  h / S = 4 exactly does not fit a 13-row frame at S = 7 or 8 (it needs 28 rows): S = 3 is added
for it (h = w = 12), and ``test_wide_and_strided_paths`` runs it at S = 128 on 512-row frames, where a tile's source rows exceed the LDS stage
and the block works in several passes; the same test takes the dword path (W % 4 == 0), more than one row tile and, at S = 300, the second
column chunk.  The image bound 2e-6: two fp32 passes of at most 9 taps on values in [0, 1] (about 1.2e-6 worst case) against fp64; masks are
bitwise."""
import numpy as np
import pytest
import torch

import window_reference as R
from iodine_amd import _lib, engine, windows
from iodine_amd.resident import ResidentDataset
from iodine_amd.windows import Augment, Center, FrameStore

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 2e-6
INDEX = [4, 2, 2, 0, 3, 1][::-1] + [4]                                       # reversed, with repeats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _arrays(n, H, W, kind, planes, seed, frames=0):
    """n frames (clips with ``frames``) in the store's formats: images of ``kind``, words with overlapping bits below ``planes``"""
    rng = np.random.default_rng(seed)
    lead = (n, frames) if frames else (n,)
    u8 = rng.integers(0, 256, lead + (H, W, 3), dtype=np.uint8)
    u8[..., 0, 0, :] = 255                                                   # (the clamp is reached whatever the draw)
    images = u8 if kind == 0 else np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) / np.float32(255), -1, -3))
    masks = rng.integers(0, 1 << planes, lead + (H, W)).astype(np.uint16)
    return images, masks, np.full(n, planes, dtype=np.uint8)


def _rows(*rows):
    return np.array(rows, dtype=np.float32)


# ---- bitwise cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 3, 16])
@pytest.mark.parametrize('kind', [0, 1])
def test_whole_pixel_windows_at_scale_one_are_the_gather_bitwise(kind, planes):
    images, masks, n_gt = _arrays(5, 16, 16, kind, planes, seed=10 * kind + planes)
    store = ResidentDataset(images, masks, n_gt, device=DEV)
    frames = FrameStore.from_resident(store)
    assert frames.images.data_ptr() == store.images.data_ptr() and (frames.height, frames.width, frames.planes) == (16, 16, planes)
    x, gt, counts = store.gather(INDEX)
    for policy in (Center(), Augment(), np.tile(_rows([0, 0, 16, 16, 0, 1, 1, 1]), (len(INDEX), 1))):
        wx, wgt, wcounts = frames.window(INDEX, 16, policy, seed=3, epoch=1)
        assert wx.dtype == torch.float32 and wgt.dtype == torch.uint8 and tuple(wgt.shape) == (len(INDEX), planes, 16, 16)
        assert torch.equal(_bits(wx), _bits(x)) and torch.equal(wgt, gt) and wcounts.tolist() == counts.tolist()
    for y0, x0 in ((0, 0), (3, 5), (8, 8)):
        for flip in (0, 1):
            rows = np.tile(_rows([y0, x0, 8, 8, flip, 1, 1, 1]), (len(INDEX), 1))
            wx, wgt, _ = frames.window(INDEX, 8, rows)
            ref_x, ref_gt = x[..., y0:y0 + 8, x0:x0 + 8], gt[..., y0:y0 + 8, x0:x0 + 8]
            if flip:
                ref_x, ref_gt = ref_x.flip(-1), ref_gt.flip(-1)
            assert torch.equal(_bits(wx), _bits(ref_x)), (y0, x0, flip)
            assert torch.equal(wgt, ref_gt.contiguous()), (y0, x0, flip)


# ---- general cases ------------------------------------------------------------------------------------------------------------------
def _general_rows(H, W, S):
    """the windows of the general cases that fit an H x W frame at size S (``windows.check_rows`` decides)"""
    cand = [
        [1, W - 4 * S, 4 * S, 4 * S, 0, 1, 1, 1],                            # h / S = w / S = 4 exactly, flush right
        [3.3, 7.7, 0.4 * S, 0.4 * S, 1, 1, 1, 1],                            # upsampling, mirrored
        [1.25, 2.6, 1.3 * S, 1.7 * S, 0, 0.5, 1, 1.5],                       # fractional origin, unequal scales, gains
        [0, 0, S + 1.5, S + 4.25, 1, 1.5, 1.5, 0.5],                         # flush top and left
        [H - (S + 1.5), W - (S + 4.25), S + 1.5, S + 4.25, 0, 1, 1.5, 1],    # flush bottom and right
        [0, 0, H, W, 0, 1.5, 1, 0.5],                                        # the whole frame
        [2, 3, S, S, 1, 1, 1, 1],                                            # scale 1
        [0.5, 0.5, 0.75 * S, 2.5 * S, 0, 1, 1, 1],
    ]
    keep = []
    for row in cand:
        try:
            keep.append(windows.check_rows(_rows(row), H, W, S)[0])
        except ValueError:
            pass
    return np.stack(keep)


def _check_against_reference(frames, images, masks, index, rows, S):
    planes = frames.planes
    x, gt, _ = frames.window(index, S, rows)
    ref_x, ref_gt = R.window_batch(images, masks, index, rows, S, planes)
    err = float(np.abs(x.cpu().numpy().astype(np.float64) - ref_x).max())
    print(f'S = {S}, {len(index)} items, frames {tuple(images.shape[1:])}: max |delta| = {err:.3e}')
    assert np.array_equal(gt.cpu().numpy(), ref_gt)
    assert err <= TOL
    x2, gt2, _ = frames.window(index, S, rows)                               # two launches: the same bits
    assert torch.equal(_bits(x2), _bits(x)) and torch.equal(gt2, gt)
    return x


@pytest.fixture(scope='module')
def small_frames():
    return {kind: _arrays(4, 13, 22, kind, 5, seed=20 + kind) for kind in (0, 1)}


@pytest.mark.parametrize('count', [1, 33])
@pytest.mark.parametrize('S', [3, 7, 8])
@pytest.mark.parametrize('kind', [0, 1])
def test_general_windows_against_the_fp64_rule(small_frames, kind, S, count):
    images, masks, n_gt = small_frames[kind]
    frames = FrameStore(images, masks, n_gt, device=DEV)
    rows = _general_rows(13, 22, S)
    assert len(rows) >= 6 and (S != 3 or (rows[0, 2] == 12 and rows[0, 3] == 12))
    if count == 1:
        for k in range(len(rows)):                                           # every window once, alone in its launch
            _check_against_reference(frames, images, masks, [k % 4], rows[k:k + 1], S)
    else:
        index = [(3 * j + 1) % 4 for j in range(count)]
        x = _check_against_reference(frames, images, masks, index, rows[np.arange(count) % len(rows)], S)
        assert float(x.max()) == 1.0 and float(x.min()) >= 0.0               # the clamp was reached


@pytest.mark.parametrize('W', [132, 130])
def test_wide_and_strided_paths(W):
    """512-row frames: W = 132 takes the dword path, 130 the byte path.  At S = 128 the stage holds 32 source rows; a tile of 8 output rows
    at h / S = 4 needs 40 (at 16 rows, the tile of a large batch, 72): several passes per block, 16 row tiles.  S = 300 from a small window: 38
    row tiles, two column chunks (256 + 44)."""
    images, masks, n_gt = _arrays(2, 512, W, 0, 2, seed=W)
    frames = FrameStore(images, masks, n_gt, device=DEV)
    rows = _rows([0, 2, 512, 128, 0, 1, 1, 1], [0.5, W - 101.25, 511.5, 101.25, 1, 1, 1.5, 0.5], [100, 1, 128, 128, 0, 1, 1, 1])
    _check_against_reference(frames, images, masks, [1, 0, 1], rows, 128)
    _check_against_reference(frames, images, masks, [0], _rows([10.5, 20.25, 40, 33, 1, 1, 0.5, 1.5]), 300)


def test_all_frames_of_a_clip_share_their_items_window():
    F, S = 3, 8
    for kind in (0, 1):
        images, masks, n_gt = _arrays(4, 13, 22, kind, 3, seed=40 + kind, frames=F)
        frames = FrameStore(images, masks, n_gt, device=DEV)
        assert frames.frames == F
        index = [2, 0, 3, 2]
        rows = _general_rows(13, 22, S)[1:5]
        x, gt, counts = frames.window(index, S, rows)
        assert tuple(x.shape) == (4, F, 3, S, S) and tuple(gt.shape) == (4, F, 3, S, S) and counts.tolist() == [3] * 4
        for f in range(F):
            ref_x, ref_gt = R.window_batch(images[:, f], masks[:, f], index, rows, S, 3)
            assert np.abs(x[:, f].cpu().numpy().astype(np.float64) - ref_x).max() <= TOL, f
            assert np.array_equal(gt[:, f].cpu().numpy(), ref_gt), f
        got = list(frames.batches(3, S, Center(13), shuffle=False))          # the epoch iterator resolves frames like window does
        assert [tuple(b[0].shape) for b in got] == [(3, F, 3, S, S), (1, F, 3, S, S)]
        assert torch.equal(_bits(torch.cat([b[0] for b in got])), _bits(frames.window([0, 1, 2, 3], S, Center(13))[0]))


# ---- epochs -------------------------------------------------------------------------------------------------------------------------
def test_an_epoch_of_augmented_batches_is_a_function_of_seed_epoch_and_item():
    n, S = 8, 8
    images, masks, n_gt = _arrays(n, 13, 22, 0, 4, seed=50)
    frames = FrameStore(images, masks, n_gt, device=DEV)
    aug = Augment(crop=12, scale=(0.5, 1), ratio=(0.8, 1.25), translate='full', flip=True, gain=0.2)

    def items(batches):
        """index -> (x bits, gt) over one epoch"""
        order = batches.order().tolist()
        got = list(batches)
        assert len(got) == len(batches) and sum(len(b[2]) for b in got) == len(order)
        x, gt = torch.cat([b[0] for b in got]).cpu(), torch.cat([b[1] for b in got]).cpu()
        return order, {i: (_bits(x[k]), gt[k]) for k, i in enumerate(order)}

    b = frames.batches(3, S, aug, shuffle=True, seed=6, epoch=2)
    order, first = items(b)
    assert sorted(order) == list(range(n))
    _, again = items(frames.batches(3, S, aug, shuffle=True, seed=6, epoch=2))
    assert all(torch.equal(first[i][0], again[i][0]) and torch.equal(first[i][1], again[i][1]) for i in range(n))
    ref_x, ref_gt = R.window_batch(images, masks, order, aug.rows(order, 13, 22, S, 6, 2), S, 4)      # ... and it is the rule
    assert all(np.abs(first[i][0].view(torch.float32).numpy() - ref_x[k]).max() <= TOL and np.array_equal(first[i][1].numpy(), ref_gt[k])
               for k, i in enumerate(order))
    b.set_epoch(3)
    assert not np.array_equal(aug.rows(np.arange(n), 13, 22, S, 6, 3), aug.rows(np.arange(n), 13, 22, S, 6, 2))
    _, other = items(b)
    assert any(not torch.equal(first[i][0], other[i][0]) for i in range(n))
    seen = {}
    for rank in (0, 1):                                                      # two ranks: together the items of the one-rank epoch, bitwise
        shard_order, shard = items(frames.batches(3, S, aug, shuffle=True, seed=6, epoch=2, rank=rank, world_size=2))
        assert shard_order == order[rank::2] and not set(shard) & set(seen)
        seen.update(shard)
    assert sorted(seen) == list(range(n))
    assert all(torch.equal(first[i][0], seen[i][0]) and torch.equal(first[i][1], seen[i][1]) for i in range(n))


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_before_any_launch():
    images, masks, n_gt = _arrays(2, 13, 22, 0, 2, seed=60)
    frames = FrameStore(images, masks, n_gt, device=DEV)
    S = 8
    idx = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    rows = torch.from_numpy(np.tile(_rows([0, 0, 13, 22, 0, 1, 1, 1]), (2, 1))).to(DEV)
    x = torch.full((2, 3, S, S), -1.0, device=DEV)
    gt = torch.full((2, 2, S, S), 7, dtype=torch.uint8, device=DEV)
    L, p = _lib.lib(), _lib.ptr

    def call(index=idx, images=frames.images, src_h=13, src_w=22, win=rows, size=S, planes=2, out=x):
        return L.iodine_batch_window(_lib.stream(), p(index), 2, p(images), 0, p(frames.masks), src_h, src_w, p(win), size, planes, p(out), p(gt))

    for kw in (dict(win=None), dict(size=513), dict(planes=17), dict(src_h=0), dict(src_w=4097), dict(index=None), dict(images=None),
               dict(out=None), dict(size=0), dict(planes=0)):
        assert call(**kw) == 1, kw
        assert b'iodine_batch_window' in L.iodine_last_error(None), kw
    torch.cuda.synchronize()
    assert bool((x == -1.0).all()) and bool((gt == 7).all())                 # nothing was launched
    assert call() == 0
    ref_x, ref_gt = R.window_batch(images, masks, [1, 0], rows.cpu().numpy(), S, 2)
    assert np.abs(x.cpu().numpy() - ref_x).max() <= TOL and np.array_equal(gt.cpu().numpy(), ref_gt)
    for bad in ([2], [-1]):
        with pytest.raises(ValueError, match='out of range'):
            frames.window(bad, S, Center(13))
    with pytest.raises(ValueError, match='row 0'):
        frames.window([0], S, _rows([0, 0, 14, 22, 0, 1, 1, 1]))              # outside the frame: refused on the host
    with pytest.raises(ValueError, match='exceeds 4'):
        frames.window([0], 3, Center(13))


# ---- the engine from windows --------------------------------------------------------------------------------------------------------
def _tiny_model():
    from iodine_amd import IODINE
    from iodine_amd.optim import make_optimizer
    from oracle import iodine_oracle as O
    from util import hip_arch
    torch.manual_seed(0)
    m = IODINE(hip_arch(O.tiny_arch())).to(DEV)                              # tests/util.py's 'tiny': K = 3, T = 2, 16 x 16
    m.manual_seed(3)
    return m, make_optimizer(m, base_lr=3e-3)


def test_training_and_evaluation_from_windows():
    store = ResidentDataset.synthetic(8, 16, device=DEV)
    frames = FrameStore.from_resident(store)
    m, opt = _tiny_model()
    aug = Augment(flip=True, scale=(0.75, 1), translate=2, gain=0.1)
    losses = engine.train(m, opt, frames.batches(4, 16, aug, shuffle=True), torch.device(DEV), 1, log=lambda *a: None)
    assert len(losses) == 1 and np.isfinite(losses).all()
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    ev = engine.evaluate(m, frames.batches(4, 16, Center(), shuffle=False), torch.device(DEV))
    assert len(ev.aris) == 8 and np.isfinite(ev.aris).all() and np.isfinite(ev.global_mean)
    runs = []
    for source in (store.batches(4, shuffle=True, seed=2), frames.batches(4, 16, Augment(), shuffle=True, seed=2)):
        m, opt = _tiny_model()
        runs.append(engine.train(m, opt, source, torch.device(DEV), 1, log=lambda *a: None))
    assert np.isfinite(runs[0]).all() and runs[0] == runs[1]                 # the identity windows: the same step, bit for bit


def test_engine_command_line_trains_from_augmented_and_native_windows(tmp_path, capsys):
    from PIL import Image
    engine.main(['--resident', '--steps', '1', '--batch', '4', '--augment', 'flip,scale=0.7:1,ratio=0.8:1.25,translate=8,gain=0.1'])
    assert 'Ari over all ranks' in capsys.readouterr().out
    root = tmp_path / 'clevr'
    (root / 'images').mkdir(parents=True), (root / 'masks').mkdir()
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(root / 'images' / f'{i}.png')
        mk = np.full((40, 56, 3), 64, dtype=np.uint8)
        mk[5:20, 10 + i:30] = (255, 0, 0)
        mk[15:35, 25:50] = (0, 0, 255)
        Image.fromarray(mk).save(root / 'masks' / f'{i}.png')
    cache = str(tmp_path / 'native.npz')
    argv = ['--config', 'dsprites', '--clevr', str(root), '--resident', cache, '--native-frames', '--crop', '36', '--steps', '1', '--batch', '2']
    engine.main(argv)
    first = capsys.readouterr().out
    assert 'resident: wrote' in first and '2 frames of 40 x 56' in first and 'windows of 36 -> 64' in first
    engine.main(argv + ['--augment', 'flip,scale=0.8:1'])
    second = capsys.readouterr().out
    assert 'resident: loading' in second and 'Ari over all ranks' in second
