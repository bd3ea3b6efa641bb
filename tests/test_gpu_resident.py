"""Device-resident datasets on the GPU (iodine_amd.resident; iodine_batch_gather / iodine_synth_scenes): every comparison is bitwise -
the gather against the ToTensor arithmetic and pack_gt, the generated scenes against synth.make_images / engine.SyntheticClips, two training
steps and an evaluation against the same batches from make_dataloader.

Shapes: S = 16 takes the vector path (S * S % 4 == 0, four pixels per thread), S = 9 the scalar path (81 pixels); N = 5 with a repeated and
reversed index list; clips of F = 3 frames.  S = 24 for the scenes has 576 pixels: more than one pass of the 256 threads of a block."""
import numpy as np
import pytest
import torch

from iodine_amd import engine, matching, resident, synth
from iodine_amd.data import make_dataloader
from iodine_amd.matching import pack_gt
from iodine_amd.resident import ResidentDataset
from oracle import philox_oracle as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INDEX = [4, 2, 2, 0, 3, 1][::-1] + [4]                                       # reversed, with repeats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _u8_items(n, S, seed, frames=0):
    """n items as a loader would hand them over: (float image = u / 255, masks (G_i, S, S) - overlapping, G_i differs, item 1 unlabelled)"""
    g = torch.Generator().manual_seed(seed)
    lead = (frames,) if frames else ()
    items = []
    for i in range(n):
        u = torch.randint(0, 256, lead + (3, S, S), generator=g, dtype=torch.uint8)
        G = [3, 0, 16, 1, 2][i % 5]
        m = (torch.rand(lead + (G, S, S), generator=g) < 0.4).float() if G else None
        items.append((u.float().div_(255.0), m))
    return items


class _Items(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.mark.parametrize('S', [16, 9])
def test_gather_uint8_store_is_totensor_and_pack_gt_bitwise(S):
    items = _u8_items(5, S, seed=S)
    store = ResidentDataset.from_dataset(_Items(items), DEV)
    assert store.images.dtype == torch.uint8 and tuple(store.images.shape) == (5, S, S, 3) and store.planes == 16
    assert store.n_gt_host.tolist() == [3, 0, 16, 1, 2] and store.n_gt.cpu().tolist() == [3, 0, 16, 1, 2]
    x, gt, counts = store.gather(INDEX)
    assert x.dtype == torch.float32 and gt.dtype == torch.uint8 and x.device.type == 'cuda' and gt.device == x.device
    ref_x = torch.stack([items[i][0] for i in INDEX])
    ref_gt = pack_gt([items[i][1] for i in INDEX], S)
    assert torch.equal(_bits(x.cpu()), _bits(ref_x))
    assert tuple(gt.shape) == tuple(ref_gt.shape) and torch.equal(gt.cpu(), ref_gt)
    assert counts.tolist() == [store.n_gt_host[i] for i in INDEX]
    x2, gt2, _ = store.gather(torch.tensor([3, 4, 1]))                       # G follows the batch: max n_gt = 2
    assert tuple(gt2.shape) == (3, 2, S, S) and torch.equal(gt2.cpu(), pack_gt([items[i][1] for i in (3, 4, 1)], S))
    assert torch.equal(_bits(x2.cpu()), _bits(torch.stack([items[i][0] for i in (3, 4, 1)])))
    x3, gt3, c3 = store.gather([1])                                          # no mask in the batch: nothing to supervise
    assert gt3 is None and c3.tolist() == [0] and torch.equal(_bits(x3.cpu()), _bits(items[1][0][None]))


@pytest.mark.parametrize('S', [16, 9])
def test_gather_float32_store_copies_bitwise(S):
    ds = engine.SyntheticScenes(5, S, seed=3)
    items = [ds[i] for i in range(5)]
    store = ResidentDataset.from_dataset(ds, DEV)
    assert store.images.dtype == torch.float32 and store.image_kind == 1
    x, gt, counts = store.gather(INDEX)
    assert torch.equal(_bits(x.cpu()), _bits(torch.stack([items[i][0] for i in INDEX])))
    assert torch.equal(gt.cpu(), pack_gt([items[i][1] for i in INDEX], S))
    assert counts.tolist() == [items[i][1].shape[0] for i in INDEX]


@pytest.mark.parametrize('S', [16, 9])
def test_gather_clip_store(S):
    F = 3
    items = _u8_items(5, S, seed=100 + S, frames=F)
    store = ResidentDataset.from_dataset(_Items(items), DEV)
    assert store.frames == F and tuple(store.images.shape) == (5, F, S, S, 3) and tuple(store.masks.shape) == (5, F, S, S)
    x, gt, counts = store.gather(INDEX)
    assert tuple(x.shape) == (len(INDEX), F, 3, S, S)
    assert torch.equal(_bits(x.cpu()), _bits(torch.stack([items[i][0] for i in INDEX])))
    for f in range(F):                                                       # per frame: pack_gt of that frame's masks
        ref = pack_gt([None if items[i][1] is None else items[i][1][f] for i in INDEX], S)
        assert torch.equal(gt[:, f].cpu(), ref), f
    got = list(store.batches(2, shuffle=False))                              # the epoch iterator resolves frames like gather does
    assert [len(b[2]) for b in got] == [2, 2, 1]
    assert torch.equal(_bits(torch.cat([b[0] for b in got]).cpu()), _bits(torch.stack([it[0] for it in items])))
    assert torch.equal(got[1][1].cpu(), store.gather([2, 3])[1].cpu()) and got[1][2].tolist() == [16, 1]
    fstore = ResidentDataset.from_dataset(engine.SyntheticClips(4, S, F, seed=2), DEV)   # a float32 clip store
    clips = [engine.SyntheticClips(4, S, F, seed=2)[i] for i in range(4)]
    x, gt, _ = fstore.gather([3, 0, 3])
    assert torch.equal(_bits(x.cpu()), _bits(torch.stack([clips[i][0] for i in (3, 0, 3)])))
    for f in range(F):
        assert torch.equal(gt[:, f].cpu(), pack_gt([clips[i][1][f] for i in (3, 0, 3)], S))


def test_gather_refuses_indices_outside_the_store_before_any_launch():
    store = ResidentDataset.from_dataset(_Items(_u8_items(5, 16, seed=1)), DEV)
    for bad in ([-1], [5], [0, 5, 1], torch.tensor([2, -1])):
        with pytest.raises(ValueError, match='out of range'):
            store.gather(bad)
    with pytest.raises(ValueError):
        store.gather([])
    with pytest.raises(ValueError):
        store.gather([0.5])
    with pytest.raises(ValueError):
        store.gather([[0, 1]])
    torch.cuda.synchronize()
    x, _, _ = store.gather([0])                                              # the device is untouched by the refusals
    assert torch.isfinite(x).all()


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------------------
def _assert_scenes(store, imgs, masks, S):
    assert store.images.dtype == torch.float32 and torch.equal(_bits(store.images.cpu()), _bits(torch.from_numpy(np.ascontiguousarray(imgs))))
    assert store.n_gt_host.tolist() == [m.shape[0] for m in masks] and store.n_gt.cpu().tolist() == store.n_gt_host.tolist()
    ref = pack_gt(masks, S)
    got = resident.unpack_words(store.masks.cpu().numpy(), ref.shape[1])
    assert store.planes == ref.shape[1] and np.array_equal(got, ref.numpy())
    assert not (store.masks.cpu().numpy() >> np.uint16(ref.shape[1])).any()  # no bit beyond the planes


@pytest.mark.parametrize('S', [16, 24])
@pytest.mark.parametrize('max_objects', [3, 6])
def test_synthetic_blobs_are_make_images_bitwise(S, max_objects):
    n, seed = 7, 11
    per_item = [synth.make_images(1, S, seed=seed + i, kind='blobs', max_objects=max_objects) for i in range(n)]
    imgs = np.concatenate([p[0] for p in per_item])
    masks = [p[1][0] for p in per_item]
    store = ResidentDataset.synthetic(n, S, seed=seed, kind='blobs', max_objects=max_objects, device=DEV)
    _assert_scenes(store, imgs, masks, S)
    again = ResidentDataset.synthetic(n, S, seed=seed, kind='blobs', max_objects=max_objects, device=DEV)   # two calls: the same bits
    assert torch.equal(_bits(again.images), _bits(store.images)) and torch.equal(again.masks.view(torch.int16), store.masks.view(torch.int16))
    assert torch.equal(again.n_gt, store.n_gt)
    # a non-zero first index: items first .. first + n - 1 of the same data set ...
    part = ResidentDataset.synthetic(3, S, seed=seed, kind='blobs', max_objects=max_objects, device=DEV, first_index=2)
    _assert_scenes(part, imgs[2:5], masks[2:5], S)
    # ... and make_images' own first_index (one seed, the image index as the stream)
    bi, bm = synth.make_images(4, S, seed=seed, kind='blobs', max_objects=max_objects, first_index=5)
    im, mk, ng = resident.synth_scenes(4, S, seed=seed, kind='blobs', max_objects=max_objects, device=DEV, seed_step=0, stream=5, stream_step=1)
    _assert_scenes(ResidentDataset(im, mk, ng), bi, bm, S)
    if S == 16 and max_objects == 6:                                         # the default scenes are engine.SyntheticScenes' items
        ds = engine.SyntheticScenes(n, S, seed=seed)
        assert all(torch.equal(_bits(ds[i][0]), _bits(store.images[i].cpu())) for i in range(n))


@pytest.mark.parametrize('S', [16, 24])
def test_synthetic_uniform_is_make_images_bitwise(S):
    n, seed = 4, 5
    imgs = np.concatenate([synth.make_images(1, S, seed=seed + i, kind='uniform') for i in range(n)])
    store = ResidentDataset.synthetic(n, S, seed=seed, kind='uniform', device=DEV)
    assert store.masks is None and store.n_gt_host.tolist() == [0] * n and store.planes == 1
    assert torch.equal(_bits(store.images.cpu()), _bits(torch.from_numpy(imgs)))
    ref = synth.make_images(3, S, seed=seed, kind='uniform', first_index=2)
    im, mk, ng = resident.synth_scenes(3, S, seed=seed, kind='uniform', device=DEV, seed_step=0, stream=2, stream_step=1)
    assert mk is None and torch.equal(_bits(im.cpu()), _bits(torch.from_numpy(ref)))
    again = ResidentDataset.synthetic(n, S, seed=seed, kind='uniform', device=DEV)
    assert torch.equal(_bits(again.images), _bits(store.images))


@pytest.mark.parametrize('S', [16, 24])
def test_synthetic_clips_are_syntheticclips_bitwise(S):
    n, F, seed = 4, 3, 2
    ds = engine.SyntheticClips(n, S, F, seed=seed)
    store = ResidentDataset.synthetic(n, S, seed=seed, frames=F, device=DEV)
    assert store.frames == F and tuple(store.images.shape) == (n, F, 3, S, S) and tuple(store.masks.shape) == (n, F, S, S)
    for i in range(n):
        clip, masks = ds[i]
        assert torch.equal(_bits(store.images[i].cpu()), _bits(clip)), i
        assert store.n_gt_host[i] == masks.shape[1]
        got = resident.unpack_words(store.masks[i].cpu().numpy(), masks.shape[1])
        assert np.array_equal(got, masks.numpy().astype(np.uint8)), i
    x, gt, counts = store.gather([1, 3])
    assert torch.equal(_bits(x.cpu()), _bits(torch.stack([ds[1][0], ds[3][0]])))
    with pytest.raises(ValueError):
        ResidentDataset.synthetic(2, S, max_objects=17, device=DEV)
    with pytest.raises(ValueError):
        ResidentDataset.synthetic(2, S, kind='discs', device=DEV)


# ---- the engine from a store --------------------------------------------------------------------------------------------------------
def _tiny_model():
    from iodine_amd import IODINE
    from iodine_amd.optim import make_optimizer
    from oracle import iodine_oracle as O
    from util import hip_arch
    torch.manual_seed(0)
    m = IODINE(hip_arch(O.tiny_arch())).to(DEV)                              # tests/util.py's 'tiny': K = 3, T = 2, 16 x 16
    m.manual_seed(3)
    return m, make_optimizer(m, base_lr=3e-3)


def test_training_and_evaluation_from_a_store_equal_the_loader_bitwise():
    ds = engine.SyntheticScenes(8, 16)
    loader = make_dataloader(ds, batch_size=4, shuffle=False)
    store = ResidentDataset.synthetic(8, 16, device=DEV)
    runs = []
    for source in (loader, store.batches(4, shuffle=False)):
        m, opt = _tiny_model()
        lines = []
        losses = engine.train(m, opt, source, torch.device(DEV), 2, print_every=1, log=lines.append, mask_loss=1.0, mask_loss_kind='ce')
        ev = engine.evaluate(m, source, torch.device(DEV), evaluator=matching.SegmentationEvaluator())
        plain = engine.evaluate(m, source, torch.device(DEV))
        runs.append((losses, [p.detach().clone() for p in m.parameters()], [s.split('mask-loss: ')[1] for s in lines],
                     (ev.aris, ev.mious, ev.scs, ev.mscs, ev.global_mean, ev.global_means), plain.aris))
    (l0, p0, k0, e0, a0), (l1, p1, k1, e1, a1) = runs
    assert len(l0) == 2 and np.isfinite(l0).all() and l0 == l1
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(p0, p1))
    assert k0 == k1 and float(k0[0]) > 0.0                                   # the mask term was on, and equal
    assert len(e0[0]) == 8 and e0 == e1                                      # ARI, mIoU, SC, mSC per image and their means
    assert len(a0) == 8 and a0 == a1                                         # (a second evaluation draws new noise: compared run to run)


def test_engine_command_line_trains_and_evaluates_from_a_store(tmp_path, capsys):
    """--resident without a data set (scenes and clips generated on the device) and with a CLEVR folder (ingested, cached, loaded again)"""
    from PIL import Image
    engine.main(['--resident', '--steps', '2', '--batch', '4', '--metrics'])
    out = capsys.readouterr().out
    assert 'resident: 32 items of 64 x 64, float32 images' in out and 'Ari over all ranks' in out and 'mIoU' in out
    engine.main(['--resident', '--clip-frames', '6', '--steps', '1', '--batch', '2'])
    assert 'Ari over all ranks' in capsys.readouterr().out
    root = tmp_path / 'clevr'
    (root / 'images').mkdir(parents=True), (root / 'masks').mkdir()
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(root / 'images' / f'{i}.png')
        m = np.full((40, 56, 3), 64, dtype=np.uint8)
        m[5:20, 10 + i:30] = (255, 0, 0)
        m[15:35, 25:50] = (0, 0, 255)
        Image.fromarray(m).save(root / 'masks' / f'{i}.png')
    cache = str(tmp_path / 'cache.npz')
    argv = ['--config', 'clevr6', '--clevr', str(root), '--resident', cache, '--steps', '1', '--batch', '2']
    engine.main(argv)
    first = capsys.readouterr().out
    assert 'resident: wrote' in first and 'uint8 images' in first
    engine.main(argv)
    second = capsys.readouterr().out
    assert 'resident: loading' in second and 'resident: wrote' not in second
    line = lambda s: [ln for ln in s.splitlines() if ln.startswith('first loss')]
    assert line(first) == line(second) and len(line(first)) == 1             # the cache gives the same bits: the same run


# ---- epoch order on the device ------------------------------------------------------------------------------------------------------
def test_two_ranks_split_the_epoch_permutation():
    n, seed, epoch = 9, 6, 4
    store = ResidentDataset.synthetic(n, 16, device=DEV)
    keys = P.randn(n, seed, epoch)
    assert np.diff(np.sort(keys)).min() > 1e-4                               # no near-tie: the device's normals sort like the oracle's
    perm = np.argsort(keys, kind='stable').tolist()
    assert resident.epoch_order(n, seed, epoch, DEV).tolist() == perm and sorted(perm) == list(range(n))
    seen = []
    for rank in (0, 1):
        batches = store.batches(2, shuffle=True, seed=seed, epoch=epoch, rank=rank, world_size=2)
        mine = batches.order().tolist()
        got = list(batches)
        assert [len(b[2]) for b in got] == [2, 2, 1] and len(batches) == 3
        x = torch.cat([b[0] for b in got])
        assert torch.equal(_bits(x), _bits(store.images[torch.tensor(mine, device=DEV)]))
        assert np.concatenate([b[2] for b in got]).tolist() == store.n_gt_host[mine].tolist()
        seen.append(mine)
    wrapped = perm + perm[:1]                                                # 9 -> 10 entries: rank 1's last one is the wrap
    assert seen[0] == wrapped[0::2] and seen[1] == wrapped[1::2]
    assert set(seen[0]) & set(seen[1][:-1]) == set() and sorted(seen[0] + seen[1][:-1]) == list(range(n))
    again = store.batches(2, shuffle=True, seed=seed, epoch=epoch, rank=0, world_size=2)
    assert again.order().tolist() == seen[0]
    again.set_epoch(epoch + 1)
    assert again.order().tolist() != seen[0]
    dropped = list(store.batches(2, shuffle=True, seed=seed, epoch=epoch, rank=0, world_size=2, drop_last=True))
    assert [len(b[2]) for b in dropped] == [2, 2]
