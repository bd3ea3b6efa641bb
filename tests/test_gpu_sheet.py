"""iodine_amd.figures on the device against the float32 numpy restatement in tests/sheet_reference.py.

Equality is exact everywhere: the sheet's arithmetic is defined operation by operation in float32 (include/iodine_hip.h,
iodine_render_sheet), so the reference gives the same bytes and no tolerance applies.  Every sheet is rendered twice, into a buffer
pre-filled with 0x5A and into one pre-filled with 0xA5, and both must equal the reference: a byte the kernel leaves unwritten differs
from the reference in at least one of the two, and the two calls are bitwise equal."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import sheet_reference as R
from iodine_amd import figures, matching, objects
from util import golden_setup, load_golden, make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD_VALUE = (7, 200, 33)

# (R, K, G, S, scale, pad) -> the forms the kernel takes (bit 0: 16-byte loads, bit 1: word stores), worked out from the rule in the
# header: loads need S % 4 == 0, stores W % 4 == 0 with W = pad + C (S scale + pad), C = 8 panels without ground truth and 9 with it.
#   (1, 1, 0, 8, 1, 0):    W = 64                    both vector forms, no padding at all
#   (3, 3, 2, 5, 3, 1):    W = 1 + 9 * 16 = 145      both scalar forms: odd S, odd width
#   (2, 16, 16, 16, 1, 2): W = 2 + 9 * 18 = 164      both vector forms; panel origins at 6 + 54 c bytes: runs start and end inside a word
#   (2, 7, 3, 23, 2, 2):   W = 2 + 9 * 48 = 434      both scalar forms, replication by 2
#   (2, 7, 0, 128, 2, 2):  W = 2 + 8 * 258 = 2066    vector loads, byte stores; four bands of 32 source rows per panel
CASES = {(1, 1, 0, 8, 1, 0): 3, (3, 3, 2, 5, 3, 1): 0, (2, 16, 16, 16, 1, 2): 3, (2, 7, 3, 23, 2, 2): 0, (2, 7, 0, 128, 2, 2): 1}
SPECIAL = {(3, 3, 2, 5, 3, 1): 'tie', (2, 16, 16, 16, 1, 2): 'nan', (2, 7, 3, 23, 2, 2): 'nan'}


def _panels(K, G):
    return (['image', 'pred', 'seg', 'overlay'] + (['gt'] if G else []) +
            ['error', ('slot_masked', K - 1), ('slot_mean', 0), ('slot_mask', K // 2)])


def _inputs(case):
    """Seeded planes: mask a softmax over K, x / pred in [0, 1], mean in [-1, 2] (outside [0, 1] on purpose), gt random overlapping
    rows with uncovered pixels, colours a random map.  'tie': slots 0 and 1 are two equal constant planes above the rest everywhere;
    'nan': the last slot's mask plane and channel 1 of the mean of slot 0 are NaN, and so is a corner of x."""
    Rr, K, G, S, _, _ = case
    g = torch.Generator().manual_seed(1000 * K + 10 * S + G)
    mask = torch.softmax(2.0 * torch.randn(Rr, K, 1, S, S, generator=g), dim=1)
    x, pred = torch.rand(Rr, 3, S, S, generator=g), torch.rand(Rr, 3, S, S, generator=g)
    mean = torch.rand(Rr, K, 3, S, S, generator=g) * 3.0 - 1.0
    gt = (torch.rand(Rr, G, S, S, generator=g) < 0.3).to(torch.uint8) * 3 if G else None      # any non-zero byte counts
    colors = torch.randint(0, 17, (Rr, K), generator=g, dtype=torch.int64).to(torch.uint8)
    gt_colors = torch.randint(0, 17, (Rr, G), generator=g, dtype=torch.int64).to(torch.uint8) if G else None
    kind = SPECIAL.get(case)
    if kind == 'tie':
        mask[:, :2] = 0.45
        mask[:, 2:] = 0.1
    if kind == 'nan':
        mask[:, K - 1] = float('nan')
        mean[:, 0, 1] = float('nan')
        x[:, :, 0, 0] = float('nan')
    return dict(mask=mask, x=x, pred=pred, mean=mean, gt=gt, colors=colors, gt_colors=gt_colors)


def _reference(case, t, **kw):
    _, K, G, _, scale, pad = case
    a = {k: (None if v is None else v.numpy()) for k, v in t.items()}
    return R.sheet(figures.expand_panels(_panels(K, G), K), figures.PALETTE, a['mask'][:, :, 0], scale=scale, pad=pad, pad_value=PAD_VALUE,
                   x=a['x'], pred=a['pred'], mean=a['mean'], gt=a['gt'], colors=a['colors'], gt_colors=a['gt_colors'], **kw)


def _render(case, t, fill, **kw):
    """(sheet rendered into a pre-filled buffer, form bits)"""
    _, K, G, _, scale, pad = case
    d = {k: (None if v is None else v.to(DEV)) for k, v in t.items()}
    sp, tensors, _ = figures._prepare(d['mask'], d['mean'], d['pred'], d['x'], d['gt'], _panels(K, G), 'masked', scale, pad, PAD_VALUE,
                                      kw.get('background', (1., 1., 1.)), kw.get('alpha', 0.5), kw.get('edges', True),
                                      kw.get('edge', (255, 255, 255)), kw.get('error_gain', 4.0), d['colors'], d['gt_colors'])
    H, W, _ = figures.layout(case[0], _panels(K, G), K, case[3], scale, pad)
    out = torch.full((H, W, 3), fill, dtype=torch.uint8, device=DEV)
    form = figures.sheet_form(out, sp, tensors)
    figures.render_into(out, sp, tensors)
    return out.cpu().numpy(), form


@pytest.mark.parametrize('case', list(CASES), ids=lambda c: 'R{}K{}G{}S{}z{}p{}'.format(*c))
def test_bytes_equal_the_reference(case):
    t = _inputs(case)
    Rr, K, G, S, scale, pad = case
    # the reference treats the planted inputs the way the header says: the tie goes to slot 0, a NaN plane never wins and quantises to 0
    lab = R.argmax_labels(t['mask'][0, :, 0].numpy())
    if SPECIAL.get(case) == 'tie':
        assert not lab.any()
    if SPECIAL.get(case) == 'nan':
        assert (lab != K - 1).all() and not R.quantise(t['mean'][0, 0, 1].numpy()).any()
    assert float(t['mean'].nan_to_num().min()) < 0.0 and float(t['mean'].nan_to_num().max()) > 1.0
    kw = dict(background=(0.25, 1.0, 0.0), alpha=0.375, edge=(1, 2, 3), error_gain=2.5)
    want = _reference(case, t, **kw)
    got_a, form = _render(case, t, 0x5A, **kw)
    got_b, _ = _render(case, t, 0xA5, **kw)
    print(f'case {case}: form {form}, sheet {want.shape}')
    assert form == CASES[case]
    assert got_a.shape == want.shape and got_a.dtype == np.uint8
    assert np.array_equal(got_a, want), f'{int((got_a != want).sum())} bytes differ'
    assert np.array_equal(got_b, want)
    # every padding pixel is pad_value (none keeps the fill)
    H, W, boxes = figures.layout(Rr, _panels(K, G), K, S, scale, pad)
    inside = np.zeros((H, W), dtype=bool)
    for row in boxes:
        for y0, x0, side in row:
            inside[y0:y0 + side, x0:x0 + side] = True
    assert int((~inside).sum()) == H * W - Rr * len(boxes[0]) * (S * scale) ** 2
    assert (got_a[~inside] == np.asarray(PAD_VALUE, dtype=np.uint8)).all()
    # the public call gives the same sheet
    d = {k: (None if v is None else v.to(DEV)) for k, v in t.items()}
    pub = figures.sheet(d['mask'], d['mean'], d['pred'], d['x'], d['gt'], panels=_panels(K, G), scale=scale, pad=pad, pad_value=PAD_VALUE,
                        edges=True, colors=d['colors'], gt_colors=d['gt_colors'], **kw)
    assert pub.dtype == torch.uint8 and pub.device.type == 'cuda' and np.array_equal(pub.cpu().numpy(), want)


def test_forms_are_covered_and_a_misaligned_plane_takes_scalar_loads():
    """Between them the cases run both forms of the loads and of the stores; an x that starts 4 bytes off a 16-byte boundary sends the
    whole launch to element loads (with word stores: the fourth combination) and changes no byte.  Edges off and identity colours too."""
    assert {f & 1 for f in CASES.values()} == {0, 1} and {f & 2 for f in CASES.values()} == {0, 2}
    case = (2, 16, 16, 16, 1, 2)
    t = _inputs(case)
    t['colors'], t['gt_colors'] = None, None
    want = _reference(case, t, edges=False)
    got, form = _render(case, t, 0x5A, edges=False)
    assert form == 3 and np.array_equal(got, want)
    d = {k: (None if v is None else v.to(DEV)) for k, v in t.items()}
    flat = torch.empty(d['x'].numel() + 1, dtype=torch.float32, device=DEV)
    x_off = flat[1:].view(d['x'].shape)
    x_off.copy_(d['x'])
    assert x_off.data_ptr() % 16 == 4 and x_off.is_contiguous()
    sp, tensors, _ = figures._prepare(d['mask'], d['mean'], d['pred'], x_off, d['gt'], _panels(16, 16), 'masked', 1, 2, PAD_VALUE,
                                      (1., 1., 1.), 0.5, False, (255, 255, 255), 4.0, None, None)
    out = torch.full(want.shape, 0x5A, dtype=torch.uint8, device=DEV)
    assert figures.sheet_form(out, sp, tensors) == 2
    assert np.array_equal(figures.render_into(out, sp, tensors).cpu().numpy(), want)


def test_seg_panel_is_slot_table_segmentation_through_the_palette():
    t = _inputs((2, 7, 3, 23, 2, 2))
    mask = t['mask'].to(DEV)
    seg = objects.slot_table(mask, segmentation=True)[1]                       # (2, 23, 23) uint8
    got = figures.sheet(mask, panels=('seg',), pad=0)                           # rows stacked: (46, 23, 3)
    pal = torch.tensor(figures.PALETTE, dtype=torch.uint8, device=DEV)
    assert torch.equal(got, pal[seg.reshape(-1, 23).long()])
    lead = figures.sheet(mask.reshape(2, 1, 7, 1, 23, 23), panels=('seg',), pad=0)                # any leading dimensions
    assert torch.equal(lead, got)


def test_matched_colors_make_seg_and_gt_panels_equal():
    """Masks that are a permutation of one-hot ground truth: every pixel belongs to one real row g and to the slot perm[g], so under
    matched colours the two panels are byte-equal.  Row 2 is padding (no pixels) and takes 16; the two slots no row is assigned to take the
    lowest indices no real row uses, 2 and 4, in slot order."""
    Rr, K, S = 3, 5, 12
    g = torch.Generator().manual_seed(5)
    part = torch.randint(0, 3, (Rr, S, S), generator=g)
    rows = [0, 1, 3]                                                            # the ground-truth row of segment 0, 1, 2
    gt = torch.zeros(Rr, 4, S, S, dtype=torch.uint8)
    mask = torch.zeros(Rr, K, 1, S, S)
    perms = [torch.randperm(K, generator=g)[:3].tolist() for _ in range(Rr)]
    for r in range(Rr):
        for i, row in enumerate(rows):
            gt[r, row] = (part[r] == i).to(torch.uint8)
            mask[r, perms[r][i], 0] = (part[r] == i).float()
    mask, gt = mask.to(DEV), gt.to(DEV)
    colors, gt_colors = figures.matched_colors(mask, gt)
    assert colors.dtype == gt_colors.dtype == torch.uint8 and colors.shape == (Rr, K) and gt_colors.shape == (Rr, 4)
    assert gt_colors.tolist() == [[0, 1, 16, 3]] * Rr
    for r in range(Rr):
        c = colors[r].tolist()
        assert [c[perms[r][i]] for i in range(3)] == rows
        assert [c[k] for k in range(K) if k not in perms[r]] == [2, 4]
    out = figures.sheet(mask, gt=gt, panels=('seg', 'gt'), pad=1, colors=colors, gt_colors=gt_colors)
    _, _, boxes = figures.layout(Rr, ('seg', 'gt'), K, S, 1, 1)
    for r in range(Rr):
        (ya, xa, side), (yb, xb, _) = boxes[r]
        assert torch.equal(out[ya:ya + side, xa:xa + side], out[yb:yb + side, xb:xb + side])
    assert len({tuple(p) for p in out[boxes[0][0][0]:boxes[0][0][0] + S, 1:1 + S].reshape(-1, 3).tolist()}) == 3


def _tiny():
    arch, params, x, _, _ = golden_setup(load_golden('tiny'))
    m = make_hip_model(arch, params, DEV)
    m.manual_seed(11)
    return arch, m, x.to(DEV)


def test_decomposition_and_trajectory_sheet_on_tiny():
    arch, m, x = _tiny()
    K, S, T, n = arch.slots, arch.img_size, arch.iters, 2
    eps = torch.randn(T + 1, n, K, arch.dim_latent, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = figures.decomposition(m, x, n=n, eps=eps, scale=2)
    H, W, boxes = figures.layout(n, ('image', 'pred', 'seg', 'slots'), K, S, 2, 2)
    assert tuple(out.shape) == (H, W, 3) and out.dtype == torch.uint8 and len(boxes[0]) == 3 + K
    pred, mask, mean = m.reconstruct(x[:n], eps=eps)
    for r in range(n):
        y0, x0, side = boxes[r][1]
        want = np.repeat(np.repeat(R.quantise(pred[r].cpu().numpy()).transpose(1, 2, 0), 2, 0), 2, 1)
        assert np.array_equal(out[y0:y0 + side, x0:x0 + side].cpu().numpy(), want)
    assert torch.equal(out, figures.sheet(mask, mean, pred, x[:n], scale=2))
    # the refinement figure: row j is the sheet of trajectory entry j
    m.reconstruct(x[:n], eps=eps, trajectory=True)
    tr = {k: v.clone() for k, v in m.trajectory.items()}
    ts = figures.trajectory_sheet(tr, image=1, x=x)
    H, W, boxes = figures.layout(T + 1, ('image', 'pred', 'seg', 'slots'), K, S, 1, 2)
    assert tuple(ts.shape) == (H, W, 3)
    for j in range(T + 1):
        one = figures.sheet(tr['mask'][j, 1:2], tr['mean'][j, 1:2], tr['pred'][j, 1:2], x[1:2])
        y0 = boxes[j][0][0]
        assert torch.equal(ts[y0:y0 + S], one[2:2 + S]), j
    assert torch.equal(ts[boxes[T][0][0]:boxes[T][0][0] + S], figures.sheet(mask[1:2], mean[1:2], pred[1:2], x[1:2])[2:2 + S])   # entry T = the final decode
    # decomposition(trajectory=b) runs image b alone; without x the image panel is dropped
    dt = figures.decomposition(m, x, trajectory=1, eps=eps[:, 1:2])
    assert tuple(dt.shape) == (H, W, 3)
    nox = figures.trajectory_sheet(tr, image=0)
    assert tuple(nox.shape) == figures.layout(T + 1, ('pred', 'seg', 'slots'), K, S, 1, 2)[:2] + (3,)


def _png_size(path):
    """(H, W) of an 8-bit RGB PNG whose IDAT decompresses to H rows of 1 + 3 W bytes"""
    b = open(path, 'rb').read()
    assert b[:8] == b'\x89PNG\r\n\x1a\n' and b[12:16] == b'IHDR'
    W, H, depth, colour = struct.unpack('>IIBB', b[16:26])
    assert (depth, colour) == (8, 2)
    i, idat = 8, b''
    while i < len(b):
        n, = struct.unpack('>I', b[i:i + 4])
        if b[i + 4:i + 8] == b'IDAT':
            idat += b[i + 8:i + 8 + n]
        i += 12 + n
    assert len(zlib.decompress(idat)) == H * (1 + 3 * W)
    return H, W


def test_engine_sheet_every_leaves_the_losses_bitwise_and_writes_pngs(tmp_path):
    from iodine_amd import engine
    from iodine_amd.data import make_dataloader
    from iodine_amd.optim import make_optimizer
    arch = golden_setup(load_golden('tiny'))[0]
    dl = make_dataloader(engine.SyntheticScenes(8, arch.img_size), batch_size=4, shuffle=False)
    runs = []
    for kw in ({}, dict(sheet_every=1, sheet_path=str(tmp_path / 'out.png'), sheet_images=3)):
        _, m, _ = _tiny()
        opt = make_optimizer(m, base_lr=3e-3)
        runs.append((engine.train(m, opt, dl, torch.device(DEV), 3, print_every=1000, **kw), [p.detach().clone() for p in m.parameters()]))
    assert len(runs[0][0]) == 3 and runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    files = sorted(os.listdir(tmp_path))
    assert files == ['out_0000001.png', 'out_0000002.png', 'out_0000003.png']
    want = figures.layout(3, ('image', 'pred', 'gt', 'seg', 'slots'), arch.slots, arch.img_size, 1, 2)[:2]     # the batches carry masks
    assert all(_png_size(str(tmp_path / f)) == want for f in files)
    # the sheet after evaluation, from a DataLoader batch and from a device-resident one; the refinement figure
    _, m, _ = _tiny()
    engine.save_sheet(m, next(iter(dl)), str(tmp_path / 'a.png'), torch.device(DEV), images=2, scale=2, log=lambda *a: None)
    assert _png_size(str(tmp_path / 'a.png')) == figures.layout(2, ('image', 'pred', 'gt', 'seg', 'slots'), arch.slots, arch.img_size, 2, 2)[:2]
    from iodine_amd.resident import ResidentDataset
    store = ResidentDataset.synthetic(8, arch.img_size, device=torch.device(DEV))
    engine.save_sheet(m, next(iter(store.batches(4, shuffle=False))), str(tmp_path / 'b.png'), torch.device(DEV), images=4, trajectory=2,
                      log=lambda *a: None)
    assert _png_size(str(tmp_path / 'b.png')) == figures.layout(arch.iters + 1, ('image', 'pred', 'gt', 'seg', 'slots'), arch.slots, arch.img_size, 1, 2)[:2]
    with pytest.raises(ValueError, match='sheet_path'):
        engine.train(m, None, [], torch.device(DEV), 1, sheet_every=2)


def test_traversal_save_png(tmp_path):
    from iodine_amd.traverse import Traversal
    pred = torch.rand(1, 2, 3, 3, 4, 4, generator=torch.Generator().manual_seed(1)).to(DEV) * 1.5 - 0.25
    t = Traversal(pred=pred, mask=None, slots=[0], dims=torch.zeros(1, 2, dtype=torch.int64), values=torch.zeros(3), base=())
    t.save_png(str(tmp_path / 't.png'), 0)
    assert _png_size(str(tmp_path / 't.png')) == (8, 12)
    b = (tmp_path / 't.png').read_bytes()
    want = R.quantise(t.grid(0).cpu().numpy()).transpose(1, 2, 0)
    assert b == figures.encode_png(np.ascontiguousarray(want))
    t.save_png(str(tmp_path / 'u.png'), 0, transpose=True)
    assert _png_size(str(tmp_path / 'u.png')) == (12, 8)
