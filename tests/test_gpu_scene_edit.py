"""IODINE.edit / iodine_scene_edit / iodine_amd.traverse on the device.

The yardstick is ``model.decode`` on the fully materialised edited scenes - the code every pull request before this one ran.  A replace
edit must return its BITS (``torch.equal``): the decoder kernels treat slot-images independently and the per-pixel kernel repeats
final_out_kernel's operation order.  A removal is compared with the decode of the K - 1 kept slots: both sides evaluate the same
expression from identical float inputs with at most K-term fp32 sums, bound 32 * 2^-24 relative on the mask and 64 * 2^-24 absolute on
pred at K = 16; asserted at twice that, rtol 4e-6 / atol 8e-6 (bitwise equality is expected with the -inf formulation; the observed
maximum is printed)."""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

from iodine_amd import _lib, synth
from iodine_amd import traverse as TR
from oracle import iodine_oracle as O
from util import make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

GEN = O.Arch(dim_latent=6, iters=2, slots=16, img_size=24, dec_chan=8, dec_layers=2, ref_chan=8, ref_layers=2, ref_mlp=12)
# name -> (arch, options, K, B)
CONFIGS = {
    'tiny': (O.tiny_arch(slots=4), {}, 4, 2),
    'dsprites': (O.dsprites_arch(slots=4, iters=2), {}, 4, 2),
    'dsprites_fp32': (O.dsprites_arch(slots=4, iters=2), {'conv_precision': 0}, 4, 2),
    'clevr': (O.clevr_arch(slots=3, iters=2), {}, 3, 1),
    'generic_k16': (GEN, {}, 16, 2),                                            # generic decoder, padded handle (L = 6), P = 576
    'generic_k1': (GEN, {}, 1, 2),
    'generic_k5x5': (dataclasses.replace(GEN, dec_kernel=5), {}, 16, 2),
}


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(model, z (B, K, L) on the device, decode(z)) of one configuration, made once and shared (treated as read-only)"""
    arch, options, K, B = CONFIGS[name]
    pn = synth.make_params(O.param_shapes(arch), seed=41, dec_gain=3.0, posterior_scale=0.05)
    m = make_hip_model(arch, {k: torch.from_numpy(v) for k, v in pn.items()}, options=options)
    g = torch.Generator().manual_seed(100 + len(name))
    z = torch.randn(B, K, arch.dim_latent, generator=g).to(DEV)
    return m, z, m.decode(z)


def _z_new(name, E, seed=0):
    _, z, _ = _setup(name)
    g = torch.Generator().manual_seed(7 + seed)
    return torch.randn(E, z.shape[2], generator=g).to(DEV)


def _full_decode(m, z, image, slot, z_new):
    """decode of the E fully materialised scenes: pred (E,3,S,S), mask (E,K,1,S,S), mean of the edited slot (E,3,S,S)"""
    E = len(image)
    ze = z[torch.as_tensor(image, device=z.device)].clone()
    ze[torch.arange(E), torch.as_tensor(slot)] = z_new
    pred, mask, mean = m.decode(ze)
    return pred, mask, mean[torch.arange(E), torch.as_tensor(slot)]


def _assert_replace_equals_decode(m, z, image, slot, z_new, what):
    out = m.edit(z, image, slot, z_new, return_mask=True, return_mean=True)
    pred, mask, mean = _full_decode(m, z, image, slot, z_new)
    assert out.pred.shape == pred.shape and out.mask.shape == mask.shape and out.mean.shape == mean.shape
    for n, a, b in (('pred', out.pred, pred), ('mask', out.mask, mask), ('mean', out.mean, mean)):
        print(what, n, 'max |diff|', float((a - b).abs().max()))
        assert torch.equal(a, b), (what, n)
    return out


def _edit_list(K, B):
    """first and last slot, every image, one (image, slot) twice"""
    image = [0, B - 1, 0, B - 1, 0]
    slot = [0, K - 1, K - 1, K // 2, 0]
    return image, slot


@pytest.mark.parametrize('name', list(CONFIGS))
def test_replace_equals_full_decode(name):
    m, z, dec = _setup(name)
    B, K = z.shape[:2]
    image, slot = _edit_list(K, B)
    if name == 'clevr':
        image, slot = image[:4], slot[:4]                     # E = 4; (0, 0) and (0, K - 1) twice each at B = 1
    zn = _z_new(name, len(image))
    out = _assert_replace_equals_decode(m, z, image, slot, zn, name)
    assert not torch.equal(out.pred[0], dec[0][image[0]])     # (the edit does change the scene: the comparison above is not vacuous)
    assert float((out.mask.sum(1) - 1.0).abs().max()) < 1e-5


@pytest.mark.parametrize('name', ['tiny', 'generic_k16', 'generic_k1'])
def test_single_edit_and_three_chunks(name):
    m, z, _ = _setup(name)
    B, K = z.shape[:2]
    _assert_replace_equals_decode(m, z, [B - 1], [K - 1], _z_new(name, 1, 1), name + ' E=1')
    # an arena of B images holds B K edit decodes: 2 B K + 1 replacements run in three chunks behind ONE base decode
    E = 2 * B * K + 1
    image = [e % B for e in range(E)]
    slot = [(e // B) % K for e in range(E)]
    m.set_option('batch_cap', B)
    try:
        _assert_replace_equals_decode(m, z, image, slot, _z_new(name, E, 2), name + ' chunks')
    finally:
        m.set_option('batch_cap', 0)


def test_three_chunks_through_the_c_entry():
    """the raw entry with chunk_images = B; more than 256 edits also split the rendering launches of a chunk"""
    m, z, _ = _setup('generic_k16')
    B, K, L = z.shape
    S = m.img_size
    E = 2 * B * K + 1
    image = [e % B for e in range(E)]
    slot = [(e // B) % K for e in range(E)]
    zn = _z_new('generic_k16', E, 3)
    ref = _full_decode(m, z, image, slot, zn)
    m.decode(z)                                              # workspace of B images on the handle
    pred = torch.empty(E, 3, S, S, device=DEV)
    arr = lambda v: (C.c_int * E)(*v)
    rc = _lib.lib().iodine_scene_edit(m._handle, _lib.stream(), B, _lib.ptr(z), E, arr(image), arr(slot), arr([0] * E), _lib.ptr(zn), B,
                                      _lib.ptr(pred), None, None, None, None, None)
    _lib.check(rc, m._handle, 'iodine_scene_edit')
    assert torch.equal(pred, ref[0])
    # one chunk of 2 * 256 + 3 edits in an arena that holds them all: three rendering launches
    m2, z2, _ = _setup('tiny')
    E2 = 2 * 256 + 3
    image2, slot2 = [e % 2 for e in range(E2)], [(e // 2) % 4 for e in range(E2)]
    _assert_replace_equals_decode(m2, z2, image2, slot2, _z_new('tiny', E2, 4), 'tiny 515 edits')


@pytest.mark.parametrize('name', ['tiny', 'dsprites', 'generic_k16'])
def test_identity_edit_gives_the_base_and_the_base_is_decode(name):
    m, z, dec = _setup(name)
    B, K = z.shape[:2]
    image, slot = _edit_list(K, B)
    zn = z[torch.as_tensor(image), torch.as_tensor(slot)].clone()
    out = m.edit(z, image, slot, zn, return_mask=True, return_mean=True, return_base=True)
    for j in range(3):
        assert torch.equal(out.base[j], dec[j]), (name, 'base', j)
    for e, (b, s) in enumerate(zip(image, slot)):
        assert torch.equal(out.pred[e], dec[0][b]) and torch.equal(out.mask[e], dec[1][b]) and torch.equal(out.mean[e], dec[2][b, s]), (name, e)


@pytest.mark.parametrize('name', ['tiny', 'dsprites', 'clevr', 'generic_k16', 'generic_k5x5'])
def test_removal(name):
    m, z, dec = _setup(name)
    B, K = z.shape[:2]
    image, slot = _edit_list(K, B)
    E = len(image)
    out = m.edit(z, image, slot, None, remove=[True] * E, return_mask=True, return_mean=True)
    worst_m = worst_p = 0.0
    for e, (b, s) in enumerate(zip(image, slot)):
        assert float(out.mask[e, s].abs().max()) == 0.0, (name, e)                 # exactly 0
        assert torch.equal(out.mean[e], dec[2][b, s])                              # the rgb of the slot that was removed
        keep = [k for k in range(K) if k != s]
        pred, mask, _ = m.decode(z[b:b + 1, keep])
        got = out.mask[e, keep]
        worst_m = max(worst_m, float(((got - mask[0]).abs() / mask[0].abs().clamp_min(1e-38)).max()))
        worst_p = max(worst_p, float((out.pred[e] - pred[0]).abs().max()))
        assert torch.allclose(got, mask[0], rtol=4e-6, atol=0.0), (name, e)
        assert torch.allclose(out.pred[e], pred[0], rtol=0.0, atol=8e-6), (name, e)
    print(name, 'removal: max relative mask difference', worst_m, 'max absolute pred difference', worst_p)


def test_removal_at_one_slot_raises_and_names_the_edit():
    m, z, _ = _setup('generic_k1')
    with pytest.raises(ValueError, match='edit 1: removes the only slot'):
        m.edit(z, [0, 1], [0, 0], _z_new('generic_k1', 2), remove=[False, True])
    # the library's own refusal, through the raw entry
    m.decode(z)
    one = (C.c_int * 1)(0)
    rm = (C.c_int * 1)(1)
    rc = _lib.lib().iodine_scene_edit(m._handle, _lib.stream(), 2, _lib.ptr(z), 1, one, one, rm, None, 0, None, None, None, None, None, None)
    assert rc == 1
    assert b'edit 0' in _lib.lib().iodine_last_error(m._handle)


@pytest.mark.parametrize('name', ['tiny', 'generic_k16'])
def test_mixed_list_gives_the_bits_of_the_separate_calls(name):
    m, z, _ = _setup(name)
    B, K = z.shape[:2]
    image = [0, B - 1, 0, B - 1, 0, B - 1, 0]
    slot = [0, K - 1, K - 1, 0, 1, 1, 0]
    remove = [False, True, False, True, True, False, False]
    E = len(image)
    zn = _z_new(name, E, 5)
    kw = dict(return_mask=True, return_mean=True)
    mixed = m.edit(z, image, slot, zn, remove=remove, **kw)
    rep = [e for e in range(E) if not remove[e]]
    rem = [e for e in range(E) if remove[e]]
    a = m.edit(z, [image[e] for e in rep], [slot[e] for e in rep], zn[rep], **kw)
    b = m.edit(z, [image[e] for e in rem], [slot[e] for e in rem], None, remove=[True] * len(rem), **kw)
    for part, idx in ((a, rep), (b, rem)):
        for j, e in enumerate(idx):
            assert torch.equal(mixed.pred[e], part.pred[j]) and torch.equal(mixed.mask[e], part.mask[j]) and torch.equal(mixed.mean[e], part.mean[j]), (name, e)
    # a small arena splits the mixed list into chunks: the same bits
    m.set_option('batch_cap', B)
    try:
        image3, slot3, remove3 = image * 6, slot * 6, remove * 6                  # 24 replacements at K = 4: three chunks of B K = 8
        zn3 = zn.repeat(6, 1)
        big = m.edit(z, image3, slot3, zn3, remove=remove3, **kw)
    finally:
        m.set_option('batch_cap', 0)
    for e in range(len(image3)):
        assert torch.equal(big.pred[e], mixed.pred[e % E]) and torch.equal(big.mask[e], mixed.mask[e % E]) and torch.equal(big.mean[e], mixed.mean[e % E]), (name, e)


def test_optional_outputs_do_not_change_the_bits():
    m, z, dec = _setup('tiny')
    B, K = z.shape[:2]
    image, slot = _edit_list(K, B)
    remove = [False, False, True, False, False]
    zn = _z_new('tiny', len(image), 6)
    full = m.edit(z, image, slot, zn, remove=remove, return_mask=True, return_mean=True, return_base=True)
    for rm in (False, True):
        for rn in (False, True):
            for rb in (False, True):
                o = m.edit(z, image, slot, zn, remove=remove, return_mask=rm, return_mean=rn, return_base=rb)
                assert torch.equal(o.pred, full.pred)
                assert (o.mask is None) == (not rm) and (o.mean is None) == (not rn) and (o.base is None) == (not rb)
                assert not rm or torch.equal(o.mask, full.mask)
                assert not rn or torch.equal(o.mean, full.mean)
                assert not rb or all(torch.equal(x, y) for x, y in zip(o.base, dec))
    assert not full.pred.requires_grad
    zg = z.clone().requires_grad_(True)
    assert not m.edit(zg, image, slot, zn).pred.requires_grad                  # detached: gradients go through decode


def test_raw_entry_refuses_bad_lists_before_any_launch():
    m, z, _ = _setup('tiny')
    B, K, L = z.shape
    S = m.img_size
    m.decode(z)
    zn = _z_new('tiny', 2, 8)
    poison = torch.full((2, 3, S, S), -7.0, device=DEV)
    pmask = torch.full((2, K, 1, S, S), -7.0, device=DEV)
    pbase = torch.full((B, 3, S, S), -7.0, device=DEV)
    arr = lambda v: (C.c_int * len(v))(*v)
    call = lambda image, slot, kind, chunk=0, n=2, znew=zn: _lib.lib().iodine_scene_edit(
        m._handle, _lib.stream(), B, _lib.ptr(z), n, arr(image), arr(slot), arr(kind), _lib.ptr(znew), chunk, _lib.ptr(poison), _lib.ptr(pmask), None,
        _lib.ptr(pbase), None, None)
    err = lambda: _lib.lib().iodine_last_error(m._handle).decode()
    assert call([0, B], [0, 0], [0, 0]) == 1 and 'edit 1: image' in err()
    assert call([0, -1], [0, 0], [0, 0]) == 1 and 'edit 1: image' in err()
    assert call([0, 1], [K, 0], [0, 0]) == 1 and 'edit 0: slot' in err()
    assert call([0, 1], [0, -1], [0, 0]) == 1 and 'edit 1: slot' in err()
    assert call([0, 1], [0, 0], [0, 2]) == 1 and 'edit 1: kind' in err()
    assert call([0, 1], [0, 0], [0, 0], chunk=B - 1) == 1 and 'chunk_images' in err()
    assert call([0, 1], [0, 0], [1, 0], znew=None) == 1 and 'edit 1' in err() and 'z_new' in err()
    assert call([0, 1], [0, 0], [0, 0], n=0) == 1
    torch.cuda.synchronize()
    for t in (poison, pmask, pbase):
        assert float((t + 7.0).abs().max()) == 0.0                                                  # nothing was launched
    assert call([0, 1], [0, 0], [1, 1], znew=None) == 0                                             # all removals: z_new may be NULL
    torch.cuda.synchronize()
    assert float(pmask[:, 0].abs().max()) == 0.0


def test_call_state_reconstruct_edit_decode():
    m, z, dec = _setup('tiny')
    B, K = z.shape[:2]
    arch = CONFIGS['tiny'][0]
    imgs, _ = synth.make_images(B, arch.img_size, seed=3, kind='blobs')
    x = torch.from_numpy(imgs).to(DEV)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, K, arch.dim_latent, seed=4)).to(DEV)
    r0 = m.reconstruct(x, eps)
    image, slot = _edit_list(K, B)
    out = m.edit(z, image, slot, _z_new('tiny', len(image), 9))               # 5 replacements: fits the arena of B images
    d1 = m.decode(z)
    assert all(torch.equal(a, b) for a, b in zip(d1, dec))
    r1 = m.reconstruct(x, eps)
    assert all(torch.equal(a, b) for a, b in zip(r1, r0))
    out2 = m.edit(z, image, slot, _z_new('tiny', len(image), 9))
    assert torch.equal(out2.pred, out.pred)
    # the last elbo()'s decoder output was overwritten by the base decode: the library says so instead of rendering the wrong scene
    S = m.img_size
    buf = torch.empty(B, 3, S, S, device=DEV)
    rc = _lib.lib().iodine_last_elbo_outputs(m._handle, _lib.stream(), B, None, None, None, None, _lib.ptr(buf))
    assert rc == 3                                                               # IODINE_ERR_STATE


def test_edit_discards_a_pending_training_forward():
    m, z, _ = _setup('tiny')
    B, K = z.shape[:2]
    arch = CONFIGS['tiny'][0]
    imgs, _ = synth.make_images(B, arch.img_size, seed=3, kind='blobs')
    x = torch.from_numpy(imgs).to(DEV)
    eps = torch.from_numpy(synth.make_eps(arch.iters, B, K, arch.dim_latent, seed=4)).to(DEV)
    loss = m(x, eps)
    m.edit(z, [0], [0], _z_new('tiny', 1))
    with pytest.raises(RuntimeError, match='stale forward'):
        loss.backward()
    m.zero_grad(set_to_none=True)


def test_traversal_end_to_end():
    m, z, dec = _setup('dsprites')
    B, K, L = z.shape
    g = torch.Generator().manual_seed(17)
    pm, plv = torch.randn(B, K, L, generator=g).to(DEV), (0.5 * torch.randn(B, K, L, generator=g) - 1.0).to(DEV)
    values = torch.linspace(-1, 1, 3)
    slots = [0, 3]
    t = TR.traverse(m, z, image=1, slots=slots, dims=None, posterior=(pm, plv), top=3, values=values, mode='sigma', return_mask=True)
    S = m.img_size
    assert t.pred.shape == (2, 3, 3, 3, S, S) and t.mask.shape == (2, 3, 3, K, 1, S, S)
    # the ranking, computed independently: descending KL with the lowest index first on a tie
    kl = (0.5 * (plv[1].double().exp() + pm[1].double() ** 2 - 1.0 - plv[1].double())).cpu()
    kl32 = TR.latent_kl(pm[1], plv[1]).cpu()
    for i, s in enumerate(slots):
        order = sorted(range(L), key=lambda d: (-float(kl32[s, d]), d))[:3]
        assert t.dims[i].tolist() == order
        assert bool((kl[s, order].diff() <= 1e-6).all())
    assert torch.equal(t.base[0], dec[0][1]) and torch.equal(t.base[1], dec[1][1]) and torch.equal(t.base[2], dec[2][1])
    # entry [i, j, v] = decode of the hand-built z
    zs = []
    for i, s in enumerate(slots):
        for j in range(3):
            d = int(t.dims[i, j])
            for v in values.tolist():
                ze = z[1].clone()
                ze[s, d] = pm[1, s, d] + torch.tensor(v, device=DEV) * torch.exp(0.5 * plv[1, s, d])
                zs.append(ze)
    pred, mask, _ = m.decode(torch.stack(zs))
    assert torch.equal(t.pred.reshape(-1, 3, S, S), pred)
    assert torch.equal(t.mask.reshape(-1, K, 1, S, S), mask)
    assert t.grid(1).shape == (3, 3 * S, 3 * S)
    assert torch.equal(t.grid(1)[:, S:2 * S, 2 * S:], t.pred[1, 1, 2])


def test_engine_save_traversal(tmp_path):
    """engine.save_traversal (behind --traverse): reconstruct, rank by KL, traverse image 0 along the posterior, save the grids"""
    import numpy as np

    from iodine_amd import engine
    m, z, _ = _setup('tiny')
    arch = CONFIGS['tiny'][0]
    B, K, L, S = 2, m.K, arch.dim_latent, arch.img_size
    imgs, _ = synth.make_images(B, S, seed=3, kind='blobs')
    path = str(tmp_path / 'trav.npz')
    m.manual_seed(5)
    t = engine.save_traversal(m, torch.from_numpy(imgs).to(DEV), path, top=3, n_values=5, log=lambda *a: None)
    f = np.load(path)
    assert f['grids'].shape == (K, 3, 3 * S, 5 * S) and f['dims'].shape == (K, 3) and f['values'].shape == (5,) and f['kl'].shape == (K, L)
    pm, plv = m.posterior.mean[0], m.posterior.logvar[0]
    assert np.array_equal(f['dims'], TR.rank_dims(pm, plv, 3).cpu().numpy())
    assert np.array_equal(f['grids'][2], t.grid(2).cpu().numpy())
    # v = 0 is the posterior mean of the unit: column 2 of every row of slot i decodes z with z[i, d] = mu[i, d]
    ze = m.z[0].clone()
    d = int(f['dims'][1, 0])
    ze[1, d] = pm[1, d]
    assert torch.equal(t.pred[1, 0, 2], m.decode(ze[None])[0][0])
