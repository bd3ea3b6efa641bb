"""iodine_amd.traverse on the CPU: the KL ranking, the edit-list builder and the grid layout are plain torch; IODINE.edit refuses bad
argument lists before it touches a device; the C entry refuses a null handle."""
import ctypes as C

import pytest
import torch

from iodine_amd import IODINE, _lib
from iodine_amd import traverse as TR
from iodine_amd.model import arch_namespace


def _module(K=3, T=2):
    return IODINE(arch_namespace(8, T, K, 16, (32, 2, 32), (32, 2)))     # tiny arch, parameters on the CPU


def test_exports():
    import iodine_amd
    assert iodine_amd.traverse is TR and callable(TR.traverse)
    assert iodine_amd.latent_kl is TR.latent_kl and iodine_amd.rank_dims is TR.rank_dims and iodine_amd.Traversal is TR.Traversal
    assert 'traverse' in iodine_amd.__all__


def test_latent_kl_against_the_formula_in_float64():
    g = torch.Generator().manual_seed(3)
    m, lv = torch.randn(2, 5, 16, generator=g, dtype=torch.float64), torch.randn(2, 5, 16, generator=g, dtype=torch.float64)
    got = TR.latent_kl(m, lv)
    assert got.shape == m.shape and got.dtype == torch.float64
    ref = torch.empty_like(m)
    for i in range(m.numel()):                           # element by element with Python floats
        a, b = float(m.view(-1)[i]), float(lv.view(-1)[i])
        ref.view(-1)[i] = 0.5 * (torch.exp(torch.tensor(b, dtype=torch.float64)).item() + a * a - 1.0 - b)
    assert torch.allclose(got, ref, rtol=1e-14, atol=1e-15)
    assert float(TR.latent_kl(torch.zeros(4), torch.zeros(4)).abs().max()) == 0.0        # N(0, 1) against itself
    assert TR.latent_kl(m.float(), lv.float()).dtype == torch.float32


def test_rank_dims_descending_stable_and_top():
    m = torch.tensor([[0.0, 2.0, 1.0, 2.0, 0.0, -2.0], [3.0, 0.0, 0.0, 1.0, 1.0, 0.5]], dtype=torch.float64)
    lv = torch.zeros_like(m)                              # KL = m^2 / 2: ties between units 1, 3, 5 and between 0, 4 of row 0
    idx = TR.rank_dims(m, lv)
    assert idx.shape == (2, 6)
    assert idx[0].tolist() == [1, 3, 5, 2, 0, 4]          # on a tie the lowest index first
    assert idx[1].tolist() == [0, 3, 4, 5, 1, 2]
    assert TR.rank_dims(m, lv, top=2).tolist() == [[1, 3], [0, 3]]
    kl = TR.latent_kl(m, lv)
    assert bool((torch.gather(kl, 1, idx).diff(dim=1) <= 0).all())
    lead = TR.rank_dims(m.reshape(2, 1, 6).expand(2, 3, 6), lv.reshape(2, 1, 6).expand(2, 3, 6), top=4)
    assert lead.shape == (2, 3, 4) and lead[1, 2].tolist() == [0, 3, 4, 5]
    for bad in (0, 7, 2.5, True):
        with pytest.raises(ValueError, match='top'):
            TR.rank_dims(m, lv, top=bad)


def test_build_edits_order_and_modes_against_hand_computed_rows():
    z = torch.arange(12, dtype=torch.float64).reshape(3, 4)           # slot k = [4k, 4k+1, 4k+2, 4k+3]
    slots, dims, values = [2, 0], [[1, 3], [0, 2]], [10.0, 20.0]
    slot, zn = TR.build_edits(z, slots, dims, values, 'set')
    assert slot.tolist() == [2, 2, 2, 2, 0, 0, 0, 0]                 # by slot, then unit, then value
    assert zn.tolist() == [[8, 10, 10, 11], [8, 20, 10, 11], [8, 9, 10, 10], [8, 9, 10, 20],
                           [10, 1, 2, 3], [20, 1, 2, 3], [0, 1, 10, 3], [0, 1, 20, 3]]
    _, za = TR.build_edits(z, slots, dims, values, 'add')
    assert za.tolist() == [[8, 19, 10, 11], [8, 29, 10, 11], [8, 9, 10, 21], [8, 9, 10, 31],
                           [10, 1, 2, 3], [20, 1, 2, 3], [0, 1, 12, 3], [0, 1, 22, 3]]
    pm = z + 100.0
    plv = torch.log(torch.tensor([[1.0, 4.0, 9.0, 16.0]], dtype=torch.float64)).expand(3, 4).contiguous()    # sigma = 1, 2, 3, 4
    _, zs = TR.build_edits(z, slots, dims, values, 'sigma', posterior=(pm, plv))
    ref = [[8, 109 + 20, 10, 11], [8, 109 + 40, 10, 11], [8, 9, 10, 111 + 40], [8, 9, 10, 111 + 80],
           [100 + 10, 1, 2, 3], [100 + 20, 1, 2, 3], [0, 1, 102 + 30, 3], [0, 1, 102 + 60, 3]]
    assert torch.allclose(zs, torch.tensor(ref, dtype=torch.float64), rtol=1e-14, atol=0)
    assert torch.equal(z, torch.arange(12, dtype=torch.float64).reshape(3, 4))       # the input is left alone
    # the same slot twice and a single value
    s1, z1 = TR.build_edits(z, [1, 1], [[0], [0]], [5.0])
    assert s1.tolist() == [1, 1] and z1.tolist() == [[5, 5, 6, 7], [5, 5, 6, 7]]


def test_build_edits_refusals():
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError, match='posterior'):
        TR.build_edits(z, [0], [[1]], [1.0], 'sigma')
    with pytest.raises(ValueError, match='mode'):
        TR.build_edits(z, [0], [[1]], [1.0], 'scale')
    with pytest.raises(ValueError, match='slots'):
        TR.build_edits(z, [3], [[1]], [1.0])
    with pytest.raises(ValueError, match='dims'):
        TR.build_edits(z, [0], [[4]], [1.0])
    with pytest.raises(ValueError, match='dims'):
        TR.build_edits(z, [0, 1], [[1]], [1.0])
    with pytest.raises(ValueError, match='posterior'):
        TR.build_edits(z, [0], [[1]], [1.0], 'sigma', posterior=(torch.zeros(3, 4), torch.zeros(2, 4)))


def test_traverse_refusals_before_any_device_call():
    m = _module(K=3)
    z = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match='posterior'):
        TR.traverse(m, z, dims=None)                                  # ranking needs the posterior
    with pytest.raises(ValueError, match='posterior'):
        TR.traverse(m, z, dims=[0, 1], mode='sigma')
    with pytest.raises(ValueError, match='image'):
        TR.traverse(m, z, image=2, dims=[0])
    with pytest.raises(ValueError, match='slots'):
        TR.traverse(m, z, slots=[3], dims=[0])
    with pytest.raises(ValueError, match='posterior'):
        TR.traverse(m, z, dims=[0], posterior=(torch.zeros(2, 3, 8), torch.zeros(2, 3, 7)))


def test_grid_layout_and_transpose():
    n_s, n_d, V, S = 2, 3, 4, 5
    code = lambda i, j, v, c: 1000.0 * i + 100.0 * j + 10.0 * v + c
    pred = torch.empty(n_s, n_d, V, 3, S, S)
    for i in range(n_s):
        for j in range(n_d):
            for v in range(V):
                for c in range(3):
                    pred[i, j, v, c] = code(i, j, v, c)             # constant tiles
    t = TR.Traversal(pred=pred, mask=None, slots=[0, 1], dims=torch.zeros(n_s, n_d, dtype=torch.int64), values=torch.zeros(V), base=(None,) * 3)
    for i in range(n_s):
        g = t.grid(i)
        assert g.shape == (3, n_d * S, V * S)
        gt = t.grid(i, transpose=True)
        assert gt.shape == (3, V * S, n_d * S)
        for j in range(n_d):
            for v in range(V):
                for c in range(3):
                    tile = g[c, j * S:(j + 1) * S, v * S:(v + 1) * S]          # rows are units, columns are values
                    assert float(tile.min()) == float(tile.max()) == code(i, j, v, c)
                    tile = gt[c, v * S:(v + 1) * S, j * S:(j + 1) * S]         # one column per unit
                    assert float(tile.min()) == float(tile.max()) == code(i, j, v, c)
    # a tile keeps its orientation: rows stay rows
    pred2 = torch.arange(S * S, dtype=torch.float32).reshape(1, 1, 1, 1, S, S).expand(1, 2, 2, 3, S, S).contiguous()
    t2 = TR.Traversal(pred=pred2, mask=None, slots=[0], dims=torch.zeros(1, 2, dtype=torch.int64), values=torch.zeros(2), base=(None,) * 3)
    assert torch.equal(t2.grid(0)[0, S:2 * S, S:2 * S], pred2[0, 1, 1, 0])
    assert torch.equal(t2.grid(0, transpose=True)[0, S:2 * S, 0:S], pred2[0, 0, 1, 0])


def test_edit_validates_arguments_before_any_device_call():
    m = _module(K=3)
    z = torch.zeros(2, 3, 8)                                          # on the CPU: a valid list would fail later, at the device
    zn = torch.zeros(2, 8)
    with pytest.raises(ValueError, match=r'z must have shape \(B, K, 8\)'):
        m.edit(torch.zeros(2, 3, 7), [0], [0], torch.zeros(1, 7))
    with pytest.raises(ValueError, match=r'1 <= K <= 16'):
        m.edit(torch.zeros(1, 17, 8), [0], [0], torch.zeros(1, 8))
    with pytest.raises(ValueError, match='slot has 1 entries, but there are 2 edits'):
        m.edit(z, [0, 1], [0], zn)
    with pytest.raises(ValueError, match='remove has 3 entries, but there are 2 edits'):
        m.edit(z, [0, 1], [0, 1], zn, remove=[False, True, False])
    with pytest.raises(ValueError, match=r'edit 1: slot 3 is outside 0\.\.2'):
        m.edit(z, [0, 1], [0, 3], zn)
    with pytest.raises(ValueError, match=r'edit 0: slot -1 is outside'):
        m.edit(z, [0, 1], [-1, 0], zn)
    with pytest.raises(ValueError, match=r'edit 1: image 2 is outside 0\.\.1'):
        m.edit(z, torch.tensor([0, 2]), torch.tensor([0, 1]), zn)
    with pytest.raises(ValueError, match=r'z_new must have shape \(2, 8\)'):
        m.edit(z, [0, 1], [0, 1], torch.zeros(3, 8))
    with pytest.raises(ValueError, match=r'z_new must have shape \(2, 8\)'):
        m.edit(z, [0, 1], [0, 1], torch.zeros(2, 7))
    with pytest.raises(ValueError, match=r'z_new must have shape \(2, 8\)'):
        m.edit(z, [0, 1], [0, 1], None, remove=[True, False])         # one replacement left: it needs its row
    with pytest.raises(ValueError, match='empty'):
        m.edit(z, [], [], torch.zeros(0, 8))
    with pytest.raises(ValueError, match='integers'):
        m.edit(z, [0.5, 1], [0, 1], zn)
    with pytest.raises(ValueError, match=r'edit 0: removes the only slot'):
        m.edit(torch.zeros(2, 1, 8), [0], [0], remove=[True])
    # a well-formed list passes every check above and is stopped by the device check only (no CPU path)
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.edit(z, [0, 1], [0, 2], zn)


def test_scene_edit_entry_refuses_a_null_handle():
    L = _lib.lib()
    assert 'iodine_scene_edit' in _lib.EXPORTS and hasattr(L, 'iodine_scene_edit')
    one = (C.c_int * 1)(0)
    assert L.iodine_scene_edit(None, None, 1, None, 1, one, one, one, None, 0, None, None, None, None, None, None) == 1    # IODINE_ERR_INVALID
    assert L.iodine_abi_version() == 3                                # additive: the ABI version stays
