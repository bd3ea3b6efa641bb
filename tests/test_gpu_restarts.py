"""iodine_chain_score / iodine_chain_consensus, IODINE.restarts and engine.evaluate(restarts=C) on the device.

Kernel level: tests/restarts_reference.py (numpy; float64 for ``ll`` and ``mask_mean``, integers for the rest) on the smallest shapes at
which the kernels can go wrong - P = 256 (exactly one vector per thread of a quarter block), P = 100 (P % 4 != 0: scalar loads), P = 576
(vector loads, a partial stride), K in {1, 3, 16}, C in {1, 2, 5}, B in {1, 3}, B = 300 (several chains per block), every pointer off
by one float (the unaligned path).

Bounds.  ``ll``: |ll - reference| <= 1e-6 sum_p |w_p LL_p|, the project's bound for the same quantity (tests/test_gpu_predictive.py).
``seg``, ``votes``, ``consensus``, ``agreement``, ``match``: bitwise.  ``mask_mean``, u = 2^-24 the unit roundoff: the sum starts from 0, so the
first addition is exact; adding the c-th value (c >= 2) rounds a partial sum <= c, an error <= c u; together u (C (C + 1) / 2 - 1), after
the division by C at most u ((C + 1) / 2 - 1 / C), plus the division's own rounding of a result <= 1, u: |mask_mean - reference| <=
u ((C + 3) / 2 - 1 / C) <= C u for every C >= 2, and exactly 0 for C = 1.  The ``bad`` cases put two slots of one chain on one common
slot - one more addition of a partial sum <= C, one more u after the division, still <= 2 C u.  Asserted at twice the derived bound,
2 C 2^-24, as the predictive tests do.

Cross-check of ``ll`` against an independent implementation, ``model.predictive``'s ``ll`` for the same latents (its per-pixel core takes log m
from the logits' softmax inside the kernel; ``iodine_chain_score`` from the rendered ``m + 1e-12``).  Measured on the MI355X on the ``tiny``
and ``generic_k16`` configurations of tests/test_gpu_predictive.py, relative to sum_p |w_p LL_p|: 9.95e-08 and 1.52e-07, asserted at four
times those (``test_ll_against_predictive``).

End to end: ``restarts`` against one ``reconstruct`` over the repeated batch, against every chain on its own, chunked against unchunked -
all bitwise, like the image-independence tests of tests/test_gpu_fullsize.py / test_gpu_boundary.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import restarts_reference as R
from iodine_amd import _lib, chains, synth
from iodine_amd.objects import slot_table
from oracle import iodine_oracle as O
from util import make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24

# (S, K, C, B)
SHAPES = [(16, 3, 2, 1), (10, 1, 5, 3), (24, 16, 5, 3), (16, 16, 1, 3), (10, 3, 2, 1), (24, 1, 2, 1), (24, 3, 5, 1), (10, 3, 2, 300)]


def _weights(B, S):
    """values in [0, 1.75) with a zero rectangle per image: zeros and values above 1 (as tests/test_gpu_predictive.py builds them)"""
    g = torch.Generator().manual_seed(5)
    w = 1.75 * torch.rand(B, 1, S, S, generator=g)
    for b in range(B):
        w[b, :, 2 + b % 3:8 + b % 3, 3:9] = 0.0
    return w.reshape(B, S, S)


@functools.lru_cache(maxsize=None)
def _decodes(S, K, C, B):
    """C decodes of B images: softmax masks with an exact zero, sigmoid means, and the float64 reference of both likelihood forms with and
    without weights - made once, shared, never modified"""
    g = torch.Generator().manual_seed(1000 * S + 100 * K + 10 * C + B)
    x = torch.rand(B, 3, S, S, generator=g)
    mask = torch.softmax(4.0 * torch.randn(C, B, K, 1, S, S, generator=g), dim=2)
    if K > 1:
        mask[0, 0, 1, 0, 1, 2] = 0.0
    mean = torch.sigmoid(2.0 * torch.randn(C, B, K, 3, S, S, generator=g))
    w = _weights(B, S)
    assert R.top_two_gap(mask.numpy()) > 0.0                                     # no ties: the reference alone decides the arg-max
    ref = {(j, ww): R.chain_score(x.numpy(), w.numpy() if ww else None, mask.numpy(), mean.numpy(), 0.1, j) for j in (False, True)
           for ww in (False, True)}
    return dict(x=x, mask=mask, mean=mean, w=w, ref=ref)


def _raw_score(x, w, mask, mean, sigma, joint, ll, seg):
    Cn, B, K, S = mask.shape[0], mask.shape[1], mask.shape[2], mask.shape[-1]
    rc = _lib.lib().iodine_chain_score(C.c_void_p(torch.cuda.current_stream().cuda_stream), _lib.ptr(x), _lib.ptr(w), _lib.ptr(mask), _lib.ptr(mean),
                                       Cn, B, K, S, sigma, int(joint), _lib.ptr(ll), _lib.ptr(seg))
    _lib.check(rc, None, 'iodine_chain_score')


def _off(t):
    """a copy of ``t`` on the device whose storage starts one element (one float: 4 bytes; one byte for uint8) past an aligned address"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('joint', [False, True])
@pytest.mark.parametrize('S,K,Cn,B', SHAPES)
def test_chain_score_against_the_reference(S, K, Cn, B, joint, weighted):
    d = _decodes(S, K, Cn, B)
    want_ll, scale, want_seg = d['ref'][(joint, weighted)]
    x, mask, mean = (d[n].to(DEV) for n in ('x', 'mask', 'mean'))
    w = d['w'].to(DEV) if weighted else None
    ll, seg = chains.chain_score(x, mask, mean, 0.1, weights=w, joint=joint)
    assert ll.shape == (Cn, B) and ll.dtype == torch.float32 and seg.shape == (Cn, B, S, S) and seg.dtype == torch.uint8
    err = np.abs(ll.double().cpu().numpy() - want_ll)
    print(f'S={S} K={K} C={Cn} B={B} joint={joint} weighted={weighted}: max |ll - ref| / sum|w LL| {float((err / scale).max()):.3e} (bound 1e-6)')
    assert (err <= 1e-6 * scale).all(), (err / scale).max()
    assert np.array_equal(seg.cpu().numpy(), want_seg)
    # the same map as slot_table's, the same bits on a second call, and each output alone
    assert torch.equal(seg, slot_table(mask, segmentation=True)[1])
    ll2, seg2 = chains.chain_score(x, mask, mean, 0.1, weights=w, joint=joint)
    assert torch.equal(ll2, ll) and torch.equal(seg2, seg)
    assert torch.equal(chains.chain_score(x, mask, mean, 0.1, weights=w, joint=joint, segmentation=False)[0], ll)
    assert torch.equal(chains.chain_score(x, mask, mean, 0.1, weights=w, joint=joint, ll=False)[1], seg)


@pytest.mark.parametrize('S,K,Cn,B', [(16, 3, 2, 1), (24, 16, 5, 3)])
def test_chain_score_unaligned_pointers(S, K, Cn, B):
    """every pointer one float (seg: one byte) past an aligned address: the scalar path, the same numbers"""
    d = _decodes(S, K, Cn, B)
    x, mask, mean, w = (d[n].to(DEV) for n in ('x', 'mask', 'mean', 'w'))
    ll, seg = chains.chain_score(x, mask, mean, 0.1, weights=w, joint=False)
    ll_o, seg_o = _off(torch.zeros_like(ll)), _off(torch.zeros_like(seg))
    _raw_score(_off(x), _off(w), _off(mask), _off(mean), 0.1, False, ll_o, seg_o)
    want_ll, scale, want_seg = d['ref'][(False, True)]
    err = np.abs(ll_o.double().cpu().numpy() - want_ll)
    print(f'unaligned S={S} K={K}: max |ll - ref| / scale {float((err / scale).max()):.3e}; max |ll - aligned ll| {float((ll_o - ll).abs().max()):.3e}')
    assert (err <= 1e-6 * scale).all() and np.array_equal(seg_o.cpu().numpy(), want_seg) and torch.equal(seg_o, seg)


def test_chain_score_on_a_side_stream_gives_the_same_bits():
    """the launch follows the caller's current stream: C = 2 chains on a side stream against the default stream"""
    d = _decodes(16, 3, 2, 1)
    x, mask, mean, w = (d[n].to(DEV) for n in ('x', 'mask', 'mean', 'w'))
    ll, seg = chains.chain_score(x, mask, mean, 0.1, weights=w)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ll2, seg2 = chains.chain_score(x, mask, mean, 0.1, weights=w)
    side.synchronize()
    assert torch.equal(ll2.view(torch.int32), ll.view(torch.int32)) and torch.equal(seg2, seg)


def test_chain_score_ties_and_nan():
    """exact ties go to the lowest index; a NaN plane never wins (and a pixel of NaNs alone reads 0)"""
    S, K = 16, 4
    mask = torch.full((2, 1, K, 1, S, S), 0.25)
    mask[0, 0, 2, 0, :, :8] = 0.5                            # chain 0: slot 2 wins the left half, the right half ties -> 0
    mask[0, 0, 0, 0, 3] = 0.125                              #          row 3: slot 0 is below the rest -> 1 on the right, 2 on the left
    mask[1, 0, 0] = float('nan')                             # chain 1: slot 0 is NaN everywhere -> the tie of the rest goes to 1
    mask[1, 0, :, 0, 5, 5] = float('nan')                    #          one pixel of NaNs alone
    mean = torch.rand(2, 1, K, 3, S, S)
    x = torch.rand(1, 3, S, S)
    want = R.chain_score(x.numpy(), None, mask.numpy(), mean.numpy(), 0.1, False)[2]
    assert want[0, 0, 0, 0] == 2 and want[0, 0, 0, 12] == 0 and want[0, 0, 3, 12] == 1 and want[1, 0, 0, 0] == 1 and want[1, 0, 5, 5] == 0
    seg = chains.chain_score(x.to(DEV), mask.to(DEV), mean.to(DEV), 0.1)[1]
    assert np.array_equal(seg.cpu().numpy(), want)
    assert torch.equal(seg, slot_table(mask.to(DEV), segmentation=True)[1])


# ---- consensus ------------------------------------------------------------------------------------------------------------------------------
def _labelled(S, K, Cn, B, bad):
    g = np.random.default_rng(7 * S + K + Cn + B)
    seg = g.integers(0, K, (Cn, B, S, S)).astype(np.uint8)
    perm = np.stack([np.stack([g.permutation(K) for _ in range(B)]) for _ in range(Cn)]).astype(np.int32)
    ref = g.integers(0, Cn, B).astype(np.int32)
    mask = torch.softmax(3.0 * torch.randn(Cn, B, K, 1, S, S, generator=torch.Generator().manual_seed(S + K)), dim=2)
    if bad:                                                  # labels and entries outside their range, at both ends of int32
        seg[0, 0, 0, :3] = (K, 255, 16)
        seg[Cn - 1, B - 1, S - 1, S - 1] = 200
        perm[0, 0, 0], perm[Cn - 1, B - 1, K - 1] = -1, K
        perm[Cn // 2, 0, K // 2] = 2 ** 31 - 1
        perm[0, B - 1, 0] = -2 ** 31
        if K > 1:
            perm[Cn - 1, 0, 1] = perm[Cn - 1, 0, 0]          # not a permutation: two slots of a chain on one common slot
        ref[B - 1] = Cn
        if B > 1:
            ref[0] = -1
    return seg, perm, ref, mask


def _check_consensus(got, want, Cn, B, K, S):
    P = S * S
    assert np.array_equal(got.votes.cpu().numpy().reshape(B, K, P), want['votes'])
    assert np.array_equal(got.consensus.cpu().numpy().reshape(B, P), want['consensus'])
    assert np.array_equal(got.agreement.cpu().numpy().reshape(B, P), want['agreement'])
    assert np.array_equal(got.match.cpu().numpy(), want['match'])
    e = float(np.abs(got.mask_mean.double().cpu().numpy().reshape(B, K, P) - want['mask_mean']).max())
    print(f'S={S} K={K} C={Cn} B={B}: max |mask_mean - ref| {e:.3e} (bound {2 * Cn * U:.3e})')
    assert e <= 2 * Cn * U


@pytest.mark.parametrize('bad', [False, True])
@pytest.mark.parametrize('S,K,Cn,B', SHAPES[:7] + [(10, 16, 5, 40)])
def test_chain_consensus_against_the_reference(S, K, Cn, B, bad):
    seg, perm, ref, mask = _labelled(S, K, Cn, B, bad)
    want = R.chain_consensus(seg, perm, ref, mask.numpy())
    total = want['votes'].sum(1)
    assert (total < Cn).any() if bad else (total == Cn).all()
    args = (torch.from_numpy(seg).to(DEV), torch.from_numpy(perm).to(DEV), torch.from_numpy(ref).to(DEV), mask.to(DEV))
    got = chains.chain_consensus(*args)
    assert got.votes.dtype == torch.int32 and got.consensus.dtype == torch.uint8 and got.match.shape == (Cn, B)
    _check_consensus(got, want, Cn, B, K, S)
    again = chains.chain_consensus(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                    # the same bits on every call
    few = chains.chain_consensus(args[0], args[1])                               # without ref and mask: the other three alone
    assert few.match is None and few.mask_mean is None and torch.equal(few.votes, got.votes) and torch.equal(few.consensus, got.consensus)


def test_chain_consensus_unaligned_pointers():
    S, K, Cn, B = 24, 3, 5, 3
    seg, perm, ref, mask = _labelled(S, K, Cn, B, True)
    want = R.chain_consensus(seg, perm, ref, mask.numpy())
    f = dict(device=DEV)
    votes, cons = _off(torch.zeros(B, K, S, S, dtype=torch.int32, **f)), _off(torch.zeros(B, S, S, dtype=torch.uint8, **f))
    agree, match = _off(torch.zeros(B, S, S, **f)), _off(torch.zeros(Cn, B, **f))
    mmean = _off(torch.zeros(B, K, 1, S, S, **f))
    sg, pr, rf, mk = _off(torch.from_numpy(seg)), _off(torch.from_numpy(perm)), _off(torch.from_numpy(ref)), _off(mask)
    rc = _lib.lib().iodine_chain_consensus(C.c_void_p(torch.cuda.current_stream().cuda_stream), _lib.ptr(sg), _lib.ptr(pr), _lib.ptr(rf), _lib.ptr(mk),
                                           Cn, B, K, S, _lib.ptr(votes), _lib.ptr(cons), _lib.ptr(agree), _lib.ptr(match), _lib.ptr(mmean))
    _lib.check(rc, None, 'iodine_chain_consensus')
    _check_consensus(chains.Consensus(votes, cons, agree, match, mmean), want, Cn, B, K, S)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------
GEN = O.Arch(dim_latent=6, iters=2, slots=16, img_size=24, dec_chan=8, dec_layers=2, ref_chan=8, ref_layers=2, ref_mlp=12)
CONFIGS = {'tiny': O.tiny_arch(slots=4), 'generic_k16': GEN}     # K = 4; K = 16, generic decoder, padded handle (tests/test_gpu_predictive.py)
FIELDS = ('pred', 'mask', 'mean', 'z', 'post_mean', 'post_logvar', 'best', 'score', 'll', 'kl', 'segmentation', 'perm', 'overlap', 'votes',
          'consensus', 'agreement', 'mask_mean', 'match', 'stability')
NB, NC = 2, 3


def _params(arch):
    pn = synth.make_params(O.param_shapes(arch), seed=41, dec_gain=3.0, posterior_scale=0.05)
    return {k: torch.from_numpy(v) for k, v in pn.items()}


@functools.lru_cache(maxsize=None)
def _setup(name):
    arch = CONFIGS[name]
    K, L, T, Si = arch.slots, arch.dim_latent, arch.iters, arch.img_size
    m = make_hip_model(arch, _params(arch))
    imgs, _ = synth.make_images(NB, Si, seed=3, kind='blobs')
    x = torch.from_numpy(imgs).to(DEV)
    eps = torch.randn(NC, T + 1, NB, K, L, generator=torch.Generator().manual_seed(77)).to(DEV)
    res = m.restarts(x, chains=NC, eps=eps, keep_decodes=True)
    return dict(m=m, arch=arch, K=K, L=L, T=T, Si=Si, x=x, eps=eps, res=res)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_restarts_selects_rows_of_one_reconstruct(name):
    c = _setup(name)
    m, x, eps, res, K, L, T, Si = (c[k] for k in ('m', 'x', 'eps', 'res', 'K', 'L', 'T', 'Si'))
    assert res.chains == NC and res.best.shape == (NB,) and res.score.shape == res.ll.shape == res.kl.shape == (NC, NB)
    assert res.segmentation.shape == (NC, NB, Si, Si) and res.perm.shape == (NC, NB, K) and not res.pred.requires_grad
    fresh = m.restarts(x, chains=NC, eps=eps)                                    # the same bits again, and what the call leaves on the module
    for f in FIELDS:
        assert torch.equal(getattr(fresh, f), getattr(res, f)), (name, f)
    assert fresh.decodes is None
    assert torch.equal(m.posterior.mean, res.post_mean) and torch.equal(m.posterior.logvar, res.post_logvar)
    assert m.objects is None and m.trajectory is None
    with pytest.raises(RuntimeError, match='refinement_state'):
        m.refinement_state()
    # the posterior of the chosen mode: a following predictive runs from it
    e1 = torch.randn(2, NB, K, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    o, o2 = m.predictive(x, samples=2, eps=e1), m.predictive(x, samples=2, posterior=(res.post_mean, res.post_logvar), eps=e1)
    assert torch.equal(o.z, o2.z) and torch.equal(o.ll, o2.ll) and torch.equal(o.pred_mean, o2.pred_mean)
    # one reconstruct over the batch repeated chain-major, with the same noise
    big = eps.permute(1, 0, 2, 3, 4).reshape(T + 1, NC * NB, K, L).contiguous()
    pred, mask, mean = m.reconstruct(x.repeat(NC, 1, 1, 1), big)
    z = m.encode(x.repeat(NC, 1, 1, 1), big)
    pm, plv = m.posterior.mean, m.posterior.logvar
    rows = (res.best * NB + torch.arange(NB, device=DEV)).tolist()
    for got, whole in zip((res.pred, res.mask, res.mean, res.z, res.post_mean, res.post_logvar), (pred, mask, mean, z, pm, plv)):
        assert torch.equal(got, whole[rows])
    for got, whole in zip(res.decodes, (pred, mask, mean)):
        assert torch.equal(got.reshape(whole.shape), whole)
    # the score: ll of the RETURNED decode (reference), the closed-form KL, the arg-max with the lowest chain on a tie
    want_ll, scale, want_seg = R.chain_score(x.cpu().numpy(), None, mask.view(NC, NB, K, 1, Si, Si).cpu().numpy(),
                                             mean.view(NC, NB, K, 3, Si, Si).cpu().numpy(), float(m.sigma), False)
    assert (np.abs(res.ll.double().cpu().numpy() - want_ll) <= 1e-6 * scale).all()
    assert np.array_equal(res.segmentation.cpu().numpy(), want_seg)
    kl = (0.5 * (plv.double().exp() + pm.double() ** 2 - 1.0 - plv.double()).sum((-2, -1))).view(NC, NB)
    assert torch.equal(res.kl, kl) and torch.equal(res.score, res.ll.double() - float(m.beta) * kl)
    s = res.score.cpu()
    print(f'{name}: scores {s.tolist()}, best {res.best.tolist()}, stability {res.stability.tolist()}')
    for b in range(NB):
        assert bool((s[res.best[b], b] >= s[:, b]).all()) and int(res.best[b]) == int(s[:, b].argmax())
    # every chain on its own is the computation reconstruct(x, eps[c]) runs: bit for bit, like the image-independence tests
    for ci in range(NC):
        p1, k1, m1 = m.reconstruct(x, eps[ci])
        assert torch.equal(p1, pred[ci * NB:(ci + 1) * NB]) and torch.equal(k1, mask[ci * NB:(ci + 1) * NB]), (name, ci)
        assert torch.equal(m1, mean[ci * NB:(ci + 1) * NB]), (name, ci)

@pytest.mark.parametrize('name', list(CONFIGS))
def test_restarts_consensus_fields(name):
    c = _setup(name)
    res, K, Si = c['res'], c['K'], c['Si']
    seg, perm, best = res.segmentation.cpu().numpy(), res.perm.cpu().numpy(), res.best.cpu().numpy()
    for b in range(NB):
        assert perm[best[b], b].tolist() == list(range(K))                      # the common labelling is the best chain's
        for ci in range(NC):
            assert sorted(perm[ci, b].tolist()) == list(range(K))               # K rows, K columns: a permutation
    seg_best = np.stack([seg[best[b], b] for b in range(NB)])
    want_tab = np.zeros((NC, NB, K, K), np.int64)
    for ci in range(NC):
        for b in range(NB):
            np.add.at(want_tab[ci, b], (seg[ci, b].ravel(), seg_best[b].ravel()), 1)
    assert np.array_equal(res.overlap.cpu().numpy(), want_tab)
    want = R.chain_consensus(seg, perm, best.astype(np.int32), res.decodes[1].cpu().numpy())
    _check_consensus(chains.Consensus(res.votes, res.consensus, res.agreement, res.match, res.mask_mean), want, NC, NB, K, Si)
    match = res.match.double().cpu()
    for b in range(NB):
        assert float(match[best[b], b]) == 1.0
        others = [float(match[ci, b]) for ci in range(NC) if ci != best[b]]
        assert abs(float(res.stability[b]) - sum(others) / len(others)) <= 1e-6
    ari = res.ari()
    assert ari.shape == (NC, NB) and all(float(ari[best[b], b]) == 1.0 for b in range(NB)) and bool((ari <= 1.0 + 1e-12).all())
    # consensus=False stops after the selection
    m = c['m']
    r0 = m.restarts(c['x'], chains=NC, eps=c['eps'], consensus=False)
    assert r0.perm is None and r0.votes is None and r0.stability is None and r0.decodes is None
    for f in FIELDS[:11]:
        assert torch.equal(getattr(r0, f), getattr(res, f)), f
    with pytest.raises(RuntimeError, match='consensus=True'):
        r0.ari()


@pytest.mark.parametrize('name', list(CONFIGS))
def test_restarts_one_chain_and_chunks(name):
    c = _setup(name)
    m, x, eps, res, K = c['m'], c['x'], c['eps'], c['res'], c['K']
    one = m.restarts(x, chains=1, eps=eps[:1])
    pred, mask, mean = m.reconstruct(x, eps[0])
    assert torch.equal(one.pred, pred) and torch.equal(one.mask, mask) and torch.equal(one.mean, mean)
    assert torch.equal(one.post_mean, m.posterior.mean) and int(one.best.abs().max()) == 0
    assert float((one.stability - 1.0).abs().max()) == 0.0 and float((one.agreement - 1.0).abs().max()) == 0.0
    assert torch.equal(one.consensus, one.segmentation[0]) and torch.equal(one.ll[0], res.ll[0])
    # every chain its own chunk: the bits of the unchunked call, every field
    m.set_option('batch_cap', NB)
    try:
        cut = m.restarts(x, chains=NC, eps=eps)
    finally:
        m.set_option('batch_cap', 0)
    for f in FIELDS:
        assert torch.equal(getattr(cut, f), getattr(res, f)), (name, f)
    # weights reach the refinement and the score; the library's own generator is reproducible from the seed
    w = _weights(NB, c['Si']).to(DEV)
    rw = m.restarts(x, chains=2, eps=eps[:2], weights=w, keep_decodes=True)
    assert not torch.equal(rw.ll, res.ll[:2])
    want = R.chain_score(x.cpu().numpy(), w.cpu().numpy(), rw.decodes[1].cpu().numpy(), rw.decodes[2].cpu().numpy(), float(m.sigma), False)
    assert (np.abs(rw.ll.double().cpu().numpy() - want[0]) <= 1e-6 * want[1]).all()
    m.manual_seed(11)
    a = m.restarts(x, chains=2)
    m.manual_seed(11)
    b = m.restarts(x, chains=2)
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS)
    assert not torch.equal(a.z, m.restarts(x, chains=2).z)                       # (the next draw differs)
    # the joint form follows model.likelihood
    m.likelihood = 'joint'
    try:
        rj = m.restarts(x, chains=2, eps=eps[:2], keep_decodes=True)
        wj = R.chain_score(x.cpu().numpy(), None, rj.decodes[1].cpu().numpy(), rj.decodes[2].cpu().numpy(), float(m.sigma), True)
        assert (np.abs(rj.ll.double().cpu().numpy() - wj[0]) <= 1e-6 * wj[1]).all()
    finally:
        m.likelihood = 'per_channel'


# four times the maximum observed on the MI355X, relative to sum_p |w_p LL_p| of the sample (see test_ll_against_predictive)
PREDICTIVE_GAP = {'tiny': 4 * 9.947e-08, 'generic_k16': 4 * 1.524e-07}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_ll_against_predictive(name):
    """An independent implementation of the same likelihood: ``predictive(x, posterior, eps).ll[s]`` for latents z_s against
    ``iodine_chain_score`` on ``decode(z_s)``.  The two take log m differently (log-softmax of the logits inside the per-pixel core, against
    logf(m + 1e-12) of the rendered mask here), so the difference is measured, not derived.  Observed on an MI355X, 5 samples, B = 2, as the
    maximum of |difference| / sum_p |w_p LL_p|: ``tiny`` 7.97e-08 unweighted and 9.95e-08 weighted, ``generic_k16`` 1.13e-07 and 1.52e-07 -
    about one float32 rounding of the sum.  Asserted at four times the larger figure of each configuration: 3.98e-07 and 6.10e-07."""
    c = _setup(name)
    m, x, K, L, Si = c['m'], c['x'], c['K'], c['L'], c['Si']
    g = torch.Generator().manual_seed(200 + len(name))
    pm = torch.randn(NB, K, L, generator=g).to(DEV)
    plv = (0.5 * torch.randn(NB, K, L, generator=g) - 1.0).to(DEV)
    eps = torch.randn(5, NB, K, L, generator=g).to(DEV)
    worst = 0.0
    for weighted in (False, True):
        w = _weights(NB, Si).to(DEV) if weighted else None
        out = m.predictive(x, samples=5, posterior=(pm, plv), eps=eps, weights=w)
        dec = [m.decode(out.z[s]) for s in range(5)]
        mask, mean = torch.stack([d[1] for d in dec]), torch.stack([d[2] for d in dec])
        ll = chains.chain_score(x, mask, mean, float(m.sigma), weights=w)[0]
        scale = R.chain_score(x.cpu().numpy(), None if w is None else w.cpu().numpy(), mask.cpu().numpy(), mean.cpu().numpy(), float(m.sigma), False)[1]
        rel = float((np.abs((ll.double() - out.ll.double()).cpu().numpy()) / scale).max())
        print(f'{name} weighted={weighted}: max |chain_score ll - predictive ll| / sum|w LL| {rel:.3e}')
        worst = max(worst, rel)
    bound = PREDICTIVE_GAP[name]
    assert bound is not None and worst <= bound, (name, worst, bound)


def test_restarts_sheet_colours_follow_perm():
    from iodine_amd import figures
    c = _setup('tiny')
    res, x, K, Si = c['res'], c['x'], c['K'], c['Si']
    sh = figures.restarts_sheet(res, image=1, x=x, panels=('seg',), pad=0, edges=False)
    assert sh.shape == (NC * Si, Si, 3) and sh.dtype == torch.uint8
    pal = torch.tensor(figures.PALETTE, dtype=torch.uint8, device=DEV)
    want = pal[res.perm[:, 1].long().gather(1, res.segmentation[:, 1].reshape(NC, -1).long())].view(NC * Si, Si, 3)
    assert torch.equal(sh, want)
    assert figures.restarts_sheet(res, image=0, x=x).shape[0] == 2 + NC * (Si + 2)


def test_engine_evaluate_restarts():
    from iodine_amd import IODINE, engine
    from iodine_amd.ari import ari_tables, compute_ari
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    dl = make_dataloader(engine.SyntheticScenes(4, 16), batch_size=2, shuffle=False)
    m.manual_seed(3)
    ev0 = engine.evaluate(m, dl, torch.device(DEV))
    aris0, mean0 = list(ev0.aris), ev0.global_mean
    for r in (0, 1):                                                             # the present path, the present bits
        m.manual_seed(3)
        e = engine.evaluate(m, dl, torch.device(DEV), restarts=r)
        assert e.aris == aris0 and e.global_mean == mean0 and not hasattr(e, 'stability')
    m.manual_seed(3)
    ev = engine.evaluate(m, dl, torch.device(DEV), restarts=3)
    assert len(ev.aris) == 4 and all(math.isfinite(v) for v in (ev.stability, ev.best_score, ev.first_score))
    assert 0.0 <= ev.stability <= 1.0 and ev.best_score >= ev.first_score
    # the same numbers by hand, without the proxy
    m.manual_seed(3)
    aris, rows = [], []
    for data in dl:
        res = m.restarts(data[0].to(DEV), chains=3)
        gt = [g.numpy() for g in data[1]]
        tables = ari_tables(res.mask, gt)
        aris += [compute_ari(tables[b, :gt[b].shape[0]]) for b in range(len(gt))]
        best = res.score.gather(0, res.best.view(1, -1))[0]
        rows += list(zip(res.stability.tolist(), best.tolist(), res.score[0].tolist()))
    assert aris == ev.aris and ev.global_mean == float(torch.tensor(aris, dtype=torch.float64).sum() / 4)
    for i, got in enumerate((ev.stability, ev.best_score, ev.first_score)):
        assert abs(got - sum(r[i] for r in rows) / 4) <= 1e-12 * max(1.0, abs(got))
    with pytest.raises(ValueError, match='restarts must be an integer'):
        engine.evaluate(m, dl, torch.device(DEV), restarts=-1)
