"""Host-side checks of the refinement restarts (IODINE.restarts, iodine_chain_score / iodine_chain_consensus): header and exports, the numpy
definition the GPU tests compare against - its likelihood against the oracle's expression, its consensus on constructed cases -, the
refusals of the wrapper and of the two entry points, all before any device work.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import joint_reference as J
import restarts_reference as R
from iodine_amd import _lib
from oracle import iodine_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                      # IODINE_ERR_INVALID
NEW = ('iodine_chain_score', 'iodine_chain_consensus')


def _declaration(header, name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\);', header)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_exports_and_bindings_agree():
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    assert '#define IODINE_ABI_VERSION 3' in header and L.iodine_abi_version() == 3          # additive: the ABI version stays
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        args = _declaration(header, name)
        argtypes = _lib._SYMBOLS[name][0]
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):                                                     # pointer / int / double, position by position
            want = C.c_void_p if '*' in a else C.c_double if a.startswith('double ') else C.c_int
            assert t is want, (name, a, t)
    assert _declaration(header, 'iodine_chain_score')[:5] == ['void* stream', 'const float* x', 'const float* w_or_null', 'const float* mask',
                                                               'const float* mean']
    assert 'VOTES SUM TO LESS THAN C' in header and 'iodine.py:213-216, 661-666' in header
    import iodine_amd
    from iodine_amd import chains, model
    assert iodine_amd.Restarts is model.Restarts and iodine_amd.chain_score is chains.chain_score
    assert 'kernels_chains.hip' in __import__('iodine_amd.build', fromlist=['SOURCES']).SOURCES


def _decode(B=2, K=4, S=6, seed=0):
    g = np.random.default_rng(seed)
    x = g.random((B, 3, S, S))
    mask = g.random((B, K, 1, S, S)) ** 3
    mask /= mask.sum(1, keepdims=True)
    mask[0, 1, 0, 2, 3] = 0.0                               # an exact zero: log(0 + 1e-12)
    mean = g.random((B, K, 3, S, S))
    return x, mask, mean


@pytest.mark.parametrize('joint', [False, True])
def test_reference_ll_is_the_oracles_likelihood(joint):
    """``O.gaussian_log_likelihood`` + torch.logsumexp, as O.elbo_terms / joint_reference.joint_ll_px compose them, in float64"""
    x, mask, mean = _decode()
    sigma = 0.13
    w = np.random.default_rng(1).random((2, 6, 6)) * 1.75
    tx, tm, tu = (torch.from_numpy(t) for t in (x, mask, mean))
    k_ll = O.gaussian_log_likelihood(tx[:, None], tu, sigma)
    px = J.joint_ll_px(tm, k_ll) if joint else torch.logsumexp(torch.log(tm + 1e-12) + k_ll, dim=1)
    want_px = px.sum(1).numpy()
    got_px = R.pixel_ll(x, mask, mean, sigma, joint)
    assert got_px.shape == want_px.shape == (2, 6, 6)
    assert np.abs(got_px - want_px).max() <= 1e-13 * np.abs(want_px).max()
    ll, scale, seg = R.chain_score(x, w, np.stack([mask, mask[:, ::-1]]), np.stack([mean, mean[:, ::-1]]), sigma, joint)
    want = (w * want_px).sum((1, 2))
    assert ll.shape == (2, 2) and np.abs(ll[0] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(ll[1] - ll[0]).max() <= 1e-12 * np.abs(want).max()                         # a mixture does not depend on the slot order
    assert (scale >= np.abs(ll)).all()
    assert np.array_equal(seg[0], mask[:, :, 0].argmax(1)) and np.array_equal(seg[1], 3 - seg[0])
    assert R.top_two_gap(mask) > 0.0


def test_reference_argmax_rules():
    m = np.full((1, 1, 3, 1, 2, 2), 0.25, np.float32)
    m[0, 0, 2, 0, 0, 0] = 0.5                               # a clear winner, ties elsewhere
    m[0, 0, 0, 0, 1, 1] = np.nan                            # a NaN never wins: slot 1 takes the tie of the rest
    seg = R.chain_score(np.zeros((1, 3, 2, 2)), None, m, np.zeros((1, 1, 3, 3, 2, 2)), 0.1, False)[2]
    assert seg[0, 0].tolist() == [[2, 0], [0, 1]]
    assert R.top_two_gap(m[..., :1, :1]) == 0.25 and R.top_two_gap(m[..., :1, 1:]) == 0.0


def _permuted_copies(C=4, B=2, K=5, S=7, seed=3):
    g = np.random.default_rng(seed)
    base = g.integers(0, K, (B, S, S)).astype(np.uint8)     # the common labelling
    seg = np.zeros((C, B, S, S), np.uint8)
    perm = np.zeros((C, B, K), np.int32)
    for c in range(C):
        for b in range(B):
            q = g.permutation(K)                            # chain c calls common slot j  q[j]
            seg[c, b] = q[base[b]]
            perm[c, b, q] = np.arange(K)                    # slot i = q[j] of the chain is slot j of the common labelling
    return base, seg, perm


def test_consensus_of_permuted_copies():
    C, B, K, S = 4, 2, 5, 7
    base, seg, perm = _permuted_copies(C, B, K, S)
    mask = np.eye(K)[seg.astype(int)].transpose(0, 1, 4, 2, 3)[:, :, :, None]               # one-hot soft masks (C,B,K,1,S,S)
    r = R.chain_consensus(seg, perm, np.array([2, 0], np.int32), mask)
    assert np.array_equal(r['consensus'], base.reshape(B, -1))
    assert (r['agreement'] == 1.0).all() and (r['match'] == 1.0).all()
    assert np.array_equal(r['votes'].sum(1), np.full((B, S * S), C))
    assert np.array_equal(r['mask_mean'], np.eye(K)[base.reshape(B, -1).astype(int)].transpose(0, 2, 1))
    # out-of-range labels and perm entries are left out: fewer votes there, and only there
    seg2, perm2 = seg.copy(), perm.copy()
    seg2[1, 0, 0, 0] = K                                    # one pixel of chain 1
    seg2[3, 1, 2, 2] = 255
    lost = int(seg[0, 1, 3, 3])
    perm2[0, 1, lost] = K + 3                               # every pixel chain 0 of image 1 labels `lost`
    perm2[2, 0, int(seg[2, 0, 6, 6])] = -1
    r2 = R.chain_consensus(seg2, perm2, np.array([2, 7], np.int32), mask)
    total = r2['votes'].sum(1).reshape(B, S, S)
    assert total[0, 0, 0] < C and total[1, 2, 2] < C and total[1, 3, 3] == C - 1 and total[0, 6, 6] < C
    assert total.max() == C and (total == C).sum() > 0 and (total < C).sum() == int((r2['relabelled'] < 0).any(0).sum())
    assert (r2['match'][:, 1] == 0.0).all()                 # ref 7 is no chain
    assert r2['match'][2, 0] < 1.0                          # the reference chain itself loses the pixels its perm entry drops
    assert r2['mask_mean'].sum(1).max() <= 1.0 + 1e-12 and r2['mask_mean'].sum(1).min() < 1.0
    # a tie goes to the lowest index: two chains, two different labels
    t = R.chain_consensus(np.array([[[[1]]], [[[0]]]], np.uint8), np.tile(np.arange(2, dtype=np.int32), (2, 1, 1)))
    assert t['consensus'].tolist() == [[0]] and t['agreement'].tolist() == [[0.5]] and t['votes'][0, :, 0].tolist() == [1, 1]


def _model():
    from util import golden_setup, hip_arch, load_golden
    from iodine_amd import IODINE
    arch = golden_setup(load_golden('tiny'))[0]
    return IODINE(hip_arch(arch)), arch


def test_restarts_refuses_bad_arguments_without_a_device():
    m, arch = _model()
    B, K, T, L, S = 2, arch.slots, arch.iters, arch.dim_latent, arch.img_size
    x = torch.rand(B, 3, S, S)
    for bad in (0, -1, 2.0, True, '3', None, 1025):
        with pytest.raises(ValueError, match='chains must be an integer'):
            m.restarts(x, chains=bad)
    with pytest.raises(ValueError, match='a clip is not supported'):
        m.restarts(torch.rand(B, T, 3, S, S), chains=2)
    with pytest.raises(ValueError, match='x must be images'):
        m.restarts(torch.rand(B, 3, S, S + 1), chains=2)
    with pytest.raises(ValueError, match='state= and trajectory='):
        m.restarts(x, chains=2, trajectory=True)
    with pytest.raises(ValueError, match='state= and trajectory='):
        m.restarts(x, chains=2, state=tuple(torch.zeros(B, K, L) for _ in range(4)))
    for shape in ((T + 1, B, K, L), (3, T + 1, B, K, L), (2, T, B, K, L), (2, T + 1, B, K, L + 1)):
        with pytest.raises(ValueError, match='eps must have shape'):
            m.restarts(x, chains=2, eps=torch.zeros(shape))
    with pytest.raises(ValueError, match='eps must have shape'):
        m.restarts(x, chains=2, eps=[0.0])
    m.K = 17
    with pytest.raises(ValueError, match='slot count'):
        m.restarts(x, chains=2)
    m.K = K
    # well-formed arguments get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match='ROCm device'):
        m.restarts(x, chains=2, eps=torch.zeros(2, T + 1, B, K, L))
    assert m.posterior.mean is None and m.objects is None


def test_python_wrappers_refuse_before_the_device():
    from iodine_amd import chains
    x, mask, mean = torch.rand(2, 3, 8, 8), torch.rand(3, 2, 4, 1, 8, 8), torch.rand(3, 2, 4, 3, 8, 8)
    with pytest.raises(ValueError, match='mask must be'):
        chains.chain_score(x, mask[0], mean, 0.1)
    with pytest.raises(ValueError, match='mean must be'):
        chains.chain_score(x, mask, mean[:2], 0.1)
    with pytest.raises(ValueError, match='sigma must be > 0'):
        chains.chain_score(x, mask, mean, 0.0)
    with pytest.raises(RuntimeError, match='ROCm device'):
        chains.chain_score(x, mask, mean, 0.1)
    seg, perm = torch.zeros(3, 2, 8, 8, dtype=torch.uint8), torch.zeros(3, 2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match='perm must be int32'):
        chains.chain_consensus(seg, perm.long())
    with pytest.raises(ValueError, match='ref must be int32'):
        chains.chain_consensus(seg, perm, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='ROCm device'):
        chains.chain_consensus(seg, perm)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every one of these returns IODINE_ERR_INVALID before a launch, with the argument named: the pointers are never dereferenced on the
    host, so dummy non-null addresses stand in for device memory."""
    L = _lib.lib()
    p, null, st = C.c_void_p(4096), None, C.c_void_p(0)
    err = lambda: L.iodine_last_error(None).decode()

    def score(x=p, w=null, mask=p, mean=p, chains=2, batch=1, slots=3, size=8, sigma=0.1, joint=0, ll=p, seg=p):
        return L.iodine_chain_score(st, x, w, mask, mean, chains, batch, slots, size, sigma, joint, ll, seg)
    cases = [(dict(x=null), 'x is NULL'), (dict(mask=null), 'mask is NULL'), (dict(mean=null), 'mean is NULL'),
             (dict(chains=0), 'chains'), (dict(chains=-4), 'chains'), (dict(chains=1025), 'chains'), (dict(batch=0), 'batch'),
             (dict(batch=2 ** 31 - 1), 'chains * batch'), (dict(slots=0), 'slots'), (dict(slots=17), 'slots'), (dict(size=0), 'size'),
             (dict(size=1025), 'size'), (dict(sigma=0.0), 'sigma'), (dict(sigma=-1.0), 'sigma'), (dict(sigma=float('nan')), 'sigma'),
             (dict(joint=2), 'joint'), (dict(joint=-1), 'joint'), (dict(ll=null, seg=null), 'both NULL')]
    for kw, word in cases:
        assert score(**kw) == INVALID, kw
        assert err().startswith('iodine_chain_score: ') and word in err(), (kw, err())

    def fold(seg=p, perm=p, ref=p, mask=p, chains=2, batch=1, slots=3, size=8, votes=p, cons=p, agree=p, match=p, mmean=p):
        return L.iodine_chain_consensus(st, seg, perm, ref, mask, chains, batch, slots, size, votes, cons, agree, match, mmean)
    cases = [(dict(seg=null), 'seg is NULL'), (dict(perm=null), 'perm is NULL'), (dict(chains=0), 'chains'), (dict(chains=1025), 'chains'),
             (dict(batch=0), 'batch'), (dict(batch=2 ** 31 - 1), 'chains * batch'), (dict(slots=0), 'slots'), (dict(slots=17), 'slots'),
             (dict(size=0), 'size'), (dict(size=1025), 'size'), (dict(ref=null), 'match needs ref'), (dict(mask=null), 'mask_mean needs mask'),
             (dict(votes=null, cons=null, agree=null, match=null, mmean=null), 'all NULL')]
    for kw, word in cases:
        assert fold(**kw) == INVALID, kw
        assert err().startswith('iodine_chain_consensus: ') and word in err(), (kw, err())
