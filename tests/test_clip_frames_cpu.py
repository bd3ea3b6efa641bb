"""Video input / resumable refinement, CPU side: the new C-ABI symbols, and the composed clip reference (tests/clip_reference.py)
pinned to the oracle that the goldens pin - plus the proof that the moving-frames inputs of the GPU tests can tell a correct
composition from the three wrong ones a frame-indexing bug would compute."""
import os
import re

import pytest
import torch

import clip_reference as R
from iodine_amd import _lib
from oracle import iodine_oracle as O
from util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('iodine_set_frames', 'iodine_reconstruct_seq', 'iodine_last_refine_state')
SEED = R.SEED
GPU_GATE = 2e-4     # the GPU tests' gate on pred / mask / post_mean


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.iodine_abi_version() == 3


def test_module_surface():
    """signatures only (no device): the new keyword arguments exist with defaults that change nothing"""
    import inspect
    from iodine_amd import IODINE
    sig = inspect.signature(IODINE.reconstruct).parameters
    assert sig['trajectory'].default is False and sig['state'].default is None
    assert inspect.signature(IODINE.encode).parameters['state'].default is None
    assert inspect.signature(IODINE.forward).parameters['state'].default is None
    assert callable(IODINE.refinement_state)


@pytest.mark.parametrize('family', ['tiny16', 'tiny32c64'])
def test_composed_reference_is_the_oracle_on_identical_frames(family):
    arch = O.tiny_arch(slots=3, iters=3) if family == 'tiny16' else O.tiny_arch(slots=3, iters=3, img_size=32, chan=64)
    p = R.params(arch, seed=61)
    x, _ = R.scene(arch, 2, seed=7)
    eps = R.noise(arch, 2, seed=8)
    ref = O.reconstruct(x, eps, p, arch)
    got = R.clip_reconstruct(R.static_clip(x, arch.iters), eps, p, arch)
    for k in ('pred', 'mask', 'mean', 'z', 'post_mean', 'post_logvar', 'elbos', 'kls', 'lls'):
        assert torch.equal(got[k], ref[k]), k
    # the per-image terms are those whose batch means the oracle reports
    assert rel_err(got['traj']['kl'].mean(1), ref['kls']) < 1e-6 and rel_err(got['traj']['ll'].mean(1), ref['lls']) < 1e-6
    out, grads = O.train_step_grads(x, eps, p, arch)
    out_c, grads_c = R.clip_train_step_grads(R.static_clip(x, arch.iters + 1), eps, p, arch)
    assert torch.equal(out_c['loss'], out['loss']) and torch.equal(out_c['elbos'], out['elbos'])
    for n in grads:
        assert torch.equal(grads_c[n], grads[n]), n


def test_continuation_of_the_composed_reference():
    """T = 4 equals T = 2 + T = 2 from the state, in the reference itself (the GPU test asks the library for the same, bitwise)"""
    import dataclasses
    arch = O.tiny_arch(slots=3, iters=4)
    half = dataclasses.replace(arch, iters=2)
    p = R.params(arch, seed=61)
    x, _ = R.scene(arch, 2, seed=7)
    clip, eps = R.moving_clip(x, 4), R.noise(arch, 2, seed=8)
    whole = R.clip_reconstruct(clip, eps, p, arch)
    a = R.clip_reconstruct(clip[:, :2].contiguous(), eps[:3], p, half)
    b = R.clip_reconstruct(clip[:, 2:].contiguous(), eps[2:], p, half, init=a['state'])
    for k in ('pred', 'mask', 'mean', 'post_mean', 'post_logvar'):
        assert torch.equal(b[k], whole[k]), k
    assert torch.equal(b['elbos'], whole['elbos'][2:])
    assert all(torch.equal(s, t) for s, t in zip(b['state'], whole['state']))


def test_moving_frames_tell_the_correct_composition_from_the_wrong_ones():
    """The test can fail: on the moving clip the static run on frame 0, a run that scores frame i but encodes frame 0 and the
    reverse each differ from the correct composition by more than 10 x the GPU gate in pred, mask and post_mean."""
    arch = O.tiny_arch(slots=3, iters=3)
    p = R.params(arch, seed=SEED)
    x, _ = R.scene(arch, 2, seed=SEED + 1)
    clip, eps = R.moving_clip(x, arch.iters), R.noise(arch, 2, seed=SEED + 2)
    good = R.clip_reconstruct(clip, eps, p, arch)
    zero = lambda i: 0
    wrong = dict(static_frame0=O.reconstruct(x, eps, p, arch),
                 score_i_encode_0=R.clip_reconstruct(clip, eps, p, arch, encode=zero),
                 score_0_encode_i=R.clip_reconstruct(clip, eps, p, arch, score=zero))
    assert torch.equal(R.clip_reconstruct(clip, eps, p, arch, score=zero, encode=zero)['pred'], wrong['static_frame0']['pred'])
    bad = []
    for name, w in wrong.items():
        for k in ('pred', 'mask', 'post_mean'):
            e = rel_err(w[k], good[k])
            print(name, k, e)
            if not e > 10 * GPU_GATE:
                bad.append((name, k, e))
    assert not bad, bad
