"""Video input and resumable refinement on the GPU: a clip (B, E, 3, S, S) with one frame per ELBO evaluation, the per-iteration
trajectory, and (lambda, h, c) carried from one call into the next - against the reference composed from the oracle's pieces
(tests/clip_reference.py), and bit for bit against the library's own static / single-call results where the launches are the same
kernels on the same values.

Scene: synth blobs, frame i = the scene rolled by (i, 2 i) pixels; parameters as in tests/test_gpu_runshape.py.  Gates of the
comparisons with the reference are those of test_gpu_runshape.py (_check_reconstruct, _train_vs_oracle)."""
import dataclasses
import functools

import pytest
import torch

import clip_reference as R
from clip_reference import SEED
from iodine_amd import _lib
from oracle import iodine_oracle as O
from util import grad_views, make_hip_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 2
PRECS = pytest.mark.parametrize('prec', [1, 0], ids=['split_f16x3', 'exact_fp32'])
FAMS = pytest.mark.parametrize('family', ['tiny16', 'tiny32c64'])


def _arch(family, iters=3, slots=3):
    if family == 'tiny16':                     # 16 x 16, 32 channels: pixel_pass2 writes the encoding
        return O.tiny_arch(slots=slots, iters=iters)
    if family == 'tiny16_L6':                  # DIM_LATENT 6: the padded inner handle
        return dataclasses.replace(O.tiny_arch(slots=slots, iters=iters), dim_latent=6)
    return O.tiny_arch(slots=slots, iters=iters, img_size=32, chan=64)      # weight-stationary convs, refine_l0_fused


@functools.lru_cache(maxsize=None)
def _setup(family, iters=3, slots=3, extra=0):
    """(arch, params, scene, clip of iters + extra moving frames, eps) - computed once, shared, never modified"""
    arch = _arch(family, iters, slots)
    x, _ = R.scene(arch, B, seed=SEED + 1)
    return arch, R.params(_arch(family), seed=SEED), x, R.moving_clip(x, iters + extra), R.noise(arch, B, seed=SEED + 2)


@functools.lru_cache(maxsize=None)
def _ref_reconstruct(family, iters=3, slots=3):
    arch, p, _, clip, eps = _setup(family, iters, slots)
    return R.clip_reconstruct(clip, eps, p, arch)


@functools.lru_cache(maxsize=None)
def _ref_train(family):
    arch, p, _, clip, eps = _setup(family, 3, 3, 1)
    return R.clip_train_step_grads(clip, eps, p, arch)


def _model(family, prec=1, options=None):
    arch, p = _arch(family), _setup(family)[1]
    return make_hip_model(arch, p, options=dict({'conv_precision': prec}, **(options or {})))


def _check_vs_reference(m, clip, eps, ref, K, T, tag):
    """the checks and gates of test_gpu_runshape._check_reconstruct, on a clip"""
    xd, ed = clip.to(DEV), eps.to(DEV)
    pred, mask, mean = m.reconstruct(xd, ed)
    S = clip.shape[-1]
    assert tuple(mask.shape) == (B, K, 1, S, S) and tuple(m.elbo_terms.shape) == (T, 3)
    checks = [('elbo', rel_err(m.elbo_terms[:, 0].cpu(), ref['elbos']), 1e-4), ('kl', rel_err(m.elbo_terms[:, 1].cpu(), ref['kls']), 1e-4),
              ('pred', rel_err(pred.cpu(), ref['pred']), 2e-4), ('mask', rel_err(mask.cpu(), ref['mask']), 2e-4),
              ('mean', rel_err(mean.cpu(), ref['mean']), 2e-4),
              ('post_mean', rel_err(m.posterior.mean.cpu(), ref['post_mean']), 2e-4),
              ('post_logvar', rel_err(m.posterior.logvar.cpu(), ref['post_logvar']), 2e-4),
              ('self.mask', rel_err(m.mask.cpu(), ref['last_mask']), 2e-4), ('self.mean', rel_err(m.mean.cpu(), ref['last_mean']), 2e-4)]
    agree = (mask[:, :, 0].argmax(1).cpu() == ref['mask'][:, :, 0].argmax(1)).float().mean().item()
    z = m.encode(xd, ed)
    checks.append(('z', rel_err(z.cpu(), ref['z']), 2e-4))
    for n, e, tol in checks:
        print(tag, n, e)
    bad = [(tag, n, e) for n, e, tol in checks if not e < tol]
    if not agree >= 0.999:
        bad.append((tag, 'argmax', agree))
    from iodine_amd.model import logger
    if clip.dim() == 5 and not torch.equal(logger['image'].cpu(), clip[0, T - 1]):
        bad.append((tag, 'logger image'))
    return bad


# ---- 1. a clip against the composed reference ---------------------------------------------------------------------------------
@PRECS
@FAMS
def test_clip_matches_composed_reference(family, prec):
    arch, _, _, clip, eps = _setup(family)
    m = _model(family, prec)
    bad = _check_vs_reference(m, clip, eps, _ref_reconstruct(family), arch.slots, arch.iters, (family, prec))
    assert not bad, bad


@PRECS
def test_clip_at_ten_slots_takes_the_unfused_encoding(prec):
    """K' = 10 > 9 at 64 channels: pixel_pass2 + two convs instead of the fused encoding / first layer"""
    arch, _, _, clip, eps = _setup('tiny32c64', 3, 10)
    m = _model('tiny32c64', prec)
    m.K = 10
    bad = _check_vs_reference(m, clip, eps, _ref_reconstruct('tiny32c64', 3, 10), 10, 3, ('K10', prec))
    assert not bad, bad


@PRECS
def test_clip_through_the_padded_handle(prec):
    arch, _, _, clip, eps = _setup('tiny16_L6')
    m = _model('tiny16_L6', prec)
    bad = _check_vs_reference(m, clip, eps, _ref_reconstruct('tiny16_L6'), arch.slots, arch.iters, ('L6', prec))
    assert not bad, bad


# ---- 2. E identical frames are the static call, bit for bit -------------------------------------------------------------------
def _recon_state(m, x, eps, **kw):
    out = [t.clone() for t in m.reconstruct(x, eps, **kw)]
    return out + [m.posterior.mean.clone(), m.posterior.logvar.clone(), m.elbo_terms.clone(), m.z.clone(), m.mask.clone(), m.mean.clone()]


def _train_flat(m, x, eps):
    m.zero_grad(set_to_none=True)
    loss = m(x, eps)
    loss.backward()
    return loss.detach().clone(), torch.cat([p.grad.flatten() for p in m.parameters()]), m.elbo_terms.clone()


@PRECS
@FAMS
def test_identical_frames_are_the_static_call_bitwise(family, prec):
    arch, _, x, _, eps = _setup(family)
    T = arch.iters
    m = _model(family, prec)
    xd, ed = x.to(DEV), eps.to(DEV)
    a = _recon_state(m, xd, ed)
    b = _recon_state(m, R.static_clip(x, T).to(DEV), ed)
    assert all(torch.equal(s, t) for s, t in zip(a, b)), [torch.equal(s, t) for s, t in zip(a, b)]
    la, ga, ea = _train_flat(m, xd, ed)
    lb, gb, eb = _train_flat(m, R.static_clip(x, T + 1).to(DEV), ed)
    assert torch.equal(la, lb) and torch.equal(ea, eb) and torch.equal(ga, gb)


# ---- 3. trajectory ------------------------------------------------------------------------------------------------------------
@PRECS
@FAMS
def test_trajectory_bitwise_and_against_reference(family, prec):
    arch, _, _, clip, eps = _setup(family)
    T, K, S = arch.iters, arch.slots, arch.img_size
    m = _model(family, prec)
    xd, ed = clip.to(DEV), eps.to(DEV)
    plain = [t.clone() for t in m.reconstruct(xd, ed)]
    assert m.trajectory is None
    pred, mask, mean = m.reconstruct(xd, ed, trajectory=True)
    tr = m.trajectory
    assert all(torch.equal(s, t) for s, t in zip(plain, (pred, mask, mean)))       # asking for it changes nothing else
    assert tuple(tr['pred'].shape) == (T + 1, B, 3, S, S) and tuple(tr['mask'].shape) == (T + 1, B, K, 1, S, S)
    assert tuple(tr['mean'].shape) == (T + 1, B, K, 3, S, S) and tuple(tr['kl'].shape) == (T, B) and tuple(tr['ll'].shape) == (T, B)
    assert torch.equal(tr['pred'][T], pred) and torch.equal(tr['mask'][T], mask) and torch.equal(tr['mean'][T], mean)
    assert torch.equal(tr['mask'][T - 1], m.mask) and torch.equal(tr['mean'][T - 1], m.mean)
    terms = m.elbo_terms.clone()
    assert rel_err(tr['kl'].mean(1).cpu(), terms[:, 1].cpu()) < 1e-6 and rel_err(tr['ll'].mean(1).cpu(), terms[:, 2].cpu()) < 1e-6
    ref = _ref_reconstruct(family)['traj']
    for k in ('kl', 'll'):
        e = rel_err(tr[k].cpu(), ref[k])
        print(family, prec, k, e)
        assert e < 1e-4, (k, e)
    for k in ('pred', 'mask', 'mean'):                       # (not asked for bitwise: against the reference at the tensors' gate)
        assert rel_err(tr[k].cpu(), ref[k]) < 2e-4, k
    tr = {k: v.clone() for k, v in tr.items()}
    for i in range(1, T):                                    # entry i = the final decode of the same model at n_iters = i
        m.n_iters = i
        out = m.reconstruct(xd[:, :i].contiguous(), ed[:i + 1].contiguous())
        for k, t in zip(('pred', 'mask', 'mean'), out):
            assert torch.equal(tr[k][i], t), (i, k)
    m.n_iters = T
    m.reconstruct(xd, ed)
    assert m.trajectory is None


# ---- 4. continuation ----------------------------------------------------------------------------------------------------------
NAMES = ('pred', 'mask', 'mean', 'post_mean', 'post_logvar', 'elbo_terms', 'state.pm', 'state.plv', 'state.h', 'state.c')


def _whole(m, clip, eps, **kw):
    """T = 4 in one call: the final tuple, the posterior, the last two rows of the ELBO terms, the state"""
    m.n_iters = 4
    out = [t.clone() for t in m.reconstruct(clip, eps, **kw)]
    return out + [m.posterior.mean.clone(), m.posterior.logvar.clone(), m.elbo_terms[2:].clone()] + list(m.refinement_state())


def _continued(m, clip, eps, **kw):
    """T = 2 on frames 0-1, then T = 2 from the state on frames 2-3"""
    m.n_iters = 2
    m.reconstruct(clip[:, :2].contiguous(), eps[:3].contiguous(), **kw)
    state = m.refinement_state()
    out = [t.clone() for t in m.reconstruct(clip[:, 2:].contiguous(), eps[2:].contiguous(), state=state)]
    return out + [m.posterior.mean.clone(), m.posterior.logvar.clone(), m.elbo_terms.clone()] + list(m.refinement_state())


@pytest.mark.parametrize('mode', ['eager', 'graph', 'chunked', 'padded'])
@PRECS
def test_continuation_is_the_long_call_bitwise(prec, mode):
    family = 'tiny16_L6' if mode == 'padded' else 'tiny32c64'
    arch, _, _, clip, eps = _setup(family, 4)
    xd, ed = clip.to(DEV), eps.to(DEV)
    w = _whole(_model(family, prec), xd, ed)                 # one un-chunked eager call: an independent path for every mode
    assert tuple(w[-1].shape) == (B, arch.slots, arch.ref_mlp) and tuple(w[-4].shape) == (B, arch.slots, arch.dim_latent)
    kw = {}
    if mode == 'chunked':
        # a chunked call copies its chunks' LSTM states out only when asked to (keep_state); everything per image is the un-chunked
        # call's, bit for bit, while the ELBO terms of a chunked call are the size-weighted fp32 means of its chunks' terms: those
        # are compared with a chunked T = 4 call
        kw = dict(keep_state=True)
        chunked = _model(family, prec, options={'batch_cap': 1})
        wc = _whole(chunked, xd, ed, **kw)
        bad = [n for n, s, t in zip(NAMES, wc, w) if n != 'elbo_terms' and not torch.equal(s, t)]
        assert not bad, bad
        assert rel_err(wc[5].cpu(), w[5].cpu()) < 1e-6       # to fp32 summation order
        w[5] = wc[5]
        chunked.reconstruct(xd, ed)
        with pytest.raises(RuntimeError, match='keep_state'):
            chunked.refinement_state()
    m = _model(family, prec, options={'graph': 1} if mode == 'graph' else {'batch_cap': 1} if mode == 'chunked' else None)
    with torch.cuda.stream(torch.cuda.Stream()):
        for rep in range(3 if mode == 'graph' else 1):       # graph: eager, captured, replayed
            c = _continued(m, xd, ed, **kw)
            torch.cuda.synchronize()
            bad = [(rep, n) for n, s, t in zip(NAMES, c, w) if not torch.equal(s, t)]
            assert not bad, bad
    if mode == 'graph':
        assert m.profile_read('graph_replays')[1] > 0
    # the state is the reference's too
    ref = _ref_reconstruct(family, 4)
    for n, s, t in zip(NAMES[6:], c[6:], ref['state']):
        assert rel_err(s.cpu(), t) < 2e-4, n


def test_forward_ends_the_state_of_an_earlier_reconstruct():
    arch, _, x, clip, eps = _setup('tiny16')
    m = _model('tiny16')
    xd, ed = clip.to(DEV), eps.to(DEV)
    m.reconstruct(xd, ed)
    held = m.refinement_state()
    m.decode(m.z)                                            # a state once fetched outlives single-pass calls ...
    assert all(torch.equal(s, t) for s, t in zip(held, m.refinement_state()))
    m.reconstruct(xd, ed)
    m.decode(m.z)                                            # ... one still in the workspace does not
    with pytest.raises(RuntimeError, match='re-used the workspace'):
        m.refinement_state()
    m.reconstruct(xd, ed)
    m.refinement_state()
    m(x.to(DEV), ed)
    with pytest.raises(RuntimeError, match='no encode / reconstruct'):
        m.refinement_state()


# ---- 5. training on a clip ----------------------------------------------------------------------------------------------------
@PRECS
@FAMS
def test_training_on_a_clip_matches_autograd_through_the_reference(family, prec):
    arch, _, _, clip, eps = _setup(family, 3, 3, 1)
    T = arch.iters
    out, grads = _ref_train(family)
    m = _model(family, prec)
    for chunked in ((False, True) if family == 'tiny16' else (False,)):
        m.set_option('batch_cap', 1 if chunked else 0)
        m.zero_grad(set_to_none=True)
        loss = m(clip.to(DEV), eps.to(DEV))
        loss.backward()
        m.set_option('batch_cap', 0)
        print(family, prec, chunked, 'loss', loss.item(), out['loss'].item())
        assert abs(loss.item() - out['loss'].item()) <= 1e-5 * abs(out['loss'].item()), chunked
        assert tuple(m.elbo_terms.shape) == (T + 1, 3)
        assert rel_err(m.elbo_terms[:, 0].cpu(), out['elbos']) < 1e-4
        errs = [(n, rel_l2(*grad_views(n, p.grad.cpu().numpy(), grads[n].numpy()))) for n, p in m.named_parameters()]
        print(family, prec, chunked, max(e for _, e in errs))
        bad = [(n, e) for n, e in errs if not e < 1e-3]
        assert not bad, (chunked, bad)
        assert rel_err(m.mask.cpu(), out['final_mask']) < 2e-4


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_launch_and_leave_the_model_usable():
    family = 'tiny16'
    arch, p, x, clip, eps = _setup(family)
    T, K = arch.iters, arch.slots
    m = _model(family)
    xd, ed = clip.to(DEV), eps.to(DEV)
    m.reconstruct(xd, ed)
    state = m.refinement_state()
    with pytest.raises(RuntimeError, match=r'\(B, 3, 3, 16, 16\)'):                 # wrong frame count: names the expected shape
        m.reconstruct(xd[:, :2].contiguous(), ed)
    with pytest.raises(RuntimeError, match=r'\(B, 4, 3, 16, 16\)'):
        m(xd, ed)                                                                    # forward makes T + 1 evaluations
    with pytest.raises(RuntimeError, match='state'):
        m.reconstruct(xd, ed, state=tuple(t[:1] for t in state))                     # another B
    with pytest.raises(RuntimeError, match='state'):
        m.reconstruct(xd, ed, state=tuple(t[:, :2] for t in state))                  # another K
    with pytest.raises(RuntimeError, match='state'):
        m(xd, ed, state=state)
    m.set_option('stop_after_iters', 1)
    with pytest.raises(RuntimeError, match='stop_after_iters'):
        m.reconstruct(xd, ed, trajectory=True)
    m.set_option('stop_after_iters', -1)
    # the library's own refusals: return codes with a message
    import ctypes as C
    L, h = _lib.lib(), m._handle
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.iodine_set_frames(h, -1) == 1
    assert L.iodine_set_frames(h, T + 2) == 0
    f = dict(device=DEV, dtype=torch.float32)
    pm = torch.empty((B, K, arch.dim_latent), **f)
    args = [_lib.ptr(xd), _lib.ptr(ed), None, None, None, None, _lib.ptr(pm), None, None]
    assert L.iodine_reconstruct(h, st, B, *args) == 1 and b'(B, 3, 3, 16, 16)' in L.iodine_last_error(h)
    loss = torch.empty((), **f)
    assert L.iodine_train_forward(h, st, B, _lib.ptr(xd), _lib.ptr(ed), _lib.ptr(loss), None) == 1
    assert b'(B, 4, 3, 16, 16)' in L.iodine_last_error(h)
    assert L.iodine_set_frames(h, T) == 0
    half = (C.c_void_p * 4)(pm.data_ptr(), pm.data_ptr(), None, None)                # lambda without the LSTM state
    assert L.iodine_reconstruct_seq(h, st, B, *args, half, None) == 1 and b'four' in L.iodine_last_error(h)
    part = (C.c_void_p * 5)(None, None, None, pm.data_ptr(), pm.data_ptr())          # trajectory buffers missing
    assert L.iodine_reconstruct_seq(h, st, B, *args, None, part) == 1 and b'five' in L.iodine_last_error(h)
    torch.cuda.synchronize()
    # a following static reconstruct still passes the gates of check 1
    ref = O.reconstruct(x, eps, p, arch)
    ref = dict(ref, last_mask=None, last_mean=None)
    xs = x.to(DEV)
    pred, mask, mean = m.reconstruct(xs, ed)
    for n, got, want, tol in (('elbo', m.elbo_terms[:, 0], ref['elbos'], 1e-4), ('kl', m.elbo_terms[:, 1], ref['kls'], 1e-4),
                              ('pred', pred, ref['pred'], 2e-4), ('mask', mask, ref['mask'], 2e-4), ('mean', mean, ref['mean'], 2e-4),
                              ('post_mean', m.posterior.mean, ref['post_mean'], 2e-4), ('post_logvar', m.posterior.logvar, ref['post_logvar'], 2e-4),
                              ('z', m.encode(xs, ed), ref['z'], 2e-4)):
        assert rel_err(got.cpu(), want) < tol, n
    assert (mask[:, :, 0].argmax(1).cpu() == ref['mask'][:, :, 0].argmax(1)).float().mean() >= 0.999
