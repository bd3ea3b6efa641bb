"""IODINE.predictive / iodine_predictive on the device.

The yardstick for everything per pixel is the code every pull request before this one ran, on inputs that are bit-identical on both sides:
``model.decode(out.z[s])`` per sample, reduced in float64 (mean, population variance, arg-max counts through ``slot_table``), and
``model.elbo`` / ``weighted_elbo`` per sample for the likelihood.

Bounds of the moments.  The samples are fp32 values v_s in [0, 1] (pred, mask), u = 2^-24.  One sequential Welford step in fp32,
``mean += (v - mean) / n``, is three rounded operations on numbers of magnitude <= 1: it adds at most 3 u to the error of the mean, so
after S steps |mean - exact mean| <= 3 S u.  One step of ``M2 += (v - mean_old) (v - mean_new)`` rounds two differences, one product and
one sum of magnitude <= S (4 u relative to a term <= 1, the running sum rounded once more as it grows) and inherits the error of the two
means, each entering times a factor <= 1: per step at most (4 + 6 S) u in units of the variance's own scale once M2 is divided by S -
|M2 / S - exact variance| <= (4 + 6 S) u.  Asserted at twice those: atol 6 S 2^-24 on the means, (8 + 12 S) 2^-24 on the variances; the
observed maxima are printed.

Likelihood.  ``ll[s, b]`` and the sum over (c, p) of ``w_p log_likelihood[b]`` after ``weighted_elbo(x, w, eps=eps[s])`` evaluate the same
expression in a different but equivalent order, a few ulp per term: |diff| <= 1e-6 sum |w_p ll_c(p)|.  The batch mean of ``ll[s]`` and the
reported ``elbo_terms[0, 2]`` share the per-pixel core and the fp64 partial sums and differ in the final fp32 roundings: 2^-21 relative."""
import dataclasses
import functools

import pytest
import torch

from iodine_amd import _lib, synth
from iodine_amd.objects import slot_table
from oracle import iodine_oracle as O
from util import make_hip_model

import predictive_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24

GEN = O.Arch(dim_latent=6, iters=2, slots=16, img_size=24, dec_chan=8, dec_layers=2, ref_chan=8, ref_layers=2, ref_mlp=12)
# name -> (arch, options, B); K = arch.slots
CONFIGS = {
    'tiny': (O.tiny_arch(slots=4), {}, 2),                                      # P = 256: exactly one block
    'dsprites': (O.dsprites_arch(slots=4, iters=2), {}, 2),
    'dsprites_fp32': (O.dsprites_arch(slots=4, iters=2), {'conv_precision': 0}, 3),   # strict per-pixel arithmetic
    'clevr': (O.clevr_arch(slots=3, iters=2), {}, 1),
    'generic_k16': (GEN, {}, 2),                                                # generic decoder, padded handle (L = 6), P = 576: a partial block;
    'generic_k1': (dataclasses.replace(GEN, slots=1), {}, 3),                   # K = 16: mask moments and votes in global memory
}
S_MAX = 5
FIELDS = ('z', 'pred_mean', 'pred_var', 'mask_mean', 'mask_var', 'votes', 'segmentation', 'agreement', 'll', 'log_w', 'iwae', 'elbo_mc', 'elbo')


def _params(arch):
    pn = synth.make_params(O.param_shapes(arch), seed=41, dec_gain=3.0, posterior_scale=0.05)
    return {k: torch.from_numpy(v) for k, v in pn.items()}


def _weights(B, S):
    """values in [0, 1.75) with a zero rectangle per image: zeros and values above 1"""
    g = torch.Generator().manual_seed(5)
    w = 1.75 * torch.rand(B, 1, S, S, generator=g)
    for b in range(B):
        w[b, :, 2 + b:8 + b, 3:9] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _setup(name):
    """One configuration, made once and shared (read-only): the model, its inputs, the un-capped 5-sample call with an image and the
    per-sample ``decode(out.z[s])`` of the parent's code"""
    arch, options, B = CONFIGS[name]
    K, L, Si = arch.slots, arch.dim_latent, arch.img_size
    m = make_hip_model(arch, _params(arch), options=options)
    g = torch.Generator().manual_seed(200 + len(name))
    pm = torch.randn(B, K, L, generator=g).to(DEV)
    plv = (0.5 * torch.randn(B, K, L, generator=g) - 1.0).to(DEV)
    eps = torch.randn(S_MAX, B, K, L, generator=g).to(DEV)
    imgs, _ = synth.make_images(B, Si, seed=3, kind='blobs')
    x = torch.from_numpy(imgs).to(DEV)
    out = m.predictive(x, samples=S_MAX, posterior=(pm, plv), eps=eps)
    dec = [m.decode(out.z[s]) for s in range(S_MAX)]
    return dict(m=m, arch=arch, B=B, K=K, L=L, Si=Si, pm=pm, plv=plv, eps=eps, x=x, out=out, dec=dec)


def _same(a, b, what):
    for f in FIELDS:
        p, q = getattr(a, f), getattr(b, f)
        assert (p is None) == (q is None), (what, f)
        if p is not None:
            assert p.dtype == q.dtype and torch.equal(p, q), (what, f)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_samples_are_the_bits_of_elbo_and_decode(name):
    c = _setup(name)
    m, out, K, B, Si = c['m'], c['out'], c['K'], c['B'], c['Si']
    assert out.z.shape == (S_MAX, B, K, c['L']) and out.votes.dtype == torch.int32 and out.segmentation.dtype == torch.uint8
    assert out.log_w.dtype == torch.float64 and out.samples == S_MAX and not out.pred_mean.requires_grad
    saved = (m.posterior.mean, m.posterior.logvar)
    try:
        m.posterior.mean, m.posterior.logvar = c['pm'], c['plv']
        for s in range(S_MAX):
            m.elbo(c['x'], eps=c['eps'][s])
            assert torch.equal(out.z[s], m.z), (name, s)
    finally:
        m.posterior.mean, m.posterior.logvar = saved
    # one sample: the moments ARE that sample's decode, both variances exactly 0, the votes the one-hot of the segmentation
    o1 = m.predictive(samples=1, posterior=(c['pm'], c['plv']), eps=c['eps'][:1])
    pred, mask, mean = c['dec'][0]
    assert o1.ll is None and o1.iwae is None and torch.equal(o1.z[0], out.z[0])
    print(f'{name} S=1: max |pred_mean - decode pred| {float((o1.pred_mean - pred).abs().max()):.3e}, max |mask_mean - decode mask| '
          f'{float((o1.mask_mean - mask).abs().max()):.3e}')
    assert torch.equal(o1.pred_mean, pred) and torch.equal(o1.mask_mean, mask)
    assert float(o1.pred_var.abs().max()) == 0.0 and float(o1.mask_var.abs().max()) == 0.0
    seg = slot_table(mask, mean, segmentation=True)[1]
    assert torch.equal(o1.segmentation, seg)
    onehot = (torch.arange(K, device=DEV).view(1, K, 1, 1) == seg[:, None].long()).to(torch.int32)
    assert torch.equal(o1.votes, onehot) and float((o1.agreement - 1.0).abs().max()) == 0.0


@pytest.mark.parametrize('S', [2, 5])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_moments_and_votes(name, S):
    c = _setup(name)
    m, K = c['m'], c['K']
    out = c['out'] if S == S_MAX else m.predictive(c['x'], samples=S, posterior=(c['pm'], c['plv']), eps=c['eps'][:S])
    assert torch.equal(out.z, c['out'].z[:S])                                   # (so the per-sample decodes of _setup are this call's)
    preds = torch.stack([c['dec'][s][0] for s in range(S)]).double()
    masks = torch.stack([c['dec'][s][1] for s in range(S)]).double()
    assert float(preds.min()) >= 0.0 and float(preds.max()) <= 1.0 + 8 * U and float(masks.min()) >= 0.0 and float(masks.max()) <= 1.0 + 8 * U
    for what, got_mean, got_var, v in (('pred', out.pred_mean, out.pred_var, preds), ('mask', out.mask_mean, out.mask_var, masks)):
        e_mean = float((got_mean.double() - v.mean(0)).abs().max())
        e_var = float((got_var.double() - v.var(0, unbiased=False)).abs().max())
        print(f'{name} S={S} {what}: max |mean err| {e_mean:.3e} (bound {6 * S * U:.3e}), max |var err| {e_var:.3e} (bound {(8 + 12 * S) * U:.3e}), '
              f'max var {float(got_var.max()):.3e}')
        assert e_mean <= 6 * S * U and e_var <= (8 + 12 * S) * U, (name, S, what, e_mean, e_var)
        assert float(got_var.min()) >= 0.0
    if K > 1:
        assert float(out.mask_var.max()) > 1e-4                                 # (the masks do vary over the samples: not vacuous)
    # votes: exact counts of the segmentation maps of slot_table over the samples
    segs = torch.stack([slot_table(c['dec'][s][1], c['dec'][s][2], segmentation=True)[1] for s in range(S)]).long()
    want = (segs[:, :, None] == torch.arange(K, device=DEV).view(1, 1, K, 1, 1)).sum(0).to(torch.int32)
    assert torch.equal(out.votes, want)
    assert torch.equal(out.votes.sum(1), torch.full_like(out.votes[:, 0], S))
    top = out.votes.max(1)
    assert torch.equal(out.agreement, top.values.float() / S)
    assert torch.equal(out.votes.gather(1, out.segmentation[:, None].long())[:, 0], top.values)
    first = ((out.votes == top.values[:, None]).cumsum(1) == 0).sum(1)          # the lowest slot that holds the maximum
    assert torch.equal(out.segmentation.long(), first)


@pytest.mark.parametrize('name', ['tiny', 'dsprites_fp32', 'generic_k16', 'generic_k1'])
def test_chunk_invariance(name):
    c = _setup(name)
    m, B, K, L, Si = c['m'], c['B'], c['K'], c['L'], c['Si']
    w = _weights(B, Si).to(DEV)
    full = m.predictive(c['x'], samples=S_MAX, posterior=(c['pm'], c['plv']), eps=c['eps'], weights=w)
    assert torch.equal(full.pred_mean, c['out'].pred_mean) and not torch.equal(full.ll, c['out'].ll)
    try:
        for cap, what in ((B, 'five chunks of one sample'), (2 * B, 'chunks of 2, 2 and 1 samples')):
            m.set_option('batch_cap', cap)
            _same(m.predictive(c['x'], samples=S_MAX, posterior=(c['pm'], c['plv']), eps=c['eps'], weights=w), full, (name, what))
        if B > 1:                                                               # a cap below the batch: groups of images, each in chunks
            m.set_option('batch_cap', B - 1)
            g = m.predictive(c['x'], samples=S_MAX, posterior=(c['pm'], c['plv']), eps=c['eps'], weights=w)
            for f in FIELDS:                                                    # (the float64 host reductions run on other shapes: rounding)
                if f in ('log_w', 'iwae', 'elbo_mc', 'elbo'):
                    assert torch.allclose(getattr(g, f), getattr(full, f), rtol=1e-13, atol=0.0), (name, 'image groups', f)
                else:
                    assert torch.equal(getattr(g, f), getattr(full, f)), (name, 'image groups', f)
    finally:
        m.set_option('batch_cap', 0)
    # the raw entry with chunk_images = batch, the weights through iodine_set_pixel_weights
    m.decode(c['out'].z[0])                                                     # workspace of B images on the handle
    f = dict(device=DEV, dtype=torch.float32)
    z, ll = torch.empty(S_MAX, B, K, L, **f), torch.empty(S_MAX, B, **f)
    pmean, pm2 = torch.empty(B, 3, Si, Si, **f), torch.empty(B, 3, Si, Si, **f)
    mmean, mm2 = torch.empty(B, K, 1, Si, Si, **f), torch.empty(B, K, 1, Si, Si, **f)
    votes = torch.empty(B, K, Si, Si, device=DEV, dtype=torch.int32)
    wc = w.reshape(B, Si, Si).contiguous()
    _lib.check(_lib.lib().iodine_set_pixel_weights(m._handle, _lib.ptr(wc), 0), m._handle)
    rc = _lib.lib().iodine_predictive(m._handle, _lib.stream(), B, S_MAX, _lib.ptr(c['pm']), _lib.ptr(c['plv']), _lib.ptr(c['eps']), _lib.ptr(c['x']), B,
                                      _lib.ptr(z), _lib.ptr(pmean), _lib.ptr(pm2), _lib.ptr(mmean), _lib.ptr(mm2), _lib.ptr(votes), _lib.ptr(ll))
    _lib.check(rc, m._handle, 'iodine_predictive')
    for got, want in ((z, full.z), (pmean, full.pred_mean), (pm2 / S_MAX, full.pred_var), (mmean, full.mask_mean), (mm2 / S_MAX, full.mask_var),
                      (votes, full.votes), (ll, full.ll)):
        assert torch.equal(got, want)
    # outputs the caller does not ask for keep their running state in the workspace: the others are the same bits
    v2 = torch.empty_like(votes)
    m2b = torch.empty_like(mm2)
    rc = _lib.lib().iodine_predictive(m._handle, _lib.stream(), B, S_MAX, _lib.ptr(c['pm']), _lib.ptr(c['plv']), _lib.ptr(c['eps']), None, B,
                                      None, None, None, None, _lib.ptr(m2b), _lib.ptr(v2), None)
    _lib.check(rc, m._handle, 'iodine_predictive')
    assert torch.equal(v2, full.votes) and torch.equal(m2b, mm2)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_likelihood_against_the_single_sample_elbo(name, weighted):
    c = _setup(name)
    m, B, Si = c['m'], c['B'], c['Si']
    w = _weights(B, Si).to(DEV) if weighted else None
    out = m.predictive(c['x'], samples=S_MAX, posterior=(c['pm'], c['plv']), eps=c['eps'], weights=w) if weighted else c['out']
    saved = (m.posterior.mean, m.posterior.logvar, m.likelihood_maps)
    try:
        m.posterior.mean, m.posterior.logvar, m.likelihood_maps = c['pm'], c['plv'], True
        for s in range(S_MAX):
            m.weighted_elbo(c['x'], w, eps=c['eps'][s])
            terms = (m.log_likelihood.double() * (w.double() if weighted else 1.0))
            ref, scale = terms.sum((1, 2, 3)), terms.abs().sum((1, 2, 3))
            d = (out.ll[s].double() - ref).abs()
            mean_ll, rep = float(out.ll[s].double().mean()), float(m.elbo_terms[0, 2])
            print(f'{name} weighted={weighted} s={s}: max |ll - sum of maps| / scale {float((d / scale).max()):.3e} (bound 1e-6), '
                  f'batch mean {mean_ll:.6f} vs reported {rep:.6f}: rel {abs(mean_ll - rep) / abs(rep):.3e} (bound {2.0 ** -21:.3e})')
            assert bool((d <= 1e-6 * scale).all()), (name, s, d, scale)
            assert abs(mean_ll - rep) <= 2.0 ** -21 * abs(rep), (name, s, mean_ll, rep)
    finally:
        m.posterior.mean, m.posterior.logvar, m.likelihood_maps = saved


@pytest.mark.parametrize('name', list(CONFIGS))
def test_bounds_are_the_reference_host_arithmetic(name):
    c = _setup(name)
    out = c['out']
    r = R.bounds(out.ll.cpu(), out.z.cpu(), c['eps'].cpu(), c['pm'].cpu(), c['plv'].cpu())
    for f in ('log_w', 'iwae', 'elbo_mc', 'elbo'):
        got = getattr(out, f).cpu()
        assert got.dtype == torch.float64 and got.shape == r[f].shape
        assert torch.allclose(got, r[f], rtol=1e-12, atol=1e-9), (name, f, float((got - r[f]).abs().max()))
    assert bool((out.iwae >= out.elbo_mc).all())


@pytest.mark.parametrize('name', ['tiny', 'dsprites_fp32'])
def test_whole_chain_against_the_float64_oracle(name):
    """The established single-sample yardstick: the error of ``model.elbo``'s reported LL against the oracle on the same inputs, measured
    here; the batch mean of the new ``ll[s]`` may be off by twice that.  mean_s / mean_b are linear, so the batch means of ``elbo_mc`` and
    ``elbo`` inherit that bound plus the fp32 rounding of z in the latent part, |d z| <= 4 u (|mu| + sigma |eps|) per entry (one fma, expf to
    2 ulp), times |z| in z^2 / 2; logsumexp is 1-Lipschitz in the sup norm, so ``iwae`` moves by at most max_s |d log_w|."""
    c = _setup(name)
    m, arch, out, B = c['m'], c['arch'], c['out'], c['B']
    p64 = {k: v.double() for k, v in _params(arch).items()}
    x, pm, plv, eps = (t.double().cpu() for t in (c['x'], c['pm'], c['plv'], c['eps']))
    r = R.predictive(x, None, pm, plv, eps, p64, arch)
    saved = (m.posterior.mean, m.posterior.logvar)
    e_old = e_new = 0.0
    try:
        m.posterior.mean, m.posterior.logvar = c['pm'], c['plv']
        for s in range(S_MAX):
            m.elbo(c['x'], eps=c['eps'][s])
            want = float(r['ll'][s].mean())
            e_old = max(e_old, abs(float(m.elbo_terms[0, 2]) - want))
            e_new = max(e_new, abs(float(out.ll[s].double().mean()) - want))
    finally:
        m.posterior.mean, m.posterior.logvar = saved
    print(f'{name}: |batch-mean LL - oracle|: model.elbo {e_old:.4e}, predictive {e_new:.4e} (LL about {float(r["ll"].mean()):.1f})')
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    lat = float((4 * U * r['z'].abs() * (pm.abs()[None] + (0.5 * plv).exp()[None] * eps.abs())).sum((-2, -1)).max())
    for f in ('elbo_mc', 'elbo'):
        d = abs(float(getattr(out, f).mean().cpu()) - float(r[f].mean()))
        print(f'{name}: |batch-mean {f} - oracle| {d:.4e} (bound {2 * e_old + lat:.4e})')
        assert d <= 2.0 * e_old + lat, (f, d, e_old, lat)
    d_w = float((out.log_w.cpu() - r['log_w']).abs().max())
    d_i = float((out.iwae.cpu() - r['iwae']).abs().max())
    print(f'{name}: max |log_w - oracle| {d_w:.4e}, max |iwae - oracle| {d_i:.4e}')
    assert d_i <= d_w * (1 + 1e-9) + 1e-9
    assert torch.equal(out.votes.cpu().long().sum(1), r['votes'].sum(1))


def test_raw_entry_refuses_before_any_launch():
    c = _setup('tiny')
    m, B, K, L, Si = c['m'], c['B'], c['K'], c['L'], c['Si']
    m.decode(c['out'].z[0])
    pz = torch.full((2, B, K, L), -7.0, device=DEV)
    pmean = torch.full((B, 3, Si, Si), -7.0, device=DEV)
    pll = torch.full((2, B), -7.0, device=DEV)
    pv = torch.full((B, K, Si, Si), -7, device=DEV, dtype=torch.int32)
    eps2 = c['eps'][:2].contiguous()

    def call(n=2, batch=B, chunk=0, x=c['x'], ll=pll, eps=eps2, plv=c['plv']):
        return _lib.lib().iodine_predictive(m._handle, _lib.stream(), batch, n, _lib.ptr(c['pm']), _lib.ptr(plv), _lib.ptr(eps), _lib.ptr(x), chunk,
                                            _lib.ptr(pz), _lib.ptr(pmean), None, None, None, _lib.ptr(pv), _lib.ptr(ll))
    err = lambda: _lib.lib().iodine_last_error(m._handle).decode()
    assert call(n=0) == 1 and 'n_samples' in err()
    assert call(n=-2) == 1 and 'n_samples' in err()
    assert call(n=2 ** 24 + 1) == 1 and 'n_samples' in err() and 'int32' in err()
    assert call(chunk=B - 1) == 1 and 'chunk_images' in err()
    assert call(x=None) == 1 and 'll' in err() and 'x is NULL' in err()
    assert call(eps=None) == 1 and 'eps' in err()
    assert call(plv=None) == 1 and 'post_logvar' in err()
    assert call(batch=0) == 1 and 'batch' in err()
    assert call(batch=2 ** 30) == 1 and '2^31' in err()
    assert call(chunk=2 ** 30) == 1 and '2^31' in err()
    assert _lib.lib().iodine_predictive(None, None, 1, 1, *([None] * 4), 0, *([None] * 7)) == 1
    torch.cuda.synchronize()
    for t in (pz, pmean, pll):
        assert float((t + 7.0).abs().max()) == 0.0                              # nothing was launched
    assert int((pv + 7).abs().max()) == 0
    assert call() == 0                                                          # and the same call, un-poisoned, runs
    torch.cuda.synchronize()
    assert torch.equal(pz, c['out'].z[:2]) and torch.equal(pll, c['out'].ll[:2])


def test_call_state_and_graph_option():
    c = _setup('tiny')
    m, arch, B, K = c['m'], c['arch'], c['B'], c['K']
    post = (c['pm'], c['plv'])
    e = torch.from_numpy(synth.make_eps(arch.iters, B, K, arch.dim_latent, seed=4)).to(DEV)
    saved = (m.posterior.mean, m.posterior.logvar)
    try:
        m.reconstruct(c['x'], e)
        z0, mask0 = m.z, m.mask
        o = m.predictive(c['x'], samples=2, eps=c['eps'][:2])                   # the posterior the reconstruct left
        assert m.z is z0 and m.mask is mask0                                    # self.z / mean / mask are not touched
        assert o.z.shape[0] == 2 and o.iwae.shape == (B,)
        st = m.refinement_state()                                               # the LSTM state of the reconstruct is still there
        assert len(st) == 4 and bool(torch.isfinite(st[2]).all())
        m.reconstruct(c['x'], e)
        st2 = m.refinement_state()
        assert all(torch.equal(a, b) for a, b in zip(st, st2))
    finally:
        m.posterior.mean, m.posterior.logvar = saved
    # a saved differentiable decode is discarded
    zg = c['out'].z[0].clone().requires_grad_(True)
    pred = m.decode(zg)[0]
    m.predictive(samples=1, posterior=post, eps=c['eps'][:1])
    with pytest.raises(RuntimeError, match='stale decode'):
        pred.sum().backward()
    m.zero_grad(set_to_none=True)
    # no posterior on the module, none given
    m.posterior.mean = m.posterior.logvar = None
    try:
        with pytest.raises(RuntimeError, match='no posterior'):
            m.predictive(c['x'], samples=2)
    finally:
        m.posterior.mean, m.posterior.logvar = saved
    # option graph: the call is not captured, runs eagerly and returns the same bits
    m.set_option('graph', 1)
    try:
        for _ in range(3):
            _same(m.predictive(c['x'], samples=S_MAX, posterior=post, eps=c['eps']), c['out'], 'graph')
        assert m.profile_read('graph_captures')[1] == 0
    finally:
        m.set_option('graph', 0)
    # the library's own generator: one draw per sample, reproducible from the seed
    m.manual_seed(9)
    a = m.predictive(c['x'], samples=3, posterior=post)
    m.manual_seed(9)
    b = m.predictive(c['x'], samples=3, posterior=post)
    _same(a, b, 'seeded')
    assert not torch.equal(a.z[0], a.z[1])
    # sigma is read per call; beta plays no part
    s0, b0 = m.sigma, m.beta
    try:
        m.beta = 4.0
        _same(m.predictive(c['x'], samples=S_MAX, posterior=post, eps=c['eps']), c['out'], 'beta')
        m.sigma = torch.tensor([2.0 * float(s0)])
        o2 = m.predictive(c['x'], samples=S_MAX, posterior=post, eps=c['eps'])
        assert torch.equal(o2.pred_mean, c['out'].pred_mean) and not torch.equal(o2.ll, c['out'].ll)
    finally:
        m.sigma, m.beta = s0, b0
    _same(m.predictive(c['x'], samples=S_MAX, posterior=post, eps=c['eps']), c['out'], 'sigma restored')


def test_engine_evaluate_reports_the_bounds():
    import math

    from iodine_amd import IODINE, engine
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    dl = make_dataloader(engine.SyntheticScenes(4, 16), batch_size=2, shuffle=False)
    m.manual_seed(3)
    ev0 = engine.evaluate(m, dl, torch.device(DEV))
    assert not hasattr(ev0, 'iwae') and len(ev0.aris) == 4
    m.manual_seed(3)
    ev0b = engine.evaluate(m, dl, torch.device(DEV), bound_samples=0)
    assert ev0b.aris == ev0.aris and ev0b.global_mean == ev0.global_mean and not hasattr(ev0b, 'iwae')
    m.manual_seed(3)
    ev = engine.evaluate(m, dl, torch.device(DEV), bound_samples=2)
    assert len(ev.aris) == 4 and math.isfinite(ev.iwae) and math.isfinite(ev.elbo_mc) and ev.iwae >= ev.elbo_mc
