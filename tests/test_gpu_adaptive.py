"""iodine_adaptive_select / iodine_adaptive_move, IODINE.reconstruct_adaptive and engine.evaluate(adaptive=...) on the device.

Kernel level: tests/adaptive_reference.py (numpy) - integers and copied floats, so everything is compared bit for bit.  ``select`` at the n
that sit on the wave (64) and block (1024) boundaries of its scan and at several blocks' worth (5000), four stop patterns each, rounds of
1 (the previous score comes from the traces) and 3 evaluations, with and without a budget; ``move`` at row sizes on both sides of the
float4 path, with every pointer one float off, and all kinds in one table.

End to end the contract is: image b of an adaptive call equals, bit for bit, image b of the fixed ``reconstruct`` at ``n_iters = iters[b]``
with the noise rows ``cat(eps[:t], eps[max_iters:])`` - decode, posterior, LSTM state and the per-image ELBO terms.  One fixed call per
distinct t is made, cached and shared by the tests (never modified)."""
import functools
import math

import numpy as np
import pytest
import torch

import adaptive_reference as A
from iodine_amd import _lib, synth
from iodine_amd import adaptive as ad
from oracle import iodine_oracle as O
from util import make_hip_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _off(t):
    """a copy of ``t`` on the device whose storage starts one element past an aligned address"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


# ---- select -----------------------------------------------------------------------------------------------------------------------------
M_SEL = 8
PATTERNS = ('none', 'all', 'alternating', 'scores')


def _select_case(n, R, pattern, with_budget):
    """inputs of one select call after t updates (t = 3 at R = 1: row t - 2 of the traces is read; t = 6 at R = 3)"""
    g = np.random.default_rng(1000 * n + 10 * R + PATTERNS.index(pattern) + (5 if with_budget else 0))
    B, t = n + 7, (3 if R == 1 else 6)
    idx = g.permutation(B)[:n].astype(np.int32)
    ll = np.full((M_SEL, B), np.nan, np.float32)
    kl = np.full((M_SEL, B), np.nan, np.float32)
    ll[:t - R] = g.normal(1000.0, 50.0, (t - R, B)).astype(np.float32)      # what the rounds before left
    kl[:t - R] = g.uniform(0.0, 20.0, (t - R, B)).astype(np.float32)
    terms = np.stack([g.normal(1000.0, 50.0, (R, n)), g.uniform(0.0, 20.0, (R, n))], -1).astype(np.float32)
    tol, rtol = 0.0, 1e-3
    if pattern != 'scores':                                  # the last evaluation = the one before it plus a chosen gain; tol = 50 between
        prev = terms[R - 2] if R >= 2 else np.stack([ll[t - 2, idx], kl[t - 2, idx]], -1)
        gain = {'none': np.full(n, 100.0), 'all': np.zeros(n), 'alternating': np.where(np.arange(n) % 2 == 0, 0.0, 100.0)}[pattern]
        terms[R - 1, :, 0] = prev[:, 0] + gain.astype(np.float32)
        terms[R - 1, :, 1] = prev[:, 1]
        tol, rtol = 50.0, 0.0
    budget = g.integers(1, M_SEL + 1, B).astype(np.int32) if with_budget else None
    if with_budget and pattern == 'none':
        budget[:] = M_SEL
    return dict(B=B, t=t, idx=idx, ll=ll, kl=kl, terms=terms, tol=tol, rtol=rtol, budget=budget, beta=0.5)


def _run_select(c, R):
    dv = lambda a, dt=None: None if a is None else torch.from_numpy(a).to(DEV)
    ll, kl, iters = dv(c['ll'].copy()), dv(c['kl'].copy()), torch.full((c['B'],), -1, dtype=torch.int32, device=DEV)
    out = ad.select(dv(c['terms']), c['t'], iters, ll, kl, tol=c['tol'], rtol=c['rtol'], min_iters=2, check_every=R, beta=c['beta'],
                    idx=dv(c['idx']), budget=dv(c['budget']))
    return out, iters, ll, kl


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_select_against_the_reference(n):
    seen = set()
    for R in (1, 3):
        for pattern in PATTERNS:
            for with_budget in (False, True):
                c = _select_case(n, R, pattern, with_budget)
                ll, kl, iters = c['ll'].copy(), c['kl'].copy(), np.full(c['B'], -1, np.int32)
                want = A.select(c['terms'], c['idx'], c['t'], c['B'], ll, kl, iters, M_SEL, 2, R, c['tol'], c['rtol'], c['beta'], c['budget'])
                (idx_out, pos_out, stop_idx, stop_pos, counts), d_iters, d_ll, d_kl = _run_select(c, R)
                n_c, n_s = (int(v) for v in counts.tolist())
                assert (n_c, n_s) == (len(want[0]), len(want[2])) and n_c + n_s == n, (R, pattern, with_budget)
                for got, w, k in ((idx_out, want[0], n_c), (pos_out, want[1], n_c), (stop_idx, want[2], n_s), (stop_pos, want[3], n_s)):
                    assert np.array_equal(got[:k].cpu().numpy(), w), (R, pattern, with_budget)
                assert np.array_equal(d_iters.cpu().numpy(), iters)
                assert np.array_equal(d_ll.cpu().numpy().view(np.int32), ll.view(np.int32))
                assert np.array_equal(d_kl.cpu().numpy().view(np.int32), kl.view(np.int32))
                if not with_budget:
                    seen.add((pattern, n_s == 0, n_c == 0))
                    if pattern == 'alternating':
                        assert n_s == (n + 1) // 2 and stop_pos[:n_s].tolist() == list(range(0, n, 2))
    # the patterns are what they are called (the score-driven one stops some and keeps some wherever there are enough images)
    assert ('none', True, False) in seen and ('all', False, True) in seen
    assert n < 63 or ('scores', False, False) in seen


def test_select_first_round_all_stop_at_max_iters_and_bad_indices():
    """idx = None is the identity; at t = max_iters everything stops whatever the scores; an index outside the batch addresses nothing"""
    n, B = 70, 70
    terms = torch.zeros(1, n, 2, device=DEV)
    terms[0, :, 0] = torch.arange(n, device=DEV).float()
    ll, kl = (torch.full((4, B), float('nan'), device=DEV) for _ in range(2))
    iters = torch.zeros(B, dtype=torch.int32, device=DEV)
    idx_out, pos_out, stop_idx, stop_pos, counts = ad.select(terms, 1, iters, ll, kl, tol=INF, check_every=1)
    assert counts.tolist() == [n, 0] and idx_out.tolist() == list(range(n)) and pos_out.tolist() == list(range(n))     # t = 1 < 2: no score yet
    assert ll[0].tolist() == list(map(float, range(n))) and torch.isnan(ll[1:]).all() and iters.sum() == 0
    t4 = torch.zeros(1, n, 2, device=DEV)
    ll[:3] = 0.0
    kl[:3] = 0.0
    counts = ad.select(t4, 4, iters, ll, kl, tol=-INF)[4]
    assert counts.tolist() == [0, n] and iters.tolist() == [4] * B
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    idx[5], idx[69] = -1, B
    iters.zero_()
    out = ad.select(t4, 2, iters, ll, kl, tol=-INF, idx=idx)
    assert out[4].tolist() == [n - 2, 2] and out[2][:2].tolist() == [-1, B] and out[3][:2].tolist() == [5, 69] and iters.sum() == 0


def test_select_twice_and_on_a_side_stream_gives_the_same_bits():
    c = _select_case(1025, 3, 'scores', True)
    first = _run_select(c, 3)
    second = _run_select(c, 3)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = _run_select(c, 3)
    side.synchronize()
    n_c, n_s = first[0][4].tolist()
    assert 0 < n_c and 0 < n_s
    for other in (second, third):
        assert other[0][4].tolist() == [n_c, n_s]
        for j, k in ((0, n_c), (1, n_c), (2, n_s), (3, n_s)):
            assert torch.equal(other[0][j][:k], first[0][j][:k])
        assert all(_same(a, b) for a, b in zip(other[1:], first[1:]))


# ---- move -------------------------------------------------------------------------------------------------------------------------------
ROW_FLOATS = (1, 3, 4, 24, 1024 * 4)


def _move_case(w, seed):
    g = np.random.default_rng(seed + w)
    n_src, n_dst, rows = 37, 41, 20
    src = g.normal(size=(n_src, w)).astype(np.float32)
    dst = g.normal(size=(n_dst, w)).astype(np.float32)
    si = g.permutation(n_src)[:rows].astype(np.int32)
    di = g.permutation(n_dst)[:rows].astype(np.int32)
    return src, dst, si, di, rows


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('w', ROW_FLOATS)
def test_move_against_the_reference(w, unaligned):
    put = _off if unaligned else (lambda t: t.to(DEV))
    src, dst, si, di, rows = _move_case(w, 11)
    for use_si, use_di in ((True, True), (True, False), (False, True), (False, False)):
        want = dst.copy()
        A.move([(src, want, si if use_si else None, di if use_di else None, rows)])
        d_src, d_dst = put(torch.from_numpy(src)), put(torch.from_numpy(dst.copy()))
        ad.move([(d_src, d_dst, torch.from_numpy(si).to(DEV) if use_si else None, torch.from_numpy(di).to(DEV) if use_di else None, rows)])
        assert np.array_equal(d_dst.cpu().numpy().view(np.int32), want.view(np.int32)), (use_si, use_di)
        assert np.array_equal(d_src.cpu().numpy().view(np.int32), src.view(np.int32))


@pytest.mark.parametrize('unaligned', [False, True])
def test_move_table_with_every_row_kind(unaligned):
    """all five row sizes in one launch (the float4 and the scalar path side by side), twice and on a side stream: the same bits"""
    put = _off if unaligned else (lambda t: t.to(DEV))
    cases = [_move_case(w, 23) for w in ROW_FLOATS]
    wants = []
    for src, dst, si, di, rows in cases:
        want = dst.copy()
        A.move([(src, want, si, di, rows)])
        wants.append(want)

    def run():
        dsts = [put(torch.from_numpy(c[1].copy())) for c in cases]
        ad.move([(put(torch.from_numpy(c[0])), d, torch.from_numpy(c[2]).to(DEV), torch.from_numpy(c[3]).to(DEV), c[4]) for c, d in zip(cases, dsts)])
        return dsts
    first, second = run(), run()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for got in (first, second, third):
        for d, want in zip(got, wants):
            assert np.array_equal(d.cpu().numpy().view(np.int32), want.view(np.int32))


def test_move_out_of_range_indices_move_nothing_and_overlap_is_refused():
    src = torch.arange(12.0, device=DEV).view(4, 3)
    dst = torch.zeros(5, 3, device=DEV)
    si = torch.tensor([3, 7, -1, 0], dtype=torch.int32, device=DEV)
    di = torch.tensor([1, 2, 3, 9], dtype=torch.int32, device=DEV)
    ad.move([(src, dst, si, di, 4)])
    assert dst.tolist() == [[0, 0, 0], [9, 10, 11], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    buf = torch.zeros(8, 4, device=DEV)
    with pytest.raises(RuntimeError, match='overlap'):
        ad.move([(buf, buf, None, None, 4)])
    with pytest.raises(RuntimeError, match='overlap'):
        ad.move([(buf[:6], buf[2:], None, None, 4)])
    ad.move([(buf[4:], buf[:4], None, None, 4)])             # two halves of one tensor do not overlap


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
GEN = O.Arch(dim_latent=6, iters=2, slots=16, img_size=24, dec_chan=8, dec_layers=2, ref_chan=8, ref_layers=2, ref_mlp=12)
FIELDS = ('pred', 'mask', 'mean', 'z', 'post_mean', 'post_logvar')
BUDGET = [1, 2, 2, 5, 8, 8]


def _weights(B, S):
    """values in [0, 1.75) with a zero rectangle per image (the rectangle weights of tests/test_gpu_restarts.py)"""
    g = torch.Generator().manual_seed(5)
    w = 1.75 * torch.rand(B, 1, S, S, generator=g)
    for b in range(B):
        w[b, :, 2 + b % 3:8 + b % 3, 3:9] = 0.0
    return w.reshape(B, S, S)


@functools.lru_cache(maxsize=None)
def _setup(name):
    arch = O.tiny_arch(slots=3) if name == 'tiny' else GEN
    pn = synth.make_params(O.param_shapes(arch), seed=41, dec_gain=3.0, posterior_scale=0.05)
    m = make_hip_model(arch, {k: torch.from_numpy(v) for k, v in pn.items()})
    K, L, S = arch.slots, arch.dim_latent, arch.img_size
    if name == 'tiny':
        imgs, _ = synth.make_images(4, S, seed=3, kind='blobs')
        x = torch.cat([torch.from_numpy(imgs), torch.full((1, 3, S, S), 0.5), torch.zeros(1, 3, S, S)]).to(DEV)
        M = 8
    else:
        imgs, _ = synth.make_images(3, S, seed=3, kind='blobs')
        x, M = torch.from_numpy(imgs).to(DEV), 4
    B = x.shape[0]
    eps = torch.randn(M + 1, B, K, L, generator=torch.Generator().manual_seed(77)).to(DEV)
    return dict(m=m, x=x, eps=eps, M=M, B=B, K=K, L=L, S=S, fixed={})


def _fixed(c, t, variant=None, state=None, weights=None):
    """the fixed ``reconstruct`` at n_iters = t with the noise rows cat(eps[:t], eps[M:]) and its state; made once per (t, variant)"""
    key = (t, variant)
    if key not in c['fixed']:
        m, saved = c['m'], c['m'].n_iters
        m.n_iters = t
        try:
            # (reconstruct's own call path, which also hands back the final sample z)
            pred, mask, mean, z = m._reconstruct(c['x'], torch.cat([c['eps'][:t], c['eps'][c['M']:]]), trajectory=True, state=state, weights=weights)
            pm, plv, h, cc = m.refinement_state()
            c['fixed'][key] = dict(pred=pred, mask=mask, mean=mean, z=z, post_mean=pm, post_logvar=plv, h=h, c=cc,
                                   ll=m.trajectory['ll'].clone(), kl=m.trajectory['kl'].clone())
        finally:
            m.n_iters = saved
    return c['fixed'][key]


def _check_contract(c, res, variant=None, state=None, weights=None):
    m, M = c['m'], c['M']
    st = m.refinement_state()
    assert _same(st[0], res.post_mean) and _same(st[1], res.post_logvar) and _same(m.posterior.mean, res.post_mean)
    assert m.elbo_terms is None and m.trajectory is None and m.objects is None
    assert res.iters.dtype == torch.int32 and res.ll.shape == res.kl.shape == res.score.shape == (M, c['B']) and res.score.dtype == torch.float64
    iters = res.iters.tolist()
    for b, t in enumerate(iters):
        f = _fixed(c, t, variant, state, weights)
        for name in FIELDS:
            assert _same(getattr(res, name)[b], f[name][b]), (name, b, t)
        assert _same(st[2][b], f['h'][b]) and _same(st[3][b], f['c'][b]), (b, t)
        assert _same(res.ll[:t, b], f['ll'][:, b]) and _same(res.kl[:t, b], f['kl'][:, b]), (b, t)
        assert torch.isnan(res.ll[t:, b]).all() and torch.isnan(res.kl[t:, b]).all()
        assert torch.equal(res.score[:t, b], res.ll[:t, b].double() - float(m.beta) * res.kl[:t, b].double())
    return iters


@pytest.mark.parametrize('R', [1, 2, 3])
def test_budget_schedule_shrinks_the_batch(R):
    c = _setup('tiny')
    bud = torch.tensor(BUDGET, device=DEV)
    res = c['m'].reconstruct_adaptive(c['x'], max_iters=8, budget=bud, check_every=R, eps=c['eps'])
    want = [min(-(-b // R) * R, 8) for b in BUDGET]
    zeros = np.zeros((8, 6), np.float32)
    want_ref, active = A.iterations(zeros, zeros, 1.0, 8, 2, R, -INF, 0.0, np.array(BUDGET))
    assert want_ref.tolist() == want
    assert res.iters.tolist() == want
    assert res.active == active and active[0] == 6 and active[-1] < 6          # the proof that the batch shrank
    assert _check_contract(c, res) == want


@pytest.mark.parametrize('R', [1, 2])
def test_tolerance_rule_follows_the_devices_own_trajectory(R):
    """Expectation: the stopping rule (numpy) on the device's own fixed 8-iteration trajectory.  tol = -1420 nats sits between the
    improvements of these images (checked on the CPU oracle: iters [3, 8, 2, 8, 5, 3] at R = 1, [8, 8, 2, 8, 8, 6] at R = 2, the nearest
    improvement 52 nats from the threshold on values of order 1e3)."""
    c = _setup('tiny')
    f8 = _fixed(c, 8)
    want, active = A.iterations(f8['ll'].cpu().numpy(), f8['kl'].cpu().numpy(), 1.0, 8, 2, R, -1420.0, 0.0)
    print(f'R={R}: expected iters {want.tolist()} active {active}')
    assert len(set(want.tolist())) >= 3 and 8 in want and (want < 8).any(), want
    res = c['m'].reconstruct_adaptive(c['x'], tol=-1420.0, rtol=0.0, max_iters=8, min_iters=2, check_every=R, eps=c['eps'])
    print(f'R={R}: got iters {res.iters.tolist()} active {res.active}')
    assert res.iters.tolist() == want.tolist() and res.active == active
    _check_contract(c, res)


def test_never_and_first_check():
    c = _setup('tiny')
    m = c['m']
    res = m.reconstruct_adaptive(c['x'], tol=-INF, max_iters=8, eps=c['eps'])
    assert res.iters.tolist() == [8] * 6 and res.active == [6] * 8
    _check_contract(c, res)
    f8 = _fixed(c, 8)
    assert all(_same(getattr(res, n), f8[n]) for n in FIELDS) and _same(res.ll, f8['ll']) and _same(res.kl, f8['kl'])
    res = m.reconstruct_adaptive(c['x'], tol=INF, min_iters=3, max_iters=8, eps=c['eps'])
    assert res.iters.tolist() == [3] * 6 and res.active == [6, 6, 6, 0, 0, 0, 0, 0]
    _check_contract(c, res)
    res = m.reconstruct_adaptive(c['x'], tol=-INF, max_iters=8, check_every=8, eps=c['eps'])      # one round of everything
    assert res.iters.tolist() == [8] * 6 and res.active == [6] and _same(res.pred, f8['pred'])


def test_state_in_and_state_out():
    c = _setup('tiny')
    m, x, M = c['m'], c['x'], c['M']
    g = torch.Generator().manual_seed(5)
    e2 = torch.randn(3, 6, c['K'], c['L'], generator=g).to(DEV)
    saved = m.n_iters
    try:
        m.n_iters = 2
        m.reconstruct(x, eps=e2)
        st = m.refinement_state()
        # state=: max_iters further iterations from the state; the fixed continuation is reconstruct(state=st) at n_iters = t
        res = m.reconstruct_adaptive(x, max_iters=8, budget=torch.tensor(BUDGET, device=DEV), eps=c['eps'], state=st)
        assert _check_contract(c, res, variant='state', state=st) == BUDGET
        # refinement_state() afterwards feeds a further reconstruct: for every image what its fixed path gives
        res = m.reconstruct_adaptive(x, max_iters=8, budget=torch.tensor(BUDGET, device=DEV), eps=c['eps'])
        after = m.refinement_state()
        m.n_iters = 2
        out = m.reconstruct(x, eps=e2, state=after)
        for t in sorted(set(BUDGET)):
            f = _fixed(c, t)
            m.n_iters = 2
            o = m.reconstruct(x, eps=e2, state=(f['post_mean'], f['post_logvar'], f['h'], f['c']))
            for b in (b for b, tb in enumerate(BUDGET) if tb == t):
                assert all(_same(a[b], q[b]) for a, q in zip(out, o)), (b, t)
    finally:
        m.n_iters = saved


def test_weights_chunks_repeat_and_graph_mode():
    c = _setup('tiny')
    m, x = c['m'], c['x']
    bud = torch.tensor(BUDGET, device=DEV)
    w = _weights(6, c['S']).to(DEV)
    res = m.reconstruct_adaptive(x, max_iters=8, budget=bud, eps=c['eps'], weights=w)
    _check_contract(c, res, variant='weights', weights=w)
    plain = m.reconstruct_adaptive(x, max_iters=8, budget=bud, check_every=2, eps=c['eps'])
    assert not _same(plain.pred, res.pred)
    names = FIELDS + ('iters', 'll', 'kl')
    again = m.reconstruct_adaptive(x, max_iters=8, budget=bud, check_every=2, eps=c['eps'])
    assert all(_same(getattr(again, n), getattr(plain, n)) for n in names) and again.active == plain.active
    st = m.refinement_state()
    try:
        m.set_option('batch_cap', 4)                         # two chunks of three images
        parts = m.reconstruct_adaptive(x, max_iters=8, budget=bud, check_every=2, eps=c['eps'])
        assert all(_same(getattr(parts, n), getattr(plain, n)) for n in names) and parts.active == plain.active
        assert all(_same(a, b) for a, b in zip(m.refinement_state(), st))
    finally:
        m.set_option('batch_cap', 0)
    try:
        m.set_option('graph', 1)                             # never captured: the eager result
        for _ in range(3):
            graphed = m.reconstruct_adaptive(x, max_iters=8, budget=bud, check_every=2, eps=c['eps'])
            assert all(_same(getattr(graphed, n), getattr(plain, n)) for n in names) and graphed.active == plain.active
        assert m.profile_read('graph_captures')[1] == 0
    finally:
        m.set_option('graph', 0)


@pytest.mark.parametrize('R', [1, 2])
def test_padded_generic_handle(R):
    """K = 16, L = 6, MLP_UNITS = 12 (widths that are no multiple of 4: the padded adapter), generic decoder and refinement stack"""
    c = _setup('generic_k16')
    res = c['m'].reconstruct_adaptive(c['x'], max_iters=4, budget=torch.tensor([1, 3, 4], device=DEV), check_every=R, eps=c['eps'])
    want = [min(-(-b // R) * R, 4) for b in (1, 3, 4)]
    assert res.iters.tolist() == want
    assert _check_contract(c, res) == want


def test_library_refusals_on_a_live_handle():
    c = _setup('tiny')
    m, x = c['m'], c['x']
    m.reconstruct_adaptive(x, tol=-INF, max_iters=2, eps=c['eps'][:3])
    ses = m._session
    with pytest.raises(RuntimeError, match='no iodine_reconstruct has run'):
        ses.call('iodine_last_refine_state', 6, torch.empty(6, 3, 32, device=DEV), torch.empty(6, 3, 32, device=DEV))
    with pytest.raises(RuntimeError, match='no elbo'):
        m._fetch_last_elbo(x, torch.zeros(3))
    import ctypes as C
    ctl = _lib.AdaptiveCtl(4, 2, 2, 0.0, 0.0)               # check_every = 2 on a handle at T = 1
    f = dict(device=DEV, dtype=torch.float32)
    outs = [torch.empty(6, 3, 8, **f) for _ in range(2)] + [torch.empty(6, 3, 32, **f) for _ in range(2)]
    with pytest.raises(RuntimeError, match='must equal check_every'):
        ses.call('iodine_reconstruct_adaptive', 6, x, c['eps'], C.byref(ctl), None, None, None, None, None, None, *outs,
                 torch.empty(6, dtype=torch.int32, device=DEV), torch.empty(4, 6, **f), torch.empty(4, 6, **f), None)


def test_engine_evaluate_adaptive():
    from iodine_amd import IODINE, engine
    from iodine_amd.ari import ari_tables, compute_ari
    from iodine_amd.data import make_dataloader
    from iodine_amd.model import arch_namespace
    torch.manual_seed(0)
    m = IODINE(arch_namespace(8, 2, 3, 16, (32, 2, 32), (32, 2))).to(DEV)
    dl = make_dataloader(engine.SyntheticScenes(4, 16), batch_size=2, shuffle=False)
    opts = dict(tol=0.0, rtol=1e-3, max_iters=4, check_every=1)
    m.manual_seed(3)
    ev = engine.evaluate(m, dl, torch.device(DEV), adaptive=opts)
    a = ev.adaptive
    assert len(ev.aris) == 4 and a['max_iters'] == 4 and len(a['hist']) == 5 and sum(a['hist']) == 4 and a['hist'][0] == a['hist'][1] == 0
    assert abs(a['mean_iters'] - sum(t * n for t, n in enumerate(a['hist'])) / 4) < 1e-12 and a['at_max'] == a['hist'][4] / 4
    assert m.n_iters == 2
    # the same numbers by hand, without the proxy: the metrics are those of the adaptive decodes
    m.manual_seed(3)
    aris, iters = [], []
    for data in dl:
        res = m.reconstruct_adaptive(data[0].to(DEV), **opts)
        gt = [g.numpy() for g in data[1]]
        tables = ari_tables(res.mask, gt)
        aris += [compute_ari(tables[b, :gt[b].shape[0]]) for b in range(len(gt))]
        iters += res.iters.tolist()
    assert aris == ev.aris and [iters.count(t) for t in range(5)] == a['hist']
    assert not hasattr(engine.evaluate(m, dl, torch.device(DEV)), 'adaptive')
    with pytest.raises(ValueError, match='adaptive must be a dict'):
        engine.evaluate(m, dl, torch.device(DEV), adaptive=dict(tolerance=1.0))
    with pytest.raises(ValueError, match='do not combine'):
        engine.evaluate(m, dl, torch.device(DEV), adaptive=opts, restarts=2)
