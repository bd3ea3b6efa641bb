"""Kernel-level parity of the generic path's spatial-broadcast layer (kernels_genl0.hip: decoder layer 0 WITHOUT the broadcast tensor - a
prefix table of per-tap latent products forward, tap-window sums of the gradient backward) against the materialised fp64 layer:
F.conv2d(oracle.spatial_broadcast(z, S), w, b, padding = k // 2), F.elu, and autograd.  The oracle fixes the order of the two coordinate
planes (the goldens pin it to the reference).  Both directions form their sums by CANCELLATION (four corner reads of a prefix table; a row
sum minus its edge pixels), so next to random inputs there are structured ones: latents x 100, and gradients that live only in the border
band, only in the interior, only in the left columns - where a tap whose window misses every populated pixel must come out at rounding
level of the largest tap sum, not as a wrong value.  The case table is imported by test_gen_tiers_cpu.py: no GPU work at import.
Observed on MI355X, relative to each tensor's largest element: forward 3.92e-7 or less (border band and interior alike), dz 3.32e-7, gw 2.20e-7,
gb 1.43e-7, accumulation 1.6e-7; z x 100: 1.26e-7 of max |PS|; taps outside a left-column gradient: exactly 0."""
import functools

import pytest
import torch
import torch.nn.functional as F

from iodine_amd import _lib
from oracle import iodine_oracle as O
from util import nhwc, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.25e9
GATE = 2e-6                                                     # the generic path's gate of exact-fp32 kernels (test_gpu_gen_s2.py)

# (L, co, k, S, N); every co is a multiple of 4 as DEC.CONV_CHAN is: the V = 4 forward
CASES = [(8, 32, 5, 16, 3), (16, 32, 5, 64, 2), (128, 64, 5, 32, 2),   # the last: the `defaults` shapes
         (7, 12, 3, 9, 4), (10, 20, 7, 8, 3),                          # S = k + 1: every pixel's window is clipped
         (6, 8, 7, 24, 2), (64, 64, 3, 40, 7), (2, 256, 5, 17, 1), (13, 36, 5, 33, 2)]
STRUCTURED = [(8, 32, 5, 16, 3), (6, 8, 7, 24, 2)]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _check(rc, what):
    if rc == 2:     # IODINE_ERR_HIP: a launch or kernel failed - the session ends, nothing more runs on a device that may have faulted
        pytest.exit(f'iodine_op_gen_l0, {what}: {_lib.lib().iodine_last_error(None).decode()}', 3)
    _lib.check(rc, None, 'iodine_op_gen_l0')


def _fwd(z, w, b, N, L, S, co, k):
    out = torch.full((N, S, S, co), float('nan'), device=DEV)
    t = [v.to(DEV).contiguous() for v in (z, w, b)]
    _check(_lib.lib().iodine_op_gen_l0(None, 0, _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), None, _lib.ptr(out), None, None, None,
                                       N, L, S, co, k, L, 0.0), f'forward {(L, co, k, S, N)}')
    torch.cuda.synchronize()
    return out.cpu()


def _bwd(z, w, dpre_nchw, N, L, S, co, k, alpha=1.0, gw0=None, gb0=None):
    """-> dz [N][ld] (ld = 9 co as the library passes, or L where that is smaller; sentinel past L), gw, gb"""
    ld = max(L, 9 * co)
    dz = torch.full((N, ld), SENTINEL, device=DEV)
    gw = (torch.zeros(co, L + 2, k, k) if gw0 is None else gw0.clone()).to(DEV)
    gb = (torch.zeros(co) if gb0 is None else gb0.clone()).to(DEV)
    t = [v.to(DEV).contiguous() for v in (z, w, nhwc(dpre_nchw))]
    _check(_lib.lib().iodine_op_gen_l0(None, 1, _lib.ptr(t[0]), _lib.ptr(t[1]), None, _lib.ptr(t[2]), None, _lib.ptr(gw), _lib.ptr(gb),
                                       _lib.ptr(dz), N, L, S, co, k, ld, alpha), f'backward {(L, co, k, S, N)}')
    torch.cuda.synchronize()
    dz = dz.cpu()
    assert bool((dz[:, L:] == SENTINEL).all()), 'dz: the row padding was written'
    return dz[:, :L].contiguous(), gw.cpu(), gb.cpu()


def _inputs(L, co, k, S, N):
    z = _rand(N, L, seed=90)
    w = _rand(co, L + 2, k, k, seed=91, scale=3.0 / ((L + 2) * k * k) ** 0.5)
    b = _rand(co, seed=92, scale=0.5)
    d = _rand(N, co, S, S, seed=93, scale=1e-2)
    return z, w, b, d


def _reference(z, w, b, d, S, k):
    """the materialised layer in fp64: ELU output NHWC; gradients wrt z, w, b of sum(pre * d)"""
    zr, wr, br = (t.double().requires_grad_(True) for t in (z, w, b))
    pre = F.conv2d(O.spatial_broadcast(zr, S), wr, br, padding=k // 2)
    (pre * d.double()).sum().backward()
    return nhwc(F.elu(pre.detach())).float(), zr.grad.float(), wr.grad.float(), br.grad.float()


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs and fp64 reference of a case: computed once, shared by the tests, never modified"""
    L, co, k, S, N = case
    z, w, b, d = _inputs(L, co, k, S, N)
    return (z, w, b, d) + _reference(z, w, b, d, S, k)


def _border(S, k):
    m = torch.ones(S, S, dtype=torch.bool)
    p = k // 2
    if S > 2 * p:
        m[p:S - p, p:S - p] = False
    return m


def _gw_groups(gw, L):
    """the latent channels, the x plane, the y plane: three kernels' worth of sums of different size"""
    return {'latent': gw[:, :L], 'x': gw[:, L], 'y': gw[:, L + 1]}


@pytest.mark.parametrize('case', CASES, ids=str)
def test_gen_l0_forward(case):
    L, co, k, S, N = case
    z, w, b, _, ref = _case(case)[:5]
    out = _fwd(z, w, b, N, L, S, co, k)
    m = _border(S, k)
    e_all, e_border = rel_err(out, ref), rel_err(out[:, m], ref[:, m])
    e_inner = rel_err(out[:, ~m], ref[:, ~m]) if bool((~m).any()) else 0.0
    print(f'[gen l0 fwd] L{L} co{co} k{k} S{S} N{N}: rel err {e_all:.2e}, border band {e_border:.2e}, interior {e_inner:.2e}')
    assert e_all < GATE and e_border < GATE and e_inner < GATE, (e_all, e_border, e_inner)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_gen_l0_backward(case):
    L, co, k, S, N = case
    z, w, b, d, _, r_z, r_w, r_b = _case(case)
    dz, gw, gb = _bwd(z, w, d, N, L, S, co, k)
    e = {'dz': rel_err(dz, r_z), 'gb': rel_err(gb, r_b)}
    for name, g in _gw_groups(gw, L).items():
        e['gw ' + name] = rel_err(g, _gw_groups(r_w, L)[name])
    # second run: bit-identical (fixed summation order)
    dz2, gw2, gb2 = _bwd(z, w, d, N, L, S, co, k)
    same = torch.equal(dz, dz2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # alpha = 0.5 into pre-filled gw / gb (values of the gradient's size): what was added is half the gradient
    pw = _rand(co, L + 2, k, k, seed=94, scale=float(r_w.abs().max()))
    pb = _rand(co, seed=95, scale=float(r_b.abs().max()))
    _, aw, ab = _bwd(z, w, d, N, L, S, co, k, alpha=0.5, gw0=pw, gb0=pb)
    e_acc = max(rel_err((aw.double() - pw.double()) * 2, gw), rel_err((ab.double() - pb.double()) * 2, gb))
    # alpha = 0: dz only, gw / gb bit-unchanged
    dz0, zw, zb = _bwd(z, w, d, N, L, S, co, k, alpha=0.0, gw0=pw, gb0=pb)
    print(f'[gen l0 bwd] L{L} co{co} k{k} S{S} N{N}: ' + ', '.join(f'{n} {v:.2e}' for n, v in e.items()) + f', accumulated {e_acc:.2e}')
    assert all(v < GATE for v in e.values()), e
    assert same
    assert e_acc < 1e-6, e_acc
    assert torch.equal(zw, pw) and torch.equal(zb, pb) and torch.equal(dz0, dz)


def test_gen_l0_forward_large_latents():
    """z x 100: the prefix-table entries are 100 x larger than the coordinate term and the window sum is a four-corner DIFFERENCE of them -
    its error is relative to the largest prefix entry, not to the result: gated against max |PS| (recomputed here in fp64)"""
    L, co, k, S, N = case = CASES[2]
    z, w, b = _case(case)[:3]
    z = z * 100
    ref = _reference(z, w, b, torch.zeros(N, co, S, S), S, k)[0]
    out = _fwd(z, w, b, N, L, S, co, k)
    u = torch.einsum('nl,olyx->noyx', z.double(), w[:, :L].double())             # U[n][co][ky][kx]
    ps_max = float(u.cumsum(2).cumsum(3).abs().max())
    err = float((out.double() - ref.double()).abs().max())
    print(f'[gen l0 fwd, z x 100] L{L} co{co} k{k} S{S}: max err {err:.2e}, max |PS| {ps_max:.2e}, ratio {err / ps_max:.2e}; '
          f'max |out| {float(ref.abs().max()):.2e}')
    assert err < GATE * ps_max, (err, ps_max)


@pytest.mark.parametrize('where', ['border', 'interior', 'left'])
@pytest.mark.parametrize('case', STRUCTURED, ids=str)
def test_gen_l0_backward_structured_gradient(case, where):
    """dpre populated only in the border band of width k // 2, only in the interior, only in the k // 2 left columns.  The row sums are 'full
    sum minus edge pixels': a tap whose window misses the populated pixels (left columns: every tap with kx = 0) is a difference of two equal
    sums taken in different orders - it must be rounding of the largest tap sum, i.e. pass the same element-wise gate against a reference
    that is exactly zero there."""
    L, co, k, S, N = case
    z, w, b, d = _case(case)[:4]
    m = _border(S, k)
    if where == 'interior':
        m = ~m
    elif where == 'left':
        m = torch.zeros(S, S, dtype=torch.bool)
        m[:, :k // 2] = True
    d = d * m
    _, r_z, r_w, r_b = _reference(z, w, b, d, S, k)
    dz, gw, gb = _bwd(z, w, d, N, L, S, co, k)
    e = {'dz': rel_err(dz, r_z), 'gb': rel_err(gb, r_b)}
    for name, g in _gw_groups(gw, L).items():
        e['gw ' + name] = rel_err(g, _gw_groups(r_w, L)[name])
    print(f'[gen l0 bwd, {where} gradient] L{L} co{co} k{k} S{S} N{N}: ' + ', '.join(f'{n} {v:.2e}' for n, v in e.items()))
    if where == 'left':
        assert float(r_w[..., 0].abs().max()) == 0.0           # the window of kx = 0 starts right of the populated columns
        e_out = float(gw[..., 0].abs().max()) / float(r_w.abs().max())
        print(f'    taps outside the populated columns: {e_out:.2e} of the largest tap sum')
        assert e_out < GATE, e_out
    assert all(v < GATE for v in e.values()), e
