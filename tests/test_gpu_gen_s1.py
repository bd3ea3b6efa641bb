"""Kernel-level parity of the generic path's STRIDE-1 convolutions (kernels_generic.hip) against PyTorch-CPU fp64 convs: what the decoder of
the reference's default architecture (DEC.KERNEL_SIZE 5, lib/config/defaults.py:100) and of configs/test.yaml runs on - the exact-fp32 MFMA
forward / data gradient at its three chunk widths, the three weight-gradient forms, the GEMM-form weight gradient of the 4-channel output
conv at its four NP instantiations, and the scalar kernels (which also carry REF.STRIDE 3..8).  Every case
  - asserts the tier it is meant to hit (iodine_op_gen_conv_tier: the selector the launchers switch on), so that a changed LDS budget cannot
    move it onto another kernel unnoticed;
  - compares every output element with fp64, with NaN in the padding channels of the inputs and NaN in the outputs before the call;
  - has a guard band of 4096 floats behind every output, which must come back untouched;
  - runs each direction twice: bit-equal (fixed summation order).
Conventions of test_gpu_gen_s2.py (inputs, layouts, gates).  The case table is imported by test_gen_tiers_cpu.py: no GPU work at import."""
import pytest
import torch
import torch.nn.functional as F

from iodine_amd import _lib
from util import nhwc, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4096
SENTINEL = -7.25e9

# iodine_op_gen_conv_tier's values (include/iodine_hip.h)
TIER = {'cch16': 0, 'cch8': 1, 'cch4': 2, 's2': 3, 'scalar': 4, 'out': 5, 'rows': 6, 'wmfma': 7}

# (ci, ldc, co, k, S, N, forward tier, data-gradient tier, weight-gradient tier, NP of the 'out' form or 0)
CASES = [
    (64, 64, 64, 5, 40, 2, 'cch16', 'cch16', 'rows', 0),        # the reference's default decoder layer
    (80, 80, 80, 5, 24, 2, 'cch8', 'cch8', 'rows', 0),          # chunk 8 by step-down (the 16-channel chunk no longer fits the LDS)
    (32, 32, 32, 7, 24, 2, 'cch8', 'cch8', 'rows', 0),          # 7 x 7: chunk 8 by rule
    (44, 44, 44, 7, 16, 3, 'cch4', 'cch4', 'rows', 0),          # 7 x 7: chunk 4 by step-down; 44 = 2.75 chunks of 16
    (256, 256, 256, 3, 40, 1, 'cch4', 'cch4', 'wmfma', 0),      # chunk 4 by step-down at 3 x 3
    (4, 4, 8, 5, 9, 3, 'cch4', 'cch8', 'rows', 0),              # <= 4 reduction channels
    (64, 64, 64, 7, 16, 2, 'scalar', 'scalar', 'rows', 0),      # scalar tier: the slice does not fit the LDS
    (96, 96, 96, 5, 16, 2, 'scalar', 'scalar', 'rows', 0),
    (17, 20, 32, 3, 16, 3, 'scalar', 'cch16', 'rows', 0),       # first refinement layer at REF.STRIDE 1: scalar forward by channel padding
    (17, 20, 32, 5, 16, 2, 'scalar', 'cch16', 'rows', 0),
    (32, 32, 64, 5, 17, 2, 'cch16', 'cch16', 'rows', 0),        # rectangular
    (12, 12, 20, 5, 23, 3, 'cch16', 'cch16', 'rows', 0),
    (128, 128, 128, 3, 72, 1, 'cch16', 'cch16', 'wmfma', 0),    # weight gradient: the per-tap fallback form
    (64, 64, 4, 3, 40, 2, 'cch16', 'cch4', 'out', 1),           # output conv, NP = 1
    (8, 8, 4, 3, 8, 3, 'cch8', 'cch4', 'out', 1),
    (64, 64, 4, 5, 33, 2, 'cch16', 'cch4', 'out', 2),           # NP = 2
    (64, 64, 4, 7, 24, 2, 'scalar', 'cch4', 'out', 4),          # NP = 4
    (128, 128, 4, 7, 16, 2, 'scalar', 'cch4', 'out', 8),        # NP = 8
    (256, 256, 4, 7, 16, 2, 'scalar', 'cch4', 'rows', 0),       # output conv falling out of the GEMM form (too many tile pairs)
    (128, 128, 4, 3, 120, 1, 'cch16', 'cch4', 'wmfma', 0),      # ... and out of the row-staged form as well (row too long)
    # sums of more than 1600 products are split into segments (segment_of): the split instantiations of the MFMA kernel that the table above
    # does not reach - 3 x 3 at chunk 16 and 8, 5 x 5 at chunk 4 (chunk 4 at 3 x 3 and 7 x 7, chunk 8 at 5 x 5: rows 2, 4, 5)
    (192, 192, 192, 3, 17, 1, 'cch16', 'cch16', 'rows', 0), (200, 200, 200, 3, 17, 1, 'cch8', 'cch8', 'rows', 0),
    (84, 84, 84, 5, 17, 2, 'cch4', 'cch4', 'rows', 0),
    # image sizes: 8 = one partial tile (the library's minimum), 16, 17 = a tile with one valid row and column, 33, 40
    (64, 64, 64, 5, 8, 3, 'cch16', 'cch16', 'rows', 0), (64, 64, 64, 5, 16, 2, 'cch16', 'cch16', 'rows', 0),
    (64, 64, 64, 5, 17, 2, 'cch16', 'cch16', 'rows', 0), (64, 64, 64, 5, 33, 2, 'cch16', 'cch16', 'rows', 0),
    (32, 32, 32, 7, 8, 3, 'cch8', 'cch8', 'rows', 0), (32, 32, 32, 7, 16, 2, 'cch8', 'cch8', 'rows', 0),
    (32, 32, 32, 7, 17, 2, 'cch8', 'cch8', 'rows', 0), (32, 32, 32, 7, 33, 2, 'cch8', 'cch8', 'rows', 0),
    (32, 32, 32, 7, 40, 2, 'cch8', 'cch8', 'rows', 0),
    (64, 64, 4, 5, 8, 3, 'cch16', 'cch4', 'out', 2), (64, 64, 4, 5, 16, 2, 'cch16', 'cch4', 'out', 2),
    (64, 64, 4, 5, 17, 2, 'cch16', 'cch4', 'out', 2), (64, 64, 4, 5, 40, 2, 'cch16', 'cch4', 'out', 2),
]

# one case per weight-gradient form that is also called with gw / gb pre-filled (the header: the gradient is ADDED)
ACCUMULATE = [c for c in CASES if c[:5] in ((64, 64, 64, 5, 40), (128, 128, 128, 3, 72), (64, 64, 4, 5, 33), (64, 64, 4, 7, 24))]

# REF.STRIDE 3 / 4 run on the scalar kernels: (ci, ldc, co, k, S, N, s).  S = 16 at stride 3 and S = 18 at stride 4: the window of the last
# output column is cut by the image edge ((So - 1) s + k / 2 >= S); S = 17 / 18 / 23: (S - 1) % s != 0, the last pixel is no window centre
STRIDED = [(17, 20, 32, 3, 16, 3, 3), (17, 20, 32, 3, 17, 2, 3), (32, 32, 32, 5, 18, 2, 4), (32, 32, 32, 5, 23, 2, 4)]

# forward / data gradient walk several tiles per block (software pipeline): (ci, co, k, blocks per CU) at S = 40 = 9 tiles per image.
# Dynamic LDS of the kernel: 5 x 5 x 64 channels, 16-channel chunks 158 KB -> one block per CU; 3 x 3 x 16 channels 56 KB (<= 80 KB) -> two
TILE_LOOP = [(64, 64, 5, 1), (16, 16, 3, 2)]


def gate(products):
    """test_gpu_gen_s2.py's gates of the exact-fp32 generic kernels: 2e-6 of the largest element, 4e-6 where one output is a sum of more
    than 3000 fp32 products (7 x 7 with >= 64 channels) - the accumulation order's rounding, where the fp32 ATen conv sits as well"""
    return 4e-6 if products > 3000 else 2e-6


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def tier_of(mode, S, ci, ldc, co, k, s=1):
    """(tier, NP) the library picks - host arithmetic, no GPU"""
    v = _lib.lib().iodine_op_gen_conv_tier(mode, S, ci, ldc, co, k, s)
    assert v >= 0, (mode, S, ci, ldc, co, k, s)
    return v & 0xff, (v >> 8) & 0xff


def segment_of(mode, S, ci, ldc, co, k, s=1):
    """segment length of the forward / data gradient's sums (0: one fmaf chain; chains of more than 1600 products are split)"""
    return _lib.lib().iodine_op_gen_conv_tier(mode, S, ci, ldc, co, k, s) >> 16


def _guarded(shape, fill):
    """a buffer of the given shape (filled with `fill`: a number or a tensor) followed by the guard band"""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV)
    if isinstance(fill, torch.Tensor):
        buf[:n] = fill.to(DEV).reshape(-1)
    else:
        buf[:n] = fill
    return buf, buf[:n].view(shape)


def _guard_intact(buf):
    return bool((buf[-GUARD:] == SENTINEL).all())


def _op(mode, a, w, bias, aux, out, gb, n, si, ci, ldc, co, k, s, elu):
    t = [v.to(DEV).contiguous() if v is not None else None for v in (a, w, bias, aux)]
    rc = _lib.lib().iodine_op_gen_conv(None, mode, _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), _lib.ptr(out),
                                       _lib.ptr(gb) if gb is not None else None, n, si, ci, ldc, co, k, s, elu)
    if rc == 2:     # IODINE_ERR_HIP: a launch or kernel failed - the session ends, nothing more runs on a device that may have faulted
        pytest.exit(f'iodine_op_gen_conv mode {mode}, case {(n, si, ci, ldc, co, k, s)}: {_lib.lib().iodine_last_error(None).decode()}', 3)
    _lib.check(rc, None, 'iodine_op_gen_conv')
    torch.cuda.synchronize()


def _inputs(ci, co, k, S, N, s):
    So = (S - 1) // s + 1
    x = _rand(N, ci, S, S, seed=80)
    w = _rand(co, ci, k, k, seed=81, scale=3.0 / (ci * k * k) ** 0.5)
    b = _rand(co, seed=82, scale=0.5)
    d = _rand(N, co, So, So, seed=83, scale=1e-2)
    a = F.elu(_rand(N, ci, S, S, seed=84, scale=2.0))           # an ELU output: the data gradient's derivative operand
    return x, w, b, d, a


def _reference(x, w, b, d, a, k, s):
    """fp64 on the CPU, one autograd pass: ELU output, data gradient x ELU'(a), weight and bias gradient"""
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xr, wr, br, stride=s, padding=k // 2)
    (y * d.double()).sum().backward()
    da = torch.where(a > 0, torch.ones_like(a), a + 1).double()
    return nhwc(F.elu(y.detach())).float(), nhwc(xr.grad * da).float(), wr.grad.float(), br.grad.float()


def _pad_c(t_nchw, ldc):
    """NHWC with channel stride ldc, NaN past the real channels: what lies there must never reach a sum"""
    n, c, h, w_ = t_nchw.shape
    p = torch.full((n, h, w_, ldc), float('nan'))
    p[..., :c] = nhwc(t_nchw)
    return p


def _run_forward(x, w, b, ref, ci, ldc, co, k, S, N, s):
    xp = _pad_c(x, ldc)
    outs = []
    for _ in range(2):
        buf, out = _guarded(ref.shape, float('nan'))
        _op(0, xp, w, b, None, out, None, N, S, ci, ldc, co, k, s, 1)
        assert _guard_intact(buf), 'forward wrote behind its output'
        outs.append(out.cpu())
    return rel_err(outs[0], ref), torch.equal(outs[0], outs[1])


def _run_dgrad(w, d, a, ref, ci, ldc, co, k, S, N, s):
    # mode 1 takes the weights with ldc input channels (the packed input-channel count is din's stride) and computes ci of them: the
    # weights, the derivative operand and the output are NaN past channel ci - none of it may be read, the output's must stay
    wp = torch.full((co, ldc, k, k), float('nan'))
    wp[:, :ci] = w
    ap = _pad_c(a, ldc)
    outs = []
    for _ in range(2):
        buf, out = _guarded((N, S, S, ldc), float('nan'))
        _op(1, nhwc(d), wp, None, ap, out, None, N, S, ci, ldc, co, k, s, 0)
        assert _guard_intact(buf), 'data gradient wrote behind its output'
        outs.append(out.cpu())
    assert bool(torch.isnan(outs[0][..., ci:]).all()), 'data gradient wrote into the padding channels'
    return rel_err(outs[0][..., :ci], ref), torch.equal(outs[0][..., :ci], outs[1][..., :ci])


def _wgrad_call(xp, dn, gw0, gb0, ci, ldc, co, k, S, N, s):
    bw, gw = _guarded((co, ci, k, k), gw0)
    bb, gb = _guarded((co,), gb0)
    _op(2, xp, None, None, dn, gw, gb, N, S, ci, ldc, co, k, s, 0)
    assert _guard_intact(bw) and _guard_intact(bb), 'weight gradient wrote behind its outputs'
    return gw.cpu(), gb.cpu()


def _run_wgrad(x, d, ref_w, ref_b, ci, ldc, co, k, S, N, s, accumulate=False):
    xp, dn = _pad_c(x, ldc), nhwc(d)
    r0 = _wgrad_call(xp, dn, 0.0, 0.0, ci, ldc, co, k, S, N, s)
    r1 = _wgrad_call(xp, dn, 0.0, 0.0, ci, ldc, co, k, S, N, s)
    same = torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    e_acc = None
    if accumulate:                                              # gw / gb are ADDED to: pre-filled with values of the gradient's size
        pw = _rand(co, ci, k, k, seed=85, scale=float(ref_w.abs().max()))
        pb = _rand(co, seed=86, scale=float(ref_b.abs().max()))
        aw, ab = _wgrad_call(xp, dn, pw, pb, ci, ldc, co, k, S, N, s)
        e_acc = max(rel_err(aw.double() - pw.double(), r0[0]), rel_err(ab.double() - pb.double(), r0[1]))
    return rel_err(r0[0], ref_w), rel_err(r0[1], ref_b), same, e_acc


def _id(c):
    return '-'.join(str(v) for v in c[:6])


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_gen_stride1_conv(case):
    """all three directions of one layer against one fp64 reference.  Gates: gate() above, per direction by the products one output sums
    (forward ci k^2, data gradient co k^2; the weight gradient at test_gpu_gen_s2.py's 2e-6).

    Observed on MI355X (worst per direction): forward 1.89e-6 (MFMA, one chain of 1600 products), data gradient 1.96e-6 (likewise), weight
    gradient 3.48e-7, bias 2.23e-7, accumulation 7.6e-8.  Sums of more than 1600 products are split into segments (segment_of): before
    that, 256-256-4-7-16-2 forward (scalar kernel, one chain of 12544 products) was at 4.33e-6 and 256-256-256-3-40-1 data gradient (MFMA,
    2304 products) at 2.56e-6, past their gates; a CPU emulation of the chain gave exactly those figures, the fp32 ATen CPU conv is at
    5.41e-7 / 2.50e-7 on the same inputs, so the gates stayed and the kernels changed: now 5.41e-7 and 7.59e-7, the split cases 8.8e-7 or less."""
    ci, ldc, co, k, S, N, t_f, t_d, t_w, np_ = case
    assert tier_of(0, S, ci, ldc, co, k) == (TIER[t_f], 0)
    assert tier_of(1, S, ci, ldc, co, k) == (TIER[t_d], 0)
    assert tier_of(2, S, ci, ldc, co, k) == (TIER[t_w], np_)
    x, w, b, d, a = _inputs(ci, co, k, S, N, 1)
    r_f, r_d, r_w, r_b = _reference(x, w, b, d, a, k, 1)
    e_f, same_f = _run_forward(x, w, b, r_f, ci, ldc, co, k, S, N, 1)
    e_d, same_d = _run_dgrad(w, d, a, r_d, ci, ldc, co, k, S, N, 1)
    e_w, e_b, same_w, e_acc = _run_wgrad(x, d, r_w, r_b, ci, ldc, co, k, S, N, 1, accumulate=case in ACCUMULATE)
    print(f'[gen s1] ci{ci}/{ldc} co{co} k{k} S{S} N{N} ({t_f}/{t_d}/{t_w}{np_ or ""}, segments {segment_of(0, S, ci, ldc, co, k)}/'
          f'{segment_of(1, S, ci, ldc, co, k)}): forward {e_f:.2e}, dgrad {e_d:.2e}, '
          f'wgrad {e_w:.2e}, bias {e_b:.2e}' + (f', accumulated {e_acc:.2e}' if e_acc is not None else ''))
    assert e_f < gate(ci * k * k), e_f
    assert e_d < gate(co * k * k), e_d
    assert e_w < 2e-6 and e_b < 2e-6, (e_w, e_b)
    assert same_f and same_d and same_w, (same_f, same_d, same_w)
    assert e_acc is None or e_acc < 1e-6, e_acc


@pytest.mark.parametrize('case', STRIDED, ids=_id)
def test_gen_strides_3_and_4_on_the_scalar_kernels(case):
    ci, ldc, co, k, S, N, s = case
    for mode in range(3):
        assert tier_of(mode, S, ci, ldc, co, k, s) == (TIER['scalar'], 0)
    x, w, b, d, a = _inputs(ci, co, k, S, N, s)
    r_f, r_d, r_w, r_b = _reference(x, w, b, d, a, k, s)
    e_f, same_f = _run_forward(x, w, b, r_f, ci, ldc, co, k, S, N, s)
    e_d, same_d = _run_dgrad(w, d, a, r_d, ci, ldc, co, k, S, N, s)
    e_w, e_b, same_w, _ = _run_wgrad(x, d, r_w, r_b, ci, ldc, co, k, S, N, s)
    print(f'[gen s{s}] ci{ci}/{ldc} co{co} k{k} S{S} N{N}: forward {e_f:.2e}, dgrad {e_d:.2e}, wgrad {e_w:.2e}, bias {e_b:.2e}')
    assert e_f < 2e-6 and e_d < 2e-6 and e_w < 2e-6 and e_b < 2e-6, (e_f, e_d, e_w, e_b)
    assert same_f and same_d and same_w


def tile_loop_batch(ci, co, per_cu, n_cu):
    """the batch at which the blocks of the forward / data-gradient kernel take unequal tile counts of 2 and 3: nb = per_cu n_cu / ncg blocks
    per channel group (launcher), 9 N tiles, 9 N >= 2 nb + 1 and no multiple of nb; capped at 256 (6.5 M floats at 16 channels)"""
    nb = max(1, per_cu * n_cu // ((max(ci, co) + 15) // 16))
    n = (2 * nb + 1 + 8) // 9
    while (9 * n) % nb == 0:
        n += 1
    return min(n, 256), nb


@pytest.mark.parametrize('ci,co,k,per_cu', TILE_LOOP)
def test_gen_stride1_tile_loop(ci, co, k, per_cu):
    """more tiles than blocks, unevenly: every element is compared - a tile dropped at the end of a block's loop is in the last images"""
    S = 40
    N, nb = tile_loop_batch(ci, co, per_cu, torch.cuda.get_device_properties(0).multi_processor_count)
    assert tier_of(0, S, ci, ci, co, k) == (TIER['cch16'], 0) and tier_of(1, S, ci, ci, co, k) == (TIER['cch16'], 0)
    x, w, b, d, a = _inputs(ci, co, k, S, N, 1)
    r_f, r_d, _, _ = _reference(x, w, b, d, a, k, 1)
    e_f, same_f = _run_forward(x, w, b, r_f, ci, ci, co, k, S, N, 1)
    e_d, same_d = _run_dgrad(w, d, a, r_d, ci, ci, co, k, S, N, 1)
    print(f'[gen s1 tile loop] c{ci} k{k} N{N}: {9 * N} tiles on {nb} blocks per channel group: forward {e_f:.2e}, dgrad {e_d:.2e}')
    assert e_f < 2e-6 and e_d < 2e-6, (e_f, e_d)
    assert same_f and same_d
