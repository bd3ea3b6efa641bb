"""Plain torch reference of one ELBO evaluation as the per-pixel mixture kernels see it (kernels_pixel.hip, pixel_terms.h), for the
kernel-level tests through iodine_op_pixel_encode: from a raw decoder output to every tensor the entry point returns.  Written from the
model's formulae - IODINE.elbo (iodine.py:161-241: softmax :185, gaussian_log_likelihood :210,661-666, logsumexp of log(mask + 1e-12) + l
:213-216, .mean(0).sum() :220, the KL against N(0, 1) :653-659), get_input_encoding (iodine.py:277-340, channels in code order) and the
5-D layernorm (iodine.py:385-394: biased sd, division by sd + 1e-5), decode (iodine.py:59-71) - in whatever dtype is asked for: float64 is
the reference, the same function in float32 on the CPU gives the rounding level a correct fp32 implementation reaches (the tests' gates are
multiples of it).  The gradients are autograd's of B x ELBO (iodine.py:90,137), d LL / d sigma autograd's with sigma as a leaf; no closed
form is used.  The pixel weights of iodine_set_pixel_weights stand in front of the pixel sum of the likelihood, so the gradients carry them;
likelihood, leave-one-out likelihood and mask posterior describe the scene and stay raw.

Also the case tables and the input makers of tests/test_pixel_cpu.py and tests/test_gpu_pixel.py.  No GPU work here."""
import functools
import math

import torch

# ---- the encoding ---------------------------------------------------------------------------------------------------------------------------
# internal channel c of the 17 (bit c of the channel mask), in the code order of iodine.py:277-340
CHANNELS = ('image',) * 3 + ('means',) * 3 + ('mask', 'mask_logits', 'mask_posterior') + ('ln_g_mean',) * 3 + ('ln_g_mask', 'ln_like', 'ln_loo') + \
           ('coord',) * 2
GROUPS = tuple(dict.fromkeys(CHANNELS))
LN_GROUPS = ('ln_g_mean', 'ln_g_mask', 'ln_like', 'ln_loo')
STATS = ('stat_g_mean', 'stat_g_mask', 'stat_loo', 'stat_like')          # lnstat[..., 2 j : 2 j + 2] = {mean, 1 / (sd + 1e-5)}
CH_FULL = 0x1FFFF
CH_DEFAULT = 0x07FFF                                                     # the reference's default ARCH.ENCODING: everything but the coordinates
CH_HOLES = CH_FULL & ~(1 << 4 | 1 << 8 | 1 << 10 | 1 << 13 | 1 << 14)    # holes in the middle, the three channels that can be NaN / Inf among them
# the split form of pass 2: lane j of enc[..][12] / enc_sh[..][8] holds internal channel ...; -1: padding
SPLIT_SLOT = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, -1)
SPLIT_SHARED = (0, 1, 2, 13, 15, 16, -1, -1)

SCALARS = ('ll_img', 'kl_img', 'scal', 'sgrad')
PLANES = ('g', 'pred', 'mask', 'mean', 'logits')


def f32(v):
    """the float the entry point receives for a Python number"""
    return float(torch.tensor(v, dtype=torch.float32))


def layernorm(v, use_ln=True):
    """5-D layernorm of iodine.py:385-394 over everything behind (image, slot) -> (normalised, mean (B, K), 1 / (sd + 1e-5) (B, K))"""
    if not use_ln:
        one = torch.ones(v.shape[:2], dtype=v.dtype)
        return v, torch.zeros_like(one), one
    dims = tuple(range(2, v.dim()))
    m = v.mean(dim=dims, keepdim=True)
    s = torch.sqrt(((v - m) ** 2).mean(dim=dims, keepdim=True))
    r = 1 / (s + 1e-5)
    return (v - m) * r, m.reshape(v.shape[:2]), r.reshape(v.shape[:2])


def evaluate(inp, dtype=torch.float64):
    """inp: dict(x (B, 3, P), w (B, P) or None, dec (B, K, P, 4) = rgb logits and mask logit, pm / plv (B, K, L), lin (S), sigma, beta, use_ln)
    -> every tensor iodine_op_pixel_encode returns, in ``dtype``; enc (B, K, P, 17) carries channel 8 of the reference, 'mask_post_stable'
    (B, K, P) the one of option stable_encoding (softmax over the slots of sum_c l_kc)"""
    c = lambda t: None if t is None else t.detach().to(dtype)
    x, w, pm, plv, lin = c(inp['x']), c(inp['w']), c(inp['pm']), c(inp['plv']), c(inp['lin'])
    B, K, P = inp['dec'].shape[:3]
    S = lin.numel()
    assert S * S == P
    sigma = torch.tensor(inp['sigma'], dtype=dtype, requires_grad=True)
    dec = c(inp['dec']).requires_grad_(True)
    mean = torch.sigmoid(dec[..., :3]).permute(0, 1, 3, 2)                # (B, K, 3, P)
    logits = dec[..., 3][:, :, None]                                      # (B, K, 1, P)
    mask = torch.softmax(logits, dim=1)
    k_ll = -(x[:, None] - mean) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)
    ll_px = torch.logsumexp(torch.log(mask + 1e-12) + k_ll, dim=1)        # (B, 3, P)
    ll_img = (ll_px if w is None else w[:, None] * ll_px).sum(dim=(1, 2))
    kl_img = (0.5 * (torch.exp(plv) + pm ** 2 - 1 - plv)).sum(dim=(1, 2))
    ll, kl = ll_img.mean(0), kl_img.mean(0)
    elbo = ll - inp['beta'] * kl
    g, g_mean, g_mask = torch.autograd.grad(B * elbo, [dec, mean, mask], retain_graph=True)
    sgrad, = torch.autograd.grad(ll, sigma)
    with torch.no_grad():
        use_ln = bool(inp['use_ln'])
        ls = k_ll.sum(dim=2, keepdim=True)                                # (B, K, 1, P)
        k_like = torch.exp(ls)
        mask_post = k_like / k_like.sum(dim=1, keepdim=True)
        like = torch.exp(ll_px.sum(dim=1, keepdim=True))[:, None].expand(B, K, 1, P).contiguous()
        mixture = (mask * k_like).sum(dim=1, keepdim=True)
        loo = (mixture - mask * k_like) / (1 - mask + 1e-5)
        n_gmean, *st_gmean = layernorm(g_mean, use_ln)
        n_gmask, *st_gmask = layernorm(g_mask, use_ln)
        n_like, *st_like = layernorm(like, use_ln)
        n_loo, *st_loo = layernorm(loo, use_ln)
        if K == 1:
            # planes that are constant by construction: a single slot has mask = 1, so its mask posterior is 1 and its leave-one-out
            # likelihood 0, and without weights d / d mask = 3 / (1 + 1e-12) at every pixel.  Their normalised value is 0, stated here: what the
            # arithmetic above leaves is rounding noise x 1e5
            mask_post = torch.ones_like(mask_post)
            n_loo = torch.zeros_like(n_loo)
            if w is None and use_ln:
                n_gmask = torch.zeros_like(n_gmask)
        cx = lin.repeat(S)[None, None, None].expand(B, K, 1, P)          # lin[p % S]
        cy = lin.repeat_interleave(S)[None, None, None].expand(B, K, 1, P)   # lin[p / S]
        enc = torch.cat([x[:, None].expand(B, K, 3, P), mean, mask, logits, mask_post, n_gmean, n_gmask, n_like, n_loo, cx, cy], dim=2)
        lnstat = torch.stack([st_gmean[0], st_gmean[1], st_gmask[0], st_gmask[1], st_loo[0], st_loo[1], st_like[0], st_like[1]], dim=2)
        return dict(g=g.detach(), lnstat=lnstat, ll_img=ll_img.detach(), kl_img=kl_img, scal=torch.stack([elbo, kl, ll]).detach(),
                    sgrad=sgrad.reshape(1), enc=enc.permute(0, 1, 3, 2).contiguous(), mask_post_stable=torch.softmax(ls[:, :, 0], dim=1),
                    pred=(mask * mean).sum(dim=1).detach(), mask=mask[:, :, 0].detach(), mean=mean.detach(), logits=logits[:, :, 0].detach(),
                    g_mean=g_mean, g_mask=g_mask[:, :, 0], k_ll=k_ll.detach(), ll_px=ll_px.detach())


# ---- error measures -------------------------------------------------------------------------------------------------------------------------
def plane_err(a, b, dim):
    """largest error of a plane relative to the plane's largest reference element, worst plane; ``dim``: the dimension the planes run
    along (the pixels).  A plane the reference states as 0 must be 0: any other value counts as an infinite error."""
    a, b = a.double(), b.double()
    d = (a - b).abs().amax(dim=dim)
    m = b.abs().amax(dim=dim)
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float('inf')), torch.zeros_like(d)))
    return float(e.max()) if e.numel() else 0.0


def scalar_err(a, b):
    """every element relative to its own magnitude"""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def stat_err(a, b):
    """a, b (B, K, 2) = {mean, 1 / (sd + 1e-5)}: the mean on the scale it is used on, the standard deviation (it is subtracted from values
    that are then divided by sd + 1e-5), or its own magnitude where that is larger; the reciprocal relative to itself"""
    a, b = a.double(), b.double()
    scale = torch.maximum(b[..., 0].abs(), 1 / b[..., 1])
    return max(float(((a[..., 0] - b[..., 0]).abs() / scale).max()), scalar_err(a[..., 1], b[..., 1]))


PLANE_DIM = {'g': 2, 'pred': 2, 'mask': 2, 'mean': 3, 'logits': 2}


def errors(got, ref, case, stable=0):
    """{tensor name: error} over what ``case`` compares.  got: the entry point's tensors with enc as (B, K, P, 17); names: SCALARS, PLANES,
    the channel GROUPS of enc, STATS"""
    out = {}
    for k in SCALARS:
        if k in got:
            out[k] = scalar_err(got[k], ref[k])
    for k in PLANES:
        if k in got:
            out[k] = plane_err(got[k], ref[k], PLANE_DIM[k])
    skip = excluded(case, stable)
    if 'enc' in got:
        renc = ref['enc']
        if stable:
            renc = renc.clone()
            renc[..., 8] = ref['mask_post_stable']
        for name in GROUPS:
            if name not in skip:
                ch = [i for i, n in enumerate(CHANNELS) if n == name]
                out[name] = plane_err(got['enc'][..., ch], renc[..., ch], 2)
    if 'lnstat' in got:
        for j, name in enumerate(STATS):
            if name not in skip:
                out[name] = stat_err(got['lnstat'][..., 2 * j:2 * j + 2], ref['lnstat'][..., 2 * j:2 * j + 2])
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
# name -> family, B, K, S, L, sigma, beta, use_ln, weighted, mask-logit scale.  nblk = ceil(P / 512) blocks of ppb = ceil(P / nblk) pixels.
#   near: x in [0.05, 0.95], means within 0.25 of it, mask logits 0.5 randn, sigma 0.1 - every fp32 term stays in range: all 17 channels
#   far:  rgb logits 1.5 randn, mask logits 1.5 (one case 4) randn - p_k and the pixel likelihood underflow in fp32: see FAR_EXCLUDED
def _case(family, B, K, S, L=8, sigma=0.1, beta=1.0, use_ln=1, weighted=False, mask_scale=None):
    return dict(family=family, B=B, K=K, S=S, L=L, sigma=f32(sigma), beta=f32(beta), use_ln=use_ln, weighted=weighted,
                mask_scale=mask_scale if mask_scale is not None else (0.5 if family == 'near' else 1.5))


CASES = {
    'near_k2_s5': _case('near', 1, 2, 5),                                      # a partial wave
    'near_k7_s8_kl448': _case('near', 2, 7, 8, L=64),                          # exactly one wave; K L = 448: two trips of the KL loop for some
    'near_k1_s9_w_kl3': _case('near', 2, 1, 9, L=3, weighted=True),            # a wave plus 17 pixels; K L = 3; K = 1 with a real LN(g_mask)
    'near_k3_s16_noln': _case('near', 2, 3, 16, use_ln=0),                     # one full block; statistics exactly {0, 1}
    'near_k1_s17': _case('near', 1, 1, 17),                                    # a second loop trip for 33 threads; the constant planes of K = 1
    'near_k3_s23_w_beta': _case('near', 2, 3, 23, beta=0.5, weighted=True),    # two blocks, ppb 265: an unaligned block start, a 9-pixel wave
    # 99 statistics; K L = 1024.  beta 0.5: at beta 1 the ELBO of this case is ll - kl = 744 - 580, a fifth of its terms
    'near_k16_s23_w_kl1024': _case('near', 2, 16, 23, L=64, beta=0.5, weighted=True),
    'near_k7_s33_kl56': _case('near', 3, 7, 33),                               # three blocks, ppb 363; K L = 56
    'near_k2_s64': _case('near', 1, 2, 64),                                    # nblk 8: the unrolled finalize loop, no remainder
    'near_k11_s65': _case('near', 2, 11, 65, L=4),                             # nblk 9: the unrolled loop and its remainder
    'near_k16_s65_beta': _case('near', 1, 16, 65, beta=0.5),                   # K = 16 on several blocks
    'near_k3_s68_w': _case('near', 2, 3, 68, weighted=True),                   # nblk 10
    'raw_k3_s1': _case('near', 2, 3, 1),                                       # one pixel: raw outputs and sentinels
    'raw_k16_s2': _case('near', 3, 16, 2),                                     # four pixels
    # the finalize's loops over more than 256 images.  sigma 1: every log-likelihood term is negative, so no image's sum of 12 terms cancels
    # (at sigma 0.1 the terms have both signs and one of 300 four-pixel images sums to 1e-4 of its terms: ll_img is then not comparable)
    'raw_k1_s2_b300_kl3': _case('near', 300, 1, 2, L=3, sigma=1.0, beta=0.5),
    'far_k2_s9': _case('far', 2, 2, 9),
    'far_k16_s17_kl1024': _case('far', 1, 16, 17, L=64),
    'far_k3_s23_sat_s03': _case('far', 3, 3, 23, sigma=0.3, mask_scale=4.0),   # saturated masks
    'far_k7_s33_w_s03_beta': _case('far', 2, 7, 33, sigma=0.3, beta=0.5, weighted=True),
    'far_k11_s65_noln': _case('far', 1, 11, 65, use_ln=0),
}
# what a far case does not compare against float64: p_k = exp(sum_c l_kc) and exp(ll_sum) underflow in fp32 there, so the reference's
# un-stabilised mask posterior (channel 8 without stable_encoding) is 0 / 0, and the likelihood and leave-one-out channels (13, 14) and their
# statistics are quotients of denormals.  By name, per family - never decided from the data
FAR_EXCLUDED = ('mask_posterior', 'ln_like', 'ln_loo', 'stat_like', 'stat_loo')
FAR_EXCLUDED_STABLE = ('ln_like', 'ln_loo', 'stat_like', 'stat_loo')
# below S = 5 a plane has at most four values: layer-norm channels and statistics are not compared (LN of four values is conditioned like 1 / sd)
RAW_EXCLUDED = LN_GROUPS + STATS


def excluded(case, stable=0):
    c = CASES[case]
    skip = ()
    if c['family'] == 'far':
        skip += FAR_EXCLUDED_STABLE if stable else FAR_EXCLUDED
    if c['S'] < 5:
        skip += RAW_EXCLUDED
    return skip


def weights(B, P, g):
    """as test_gpu_input_grad._kernel_inputs: 0.25 + 1.25 U with one all-zero region"""
    w = 0.25 + 1.25 * torch.rand(B, P, generator=g)
    w[:, P // 3:P // 3 + max(1, P // 4)] = 0.0
    return w


def make_inputs(family, B, K, S, L, sigma, beta, use_ln, weighted, mask_scale, far_scale=1.0):
    """fp32 inputs, seeded per (K, S).  far_scale multiplies the far family's rgb logits (means pushed to 0 / 1: every p_k underflows)"""
    g = torch.Generator().manual_seed(100000 + 1000 * K + S)
    P = S * S
    x = 0.05 + 0.9 * torch.rand(B, 3, P, generator=g)
    if family == 'near':
        mu = (x[:, None] + 0.25 * (2 * torch.rand(B, K, 3, P, generator=g) - 1)).clamp(0.02, 0.98)
        rgb = torch.logit(mu.double()).float().permute(0, 1, 3, 2)
    else:
        rgb = 1.5 * far_scale * torch.randn(B, K, P, 3, generator=g)
    dec = torch.cat([rgb, mask_scale * torch.randn(B, K, P, 1, generator=g)], dim=3).contiguous()
    pm = torch.randn(B, K, L, generator=g)
    plv = 0.5 * torch.randn(B, K, L, generator=g)
    w = weights(B, P, g) if weighted else None
    return dict(x=x, w=w, dec=dec, pm=pm, plv=plv, lin=torch.linspace(-1, 1, S), sigma=sigma, beta=beta, use_ln=use_ln)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    return make_inputs(**CASES[case])


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(float64 reference, {stable: errors of the float32 evaluation on the CPU against it}): computed once, never modified"""
    inp = case_inputs(case)
    ref = evaluate(inp, torch.float64)
    lo = evaluate(inp, torch.float32)
    errs = {}
    for stable in (0, 1):
        got = dict(lo)
        if stable:
            got['enc'] = lo['enc'].clone()
            got['enc'][..., 8] = lo['mask_post_stable']
        errs[stable] = errors(got, ref, case, stable)
    return ref, errs


GATE_CAP = 1e-5
MARGIN = {1: 4.0, 0: 16.0}                                               # strict -> multiple of the CPU fp32 error


@functools.lru_cache(maxsize=None)
def cpu_floor():
    """{tensor: worst error of the float32 CPU evaluation over the cases (both forms of channel 8)}"""
    worst = {}
    for case in CASES:
        for e in case_reference(case)[1].values():
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


def gates(strict):
    return {k: min(MARGIN[strict] * v, GATE_CAP) for k, v in cpu_floor().items()}
