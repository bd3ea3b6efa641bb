"""Plain torch references of the refinement head (RefinementNetwork.forward behind the conv stack, iodine.py:481-503, and the posterior
update, iodine.py:642-643) for the kernel-level tests: one step forward, and back-propagation through T steps by autograd.  Written from the
model's formulae - adaptive_avg_pool2d, Linear + ELU, another ELU, torch.nn.LSTMCell with gate order i, f, g, o, the update layers reading the
CELL state (the reference's `(c, h) = lstm(...)` names h1 "c" and c1 "h") - in whatever dtype the inputs have: float64 is the reference, the
same functions in float32 on the CPU give the rounding level a correct fp32 implementation reaches (the tests' gates are 4 x that).
No GPU work here: test_head_cpu.py imports this module and the case tables."""
import torch
import torch.nn.functional as F

PARAMS = ('mlp_w', 'mlp_b', 'wih', 'whh', 'bih', 'bhh', 'wm', 'bm', 'wv', 'bv')
FWD_OUT = ('h', 'c', 'pm', 'plv', 'd_mean', 'd_logvar', 'pooled', 's', 'gates', 'xin')
BPTT_OUT = ('ddm', 'ddv', 'dgates', 'ds', 'dpooled', 'dh_out', 'dc_out')


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


def make_params(C, H, L, seed=0):
    """reference-shaped parameters in fp32.  The LSTM weights are scaled so that the gate pre-activations have a standard deviation near 2:
    sigmoid and tanh are used on both sides of saturation."""
    IN = H + 4 * L
    return {
        'mlp_w': _rand(H, C, seed=seed + 1, scale=2.0 / C ** 0.5), 'mlp_b': _rand(H, seed=seed + 2, scale=0.5),
        'wih': _rand(4 * H, IN, seed=seed + 3, scale=4.5 / (IN + H) ** 0.5), 'whh': _rand(4 * H, H, seed=seed + 4, scale=4.5 / (IN + H) ** 0.5),
        'bih': _rand(4 * H, seed=seed + 5, scale=0.5), 'bhh': _rand(4 * H, seed=seed + 6, scale=0.5),
        'wm': _rand(L, H, seed=seed + 7, scale=1.0 / H ** 0.5), 'bm': _rand(L, seed=seed + 8, scale=0.1),
        'wv': _rand(L, H, seed=seed + 9, scale=1.0 / H ** 0.5), 'bv': _rand(L, seed=seed + 10, scale=0.1),
    }


def cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in d.items()}


def lstm_cell(P, xin, h_prev, c_prev):
    """torch.nn.LSTMCell, returning the gate pre-activations as well"""
    pre = xin @ P['wih'].T + P['bih'] + h_prev @ P['whh'].T + P['bhh']
    i, f, g, o = pre.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    h = o * torch.tanh(c)
    return h, c, pre, torch.cat((i, f, g, o), dim=1)


def head_step(P, pooled, latent, h_prev, c_prev):
    s = pooled @ P['mlp_w'].T + P['mlp_b']
    u = F.elu(F.elu(s))
    xin = torch.cat((u, latent), dim=1)
    h, c, pre, gates = lstm_cell(P, xin, h_prev, c_prev)
    d_mean = c @ P['wm'].T + P['bm']                      # read from the cell state
    d_logvar = c @ P['wv'].T + P['bv']
    return {'h': h, 'c': c, 'd_mean': d_mean, 'd_logvar': d_logvar, 's': s, 'pre': pre, 'gates': gates, 'xin': xin}


def head_forward(P, feat, latent, h_prev, c_prev, pm, plv):
    """feat [N][PL][C] (the ELU output of the last conv layer), latent [N][4L], h_prev / c_prev [N][H], pm / plv [N][L] -> every tensor
    iodine_op_refine_head returns (FWD_OUT)"""
    pooled = feat.mean(dim=1)                             # adaptive_avg_pool2d to 1 x 1
    r = head_step(P, pooled, latent, h_prev, c_prev)
    r.update(pooled=pooled, pm=pm + r['d_mean'], plv=plv + r['d_logvar'])
    return r


def head_inputs(C, H, L, PL, N, seed=100):
    return {'feat': F.elu(_rand(N, PL, C, seed=seed, scale=2.0).double()).float(), 'latent': _rand(N, 4 * L, seed=seed + 1),
            'h_prev': _rand(N, H, seed=seed + 2), 'c_prev': _rand(N, H, seed=seed + 3, scale=2.0),
            'pm': _rand(N, L, seed=seed + 4), 'plv': _rand(N, L, seed=seed + 5)}


def default_alpha(i, T, B, dtype=torch.float64):
    """the weight of delta_i in the loss, -(i + 2) / (T + 1) / B, evaluated in dtype"""
    return -(torch.tensor(i + 2, dtype=dtype) / (T + 1)) / B


def bptt_inputs(L, H, Cr, N, T, seed=200):
    """the saved inputs of T head steps and the upstream gradients; every tensor fp32"""
    return {'pooled': _rand(T, N, Cr, seed=seed), 'latent': _rand(T, N, 4 * L, seed=seed + 1), 'h0': _rand(N, H, seed=seed + 2),
            'c0': _rand(N, H, seed=seed + 3, scale=2.0), 'g_pm': _rand(T + 1, N, L, seed=seed + 4), 'g_plv': _rand(T + 1, N, L, seed=seed + 5),
            'seed1_m': _rand(N, L, seed=seed + 6, scale=0.3), 'seed1_v': _rand(N, L, seed=seed + 7, scale=0.3),
            'seedT_m': _rand(T, N, L, seed=seed + 8, scale=0.3), 'seedT_v': _rand(T, N, L, seed=seed + 9, scale=0.3),
            'wtab': _rand(T + 1, seed=seed + 10).abs() + 0.25, 'dh_in': _rand(N, H, seed=seed + 11, scale=0.5),
            'dc_in': _rand(N, H, seed=seed + 12, scale=0.5)}


# variants of the backward: which optional inputs are given.  seeds: 0 none (the unseeded instance), 1 one slice joining step T - 1,
# 'T' one slice per step (seed_stride = N L); gl: None = absent (the seeded instance then scales the ELBO seeds by 0)
VARIANTS = {
    'plain': dict(seeds=0, gl=None, wtab=False, dh_in=False, dc_in=False, carry_out=False),
    'plain_wtab': dict(seeds=0, gl=None, wtab=True, dh_in=False, dc_in=False, carry_out=False),
    'seed1': dict(seeds=1, gl=0.37, wtab=True, dh_in=True, dc_in=True, carry_out=True),
    'seedT': dict(seeds='T', gl=0.37, wtab=False, dh_in=False, dc_in=True, carry_out=True),
    'seedT_gl0': dict(seeds='T', gl=0.0, wtab=False, dh_in=True, dc_in=False, carry_out=False),
    'seed1_nogl': dict(seeds=1, gl=None, wtab=True, dh_in=False, dc_in=False, carry_out=True),
}


def cotangents(X, var, T, B):
    """a_i, b_i [T][N][L]: d objective / d (d_mean_i, d_logvar_i)"""
    a, b = [], []
    dtype = X['g_pm'].dtype
    for i in range(T):
        al = (-X['wtab'][i + 1] / B) if var['wtab'] else default_alpha(i, T, B, dtype)
        am, av = al * X['g_pm'][i + 1], al * X['g_plv'][i + 1]
        if var['seeds']:
            gl = torch.tensor(0.0 if var['gl'] is None else var['gl'], dtype=torch.float32).to(dtype)   # (the kernel reads an fp32 scalar)
            am, av = am * gl, av * gl
            if var['seeds'] == 'T':
                am, av = am + X['seedT_m'][i], av + X['seedT_v'][i]
            elif i == T - 1:
                am, av = am + X['seed1_m'], av + X['seed1_v']
        a.append(am)
        b.append(av)
    return torch.stack(a), torch.stack(b)


def head_unroll(P, X, T):
    """T head steps from pooled_i, latent_i and (h_0, c_0); the LSTM state is the only thing carried (lambda_{i+1} = detach(lambda_i) +
    delta_i and the refinement inputs are detached).  -> the per-step dicts of head_step, and the states h [T + 1], c [T + 1]"""
    h, c = [X['h0']], [X['c0']]
    steps = []
    for i in range(T):
        r = head_step(P, X['pooled'][i], X['latent'][i], h[-1], c[-1])
        steps.append(r)
        h.append(r['h'])
        c.append(r['c'])
    return steps, h, c


def head_bptt(P, X, T, B, var):
    """autograd through head_unroll of  sum_i <a_i, d_mean_i> + <b_i, d_logvar_i> + <dh_in, h_T> + <dc_in, c_T>.
    -> saved forward tensors (gates [T][N][4H], c [T + 1][N][H], s [T][N][H]) and the gradients BPTT_OUT"""
    X = dict(X)
    for k in ('pooled', 'h0', 'c0'):
        X[k] = X[k].clone().requires_grad_(True)
    steps, h, c = head_unroll(P, X, T)
    for r in steps:
        r['pre'].retain_grad()
        r['s'].retain_grad()
    a, b = cotangents(X, var, T, B)
    obj = sum((a[i] * steps[i]['d_mean']).sum() + (b[i] * steps[i]['d_logvar']).sum() for i in range(T))
    if var['dh_in']:
        obj = obj + (X['dh_in'] * h[T]).sum()
    if var['dc_in']:
        obj = obj + (X['dc_in'] * c[T]).sum()
    obj.backward()
    return {'gates': torch.stack([r['gates'] for r in steps]).detach(), 'c': torch.stack(c).detach(),
            's': torch.stack([r['s'] for r in steps]).detach(),
            'ddm': a, 'ddv': b, 'dgates': torch.stack([r['pre'].grad for r in steps]), 'ds': torch.stack([r['s'].grad for r in steps]),
            'dpooled': X['pooled'].grad, 'dh_out': X['h0'].grad, 'dc_out': X['c0'].grad, 'objective': obj.detach()}


def pool_bwd(pre, dpooled):
    """autograd of mean over the pixels of ELU(pre): pre [N][PL][C], dpooled [N][C] -> (act = ELU(pre), d / d pre)"""
    pre = pre.clone().requires_grad_(True)
    act = F.elu(pre)
    (act.mean(dim=1) * dpooled).sum().backward()
    return act.detach(), pre.grad


def rel_max(a, b):
    """largest error relative to the reference's largest element"""
    b = b.double()
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
# head forward: (C, H, L, PL, N) -> the forms that apply (0 single launch, 1 three launches)
FWD_CASES = {
    (32, 32, 8, 16, 3): (0, 1),
    (64, 256, 64, 64, 33): (0, 1),
    (32, 128, 16, 64, 1): (0, 1),
    (4, 4, 16, 1, 2): (0,),                # L > 2H, PL = 1
    (32, 32, 128, 4, 3): (0, 1),           # L > 2H
    (64, 64, 256, 9, 2): (0, 1),           # L > 2H
    (256, 260, 8, 5, 3): (0,),             # second column pass, NS < 16, G = 1
    (128, 320, 12, 7, 5): (0, 1),
    (64, 356, 64, 4, 2): (0,),             # largest single-launch
    (64, 512, 8, 4, 33): (1,),             # three-launch only
    (32, 1024, 256, 4, 2): (1,),           # three-launch only
    (8, 36, 16, 3, 4): (0,),               # single-launch only
}
# BPTT: (L, H, Cr, N) -> forms (0 fused kernel, 1 launch sequence)
BPTT_CASES = {
    (8, 32, 32, 3): (0, 1),
    (64, 256, 64, 33): (0, 1),
    (4, 4, 4, 1): (0, 1),
    (16, 36, 8, 2): (0, 1),
    (100, 260, 256, 3): (0, 1),
    (8, 512, 64, 5): (0, 1),
    (256, 1024, 32, 2): (0, 1),
    (16, 8, 32, 3): (1,),                  # Cr > H: the fused kernel refuses
}
BPTT_T = (1, 2, 5)
# which variants a (case, T) runs: the unseeded and the fully seeded instance everywhere, the others spread over T
BPTT_VARIANTS = {1: ('plain', 'seed1', 'seedT_gl0'), 2: ('plain_wtab', 'seed1', 'seedT'), 5: ('plain', 'seed1', 'seedT', 'seed1_nogl')}
BPTT_B = {1: 1, 2: 1, 3: 1, 5: 1, 33: 11}                    # N -> the batch size in the loss weight (N = B K)
POOL_CASES = [(3, 1, 32), (2, 5, 8), (33, 64, 64)]            # (N, PL, C)
HEAD_GATE_CAP = 1e-5
