"""Digest of everything the Python wrapper computes, for comparing two revisions of iodine_amd/ on the same box and the same build of
the library: every public entry point at the tiny architecture, chunked (B = 3, batch_cap = 2) and un-chunked (B = 2), eager and in graph
mode, with fixed eps and manual_seed.  Prints one line per tensor - a SHA-256 of every returned tensor, of the state left on the module and
of every .grad - and per call the launch counts of profile level 2 (eager) or the graph captures / replays (graph mode).

usage: python tools/model_split_equivalence.py [--root DIR]     (DIR: the checkout whose iodine_amd is imported; default: this one)
Two outputs of the same library must be identical: diff them (profiles/model_split_equivalence.md)."""
import argparse
import hashlib
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from iodine_amd import IODINE                                   # noqa: E402
from iodine_amd.model import arch_namespace, logger             # noqa: E402

DEV, K, T, L, S = 'cuda:0', 2, 1, 8, 16
CATS = ('conv_tile_fwd', 'conv_tile_dgrad', 'conv_tile_wgrad', 'dec_out', 'dec_out_dgrad', 'dec_out_wgrad', 'dec_out_bwd', 'dec_l0', 'gen_conv',
        'gen_conv_f16x3', 'gen_l0', 'l0_reduce', 'l0_slot_sum', 'pixel_pass1', 'pixel_pass2', 'pixel_input_grad', 'pixel_sigma_grad', 'refine_l0',
        'refine_l0f', 'refine_conv', 'refine_head', 'refine_wgrad', 'refine_dgrad', 'refine_bwd01', 'refine_bias_grad', 'head_bwd', 'render_bwd',
        'frames_in', 'traj_out', 'predictive', 'scene_edit')
STATE = ('z', 'mean', 'mask', 'mask_logits', 'elbo_terms', 'log_likelihood', 'K_log_likelihood', 'trajectory', 'objects', 'frames', 'lstm_hidden')


def digest(t):
    t = t.detach().contiguous().cpu()
    return f'{hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:24]} {str(t.dtype)[6:]}{list(t.shape)}'


def walk(name, v, out):
    if torch.is_tensor(v):
        out.append(f'{name}: {digest(v)}')
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            walk(f'{name}.{k}', v[k], out)
    elif isinstance(v, (tuple, list)):
        for i, u in enumerate(v):
            walk(f'{name}[{i}]', u, out)
    elif hasattr(v, '__dataclass_fields__'):
        walk(name, vars(v), out)
    elif v is not None:
        out.append(f'{name}: {v!r}')


def model(B, graph):
    torch.manual_seed(0)
    m = IODINE(arch_namespace(L, T, K, S, (32, 2, 32), (32, 2)))
    with torch.no_grad():
        for p in m.parameters():                                # (the default initial posterior is all zeros: make every parameter count)
            p.add_(0.05 * torch.randn_like(p))
    m = m.to(DEV)
    if B == 3:
        m.set_option('batch_cap', 2)
    m.set_option('graph', graph)
    m.likelihood_maps = True
    return m.manual_seed(7)


def inputs(B):
    g = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.rand(*shape, generator=g).to(DEV)
    n = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    return dict(x=r(B, 3, S, S), clip=r(B, T + 1, 3, S, S), eps=n(T + 1, B, K, L), eps1=n(B, K, L), w=r(B, 1, S, S), z=n(B, K, L),
                eps_s=n(3, B, K, L))


def calls(m, c, B):
    """(name, thunk -> what the call returned, tensors whose .grad to report)"""
    def train(x=None, **kw):
        def run():
            m.zero_grad(set_to_none=True)
            loss = m(c['x'] if x is None else x, c['eps'], **kw)
            aux = 0.0
            if kw.get('attach_state'):
                aux = m.z.sum() + m.mask.square().sum() + m.lstm_hidden[0].sum()
            if kw.get('attach_frames') is not None:
                aux = m.frames['mask'].square().sum() + m.frames['z'].sum()
            (loss + aux).backward()
            return loss
        return run

    def elbo(diff):
        def run():
            m.zero_grad(set_to_none=True)
            out = m.elbo(c['x'], c['eps1'], differentiable=diff)
            if diff:
                out.backward()
            return out
        return run

    def decode(diff):
        def run():
            m.zero_grad(set_to_none=True)
            z = c['z'].clone().requires_grad_(diff)
            out = m.decode(z, differentiable=diff)
            if diff:
                (out[0].sum() + out[1].square().sum() + out[2].sum()).backward()
            return (*out, z.grad)
        return run

    def state_and_trajectory():
        m.reconstruct(c['x'], c['eps'], keep_state=True)
        st = m.refinement_state()
        return m.reconstruct(c['x'], c['eps'], state=st, trajectory=True, objects=True), m.refinement_state()

    def sigma_grad():
        m.sigma = torch.tensor(0.1, device=DEV, requires_grad=True)
        try:
            return train()(), m.sigma.grad
        finally:
            m.sigma = 0.1

    wg = c['w'].clone().requires_grad_(True)
    xg = c['x'].clone().requires_grad_(True)
    yield 'reconstruct', lambda: m.reconstruct(c['x'], c['eps'])
    yield 'reconstruct(seed)', lambda: m.reconstruct(c['x'])
    yield 'reconstruct(state, trajectory)', state_and_trajectory
    yield 'reconstruct(clip, weights)', lambda: m.reconstruct(c['clip'][:, :T], c['eps'], weights=c['w'])
    yield 'encode', lambda: m.encode(c['x'], c['eps'])
    yield 'elbo', elbo(False)
    yield 'elbo(differentiable)', elbo(True)
    yield 'decode', decode(False)
    yield 'decode(differentiable)', decode(True)
    yield 'forward', train()
    yield 'forward(seed)', lambda: (m.zero_grad(set_to_none=True), m(c['x']).backward())
    yield 'forward(keep_state)', lambda: (train(keep_state=True)(), m.refinement_state())
    if B == 2:                                                  # (refused for a chunked batch)
        yield 'forward(attach_state)', train(attach_state=True)
        yield 'forward(attach_frames)', train(attach_frames=True, x=c['clip'])
    yield 'forward(weights)', train(weights=c['w'])
    yield 'forward(x, weights that require grad)', lambda: (train(x=xg, weights=wg)(), xg.grad, wg.grad)
    yield 'forward(sigma that requires grad)', sigma_grad
    yield 'predictive', lambda: (m.reconstruct(c['x'], c['eps']), m.predictive(c['x'], samples=3, eps=c['eps_s'], weights=c['w']))[1]
    yield 'predictive(seed)', lambda: m.predictive(samples=2)
    yield 'edit', lambda: m.edit(c['z'][:2], [0, 1], [1, 0], c['z'][:2, 0], [False, True], return_mask=True, return_mean=True, return_base=True)


def main():
    for graph in (0, 1):
        for B in (3, 2):
            m, c = model(B, graph), inputs(B)
            m.reconstruct(c['x'], c['eps'])                      # (the handle exists from here on: options reach it)
            for rep in range(2 if graph else 1):                # graph mode: the second round replays what the first captured
                for name, run in calls(m, c, B):
                    tag = f'[graph {graph} B {B}' + (f' round {rep}] ' if graph else '] ') + name
                    if not graph:
                        m.set_option('profile', 2)
                        for cat in CATS:
                            m.profile_read(cat)
                    for cat in ('graph_captures', 'graph_replays'):
                        m.profile_read(cat)
                    got = run()
                    torch.cuda.synchronize()
                    out = []
                    walk('returned', got, out)
                    for a in STATE:
                        walk('model.' + a, getattr(m, a), out)
                    walk('model.posterior', (m.posterior.mean, m.posterior.logvar), out)
                    walk('logger', {k: v for k, v in logger.things.items()}, out)
                    walk('grad', {n: p.grad for n, p in m.named_parameters()}, out)
                    if graph:
                        counts = {cat: m.profile_read(cat)[1] for cat in ('graph_captures', 'graph_replays')}
                    else:
                        counts = {cat: n for cat in CATS for n in [m.profile_read(cat)[1]] if n}
                        m.set_option('profile', 0)
                    print(tag)
                    print('  launches: ' + ' '.join(f'{k}={v}' for k, v in counts.items()))
                    for line in out:
                        print('  ' + line)


if __name__ == '__main__':
    main()
