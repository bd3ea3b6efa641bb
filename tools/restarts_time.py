"""Time of ``IODINE.restarts(x, chains=8)`` and of its parts, HIP events after warm-up.

    python tools/restarts_time.py [--reps 7] [--warmup 2] [--chains 8] [--out FILE.json] [--md FILE.md]

Two configurations: the dSprites architecture at B = 32, K = 6 and the CLEVR architecture at B = 8, K = 7; synthetic weights, uniform
images, fixed noise (the time depends on none of them).  Timed, each as one window between two events, the routes alternating sample by
sample in one process, the figure the median of ``reps`` samples:

* *restarts*: the whole call, consensus included;
* *reconstruct*: the one ``reconstruct`` over the C B batch inside it (the same repeated batch and noise);
* *post*: everything after it on the tensors it returned - ``chain_score``, the closed-form KL, the selection gathers, ``overlap_table``,
  ``slot_iou`` + ``matching.assign``, ``chain_consensus``, stability - as ``restarts`` runs it;
* *post by hand*: the same results from torch ops on the same tensors: the likelihood as ``logsumexp`` over broadcast planes, ``argmax``
  maps, one-hot contingency tables, one-hot votes, ``scatter_add_`` for the mean masks (the assignment itself stays ``matching.assign``:
  torch has no device solver).  Its outputs are compared with the library's before anything is timed.

The two new kernels alone: ``--kernel-reps`` back-to-back launches of one entry between two events, divided by their number - launch gaps
included, so a lower bound on the kernel's rate.  Bytes the algorithm must move, from the shapes: ``chain_score`` reads mask and mean once
(C B K 4 P floats) and x once per image (3 P floats; no weights here) and writes ll and the maps (C B P bytes); ``chain_consensus`` reads
the maps (C B P bytes for the votes and again for match, plus the reference chain's per chain), perm, and mask once (C B K P floats), and
writes votes (B K P int32), consensus (B P bytes), agreement (B P floats), mask_mean (B K P floats) and match."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iodine_amd import IODINE, chains                                   # noqa: E402
from iodine_amd.matching import assign                                  # noqa: E402
from iodine_amd.model import clevr6_arch, dsprites_arch                 # noqa: E402
from iodine_amd.objects import overlap_table, slot_iou                  # noqa: E402

CONFIGS = (('dsprites', dsprites_arch, 6, 32), ('clevr', clevr6_arch, 7, 8))
HBM_COPY_BPS = 6.29e12           # measured float4 copy rate of the MI355X (the achievable roof); the 8.0e12 of the data sheet is the other
HBM_SPEC_BPS = 8.0e12


def timed(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def measure(name, make_arch, K, B, C, reps, warmup, kernel_reps, dev):
    import math
    arch = make_arch()
    torch.manual_seed(0)
    model = IODINE(arch).to(dev)
    model.K = K
    L, S, T = int(arch.DIM_LATENT), int(arch.IMG_SIZE), int(model.n_iters)
    P = S * S
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    eps = torch.randn(C, T + 1, B, K, L, generator=g).to(dev)
    xr = x.repeat(C, 1, 1, 1)
    er = eps.permute(1, 0, 2, 3, 4).reshape(T + 1, C * B, K, L).contiguous()
    sigma, beta = float(model.sigma), float(model.beta)

    def whole():
        return model.restarts(x, chains=C, eps=eps)

    def recon():
        return model.reconstruct(xr, er)

    pred, mask, mean = recon()
    z = model.z
    pm, plv = model.posterior.mean, model.posterior.logvar
    m6, u6 = mask.view(C, B, K, 1, S, S), mean.view(C, B, K, 3, S, S)
    ar = torch.arange(B, device=dev)

    def post():
        ll, seg = chains.chain_score(x, m6, u6, sigma)
        kl = (0.5 * (plv.double().exp() + pm.double() ** 2 - 1.0 - plv.double()).sum((-2, -1))).view(C, B)
        score = ll.double() - beta * kl
        best = ((score == score.max(0).values).cumsum(0) == 0).sum(0)
        rows = best * B + ar
        sel = [t.index_select(0, rows) for t in (pred, mask, mean, z, pm, plv)]
        tab = overlap_table(seg, seg.view(C * B, S, S).index_select(0, rows).unsqueeze(0).expand(C, B, S, S).contiguous(), K, K)
        perm = assign((1.0 - slot_iou(tab)).float())[0]
        perm.view(C * B, K)[rows] = torch.arange(K, dtype=torch.int32, device=dev)
        cons = chains.chain_consensus(seg, perm, best.to(torch.int32), m6)
        m64 = cons.match.double()
        stab = (m64.sum(0) - m64.gather(0, best.view(1, B))[0]) / max(C - 1, 1)
        return dict(ll=ll, seg=seg, best=best, sel=sel, perm=perm, votes=cons.votes, consensus=cons.consensus, agreement=cons.agreement,
                    match=cons.match, mask_mean=cons.mask_mean, stability=stab)

    def post_by_hand():
        l = -(x[None, :, None] - u6) ** 2 / (2.0 * sigma * sigma) - math.log(sigma) - 0.5 * math.log(2.0 * math.pi)
        ll = torch.logsumexp(torch.log(m6 + 1e-12) + l, dim=2).sum((2, 3, 4))
        seg = m6[:, :, :, 0].argmax(2)
        kl = (0.5 * (plv.double().exp() + pm.double() ** 2 - 1.0 - plv.double()).sum((-2, -1))).view(C, B)
        score = ll.double() - beta * kl
        best = score.argmax(0)
        rows = best * B + ar
        sel = [t.index_select(0, rows) for t in (pred, mask, mean, z, pm, plv)]
        flat = seg.view(C, B, P)
        oa = torch.nn.functional.one_hot(flat, K).float()
        ob = torch.nn.functional.one_hot(flat[best, ar], K).float()
        tab = torch.einsum('cbpi,bpj->cbij', oa, ob)
        perm = assign((1.0 - slot_iou(tab)).float())[0]
        perm.view(C * B, K)[rows] = torch.arange(K, dtype=torch.int32, device=dev)
        t = perm.long().gather(2, flat)
        votes = torch.nn.functional.one_hot(t, K).sum(0).permute(0, 2, 1)
        top = votes.max(1)
        match = (t == t[best, ar][None]).float().mean(-1)
        mm = torch.zeros(B, K, P, device=dev)
        for c in range(C):
            mm.scatter_add_(1, perm[c].long()[:, :, None].expand(B, K, P), m6[c, :, :, 0].reshape(B, K, P))
        m64 = match.double()
        stab = (m64.sum(0) - m64.gather(0, best.view(1, B))[0]) / max(C - 1, 1)
        return dict(ll=ll, seg=seg.to(torch.uint8), best=best, sel=sel, perm=perm, votes=votes.to(torch.int32).reshape(B, K, S, S),
                    consensus=top.indices.to(torch.uint8).view(B, S, S), agreement=(top.values.float() / C).view(B, S, S), match=match,
                    mask_mean=(mm / C).view(B, K, 1, S, S), stability=stab)

    a, b = post(), post_by_hand()
    check = dict(ll_max_rel_diff=float(((a['ll'] - b['ll']).abs() / b['ll'].abs()).max()), seg_differ_pixels=int((a['seg'] != b['seg']).sum()),
                 best_equal=bool(torch.equal(a['best'], b['best'])), perm_equal=bool(torch.equal(a['perm'], b['perm'])),
                 votes_differ=int((a['votes'] != b['votes']).sum()), consensus_differ_pixels=int((a['consensus'] != b['consensus']).sum()),
                 match_max_diff=float((a['match'] - b['match']).abs().max()), mask_mean_max_diff=float((a['mask_mean'] - b['mask_mean']).abs().max()))
    seg, perm, best32 = a['seg'], a['perm'], a['best'].to(torch.int32)
    del a, b
    runs = {'restarts': whole, 'reconstruct': recon, 'post': post, 'post_by_hand': post_by_hand}
    times = {k: [] for k in runs}
    for r in range(warmup + reps):
        for k, fn in runs.items():
            t = timed(fn)
            if r >= warmup:
                times[k].append(t)
    score_ms = timed(lambda: chains.chain_score(x, m6, u6, sigma), kernel_reps)
    cons_ms = timed(lambda: chains.chain_consensus(seg, perm, best32, m6), kernel_reps)
    score_bytes = C * B * K * 4 * P * 4 + B * 3 * P * 4 + C * B * P + C * B * 4
    cons_bytes = 3 * C * B * P + C * B * K * 4 + C * B * K * P * 4 + B * K * P * 4 + B * P + B * P * 4 + B * K * P * 4 + C * B * 4
    med = lambda v: sorted(v)[len(v) // 2]
    out = {k + '_ms_median': round(med(v), 4) for k, v in times.items()}
    out.update({k + '_ms_min': round(min(v), 4) for k, v in times.items()})
    out.update({k + '_ms_max': round(max(v), 4) for k, v in times.items()})
    out.update(config=name, K=K, B=B, C=C, L=L, S=S, T=T, max_batch=model.max_batch(K=K),
               by_hand_over_post=round(med(times['post_by_hand']) / med(times['post']), 2),
               post_share_of_restarts=round(med(times['post']) / med(times['restarts']), 4),
               chain_score_ms=round(score_ms, 5), chain_score_bytes=score_bytes, chain_score_bytes_per_s=round(score_bytes / (score_ms * 1e-3), 1),
               chain_score_share_of_copy_rate=round(score_bytes / (score_ms * 1e-3) / HBM_COPY_BPS, 4),
               chain_consensus_ms=round(cons_ms, 5), chain_consensus_bytes=cons_bytes,
               chain_consensus_bytes_per_s=round(cons_bytes / (cons_ms * 1e-3), 1),
               chain_consensus_share_of_copy_rate=round(cons_bytes / (cons_ms * 1e-3) / HBM_COPY_BPS, 4), kernel_reps=kernel_reps, **check)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chains', type=int, default=8)
    ap.add_argument('--kernel-reps', type=int, default=50)
    ap.add_argument('--out')
    ap.add_argument('--md')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('restarts_time.py needs a ROCm device: a timing taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    rows = [measure(n, a, K, B, args.chains, args.reps, args.warmup, args.kernel_reps, dev) for n, a, K, B in CONFIGS]
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, hbm_copy_bps=HBM_COPY_BPS, hbm_spec_bps=HBM_SPEC_BPS,
               rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if args.md:
        with open(args.md, 'w') as f:
            f.write('| config | B | K | C | restarts ms | reconstruct (C B) ms | post ms | post by hand ms | by hand / post | post / restarts |\n'
                    '|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {} | {} | {} | {:.2f} ({:.2f} .. {:.2f}) | {:.2f} ({:.2f} .. {:.2f}) | {:.3f} ({:.3f} .. {:.3f}) | {:.3f} ({:.3f} .. {:.3f}) | {:.2f} | {:.4f} |\n'.format(
                    r['config'], r['B'], r['K'], r['C'], r['restarts_ms_median'], r['restarts_ms_min'], r['restarts_ms_max'],
                    r['reconstruct_ms_median'], r['reconstruct_ms_min'], r['reconstruct_ms_max'], r['post_ms_median'], r['post_ms_min'],
                    r['post_ms_max'], r['post_by_hand_ms_median'], r['post_by_hand_ms_min'], r['post_by_hand_ms_max'], r['by_hand_over_post'],
                    r['post_share_of_restarts']))
            f.write('\n| config | kernel | ms per launch | MB it must move | bytes / s | share of 6.29 TB/s |\n|---|---|---|---|---|---|\n')
            for r in rows:
                for k in ('chain_score', 'chain_consensus'):
                    f.write('| {} | {} | {:.5f} | {:.2f} | {:.4g} | {:.4f} |\n'.format(r['config'], k, r[k + '_ms'], r[k + '_bytes'] / 1e6,
                                                                                 r[k + '_bytes_per_s'], r[k + '_share_of_copy_rate']))


if __name__ == '__main__':
    main()
