"""iodine_amd._chunked on CPU tensors against a straightforward reference: the balanced split, the None-tolerant cut and the merge rules,
bit for bit and in the left-to-right order the chunk loops of the wrapper have always summed in."""
import pytest
import torch

from iodine_amd._chunked import CAT0, CAT1, FIRST, SHARE, SUM, cut, merge, scaled, split


@pytest.mark.parametrize('B', [1, 2, 5, 7])
@pytest.mark.parametrize('cap', [1, 2, 3, 7, 8])
def test_split_covers_the_batch_in_balanced_runs(B, cap):
    runs = split(B, cap)
    assert len(runs) == -(-B // cap) and runs[0][0] == 0 and runs[-1][1] == B
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))                        # no gap, no overlap
    sizes = [e - s for s, e, _ in runs]
    assert max(sizes) <= cap and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    assert [w for _, _, w in runs] == [n / float(B) for n in sizes]


def test_cut_slices_the_named_axis_and_passes_none_through():
    t = torch.arange(24.).view(2, 4, 3)
    assert cut(None, 1, 3) is None and cut(None, 1, 3, axis=1) is None
    assert torch.equal(cut(t, 1, 2), t[1:2]) and torch.equal(cut(t, 1, 3, axis=1), t[:, 1:3]) and torch.equal(cut(t, 0, 2, 2), t[:, :, 0:2])
    assert cut(t, 1, 3, 1).data_ptr() == t[:, 1:3].data_ptr()                       # a view, like the slice it replaces


def _parts(sizes):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(n, 3, generator=g), torch.randn(2, n, generator=g), torch.randn(4, 3, generator=g) * 1e3, None, 'chunk %d' % i)
            for i, n in enumerate(sizes)]


def test_merge_rules_on_tuples_with_none_fields():
    sizes = [3, 2, 2]
    parts, shares = _parts(sizes), [n / 7.0 for n in sizes]
    a, b, c, d, e = merge(parts, (CAT0, CAT1, SHARE, CAT0, FIRST), shares)
    assert torch.equal(a, torch.cat([p[0] for p in parts], 0)) and torch.equal(b, torch.cat([p[1] for p in parts], 1))
    want = sum(p[2] * (n / 7.0) for p, n in zip(parts, sizes))                      # the size-weighted sum, left to right from 0
    assert torch.equal(c, want) and not torch.equal(c, parts[2][2] * shares[2] + parts[1][2] * shares[1] + parts[0][2] * shares[0])
    assert d is None and e == 'chunk 0'
    assert merge(parts, (FIRST,) * 5)[0] is parts[0][0]


def test_merge_rules_on_dicts():
    parts = [dict(x=p[0], y=p[3], z=p[2]) for p in _parts([1, 2])]
    m = merge(parts, dict(x=CAT0, y=CAT1, z=SHARE), [1 / 3.0, 2 / 3.0])
    assert list(m) == ['x', 'y', 'z'] and m['y'] is None
    assert torch.equal(m['x'], torch.cat([p['x'] for p in parts], 0))
    assert torch.equal(m['z'], 0 + parts[0]['z'] * (1 / 3.0) + parts[1]['z'] * (2 / 3.0))


@pytest.mark.parametrize('with_weights', [True, False])
def test_accumulated_sigma_and_input_gradients_equal_the_left_to_right_reference(with_weights):
    B, g = 7, torch.Generator().manual_seed(5)
    runs = split(B, 3)
    chunks, sig, igs = [], None, []
    for s, e, share in runs:
        w = torch.full((), share, dtype=torch.float32)
        sc, gx = torch.randn((), generator=g) * 1e4, torch.randn(e - s, 3, 4, 4, generator=g)
        gw = torch.randn(e - s, 4, 4, generator=g) if with_weights else None
        chunks.append(scaled(w, sc, gx, gw))
        # the reference: what the two chunk loops did by hand
        igs.append(tuple(None if t is None else t * w for t in (gx, gw)))
        sig = sc * w if sig is None else sig + sc * w
    got_sig, got_gx, got_gw = merge(chunks, (SUM, CAT0, CAT0))
    assert torch.equal(got_sig, sig) and torch.equal(got_gx, torch.cat([t[0] for t in igs], 0))
    assert (got_gw is None) if not with_weights else torch.equal(got_gw, torch.cat([t[1] for t in igs], 0))
    assert merge([scaled(torch.ones(()), None, None)], (SUM, CAT0)) == (None, None)  # a call that asked for neither
