"""Host side of global-norm gradient clipping (lib/engine/train.py:64, commented out in the reference): argument checks, the
state-dict layout and the C-ABI header text.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ('iodine_grad_norm_scratch_bytes', 'iodine_grad_norm', 'iodine_grad_scale', 'iodine_adam_step_clipped')


def _model():
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))


def test_state_dict_layout_is_unchanged_by_clipping():
    from iodine_amd.optim import make_optimizer
    m = _model()
    plain = make_optimizer(m, base_lr=3e-4, weight_decay=0.01).state_dict()
    opt = make_optimizer(m, base_lr=3e-4, weight_decay=0.01, max_grad_norm=5.0, nonfinite='skip')
    clipped = opt.state_dict()
    assert opt.max_grad_norm == 5.0 and opt.nonfinite == 'skip'
    assert clipped == plain                                               # same groups, same keys, same values, empty state
    assert len(clipped['param_groups']) == 4                              # one group per parameter (lib/solver/build.py:10-14)
    for gc, gp in zip(clipped['param_groups'], plain['param_groups']):
        assert list(gc.keys()) == list(gp.keys())
        assert 'max_grad_norm' not in gc and 'nonfinite' not in gc
    assert 'max_grad_norm' not in opt.defaults and 'nonfinite' not in opt.defaults
    ref = torch.optim.Adam([{'params': [p], 'lr': 3e-4, 'weight_decay': 0.01} for p in m.parameters()], lr=3e-4).state_dict()
    assert [set(g) >= {'lr', 'betas', 'eps', 'weight_decay', 'params'} for g in ref['param_groups']] == [True] * 4
    opt.load_state_dict(plain)                                            # and it loads back
    assert opt.max_grad_norm == 5.0 and opt.nonfinite == 'skip'           # attributes of the optimizer, not of its state


def test_defaults_leave_clipping_off():
    from iodine_amd.optim import FusedAdam, make_optimizer
    m = _model()
    assert FusedAdam(m.parameters(), lr=1e-3).max_grad_norm is None
    opt = make_optimizer(m)
    assert opt.max_grad_norm is None and opt.nonfinite == 'propagate'
    assert opt.last_grad_norm is None and opt.skipped_steps is None       # no step with clipping yet
    assert FusedAdam(m.parameters(), max_grad_norm=float('inf')).max_grad_norm == float('inf')


@pytest.mark.parametrize('bad', [0, 0.0, -1, float('nan')])
def test_bad_max_norm_is_rejected(bad):
    from iodine_amd.optim import FusedAdam, clip_grad_norm_, make_optimizer
    m = _model()
    with pytest.raises(ValueError):
        FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=bad)
    with pytest.raises(ValueError):
        make_optimizer(m, max_grad_norm=bad)
    with pytest.raises(ValueError):
        clip_grad_norm_(m.parameters(), bad)


def test_other_norm_types_and_nonfinite_modes_are_rejected():
    from iodine_amd.optim import FusedAdam, clip_grad_norm_, make_optimizer
    m = _model()
    for nt in (1, 1.0, float('inf'), 0.5):
        with pytest.raises(ValueError):
            clip_grad_norm_(m.parameters(), 5.0, norm_type=nt)
    with pytest.raises(ValueError):
        FusedAdam(m.parameters(), max_grad_norm=5.0, nonfinite='bogus')
    with pytest.raises(ValueError):
        make_optimizer(m, max_grad_norm=5.0, nonfinite='bogus')


def test_cpu_and_non_float32_gradients_raise():
    """no CPU / eager fallback, as for FusedAdam.step"""
    from iodine_amd.optim import clip_grad_norm_
    m = _model()
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='ROCm device'):
        clip_grad_norm_(m.parameters(), 5.0)
    d = _model().double()
    for p in d.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='float32'):
        clip_grad_norm_(d.parameters(), 5.0)


def test_header_cites_the_reference_line_for_every_new_entry():
    header = open(os.path.join(ROOT, 'include', 'iodine_hip.h')).read()
    for name in NEW_ENTRIES:
        m = re.search(r'/\*(?:(?!\*/).)*\*/\s*(?:int|size_t)\s+' + name + r'\s*\(', header, flags=re.S)
        assert m, name
        comment = m.group(0)
        assert 'train.py:64' in comment, name
    block = header[header.index('Global-norm gradient clipping'):header.index('iodine_ari_table')]
    assert 'clip_grad_norm_' in block and 'synchronise' in block and 'owns' in block


def test_new_entries_are_exported_and_reject_bad_arguments():
    import ctypes as C
    from iodine_amd import _lib
    L = _lib.lib()
    assert set(NEW_ENTRIES) <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW_ENTRIES)
    assert L.iodine_abi_version() == 3
    # scratch: a function of total alone, one fp64 partial per block, bounded
    n = L.iodine_grad_norm_scratch_bytes(1109956)
    assert n == L.iodine_grad_norm_scratch_bytes(1109956) and n % 8 == 0 and 8 <= n <= 8 * 1024
    assert L.iodine_grad_norm_scratch_bytes(7) == 8 and L.iodine_grad_norm_scratch_bytes(10 ** 9) == 8 * 1024
    fake = C.c_void_p(4096)                       # never dereferenced: every call below is refused before any launch
    for bad in (0.0, -1.0, float('nan')):
        assert L.iodine_grad_norm(None, fake, fake, 1, 16, bad, fake, 8, fake) == 1
    assert b'max_norm' in L.iodine_last_error(None)
    assert L.iodine_grad_norm(None, fake, fake, 1, 1 << 20, 5.0, fake, 8, fake) == 1          # scratch too small
    assert L.iodine_grad_norm(None, None, fake, 1, 16, 5.0, fake, 8, fake) == 1
    assert L.iodine_grad_scale(None, fake, fake, 1, 16, None) == 1
    assert L.iodine_adam_step_clipped(None, fake, fake, 1, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0) == 1
