"""iodine_amd._session.Session against a recording stub of the library: which setters a ``prepare`` sends, in which order, and what
invalidates what.  No device and no shared library: ``_lib.lib`` is replaced by an object that records every call and returns 0."""
import contextlib

import pytest
import torch

from iodine_amd import _lib, _session

DEV = torch.device('cuda', 0)
OBJ = (0.2, 0.5, (0.0, 0.25, 0.25, 0.5))
FIRST = dict(B=2, mode=1, K=4, T=3, frames=4, objective=OBJ, sigma_grad=True, input_grad=1, stable_encoding=True)
PLAN = ['iodine_workspace_bytes', 'iodine_set_workspace']      # a re-plan: the workspace depends on (B, mode, K, T, frames) and on input_grad


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def take(self):
        """what was called since the last take: names, with the key of a set_option"""
        out = [n + (':' + a[1].decode() if n == 'iodine_set_option' else '') for n, a in self.calls]
        self.calls.clear()
        return out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    real_empty = torch.empty
    monkeypatch.setattr(_lib, 'lib', lambda: r)
    monkeypatch.setattr(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch, 'empty', lambda *a, device=None, **kw: real_empty(*a, **kw))
    monkeypatch.setattr(_session.Session, 'stream', lambda self: None)
    return r


def _session_(options=None):
    cfg = _lib.Config(dim_latent=8, iters=2, slots=3, img_size=16, img_channels=3, sigma=0.1)
    return _session.Session(cfg, lambda: [], options)


def _prepare(s, **change):
    kw = dict(FIRST, **change)
    return s.prepare(DEV, kw.pop('B'), kw.pop('mode'), kw.pop('K'), kw.pop('T'), **kw)


def test_a_new_session_starts_with_every_mirror_field_at_its_creation_value():
    s = _session_({'input_grad': 2, 'sigma_grad': 1, 'batch_cap': 4})
    assert s.handle is None and s.device is None and s.param_versions is None and s.workspace is None and s.ws_key is None
    assert s.shape == (3, 2) and s.frames == 0 and s.objective == (0.1, 1.0, ()) and s.call_serial == 0
    assert s.modes == {'stable_encoding': False, 'sigma_grad': True} and s.ig == 2
    assert s.graph_stream is None and s.graph_bufs == {} and s.options == {'input_grad': 2.0, 'sigma_grad': 1.0, 'batch_cap': 4.0}
    t = _session.Session(s.cfg, s.named_parameters, s.options, call_serial=7)          # what a device change makes
    assert t.call_serial == 7 and t.options == s.options and t.options is not s.options and t.ig == 2 and t.ws_key is None


def test_identical_prepares_send_each_setter_once_and_in_order(rec):
    s = _session_()
    _prepare(s)
    assert rec.take() == ['iodine_create', 'iodine_num_params', 'iodine_set_params', 'iodine_set_option:input_grad', 'iodine_set_run_shape',
                          'iodine_set_frames', *PLAN, 'iodine_set_option:stable_encoding', 'iodine_set_option:sigma_grad',
                          'iodine_set_objective']
    assert (s.shape, s.frames, s.objective, s.ig, s.modes) == ((4, 3), 4, OBJ, 1, {'stable_encoding': True, 'sigma_grad': True})
    _prepare(s)
    assert rec.take() == []
    s.close()


@pytest.mark.parametrize('change,sent', [
    (dict(K=5), ['iodine_set_run_shape', *PLAN]), (dict(T=2), ['iodine_set_run_shape', *PLAN]), (dict(frames=0), ['iodine_set_frames', *PLAN]),
    (dict(objective=(0.2, 1.0, OBJ[2])), ['iodine_set_objective']), (dict(sigma_grad=False), ['iodine_set_option:sigma_grad']),
    (dict(input_grad=3), ['iodine_set_option:input_grad', *PLAN]), (dict(B=3), PLAN),
    (dict(frames=None, objective=None, input_grad=None), [])])           # None: the step is skipped, the handle keeps what it has
def test_one_change_resends_exactly_its_setter(rec, change, sent):
    s = _session_()
    _prepare(s)
    rec.take()
    _prepare(s, **change)
    assert rec.take() == sent
    _prepare(s, **change)
    assert rec.take() == []
    s.close()


def test_options_invalidate_what_depends_on_them(rec):
    s = _session_()
    s.set_option('batch_cap', 2)                        # before the handle exists ...
    _prepare(s)
    rec.take()
    s.set_option('conv_precision', 0)
    assert rec.take() == ['iodine_set_option:conv_precision']
    _prepare(s)
    assert rec.take() == ['iodine_set_params']
    s.set_option('wgrad_accum', 1)
    assert rec.take() == ['iodine_set_option:wgrad_accum']
    _prepare(s)
    assert rec.take() == PLAN
    s.set_option('batch_cap', 3)                        # ... and after: read by the wrapper, never sent
    _prepare(s)
    assert rec.take() == [] and s.options['batch_cap'] == 3.0
    s.close()
    names = [n for n, _ in rec.calls]
    assert names == ['iodine_destroy']


def test_options_set_before_the_handle_exists_are_replayed_without_the_wrapper_s_own(rec):
    s = _session_({'batch_cap': 2, 'graph': 0, 'input_grad': 1})
    s.open(DEV)
    assert rec.take() == ['iodine_create', 'iodine_set_option:graph', 'iodine_set_option:input_grad', 'iodine_num_params']
    s.close()
