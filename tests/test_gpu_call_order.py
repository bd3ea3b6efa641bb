"""What a call leaves behind, and what every entry point refuses, as return codes of the C ABI - on a compute handle and on the
reference-shaped boundary of a zero-padded one (DIM_LATENT 6 / REF.MLP_UNITS 30).

The handles are driven through ``_lib`` directly at the smallest shape the library runs (16 px, 2 slots, 2 iterations, batch 1,
32 channels).  After each event the codes of every reader and every backward are recorded; then the codes of each entry point's own
argument refusals (all host-side: none reaches a kernel).  EXPECTED was recorded with ``record()`` below against a build of the commit
before the host layer was split into iodine_api.cpp / iodine_pad.cpp / iodine_ops.cpp (selected with IODINE_HIP_LIB); both kinds of handle
gave the same table there, and the test passes against that build and this tree's.  Every cell is asserted.

Against this tree's own library (IODINE_HIP_LIB unset) the test also asserts that the padded handle reports every refusal in the words of
the compute handle: both run the same check functions.  The earlier build worded some of the padded path's refusals differently.
"""
import ctypes as C
import os

import pytest
import torch

from iodine_amd import _lib

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, 1, 3                      # IODINE_OK, IODINE_ERR_INVALID, IODINE_ERR_STATE (include/iodine_hip.h)
B, K, T, S = 1, 2, 2, 16
P, N = S * S, B * K
HANDLES = {'plain': (8, 32), 'padded': (6, 30)}   # DIM_LATENT, REF.MLP_UNITS

PROBES = ('last_elbo_outputs', 'last_posterior', 'last_refine_state', 'debug_copy_enc', 'train_backward_flat', 'decode_backward',
          'elbo_backward')

# event -> codes of PROBES after it
EXPECTED_EVENTS = {
    'fresh':                           (3, 3, 3, 3, 3, 3, 3),
    'set_params':                      (3, 3, 3, 3, 3, 3, 3),
    'reconstruct':                     (0, 0, 0, 0, 3, 3, 3),
    'elbo':                            (0, 0, 3, 0, 3, 3, 3),
    'elbo_saved':                      (0, 0, 3, 3, 3, 3, 0),
    'elbo_saved/consumed':             (0, 0, 3, 3, 3, 3, 3),
    'decode':                          (3, 3, 3, 3, 3, 3, 3),
    'decode_saved':                    (3, 3, 3, 3, 3, 0, 3),
    'decode_saved/consumed':           (3, 3, 3, 3, 3, 3, 3),
    'train_forward':                   (0, 0, 3, 0, 0, 3, 3),
    'train_forward/consumed':          (0, 0, 3, 0, 3, 3, 3),
    'reconstruct/set_params':          (0, 0, 0, 0, 3, 3, 3),
    'elbo_saved/set_params':           (0, 0, 3, 3, 3, 3, 3),
    'train_forward/set_params':        (0, 0, 3, 0, 3, 3, 3),
    'reconstruct/set_workspace':       (3, 3, 3, 3, 3, 3, 3),
    'elbo_saved/set_workspace':        (3, 3, 3, 3, 3, 3, 3),
    'train_forward/set_workspace':     (3, 3, 3, 3, 3, 3, 3),
    'reconstruct/run_shape':           (0, 0, 0, 0, 3, 3, 3),
    'elbo_saved/run_shape':            (0, 0, 3, 3, 3, 3, 3),
    'train_forward/run_shape':         (0, 0, 3, 0, 3, 3, 3),
    'reconstruct/frames':              (0, 0, 0, 0, 3, 3, 3),
    'elbo_saved/frames':               (0, 0, 3, 3, 3, 3, 3),
    'train_forward/frames':            (0, 0, 3, 0, 3, 3, 3),
    'reconstruct/wgrad_accum':         (3, 3, 3, 3, 3, 3, 3),
    'elbo_saved/wgrad_accum':          (3, 3, 3, 3, 3, 3, 3),
    'train_forward/wgrad_accum':       (3, 3, 3, 3, 3, 3, 3),
}

# refused call -> its code (parameters set, nothing saved unless the name says so)
EXPECTED_REFUSALS = {
    'reconstruct(x=NULL)': 1,
    'reconstruct(eps=NULL)': 1,
    'reconstruct(batch=0)': 1,
    'reconstruct_seq(state_in, one tensor missing)': 1,
    'reconstruct_seq(traj, stop_after_iters)': 1,
    'reconstruct(frames != T)': 1,
    'train_forward(frames != T + 1)': 1,
    'decode(z=NULL)': 1,
    'decode(batch=0)': 1,
    'elbo(x=NULL)': 1,
    'elbo(eps=NULL)': 1,
    'elbo(batch=0)': 1,
    'elbo(post_mean only)': 1,
    'train_forward(x=NULL)': 1,
    'train_forward(eps=NULL)': 1,
    'train_forward(loss=NULL)': 1,
    'train_forward(batch=0)': 1,
    'train_forward(weights != T + 1)': 1,
    'train_backward_flat(flat=NULL)': 1,
    'decode_saved; decode_backward(batch=2)': 1,
    'last_elbo_outputs(count=0)': 1,
    'last_posterior(count=2)': 1,
    'last_refine_state(count=0)': 1,
}


class Handle:
    """One library handle with caller tensors at the reference's shapes (generously sized: a reader may answer at an earlier run shape)."""

    def __init__(self, kind):
        self.L, self.H = HANDLES[kind]
        self.lib = _lib.lib()
        cfg = _lib.Config(dim_latent=self.L, iters=T, slots=K, img_size=S, img_channels=3, sigma=0.1, layernorm=1, stop_gradient=0,
                          encoding=_lib.ENC_FULL, ref_conv_chan=32, ref_conv_layers=2, ref_mlp_units=self.H, ref_kernel_size=3,
                          ref_stride=2, dec_conv_chan=32, dec_conv_layers=2, dec_kernel_size=3)
        self.h = C.c_void_p()
        assert self.lib.iodine_create(C.byref(cfg), C.byref(self.h)) == OK, self.lib.iodine_last_error(None)
        g = torch.Generator().manual_seed(5)
        self.params = []
        name, nd, dims = C.c_char_p(), C.c_int(), (C.c_longlong * 4)()
        for i in range(self.lib.iodine_num_params(self.h)):
            assert self.lib.iodine_param_info(self.h, i, C.byref(name), C.byref(nd), dims) == OK
            self.params.append((0.05 * torch.randn(*dims[:nd.value], generator=g)).cuda())
        self.n_flat = sum(p.numel() for p in self.params)
        self.x = torch.rand(3, B, 3, S, S, generator=g).cuda()                      # (room for a clip of 3 frames)
        self.eps = torch.randn(T + 1, N, self.L, generator=g).cuda()
        self.bufs = {}

    def buf(self, name, n=1 << 15):
        if name not in self.bufs:
            self.bufs[name] = torch.zeros(n, device='cuda')
        return _lib.ptr(self.bufs[name])

    def close(self):
        self.lib.iodine_destroy(self.h)

    def err(self):
        return self.lib.iodine_last_error(self.h).decode()

    # ---- events
    def set_params(self):
        ptrs = (C.c_void_p * len(self.params))(*[p.data_ptr() for p in self.params])
        return self.lib.iodine_set_params(self.h, None, ptrs, len(self.params))

    def option(self, key, value):
        return self.lib.iodine_set_option(self.h, key.encode(), float(value))

    def reconstruct(self, x='x', eps='eps', batch=B, state_in=None, traj=None):
        f = self.buf
        args = [self.h, None, batch, _lib.ptr(self.x) if x else None, _lib.ptr(self.eps) if eps else None, f('pred'), f('mask'), f('mean'),
                f('z'), f('pm'), f('plv'), f('elbo_iter')]
        if state_in is None and traj is None:
            return self.lib.iodine_reconstruct(*args)
        return self.lib.iodine_reconstruct_seq(*args, state_in, traj)

    def elbo(self, x='x', eps='eps', batch=B, post_mean=None, post_logvar=None):
        return self.lib.iodine_elbo(self.h, None, batch, _lib.ptr(self.x) if x else None, post_mean, post_logvar,
                                    _lib.ptr(self.eps) if eps else None, self.buf('terms'))

    def decode(self, z='z_in', batch=B):
        return self.lib.iodine_decode(self.h, None, batch, self.buf(z) if z else None, self.buf('pred'), self.buf('mask'), self.buf('mean'))

    def saved(self, call):
        assert self.option('save_for_backward', 1) == OK
        rc = call()
        assert self.option('save_for_backward', 0) == OK
        return rc

    def train_forward(self, x='x', eps='eps', loss='loss', batch=B):
        return self.lib.iodine_train_forward(self.h, None, batch, _lib.ptr(self.x) if x else None, _lib.ptr(self.eps) if eps else None,
                                             self.buf(loss) if loss else None, self.buf('elbo_iter'))

    # ---- readers and backwards
    def train_backward_flat(self, flat='flat'):
        return self.lib.iodine_train_backward_flat(self.h, None, self.buf('gl'), self.buf(flat, self.n_flat) if flat else None, 0)

    def decode_backward(self, batch=B):
        f = self.buf
        return self.lib.iodine_decode_backward(self.h, None, batch, f('g_pred'), f('g_mask'), f('g_mean'), f('dz'), f('flat', self.n_flat), 0)

    def elbo_backward(self):
        f = self.buf
        return self.lib.iodine_elbo_backward(self.h, None, f('gl'), f('g_pm'), f('g_plv'), f('flat', self.n_flat), 0)

    def last_elbo_outputs(self, count=B):
        f = self.buf
        return self.lib.iodine_last_elbo_outputs(self.h, None, count, f('z'), f('mean'), f('mask'), f('logits'), f('pred'))

    def last_posterior(self, count=B):
        return self.lib.iodine_last_posterior(self.h, None, count, self.buf('pm'), self.buf('plv'))

    def last_refine_state(self, count=B):
        return self.lib.iodine_last_refine_state(self.h, None, count, self.buf('lstm_h'), self.buf('lstm_c'))

    def debug_copy_enc(self):
        n = C.c_size_t()
        return self.lib.iodine_debug_copy(self.h, None, b'enc', 0, self.buf('enc', 1 << 16), 1 << 16, C.byref(n))

    def probe(self):
        """(code, message) of every reader, then of every backward: a reader changes nothing, and of the three backwards at most one finds
        something saved (consuming it changes no reader's answer)"""
        out = []
        for name in PROBES:
            rc = getattr(self, name)()
            out.append((rc, self.err() if rc else ''))
        torch.cuda.synchronize()
        return tuple(out)


def _events(hd):
    """yields (event name, probe result)"""
    yield 'fresh', hd.probe()
    assert hd.set_params() == OK, hd.err()
    yield 'set_params', hd.probe()
    preps = {
        'reconstruct': hd.reconstruct,
        'elbo': hd.elbo,
        'elbo_saved': lambda: hd.saved(hd.elbo),
        'decode': hd.decode,
        'decode_saved': lambda: hd.saved(hd.decode),
        'train_forward': hd.train_forward,
    }
    for name, prep in preps.items():
        assert prep() == OK, hd.err()
        yield name, hd.probe()
        if name in ('elbo_saved', 'decode_saved', 'train_forward'):        # the probe ran the matching backward: it is consumed now
            yield name + '/consumed', hd.probe()

    def run_shape():
        assert hd.lib.iodine_set_run_shape(hd.h, 3, T) == OK, hd.err()
        res = hd.probe()
        assert hd.lib.iodine_set_run_shape(hd.h, K, T) == OK
        return res

    def frames():
        assert hd.lib.iodine_set_frames(hd.h, 3) == OK, hd.err()
        res = hd.probe()
        assert hd.lib.iodine_set_frames(hd.h, 0) == OK
        return res

    def wgrad_accum():
        assert hd.option('wgrad_accum', 1) == OK, hd.err()
        res = hd.probe()
        assert hd.option('wgrad_accum', 0) == OK
        return res

    def set_params():
        assert hd.set_params() == OK, hd.err()
        return hd.probe()

    def set_workspace():
        assert hd.lib.iodine_set_workspace(hd.h, None, 0) == OK, hd.err()      # (back to the library's own arena: a new one)
        return hd.probe()

    for ev_name, ev in (('set_params', set_params), ('set_workspace', set_workspace), ('run_shape', run_shape), ('frames', frames),
                        ('wgrad_accum', wgrad_accum)):
        for name in ('reconstruct', 'elbo_saved', 'train_forward'):
            assert preps[name]() == OK, hd.err()
            yield name + '/' + ev_name, ev()


def _refusals(hd):
    """yields (name, (code, message)); the handle has its parameters and nothing saved"""
    vp = C.c_void_p

    def cell(rc):
        return rc, hd.err() if rc else ''

    yield 'reconstruct(x=NULL)', cell(hd.reconstruct(x=None))
    yield 'reconstruct(eps=NULL)', cell(hd.reconstruct(eps=None))
    yield 'reconstruct(batch=0)', cell(hd.reconstruct(batch=0))
    state = (vp * 4)(hd.buf('pm'), hd.buf('plv'), hd.buf('lstm_h'), None)
    yield 'reconstruct_seq(state_in, one tensor missing)', cell(hd.reconstruct(state_in=state))
    traj = (vp * 5)(*[hd.buf('traj%d' % j) for j in range(5)])
    assert hd.option('stop_after_iters', 1) == OK
    yield 'reconstruct_seq(traj, stop_after_iters)', cell(hd.reconstruct(traj=traj))
    assert hd.option('stop_after_iters', -1) == OK
    assert hd.lib.iodine_set_frames(hd.h, T + 1) == OK
    yield 'reconstruct(frames != T)', cell(hd.reconstruct())
    assert hd.lib.iodine_set_frames(hd.h, T) == OK
    yield 'train_forward(frames != T + 1)', cell(hd.train_forward())
    assert hd.lib.iodine_set_frames(hd.h, 0) == OK
    yield 'decode(z=NULL)', cell(hd.decode(z=None))
    yield 'decode(batch=0)', cell(hd.decode(batch=0))
    yield 'elbo(x=NULL)', cell(hd.elbo(x=None))
    yield 'elbo(eps=NULL)', cell(hd.elbo(eps=None))
    yield 'elbo(batch=0)', cell(hd.elbo(batch=0))
    yield 'elbo(post_mean only)', cell(hd.elbo(post_mean=hd.buf('pm')))
    yield 'train_forward(x=NULL)', cell(hd.train_forward(x=None))
    yield 'train_forward(eps=NULL)', cell(hd.train_forward(eps=None))
    yield 'train_forward(loss=NULL)', cell(hd.train_forward(loss=None))
    yield 'train_forward(batch=0)', cell(hd.train_forward(batch=0))
    w = (C.c_double * T)(*([1.0] * T))
    assert hd.lib.iodine_set_objective(hd.h, 0.1, 1.0, w, T) == OK, hd.err()
    yield 'train_forward(weights != T + 1)', cell(hd.train_forward())
    assert hd.lib.iodine_set_objective(hd.h, 0.1, 1.0, None, 0) == OK
    yield 'train_backward_flat(flat=NULL)', cell(hd.train_backward_flat(flat=None))
    assert hd.saved(hd.decode) == OK, hd.err()
    yield 'decode_saved; decode_backward(batch=2)', cell(hd.decode_backward(batch=2))
    assert hd.elbo() == OK, hd.err()
    yield 'last_elbo_outputs(count=0)', cell(hd.last_elbo_outputs(count=0))
    yield 'last_posterior(count=2)', cell(hd.last_posterior(count=B + 1))
    assert hd.reconstruct() == OK, hd.err()
    yield 'last_refine_state(count=0)', cell(hd.last_refine_state(count=0))
    torch.cuda.synchronize()


def record(kind):
    """({event: ((code, message), ...)}, {refusal: (code, message)}) of one kind of handle"""
    hd = Handle(kind)
    try:
        events = dict(_events(hd))
        return events, dict(_refusals(hd))
    finally:
        hd.close()


@pytest.fixture(scope='module')
def recorded():
    return {kind: record(kind) for kind in HANDLES}


@pytest.mark.parametrize('kind', list(HANDLES))
def test_codes_after_every_event_and_of_every_refusal(recorded, kind):
    events, refusals = recorded[kind]
    assert list(events) == list(EXPECTED_EVENTS) and list(refusals) == list(EXPECTED_REFUSALS)
    got = {ev: tuple(rc for rc, _ in cells) for ev, cells in events.items()}
    for ev in EXPECTED_EVENTS:
        print(kind, ev, got[ev])
    assert got == EXPECTED_EVENTS
    got_r = {name: rc for name, (rc, _) in refusals.items()}
    print(kind, got_r)
    assert got_r == EXPECTED_REFUSALS


@pytest.mark.skipif(bool(os.environ.get('IODINE_HIP_LIB')), reason='another build of the library is selected: only this tree promises it')
def test_padded_handle_refuses_in_the_words_of_the_compute_handle(recorded):
    (ev_a, ref_a), (ev_b, ref_b) = recorded['plain'], recorded['padded']
    n = 0
    for ev in EXPECTED_EVENTS:
        for probe, (rc_a, msg_a), (rc_b, msg_b) in zip(PROBES, ev_a[ev], ev_b[ev]):
            if rc_a or rc_b:
                assert msg_a and msg_a == msg_b, (ev, probe, msg_a, msg_b)
                n += 1
    for name in EXPECTED_REFUSALS:
        assert ref_a[name][1] and ref_a[name][1] == ref_b[name][1], (name, ref_a[name], ref_b[name])
        n += 1
    assert n > 100                                 # (every refused cell was compared)
