"""``_lib.call``, the one place a handle-free entry point is invoked, against a recording stub of the library - what it passes, in which
order, under which device, and what it raises - and the per-thread slot of ``iodine_last_error(NULL)`` on the real library, which loads
without a device.  No GPU."""
import contextlib
import ctypes as C
import threading

import pytest
import torch

from iodine_amd import _lib, _session

STREAM = C.c_void_p(0x5ea)
DEV = torch.device('cuda', 1)


class Stub:
    """records (name, args) of every call; ``status`` is what the entry points return, ``missing`` the symbols this build lacks"""

    def __init__(self, status=0, missing=()):
        self.calls, self.status, self.missing = [], status, missing

    def __getattr__(self, name):
        if name in self.missing:
            raise AttributeError(name)
        if name == 'iodine_last_error':
            return lambda handle: b'iodine_x: the message of the library'

        def fn(*args):
            self.calls.append((name, args))
            return self.status
        return fn


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    s.devices = []

    @contextlib.contextmanager
    def device(d):
        s.devices.append(('enter', d))
        yield
        s.devices.append(('exit', d))
    monkeypatch.setattr(_lib, 'lib', lambda: s)
    monkeypatch.setattr(torch.cuda, 'device', device)
    monkeypatch.setattr(_lib, 'stream', lambda: STREAM)
    return s


def test_call_puts_the_stream_first_and_turns_tensors_and_none_into_pointers(stub):
    t = torch.arange(6, dtype=torch.float32)
    n, ref = C.c_int(3), C.c_void_p(t.data_ptr() + 4)
    by = C.byref(n)
    assert _lib.call('iodine_x', DEV, t, None, 7, 0.5, by, ref) is None
    (name, args), = stub.calls
    assert name == 'iodine_x' and len(args) == 7
    assert args[0] is STREAM
    assert isinstance(args[1], C.c_void_p) and args[1].value == t.data_ptr()
    assert args[2] is None                                                # NULL
    assert args[3] == 7 and type(args[3]) is int and args[4] == 0.5 and type(args[4]) is float
    assert args[5] is by and args[6] is ref                               # byref and a raw pointer go as given
    assert stub.devices == [('enter', DEV), ('exit', DEV)]


def test_call_runs_the_entry_point_inside_the_device_guard(stub):
    order = stub.devices
    real = stub.__getattr__('iodine_y')
    stub.__dict__['iodine_y'] = lambda *a: (order.append('call'), real(*a))[1]
    _lib.call('iodine_y', DEV, 1)
    assert order == [('enter', DEV), 'call', ('exit', DEV)]


def test_call_refuses_a_non_contiguous_tensor(stub):
    t = torch.zeros(4, 4).t()[1:]
    assert not t.is_contiguous()
    with pytest.raises(AssertionError, match='tensor must be contiguous'):
        _lib.call('iodine_x', DEV, t)
    assert stub.calls == []


def test_a_build_without_the_symbol_is_named(stub):
    stub.missing = ('iodine_gone',)
    with pytest.raises(RuntimeError, match='IODINE: this build of libiodine_hip.so has no iodine_gone'):
        _lib.call('iodine_gone', DEV, 1)
    with pytest.raises(RuntimeError, match='IODINE: this build of libiodine_hip.so has no iodine_gone'):
        _session.Session._fn('iodine_gone')                               # the handle-bound path: the same lookup
    assert stub.calls == [] and stub.devices == []


def test_a_non_zero_status_raises_with_the_symbol_and_the_library_s_message(stub):
    stub.status = 2
    with pytest.raises(RuntimeError) as e:
        _lib.call('iodine_x', DEV, 1)
    assert str(e.value) == 'iodine_x failed (status 2): iodine_x: the message of the library'
    assert stub.devices == [('enter', DEV), ('exit', DEV)]


def test_session_stream_is_the_shared_one(monkeypatch):
    monkeypatch.setattr(_lib, 'stream', lambda: STREAM)
    cfg = _lib.Config(dim_latent=8, iters=2, slots=3, img_size=16, img_channels=3, sigma=0.1)
    assert _session.Session(cfg, lambda: []).stream() is STREAM


# ---- the per-thread error slot, on the real library ------------------------------------------------------------------------------------
def _fail_assign_host(L):
    p = C.c_void_p(4096)                                                  # never dereferenced: n_rows = 0 is refused first
    return L.iodine_assign_host(p, None, 0, 2, p, p)


def _fail_sheet_size(L):
    return L.iodine_sheet_size(C.byref(_lib.SheetSpec()), None, None)


def test_last_error_after_one_failure_on_one_thread():
    L = _lib.lib()
    assert _fail_assign_host(L) == 1
    assert L.iodine_last_error(None).startswith(b'iodine_assign_host: bad argument')
    assert _fail_sheet_size(L) == 1
    assert L.iodine_last_error(None) == b'iodine_sheet_size: height or width is NULL'
    with pytest.raises(RuntimeError, match=r'iodine_sheet_size failed \(status 1\): iodine_sheet_size: height or width is NULL'):
        _lib.check(_fail_sheet_size(L), None, 'iodine_sheet_size')


def test_each_thread_reads_its_own_last_error():
    """A fails, then B fails, then A reads: A must see its own message, not B's (one slot per thread)."""
    L = _lib.lib()
    barrier = threading.Barrier(2, timeout=30)
    seen, errors = {}, []

    def run(name, body):
        try:
            body()
        except BaseException as e:          # (a broken barrier included: the other thread then fails too, the test reports both)
            errors.append((name, repr(e)))

    def a():
        assert _fail_assign_host(L) == 1
        barrier.wait()                      # 1: A has failed
        barrier.wait()                      # 2: B has failed and read its message
        seen['a'] = L.iodine_last_error(None)

    def b():
        barrier.wait()                      # 1
        assert _fail_sheet_size(L) == 1
        seen['b'] = L.iodine_last_error(None)
        barrier.wait()                      # 2

    threads = [threading.Thread(target=run, args=(n, f)) for n, f in (('a', a), ('b', b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    assert seen['b'] == b'iodine_sheet_size: height or width is NULL'
    assert seen['a'].startswith(b'iodine_assign_host: bad argument'), seen['a']
