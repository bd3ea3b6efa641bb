"""``Session``: the library handle of one ``IODINE`` module on one device, and everything that has to stay in step with it.

The handle is stateful - parameters, run shape, frame count, workspace, objective and options are set once and hold until changed -,
so the wrapper mirrors what it last sent and sends a setter only when a call needs something else.  Every mirror field is initialised
in ``__init__`` and nowhere else: a device change makes a new session, there is no partial reset."""
import contextlib
import ctypes as C

import torch

from . import _lib

_WRAPPER_OPTIONS = ('batch_cap',)      # max images per library call (IODINE.max_batch): read by the wrapper, never sent to the library


class Session:
    def __init__(self, cfg, named_parameters, options=None, call_serial=0):
        self.cfg, self.named_parameters = cfg, named_parameters
        self.options = dict(options or {})
        self.handle, self.device = None, None       # made by ``open``
        self.param_versions = None                  # (data_ptr, version) of every parameter as last packed (iodine_set_params)
        self.workspace, self.ws_key = None, None    # the workspace tensor and the (B, mode, K, T, frames, device) it was planned for
        self.shape = (int(cfg.slots), int(cfg.iters))       # (slots, iters) the handle runs at (iodine_set_run_shape)
        self.frames = 0                             # frames per call the handle expects (iodine_set_frames; 0 = one image)
        self.objective = (float(cfg.sigma), 1.0, ())        # (sigma, beta, weights) the handle holds (iodine_set_objective)
        self.modes = {k: bool(self.options.get(k)) for k in ('stable_encoding', 'sigma_grad')}     # these options as the handle holds them
                                                                                                   # (a third mode of the same kind: self.joint below)
        self.ig = int(self.options.get('input_grad', 0))    # option input_grad as the handle holds it
        self.joint = bool(self.options.get('joint_likelihood'))     # option joint_likelihood as the handle holds it (IODINE.likelihood)
        self.graph_stream, self.graph_bufs = None, {}
        self.call_serial = call_serial              # bumped by every compute call; a backward must match the forward that saved state

    def close(self):
        if self.handle is not None:
            _lib.lib().iodine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def open(self, device):
        """The handle on ``device`` (made on first use, with the options set so far)."""
        if self.handle is not None:
            return self.handle
        L, h = _lib.lib(), C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(L.iodine_create(C.byref(self.cfg), C.byref(h)), None, 'iodine_create')
        self.handle, self.device = h, device
        for k, v in self.options.items():
            if k not in _WRAPPER_OPTIONS:
                _lib.check(L.iodine_set_option(h, k.encode(), v), h)
        names = []
        for i in range(L.iodine_num_params(h)):
            nm, nd, dims = C.c_char_p(), C.c_int(), (C.c_longlong * 4)()
            _lib.check(L.iodine_param_info(h, i, C.byref(nm), C.byref(nd), dims), h)
            names.append((nm.value.decode(), tuple(dims[:nd.value])))
        mine = [(n, tuple(p.shape)) for n, p in self.named_parameters()]
        if names != mine:
            raise RuntimeError(f'parameter table mismatch between module and library:\n{names}\n{mine}')
        return h

    def stream(self):
        return _lib.stream()

    _fn = staticmethod(_lib.fn)

    def _set(self, symbol, *args):
        _lib.check(self._fn(symbol)(self.handle, *args), self.handle, symbol)

    def set_option(self, key, value):
        self.options[key] = float(value)
        if key in _WRAPPER_OPTIONS:
            return
        if self.handle is not None:
            self._set('iodine_set_option', key.encode(), float(value))
        if key in self.modes:
            self.modes[key] = bool(value)
        if key in ('conv_precision', 'conv_variant', 'gen_conv_precision'):
            self.param_versions = None      # the library keeps only the selected path's weight packs: re-send the parameters
        if key == 'input_grad':
            self.ig = int(value)
        if key == 'joint_likelihood':
            self.joint = bool(value)
        if key in ('wgrad_accum', 'input_grad'):
            self.ws_key = None              # the workspace plan depends on it: ask the library again

    # ---- preparation: what the handle must hold before a compute call -----------------------------------------------------------
    def sync_params(self):
        """Re-pack the module's parameters when any was written since the last pack (autograd's version counter) -> the handle."""
        params = [p for _, p in self.named_parameters()]
        for p in params:
            if p.device != self.device or p.dtype != torch.float32:
                raise RuntimeError('all parameters must be float32 on the same ROCm device as the input')
        versions = tuple((p.data_ptr(), p._version) for p in params)
        if versions != self.param_versions:
            keep = [p.detach().contiguous() for p in params]
            self._set('iodine_set_params', self.stream(), _lib.ptrs(keep), len(keep))
            self.param_versions = versions
        return self.handle

    def prepare(self, device, B, mode, K, T, frames=None, objective=None, sigma_grad=False, input_grad=None, stable_encoding=False,
                joint_likelihood=False):
        """Everything the compute call that follows needs on the handle, each step sent only when it differs from what the handle holds,
        in this order: the parameters; option input_grad (bit 1: image, bit 2: pixel weights - its accumulators are part of the workspace
        plan, so it comes before the workspace; ``set_option('input_grad', bits)`` keeps bits on for every call); the run shape (K, T);
        the frame count (0 = one image per batch entry, E = a clip of E frames); a workspace planned for (B, mode, K, T, frames); the
        modes stable_encoding / sigma_grad (``set_option('sigma_grad', 1)`` keeps it on), the form of the likelihood (option
        joint_likelihood) and the objective (sigma, beta, weights).
        A None ``input_grad`` / ``frames`` / ``objective`` skips its step: the handle keeps what it has.  -> the handle."""
        h = self.open(device)
        self.sync_params()
        if input_grad is not None:
            want = int(input_grad) | int(self.options.get('input_grad', 0))
            if want != self.ig:
                self._set('iodine_set_option', b'input_grad', float(want))
                self.ig, self.ws_key = want, None
        if self.shape != (K, T):
            self._set('iodine_set_run_shape', K, T)
            self.shape = (K, T)
        if frames is not None and frames != self.frames:
            self._set('iodine_set_frames', frames)
            self.frames = frames
        key = (B, mode, K, T, self.frames, device)
        if self.ws_key != key:
            need = _lib.lib().iodine_workspace_bytes(h, B, mode)
            if self.workspace is None or self.workspace.numel() < need or self.workspace.device != device:
                self.workspace = None
                self.workspace = torch.empty(need, dtype=torch.uint8, device=device)
            self._set('iodine_set_workspace', C.c_void_p(self.workspace.data_ptr()), self.workspace.numel())
            self.ws_key = key
        if objective is not None:
            for k, want in (('stable_encoding', bool(stable_encoding)), ('sigma_grad', bool(sigma_grad or self.options.get('sigma_grad')))):
                if self.modes[k] != want:
                    self._set('iodine_set_option', k.encode(), float(want))
                    self.modes[k] = want
            if self.joint != bool(joint_likelihood):        # (the handle discards a saved pass of the other form: its backward is refused)
                self._set('iodine_set_option', b'joint_likelihood', float(bool(joint_likelihood)))
                self.joint = bool(joint_likelihood)
            if objective != self.objective:
                sigma, beta, w = objective
                with torch.cuda.device(device):             # (a new weight table is a small device allocation of the handle)
                    self._set('iodine_set_objective', sigma, beta, _lib.ints(w, C.c_double) if w else None, len(w))
                self.objective = objective
        return h

    # ---- calls --------------------------------------------------------------------------------------------------------------------
    def call(self, symbol, *args):
        """``symbol(handle, stream, *args)`` on the current stream with the session's device current; tensors and None go as pointers,
        everything else as given.  With option ``graph`` the call goes to a private non-default stream (the legacy null stream cannot be
        captured), ordered after / before the caller's.  Raises on a non-zero status.  (Handle-free entry points: ``_lib.call``.)"""
        fn = self._fn(symbol)
        args = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
        run = lambda: _lib.check(fn(self.handle, self.stream(), *args), self.handle, symbol)
        with torch.cuda.device(self.device):
            if not self.graph_on():
                return run()
            if self.graph_stream is None:
                self.graph_stream = torch.cuda.Stream(device=self.device)
            cur = torch.cuda.current_stream()
            self.graph_stream.wait_stream(cur)
            with torch.cuda.stream(self.graph_stream):
                run()
            cur.wait_stream(self.graph_stream)

    def send_weights(self, w):
        """Hand the checked pixel weights ``w`` (None: nothing to do, the library's default is no weights) to the handle for the compute
        call that follows (iodine_set_pixel_weights: consumed and cleared by that call).  Graph mode: through the staging buffer 'w'."""
        if w is None:
            return None
        ws = self.stage('w', w)
        self._set('iodine_set_pixel_weights', _lib.ptr(ws), 1 if ws.dim() == 4 else 0)
        return ws

    @contextlib.contextmanager
    def saving(self, on=True):
        """Option save_for_backward of the library around the call inside (workspace mode 2; see include/iodine_hip.h)."""
        if on:
            self._set('iodine_set_option', b'save_for_backward', 1.0)
        try:
            yield
        finally:
            if on:
                self._set('iodine_set_option', b'save_for_backward', 0.0)

    def profile_read(self, category, reset=True):
        tot, cnt = C.c_double(), C.c_longlong()
        self._set('iodine_profile_read', category.encode(), C.byref(tot), C.byref(cnt), int(reset))
        return tot.value, cnt.value

    def debug_buffer(self, name, iteration=0):
        n = C.c_size_t()
        self._set('iodine_debug_copy', self.stream(), name.encode(), iteration, None, 0, C.byref(n))
        out = torch.empty(n.value, dtype=torch.float32, device=self.device)
        self._set('iodine_debug_copy', self.stream(), name.encode(), iteration, C.c_void_p(out.data_ptr()), n.value, C.byref(n))
        return out

    # With option ``graph`` the library keys its hipGraphs on the full argument tuple, device addresses included.  Tensors the
    # caching allocator hands out per call (inputs made contiguous, noise, outputs, the flat gradient buffer) would change that
    # key from step to step - every call an eager run or a re-capture instead of a replay.  So in graph mode the library only
    # ever sees persistent staging buffers owned by the session: inputs are copied in, outputs are cloned out.  Host-side scalars are baked
    # into captured nodes, so the key also holds the objective (sigma, beta, the weight table): a schedule that changes ``model.beta`` every
    # step sees each key once and simply runs eagerly, a repeated objective is captured and replayed.
    def graph_on(self):
        return bool(self.options.get('graph'))

    def _gbuf(self, name, shape):
        key = (name, tuple(shape))
        t = self.graph_bufs.get(key)
        if t is None:
            t = self.graph_bufs[key] = torch.empty(key[1], device=self.device, dtype=torch.float32)
        return t

    def stage(self, name, t):
        """``t`` as the library should see it: itself, or (graph mode) its copy in the persistent buffer ``name``."""
        if t is None or not self.graph_on():
            return t
        buf = self._gbuf(name, t.shape)
        if buf.data_ptr() != t.data_ptr():
            buf.copy_(t)
        return buf

    def out(self, name, shape):                 # a float32 output: fresh, or (graph mode) the persistent buffer ``name``
        return self._gbuf(name, shape) if self.graph_on() else torch.empty(tuple(shape), device=self.device, dtype=torch.float32)

    def own(self, t):
        """What the caller gets: the tensor itself, or (graph mode) a copy that the next call will not overwrite."""
        return t.clone() if (t is not None and self.graph_on()) else t
