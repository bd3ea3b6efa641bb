"""ctypes binding of libiodine_hip.so (the C ABI declared in include/iodine_hip.h).

There is deliberately no fallback: if the shared library is missing or a call fails the
error is raised, never papered over with a PyTorch / CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# IODINE_HIP_LIB selects another build of the same library (tools/ab_libs.sh: same-box A/B of two builds)
LIB_PATH = os.environ.get('IODINE_HIP_LIB') or os.path.join(_HERE, 'libiodine_hip.so')

ENC_ORDER = ('posterior', 'grad_post', 'image', 'means', 'mask', 'mask_logits', 'mask_posterior',
             'grad_means', 'grad_mask', 'likelihood', 'leave_one_out_likelihood', 'coordinate')
ENC_FULL = 0xFFF

class Config(C.Structure):
    _fields_ = [
        ('dim_latent', C.c_int), ('iters', C.c_int), ('slots', C.c_int), ('img_size', C.c_int),
        ('img_channels', C.c_int), ('sigma', C.c_double), ('layernorm', C.c_int), ('stop_gradient', C.c_int),
        ('encoding', C.c_uint), ('ref_conv_chan', C.c_int), ('ref_conv_layers', C.c_int),
        ('ref_mlp_units', C.c_int), ('ref_kernel_size', C.c_int), ('ref_stride', C.c_int),
        ('dec_conv_chan', C.c_int), ('dec_conv_layers', C.c_int), ('dec_kernel_size', C.c_int),
    ]


class SheetSpec(C.Structure):
    """``iodine_sheet_spec`` (include/iodine_hip.h): sizes, panel list and colours of one decomposition sheet"""
    _fields_ = [
        ('rows', C.c_int), ('slots', C.c_int), ('n_gt', C.c_int), ('size', C.c_int), ('scale', C.c_int), ('pad', C.c_int),
        ('n_panels', C.c_int), ('draw_edges', C.c_int), ('background', C.c_float * 3), ('alpha', C.c_float), ('error_gain', C.c_float),
        ('pad_value', C.c_ubyte * 3), ('edge', C.c_ubyte * 3), ('panel_kind', C.c_ubyte * 64), ('panel_slot', C.c_ubyte * 64),
        ('palette', C.c_ubyte * 51),
    ]


class AdaptiveCtl(C.Structure):
    """``iodine_adaptive_ctl`` (include/iodine_hip.h): the controls of the adaptive stopping rule"""
    _fields_ = [('max_iters', C.c_int), ('min_iters', C.c_int), ('check_every', C.c_int), ('tol', C.c_double), ('rtol', C.c_double)]


class MoveEntry(C.Structure):
    """``iodine_move_entry`` (include/iodine_hip.h): one row gather / scatter of ``iodine_adaptive_move``"""
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('row_floats', C.c_longlong), ('src_index', C.c_void_p), ('dst_index', C.c_void_p),
                ('rows', C.c_int), ('src_rows', C.c_int), ('dst_rows', C.c_int)]


_vp, _ci, _cf, _dbl, _ll, _ull, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong, C.c_size_t
_FP, _VPP, _CIP = C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_int)

# Every symbol include/iodine_hip.h declares: name -> (argtypes or None, restype - int status unless given).  ``lib()`` applies the rows
# the loaded library has: a build loaded through IODINE_HIP_LIB for same-box A/B may predate the later groups.
_SYMBOLS = {
    'iodine_abi_version': (None, _ci),
    'iodine_create': ([C.POINTER(Config), _VPP],),
    'iodine_destroy': ([_vp], None),
    'iodine_last_error': ([_vp], C.c_char_p),
    'iodine_num_params': ([_vp],),
    'iodine_param_info': ([_vp, _ci, C.POINTER(C.c_char_p), _CIP, C.POINTER(_ll)],),
    'iodine_set_params': ([_vp, _vp, _VPP, _ci],),
    'iodine_workspace_bytes': ([_vp, _ci, _ci], _sz),
    'iodine_set_workspace': ([_vp, _vp, _sz],),
    'iodine_set_run_shape': ([_vp, _ci, _ci],),
    'iodine_reconstruct': ([_vp, _vp, _ci] + [_vp] * 9,),
    'iodine_decode': ([_vp, _vp, _ci] + [_vp] * 4,),
    'iodine_elbo': ([_vp, _vp, _ci] + [_vp] * 5,),
    'iodine_last_elbo_outputs': ([_vp, _vp, _ci] + [_vp] * 5,),
    'iodine_last_posterior': ([_vp, _vp, _ci, _vp, _vp],),
    'iodine_randn': ([_vp, _vp, _ll, _ull, _ull],),
    'iodine_train_forward': ([_vp, _vp, _ci] + [_vp] * 4,),
    'iodine_train_backward': ([_vp, _vp, _cf, _VPP, _ci],),
    'iodine_train_backward_flat': ([_vp, _vp, _vp, _vp, _ci],),
    'iodine_logger_scalars': ([_vp, _vp, _vp],),
    'iodine_adam_step': ([_vp, _vp, _vp, _ci, _ll] + [_dbl] * 5 + [_ci],),
    'iodine_ari_table': ([_vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp],),
    'iodine_set_option': ([_vp, C.c_char_p, _dbl],),
    'iodine_profile_read': ([_vp, C.c_char_p, C.POINTER(_dbl), C.POINTER(_ll), _ci],),
    'iodine_debug_copy': ([_vp, _vp, C.c_char_p, _ci, _vp, _sz, C.POINTER(_sz)],),
    'iodine_linspace_host': ([_ci, _FP], None),
    'iodine_op_conv3x3': ([_vp, _ci] + [_vp] * 5 + [_ci] * 10,),
    'iodine_op_dec_out': ([_vp] + [_vp] * 4 + [_ci] * 3,),
    'iodine_op_conv3x3_wgrad': ([_vp] + [_vp] * 4 + [_ci] * 6,),
    'iodine_op_conv3x3_wgrad_f32': ([_vp] + [_vp] * 4 + [_ci] * 3,),
    'iodine_op_dec_out_f16x3': ([_vp] + [_vp] * 4 + [_ci] * 4,),
    'iodine_op_gen_conv': ([_vp, _ci] + [_vp] * 6 + [_ci] * 8,),
    'iodine_op_gen_conv_f16x3': ([_vp, _ci] + [_vp] * 6 + [_ci] * 8,),
    # kernel-level tests of the generic stride-1 convs and broadcast layer
    'iodine_op_gen_conv_tier': ([_ci] * 7,),
    'iodine_op_gen_l0': ([_vp, _ci] + [_vp] * 8 + [_ci] * 6 + [_cf],),
    # global-norm gradient clipping fused into the Adam step
    'iodine_grad_norm_scratch_bytes': ([_ll], _sz),
    'iodine_grad_norm': ([_vp, _vp, _vp, _ci, _ll, _dbl, _vp, _sz, _vp],),
    'iodine_grad_scale': ([_vp, _vp, _vp, _ci, _ll, _vp],),
    'iodine_adam_step_clipped': ([_vp, _vp, _vp, _ci, _ll] + [_dbl] * 5 + [_ci, _vp, _ci],),
    # differentiable decode / elbo
    'iodine_decode_backward': ([_vp, _vp, _ci] + [_vp] * 5 + [_ci],),
    'iodine_elbo_backward': ([_vp, _vp] + [_vp] * 4 + [_ci],),
    'iodine_op_render_bwd': ([_vp] + [_vp] * 5 + [_ci] * 4,),
    # video input / resumable refinement
    'iodine_set_frames': ([_vp, _ci],),
    'iodine_reconstruct_seq': ([_vp, _vp, _ci] + [_vp] * 9 + [_VPP, _VPP],),
    'iodine_last_refine_state': ([_vp, _vp, _ci, _vp, _vp],),
    # auxiliary cotangents on the training forward
    'iodine_train_backward_aux': ([_vp, _vp] + [_vp] * 8 + [_ci],),
    'iodine_op_render_bwd_logits': ([_vp] + [_vp] * 6 + [_ci] * 4,),
    # model.sigma / beta / iter_weights (a build without it runs the default objective)
    'iodine_set_objective': ([_vp, _dbl, _dbl, C.POINTER(_dbl), _ci],),
    # training from a carried state
    'iodine_train_forward_seq': ([_vp, _vp, _ci, _vp, _vp, _VPP, _vp, _vp],),
    'iodine_train_backward_seq': ([_vp, _vp] + [_vp] * 10 + [_ci, _VPP],),
    'iodine_last_train_state': ([_vp, _vp, _ci, _vp, _vp],),
    # weights= (a build without it refuses the keyword)
    'iodine_set_pixel_weights': ([_vp, _vp, _ci],),
    # the wrapper's one training forward / backward (a build without them cannot train)
    'iodine_train_forward_frames': ([_vp, _vp, _ci, _vp, _vp, _VPP, _vp, _vp, _CIP, _ci, _VPP],),
    'iodine_train_backward_frames': ([_vp, _vp] + [_vp] * 10 + [_ci, _VPP, _CIP, _ci, _VPP],),
    # a sigma that requires grad (a build without it raises on one)
    'iodine_last_sigma_grad': ([_vp, _vp, _vp, _ci],),
    # x / weights that require grad, likelihood maps (a build without them raises on them)
    'iodine_last_input_grad': ([_vp, _vp, _vp, _vp],),
    'iodine_last_likelihood': ([_vp, _vp, _ci, _vp, _vp],),
    'iodine_op_pixel_maps': ([_vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _ci, _cf, _vp, _vp, _vp, _vp, _ci],),
    # kernel-level tests of the refinement head
    'iodine_op_sgemm': ([_vp] + [_ci] * 6 + [_cf, _vp, _ci, _vp, _ci, _cf, _vp, _ci, _ci],),
    'iodine_op_colsum': ([_vp, _ci, _vp, _ci, _ci, _ci, _cf, _vp],),
    'iodine_op_refine_head': ([_vp, _ci, _VPP, _VPP] + [_ci] * 5,),
    'iodine_op_refine_head_form': ([_ci] * 4,),
    'iodine_op_head_bptt': ([_vp, _ci, _VPP, _VPP] + [_ci] * 6 + [_ll],),
    'iodine_op_pool_bwd': ([_vp, _vp, _vp, _vp, _ci, _ci, _ci],),
    # object tables, iodine_amd.objects
    'iodine_slot_table': ([_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp],),
    'iodine_seg_overlap': ([_vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp],),
    # connected components, iodine_amd.objects.components
    'iodine_seg_components_scratch_bytes': ([_ci, _ci], _sz),
    'iodine_seg_components': ([_vp, _vp] + [_ci] * 6 + [_vp] * 7 + [_sz],),
    'iodine_seg_components_host': ([_vp] + [_ci] * 5 + [_vp] * 6,),
    # refinement restarts, iodine_amd.chains / IODINE.restarts (a build without them raises on it)
    'iodine_chain_score': ([_vp] * 5 + [_ci] * 4 + [_dbl, _ci, _vp, _vp],),
    'iodine_chain_consensus': ([_vp] * 5 + [_ci] * 4 + [_vp] * 5,),
    # adaptive refinement, iodine_amd.adaptive / IODINE.reconstruct_adaptive (a build without them raises on it)
    'iodine_adaptive_select': ([_vp, _vp, _vp, _ci, _ci, _ci, _ci, C.POINTER(AdaptiveCtl), _dbl] + [_vp] * 9,),
    'iodine_adaptive_move': ([_vp, C.POINTER(MoveEntry), _ci],),
    'iodine_reconstruct_adaptive': ([_vp, _vp, _ci, _vp, _vp, C.POINTER(AdaptiveCtl), _vp, _VPP] + [_vp] * 11 + [_CIP],),
    # IODINE.edit, iodine_amd.traverse (a build without it raises on them)
    'iodine_scene_edit': ([_vp, _vp, _ci, _vp, _ci, _CIP, _CIP, _CIP, _vp, _ci] + [_vp] * 6,),
    # kernel-level tests of the per-pixel mixture kernels
    'iodine_op_pixel_encode': ([_vp] * 7 + [_ci] * 4 + [_cf, _cf, _ci, C.c_uint, _ci, _VPP],),
    # IODINE.predictive (a build without it raises on it)
    'iodine_predictive': ([_vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _ci] + [_vp] * 7,),
    # matched masks, iodine_amd.matching
    'iodine_mask_overlap': ([_vp, _vp, _vp, _ci, _ci, _ci, _ci, _cf, _vp, _vp, _vp, _vp],),
    'iodine_assign': ([_vp, _vp, _vp, _ci, _ci, _ci, _vp, _vp],),
    'iodine_assign_host': ([_vp, _vp, _ci, _ci, _vp, _vp],),
    'iodine_mask_match': ([_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp],),
    'iodine_mask_match_backward': ([_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cf, _vp],),
    # device-resident datasets, iodine_amd.resident
    'iodine_batch_gather': ([_vp, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _vp, _vp],),
    'iodine_synth_scenes': ([_vp, _ci, _ci] + [_ull] * 4 + [_ci, _ci, _ci, _vp, _vp, _vp],),
    # windowed batches, iodine_amd.windows
    'iodine_batch_window': ([_vp, _vp, _ci, _vp, _ci, _vp, _ci, _ci, _vp, _ci, _ci, _vp, _vp],),
    # decomposition sheets, iodine_amd.figures
    'iodine_sheet_size': ([C.POINTER(SheetSpec), _CIP, _CIP],),
    'iodine_sheet_form': ([C.POINTER(SheetSpec)] + [_vp] * 6,),
    'iodine_render_sheet': ([_vp, C.POINTER(SheetSpec)] + [_vp] * 8,),
}
EXPORTS = tuple(_SYMBOLS)

_lib = None


def encoding_bits(names) -> int:
    bits = 0
    for n in names:
        if n not in ENC_ORDER:
            raise ValueError(f'unknown ARCH.ENCODING entry {n!r}')
        bits |= 1 << ENC_ORDER.index(n)
    return bits


def lib() -> C.CDLL:
    """Load the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -m iodine_amd.build` '
                           '(there is no CPU / PyTorch fallback for this path)')
    # torch is imported first (above): its bundled libamdhip64 (same soname) then serves both torch and this
    # library, so streams and device pointers are shared within ONE HIP runtime instance.
    L = C.CDLL(LIB_PATH)
    for name, (argtypes, *restype) in _SYMBOLS.items():
        fn = getattr(L, name, None)
        if fn is None:
            continue
        if argtypes is not None:
            fn.argtypes = argtypes
        if restype:
            fn.restype = restype[0]
    if L.iodine_abi_version() != 3:
        raise RuntimeError('libiodine_hip.so ABI version mismatch')
    _lib = L
    return L


def check(rc: int, handle=None, what: str = ''):
    if rc != 0:
        msg = lib().iodine_last_error(handle)
        raise RuntimeError(f'{what or "libiodine_hip"} failed (status {rc}): '
                           f'{msg.decode() if msg else "unknown error"}')


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return C.c_void_p(t.data_ptr())


def stream():
    """The current torch stream, as the entry points take it."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fn(symbol):
    """The entry point ``symbol`` of the loaded library (a build loaded through IODINE_HIP_LIB may predate it: that is an error)."""
    f = getattr(lib(), symbol, None)
    if f is None:
        raise RuntimeError(f'IODINE: this build of libiodine_hip.so has no {symbol}')
    return f


def call(symbol, device, *args):
    """``symbol(stream, *args)``: the one place a handle-free entry point is invoked - on the current stream with ``device`` current;
    tensors and None go as pointers, everything else (numbers, ``byref``, raw ``c_void_p``) as given.  Raises on a non-zero status.
    (The entry points that take a handle go through ``Session.call``.)"""
    f = fn(symbol)
    args = [ptr(a) if a is None or torch.is_tensor(a) else a for a in args]
    with torch.cuda.device(device):
        rc = f(stream(), *args)
    check(rc, None, symbol)


def ptrs(tensors, ctype=C.c_void_p):
    """A C array of the device pointers of ``tensors`` (None -> NULL), for the entry points that take a pointer table."""
    return (ctype * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def ints(values, ctype=C.c_int):
    """A C array of host numbers (``int`` by default)."""
    return (ctype * len(values))(*values)


def as_float32(v) -> float:
    """``v`` rounded to float32, as the library will read it."""
    return C.c_float(v).value
