"""The batched top-down renderer (include/hrl_render.h): loader of libhrl_render_hip.so, the ctypes mirror of `hrl_view`, and the launch
behind `BatchedEnv.render()` -- an RGB image of every env of a shard, [N, H, W, 3] uint8 in HBM, from one kernel launch.

The library is the step library's neighbour, not a part of it: `HRL_ENVS_LIB` may point at any build of the step ABI and the renderer
still loads.  There is no CPU fallback: a missing library is an error (`render(mode='rgb_array')` of one env, envs/render.py, is the
host-side debugging aid)."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor

HRL_VIEW_WORLD, HRL_VIEW_EGO, HRL_VIEW_EGO_HEADING = 0, 1, 2
MODES = {'world': HRL_VIEW_WORLD, 'ego': HRL_VIEW_EGO, 'ego_heading': HRL_VIEW_EGO_HEADING}

# the palette of include/hrl_render.h (R, G, B)
PALETTE = {'ground': (240, 240, 240), 'wall': (60, 60, 60), 'box': (170, 170, 170), 'target': (255, 200, 0), 'food': (0, 170, 0), 'poison': (210, 0, 0),
           'leg0': (120, 80, 20), 'leg1': (150, 100, 30), 'leg2': (200, 140, 40), 'torso': (0, 50, 200)}

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_RENDER_LIB') or os.path.join(_PKG, 'libhrl_render_hip.so')
SYMBOLS = ['hrl_render_default_view', 'hrl_render', 'hrl_render_last_error']   # every symbol include/hrl_render.h declares


class hrl_view(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('mode', C.c_int32),
                ('centre', C.c_float * 2), ('half_extent', C.c_float)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_render', 'the batched renderer has', {
    'hrl_render_default_view': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_view)],
    'hrl_render': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_view), C.c_void_p, C.c_void_p, C.c_void_p]})


def _mode(mode):
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f'view mode {mode!r}: one of {sorted(MODES)}')
        return MODES[mode]
    return int(mode)


def default_view(cfg, mode=HRL_VIEW_WORLD, width=64, height=64):
    """The library's default view of `cfg`'s kind (hrl_render_default_view: the whole arena in world mode, 3 m around the robot in the ego
    modes) at width x height pixels.  A world view wider than it is tall is widened so that the arena's height still fits."""
    v = hrl_view()
    check(lib().hrl_render_default_view(C.byref(cfg), _mode(mode), C.byref(v)))
    v.width, v.height = int(width), int(height)
    if v.mode == HRL_VIEW_WORLD and height < width:
        v.half_extent = v.half_extent * width / height
    return v


def render(cfg, bufs_ref, view, mask_ptr, out, stream):
    """One launch: `out` [N, H, W, 3] uint8 on the current device from the buffer record behind `bufs_ref`."""
    check(lib().hrl_render(C.byref(cfg), bufs_ref, C.byref(view), mask_ptr, out.data_ptr(), stream))
    return out


def check_out(out, n, view, device):
    """`out=` of BatchedEnv.render(): uint8 [N, H, W, 3], contiguous, 16-byte aligned, on the env's device."""
    return _sensor.check_tensors((out,), 'out', (('', torch.uint8),), ((n, view.height, view.width, 3),), device, 16)[0]
