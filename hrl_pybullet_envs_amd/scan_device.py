"""The batched range scanner (include/hrl_scan.h): loader of libhrl_scan_hip.so, the ctypes mirror of `hrl_scan_spec`, and the launch
behind `BatchedEnv.scan()` -- a ring of rays per env of a shard, range [N, n_rays] float32 and hit [N, n_rays] int32 in HBM, from one
kernel launch.

Like the renderer's, the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import math
import os

import torch

from . import _capi as K
from . import _sensor

HRL_SCAN_WORLD, HRL_SCAN_HEADING = 0, 1
FRAMES = {'world': HRL_SCAN_WORLD, 'heading': HRL_SCAN_HEADING}
MAX_RAYS = 512
WALL, BOX, FOOD, POISON, TARGET, ALL = 1, 2, 4, 8, 16, 31                      # hrl_scan_spec.classes
HIT_NONE, HIT_WALL, HIT_BOX, HIT_FOOD, HIT_POISON, HIT_TARGET = range(6)       # the low byte of `hit`
HIT_NAMES = ('none', 'wall', 'box', 'food', 'poison', 'target')
FIELDS = (('range', torch.float32), ('hit', torch.int32))                         # the two outputs

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_SCAN_LIB') or os.path.join(_PKG, 'libhrl_scan_hip.so')
SYMBOLS = ['hrl_scan_default_spec', 'hrl_scan', 'hrl_scan_last_error']   # every symbol include/hrl_scan.h declares


class hrl_scan_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('n_rays', C.c_int32), ('frame', C.c_int32), ('first_angle', C.c_float), ('step_angle', C.c_float),
                ('max_range', C.c_float), ('classes', C.c_uint32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_scan', 'the batched range scanner has', {
    'hrl_scan_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_scan_spec)],
    'hrl_scan': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_scan_spec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]})


def _frame(frame):
    if isinstance(frame, str):
        if frame not in FRAMES:
            raise ValueError(f'scan frame {frame!r}: one of {sorted(FRAMES)}')
        return FRAMES[frame]
    return int(frame)


def default_spec(cfg, frame='heading', n_rays=64):
    """The library's default scan of `cfg`'s kind (hrl_scan_default_spec: all classes out to the arena's diagonal) as a full circle of
    `n_rays` rays centred on forward: first_angle = -pi + pi / n_rays, step_angle = 2 pi / n_rays."""
    s = hrl_scan_spec()
    check(lib().hrl_scan_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    if int(n_rays) != s.n_rays:
        s.n_rays = int(n_rays)
        s.first_angle, s.step_angle = -math.pi + math.pi / s.n_rays if s.n_rays > 0 else 0.0, 2 * math.pi / max(s.n_rays, 1)
    return s


def sensor_spec(n_bins, span, max_range, classes=WALL):
    """The rays of the reference's `sense_walls` (sizeable_enclosed_scene.py:66-71) in the heading frame: ray i points at yaw + pi / 2 +
    frac_i * span, frac_i = (i + 1) / n for a span of 2 pi and i / (n - 1) otherwise."""
    n = int(n_bins)
    if span == 2 * math.pi:
        first, step = math.pi / 2 + 2 * math.pi / n, 2 * math.pi / n
    else:
        first, step = math.pi / 2, span / (n - 1)
    return hrl_scan_spec(n_rays=n, frame=HRL_SCAN_HEADING, first_angle=first, step_angle=step, max_range=max_range, classes=classes)


def decode(hit):
    """(class code, index) of a `hit` tensor or array: the low byte and bits 8 and up."""
    return hit & 0xFF, hit >> 8


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    return None if 1 <= spec.n_rays <= MAX_RAYS else f'spec.n_rays must be within 1..{MAX_RAYS}, got {spec.n_rays}'


def scan(cfg, bufs_ref, spec, mask_ptr, rng, hit, stream):
    """One launch: `rng` float32 and `hit` int32, [N, n_rays] on the current device, from the buffer record behind `bufs_ref`."""
    check(lib().hrl_scan(C.byref(cfg), bufs_ref, C.byref(spec), mask_ptr, rng.data_ptr(), hit.data_ptr(), stream))
    return rng, hit


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.scan(): (range float32, hit int32), each contiguous [N, n_rays], 4-byte aligned, on the env's device."""
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise TypeError('out must be a pair (range, hit)')
    _sensor.check_tensors(out, 'out ', FIELDS, ((n, spec.n_rays),) * 2, device, 4)
    return out[0], out[1]
