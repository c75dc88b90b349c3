"""The batched visibility map (include/hrl_see.h): loader of libhrl_see_hip.so, the ctypes mirrors of `hrl_see_spec` and `hrl_see_out`,
and the launch behind `BatchedEnv.see()` -- for every env of a shard, on the field's and the renderer's grid, which cells the robot can see
right now (`visible` uint8 [N, H, W]), which it has seen so far in this episode (`seen` uint8 [N, H, W], a memory the caller holds: read
and written) and how many it saw for the first time (`fresh` int32 [N]), in HBM, from one kernel launch.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import math
import os

import torch

from . import _capi as K
from . import _sensor
from .field_device import MAX_SIZE, MIN_SIZE, cell_size, size_error  # noqa: F401  (the field's grid)
from .render_device import HRL_VIEW_EGO, HRL_VIEW_EGO_HEADING, HRL_VIEW_WORLD, MODES, _mode  # noqa: F401  (the renderer's modes)
from .scan_device import ALL, BOX, FOOD, POISON, TARGET, WALL  # noqa: F401  (the scanner's class bits)

MAX_SLACK = 2.0   # HRL_PROBE_MAX_MARGIN

FIELDS = (('visible', torch.uint8), ('seen', torch.uint8), ('fresh', torch.int32))
See, hrl_see_out = _sensor.out_types('See', 'hrl_see_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_SEE_LIB') or os.path.join(_PKG, 'libhrl_see_hip.so')
SYMBOLS = ['hrl_see_default_spec', 'hrl_see', 'hrl_see_last_error']   # every symbol include/hrl_see.h declares


class hrl_see_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('mode', C.c_int32), ('centre', C.c_float * 2),
                ('half_extent', C.c_float), ('occluders', C.c_uint32), ('max_range', C.c_float), ('fov_cos', C.c_float), ('slack', C.c_float)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_see', 'the batched visibility map has', {
    'hrl_see_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_see_spec)],
    'hrl_see': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_see_spec), C.c_void_p, C.c_void_p, C.POINTER(hrl_see_out), C.c_void_p]})


def one_cell(spec):
    """The width of a cell as the library computes it in fp32, (2 / width) * half_extent, as a slack: at most MAX_SLACK (a coarse grid
    of a large arena has wider cells than the library accepts as slack)."""
    return min(C.c_float(C.c_float(2.0 / spec.width).value * spec.half_extent).value, MAX_SLACK)


def default_spec(cfg, mode='world', width=64, height=64, fov_degrees=360, max_range=None, slack=None):
    """The library's default map of `cfg`'s kind (hrl_see_default_spec: the grid of field_device.default_spec, occluders = WALL | BOX,
    max_range = the scanner's, the arena's diagonal) at width x height cells in `mode` ('world', 'ego' or 'ego_heading'), with a field of
    view of `fov_degrees` about the robot's heading (360 = all round), `max_range` metres (None: the default) and `slack` metres (None:
    one cell of the resized grid, at most MAX_SLACK).  Like field_device.default_spec, a world grid wider than it is tall is widened so that the arena's
    height still fits."""
    s = hrl_see_spec()
    check(lib().hrl_see_default_spec(C.byref(cfg), _mode(mode), C.byref(s)))
    s.width, s.height = int(width), int(height)
    if s.mode == HRL_VIEW_WORLD and height < width:
        s.half_extent = s.half_extent * width / height
    s.fov_cos = -1.0 if fov_degrees >= 360 else math.cos(math.radians(fov_degrees) / 2)
    if max_range is not None:
        s.max_range = max_range
    s.slack = one_cell(s) if slack is None else slack
    return s


def memory(n, spec, device):
    """The zeroed `seen` tensor of `n` envs on the grid of `spec`: uint8 [n, height, width] on `device`."""
    return torch.zeros(n, spec.height, spec.width, dtype=torch.uint8, device=device)


def shapes(spec, lead=()):
    """The shape after N of each member of See (with `lead` = (N,): the whole shape)."""
    grid = lead + (spec.height, spec.width)
    return (grid, grid, lead)


def see(cfg, bufs_ref, spec, clear_ptr, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a See; a None one is not computed; `seen` is read and written) on the current device, from the
    buffer record behind `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_see, hrl_see_out, FIELDS, cfg, bufs_ref, spec, (clear_ptr, mask_ptr), out, stream)


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.see(): a See whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's dtype --
    visible and seen [N, height, width], fresh [N] -- on the env's device; at least one must be given.  `seen` needs the world mode, `fresh`
    needs `seen`, and `visible` and `seen` must be different memory (the library refuses these too)."""
    _sensor.check_out(See, 'see_device', FIELDS, shapes(spec, (n,)), out, device)
    if out.seen is not None and spec.mode != HRL_VIEW_WORLD:
        raise ValueError("out.seen needs a spec in the 'world' mode: an ego grid moves under the memory")
    if out.fresh is not None and out.seen is None:
        raise ValueError('out.fresh needs out.seen: it counts the cells the memory did not hold')
    if out.visible is not None and out.seen is not None and out.visible.data_ptr() == out.seen.data_ptr():
        raise ValueError('out.visible and out.seen must not be the same memory')
    return out
