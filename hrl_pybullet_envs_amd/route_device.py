"""The batched routes (include/hrl_route.h): loader of libhrl_route_hip.so, the ctypes mirrors of `hrl_route_spec` and `hrl_route_out`,
and the launch behind `BatchedEnv.route()` -- for P start points per env of a shard the way to the nearest source of the env's navigation
field, pulled tight into at most K waypoints: `waypoints` float32 [N, P, K, 2] (world x, y), `count` int32 [N, P], `length` float32
[N, P] and `cells` int32 [N, P, K] (row * width + column on the field's grid), in HBM, from one kernel launch.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor
from .field_device import ALL, BLOCKED, BOX, DIRECTIONS, FOOD, POISON, ROBOT, SOURCE, TARGET, UNREACHED, WALL, cell_size  # noqa: F401  (the field's bits and codes)
from .probe_device import FRAMES, HRL_PROBE_EGO, HRL_PROBE_HEADING, HRL_PROBE_WORLD, _frame  # noqa: F401  (the probe's frames)
from .render_device import HRL_VIEW_EGO, HRL_VIEW_EGO_HEADING, HRL_VIEW_WORLD, MODES, _mode  # noqa: F401  (the renderer's modes)

MAX_STARTS = 64
MIN_WAYPOINTS, MAX_WAYPOINTS = 2, 32

FIELDS = (('waypoints', torch.float32), ('count', torch.int32), ('length', torch.float32), ('cells', torch.int32))
Route, hrl_route_out = _sensor.out_types('Route', 'hrl_route_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_ROUTE_LIB') or os.path.join(_PKG, 'libhrl_route_hip.so')
SYMBOLS = ['hrl_route_default_spec', 'hrl_route', 'hrl_route_last_error']   # every symbol include/hrl_route.h declares


class hrl_route_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('mode', C.c_int32), ('centre', C.c_float * 2),
                ('half_extent', C.c_float), ('blocking', C.c_uint32), ('sources', C.c_uint32), ('margin', C.c_float),
                ('n_starts', C.c_int32), ('frame', C.c_int32), ('max_waypoints', C.c_int32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_route', 'the batched routes have', {
    'hrl_route_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_route_spec)],
    'hrl_route': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_route_spec), C.c_void_p, C.c_void_p, C.POINTER(hrl_route_out), C.c_void_p]})


def default_spec(cfg, mode='world', width=64, height=64, frame='ego', n_starts=1, max_waypoints=16):
    """The library's default route of `cfg`'s kind (hrl_route_default_spec: the field of field_device.default_spec, starts given as
    offsets from the robot, 16 waypoints) at width x height cells in `mode`, for `n_starts` starts per env in `frame` ('world', 'ego' or
    'heading').  Like field_device.default_spec, a world grid wider than it is tall is widened so that the arena's height still fits."""
    s = hrl_route_spec()
    check(lib().hrl_route_default_spec(C.byref(cfg), _mode(mode), C.byref(s)))
    s.width, s.height = int(width), int(height)
    if s.mode == HRL_VIEW_WORLD and height < width:
        s.half_extent = s.half_extent * width / height
    s.frame, s.n_starts, s.max_waypoints = _frame(frame), int(n_starts), int(max_waypoints)
    return s


def field_spec(spec):
    """The hrl_field_spec whose field the routes of `spec` run on: BatchedEnv.field(field_spec(spec)) is that field."""
    from .field_device import hrl_field_spec
    return hrl_field_spec(width=spec.width, height=spec.height, mode=spec.mode, centre=spec.centre, half_extent=spec.half_extent, blocking=spec.blocking,
                          sources=spec.sources, margin=spec.margin)


def from_field_spec(fspec, frame='ego', n_starts=1, max_waypoints=16):
    """The route spec on the field of the hrl_field_spec `fspec`."""
    return hrl_route_spec(width=fspec.width, height=fspec.height, mode=fspec.mode, centre=fspec.centre, half_extent=fspec.half_extent, blocking=fspec.blocking,
                          sources=fspec.sources, margin=fspec.margin, n_starts=int(n_starts), frame=_frame(frame), max_waypoints=int(max_waypoints))


def shapes(spec, lead=()):
    """The shape after N of each member of Route (with `lead` = (N,): the whole shape)."""
    starts = lead + (spec.n_starts,)
    kept = starts + (spec.max_waypoints,)
    return (kept + (2,), starts, starts, kept)


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    if MIN_WAYPOINTS <= spec.max_waypoints <= MAX_WAYPOINTS:
        return None
    return f'spec.max_waypoints must be within {MIN_WAYPOINTS}..{MAX_WAYPOINTS}, got {spec.max_waypoints}'


def route(cfg, bufs_ref, spec, starts, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Route; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref` and `starts` float32 [N, n_starts, 2] (None: the robot's place)."""
    return _sensor.launch(check, lib().hrl_route, hrl_route_out, FIELDS, cfg, bufs_ref, spec, (None if starts is None else starts.data_ptr(), mask_ptr), out, stream)


def check_starts(starts, n, device):
    """`starts` of BatchedEnv.route(): float32, contiguous [N, P, 2] with 1 <= P <= 64, on the env's device."""
    return _sensor.check_points(starts, 'starts', MAX_STARTS, n, device)


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.route(): a Route whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's dtype
    and shape (shapes(spec) after N) on the env's device; at least one must be given."""
    return _sensor.check_out(Route, 'route_device', FIELDS, shapes(spec, (n,)), out, device)
