"""The batched point probes (include/hrl_probe.h): loader of libhrl_probe_hip.so, the ctypes mirrors of `hrl_probe_spec` and
`hrl_probe_out`, and the launch behind `BatchedEnv.probe()` -- for P query points per env of a shard: clearance / nearest, sight /
blocker and path / via, each [N, P] in HBM, from one kernel launch.

Like the renderer's and the scanner's, the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a
missing library is an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor
from .scan_device import ALL, BOX, FOOD, HIT_BOX, HIT_FOOD, HIT_NAMES, HIT_NONE, HIT_POISON, HIT_TARGET, HIT_WALL, POISON, TARGET, WALL, decode  # noqa: F401  (the scanner's classes and codes)

HRL_PROBE_WORLD, HRL_PROBE_EGO, HRL_PROBE_HEADING = 0, 1, 2
FRAMES = {'world': HRL_PROBE_WORLD, 'ego': HRL_PROBE_EGO, 'heading': HRL_PROBE_HEADING}
MAX_POINTS = 512
MAX_MARGIN = 2.0
SKIN = 1e-3
VIA_NONE, VIA_STRAIGHT, VIA_CORNER0 = 0, 1, 2                                    # `via`: 2 + k = the route first turns at corner k

FIELDS = (('clearance', torch.float32), ('nearest', torch.int32), ('sight', torch.float32), ('blocker', torch.int32), ('path', torch.float32), ('via', torch.int32))
Probe, hrl_probe_out = _sensor.out_types('Probe', 'hrl_probe_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_PROBE_LIB') or os.path.join(_PKG, 'libhrl_probe_hip.so')
SYMBOLS = ['hrl_probe_default_spec', 'hrl_probe', 'hrl_probe_last_error']   # every symbol include/hrl_probe.h declares


class hrl_probe_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('n_points', C.c_int32), ('frame', C.c_int32), ('classes', C.c_uint32), ('margin', C.c_float)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_probe', 'the batched point probes have', {
    'hrl_probe_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_probe_spec)],
    'hrl_probe': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_probe_spec), C.c_void_p, C.c_void_p, C.POINTER(hrl_probe_out), C.c_void_p]})


def _frame(frame):
    if isinstance(frame, str):
        if frame not in FRAMES:
            raise ValueError(f'probe frame {frame!r}: one of {sorted(FRAMES)}')
        return FRAMES[frame]
    return int(frame)


def default_spec(cfg, frame='world', n_points=64):
    """The library's default probe of `cfg`'s kind (hrl_probe_default_spec: all classes, margin = the torso's radius, the cube's half
    side for the point bot) for `n_points` points per env in `frame` ('world', 'ego' or 'heading')."""
    s = hrl_probe_spec()
    check(lib().hrl_probe_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    s.n_points = int(n_points)
    return s


def corner_table(cfg, margin):
    """The waypoints `via` indexes, float64 [6, 2] in world coordinates: rows 2 + k are corner k = (+x, +y), (-x, +y), (-x, -y), (+x, -y)
    of the maze box grown by margin + SKIN; rows 0 (unreachable) and 1 (straight) are NaN, and so is every row of a kind without a box.
    (A corner beyond the shrunk arena is listed too; no route turns there.)"""
    t = torch.full((6, 2), float('nan'), dtype=torch.float64)
    if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        (cx, cy), (hx, hy) = (-2.0, 0.0), (3.0, 2.0)   # host_cfg.h build_devcfg: box (-5, -2) .. (1, 2) (box.xml, maze_scene.py)
        e = float(margin) + SKIN
        for k, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
            t[2 + k, 0], t[2 + k, 1] = cx + sx * (hx + e), cy + sy * (hy + e)
    return t


def probe(cfg, bufs_ref, spec, points, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Probe; None fields are not computed), each [N, n_points] on the current device, from the
    buffer record behind `bufs_ref` and `points` float32 [N, n_points, 2]."""
    return _sensor.launch(check, lib().hrl_probe, hrl_probe_out, FIELDS, cfg, bufs_ref, spec, (points.data_ptr(), mask_ptr), out, stream)


def shapes(spec, lead=()):
    """The shape after N of each member of Probe (with `lead` = (N,): the whole shape)."""
    return (lead + (spec.n_points,),) * 6


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    return None if 1 <= spec.n_points <= MAX_POINTS else f'spec.n_points must be within 1..{MAX_POINTS}, got {spec.n_points}'


def check_points(points, n, device):
    """`points` of BatchedEnv.probe(): float32, contiguous [N, P, 2] with 1 <= P <= 512, on the env's device."""
    return _sensor.check_points(points, 'points', MAX_POINTS, n, device)


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.probe(): a Probe whose fields are None (skipped) or contiguous, 4-byte aligned [N, n_points] tensors of the field's dtype
    on the env's device; at least one must be given."""
    return _sensor.check_out(Probe, 'probe_device', FIELDS, shapes(spec, (n,)), out, device, note='None fields are skipped')
