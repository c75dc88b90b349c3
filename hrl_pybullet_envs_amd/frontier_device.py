"""The batched frontier map (include/hrl_frontier.h): loader of libhrl_frontier_hip.so, the ctypes mirrors of `hrl_frontier_spec` and
`hrl_frontier_out`, and the launch behind `BatchedEnv.frontier()` -- for every env of a shard, on the world grid of the visibility map's
memory (`seen` of see_device.py, only read here): where the seen space ends (`edge` uint8 [N, H, W]), the field through what is known
(`dist` float32, `parent` uint8 [N, H, W], the navigation field's codes) and its summary per env (`count` int32 [N] edge cells, `length`
float32 [N] from the robot to the nearest source, `goal` float32 [N, 2] the world place of that source's cell and `cell` int32 [N] its
index), in HBM, from one kernel launch.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor
from .field_device import BLOCKED, DIRECTIONS, MAX_MARGIN, MAX_SIZE, MIN_SIZE, ROBOT, SOURCE, UNREACHED, cell_size, size_error  # noqa: F401  (the field's grid and codes)
from .scan_device import ALL, BOX, FOOD, POISON, TARGET, WALL  # noqa: F401  (the scanner's class bits)

EDGE = 64                                    # HRL_FRONTIER_EDGE: a source bit next to ROBOT | FOOD | POISON | TARGET
KNOWN_ONLY, OPTIMISTIC = 0, 1                # hrl_frontier_spec.unknown
UNKNOWN = {'known': KNOWN_ONLY, 'optimistic': OPTIMISTIC}

FIELDS = (('edge', torch.uint8), ('dist', torch.float32), ('parent', torch.uint8), ('count', torch.int32), ('length', torch.float32), ('goal', torch.float32),
          ('cell', torch.int32))
Frontier, hrl_frontier_out = _sensor.out_types('Frontier', 'hrl_frontier_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_FRONTIER_LIB') or os.path.join(_PKG, 'libhrl_frontier_hip.so')
SYMBOLS = ['hrl_frontier_default_spec', 'hrl_frontier', 'hrl_frontier_last_error']   # every symbol include/hrl_frontier.h declares


class hrl_frontier_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('centre', C.c_float * 2), ('half_extent', C.c_float),
                ('blocking', C.c_uint32), ('sources', C.c_uint32), ('margin', C.c_float), ('unknown', C.c_int32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_frontier', 'the batched frontier map has', {
    'hrl_frontier_default_spec': [C.POINTER(K.hrl_config), C.POINTER(hrl_frontier_spec)],
    'hrl_frontier': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_frontier_spec), C.c_void_p, C.c_void_p, C.POINTER(hrl_frontier_out), C.c_void_p]})


def _unknown(unknown):
    if unknown in UNKNOWN:
        return UNKNOWN[unknown]
    if unknown in UNKNOWN.values():
        return int(unknown)
    raise ValueError(f"unknown must be 'known' or 'optimistic', got {unknown!r}")


def default_spec(cfg, width=64, height=64, sources=EDGE, unknown='known', margin=None):
    """The library's default map of `cfg`'s kind (hrl_frontier_default_spec: the world grid, blocking and margin of
    field_device.default_spec, so the grid of see_device.default_spec) at width x height cells, towards `sources` (EDGE and / or ROBOT,
    FOOD, POISON, TARGET), with unknown cells blocked ('known') or free ('optimistic'), for a disc of `margin` metres (None: the
    default).  Like field_device.default_spec, a grid wider than it is tall is widened so that the arena's height still fits."""
    s = hrl_frontier_spec()
    check(lib().hrl_frontier_default_spec(C.byref(cfg), C.byref(s)))
    s.width, s.height = int(width), int(height)
    if height < width:
        s.half_extent = s.half_extent * width / height
    s.sources, s.unknown = int(sources), _unknown(unknown)
    if margin is not None:
        s.margin = margin
    return s


def spec_like(cfg, see_spec, sources=EDGE, unknown='known', margin=None):
    """default_spec(cfg, ...) on the grid of `see_spec` (an hrl_see_spec in the world mode, or any record with width, height, centre and
    half_extent), so that the memory of BatchedEnv.see(see_spec) lines up with the map cell for cell."""
    if getattr(see_spec, 'mode', 0) != 0:
        raise ValueError("the memory exists on world grids only: see_spec must be in the 'world' mode")
    s = default_spec(cfg, sources=sources, unknown=unknown, margin=margin)
    s.width, s.height, s.half_extent = see_spec.width, see_spec.height, see_spec.half_extent
    s.centre[0], s.centre[1] = see_spec.centre[0], see_spec.centre[1]
    return s


def shapes(spec, lead=()):
    """The shape after N of each member of Frontier (with `lead` = (N,): the whole shape)."""
    grid = lead + (spec.height, spec.width)
    return (grid, grid, grid, lead, lead, lead + (2,), lead)


def frontier(cfg, bufs_ref, spec, seen_ptr, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Frontier; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref` and the memory at `seen_ptr`, which is only read."""
    return _sensor.launch(check, lib().hrl_frontier, hrl_frontier_out, FIELDS, cfg, bufs_ref, spec, (seen_ptr, mask_ptr), out, stream)


def check_seen(seen, n, spec, device):
    """`seen` of BatchedEnv.frontier(): the memory of BatchedEnv.see() on the same grid -- a contiguous, 4-byte aligned uint8 [N, height,
    width] tensor on the env's device."""
    _sensor.check_tensors((seen,), '', (('seen', torch.uint8),), ((n, spec.height, spec.width),), device, 4)
    return seen


def check_out(out, n, spec, device, seen=None):
    """`out=` of BatchedEnv.frontier(): a Frontier whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's
    dtype -- edge, dist and parent [N, height, width], count, length and cell [N], goal [N, 2] -- on the env's device; at least one must
    be given.  `edge` and `parent` must not be the memory of `seen` (the library refuses that too)."""
    _sensor.check_out(Frontier, 'frontier_device', FIELDS, shapes(spec, (n,)), out, device)
    if seen is not None:
        for name in ('edge', 'parent'):
            t = getattr(out, name)
            if t is not None and t.data_ptr() == seen.data_ptr():
                raise ValueError(f'out.{name} and seen must not be the same memory: seen is only read')
    return out
