"""The batched navigation field (include/hrl_field.h): loader of libhrl_field_hip.so, the ctypes mirrors of `hrl_field_spec` and
`hrl_field_out`, and the launch behind `BatchedEnv.field()` -- for every env of a shard a top-down grid of the length of the shortest
8-connected way to the nearest source cell (`dist` float32 [N, H, W]) and the step that way takes (`parent` uint8 [N, H, W]), in HBM, from
one kernel launch.  The grid is the renderer's pixel grid: a field and an image of the same mode, size and extent line up cell for pixel.

Like the renderer's, the scanner's and the probes', the library is the step library's neighbour, not a part of it.  There is no CPU
fallback: a missing library is an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor
from .render_device import HRL_VIEW_EGO, HRL_VIEW_EGO_HEADING, HRL_VIEW_WORLD, MODES, _mode  # noqa: F401  (the renderer's modes)
from .scan_device import ALL, BOX, FOOD, POISON, TARGET, WALL  # noqa: F401  (the scanner's class bits)

ROBOT = 32                                   # HRL_FIELD_ROBOT: a source bit next to FOOD | POISON | TARGET
MIN_SIZE, MAX_SIZE = 8, 64
MAX_MARGIN = 2.0
SOURCE, UNREACHED, BLOCKED = 8, 9, 10        # `parent` beyond the direction codes 0..7
DIRECTIONS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))   # (dcol, drow) of code 0..7 = E, NE, N, NW, W, SW, S, SE; row - 1 is N
SQRT2 = 1.41421354

FIELDS = (('dist', torch.float32), ('parent', torch.uint8))
Field, hrl_field_out = _sensor.out_types('Field', 'hrl_field_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_FIELD_LIB') or os.path.join(_PKG, 'libhrl_field_hip.so')
SYMBOLS = ['hrl_field_default_spec', 'hrl_field', 'hrl_field_last_error']   # every symbol include/hrl_field.h declares


class hrl_field_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('mode', C.c_int32), ('centre', C.c_float * 2),
                ('half_extent', C.c_float), ('blocking', C.c_uint32), ('sources', C.c_uint32), ('margin', C.c_float)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_field', 'the batched navigation field has', {
    'hrl_field_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_field_spec)],
    'hrl_field': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_field_spec), C.c_void_p, C.POINTER(hrl_field_out), C.c_void_p]})


def default_spec(cfg, mode='world', width=64, height=64):
    """The library's default field of `cfg`'s kind (hrl_field_default_spec: the renderer's default view, blocking = WALL | BOX | POISON,
    margin = the torso's radius, sources = TARGET for the maze kinds and flagrun, FOOD for the gather kinds, ROBOT for the flat kind) at
    width x height cells in `mode` ('world', 'ego' or 'ego_heading').  Like render_device.default_view, a world grid wider than it is
    tall is widened so that the arena's height still fits."""
    s = hrl_field_spec()
    check(lib().hrl_field_default_spec(C.byref(cfg), _mode(mode), C.byref(s)))
    s.width, s.height = int(width), int(height)
    if s.mode == HRL_VIEW_WORLD and height < width:
        s.half_extent = s.half_extent * width / height
    return s


def cell_size(spec):
    """Metres per cell: w1, the cost of an orthogonal step (a diagonal one costs cell_size * SQRT2)."""
    return 2.0 / spec.width * spec.half_extent


def axes(spec, state):
    """(centre, right, up) of the grid per env, float32 [N, 2] each in world coordinates: hrl_view's camera (render_core.h: view_frame),
    in torch on `state`'s device."""
    n = state.shape[0]
    right = torch.tensor([1.0, 0.0], device=state.device).expand(n, 2)
    up = torch.tensor([0.0, 1.0], device=state.device).expand(n, 2)
    centre = torch.tensor([spec.centre[0], spec.centre[1]], device=state.device).expand(n, 2)
    if spec.mode != HRL_VIEW_WORLD:
        centre = state[:, 0:2]
    if spec.mode == HRL_VIEW_EGO_HEADING:
        x, y, z, w = state[:, 3], state[:, 4], state[:, 5], state[:, 6]
        fx, fy = 1 - 2 * (y * y + z * z), 2 * (x * y + w * z)   # the ground projection of the torso's body X axis
        n2 = fx * fx + fy * fy
        ok = ((n2 >= 1e-12) & (n2 <= 3.0e38)).unsqueeze(1)
        f = torch.stack([fx, fy], 1) / torch.sqrt(torch.where(ok[:, 0], n2, torch.ones_like(n2))).unsqueeze(1)
        up = torch.where(ok, f, up)
        right = torch.where(ok, torch.stack([f[:, 1], -f[:, 0]], 1), right)
    return centre, right, up


def direction_vectors(spec, state):
    """The eight unit steps in world axes per env: float32 [N, 8, 2]; row k is where the step `parent == k` leads (E = the grid's right,
    N = its up).  `state`: the env's state tensor [N, 32]."""
    _, right, up = axes(spec, state)
    d = torch.tensor(DIRECTIONS, dtype=torch.float32, device=state.device)
    d = d / d.norm(dim=1, keepdim=True)
    return d[None, :, 0:1] * right[:, None, :] - d[None, :, 1:2] * up[:, None, :]


def cell_index(spec, state, xy):
    """World points `xy` [N, P, 2] -> (row, col), int64 [N, P] each: the cell whose square holds the point.  A point outside the grid
    gets an index outside 0..H-1 / 0..W-1 (clamp or mask as needed); a point that is not finite gets -1."""
    centre, right, up = axes(spec, state)
    d = xy - centre[:, None, :]
    u, v = (d * right[:, None, :]).sum(-1), (d * up[:, None, :]).sum(-1)
    cell = cell_size(spec)
    col = torch.floor(u / cell + spec.width / 2)
    row = torch.floor(spec.height / 2 - v / cell)
    bad = ~(torch.isfinite(col) & torch.isfinite(row))
    return torch.where(bad, -torch.ones_like(row), row).long(), torch.where(bad, -torch.ones_like(col), col).long()


def field(cfg, bufs_ref, spec, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Field; a None one is not computed), each [N, height, width] on the current device, from the
    buffer record behind `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_field, hrl_field_out, FIELDS, cfg, bufs_ref, spec, (mask_ptr,), out, stream)


def shapes(spec, lead=()):
    """The shape after N of each member of Field (with `lead` = (N,): the whole shape)."""
    return (lead + (spec.height, spec.width),) * 2


def size_error(spec):
    """Why no tensors can be shaped after the spec's grid (the library refuses it too), or None.  The grids of see_device and
    frontier_device are this one."""
    if MIN_SIZE <= spec.width <= MAX_SIZE and MIN_SIZE <= spec.height <= MAX_SIZE:
        return None
    return f'spec.width and spec.height must be within {MIN_SIZE}..{MAX_SIZE}, got {spec.width} x {spec.height}'


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.field(): a Field whose members are None (skipped) or contiguous, 4-byte aligned [N, height, width] tensors of the
    member's dtype on the env's device; at least one must be given."""
    return _sensor.check_out(Field, 'field_device', FIELDS, shapes(spec, (n,)), out, device)
