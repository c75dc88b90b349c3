"""The batched chase camera (include/hrl_chase.h): loader of libhrl_chase_hip.so, the ctypes mirrors of `hrl_chase_spec` and
`hrl_chase_out`, and the launch behind `BatchedEnv.chase()` -- for every env of a shard a pinhole image from a camera that orbits the
robot at a distance, a yaw and a pitch and looks at it, the robot's body in the picture: `depth` float32 [N, H, W] (metres along the
optical axis), `seg` int32 [N, H, W] (which shape or which link, and which face) and `rgb` uint8 [N, H, W, 3], in HBM, from one kernel
launch.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import math
import os

import torch

from . import _capi as K
from . import _sensor
from .camera_device import (ALL, BOX, EYES, FACE_BOTTOM, FACE_GROUND, FACE_INSIDE, FACE_ROUND, FACE_SIDE_X, FACE_SIDE_Y, FACE_TOP, FACES, FOOD, FRAMES,  # noqa: F401  (the camera's class bits, hit codes, faces and target modes)
                            GROUND, HIT_BOX, HIT_FOOD, HIT_GROUND, HIT_NONE, HIT_POISON, HIT_TARGET, HIT_WALL, HRL_EYE_GROUND, HRL_EYE_TORSO, HRL_SCAN_HEADING,
                            HRL_SCAN_WORLD, POISON, RGB_SKY, SHADES, TARGET, WALL, _eye, _frame)

ROBOT = 32                      # HRL_CHASE_ROBOT: the class bit of the robot's own body
EVERYTHING = ALL | ROBOT | GROUND   # HRL_CHASE_ALL
HIT_ROBOT = 7                   # HRL_HIT_ROBOT; index: the link, in links_device.NAMES order
TILE_SHADE = 208                # HRL_CHASE_TILE_SHADE: the ground of tile parity 1, every channel * 208 >> 8
RGB_TORSO, RGB_LEG0, RGB_LEG1, RGB_LEG2 = (0, 50, 200), (120, 80, 20), (150, 100, 30), (200, 140, 40)   # HRL_RGB_TORSO, _LEG0 (hip capsules), _LEG1 (aux), _LEG2 (feet)
MIN_WIDTH, MIN_HEIGHT, MAX_SIZE = 16, 8, 256   # HRL_CHASE_MIN_WIDTH, _MIN_HEIGHT, _MAX_SIZE: multiples of 16 and of 8
MIN_DISTANCE, MAX_DISTANCE = 0.5, 50.0         # HRL_CHASE_MIN_DISTANCE, _MAX_DISTANCE

FIELDS = (('depth', torch.float32), ('seg', torch.int32), ('rgb', torch.uint8))
Chase, hrl_chase_out = _sensor.out_types('Chase', 'hrl_chase_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_CHASE_LIB') or os.path.join(_PKG, 'libhrl_chase_hip.so')
SYMBOLS = ['hrl_chase_default_spec', 'hrl_chase', 'hrl_chase_last_error']   # every symbol include/hrl_chase.h declares


class hrl_chase_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('frame', C.c_int32), ('target_mode', C.c_int32), ('target_height', C.c_float),
                ('yaw', C.c_float * 2), ('pitch', C.c_float * 2), ('distance', C.c_float), ('tan_half_h', C.c_float), ('tan_half_v', C.c_float), ('max_range', C.c_float),
                ('classes', C.c_uint32), ('tile', C.c_float)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_chase', 'the batched chase camera has', {
    'hrl_chase_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_chase_spec)],
    'hrl_chase': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_chase_spec), C.c_void_p, C.POINTER(hrl_chase_out), C.c_void_p]})


def pair(degrees):
    """(cos, sin) of an angle in degrees, taken in float64: what the spec's `yaw` and `pitch` hold."""
    return math.cos(math.radians(degrees)), math.sin(math.radians(degrees))


def default_spec(cfg, frame='heading', width=64, height=48, yaw_degrees=0.0, pitch_degrees=-30.0, distance=3.0, hfov_degrees=60.0, vfov_degrees=None, target='torso',
                 target_height=0.0, max_range=None, classes=None, tile=1.0):
    """The library's default chase camera of `cfg`'s kind (hrl_chase_default_spec: 3 m behind the torso and 30 degrees above it, 60
    degrees wide, a ground checker of 1 m, every class, max_range = the scanner's + the distance) at width x height pixels in `frame`
    ('world' or 'heading': what the yaw is counted from), `yaw_degrees` round the robot (0 = behind it, looking along forward; 180 =
    in front of it, looking back) and `pitch_degrees` within -90..90 (negative looks down; -90 = straight down).  `vfov_degrees`
    None: square pixels.  The cosines, sines and tangents are taken here in float64 and rounded once to float32: the kernel evaluates
    no trigonometric function of the spec.  `target`: 'torso' (the point looked at is the torso's centre + target_height) or 'ground'
    (ground_z + target_height under the torso).  `tile`: the side of the ground checker's squares in metres, 0 = plain ground."""
    if not -90.0 <= pitch_degrees <= 90.0:
        raise ValueError(f'pitch_degrees must be within -90..90, got {pitch_degrees!r}')
    s = hrl_chase_spec()
    check(lib().hrl_chase_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    s.width, s.height = int(width), int(height)
    s.yaw[0], s.yaw[1] = pair(yaw_degrees)
    s.pitch[0], s.pitch[1] = pair(pitch_degrees)
    th = math.tan(math.radians(hfov_degrees) / 2)
    s.tan_half_h = th
    s.tan_half_v = th * s.height / s.width if vfov_degrees is None else math.tan(math.radians(vfov_degrees) / 2)
    s.target_mode = _eye(target)
    s.target_height = target_height
    if max_range is None:
        s.max_range = s.max_range - s.distance + distance   # the library's: the scanner's range + the distance
    else:
        s.max_range = max_range
    s.distance = distance
    if classes is not None:
        s.classes = classes
    s.tile = tile
    return s


def decode(seg):
    """(kind, index, face) of a `seg` tensor, on its device: kind = HIT_* (0 = nothing, the sky; HIT_ROBOT = the robot), index = the wall,
    item, target, the ground's tile parity or the robot's link (links_device.NAMES order), face = FACE_*."""
    return seg & 255, (seg >> 8) & 255, seg >> 16


def pixel_rays(spec):
    """(u [W], s [H]) float32 tensors on the host: the u_j and s_i of include/hrl_chase.h as the library computes them, so that `depth`
    unprojects to points: E + depth[i, j] * (F + u[j] * L + s[i] * U) with eye(cfg, state, spec)'s E, F, L and U."""
    w, h = spec.width, spec.height
    one = torch.tensor(1.0, dtype=torch.float32)
    inv_w, inv_h = one / torch.tensor(float(w), dtype=torch.float32), one / torch.tensor(float(h), dtype=torch.float32)
    u = ((w - (2 * torch.arange(w) + 1)).to(torch.float32) * inv_w) * torch.tensor(spec.tan_half_h, dtype=torch.float32)
    s = ((h - (2 * torch.arange(h) + 1)).to(torch.float32) * inv_h) * torch.tensor(spec.tan_half_v, dtype=torch.float32)
    return u, s


def eye(cfg, state, spec):
    """(E, F, L, U), float64 tensors [N, 3] on the state's device: every env's eye and the camera's axes (include/hrl_chase.h), from
    `state` [N, 32] -- the optical axis F, left L, up U; E = T - distance F."""
    st = state.to(torch.float64)
    n = st.shape[0]
    f = torch.zeros(n, 2, dtype=torch.float64, device=st.device)
    f[:, 0] = 1.0
    if spec.frame == HRL_SCAN_HEADING:
        x, y, z, w = st[:, 3], st[:, 4], st[:, 5], st[:, 6]
        hx = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y + w * z)), 1)   # the ground projection of the torso's X axis
        n2 = (hx * hx).sum(1)
        good = torch.isfinite(n2) & (n2 >= 1e-12)
        f = torch.where(good[:, None], hx / torch.sqrt(torch.where(good, n2, torch.ones_like(n2)))[:, None], f)
    cy, sy, cp, sp = spec.yaw[0], spec.yaw[1], spec.pitch[0], spec.pitch[1]
    g = torch.stack((f[:, 0] * cy - f[:, 1] * sy, f[:, 1] * cy + f[:, 0] * sy), 1)
    zero = torch.zeros(n, dtype=torch.float64, device=st.device)
    F = torch.stack((cp * g[:, 0], cp * g[:, 1], zero + sp), 1)
    L = torch.stack((-g[:, 1], g[:, 0], zero), 1)
    U = torch.stack((-sp * g[:, 0], -sp * g[:, 1], zero + cp), 1)
    tz = (st[:, 2] if spec.target_mode == HRL_EYE_TORSO else zero + float(cfg.model.ground_z)) + float(spec.target_height)
    T = torch.stack((st[:, 0], st[:, 1], tz), 1)
    return T - float(spec.distance) * F, F, L, U


def shapes(spec, lead=()):
    """The shape after N of each member of Chase (with `lead` = (N,): the whole shape)."""
    grid = lead + (spec.height, spec.width)
    return (grid, grid, grid + (3,))


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    if MIN_WIDTH <= spec.width <= MAX_SIZE and MIN_HEIGHT <= spec.height <= MAX_SIZE:
        return None
    return f'spec.width must be within {MIN_WIDTH}..{MAX_SIZE} and spec.height within {MIN_HEIGHT}..{MAX_SIZE}, got {spec.width} x {spec.height}'


def sized(spec):
    """Whether tensors can be shaped after the spec."""
    return size_error(spec) is None


def chase(cfg, bufs_ref, spec, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Chase; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_chase, hrl_chase_out, FIELDS, cfg, bufs_ref, spec, (mask_ptr,), out, stream)


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.chase(): a Chase whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's
    dtype -- depth and seg [N, height, width], rgb [N, height, width, 3] -- on the env's device, no two of them the same memory; at least
    one must be given."""
    return _sensor.check_out(Chase, 'chase_device', FIELDS, shapes(spec, (n,)), out, device, distinct=True)
