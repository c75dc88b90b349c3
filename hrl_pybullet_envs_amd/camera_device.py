"""The batched first-person camera (include/hrl_camera.h): loader of libhrl_camera_hip.so, the ctypes mirrors of `hrl_camera_spec` and
`hrl_camera_out`, and the launch behind `BatchedEnv.camera()` -- for every env of a shard a pinhole image as the robot sees it: `depth`
float32 [N, H, W] (metres along the optical axis), `seg` int32 [N, H, W] (which shape and which of its faces) and `rgb` uint8 [N, H, W, 3],
in HBM, from one kernel launch.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import math
import os

import torch

from . import _capi as K
from . import _sensor
from .scan_device import (ALL, BOX, FOOD, FRAMES, HIT_BOX, HIT_FOOD, HIT_NONE, HIT_POISON, HIT_TARGET, HIT_WALL, HRL_SCAN_HEADING,  # noqa: F401  (the scanner's frames, class bits and hit codes)
                          HRL_SCAN_WORLD, POISON, TARGET, WALL, _frame)

GROUND = 64         # HRL_CAMERA_GROUND: a class bit next to the scanner's
EVERYTHING = ALL | GROUND
HIT_GROUND = 6      # HRL_HIT_GROUND
FACE_INSIDE, FACE_SIDE_X, FACE_SIDE_Y, FACE_ROUND, FACE_TOP, FACE_BOTTOM, FACE_GROUND = range(7)   # HRL_FACE_*: seg >> 16
FACES = ('inside', 'side_x', 'side_y', 'round', 'top', 'bottom', 'ground')
SHADES = (128, 224, 176, 200, 256, 96, 256)   # rgb = the class colour * SHADES[face] >> 8
HRL_EYE_GROUND, HRL_EYE_TORSO = 0, 1
EYES = {'ground': HRL_EYE_GROUND, 'torso': HRL_EYE_TORSO}
RGB_SKY = (150, 200, 255)   # HRL_RGB_SKY
MIN_WIDTH, MIN_HEIGHT, MAX_SIZE = 16, 8, 128   # HRL_CAMERA_MIN_WIDTH, _MIN_HEIGHT, _MAX_SIZE: multiples of 16 and of 8

FIELDS = (('depth', torch.float32), ('seg', torch.int32), ('rgb', torch.uint8))
Camera, hrl_camera_out = _sensor.out_types('Camera', 'hrl_camera_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_CAMERA_LIB') or os.path.join(_PKG, 'libhrl_camera_hip.so')
SYMBOLS = ['hrl_camera_default_spec', 'hrl_camera', 'hrl_camera_last_error']   # every symbol include/hrl_camera.h declares


class hrl_camera_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('width', C.c_int32), ('height', C.c_int32), ('frame', C.c_int32), ('eye_mode', C.c_int32), ('eye_height', C.c_float),
                ('tan_half_h', C.c_float), ('tan_half_v', C.c_float), ('max_range', C.c_float), ('classes', C.c_uint32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_camera', 'the batched first-person camera has', {
    'hrl_camera_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_camera_spec)],
    'hrl_camera': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_camera_spec), C.c_void_p, C.POINTER(hrl_camera_out), C.c_void_p]})


def _eye(eye):
    if eye not in EYES:
        raise ValueError(f'eye must be one of {sorted(EYES)}, got {eye!r}')
    return EYES[eye]


def default_spec(cfg, frame='heading', width=64, height=48, hfov_degrees=90, vfov_degrees=None, eye='torso', eye_height=None, max_range=None, classes=None):
    """The library's default camera of `cfg`'s kind (hrl_camera_default_spec: the torso's eye 0.3 m above its centre, 0.4 m for the point
    bot; every class and the ground; max_range = the scanner's, the arena's diagonal) at width x height pixels in `frame` ('world' or
    'heading'), with a horizontal field of view of `hfov_degrees` and a vertical one of `vfov_degrees` (None: square pixels, tan_half_v =
    tan_half_h * height / width).  The tangents are taken here in float64 and rounded once to float32: the kernel evaluates no
    trigonometric function.  `eye`: 'torso' (the torso's z + eye_height) or 'ground' (ground_z + eye_height)."""
    s = hrl_camera_spec()
    check(lib().hrl_camera_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    s.width, s.height = int(width), int(height)
    th = math.tan(math.radians(hfov_degrees) / 2)
    s.tan_half_h = th
    s.tan_half_v = th * s.height / s.width if vfov_degrees is None else math.tan(math.radians(vfov_degrees) / 2)
    s.eye_mode = _eye(eye)
    if eye_height is not None:
        s.eye_height = eye_height
    if max_range is not None:
        s.max_range = max_range
    if classes is not None:
        s.classes = classes
    return s


def decode(seg):
    """(kind, index, face) of a `seg` tensor, on its device: kind = HIT_* (0 = nothing, the sky), index = the wall, item or target, face =
    FACE_*."""
    return seg & 255, (seg >> 8) & 255, seg >> 16


def pixel_rays(spec):
    """(u [W], s [H]) float32 tensors on the host: the u_j and s_i of include/hrl_camera.h as the library computes them, so that `depth`
    unprojects to points: eye + depth[i, j] * (forward + u[j] * left + s[i] * up), left = (-forward_y, forward_x, 0), up = world +z."""
    w, h = spec.width, spec.height
    inv_w, inv_h = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(w), dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(h), dtype=torch.float32)
    u = ((w - (2 * torch.arange(w) + 1)).to(torch.float32) * inv_w) * torch.tensor(spec.tan_half_h, dtype=torch.float32)
    s = ((h - (2 * torch.arange(h) + 1)).to(torch.float32) * inv_h) * torch.tensor(spec.tan_half_v, dtype=torch.float32)
    return u, s


def shapes(spec, lead=()):
    """The shape after N of each member of Camera (with `lead` = (N,): the whole shape)."""
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


def camera(cfg, bufs_ref, spec, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Camera; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_camera, hrl_camera_out, FIELDS, cfg, bufs_ref, spec, (mask_ptr,), out, stream)


def check_out(out, n, spec, device):
    """`out=` of BatchedEnv.camera(): a Camera whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's
    dtype -- depth and seg [N, height, width], rgb [N, height, width, 3] -- on the env's device, no two of them the same memory; at least
    one must be given."""
    return _sensor.check_out(Camera, 'camera_device', FIELDS, shapes(spec, (n,)), out, device, distinct=True)
