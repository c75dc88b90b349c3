"""The batched ray test (include/hrl_cast.h): loader of libhrl_cast_hip.so, the ctypes mirrors of `hrl_cast_spec` and `hrl_cast_out`, and
the launch behind `BatchedEnv.cast()` -- for every env of a shard R rays of the caller's, each a 3-D segment from `from` to `to` in the
world, about the torso, in the heading's frame or in a link's body frame, against the scene and the robot's own body: `fraction` float32
[N, R] (1.0 where nothing was met), `seg` int32 [N, R] (the chase camera's word: which shape or which link, and which face), `point` and
`normal` float32 [N, R, 3] (world coordinates and axes), in HBM, from one kernel launch -- the simulator's rayTestBatch(from, to) for all
envs at once.  With it come the ray patterns users build sensors from: a 3-D lidar (`lidar_rays`), a range finder at each foot tip
(`down_rays`), rays from origins, directions and lengths (`from_to`).

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import math
import os

import torch

from . import _capi as K
from . import _sensor
from .chase_device import (ALL, BOX, EVERYTHING, FACE_BOTTOM, FACE_GROUND, FACE_INSIDE, FACE_ROUND, FACE_SIDE_X, FACE_SIDE_Y, FACE_TOP, FACES, FOOD, GROUND, HIT_BOX,  # noqa: F401  (the chase camera's class bits, hit codes and faces, and its decode)
                           HIT_FOOD, HIT_GROUND, HIT_NONE, HIT_POISON, HIT_ROBOT, HIT_TARGET, HIT_WALL, POISON, ROBOT, TARGET, WALL, decode)

HRL_CAST_WORLD, HRL_CAST_EGO, HRL_CAST_HEADING, HRL_CAST_LINK = 0, 1, 2, 3
FRAMES = {'world': HRL_CAST_WORLD, 'ego': HRL_CAST_EGO, 'heading': HRL_CAST_HEADING, 'link': HRL_CAST_LINK}
MAX_RAYS = 1024            # HRL_CAST_MAX_RAYS
FOOT_LINKS = (2, 4, 6, 8)  # HRL_LINK_FOOT(l) of the four legs, in links_device.NAMES order
FOOT_TIP = ((0.4, 0.4), (-0.4, 0.4), (-0.4, -0.4), (0.4, -0.4))   # the foot capsules' far ends in their links' body frames (hrl_links_default_spec's sites)

FIELDS = (('fraction', torch.float32), ('seg', torch.int32), ('point', torch.float32), ('normal', torch.float32))
Cast, hrl_cast_out = _sensor.out_types('Cast', 'hrl_cast_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_CAST_LIB') or os.path.join(_PKG, 'libhrl_cast_hip.so')
SYMBOLS = ['hrl_cast_default_spec', 'hrl_cast', 'hrl_cast_last_error']   # every symbol include/hrl_cast.h declares


class hrl_cast_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('n_rays', C.c_int32), ('frame', C.c_int32), ('classes', C.c_uint32), ('reserved', C.c_uint32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_cast', 'the batched ray test has', {
    'hrl_cast_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_cast_spec)],
    'hrl_cast': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_cast_spec), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(hrl_cast_out), C.c_void_p]})


def _frame(frame):
    if frame not in FRAMES:
        raise ValueError(f'frame must be one of {sorted(FRAMES)}, got {frame!r}')
    return FRAMES[frame]


def default_spec(cfg, frame='heading', n_rays=64, classes=EVERYTHING):
    """The library's default spec of `cfg`'s kind (hrl_cast_default_spec: every class) for `n_rays` rays per env (1..1024) whose
    coordinates are in `frame`: 'world' (world positions), 'ego' (offsets from the torso's origin in world axes), 'heading' (offsets
    turned by the heading: x forward, y left, z up) or 'link' (the body frame of the ray's link: `ray_link` of cast())."""
    s = hrl_cast_spec()
    check(lib().hrl_cast_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    s.n_rays = int(n_rays)
    s.classes = classes
    return s


def from_to(origin, direction, length):
    """Rays [..., 6] float32 from origins [..., 3], directions [..., 3] (of any positive length: they are normalised here) and a length
    in metres (a number or a tensor [...]): from = origin, to = origin + length * direction / |direction|."""
    o = torch.as_tensor(origin, dtype=torch.float32)
    d = torch.as_tensor(direction, dtype=torch.float32).to(o.device)
    o, d = torch.broadcast_tensors(o, d)
    d = d / torch.linalg.vector_norm(d, dim=-1, keepdim=True)
    n = torch.as_tensor(length, dtype=torch.float32, device=o.device)
    return torch.cat((o, o + (n[..., None] if n.dim() else n) * d), -1).contiguous()


def lidar_rays(n_azimuth, elevations_degrees, max_range, min_range=0.0):
    """A 3-D lidar pattern [R, 6] float32 on the host, R = len(elevations_degrees) * n_azimuth, ring by ring: ray e * n_azimuth + a
    looks along (cos el cos az, cos el sin az, sin el) with az = 2 pi a / n_azimuth (counter-clockwise from +x, which is forward in
    the 'heading' and 'link' frames) and el = elevations_degrees[e] (negative looks down), from min_range to max_range metres from the
    frame's origin.  `fraction` * (max_range - min_range) + min_range is the measured range."""
    if not 0.0 <= min_range < max_range:
        raise ValueError(f'0 <= min_range < max_range is required, got {min_range!r}, {max_range!r}')
    az = torch.arange(int(n_azimuth), dtype=torch.float64) * (2.0 * math.pi / int(n_azimuth))
    el = torch.deg2rad(torch.as_tensor(list(elevations_degrees), dtype=torch.float64))
    d = torch.stack((torch.cos(el)[:, None] * torch.cos(az)[None], torch.cos(el)[:, None] * torch.sin(az)[None], torch.sin(el)[:, None].expand(-1, az.numel())), -1).reshape(-1, 3)
    return torch.cat((min_range * d, max_range * d), -1).to(torch.float32).contiguous()


def down_rays(length):
    """(rays [4, 6] float32, ray_link [4] int32) on the host for frame 'link': a range finder at each foot tip, from the tip `length`
    metres on along the foot capsule's axis (the way the foot points: down to the ground for a standing ant's bent ankles), in the
    foot links' body frames.  The ray starts inside the foot's own end ball, which it therefore does not see."""
    rays = torch.tensor([[x, y, 0.0, x + length * math.copysign(math.sqrt(0.5), x), y + length * math.copysign(math.sqrt(0.5), y), 0.0] for x, y in FOOT_TIP], dtype=torch.float32)
    return rays, torch.tensor(FOOT_LINKS, dtype=torch.int32)


def expand(rays, n, device=None):
    """A pattern [R, 6] as the contiguous [n, R, 6] tensor cast() reads, on `device`: the kernel reads every env's own rays, so the
    broadcast has to be materialised -- do it ONCE, outside the loop, and hand the result to every call."""
    r = torch.as_tensor(rays, dtype=torch.float32)
    if r.dim() != 2 or r.shape[1] != 6:
        raise ValueError(f'a ray pattern must be [R, 6], got {tuple(r.shape)}')
    return r.to(device=device if device is not None else r.device).expand(int(n), *r.shape).contiguous()


def shapes(spec, lead=()):
    """The shape after N of each member of Cast (with `lead` = (N,): the whole shape)."""
    r = (spec.n_rays,)
    return (lead + r, lead + r, lead + r + (3,), lead + r + (3,))


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    return None if 1 <= spec.n_rays <= MAX_RAYS else f'spec.n_rays must be within 1..{MAX_RAYS}, got {spec.n_rays}'


def sized(spec):
    """Whether tensors can be shaped after the spec."""
    return size_error(spec) is None


def check_rays(rays, n, spec, device):
    """`rays` of BatchedEnv.cast(): a contiguous, 8-byte aligned float32 tensor [N, n_rays, 6] on the env's device."""
    return _sensor.check_tensors((rays,), '', (('rays', torch.float32),), ((n, spec.n_rays, 6),), device, 8)[0]


def check_ray_link(ray_link, spec, device):
    """`ray_link` of BatchedEnv.cast(): a contiguous, 4-byte aligned int32 tensor [n_rays] on the env's device."""
    return _sensor.check_tensors((ray_link,), '', (('ray_link', torch.int32),), ((spec.n_rays,),), device, 4)[0]


def cast(cfg, bufs_ref, spec, rays_ptr, ray_link_ptr, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Cast; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref` and the rays at `rays_ptr`."""
    return _sensor.launch(check, lib().hrl_cast, hrl_cast_out, FIELDS, cfg, bufs_ref, spec, (rays_ptr, ray_link_ptr, mask_ptr), out, stream)


def check_out(out, n, spec, device, rays=None):
    """`out=` of BatchedEnv.cast(): a Cast whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's dtype
    -- fraction and seg [N, n_rays], point and normal [N, n_rays, 3] -- on the env's device, no two of them the same memory, none of
    them `rays`'; at least one must be given."""
    _sensor.check_out(Cast, 'cast_device', FIELDS, shapes(spec, (n,)), out, device, distinct=True)
    if rays is not None:
        for (name, _), t in zip(FIELDS, out):
            if t is not None and t.numel() and t.data_ptr() == rays.data_ptr():
                raise ValueError(f'out.{name} and rays must not be the same memory')
    return out
