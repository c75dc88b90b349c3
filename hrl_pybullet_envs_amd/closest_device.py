"""The batched closest points (include/hrl_closest.h): loader of libhrl_closest_hip.so, the ctypes mirrors of `hrl_closest_spec` and
`hrl_closest_out`, and the launch behind `BatchedEnv.closest()` -- for every env of a shard, every link of the robot (links_device.NAMES
order: B = 13 for the ants, 1 for the point bot) against its nearest surface in each of six classes (CLASS_NAMES: ground, wall, box, food,
poison, self): `distance` float32 [N, B, 6] (the signed gap, negative = penetration, +inf where there is nothing), `which` int32 [N, B, 6]
(the scanner's word: which plane, which item, which other link), `on_link`, `on_surface` and `normal` float32 [N, B, 6, 3] (world
coordinates; the normal points from the surface to the link), in HBM, from one kernel launch -- the simulator's getClosestPoints for all
envs at once.  The surfaces are what the step collides with: a pair the step holds in contact reports the step's own distance.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor
from .chase_device import BOX, FOOD, GROUND, HIT_BOX, HIT_FOOD, HIT_GROUND, HIT_NONE, HIT_POISON, HIT_ROBOT, HIT_WALL, POISON, ROBOT, TARGET, WALL  # noqa: F401  (the class bits and the hit codes)
from .links_device import n_links
from .scan_device import decode  # noqa: F401  ((class code, index) of `which`)

GROUND_CLASS, WALL_CLASS, BOX_CLASS, FOOD_CLASS, POISON_CLASS, SELF_CLASS = range(6)   # HRL_CLOSEST_GROUND ... HRL_CLOSEST_SELF: the class axis
CLASS_NAMES = ('ground', 'wall', 'box', 'food', 'poison', 'self')
CLASSES = len(CLASS_NAMES)                                # HRL_CLOSEST_CLASSES
EVERYTHING = WALL | BOX | FOOD | POISON | ROBOT | GROUND  # HRL_CLOSEST_ALL: every class bit but the target's
CLASS_BITS = (GROUND, WALL, BOX, FOOD, POISON, ROBOT)     # the bit of spec.classes that asks for each class of the axis
CLASS_HITS = (HIT_GROUND, HIT_WALL, HIT_BOX, HIT_FOOD, HIT_POISON, HIT_ROBOT)   # the low byte of `which` in each class of the axis

FIELDS = (('distance', torch.float32), ('which', torch.int32), ('on_link', torch.float32), ('on_surface', torch.float32), ('normal', torch.float32))
Closest, hrl_closest_out = _sensor.out_types('Closest', 'hrl_closest_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_CLOSEST_LIB') or os.path.join(_PKG, 'libhrl_closest_hip.so')
SYMBOLS = ['hrl_closest_default_spec', 'hrl_closest', 'hrl_closest_last_error']   # every symbol include/hrl_closest.h declares


class hrl_closest_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('classes', C.c_uint32), ('reserved', C.c_uint32)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_closest', 'the batched closest points have', {
    'hrl_closest_default_spec': [C.POINTER(K.hrl_config), C.POINTER(hrl_closest_spec)],
    'hrl_closest': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_closest_spec), C.c_void_p, C.POINTER(hrl_closest_out), C.c_void_p]})


def default_spec(cfg, classes=EVERYTHING):
    """The library's default spec of `cfg`'s kind (hrl_closest_default_spec: every class) with `classes`, a non-empty mask of WALL, BOX,
    FOOD, POISON, ROBOT (the self class) and GROUND: a class that is not asked for reports +inf / HIT_NONE."""
    s = hrl_closest_spec()
    check(lib().hrl_closest_default_spec(C.byref(cfg), C.byref(s)))
    s.classes = classes
    return s


def shapes(cfg, spec=None, lead=()):
    """The shape after N of each member of Closest (with `lead` = (N,): the whole shape)."""
    cell = lead + (n_links(cfg), CLASSES)
    return (cell, cell, cell + (3,), cell + (3,), cell + (3,))


def size_error(spec):
    """Why no tensors can be shaped after the spec, or None: every spec has the one shape."""
    return None


def sized(spec):
    """Whether tensors can be shaped after the spec."""
    return size_error(spec) is None


def closest(cfg, bufs_ref, spec, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Closest; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_closest, hrl_closest_out, FIELDS, cfg, bufs_ref, spec, (mask_ptr,), out, stream)


def check_out(out, n, cfg, spec, device):
    """`out=` of BatchedEnv.closest(): a Closest whose members are None (skipped) or contiguous, 4-byte aligned tensors of the member's
    dtype -- distance and which [N, B, 6], on_link, on_surface and normal [N, B, 6, 3] -- on the env's device, no two of them the same
    memory; at least one must be given."""
    return _sensor.check_out(Closest, 'closest_device', FIELDS, shapes(cfg, spec, (n,)), out, device, distinct=True)


def within(closest_of_env, distance, link=None):
    """The cells of ONE env (a Closest of arrays or tensors [B, 6, ...]) whose distance is at most `distance` metres, as tuples (link,
    class code, index, distance, on_link (x, y, z), on_surface (x, y, z), normal (x, y, z)) in cell order -- class code and index as
    decode(which) gives them (HIT_GROUND, HIT_WALL with the plane, HIT_BOX, HIT_FOOD / HIT_POISON with the item, HIT_ROBOT with the
    other link).  `link`: only that link's cells."""
    d, w, a, b, nrm = (x.tolist() for x in closest_of_env)
    out = []
    for l, row in enumerate(d):
        if link is not None and l != link:
            continue
        for k, dist in enumerate(row):
            if w[l][k] != HIT_NONE and dist <= distance:
                out.append((l, w[l][k] & 0xFF, w[l][k] >> 8, dist, tuple(a[l][k]), tuple(b[l][k]), tuple(nrm[l][k])))
    return out
