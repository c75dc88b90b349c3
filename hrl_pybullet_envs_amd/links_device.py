"""The batched link states (include/hrl_links.h): loader of libhrl_links_hip.so, the ctypes mirrors of `hrl_links_spec` and
`hrl_links_out`, and the launch behind `BatchedEnv.links()` -- for every env of a shard the pose and the velocity of every rigid body of
the robot (13 for the ants, 1 for the point bot) and of caller-defined points fixed to those bodies: `origin`, `com`, `lin_vel`, `ang_vel`
float32 [N, B, 3], `quat` float32 [N, B, 4] (x, y, z, w), `site_pos`, `site_vel` float32 [N, S, 3], in HBM, from one kernel launch.  What
the reference reads one env at a time through `robot.parts[name]` and the simulator's getLinkState.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor

HRL_LINKS_WORLD, HRL_LINKS_HEADING = 0, 1
FRAMES = {'world': HRL_LINKS_WORLD, 'heading': HRL_LINKS_HEADING}
LINKS_ANT, LINKS_POINT, MAX_SITES = 13, 1, 16   # HRL_LINKS_ANT, HRL_LINKS_POINT, HRL_LINKS_MAX_SITES
TORSO = 0
AUX = (1, 3, 5, 7)      # HRL_LINK_AUX(l)
FEET = (2, 4, 6, 8)     # HRL_LINK_FOOT(l): upstream's foot_list order
HIPS = (9, 10, 11, 12)  # HRL_LINK_HIP(l)
FOOT_LIST = ('front_left_foot', 'front_right_foot', 'left_back_foot', 'right_back_foot')   # upstream Ant.foot_list

FIELDS = tuple((name, torch.float32) for name in ('origin', 'com', 'quat', 'lin_vel', 'ang_vel', 'site_pos', 'site_vel'))
Links, hrl_links_out = _sensor.out_types('Links', 'hrl_links_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_LINKS_LIB') or os.path.join(_PKG, 'libhrl_links_hip.so')
SYMBOLS = ['hrl_links_count', 'hrl_links_name', 'hrl_links_default_spec', 'hrl_links', 'hrl_links_last_error']   # every symbol include/hrl_links.h declares


class hrl_links_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('frame', C.c_int32), ('n_sites', C.c_int32), ('site_link', C.c_int32 * MAX_SITES), ('site_local', (C.c_float * 3) * MAX_SITES)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_links', 'the batched link states have', {
    'hrl_links_count': [C.c_int32],
    'hrl_links_name': [C.c_int32, C.c_int32],
    'hrl_links_default_spec': [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(hrl_links_spec)],
    'hrl_links': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_links_spec), C.c_void_p, C.POINTER(hrl_links_out), C.c_void_p]})


def _frame(frame):
    if frame not in FRAMES:
        raise ValueError(f'frame must be one of {sorted(FRAMES)}, got {frame!r}')
    return FRAMES[frame]


def n_links(kind):
    """B: 13 for the ant kinds, 1 for the point bot (`kind`: an HRL_* env kind or an hrl_config)."""
    return LINKS_POINT if getattr(kind, 'env_kind', kind) == K.HRL_POINT_GATHER else LINKS_ANT


def NAMES(kind):
    """The names of the links of a kind in index order, as assets/ant.xml spells them (hrl_links_name); ('cube',) for the point bot."""
    kind = getattr(kind, 'env_kind', kind)
    L = lib()
    L.hrl_links_name.restype = C.c_char_p
    return tuple(L.hrl_links_name(kind, i).decode() for i in range(L.hrl_links_count(kind)))


def default_spec(cfg, frame='world', sites=None):
    """The library's default spec of `cfg`'s kind in `frame` ('world' or 'heading'): the four foot tips as sites (the cube's centre for the
    point bot).  `sites`: a sequence of up to 16 (link, (x, y, z)) pairs -- a point fixed to a link, in the link's frame -- instead; () for
    none."""
    s = hrl_links_spec()
    check(lib().hrl_links_default_spec(C.byref(cfg), _frame(frame), C.byref(s)))
    if sites is not None:
        sites = list(sites)
        if len(sites) > MAX_SITES:
            raise ValueError(f'at most {MAX_SITES} sites, got {len(sites)}')
        s.n_sites = len(sites)
        for i in range(MAX_SITES):
            link, local = sites[i] if i < len(sites) else (0, (0.0, 0.0, 0.0))
            s.site_link[i] = int(link)
            s.site_local[i][0], s.site_local[i][1], s.site_local[i][2] = (float(v) for v in local)
    return s


def tip(links):
    """The far end of every link's capsule, 2 com - origin (the torso's and the cube's: their centre); tensors or arrays."""
    return 2 * links.com - links.origin


def shapes(cfg, spec, lead=()):
    """The shape after N of each member of Links (with `lead` = (N,): the whole shape)."""
    link, site = lead + (n_links(cfg), 3), lead + (spec.n_sites, 3)
    return (link, link, link[:-1] + (4,), link, link, site, site)


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    return None if 0 <= spec.n_sites <= MAX_SITES else f'spec.n_sites must be within 0..{MAX_SITES}, got {spec.n_sites}'


def sized(spec):
    """Whether tensors can be shaped after the spec."""
    return size_error(spec) is None


def links(cfg, bufs_ref, spec, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Links; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_links, hrl_links_out, FIELDS, cfg, bufs_ref, spec, (mask_ptr,), out, stream)


def check_out(out, n, cfg, spec, device):
    """`out=` of BatchedEnv.links(): a Links whose members are None (skipped) or contiguous, 4-byte aligned float32 tensors -- origin, com,
    lin_vel, ang_vel [N, B, 3], quat [N, B, 4], site_pos, site_vel [N, n_sites, 3] -- on the env's device, no two of them the same memory;
    at least one must be given."""
    return _sensor.check_out(Links, 'links_device', FIELDS, shapes(cfg, spec, (n,)), out, device, distinct=True)
