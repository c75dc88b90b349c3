"""Shared by tests/test_render_host.py and tests/test_gpu_render.py: the ctypes binding of tests/render_host/librender_host.so (the host
build of csrc/render_core.h), an independent fp64 numpy reference of the picture written from include/hrl_render.h alone (world
coordinates, rotation matrices, np.sin / np.cos, signed distances), and the states the tests render.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import render_device as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, 'tests', 'render_host')
KINDS = (K.HRL_ANT_FLAT, K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN)
MODES = (R.HRL_VIEW_WORLD, R.HRL_VIEW_EGO, R.HRL_VIEW_EGO_HEADING)
SIZES = ((32, 32), (48, 32))   # width, height
# world-view half extents under which no wall, box or arena edge runs along a row or column of pixel centres at 32 or 48 pixels
WORLD_HALF = {K.HRL_ANT_FLAT: 6.1, K.HRL_ANT_GATHER: 7.7, K.HRL_ANT_MAZE: 9.3, K.HRL_POINT_GATHER: 7.7, K.HRL_ANT_MAZE_MJ: 9.3, K.HRL_ANT_FLAGRUN: 6.1}
EGO_HALF = 3.1
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'librender_host.so'])
        L = C.CDLL(os.path.join(DIR, 'librender_host.so'))
        L.render_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(R.hrl_view), C.c_void_p, C.c_void_p]
        L.render_host_last_error.restype = C.c_char_p
        L.render_host_default_view.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(R.hrl_view)]
        L.render_sizeof_view.restype = C.c_ulonglong
        L.render_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'render_check_main'])
    return os.path.join(DIR, 'render_check_main')


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def world_half(kind):
    """The half extent of the world views and grids of the tests: WORLD_HALF of a kind; of a config (tests/sensor_configs.py) its kind's
    too where the arena is the kind's default one (or there is none), else the arena's longer half side + 0.2 m."""
    if isinstance(kind, int):
        return WORLD_HALF[kind]
    ar = arena(kind)
    if ar is None or ar == DEFAULT_ARENA[kind.env_kind]:
        return WORLD_HALF[kind.env_kind]
    return round(max(ar) + 0.05 + 0.2, 3)


def view_of(kind, mode, size, half=None):
    """`kind`: an env kind, or a config whose arena need not be the kind's default one (world_half)."""
    w, h = size
    he = half if half is not None else (world_half(kind) if mode == R.HRL_VIEW_WORLD else EGO_HALF)
    return R.hrl_view(width=w, height=h, mode=mode, centre=(C.c_float * 2)(0.0, 0.0), half_extent=he)


def render_host(cfg, state, items, aux, view, mask=None, out=None, expect_ok=True):
    """The host build's picture of (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32): uint8 [N, H, W, 3]."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if out is None:
        out = np.zeros((n, view.height, view.width, 3), np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    rc = lib().render_host(C.byref(cfg), C.byref(b), C.byref(view), ptr(m), ptr(out))
    if expect_ok:
        assert rc == K.HRL_OK, lib().render_host_last_error()
        return out
    return rc, lib().render_host_last_error().decode()


# ------------------------------------------------------------------------------------------------ the fp64 reference
def _rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _axis_rot(a, th):
    a = np.asarray(a, float)
    c, s = np.cos(th), np.sin(th)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(a, a) + s * kx


_LEG = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], float)                 # assets/ant.xml:15-58: leg directions ...
_ANK = np.array([[-1, 1], [1, 1], [-1, 1], [1, 1]], float) / np.sqrt(2)      # ... and ankle axes


def ant_segments(qpos):
    """Per leg the three capsule axes (torso -> hip point, hip -> ankle, ankle -> tip) as world points."""
    p0, r0 = np.asarray(qpos[:3], float), _rot(qpos[3:7])
    out = []
    for l in range(4):
        d = np.array([_LEG[l, 0], _LEG[l, 1], 0.0])
        rx = r0 @ _axis_rot([0, 0, 1], float(qpos[7 + 2 * l]))
        rf = rx @ _axis_rot([_ANK[l, 0], _ANK[l, 1], 0], float(qpos[8 + 2 * l]))
        hip = p0 + r0 @ (0.2 * d)
        ank = hip + rx @ (0.2 * d)
        out.append((p0, hip, ank, ank + rf @ (0.4 * d)))
    return out


def _sd_segment(px, py, a, b):
    d = b - a
    dd = d @ d
    t = np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / dd, 0, 1) if dd > 0 else np.zeros_like(px)
    return np.hypot(px - (a[0] + t * d[0]), py - (a[1] + t * d[1]))


def _sd_rect(px, py, c, hx, hy):
    qx, qy = np.abs(px - c[0]) - hx, np.abs(py - c[1]) - hy
    return np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0)


def arena(cfg):
    """Half sizes of the walled arena (the planes lie 0.05 inside, the walls' inner faces), or None."""
    k = cfg.env_kind
    if k in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) or (k == K.HRL_ANT_FLAGRUN and (cfg.flag_enclosed or cfg.use_sensor)):
        return cfg.world_size[0] / 2 - 0.05, cfg.world_size[1] / 2 - 0.05
    if k in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        return 5 - 0.05, 9 - 0.05
    return None


DEFAULT_ARENA = {K.HRL_ANT_FLAT: None, K.HRL_ANT_GATHER: (15 / 2 - 0.05, 15 / 2 - 0.05), K.HRL_POINT_GATHER: (15 / 2 - 0.05, 15 / 2 - 0.05), K.HRL_ANT_MAZE: (5 - 0.05, 9 - 0.05),
                 K.HRL_ANT_MAZE_MJ: (5 - 0.05, 9 - 0.05), K.HRL_ANT_FLAGRUN: (12 / 2 - 0.05, 12 / 2 - 0.05)}   # arena() of the default config of each kind


def shapes(cfg, st, items, aux):
    """The env's layers, back to front, in world coordinates: (name, colour, signed distance function of px, py), from section 1 alone."""
    P, k, out = R.PALETTE, cfg.env_kind, []
    ar = arena(cfg)
    if ar is not None:
        out.append(('wall', P['wall'], lambda px, py, a=ar: -_sd_rect(px, py, (0.0, 0.0), a[0], a[1])))
    if k in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        out.append(('box', P['box'], lambda px, py: _sd_rect(px, py, (-2.0, 0.0), 3.0, 2.0)))
        t = int(aux[3])
        if 0 <= t < cfg.n_targets:
            c = (float(cfg.targets[t][0]), float(cfg.targets[t][1]))
            out.append(('target', P['target'], lambda px, py, c=c: np.hypot(px - c[0], py - c[1]) - 0.2))
    if k == K.HRL_ANT_FLAGRUN and items is not None:
        c = (float(items[0]), float(items[1]))
        out.append(('target', P['target'], lambda px, py, c=c: np.hypot(px - c[0], py - c[1]) - 0.2))
    if k in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) and items is not None:
        for i in range(cfg.n_food + cfg.n_poison):
            c = (float(items[2 * i]), float(items[2 * i + 1]))
            out.append(('food' if i < cfg.n_food else 'poison', P['food' if i < cfg.n_food else 'poison'], lambda px, py, c=c: _sd_rect(px, py, c, 0.125, 0.125)))
    if k == K.HRL_POINT_GATHER:
        r, p0 = _rot(st[3:7]), np.asarray(st[:3], float)
        cs = [(p0 + r @ (0.35 * np.array(s, float)))[:2] for s in ((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))]

        def quad(px, py, cs=cs):
            e = [(cs[(i + 1) % 4][0] - cs[i][0]) * (py - cs[i][1]) - (cs[(i + 1) % 4][1] - cs[i][1]) * (px - cs[i][0]) for i in range(4)]
            inside = np.all([x >= 0 for x in e], 0) | np.all([x <= 0 for x in e], 0)
            d = np.min([_sd_segment(px, py, cs[i], cs[(i + 1) % 4]) for i in range(4)], 0)
            return np.where(inside, -d, d)
        out.append(('cube', P['torso'], quad))
    else:
        for l, pts in enumerate(ant_segments(st[:15])):
            for lev in range(3):
                a, b = pts[lev][:2], pts[lev + 1][:2]
                out.append((f'leg{lev}', P[f'leg{lev}'], lambda px, py, a=a, b=b: _sd_segment(px, py, a, b) - 0.08))
        c = (float(st[0]), float(st[1]))
        out.append(('torso', P['torso'], lambda px, py, c=c: np.hypot(px - c[0], py - c[1]) - 0.25))
    return out


def frame(st, view):
    """centre, right, up of the camera (fp64)."""
    c = np.array([view.centre[0], view.centre[1]], float)
    right, up = np.array([1.0, 0.0]), np.array([0.0, 1.0])
    if view.mode != R.HRL_VIEW_WORLD:
        c = np.array([st[0], st[1]], float)
    if view.mode == R.HRL_VIEW_EGO_HEADING:
        x = _rot(st[3:7])[:2, 0]
        n2 = x @ x
        if np.isfinite(n2) and n2 >= 1e-12:
            up = x / np.sqrt(n2)
            right = np.array([up[1], -up[0]])
    return c, right, up


def reference(cfg, st, items, aux, view, band=1e-4):
    """(image [H, W, 3] uint8, near [H, W] bool): the picture of one env in fp64 and the pixels whose centre lies within `band` metres of
    the boundary of any drawn shape."""
    w, h, he = view.width, view.height, float(view.half_extent)
    c, right, up = frame(st, view)
    u = ((np.arange(w) + 0.5) * 2 / w - 1) * he
    v = (h / w - (np.arange(h) + 0.5) * 2 / w) * he
    uu, vv = np.meshgrid(u, v)
    px, py = c[0] + uu * right[0] + vv * up[0], c[1] + uu * right[1] + vv * up[1]
    img = np.empty((h, w, 3), np.uint8)
    img[:] = R.PALETTE['ground']
    near = np.zeros((h, w), bool)
    for _, col, sd in shapes(cfg, st, items, aux):
        d = sd(px, py)
        img[d <= 0] = col
        near |= np.abs(d) < band
    return img, near


# ------------------------------------------------------------------------------------------------ states
def hand_made(cfg, state):
    """Overwrites envs 0..2 of a state array [N >= 3, 32] with hand-made poses: a torso tilted 40 degrees about a horizontal axis, every
    joint at a stop, a yaw of 30 degrees (the point bot: tilted, yawed 30 degrees, both)."""
    s = state.copy()
    tilt, yaw = np.deg2rad(40.0), np.deg2rad(30.0)
    ax = np.array([np.cos(0.7), np.sin(0.7), 0.0])
    s[0, 3:7] = np.r_[np.sin(tilt / 2) * ax, np.cos(tilt / 2)]
    s[2, 3:7] = (0, 0, np.sin(yaw / 2), np.cos(yaw / 2))
    if cfg.env_kind != K.HRL_POINT_GATHER:
        lo = np.deg2rad([-40, 30, -40, -100, -40, -100, -40, 30])
        hi = np.deg2rad([40, 100, 40, -30, 40, -30, 40, 100])
        s[1, 7:15] = np.where(np.arange(8) % 3 == 0, lo, hi)
    else:
        q1 = np.r_[np.sin(tilt / 2) * ax, np.cos(tilt / 2)]
        q2 = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
        x1, y1, z1, w1 = q2
        x2, y2, z2, w2 = q1   # yaw after tilt: q2 * q1
        s[1, 3:7] = (w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2)
    return s.astype(np.float32)


def yawed(state, items, cfg, angle):
    """The whole state turned by `angle` about the world z axis through the origin (pose only: the renderer reads nothing else)."""
    s = state.astype(np.float64).copy()
    c, sn = np.cos(angle), np.sin(angle)
    s[:, 0], s[:, 1] = c * state[:, 0] - sn * state[:, 1], sn * state[:, 0] + c * state[:, 1]
    x1, y1, z1, w1 = 0.0, 0.0, np.sin(angle / 2), np.cos(angle / 2)
    x2, y2, z2, w2 = (state[:, 3 + i].astype(np.float64) for i in range(4))
    s[:, 3] = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    s[:, 4] = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2
    s[:, 5] = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2
    s[:, 6] = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    return s.astype(np.float32)


def hostile(cfg, state, items, aux):
    """Hostile copies of a shard of >= 5 envs and, per env, what the picture must equal: a list of (state, items, aux, cleaned state,
    cleaned items, cleaned aux, far) where the cleaned record has the offending shape moved out of every view (an item at (100, 0) as an
    eaten one is; a robot far away); far: render the cleaned record with far_targets(cfg) -- an out-of-range target index names none."""
    out = []
    for bad in (np.nan, np.inf, -np.inf, 1e20):
        s, it, a = state.copy(), None if items is None else items.copy(), aux.copy()
        cs, cit, ca = state.copy(), None if items is None else items.copy(), aux.copy()
        s[0, 0] = bad; cs[0, 0] = 1e6          # the robot's x: no robot layers
        s[1, 1] = bad; cs[1, 1] = 1e6
        if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
            it[2, 0] = bad; cit[2, 0:2] = (100.0, 0.0)      # item 0 of env 2 is absent
            it[3, 2 * cfg.n_food + 1] = bad; cit[3, 2 * cfg.n_food:2 * cfg.n_food + 2] = (100.0, 0.0)   # its first poison item
        if cfg.env_kind == K.HRL_ANT_FLAGRUN:
            it[2, 1] = bad; cit[2, 0:2] = (1e6, 1e6)
        out.append((s, it, a, cs, cit, ca, False))
    # denormals are ordinary numbers: the picture equals that of zeros in their place to the last byte only if nothing is near -- not
    # claimed; out-of-range target indices name no target
    s, it, a = state.copy(), None if items is None else items.copy(), aux.copy()
    a[:, 3] = (1000, -5, 2 ** 31 - 1, -2 ** 31, 64)[:len(a)] if cfg.env_kind != K.HRL_ANT_FLAGRUN else a[:, 3]
    ca = a.copy()
    ca[:, 3] = 0 if cfg.env_kind != K.HRL_ANT_FLAGRUN else ca[:, 3]
    out.append((s, it, a, s.copy(), None if it is None else it.copy(), ca, True))
    return out


def far_targets(cfg):
    """A copy of cfg whose maze targets all lie outside every view: the picture of `no target`."""
    c = cfg.copy()
    for i in range(K.HRL_MAX_TARGETS):
        c.targets[i][0], c.targets[i][1] = 1e6, 1e6
    return c
