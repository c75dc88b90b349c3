"""Shared by tests/test_see_host.py and tests/test_gpu_see.py: the ctypes binding of tests/see_host/libsee_host.so (the host build of
csrc/see_core.h), an independent fp64 numpy reference written from include/hrl_see.h alone (world coordinates, the ray tests of the
shapes tables of probe_cases / scan_cases), and the specs the tests compute maps of.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import field_cases as fc
import probe_cases as pc
import render_cases as rc
import scan_cases as sc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import see_device as V

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'see_host')
KINDS = rc.KINDS
MODES = rc.MODES
SIZES = ((8, 8), (24, 40), (64, 8), (64, 64))   # width, height: one wave of cells | 960, no multiple of 256 | an edge shape | the maximum
NAMES = tuple(n for n, _ in V.FIELDS)
DTYPES = (np.uint8, np.uint8, np.int32)
See = collections.namedtuple('See', NAMES)   # of numpy arrays
HUGE = 3.0e38
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libsee_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libsee_host.so'))
        L.see_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(V.hrl_see_spec), C.c_void_p, C.c_void_p, C.POINTER(V.hrl_see_out), C.c_void_p]
        L.see_host_last_error.restype = C.c_char_p
        L.see_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(V.hrl_see_spec)]
        L.see_sizeof_spec.restype = C.c_ulonglong
        L.see_sizeof_out.restype = C.c_ulonglong
        L.see_validate_spec.argtypes, L.see_validate_spec.restype = [C.POINTER(V.hrl_see_spec)], C.c_char_p
        L.see_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        L.see_merge4.argtypes, L.see_merge4.restype = [C.c_uint, C.c_uint, C.POINTER(C.c_int)], C.c_uint
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'see_check_main'])
    return os.path.join(DIR, 'see_check_main')


ptr = rc.ptr


def spec_of(size, mode, occluders=V.WALL | V.BOX, fov_cos=-1.0, max_range=HUGE, slack=0.0, half=None, centre=(0.0, 0.0), kind=None):
    """slack = None: one cell of the grid (see_device.one_cell: at most the 2 m the header allows)."""
    w, h = size
    he = half if half is not None else (rc.world_half(kind) if mode == V.HRL_VIEW_WORLD else fc.EGO_HALF)   # kind: an env kind or a config
    s = V.hrl_see_spec(width=w, height=h, mode=mode, centre=(C.c_float * 2)(*centre), half_extent=he, occluders=occluders, max_range=max_range, fov_cos=fov_cos, slack=0.0)
    s.slack = V.one_cell(s) if slack is None else slack
    return s


def sweep_specs(size, mode, kind):
    """The three specs of the sweeps: everything occludes, all round, any range, a slack of one cell | walls and the box, a field of view
    of 120 degrees, 6 m, no slack | nothing occludes, the half plane ahead, 3 m."""
    kw = dict(kind=kind, centre=fc.WORLD_CENTRE)
    return (spec_of(size, mode, V.ALL, -1.0, HUGE, None, **kw), spec_of(size, mode, V.WALL | V.BOX, 0.5, 6.0, 0.0, **kw), spec_of(size, mode, 0, 0.0, 3.0, 0.0, **kw))


def shapes_of(n, spec):
    h, w = min(max(spec.height, 1), 64), min(max(spec.width, 1), 64)
    return ((n, h, w), (n, h, w), (n,))


def see_host(cfg, state, items, aux, spec, clear=None, mask=None, out=None, want=('visible',), centres=None, expect_ok=True):
    """The host build's map of (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32): a See of arrays; the members not in
    `want` are None.  `out`: a See of arrays (None members are passed as NULL); `seen` is read and written in place.  `centres`: a
    float32 [N, H, W, 2] array that receives the cell centres in the table's frame."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if out is None:
        out = See(*(np.zeros(shape, dt) if name in want else None for name, dt, shape in zip(NAMES, DTYPES, shapes_of(n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    c = None if clear is None else np.ascontiguousarray(clear, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = V.hrl_see_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().see_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(c), ptr(m), C.byref(o), ptr(centres))
    if expect_ok:
        assert code == K.HRL_OK, lib().see_host_last_error()
        return out
    return code, lib().see_host_last_error().decode()


def same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the fp64 reference
SHIFTS = pc.SHIFTS   # +-1e-4 m along x and y: the probe suite's convention and its ceiling


def first_meeting(typ, p, o, dx, dy):
    """The ray parameter t >= 0 at which the rays o + t (dx, dy) (unit directions, arrays) first meet the shape: 0 when o lies in it (for
    a plane: outside the arena), +inf when they miss it."""
    with np.errstate(divide='ignore', invalid='ignore'):
        if typ == 'half':
            (nx, ny), off0 = p
            off, den = nx * o[0] + ny * o[1] + off0, nx * dx + ny * dy
            return np.zeros_like(dx) if off < 0 else np.where(den < 0, off / -np.where(den < 0, den, -1.0), np.inf)
        if typ == 'rect':
            (cx, cy), (hx, hy) = p
            x0, x1 = sc._slab(cx - hx, cx + hx, o[0], dx)
            y0, y1 = sc._slab(cy - hy, cy + hy, o[1], dy)
            tn, tf = np.maximum(x0, y0), np.minimum(x1, y1)
            return np.where((tn <= tf) & (tf >= 0), np.maximum(tn, 0.0), np.inf)
        (cx, cy), r = p
        ex, ey = cx - o[0], cy - o[1]
        b, cc = ex * dx + ey * dy, ex * ex + ey * ey
        h = b * b - cc + r * r
        return np.zeros_like(dx) if cc <= r * r else np.where((h >= 0) & (b > 0), b - np.sqrt(np.maximum(h, 0.0)), np.inf)


def reference(cfg, st, items, aux, spec, shift=(0.0, 0.0)):
    """visible [H, W] bool of one env in fp64, with every cell centre moved by `shift` in world coordinates."""
    h, w = spec.height, spec.width
    o = np.array([st[0], st[1]], float)
    if not np.isfinite(o).all():
        return np.zeros((h, w), bool)
    pos = fc.centres(st, spec)[0] + np.asarray(shift, float)
    q = pos.reshape(-1, 2) - o
    L = np.hypot(q[:, 0], q[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        dx, dy = q[:, 0] / L, q[:, 1] / L
    fwd = sc.forward(st, sc.S.HRL_SCAN_HEADING)
    vis = np.isfinite(q).all(1) & (L <= float(spec.max_range))
    if float(spec.fov_cos) > -1.0:
        with np.errstate(invalid='ignore'):
            vis &= ~(L > 0) | (fwd[0] * dx + fwd[1] * dy >= float(spec.fov_cos))
    reach = L - float(spec.slack)
    for cls, _, typ, p in pc.shapes(cfg, items, aux):
        if not spec.occluders & cls or not np.isfinite([x for part in p for x in np.ravel(part)]).all():
            continue
        with np.errstate(invalid='ignore'):
            vis &= ~(first_meeting(typ, p, o, dx, dy) < reach)
    return vis.reshape(h, w)


def stable_reference(cfg, st, items, aux, spec):
    """(visible, exempt) [H, W] bool: exempt = the reference's verdict changes when the cell centre moves by one of SHIFTS."""
    ref = reference(cfg, st, items, aux, spec)
    exempt = np.zeros_like(ref)
    for sh in SHIFTS:
        exempt |= reference(cfg, st, items, aux, spec, sh) != ref
    return ref, exempt


def cell_of(spec, x, y):
    """(row, column) of the cell of a world grid that holds the world point (x, y)."""
    cell = 2.0 / spec.width * float(spec.half_extent)
    return int(np.floor((spec.height / spec.width * float(spec.half_extent) - (y - spec.centre[1])) / cell)), int(np.floor((x - spec.centre[0] + float(spec.half_extent)) / cell))


# ------------------------------------------------------------------------------------------------ states
hand_made = rc.hand_made
spread = pc.spread
far_targets = rc.far_targets
hostile = pc.hostile
