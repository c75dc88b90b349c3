"""Shared by tests/test_closest_host.py, tests/test_closest_launch.py and tests/test_gpu_closest.py: the ctypes binding of
tests/closest_host/libclosest_host.so (the host build of csrc/closest_core.h), an independent fp64 numpy reference written from
include/hrl_closest.h alone (its own forward kinematics of the ant from the state record, the surfaces from the config's world size and
the items record, the segment - box distance minimised piece by piece over the axis, segment - segment distances, the cube's corner
sets), the certificate that holds the build against it, and the map from the contact report's link codes to links.  Test infrastructure
only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import camera_cases as cc
import probe_cases as pc
import render_cases as rc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import closest_device as Cl

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'closest_host')
KINDS = rc.KINDS
NAMES = tuple(n for n, _ in Cl.FIELDS)
DTYPES = (np.float32, np.int32, np.float32, np.float32, np.float32)
Closest = collections.namedtuple('Closest', NAMES)   # of numpy arrays
GROUND, WALL, BOX, FOOD, POISON, SELF = range(6)     # the class axis
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libclosest_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libclosest_host.so'))
        L.closest_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(Cl.hrl_closest_spec), C.c_void_p, C.POINTER(Cl.hrl_closest_out)]
        L.closest_host_last_error.restype = C.c_char_p
        L.closest_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.POINTER(Cl.hrl_closest_spec)]
        L.closest_sizeof_spec.restype = C.c_ulonglong
        L.closest_sizeof_out.restype = C.c_ulonglong
        L.closest_validate_spec.argtypes, L.closest_validate_spec.restype = [C.POINTER(Cl.hrl_closest_spec)], C.c_char_p
        L.closest_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'closest_check_main'])
    return os.path.join(DIR, 'closest_check_main')


ptr = rc.ptr


def spec_of(classes=Cl.EVERYTHING):
    """Built field by field (no library call)."""
    return Cl.hrl_closest_spec(classes=classes)


def n_links(cfg):
    return 1 if cfg.env_kind == K.HRL_POINT_GATHER else 13


def shapes_of(n, cfg):
    cell = (n, n_links(cfg), 6)
    return (cell, cell, cell + (3,), cell + (3,), cell + (3,))


def closest_host(cfg, state, items, aux, spec=None, mask=None, out=None, want=NAMES, expect_ok=True):
    """The host build's answers for (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32): a Closest of arrays; the members
    not in `want` are None.  `out`: a Closest of arrays (None members are passed as NULL)."""
    spec = spec_of() if spec is None else spec
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if out is None:
        out = Closest(*(np.zeros(shape, dt) if name in want else None for name, dt, shape in zip(NAMES, DTYPES, shapes_of(n, cfg))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = Cl.hrl_closest_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().closest_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().closest_host_last_error()
        return out
    return code, lib().closest_host_last_error().decode()


bits = cc.bits


def same(a, b):
    """Every member equal, floats compared as uint32."""
    return cc.same(a, b)


# ------------------------------------------------------------------------------------------------ the fp64 reference, from the header
R_TORSO, R_CAPS, CUBE_HALF, ITEM_HALF, ITEM_Z = 0.25, 0.08, 0.35, 0.125, 0.1
LEG_DIR = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))    # assets/ant.xml: the legs' fromto directions ...
ANKLE_AXIS = ((-1.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, 1.0))   # ... and the ankle joints' axes
ground_z = cc.ground_z


def _rodrigues(axis, th):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)


def link_segments(st):
    """[(p0, p1, radius)] of the ant's 13 links in world coordinates, link order (hrl_links.h): the torso a segment of length zero."""
    st = np.asarray(st, float)
    o, r0 = st[0:3], rc._rot(st[3:7])
    out = [None] * 13
    out[0] = (o, o, R_TORSO)
    for l in range(4):
        d = np.array([LEG_DIR[l][0], LEG_DIR[l][1], 0.0])
        raux = r0 @ _rodrigues((0, 0, 1), st[7 + 2 * l])
        rfoot = raux @ _rodrigues((ANKLE_AXIS[l][0], ANKLE_AXIS[l][1], 0.0), st[8 + 2 * l])
        hip = o + r0 @ (0.2 * d)
        ankle = hip + raux @ (0.2 * d)
        out[9 + l], out[1 + 2 * l], out[2 + 2 * l] = (o, hip, R_CAPS), (hip, ankle, R_CAPS), (ankle, ankle + rfoot @ (0.4 * d), R_CAPS)
    return out


def leg_of(link):
    """(leg, segment) of a capsule link: segment 0 the hip capsule, 1 the aux body, 2 the foot."""
    return (link - 9, 0) if link >= 9 else ((link - 1) // 2, 1 + (link - 1) % 2)


def self_pairs(link):
    """The links the step pairs `link` with: the capsules of the other legs, never hip capsule against hip capsule; none for the torso."""
    if link == 0:
        return []
    leg, seg = leg_of(link)
    return [o for o in range(1, 13) if leg_of(o)[0] != leg and (seg != 0 or leg_of(o)[1] != 0)]


def surfaces(cfg, items):
    """{class: [(index, 'plane', n, d) or (index, 'box', lo, hi)]} of one env: what the step collides with, from the header's words."""
    out = {GROUND: [(0, 'plane', np.array([0.0, 0.0, 1.0]), ground_z(cfg))], WALL: [], BOX: [], FOOD: [], POISON: []}
    ar = rc.arena(cfg)   # the planes' half sizes: the walls' inner faces
    if ar is not None:
        for i, (n, d) in enumerate((((-1.0, 0.0, 0.0), -ar[0]), ((1.0, 0.0, 0.0), -ar[0]), ((0.0, -1.0, 0.0), -ar[1]), ((0.0, 1.0, 0.0), -ar[1]))):
            out[WALL].append((i, 'plane', np.array(n), d))
    if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        out[BOX].append((0, 'box', np.array([-5.0, -2.0, 0.0]), np.array([1.0, 2.0, 2.0])))
    if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) and items is not None:
        for i in range(cfg.n_food + cfg.n_poison):
            c = np.array([float(items[2 * i]), float(items[2 * i + 1]), ITEM_Z])
            out[FOOD if i < cfg.n_food else POISON].append((i, 'box', c - ITEM_HALF, c + ITEM_HALF))
    return out


def word_of(cls, idx):
    return Cl.CLASS_HITS[cls] | idx << 8


def seg_box(p0, p1, lo, hi):
    """(gap, t) of the segment p0 - p1 against the box in fp64: the least distance of an axis point to the solid (0: the axis meets it)
    and a parameter where it is taken.  |P(t) - clamp(P(t))|^2 is convex and, between the times at which a coordinate crosses a face,
    a quadratic: it is minimised piece by piece."""
    d = p1 - p0
    ts = [0.0, 1.0]
    for k in range(3):
        if d[k] != 0:
            ts += [t for t in ((lo[k] - p0[k]) / d[k], (hi[k] - p0[k]) / d[k]) if 0 < t < 1]
    ts = sorted(set(ts))
    cands = list(ts)
    for a, b in zip(ts[:-1], ts[1:]):
        x = p0 + 0.5 * (a + b) * d
        bound = np.where(x < lo, lo, np.where(x > hi, hi, np.nan))   # the face each coordinate is outside of, on this piece
        act = ~np.isnan(bound)
        den = (d[act] ** 2).sum()
        if den > 0:
            cands.append(float(np.clip(-(d[act] * (p0[act] - bound[act])).sum() / den, a, b)))
    best = None
    for t in cands:
        x = p0 + t * d
        g = float(np.linalg.norm(x - np.clip(x, lo, hi)))
        if best is None or g < best[0]:
            best = (g, t)
    return best


def box_depth(p0, p1, lo, hi):
    """(depth, x) of the header's rule where the axis runs through the solid: the depth of the nearest face at the middle x of the
    stretch."""
    d = p1 - p0
    a, b = 0.0, 1.0
    for k in range(3):
        if d[k] != 0:
            u, v = sorted(((lo[k] - p0[k]) / d[k], (hi[k] - p0[k]) / d[k]))
            a, b = max(a, u), min(b, v)
    x = p0 + 0.5 * (a + b) * d
    return float(min((x - lo).min(), (hi - x).min())), x


def seg_seg(p1, q1, p2, q2):
    """The least distance of two segments in fp64: each end against the other segment, and the lines' closest points where they lie
    within both."""
    def point_seg(x, a, b):
        d = b - a
        L = d @ d
        t = np.clip((x - a) @ d / L, 0, 1) if L > 0 else 0.0
        return np.linalg.norm(x - (a + t * d))
    best = min(point_seg(p1, p2, q2), point_seg(q1, p2, q2), point_seg(p2, p1, q1), point_seg(q2, p1, q1))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = d1 @ d1, d2 @ d2, d1 @ d2, d1 @ r, d2 @ r
    den = a * e - b * b
    if den > 1e-14 * a * e:
        s, t = (b * f - c * e) / den, (a * f - b * c) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            best = min(best, np.linalg.norm((p1 + s * d1) - (p2 + t * d2)))
    return float(best)


def cube_corners(st):
    o, R = np.asarray(st[0:3], float), rc._rot(np.asarray(st[3:7], float))
    return o, R, [o + R @ (CUBE_HALF * np.array([sx, sy, sz])) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]


def box_signed(x, lo, hi):
    """The signed distance of a point to an axis-aligned box's surface (negative inside)."""
    out = np.linalg.norm(x - np.clip(x, lo, hi))
    return float(out) if out > 0 else -float(min((x - lo).min(), (hi - x).min()))


def gap_of(cfg, st, link, surf, segs=None):
    """(gap, meets) in fp64 of `link` against the surface tuple `surf` (of surfaces(), or (other, 'link')): the header's distance;
    meets: the axis runs through the solid, where the header promises the depth of the nearest face at the middle of the stretch."""
    if cfg.env_kind == K.HRL_POINT_GATHER:
        o, R, corners = cube_corners(st)
        if surf[1] == 'plane':
            return min(float(surf[2] @ c - surf[3]) for c in corners), False
        lo, hi = surf[2], surf[3]
        mine = min(box_signed(c, lo, hi) for c in corners)
        theirs = min(box_signed(R.T @ (np.array([x, y, z]) - o), -CUBE_HALF * np.ones(3), CUBE_HALF * np.ones(3)) for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0]))
        return min(mine, theirs), False
    segs = link_segments(st) if segs is None else segs
    p0, p1, r = segs[link]
    if surf[1] == 'plane':
        return min(float(surf[2] @ p0 - surf[3]), float(surf[2] @ p1 - surf[3])) - r, False
    if surf[1] == 'link':
        q0, q1, _ = segs[surf[0]]
        return seg_seg(p0, p1, q0, q1) - 2 * R_CAPS, False
    g, _ = seg_box(p0, p1, surf[2], surf[3])
    if g > 0:
        return g - r, False
    return -box_depth(p0, p1, surf[2], surf[3])[0] - r, True


def class_surfaces(cfg, st, items, link):
    """{class: [surface tuples]} of one link, the self class included."""
    out = surfaces(cfg, items)
    out[SELF] = [] if cfg.env_kind == K.HRL_POINT_GATHER else [(o, 'link') for o in self_pairs(link)]
    return out


def on_shape(cfg, st, link, surf, a, b, segs, meets=False):
    """(how far `a` is from the link's surface, how far `b` is from the other shape's), fp64.  meets: the link's axis runs through the
    box -- there the header's on_link = x - r n lies on the SPHERE of radius r about the axis point x (the middle of the stretch) that
    stands in for the capsule, as in the step, and not on the capsule's surface unless the face's normal is square to the axis: `a` is
    held to that sphere."""
    def seg_dist(x, p0, p1):
        d = p1 - p0
        L = d @ d
        t = np.clip((x - p0) @ d / L, 0, 1) if L > 0 else 0.0
        return float(np.linalg.norm(x - (p0 + t * d)))
    if cfg.env_kind == K.HRL_POINT_GATHER:
        o, R, _ = cube_corners(st)
        ea = abs(box_signed(R.T @ (a - o), -CUBE_HALF * np.ones(3), CUBE_HALF * np.ones(3)))
    else:
        p0, p1, r = segs[link]
        ea = abs(np.linalg.norm(a - box_depth(p0, p1, surf[2], surf[3])[1]) - r) if meets else abs(seg_dist(a, p0, p1) - r)
    if surf[1] == 'plane':
        eb = abs(float(surf[2] @ b - surf[3]))
    elif surf[1] == 'link':
        q0, q1, _ = segs[surf[0]]
        eb = abs(seg_dist(b, q0, q1) - R_CAPS)
    else:
        eb = abs(box_signed(b, surf[2], surf[3]))
    return ea, eb


def certificate(cfg, state, items, got, classes=Cl.EVERYTHING, tol=None, where=()):
    """The certificate of tests/test_closest_host.py on every cell of a batch; returns the worst figures (a: |distance - the fp64 gap of
    the surface named by which|; b: that gap minus the fp64 minimum over the class; c: the points off their surfaces and
    ||on_link - on_surface| - |distance||; d: the normal against the points' direction) and the count of finite cells per class.  With
    `tol` = (DIST_TOL, POINT_TOL, NORMAL_TOL) every figure is asserted.  Always asserted: which is NONE exactly where distance is +inf
    and there the vectors are zeros; a finite cell names a surface of its class; a class with a surface and finite links has a finite
    cell; the normal's length is 1 within 1e-6."""
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0)
    seen = collections.Counter()
    for e in range(len(state)):
        st = np.asarray(state[e], float)
        it = None if items is None else items[e]
        point = cfg.env_kind == K.HRL_POINT_GATHER
        segs = None if point else link_segments(st)
        for link in range(n_links(cfg)):
            per_class = class_surfaces(cfg, st, it, link)
            for cls in range(6):
                w = (where, e, link, cls)
                dist, which = float(got.distance[e, link, cls]), int(got.which[e, link, cls])
                a, b, n = (got[k][e, link, cls].astype(float) for k in (2, 3, 4))
                asked = bool(classes & Cl.CLASS_BITS[cls])
                surfs = per_class[cls] if asked else []
                assert (which == Cl.HIT_NONE) == (dist == np.inf), w
                if not surfs:
                    assert which == Cl.HIT_NONE, w
                if which == Cl.HIT_NONE:
                    assert not a.any() and not b.any() and not n.any(), w
                    assert not surfs, (w, 'a class with surfaces reports nothing')
                    continue
                seen[cls] += 1
                named = [s for s in surfs if word_of(cls, s[0]) == which]
                assert len(named) == 1, (w, which)
                gaps = [gap_of(cfg, st, link, s, segs) for s in surfs]
                g, meets = gap_of(cfg, st, link, named[0], segs)
                r = 0.0 if point else segs[link][2]
                if meets:
                    assert tol is None or dist <= -r + tol[0], (w, dist)
                else:
                    worst['a'] = max(worst['a'], abs(dist - g))
                    assert tol is None or abs(dist - g) <= tol[0], (w, 'a', dist, g)
                lead = g - min(x for x, _ in gaps)
                worst['b'] = max(worst['b'], lead)
                assert tol is None or lead <= tol[0], (w, 'b', g, min(x for x, _ in gaps))
                ea, eb = on_shape(cfg, st, link, named[0], a, b, segs, meets)
                sep = np.linalg.norm(a - b)
                ec = max(ea, eb, abs(sep - abs(dist)))
                worst['c'] = max(worst['c'], ec)
                assert tol is None or ec <= tol[1], (w, 'c', ea, eb, sep, dist)
                assert abs(np.linalg.norm(n) - 1.0) <= 1e-6, (w, n)
                if abs(dist) >= 1e-3:
                    ed = float(np.abs(n - np.sign(dist) * (a - b) / sep).max())
                    worst['d'] = max(worst['d'], ed)
                    assert tol is None or ed <= tol[2], (w, 'd', n, (a - b) / sep)
    return worst, seen


# ------------------------------------------------------------------------------------------------ the contact report's link codes
def links_of_code(code, self_contact=False):
    """The links (links_device.NAMES order) a contact's link code `level | leg << 2` can name: level 1 is the aux body 1 + 2 leg, level 2
    the foot 2 + 2 leg, level 0 the hip capsule 9 + leg -- and code 0 is the torso's sphere as well (not in a self contact: the torso
    is in no capsule pair)."""
    level, leg = code & 3, code >> 2
    if level == 0:
        return (9 + leg,) if (self_contact or leg != 0) else (0, 9)
    return (2 * leg + level,)


def class_of_surface(cfg, surf):
    """(class, index) of an external contact's surface code (hrl_envs.h: HRL_SURF_*)."""
    if surf == 0:
        return GROUND, 0
    if surf < K.HRL_SURF_BOX:
        return WALL, surf - 1
    if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        return BOX, 0
    i = surf - K.HRL_SURF_ITEM if surf < K.HRL_SURF_SELF else surf - K.HRL_SURF_SELF
    return (FOOD if i < cfg.n_food else POISON), i


# ------------------------------------------------------------------------------------------------ states
hostile = cc.hostile
spread = pc.spread
far_targets = cc.far_targets
