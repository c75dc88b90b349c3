"""Shared by tests/test_cast_host.py and tests/test_gpu_cast.py: the ctypes binding of tests/cast_host/libcast_host.so (the host build of
csrc/cast_core.h), an independent fp64 numpy reference written from include/hrl_cast.h alone (world-coordinate 3-D segments against plain
spheres, finite open cylinders, an oriented box, vertical prisms and the ground plane; its own forward kinematics of the ant and of the
links' body frames from the state record; no cull and no table), and the seeded ray sets the tests cast.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import camera_cases as cc
import render_cases as rc
import scan_cases as sc
from chase_cases import ant_capsules
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import cast_device as Ca

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'cast_host')
KINDS = rc.KINDS
FRAMES = (Ca.HRL_CAST_WORLD, Ca.HRL_CAST_EGO, Ca.HRL_CAST_HEADING, Ca.HRL_CAST_LINK)
NAMES = tuple(n for n, _ in Ca.FIELDS)
DTYPES = (np.float32, np.int32, np.float32, np.float32)
Cast = collections.namedtuple('Cast', NAMES)   # of numpy arrays
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libcast_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libcast_host.so'))
        L.cast_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(Ca.hrl_cast_spec), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Ca.hrl_cast_out)]
        L.cast_host_last_error.restype = C.c_char_p
        L.cast_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(Ca.hrl_cast_spec)]
        L.cast_sizeof_spec.restype = C.c_ulonglong
        L.cast_sizeof_out.restype = C.c_ulonglong
        L.cast_validate_spec.argtypes, L.cast_validate_spec.restype = [C.POINTER(Ca.hrl_cast_spec)], C.c_char_p
        L.cast_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'cast_check_main'])
    return os.path.join(DIR, 'cast_check_main')


ptr = rc.ptr


def spec_of(frame, n_rays, classes=Ca.EVERYTHING):
    """Built field by field (no library call)."""
    return Ca.hrl_cast_spec(n_rays=n_rays, frame=frame, classes=classes)


def shapes_of(n, spec):
    r = min(max(spec.n_rays, 1), Ca.MAX_RAYS)
    return ((n, r), (n, r), (n, r, 3), (n, r, 3))


def cast_host(cfg, state, items, aux, spec, rays, ray_link=None, mask=None, out=None, want=NAMES, expect_ok=True):
    """The host build's answers for (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32, rays [N, R, 6] f32, ray_link [R] i32
    or None): a Cast of arrays; the members not in `want` are None.  `out`: a Cast of arrays (None members are passed as NULL)."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    rays = np.ascontiguousarray(rays, np.float32)
    links = None if ray_link is None else np.ascontiguousarray(ray_link, np.int32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if expect_ok:
        assert rays.shape == (n, spec.n_rays, 6) and (links is None or links.shape == (spec.n_rays,))
    if out is None:
        out = Cast(*(np.zeros(shape, dt) if name in want else None for name, dt, shape in zip(NAMES, DTYPES, shapes_of(n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = Ca.hrl_cast_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().cast_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(rays), ptr(links), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().cast_host_last_error()
        return out
    return code, lib().cast_host_last_error().decode()


bits = cc.bits


def same(a, b):
    """Every member equal, floats compared as uint32."""
    return cc.same(a, b)


# ------------------------------------------------------------------------------------------------ the fp64 reference
BAND = 1e-4   # metres: a ray with a comparison this close to changing is exempt
R_TORSO, R_CAPS, POINT_HALF = 0.25, 0.08, 0.35
LEG_DIR = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))    # assets/ant.xml: the legs' fromto directions ...
ANKLE_AXIS = ((-1.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, 1.0))   # ... and the ankle joints' axes
ground_z = cc.ground_z


def n_links(cfg):
    return 1 if cfg.env_kind == K.HRL_POINT_GATHER else 13


def _rodrigues(axis, th):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)


def link_frames(cfg, st):
    """[(origin [3], R [3, 3])] of every link in world coordinates, link order (hrl_links.h): the torso and the hip capsules carry the
    torso's frame at O; aux 1 + 2 l the frame turned by the hip angle about the body's z, at the hip; the foot 2 + 2 l that frame turned
    by the ankle angle about the ankle's axis, at the ankle."""
    st = np.asarray(st, float)
    o, r0 = st[0:3], rc._rot(st[3:7])
    if cfg.env_kind == K.HRL_POINT_GATHER:
        return [(o, r0)]
    out = [None] * 13
    out[0] = (o, r0)
    for l in range(4):
        d = np.array([LEG_DIR[l][0], LEG_DIR[l][1], 0.0])
        raux = r0 @ _rodrigues((0, 0, 1), st[7 + 2 * l])
        rfoot = raux @ _rodrigues((ANKLE_AXIS[l][0], ANKLE_AXIS[l][1], 0.0), st[8 + 2 * l])
        ph = o + r0 @ (0.2 * d)
        out[9 + l], out[1 + 2 * l], out[2 + 2 * l] = (o, r0), (ph, raux), (ph + raux @ (0.2 * d), rfoot)
    return out


def heading(st):
    return sc.forward(st, 1)   # HRL_SCAN_HEADING


def to_world(cfg, st, frame, rays, ray_link=None):
    """(from [R, 3], to [R, 3], valid [R]) in world coordinates, fp64, by the header's formulas; valid: the ray's link is in range."""
    rays = np.asarray(rays, float)
    a, b = rays[:, 0:3], rays[:, 3:6]
    o = np.asarray(st[0:3], float)
    valid = np.ones(len(rays), bool)
    with np.errstate(invalid='ignore', over='ignore'):
        if frame == Ca.HRL_CAST_WORLD:
            return a, b, valid
        if frame == Ca.HRL_CAST_EGO:
            return o + a, o + b, valid
        if frame == Ca.HRL_CAST_HEADING:
            f = heading(st)
            turn = lambda v: np.stack((f[0] * v[:, 0] - f[1] * v[:, 1], f[1] * v[:, 0] + f[0] * v[:, 1], v[:, 2]), 1)
            return o + turn(a), o + turn(b), valid
        frames = link_frames(cfg, st)
        link = np.zeros(len(rays), np.int64) if ray_link is None else np.asarray(ray_link, np.int64)
        valid = (link >= 0) & (link < len(frames))
        fw, tw = np.full((len(rays), 3), np.nan), np.full((len(rays), 3), np.nan)
        for l, (origin, R) in enumerate(frames):
            sel = link == l
            fw[sel], tw[sel] = origin + a[sel] @ R.T, origin + b[sel] @ R.T
        return fw, tw, valid


def from_world(cfg, st, frame, pts, link=None):
    """World points [R, 3] in the coordinates of `frame` (the inverse of to_world, fp64; link: one link per point)."""
    pts = np.asarray(pts, float)
    o = np.asarray(st[0:3], float)
    if frame == Ca.HRL_CAST_WORLD:
        return pts
    if frame == Ca.HRL_CAST_EGO:
        return pts - o
    if frame == Ca.HRL_CAST_HEADING:
        f, v = heading(st), pts - o
        return np.stack((f[0] * v[:, 0] + f[1] * v[:, 1], -f[1] * v[:, 0] + f[0] * v[:, 1], v[:, 2]), 1)
    frames = link_frames(cfg, st)
    out = np.empty_like(pts)
    for k, p in enumerate(pts):
        origin, R = frames[int(link[k])]
        out[k] = (p - origin) @ R
    return out


def _slab(lo, hi, o, d):
    """The interval of lam with lo <= o + lam d <= hi (arrays o, d): (-inf, inf) or empty for a parallel ray."""
    with np.errstate(divide='ignore', invalid='ignore'):
        a, b = (lo - o) / d, (hi - o) / d
    par, inside = d == 0, (lo <= o) & (o <= hi)
    return np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(a, b)), np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(a, b))


def _near_segment(oc, a, D, dn, radius):
    """Where the ray's line passes within BAND of the distance `radius` from the segment oc .. oc + a (relative to the ray's origin), at a
    place of the segment's line within its ends (widened by the radius and BAND) and along the ray's own extent (widened likewise): a
    silhouette of a cylinder, an edge of a box (radius 0)."""
    la = np.linalg.norm(a)
    ah = a / la
    m = np.cross(D, ah)
    mm = (m * m).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.abs((m * oc).sum(-1)) / np.sqrt(mm)
        n = np.cross(oc, ah)
        t = (m * n).sum(-1) / mm
        s = t * (D * ah).sum(-1) - oc @ ah
        return (np.abs(w - radius) < BAND) & (s > -radius - BAND) & (s < la + radius + BAND) & (t * dn > -radius - BAND) & ((t - 1) * dn < radius + BAND)


def reference(cfg, st, items, aux, spec, rays, ray_link=None):
    """(fraction [R], seg [R], point [R, 3], normal [R, 3], exempt [R]) of one env in fp64.  exempt: some comparison the reference made is
    within BAND of changing: a silhouette (the lateral miss distance of a ground plan, a sphere, a cylinder, an edge of the cube), a seam
    between a cylinder and the neighbouring link's ball, the ray's height at a ground plan's entry against either end of the z-interval,
    a top or bottom point against the ground plan's exit, a candidate against either end of the segment, the ray's origin against a
    solid's surface or the ground, and the winner against a runner-up of another seg that is not exactly tied with it."""
    R = spec.n_rays
    st = np.asarray(st, float)
    O = st[0:3]
    fw, tw, valid = to_world(cfg, st, spec.frame, rays, ray_link)
    with np.errstate(invalid='ignore', over='ignore'):
        D = tw - fw
    dn = np.sqrt((D * D).sum(-1))
    raw = np.asarray(rays, float)
    live = valid & np.isfinite(raw).all(1) & np.isfinite(fw).all(1) & np.isfinite(tw).all(1) & np.isfinite(D).all(1) & (dn > 0) & bool(np.isfinite(O).all())
    exempt = np.zeros(R, bool)
    none = (np.ones(R), np.zeros(R, np.int64), tw, np.zeros((R, 3)), exempt)
    if not live.any():
        return none
    E = np.where(live[:, None], fw, 0.0)
    D = np.where(live[:, None], D, 1.0)
    dn = np.sqrt((D * D).sum(-1))
    dx, dy, dz = D[:, 0], D[:, 1], D[:, 2]
    c = np.sqrt(dx * dx + dy * dy)
    with np.errstate(divide='ignore', invalid='ignore'):
        ux, uy = dx / c, dy / c
    flat = c > 0
    cands = []   # (lam [R] with inf where there is none, seg [R], normal [R, 3])

    def offer(lam, seg, ok, normal):
        nonlocal exempt
        with np.errstate(invalid='ignore'):
            exempt |= ok & ((np.abs(lam - 1.0) * dn < BAND) | (np.abs(lam) * dn < BAND))
            ok = ok & (lam > 0) & (lam <= 1.0)
        cands.append((np.where(ok, lam, np.inf), np.broadcast_to(np.asarray(seg, np.int64), (R,)), np.broadcast_to(np.asarray(normal, float), (R, 3))))

    up = np.array([0.0, 0.0, 1.0])
    for cls, code, typ, p in sc.shapes(cfg, items, aux):
        if not spec.classes & cls or not np.isfinite([x for part in p for x in np.ravel(part)]).all():
            continue
        zl, zh = cc.z_interval(cfg, cls)
        with np.errstate(divide='ignore', invalid='ignore'):
            if typ == 'half':   # the solid beyond the bounding line: n . p + off <= 0; a ray inside it never leaves it (the header's rule)
                (nx, ny), off0 = p
                off, den = nx * E[:, 0] + ny * E[:, 1] + off0, nx * dx + ny * dy
                over, sd = off < 0, np.abs(off)
                l0 = np.where(over, -np.inf, np.where(den < 0, off / -np.where(den < 0, den, -1.0), np.inf))
                l1 = np.full(R, np.inf)
                side = np.full(R, Ca.FACE_SIDE_X if abs(nx) >= abs(ny) else Ca.FACE_SIDE_Y)
                nside = np.broadcast_to(np.array([nx, ny, 0.0]), (R, 3))
            elif typ == 'rect':
                (cx, cy), (hx, hy) = p
                x0, x1 = _slab(cx - hx, cx + hx, E[:, 0], dx)
                y0, y1 = _slab(cy - hy, cy + hy, E[:, 1], dy)
                l0, l1 = np.maximum(x0, y0), np.minimum(x1, y1)
                isx = x0 >= y0
                side = np.where(isx, Ca.FACE_SIDE_X, Ca.FACE_SIDE_Y)
                nside = np.where(isx[:, None], np.stack((-np.sign(dx), 0 * dx, 0 * dx), 1), np.stack((0 * dx, -np.sign(dy), 0 * dx), 1))
                for sx in (-1, 1):   # the verdict of the ground plan changes where the ray's line passes a corner that lies along it
                    for sy in (-1, 1):
                        qx, qy = cx + sx * hx - E[:, 0], cy + sy * hy - E[:, 1]
                        al = qx * ux + qy * uy
                        exempt |= flat & (np.abs(qx * uy - qy * ux) < BAND) & (al > -BAND) & (al < c + BAND)
                sdr = rc._sd_rect(E[:, 0], E[:, 1], (cx, cy), hx, hy)
                over, sd = sdr <= 0, np.abs(sdr)
            else:
                (cx, cy), r = p
                qx, qy = cx - E[:, 0], cy - E[:, 1]
                b, e = (qx * dx + qy * dy) / (c * c), (qx * uy - qy * ux)
                hh = r * r - e * e
                root = np.sqrt(np.maximum(hh, 0.0)) / c
                l0, l1 = np.where(hh >= 0, b - root, np.inf), np.where(hh >= 0, b + root, -np.inf)
                dist = np.hypot(qx, qy)
                over, sd = dist <= r, np.abs(dist - r)
                l0 = np.where(flat, l0, np.where(over, -np.inf, np.inf))   # (a vertical ray stays over the disc, or beside it)
                l1 = np.where(flat, l1, np.where(over, np.inf, -np.inf))
                side = np.full(R, Ca.FACE_ROUND)
                hx_, hy_ = E[:, 0] + l0 * dx - cx, E[:, 1] + l0 * dy - cy
                nside = np.stack((hx_ / r, hy_ / r, 0 * dx), 1)
                exempt |= flat & (np.abs(np.abs(e) - r) < BAND) & (b * c > -r - BAND) & ((b - 1) * c < r + BAND)
            ez = E[:, 2]
            exempt |= ((sd < BAND) & (zl - BAND <= ez) & (ez <= zh + BAND)) | ((over | (sd < BAND)) & ((np.abs(ez - zl) < BAND) | (np.abs(ez - zh) < BAND)))
            z0, z1 = _slab(zl, zh, ez, dz)
            enter, leave = np.maximum(l0, z0), np.minimum(l1, z1)
            hit = (enter <= leave) & (enter > 0)
            by_side = l0 >= z0
            face = np.where(by_side, side, np.where(dz < 0, Ca.FACE_TOP, Ca.FACE_BOTTOM))
            normal = np.where(by_side[:, None], nside, np.where((dz < 0)[:, None], up, -up))
            a = np.maximum(l0, 0.0)
            span = (l0 <= l1) & (l1 >= 0) & (a <= 1.0 + BAND / dn)
            za = ez + dz * a
            exempt |= span & np.isfinite(za) & ((np.abs(za - zl) < BAND) | (np.abs(za - zh) < BAND))
            exempt |= span & np.isfinite(z0) & np.isfinite(l1) & (np.abs((z0 - l1) * c) < BAND) & (z0 >= 0)
            exempt |= hit & np.isfinite(l0) & np.isfinite(z0) & (np.abs((l0 - z0) * dn) < BAND)
        offer(enter, code | (face << 16), hit, normal)

    if spec.classes & Ca.ROBOT and np.isfinite(O).all():
        with np.errstate(divide='ignore', invalid='ignore'):
            if cfg.env_kind == K.HRL_POINT_GATHER:
                Rm = rc._rot(st[3:7])
                if np.isfinite(Rm).all():
                    ob, db = (E - O) @ Rm, D @ Rm   # the ray in body axes
                    lo, hi = [], []
                    for k in range(3):
                        a0, a1 = _slab(-POINT_HALF, POINT_HALF, ob[:, k], db[:, k])
                        lo.append(a0); hi.append(a1)
                    tn, tf = np.maximum(np.maximum(lo[0], lo[1]), lo[2]), np.minimum(np.minimum(hi[0], hi[1]), hi[2])
                    fx, fy = (lo[0] >= lo[1]) & (lo[0] >= lo[2]), lo[1] >= lo[2]
                    face = np.where(fx, Ca.FACE_SIDE_X, np.where(fy, Ca.FACE_SIDE_Y, np.where(db[:, 2] < 0, Ca.FACE_TOP, Ca.FACE_BOTTOM)))
                    axis = np.where(fx, 0, np.where(fy, 1, 2))
                    unit = Rm / np.linalg.norm(Rm, axis=0)
                    normal = -np.sign(np.take_along_axis(db, axis[:, None], 1)) * unit.T[axis]
                    for k in range(3):   # the 12 edges: silhouettes and the lines between two faces
                        for s1 in (-1, 1):
                            for s2 in (-1, 1):
                                corner = np.zeros(3)
                                corner[k], corner[(k + 1) % 3], corner[(k + 2) % 3] = -POINT_HALF, s1 * POINT_HALF, s2 * POINT_HALF
                                exempt |= _near_segment(O + Rm @ corner - E, Rm[:, k] * 2 * POINT_HALF, D, dn, 0.0)
                    exempt |= (np.abs(np.abs(ob) - POINT_HALF).min(1) < BAND) & (np.abs(ob) < POINT_HALF + BAND).all(1)
                    offer(tn, Ca.HIT_ROBOT | (face << 16), (tn <= tf) & (tn > 0), normal)
            else:
                def sphere(link, centre, r):
                    nonlocal exempt
                    if not np.isfinite(centre).all():
                        return
                    oc = centre - E
                    b = (D * oc).sum(-1) / dn
                    pp = np.sqrt((np.cross(oc, D) ** 2).sum(-1)) / dn   # the centre's distance from the ray's line
                    exempt |= (np.abs(pp - r) < BAND) & (b > -r - BAND) & (b - dn < r + BAND)
                    exempt |= np.abs(np.linalg.norm(oc, axis=1) - r) < BAND
                    lam = (b - np.sqrt(np.maximum(r * r - pp * pp, 0.0))) / dn
                    normal = (E + lam[:, None] * D - centre) / r
                    offer(lam, Ca.HIT_ROBOT | (link << 8) | (Ca.FACE_ROUND << 16), pp <= r, normal)

                sphere(0, O, R_TORSO)
                for link, p0, p1 in ant_capsules(st):
                    if np.isfinite(p0).all() and np.isfinite(p1).all():
                        oc, a = p0 - E, p1 - p0
                        la = np.linalg.norm(a)
                        ah = a / la
                        m = np.cross(D, ah)
                        mm = (m * m).sum(-1)
                        wd = (m * oc).sum(-1)
                        hh = R_CAPS * R_CAPS * mm - wd * wd
                        lam = ((m * np.cross(oc, ah)).sum(-1) - np.sqrt(np.maximum(hh, 0.0))) / mm
                        s = lam * (D * ah).sum(-1) - oc @ ah
                        q = lam[:, None] * D - oc
                        normal = (q - (q @ ah)[:, None] * ah) / R_CAPS
                        exempt |= _near_segment(oc, a, D, dn, R_CAPS)
                        exempt |= (hh >= 0) & (lam > 0) & (lam <= 1 + BAND / dn) & ((np.abs(s) < BAND) | (np.abs(s - la) < BAND))   # the seams at the cylinder's ends
                        offer(lam, Ca.HIT_ROBOT | (link << 8) | (Ca.FACE_ROUND << 16), (hh >= 0) & (s >= 0) & (s <= la), normal)
                    sphere(link, p1, R_CAPS)

    if spec.classes & Ca.GROUND:
        gz = ground_z(cfg)
        with np.errstate(divide='ignore', invalid='ignore'):
            lam = np.where(dz < 0, (gz - E[:, 2]) / np.where(dz < 0, dz, -1.0), np.inf)
        offer(lam, Ca.HIT_GROUND | (Ca.FACE_GROUND << 16), (dz < 0) & (E[:, 2] > gz), up)
        exempt |= np.abs(E[:, 2] - gz) < BAND

    if not cands:
        return none
    lams, segs, normals = np.stack([x for x, _, _ in cands]), np.stack([x for _, x, _ in cands]), np.stack([x for _, _, x in cands])
    lams = np.where(live[None], lams, np.inf)
    first = np.argmin(lams, axis=0)   # the first of equal ones: the earlier candidate wins a tie
    best = np.take_along_axis(lams, first[None], 0)[0]
    met = np.isfinite(best)
    seg = np.where(met, np.take_along_axis(segs, first[None], 0)[0], 0)
    normal = np.where(met[:, None], np.take_along_axis(normals, first[None, :, None], 0)[0], 0.0)
    with np.errstate(invalid='ignore'):   # (an exact tie is no near-tie: the tie rule decides it in any precision)
        exempt |= (((lams - best[None]) * dn[None] < BAND) & (lams > best[None]) & (segs != seg[None])).any(0)
        point = np.where(met[:, None], fw + np.where(met, best, 0.0)[:, None] * (tw - fw), tw)
    return np.where(met, best, 1.0), seg, point, normal, exempt & live


# ------------------------------------------------------------------------------------------------ ray sets
LIDAR = dict(n_azimuth=18, elevations_degrees=(-30.0, -10.0, 0.0, 15.0), max_range=8.0, min_range=0.3)
N_RANDOM = 120


def ray_set(cfg, state, items, frame, seed):
    """(rays [N, R, 6] float32, ray_link [R] int32 or None) for a shard's states, seeded and deterministic: per env a 3-D lidar of 4 rings
    x 18 (20 degrees apart: no ray along a diagonal of the point bot's cube; from the torso; in the link frame: of the torso's body, so it pitches and rolls with it), a ray at each foot tip (the link
    frame: cast_device.down_rays; elsewhere straight down from the tips), 120 random segments across the arena, and rays that start
    inside the torso, inside an item cube (gather) or the maze box, and under the ground."""
    rng = np.random.default_rng(seed)
    n = len(state)
    lidar = Ca.lidar_rays(**LIDAR).numpy().astype(float)
    feet, foot_links = (x.numpy() for x in Ca.down_rays(1.0))
    rl = rng.integers(0, n_links(cfg), N_RANDOM)   # ray_link is shared by the envs
    out, links = [], None
    for e in range(n):
        st = np.asarray(state[e], float)
        parts, lk = [], []
        w = lambda pts, link=None: from_world(cfg, st, frame, pts, link)   # world points -> the frame's coordinates
        parts.append(np.concatenate((lidar[:, 0:3] + (st[0:3] if frame == Ca.HRL_CAST_WORLD else 0), lidar[:, 3:6] + (st[0:3] if frame == Ca.HRL_CAST_WORLD else 0)), 1))
        lk += [0] * len(lidar)
        if frame == Ca.HRL_CAST_LINK:
            parts.append(feet.astype(float))
            lk += list(foot_links)
        else:
            tips = np.array([p1 for link, _, p1 in ant_capsules(st) if link in Ca.FOOT_LINKS])
            parts.append(np.concatenate((w(tips), w(tips - (0.0, 0.0, 1.0))), 1))
            lk += [0] * 4
        if frame == Ca.HRL_CAST_WORLD:
            a = np.stack((rng.uniform(-4, 4, N_RANDOM), rng.uniform(-4, 4, N_RANDOM), rng.uniform(0.05, 2.0, N_RANDOM)), 1)
            b = np.stack((rng.uniform(-6, 6, N_RANDOM), rng.uniform(-6, 6, N_RANDOM), rng.uniform(-0.5, 1.0, N_RANDOM)), 1)
        else:
            a = np.stack((rng.uniform(-2, 2, N_RANDOM), rng.uniform(-2, 2, N_RANDOM), rng.uniform(-0.4, 1.5, N_RANDOM)), 1)
            b = np.stack((rng.uniform(-6, 6, N_RANDOM), rng.uniform(-6, 6, N_RANDOM), rng.uniform(-1.0, 0.5, N_RANDOM)), 1)
        parts.append(np.concatenate((a, b), 1))
        lk += list(rl)
        # from inside the torso (the cube), inside a solid of the scene, and from under the ground
        inner = st[0:3] + rng.uniform(-0.1, 0.1, (4, 3))
        if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) and items is not None:
            solid = np.array([float(items[e][0]), float(items[e][1]), 0.1]) + rng.uniform(-0.08, 0.08, (4, 3))
        else:
            solid = np.array([-2.0, 0.0, 1.0]) + rng.uniform(-1.0, 1.0, (4, 3))   # the maze's box (elsewhere: free space)
        under = np.stack((st[0] + rng.uniform(-2, 2, 4), st[1] + rng.uniform(-2, 2, 4), ground_z(cfg) - rng.uniform(0.1, 0.5, 4)), 1)
        starts = np.concatenate((inner, solid, under))
        ends = starts + rng.uniform(-3, 3, (12, 3)) + (0.0, 0.0, 1.0) * np.repeat((0.0, 0.0, 1.5), 4)[:, None]
        sl = np.zeros(12, np.int64)
        parts.append(np.concatenate((w(starts, sl), w(ends, sl)), 1))
        lk += [0] * 12
        out.append(np.concatenate(parts))
        links = np.asarray(lk, np.int32)
    return np.stack(out).astype(np.float32), (links if frame == Ca.HRL_CAST_LINK else None)


def sized_ray_set(cfg, state, items, frame, n_rays, seed):
    """n_rays rays per env out of ray_set(), every seventh in turn so that a small count still holds rays of every sort, repeated beyond
    the set's size; a repeated ray's `to` is moved by up to 0.2 m (seeded), so no two rays are one."""
    rays, links = ray_set(cfg, state, items, frame, seed)
    idx = (7 * np.arange(n_rays)) % rays.shape[1]   # (7 and the set's 208 rays have no common factor)
    out = np.array(rays[:, idx])
    rng = np.random.default_rng(seed + 1)
    out[:, rays.shape[1]:, 3:6] += rng.uniform(-0.2, 0.2, (len(state), max(n_rays - rays.shape[1], 0), 3)).astype(np.float32)
    return np.ascontiguousarray(out), (None if links is None else np.ascontiguousarray(links[idx]))


# ------------------------------------------------------------------------------------------------ states
hostile = cc.hostile
spread = cc.spread
far_targets = cc.far_targets
