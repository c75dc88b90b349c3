"""Shared by tests/test_chase_host.py and tests/test_gpu_chase.py: the ctypes binding of tests/chase_host/libchase_host.so (the host build
of csrc/chase_core.h), an independent fp64 numpy reference written from include/hrl_chase.h alone (world-coordinate 3-D rays against plain
spheres, finite open cylinders, an oriented box, vertical prisms and the ground plane; its own forward kinematics of the ant from the state
record; no cull and no table), and the specs the tests take images with.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import camera_cases as cc
import render_cases as rc
import scan_cases as sc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import chase_device as Ch

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'chase_host')
KINDS = rc.KINDS
FRAMES = (Ch.HRL_SCAN_WORLD, Ch.HRL_SCAN_HEADING)
TARGET_MODES = (Ch.HRL_EYE_GROUND, Ch.HRL_EYE_TORSO)
SIZES = ((16, 8), (48, 24), (64, 48), (256, 256))   # width, height: 128 pixels, two waves idle | 1152, the last pass half full | 3072 | the maximum: every rgb chunk boundary
PITCHES = (-85.0, -60.0, -30.0, -10.0, 20.0)        # degrees; -90 once per kind
DISTANCES = (1.5, 3.0, 6.0)
YAWS = (0.0, 75.0, 200.0)
CLASS_SETS = (Ch.EVERYTHING, Ch.ROBOT, Ch.EVERYTHING & ~Ch.ROBOT, Ch.GROUND)   # everything | the robot alone | everything but the robot | the ground alone
TILES = (0.0, 1.0)
TANS = (0.5773502691896257, 0.9489645667148802)     # tangents of half of 60 and of 87 degrees
NAMES = tuple(n for n, _ in Ch.FIELDS)
DTYPES = (np.float32, np.int32, np.uint8)
Chase = collections.namedtuple('Chase', NAMES)   # of numpy arrays
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libchase_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libchase_host.so'))
        L.chase_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(Ch.hrl_chase_spec), C.c_void_p, C.POINTER(Ch.hrl_chase_out)]
        L.chase_host_last_error.restype = C.c_char_p
        L.chase_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(Ch.hrl_chase_spec)]
        L.chase_sizeof_spec.restype = C.c_ulonglong
        L.chase_sizeof_out.restype = C.c_ulonglong
        L.chase_validate_spec.argtypes, L.chase_validate_spec.restype = [C.POINTER(Ch.hrl_chase_spec)], C.c_char_p
        L.chase_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        L.chase_shade_rgb.argtypes, L.chase_shade_rgb.restype = [C.c_int], C.c_uint
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'chase_check_main'])
    return os.path.join(DIR, 'chase_check_main')


ptr = rc.ptr


def spec_of(size, frame, target_mode=Ch.HRL_EYE_TORSO, target_height=0.0, yaw=0.0, pitch=-30.0, distance=3.0, classes=Ch.EVERYTHING, max_range=30.0, tan_half_h=TANS[0],
            tan_half_v=None, tile=1.0):
    """yaw, pitch: degrees.  tan_half_v = None: square pixels.  Built field by field (no library call)."""
    w, h = size
    s = Ch.hrl_chase_spec(width=w, height=h, frame=frame, target_mode=target_mode, target_height=target_height, distance=distance, tan_half_h=tan_half_h,
                          tan_half_v=tan_half_h * h / w if tan_half_v is None else tan_half_v, max_range=max_range, classes=classes, tile=tile)
    s.yaw[0], s.yaw[1] = Ch.pair(yaw)
    s.pitch[0], s.pitch[1] = Ch.pair(pitch)
    return s


def sweep(kind):
    """The specs of the sweeps of one kind: both frames x both target modes x SIZES, with PITCHES, DISTANCES, YAWS, CLASS_SETS, TILES, two
    ranges and two fields of view taken in turn (the kind shifts the turn, so the pairings differ over the six kinds); the kind's first
    64 x 48 image looks straight down (pitch -90)."""
    out, turn = [], int(kind)
    for frame in FRAMES:
        for mode in TARGET_MODES:
            for size in SIZES:
                pitch = -90.0 if (frame, mode, size) == (FRAMES[0], TARGET_MODES[0], SIZES[2]) else PITCHES[turn % 5]
                out.append(spec_of(size, frame, mode, 0.3 if mode == Ch.HRL_EYE_GROUND else 0.0, YAWS[(turn // 2) % 3], pitch, DISTANCES[turn % 3],
                                   CLASS_SETS[turn % 4], 7.0 if turn % 5 == 2 else 30.0, TANS[(turn // 5) % 2], tile=TILES[(turn // 4 + turn) % 2]))
                turn += 1
    return out


def shapes_of(n, spec):
    h, w = min(max(spec.height, 1), 256), min(max(spec.width, 1), 256)
    return ((n, h, w), (n, h, w), (n, h, w, 3))


def chase_host(cfg, state, items, aux, spec, mask=None, out=None, want=NAMES, expect_ok=True):
    """The host build's images of (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32): a Chase of arrays; the members not in
    `want` are None.  `out`: a Chase of arrays (None members are passed as NULL) to write into."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if out is None:
        out = Chase(*(np.zeros(shape, dt) if name in want else None for name, dt, shape in zip(NAMES, DTYPES, shapes_of(n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = Ch.hrl_chase_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().chase_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().chase_host_last_error()
        return out
    return code, lib().chase_host_last_error().decode()


bits = cc.bits


def same(a, b):
    """Every member equal, depth compared as uint32."""
    return cc.same(a, b)


# ------------------------------------------------------------------------------------------------ the fp64 reference
BAND = 1e-4   # metres: a pixel with a comparison this close to changing is exempt
R_TORSO, R_CAPS, POINT_HALF = 0.25, 0.08, 0.35
LEG_DIR = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))    # assets/ant.xml: the legs' fromto directions ...
ANKLE_AXIS = ((-1.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, 1.0))   # ... and the ankle joints' axes
COLOURS = dict(cc.COLOURS)
LINK_COLOURS = [Ch.RGB_TORSO] + [Ch.RGB_LEG1, Ch.RGB_LEG2] * 4 + [Ch.RGB_LEG0] * 4   # the torso | aux, foot per leg | the hip capsules
ground_z = cc.ground_z


def _rodrigues(axis, th):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)


def ant_capsules(st):
    """[(link, p0, p1)] of the 12 capsule links in world coordinates, link order, from the state record: the hip capsule 9 + l from the
    torso's origin to the hip, aux 1 + 2 l from the hip to the ankle (turned by the hip angle about the body's z), the foot 2 + 2 l from
    the ankle to the tip (turned by the ankle angle about the ankle's axis)."""
    st = np.asarray(st, float)
    o, r0 = st[0:3], rc._rot(st[3:7])
    caps = {}
    for l in range(4):
        d = np.array([LEG_DIR[l][0], LEG_DIR[l][1], 0.0])
        raux = r0 @ _rodrigues((0, 0, 1), st[7 + 2 * l])
        rfoot = raux @ _rodrigues((ANKLE_AXIS[l][0], ANKLE_AXIS[l][1], 0.0), st[8 + 2 * l])
        ph = o + r0 @ (0.2 * d)
        pa = ph + raux @ (0.2 * d)
        tip = pa + rfoot @ (0.4 * d)
        caps[9 + l], caps[1 + 2 * l], caps[2 + 2 * l] = (o, ph), (ph, pa), (pa, tip)
    return [(link,) + caps[link] for link in sorted(caps)]


def camera_of(cfg, st, spec):
    """(E, F, L, U) in fp64, from the header."""
    f = sc.forward(st, spec.frame)
    cy, sy, cp, sp = (float(x) for x in (spec.yaw[0], spec.yaw[1], spec.pitch[0], spec.pitch[1]))
    g = np.array([f[0] * cy - f[1] * sy, f[1] * cy + f[0] * sy])
    F = np.array([cp * g[0], cp * g[1], sp])
    L = np.array([-g[1], g[0], 0.0])
    U = np.array([-sp * g[0], -sp * g[1], cp])
    tz = (float(st[2]) if spec.target_mode == Ch.HRL_EYE_TORSO else ground_z(cfg)) + float(spec.target_height)
    T = np.array([float(st[0]), float(st[1]), tz])
    return T - float(spec.distance) * F, F, L, U


def rays(spec, F, L, U):
    w, h = spec.width, spec.height
    u = (w - (2 * np.arange(w) + 1)) / w * float(spec.tan_half_h)
    s = (h - (2 * np.arange(h) + 1)) / h * float(spec.tan_half_v)
    return F[None, None, :] + u[None, :, None] * L[None, None, :] + s[:, None, None] * U[None, None, :]


def _near_segment(oc, a, D, dn, radius):
    """Where the ray's line passes within BAND of the distance `radius` from the segment oc .. oc + a (relative to the eye), at a place
    of the segment's line within its ends (widened by the radius and BAND) and ahead of the eye: a silhouette of a cylinder, an edge of a
    box (radius 0)."""
    la = np.linalg.norm(a)
    ah = a / la
    m = np.cross(D, ah)
    mm = (m * m).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.abs((m * oc).sum(-1)) / np.sqrt(mm)          # the distance between the two lines
        n = np.cross(oc, ah)
        t = (m * n).sum(-1) / mm                             # the ray's parameter at its closest approach
        s = t * (D * ah).sum(-1) - oc @ ah                   # the place along the segment there
        return (np.abs(w - radius) < BAND) & (s > -radius - BAND) & (s < la + radius + BAND) & (t * dn > -radius - BAND)


def reference(cfg, st, items, aux, spec):
    """(depth [H, W] f64, seg [H, W] int, exempt [H, W] bool) of one env in fp64.  exempt: some comparison the reference made is within
    BAND of changing: a silhouette (the lateral miss distance of a ground plan, a sphere, a cylinder, an edge of the cube), a seam
    between a cylinder and the neighbouring link's ball, the ray's height at a ground plan's entry against either end of the z-interval,
    a top or bottom point against the ground plan's exit, a tile line, a candidate against max_range, the eye against a solid's surface
    (containment) or the ground, and the winner against a runner-up of another seg that is not exactly tied with it."""
    h, w = spec.height, spec.width
    rmax = float(spec.max_range)
    seg0 = np.zeros((h, w), np.int64)
    exempt = np.zeros((h, w), bool)
    st = np.asarray(st, float)
    E, F, L, U = camera_of(cfg, st, spec)
    if not (np.isfinite(E).all() and np.isfinite(st[0:3] if spec.target_mode == Ch.HRL_EYE_TORSO else st[0:2]).all()):
        return np.full((h, w), rmax), seg0, exempt
    D = rays(spec, F, L, U)
    dx, dy, dz = D[..., 0], D[..., 1], D[..., 2]
    dn = np.sqrt((D * D).sum(-1))
    c = np.sqrt(dx * dx + dy * dy)   # horizontal metres per unit of lam
    with np.errstate(divide='ignore', invalid='ignore'):
        ux, uy = dx / c, dy / c
    flat = c > 0
    cands = []   # (lam [H, W] with inf where there is none, seg [H, W])

    def offer(lam, seg, ok):
        nonlocal exempt
        with np.errstate(invalid='ignore'):
            exempt |= ok & ((np.abs(lam - rmax) * dn < BAND) | (np.abs(lam) * dn < BAND))
            ok = ok & (lam > 0) & (lam <= rmax)
        cands.append((np.where(ok, lam, np.inf), np.broadcast_to(np.asarray(seg, np.int64), (h, w))))

    for cls, code, typ, p in sc.shapes(cfg, items, aux):
        if not spec.classes & cls or not np.isfinite([x for part in p for x in np.ravel(part)]).all():
            continue
        zl, zh = cc.z_interval(cfg, cls)
        with np.errstate(divide='ignore', invalid='ignore'):
            if typ == 'half':   # the solid beyond the bounding line: n . p + off <= 0
                (nx, ny), off0 = p
                off, den = nx * E[0] + ny * E[1] + off0, nx * dx + ny * dy
                over, sd = off < 0, abs(off)
                if over:
                    l0, l1 = np.full((h, w), -np.inf), np.full((h, w), np.inf)
                else:
                    l0, l1 = np.where(den < 0, off / -np.where(den < 0, den, -1.0), np.inf), np.full((h, w), np.inf)
                side = np.full((h, w), Ch.FACE_SIDE_X if abs(nx) >= abs(ny) else Ch.FACE_SIDE_Y)
            elif typ == 'rect':
                (cx, cy), (hx, hy) = p
                x0, x1 = cc._axis(cx - hx, cx + hx, E[0], dx)
                y0, y1 = cc._axis(cy - hy, cy + hy, E[1], dy)
                l0, l1 = np.maximum(x0, y0), np.minimum(x1, y1)
                side = np.where(x0 >= y0, Ch.FACE_SIDE_X, Ch.FACE_SIDE_Y)
                for sx in (-1, 1):   # the verdict of the ground plan changes where the ray's line passes a corner that lies ahead
                    for sy in (-1, 1):
                        qx, qy = cx + sx * hx - E[0], cy + sy * hy - E[1]
                        exempt |= flat & (np.abs(qx * uy - qy * ux) < BAND) & (qx * ux + qy * uy > -BAND)
                sdr = rc._sd_rect(E[0], E[1], (cx, cy), hx, hy)
                over, sd = sdr <= 0, abs(sdr)
            else:
                (cx, cy), r = p
                qx, qy = cx - E[0], cy - E[1]
                b, e = (qx * dx + qy * dy) / (c * c), (qx * uy - qy * ux)   # lam of the closest approach; the centre's distance from the line
                hh = r * r - e * e
                root = np.sqrt(np.maximum(hh, 0.0)) / c
                l0, l1 = np.where(hh >= 0, b - root, np.inf), np.where(hh >= 0, b + root, -np.inf)
                dist = np.hypot(qx, qy)
                over, sd = dist <= r, abs(dist - r)
                if over:   # (a vertical ray stays over the disc)
                    l0, l1 = np.where(flat, l0, -np.inf), np.where(flat, l1, np.inf)
                else:
                    l0, l1 = np.where(flat, l0, np.inf), np.where(flat, l1, -np.inf)
                side = np.full((h, w), Ch.FACE_ROUND)
                exempt |= flat & (np.abs(np.abs(e) - r) < BAND) & (b * c > -r - BAND)
            # containment: the eye against the solid's surface
            if (sd < BAND and zl - BAND <= E[2] <= zh + BAND) or ((over or sd < BAND) and (abs(E[2] - zl) < BAND or abs(E[2] - zh) < BAND)):
                exempt |= True
            if over and zl <= E[2] <= zh:
                continue   # the solid contains the eye: not drawn at all
            z0, z1 = cc._axis(zl, zh, E[2], dz)
            enter, leave = np.maximum(l0, z0), np.minimum(l1, z1)
            hit = (enter <= leave) & (enter > 0)
            face = np.where(l0 >= z0, side, np.where(dz < 0, Ch.FACE_TOP, Ch.FACE_BOTTOM))
            a = np.maximum(l0, 0.0)
            span = (l0 <= l1) & (l1 >= 0)
            za = E[2] + dz * a
            exempt |= span & np.isfinite(za) & ((np.abs(za - zl) < BAND) | (np.abs(za - zh) < BAND))
            exempt |= span & np.isfinite(z0) & np.isfinite(l1) & (np.abs((z0 - l1) * c) < BAND) & (z0 >= 0)
            exempt |= hit & np.isfinite(l0) & np.isfinite(z0) & (np.abs((l0 - z0) * dn) < BAND)
        offer(enter, code | (face << 16), hit)

    if spec.classes & Ch.ROBOT:
        O = st[0:3]
        with np.errstate(divide='ignore', invalid='ignore'):
            if cfg.env_kind == K.HRL_POINT_GATHER:
                R = rc._rot(st[3:7])
                if np.isfinite(R).all() and np.isfinite(O).all():
                    ob, db = (E - O) @ R, D @ R   # the ray in body axes
                    lo, hi = [], []
                    for k in range(3):
                        a0, a1 = cc._axis(-POINT_HALF, POINT_HALF, ob[k], db[..., k])
                        lo.append(a0); hi.append(a1)
                    tn, tf = np.maximum(np.maximum(lo[0], lo[1]), lo[2]), np.minimum(np.minimum(hi[0], hi[1]), hi[2])
                    face = np.where((lo[0] >= lo[1]) & (lo[0] >= lo[2]), Ch.FACE_SIDE_X, np.where(lo[1] >= lo[2], Ch.FACE_SIDE_Y, np.where(db[..., 2] < 0, Ch.FACE_TOP, Ch.FACE_BOTTOM)))
                    for k in range(3):   # the 12 edges: silhouettes and the lines between two faces
                        for s1 in (-1, 1):
                            for s2 in (-1, 1):
                                corner = np.zeros(3)
                                corner[k], corner[(k + 1) % 3], corner[(k + 2) % 3] = -POINT_HALF, s1 * POINT_HALF, s2 * POINT_HALF
                                exempt |= _near_segment(O + R @ corner - E, R[:, k] * 2 * POINT_HALF, D, dn, 0.0)
                    if np.abs(np.abs(ob) - POINT_HALF).min() < BAND and (np.abs(ob) < POINT_HALF + BAND).all():
                        exempt |= True
                    offer(tn, Ch.HIT_ROBOT | (face << 16), (tn <= tf) & (tn > 0))
            else:
                def sphere(link, centre, r):
                    nonlocal exempt
                    if not np.isfinite(centre).all():
                        return
                    oc = centre - E
                    b = (D * oc).sum(-1) / dn
                    pp = np.sqrt((np.cross(oc, D) ** 2).sum(-1)) / dn   # the centre's distance from the ray's line
                    exempt |= (np.abs(pp - r) < BAND) & (b > -r - BAND)
                    if abs(np.linalg.norm(oc) - r) < BAND:
                        exempt |= True
                    lam = (b - np.sqrt(np.maximum(r * r - pp * pp, 0.0))) / dn
                    offer(lam, Ch.HIT_ROBOT | (link << 8) | (Ch.FACE_ROUND << 16), pp <= r)

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
                        exempt |= _near_segment(oc, a, D, dn, R_CAPS)
                        exempt |= (hh >= 0) & (lam > 0) & ((np.abs(s) < BAND) | (np.abs(s - la) < BAND))   # the seams at the cylinder's ends
                        offer(lam, Ch.HIT_ROBOT | (link << 8) | (Ch.FACE_ROUND << 16), (hh >= 0) & (s >= 0) & (s <= la))
                    sphere(link, p1, R_CAPS)

    if spec.classes & Ch.GROUND:
        gz = ground_z(cfg)
        if E[2] > gz:
            with np.errstate(divide='ignore', invalid='ignore'):
                lam = np.where(dz < 0, (gz - E[2]) / np.where(dz < 0, dz, -1.0), np.inf)
                parity = np.zeros((h, w), np.int64)
                tile = float(spec.tile)
                if tile > 0:
                    qx, qy = (E[0] + lam * dx) / tile, (E[1] + lam * dy) / tile
                    ok = np.isfinite(qx) & np.isfinite(qy)
                    qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
                    parity = (np.floor(qx) + np.floor(qy)).astype(np.int64) & 1
                    exempt |= (dz < 0) & ok & ((np.abs(qx - np.rint(qx)) * tile < BAND) | (np.abs(qy - np.rint(qy)) * tile < BAND))
            offer(lam, Ch.HIT_GROUND | (parity << 8) | (Ch.FACE_GROUND << 16), dz < 0)
        if abs(E[2] - gz) < BAND:
            exempt |= True

    if not cands:
        return np.full((h, w), rmax), seg0, exempt
    lams, segs = np.stack([x for x, _ in cands]), np.stack([x for _, x in cands])
    first = np.argmin(lams, axis=0)   # the first of equal ones: the earlier candidate wins a tie
    best = np.take_along_axis(lams, first[None], 0)[0]
    seg = np.where(np.isfinite(best), np.take_along_axis(segs, first[None], 0)[0], 0)
    with np.errstate(invalid='ignore'):   # (an exact tie is no near-tie: the tie rule decides it in any precision)
        exempt |= (((lams - best[None]) * dn[None] < BAND) & (lams > best[None]) & (segs != seg[None])).any(0)
    return np.where(seg != 0, best, rmax), seg, exempt


def colour_of(seg):
    """rgb [..., 3] uint8 of a seg array, from the header: the class or link colour * shade[face] >> 8, the ground of parity 1 * 208 >> 8,
    the sky where nothing was hit."""
    seg = np.asarray(seg, np.int64)
    out = np.empty(seg.shape + (3,), np.uint8)
    out[...] = Ch.RGB_SKY
    cls, index, face = seg & 255, (seg >> 8) & 255, seg >> 16
    shades = np.asarray(Ch.SHADES)
    for kind, col in COLOURS.items():
        sel = cls == kind
        for k in range(3):
            v = (col[k] * shades[face[sel]]) >> 8
            if kind == Ch.HIT_GROUND:
                v = np.where(index[sel] & 1, (v * Ch.TILE_SHADE) >> 8, v)
            out[..., k][sel] = v
    sel = cls == Ch.HIT_ROBOT
    cols = np.asarray(LINK_COLOURS)[np.minimum(index[sel], 12)]
    for k in range(3):
        out[..., k][sel] = (cols[:, k] * shades[face[sel]]) >> 8
    return out


# ------------------------------------------------------------------------------------------------ states
hostile = cc.hostile
spread = cc.spread
far_targets = cc.far_targets
