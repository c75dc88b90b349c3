"""Shared by tests/test_links_host.py, tests/test_gpu_links.py and tests/test_gpu_links_scale.py: the ctypes binding of
tests/links_host/liblinks_host.so (the host build of csrc/links_core.h), an independent fp64 numpy reference written from
include/hrl_links.h alone (rotation matrices, Rodrigues rotations about the MJCF axes, velocities from omega x r and the joint rates), and
the states and specs the tests use.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import render_cases as rc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import links_device as Lk

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'links_host')
KINDS = rc.KINDS
FRAMES = (Lk.HRL_LINKS_WORLD, Lk.HRL_LINKS_HEADING)
NAMES = Lk.Links._fields
WIDTHS = (3, 3, 4, 3, 3, 3, 3)
Links = collections.namedtuple('Links', NAMES)   # of numpy arrays
Links.__new__.__defaults__ = (None,) * 7
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'liblinks_host.so'])
        L = C.CDLL(os.path.join(DIR, 'liblinks_host.so'))
        L.links_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(Lk.hrl_links_spec), C.c_void_p, C.POINTER(Lk.hrl_links_out)]
        L.links_host_last_error.restype = C.c_char_p
        L.links_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(Lk.hrl_links_spec)]
        L.links_host_name.argtypes, L.links_host_name.restype = [C.c_int32, C.c_int32], C.c_char_p
        L.links_sizeof_spec.restype = C.c_ulonglong
        L.links_sizeof_out.restype = C.c_ulonglong
        L.links_validate_spec.argtypes, L.links_validate_spec.restype = [C.POINTER(K.hrl_config), C.POINTER(Lk.hrl_links_spec)], C.c_char_p
        L.links_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        L.links_quat_axes.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'links_check_main'])
    return os.path.join(DIR, 'links_check_main')


ptr = rc.ptr


def spec_of(frame=Lk.HRL_LINKS_WORLD, sites=()):
    """A spec with the given sites ((link, (x, y, z)), ...), built field by field (no library call)."""
    s = Lk.hrl_links_spec(frame=frame, n_sites=len(sites))
    for i, (link, local) in enumerate(sites):
        s.site_link[i] = link
        s.site_local[i][0], s.site_local[i][1], s.site_local[i][2] = local
    return s


def foot_sites():
    """The library's default sites of the ants, spelled out: the far end of every foot capsule's fromto."""
    return tuple((2 + 2 * l, (0.4 * LEG_DIR[l][0], 0.4 * LEG_DIR[l][1], 0.0)) for l in range(4))


def sixteen_sites(b):
    """16 sites over every link of a robot of b links, at offsets that are no round numbers."""
    rng = np.random.RandomState(5)
    return tuple((i % b, tuple(float(np.float32(v)) for v in rng.uniform(-0.5, 0.5, 3))) for i in range(16))


def shapes_of(cfg, n, spec):
    b, s = Lk.n_links(cfg), min(max(spec.n_sites, 0), 16)
    return tuple((n, s if name.startswith('site') else b, w) for name, w in zip(NAMES, WIDTHS))


def links_host(cfg, state, spec, mask=None, out=None, want=NAMES, expect_ok=True, aux=None):
    """The host build's link states of state [N, 32] f32: a Links of arrays; the members not in `want` are None.  `out`: a Links of
    arrays (None members are passed as NULL) to write into."""
    state = np.ascontiguousarray(state, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE)
    aux = np.zeros((n, K.HRL_AUX_STRIDE), np.int32) if aux is None else np.ascontiguousarray(aux, np.int32)
    if out is None:
        out = Links(*(np.zeros(shape, np.float32) if name in want and shape[1] else None for name, shape in zip(NAMES, shapes_of(cfg, n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), None, ptr(aux), None, None, None, None, None)
    o = Lk.hrl_links_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().links_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().links_host_last_error()
        return out
    return code, lib().links_host_last_error().decode()


def bits(x):
    return None if x is None else np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(a, b, nan_ok=False):
    """Every member the same bits (nan_ok: or NaN in both -- the payload of a NaN is the processor's own)."""
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return False
        if x is None:
            continue
        eq = bits(x) == bits(y)
        if nan_ok:
            eq |= np.isnan(x) & np.isnan(y)
        if not eq.all():
            return False
    return True


def quat_axes_f32(q):
    """The rotation matrices [..., 3, 3] that fp32 quaternions [..., 4] stand for, by the step's quat_axes (the host build's)."""
    q = np.ascontiguousarray(q, np.float32)
    flat = q.reshape(-1, 4)
    out = np.zeros((flat.shape[0], 9), np.float32)
    for i in range(flat.shape[0]):
        lib().links_quat_axes(ptr(flat[i]), ptr(out[i]))
    return out.reshape(q.shape[:-1] + (3, 3)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the fp64 reference, from the header
LEG_DIR = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))       # assets/ant.xml:15-58: the legs' fromto directions
ANKLE_AXIS = ((-1.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, 1.0))      # the ankle joints' axes
LENGTHS = (0.2 * np.sqrt(2.0), 0.2 * np.sqrt(2.0), 0.4 * np.sqrt(2.0))   # hip capsule, aux, foot


def rot_of_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rodrigues(axis, th):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def fromto(link):
    """The local fromto vector of a link's capsule (zero for the torso and the cube)."""
    if link == 0:
        return np.zeros(3)
    l, scale = (link - 9, 0.2) if link >= 9 else ((link - 1) // 2, 0.2 if link % 2 else 0.4)
    return np.array([scale * LEG_DIR[l][0], scale * LEG_DIR[l][1], 0.0])


def yaw_matrix(R0):
    """Rotation by minus the heading: the heading is the ground projection of the torso's X axis (world +x when there is none)."""
    f = np.array([R0[0, 0], R0[1, 0]])
    n2 = f @ f
    f = f / np.sqrt(n2) if np.isfinite(n2) and n2 >= 1e-12 else np.array([1.0, 0.0])
    return np.array([[f[0], f[1], 0.0], [-f[1], f[0], 0.0], [0.0, 0.0, 1.0]])


def reference(kind, st, frame=Lk.HRL_LINKS_WORLD, sites=()):
    """One env in fp64: a dict of origin, com, lin_vel, ang_vel [B, 3], R [B, 3, 3] (the body frames as rotation matrices), far [B, 3] (the
    capsules' far ends), site_pos, site_vel [S, 3]."""
    st = np.asarray(st, np.float64)
    O, q, v0, w0 = st[0:3], st[3:7], st[15:18], st[18:21]
    R0 = rot_of_quat(q)
    b = 1 if kind == K.HRL_POINT_GATHER else 13
    origin, far, R = np.zeros((b, 3)), np.zeros((b, 3)), np.zeros((b, 3, 3))
    w, vo = np.zeros((b, 3)), np.zeros((b, 3))   # angular velocity; velocity of the link's origin
    origin[0], far[0], R[0], w[0], vo[0] = O, O, R0, w0, v0
    if b > 1:
        for l in range(4):
            d = np.array([LEG_DIR[l][0], LEG_DIR[l][1], 0.0])
            qh, qa, dqh, dqa = st[7 + 2 * l], st[8 + 2 * l], st[21 + 2 * l], st[22 + 2 * l]
            Raux = R0 @ rodrigues((0, 0, 1), qh)
            aloc = np.array([ANKLE_AXIS[l][0], ANKLE_AXIS[l][1], 0.0]) / np.sqrt(2.0)
            Rfoot = Raux @ rodrigues(aloc, qa)
            ph = O + R0 @ (0.2 * d)
            pa = ph + Raux @ (0.2 * d)
            tip = pa + Rfoot @ (0.4 * d)
            w1 = w0 + (R0 @ np.array([0.0, 0.0, 1.0])) * dqh
            w2 = w1 + (Raux @ aloc) * dqa
            v_ph = v0 + np.cross(w0, ph - O)
            v_pa = v_ph + np.cross(w1, pa - ph)
            for link, o_, f_, R_, w_, v_ in ((9 + l, O, ph, R0, w0, v0), (1 + 2 * l, ph, pa, Raux, w1, v_ph), (2 + 2 * l, pa, tip, Rfoot, w2, v_pa)):
                origin[link], far[link], R[link], w[link], vo[link] = o_, f_, R_, w_, v_
    com = 0.5 * (origin + far)
    lin = vo + np.cross(w, com - origin)
    sp = np.array([origin[k] + R[k] @ np.asarray(loc, float) for k, loc in sites]).reshape(-1, 3)
    sv = np.array([vo[k] + np.cross(w[k], R[k] @ np.asarray(loc, float)) for k, loc in sites]).reshape(-1, 3)
    out = dict(origin=origin, com=com, far=far, R=R, lin_vel=lin, ang_vel=w, site_pos=sp, site_vel=sv)
    if frame == Lk.HRL_LINKS_HEADING:
        T = yaw_matrix(R0)
        for k in ('origin', 'com', 'far', 'site_pos'):
            out[k] = (out[k] - O) @ T.T
        for k in ('lin_vel', 'ang_vel', 'site_vel'):
            out[k] = out[k] @ T.T
        out['R'] = np.einsum('ij,bjk->bik', T, R)
    return out


def quat_exp(w, h):
    """The unit quaternion (x, y, z, w) of the rotation by |w| h about w."""
    th = np.linalg.norm(w) * h
    if th == 0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(th / 2) * np.asarray(w) / np.linalg.norm(w), [np.cos(th / 2)]])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def advance(st, h):
    """The fp64 pose integration of a state over h seconds at its velocities: x + h v, exp(h omega / 2) * q (omega in world axes), joint
    angles + h * rates."""
    s = np.array(st, np.float64)
    s[0:3] += h * s[15:18]
    s[3:7] = quat_mul(quat_exp(s[18:21], h), s[3:7])
    s[7:15] += h * s[21:29]
    return s


# ------------------------------------------------------------------------------------------------ states
JOINT_LO = np.deg2rad([-40.0, 30, -40, -100, -40, -100, -40, 30])
JOINT_HI = np.deg2rad([40.0, 100, 40, -30, 40, -30, 40, 100])


def hand_made(seed=3, n=12, reach=10.0, unit=True):
    """States [n, 32] f32 with tilted torsos, the joints at either stop or anywhere between, x and y up to +-reach and velocities of a few
    m/s and rad/s.  unit: the quaternion is normalised in fp64 and rounded once; else it is left up to 1 % off the unit length."""
    rng = np.random.RandomState(seed)
    st = np.zeros((n, K.HRL_STATE_STRIDE))
    st[:, 0:2] = rng.uniform(-reach, reach, (n, 2))
    st[0, 0:2], st[1, 0:2] = (reach, -reach), (-reach, reach)
    st[:, 2] = rng.uniform(0.3, 1.2, n)
    q = rng.normal(size=(n, 4))
    q[2] = (0, 0, 0, 1)
    q[3] = (0, 0, 1, 0)       # a heading of pi: the half-angle formulas' other side
    q[4] = (0, 0, np.sin(-1.5), np.cos(-1.5))
    q /= np.linalg.norm(q, axis=1)[:, None]
    st[:, 3:7] = q if unit else q * rng.uniform(0.99, 1.01, (n, 1))
    pick = rng.randint(0, 3, (n, 8))
    st[:, 7:15] = np.where(pick == 0, JOINT_LO, np.where(pick == 1, JOINT_HI, rng.uniform(JOINT_LO, JOINT_HI, (n, 8))))
    st[:, 15:18] = rng.uniform(-3, 3, (n, 3))
    st[:, 18:21] = rng.uniform(-4, 4, (n, 3))
    st[:, 21:29] = rng.uniform(-8, 8, (n, 8))
    return st.astype(np.float32)


def config_of(cfg, n):
    """A copy of cfg for n envs."""
    c = K.hrl_config()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(K.hrl_config))
    c.num_envs = n
    return c
