"""Shared by tests/test_dyn_host.py, tests/test_dyn_launch.py and tests/test_gpu_dyn.py: the ctypes binding of
tests/dyn_host/libdyn_host.so (the host build of csrc/dyn_core.h), an independent fp64 numpy reference written from include/hrl_dyn.h
alone (per-body Jacobians of the nine rigid bodies, M = sum J^T diag(m, I) J, Newton-Euler bias forces from the classical accelerations at
udot = 0, a dense solve), and the states and models the tests use.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import links_cases as lc
import orc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import dyn_device as Dy

ROOT = lc.ROOT
DIR = os.path.join(ROOT, 'tests', 'dyn_host')
KINDS = lc.KINDS
ANTS = tuple(k for k in KINDS if k != K.HRL_POINT_GATHER)
NAMES = Dy.Dynamics._fields
Dynamics = collections.namedtuple('Dynamics', NAMES)   # of numpy arrays
Dynamics.__new__.__defaults__ = (None,) * 7
# what the feature reads of the model (the sensor config matrix varies arenas, which it does not read)
MODELS = collections.OrderedDict([
    ('defaults', {}),
    ('no-body-damping', dict(linear_damping=0.0, angular_damping=0.0)),
    ('joint-damping-and-armature', dict(joint_damping=1.0, joint_armature=0.01)),   # assets/ant.xml:8
    ('density-500', dict(density=500.0)),
    ('gravity-3.7', dict(gravity=3.7)),
])
_lib = None
ptr = lc.ptr
bits = lc.bits
same = lc.same


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libdyn_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libdyn_host.so'))
        L.dyn_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(Dy.hrl_dyn_spec), C.c_void_p, C.c_void_p, C.POINTER(Dy.hrl_dyn_out)]
        L.dyn_host_last_error.restype = C.c_char_p
        L.dyn_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.POINTER(Dy.hrl_dyn_spec)]
        L.dyn_host_nv.argtypes = [C.c_int32]
        L.dyn_sizeof_spec.restype = C.c_ulonglong
        L.dyn_sizeof_out.restype = C.c_ulonglong
        L.dyn_validate_spec.argtypes, L.dyn_validate_spec.restype = [C.POINTER(K.hrl_config), C.POINTER(Dy.hrl_dyn_spec)], C.c_char_p
        L.dyn_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'dyn_check_main'])
    return os.path.join(DIR, 'dyn_check_main')


def spec_of(sites=()):
    """A spec with the given sites ((link, (x, y, z)), ...), built field by field (no library call)."""
    s = Dy.hrl_dyn_spec(frame=Dy.HRL_DYN_WORLD, n_sites=len(sites))
    for i, (link, local) in enumerate(sites):
        s.site_link[i] = link
        s.site_local[i][0], s.site_local[i][1], s.site_local[i][2] = local
    return s


def config_of(cfg, n=None, **model):
    """A copy of cfg for n envs (None: as many as it has) with fields of its model replaced."""
    c = lc.config_of(cfg, cfg.num_envs if n is None else n)
    for k, v in model.items():
        setattr(c.model, k, v)
    return c


def shapes_of(cfg, n, spec):
    return Dy.shapes(cfg, Dy.hrl_dyn_spec(n_sites=min(max(spec.n_sites, 0), 16)), (n,))


def dyn_host(cfg, state, spec, tau=None, mask=None, out=None, want=NAMES, expect_ok=True):
    """The host build's dynamics terms of state [N, 32] f32: a Dynamics of arrays; the members not in `want` are None.  `out`: a Dynamics
    of arrays (None members are passed as NULL) to write into."""
    state = np.ascontiguousarray(state, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE)
    aux = np.zeros((n, K.HRL_AUX_STRIDE), np.int32)
    if out is None:
        out = Dynamics(*(np.zeros(shape, np.float32) if name in want and 0 not in shape[1:] else None for name, shape in zip(NAMES, shapes_of(cfg, n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    t = None if tau is None else np.ascontiguousarray(tau, np.float32)
    assert t is None or t.shape == (n, Dy.nv(cfg))
    b = K.make_buffers(ptr(state), None, ptr(aux), None, None, None, None, None)
    o = Dy.hrl_dyn_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().dyn_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(t), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().dyn_host_last_error()
        return out
    return code, lib().dyn_host_last_error().decode()


# ------------------------------------------------------------------------------------------------ the fp64 reference, from the header
def model_constants(cfg):
    """(m, alpha, beta) of the torso body, an upper body and a foot in fp64, as include/hrl_dyn.h names them, from the solids of
    assets/ant.xml:12-58 at the model's density: a sphere of radius 0.25, capsules of radius 0.08 and lengths |(0.2, 0.2)| and
    |(0.4, 0.4)| (a cylinder and two half spheres); the torso body carries the four hip capsules, centred 0.1 sqrt 2 from O in its
    xy plane.  Checked against the oracle's table (fp32 constants) to 1e-6."""
    rho, rt, rc = float(cfg.model.density), 0.25, 0.08
    msph = rho * 4 / 3 * np.pi * rt ** 3
    caps = []
    for L in (0.2 * np.sqrt(2.0), 0.4 * np.sqrt(2.0)):
        mc, ms = rho * np.pi * rc * rc * L, rho * 4 / 3 * np.pi * rc ** 3
        axial = mc * rc * rc / 2 + ms * 0.4 * rc * rc
        trans = mc * (L * L / 12 + rc * rc / 4) + ms * (0.4 * rc * rc + L * L / 4 + 3 * L * rc / 8)
        caps.append((mc + ms, trans, axial - trans))
    m1, t1, d1 = caps[0]
    # four capsules along (+-1, +-1, 0) / sqrt 2 at distance cl: their axial parts sum to 2 d1 (1 - z z^T), their offsets to m1 cl^2 (2 + 2 z z^T)
    cl = 0.1 * np.sqrt(2.0)
    alpha0 = 0.4 * msph * rt * rt + 4 * t1 + 2 * d1 + 2 * m1 * cl * cl
    beta0 = -2 * d1 + 2 * m1 * cl * cl
    table = np.array([(msph + 4 * m1, alpha0, beta0), caps[0], caps[1]])
    out = np.zeros(29)
    orc.lib().orc_model_constants_f64(C.byref(cfg.model), orc.ptr(out))
    assert np.abs(table - out[4:13].reshape(3, 3)).max() <= 1e-6 * np.abs(table).max()
    return table


def cross_matrix(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0.0]])


def bodies_of(cfg, st):
    """The rigid bodies of one env in fp64, each a dict: m, I (world axes, central), c (the centre of mass relative to O), w, v (of the
    centre of mass), alpha0, a0 (the classical accelerations at udot = 0), Jw, Jv [3, nv] (generalised order v, omega, rates)."""
    st = np.asarray(st, np.float64)
    R0, v0, w0 = lc.rot_of_quat(st[3:7]), st[15:18], st[18:21]
    if cfg.env_kind == K.HRL_POINT_GATHER:
        Jw, Jv = np.zeros((3, 6)), np.zeros((3, 6))
        Jv[:, 0:3], Jw[:, 3:6] = np.eye(3), np.eye(3)
        return [dict(m=10.0, I=np.eye(3) * (10.0 * 0.7 * 0.7 / 6.0), c=np.zeros(3), w=w0, v=v0, alpha0=np.zeros(3), a0=np.zeros(3), Jw=Jw, Jv=Jv)]
    (m0, al0, be0), (m1, al1, be1), (m2, al2, be2) = model_constants(cfg)

    def body(m, al, be, e, c, w, v, alpha0, a0, cols):
        Jw, Jv = np.zeros((3, 14)), np.zeros((3, 14))
        Jv[:, 0:3], Jw[:, 3:6], Jv[:, 3:6] = np.eye(3), np.eye(3), -cross_matrix(c)
        for j, axis, anchor in cols:
            Jw[:, 6 + j], Jv[:, 6 + j] = axis, np.cross(axis, c - anchor)
        return dict(m=m, I=al * np.eye(3) + be * np.outer(e, e), c=c, w=w, v=v, alpha0=alpha0, a0=a0, Jw=Jw, Jv=Jv)

    out = [body(m0, al0, be0, R0[:, 2], np.zeros(3), w0, v0, np.zeros(3), np.zeros(3), ())]
    for l in range(4):
        d = np.array([lc.LEG_DIR[l][0], lc.LEG_DIR[l][1], 0.0])
        qh, qa, dqh, dqa = st[7 + 2 * l], st[8 + 2 * l], st[21 + 2 * l], st[22 + 2 * l]
        Raux = R0 @ lc.rodrigues((0, 0, 1), qh)
        aloc = np.array([lc.ANKLE_AXIS[l][0], lc.ANKLE_AXIS[l][1], 0.0]) / np.sqrt(2.0)
        Rfoot = Raux @ lc.rodrigues(aloc, qa)
        ph = R0 @ (0.2 * d)
        pa = ph + Raux @ (0.2 * d)
        cx, cf = ph + Raux @ (0.1 * d), pa + Rfoot @ (0.2 * d)
        zh, za = R0[:, 2], Raux @ aloc
        w1 = w0 + zh * dqh
        w2 = w1 + za * dqa
        al_1 = np.cross(w0, zh) * dqh
        al_2 = al_1 + np.cross(w1, za) * dqa
        v_h = v0 + np.cross(w0, ph)
        a_h = np.cross(w0, np.cross(w0, ph))
        v_a = v_h + np.cross(w1, pa - ph)
        a_a = a_h + np.cross(al_1, pa - ph) + np.cross(w1, np.cross(w1, pa - ph))
        out.append(body(m1, al1, be1, Raux @ d / np.sqrt(2.0), cx, w1, v_h + np.cross(w1, cx - ph), al_1, a_h + np.cross(al_1, cx - ph) + np.cross(w1, np.cross(w1, cx - ph)),
                        ((2 * l, zh, ph),)))
        out.append(body(m2, al2, be2, Rfoot @ d / np.sqrt(2.0), cf, w2, v_a + np.cross(w2, cf - pa), al_2, a_a + np.cross(al_2, cf - pa) + np.cross(w2, np.cross(w2, cf - pa)),
                        ((2 * l, zh, ph), (2 * l + 1, za, pa))))
    return out


def reference(cfg, st, sites=(), tau=None):
    """One env in fp64: a dict of mass [nv, nv], bias, accel [nv], jac [S, 3, nv], com [3], momentum [6], energy [2]."""
    st = np.asarray(st, np.float64)
    m = cfg.model
    nv = Dy.nv(cfg)
    u = st[15:15 + nv]
    B = bodies_of(cfg, st)
    M, bias = np.zeros((nv, nv)), np.zeros(nv)
    g = np.array([0.0, 0.0, float(m.gravity)])
    for b in B:
        M += b['m'] * b['Jv'].T @ b['Jv'] + b['Jw'].T @ b['I'] @ b['Jw']
        Iw = b['I'] @ b['w']
        f = b['m'] * (b['a0'] + g) + b['m'] * b['v'] * float(m.linear_damping) * (1 + np.linalg.norm(b['v']))
        n = b['I'] @ b['alpha0'] + np.cross(b['w'], Iw) + Iw * float(m.angular_damping) * (1 + np.linalg.norm(b['w']))
        bias += b['Jv'].T @ f + b['Jw'].T @ n
    M[6:, 6:] += np.eye(nv - 6) * float(m.joint_armature)
    bias[6:] += float(m.joint_damping) * u[6:]
    t = np.zeros(nv) if tau is None else np.asarray(tau, np.float64)
    mt = sum(b['m'] for b in B)
    rG = sum(b['m'] * b['c'] for b in B) / mt
    P = sum(b['m'] * b['v'] for b in B)
    LG = sum(np.cross(b['c'] - rG, b['m'] * b['v']) + b['I'] @ b['w'] for b in B)
    T = sum(0.5 * b['m'] * b['v'] @ b['v'] + 0.5 * b['w'] @ b['I'] @ b['w'] for b in B)
    com = st[0:3] + rG
    # the sites: a point fixed to a link of hrl_links.h
    R0 = lc.rot_of_quat(st[3:7])
    jac = np.zeros((len(sites), 3, nv))
    link = lc.reference(cfg.env_kind, st, 0, sites) if sites else None
    for s, (k, loc) in enumerate(sites):
        p = link['site_pos'][s] - st[0:3]
        jac[s, :, 0:3], jac[s, :, 3:6] = np.eye(3), -cross_matrix(p)
        if nv == 14 and 1 <= k <= 8:
            l = (k - 1) // 2
            ph = link['origin'][1 + 2 * l] - st[0:3]
            jac[s, :, 6 + 2 * l] = np.cross(R0[:, 2], p - ph)
            if k % 2 == 0:
                pa = link['origin'][2 + 2 * l] - st[0:3]
                za = link['R'][1 + 2 * l] @ (np.array([lc.ANKLE_AXIS[l][0], lc.ANKLE_AXIS[l][1], 0.0]) / np.sqrt(2.0))
                jac[s, :, 7 + 2 * l] = np.cross(za, p - pa)
    return dict(mass=M, bias=bias, accel=np.linalg.solve(M, t - bias), jac=jac, com=com, momentum=np.concatenate([P, LG]), energy=np.array([T, mt * float(m.gravity) * com[2]]))


# ------------------------------------------------------------------------------------------------ the textbook's order
TB = np.r_[3:6, 0:3, 6:14]   # generalised (v, omega, rates) <-> the textbook's (omega, v, rates): the permutation is its own inverse


def tb_state(st):
    """(q [15], u [14] in the textbook's order) of a state record, fp64."""
    st = np.asarray(st, np.float64)
    return st[:15].copy(), st[15:29][TB].copy()


# ------------------------------------------------------------------------------------------------ states
def hand_made(seed=3, n=12, unit=True):
    """links_cases.hand_made poses (tilted torsos, joints at both stops, |x|, |y| up to 10 m) with velocities of the shards' scale: the
    shards' ants move at up to a few m/s and turn their joints at tens of rad/s."""
    st = np.array(lc.hand_made(seed, n, unit=unit))
    st[:, 15:21] *= np.float32(1.5)
    st[:, 21:29] *= np.float32(3.0)
    return st


def state_sets(kind, state):
    """(label, states, unit quaternions) of a kind: its shard, and for the ants the hand-made poses."""
    sets = [('shard', np.asarray(state), True)]
    if kind != K.HRL_POINT_GATHER:
        sets += [('hand-made', hand_made(), True), ('non-unit', hand_made(4, unit=False), False)]
    return sets


def speed_scale(st):
    """1 + the largest speed of a state's bodies, roughly (test_links_host.scale_of): |v| + 1.2 m * (|omega| + the fastest hip + the
    fastest ankle)."""
    return 1.0 + np.linalg.norm(st[15:18]) + 1.2 * (np.linalg.norm(st[18:21]) + np.abs(st[21:29:2]).max() + np.abs(st[22:29:2]).max())


def taus(cfg, n, seed=9):
    """An applied force per env of the step's scale: joint torques up to torque_scale and, unlike the step, a wrench on the base too."""
    rng = np.random.RandomState(seed)
    nv = Dy.nv(cfg)
    t = rng.uniform(-1, 1, (n, nv)) * float(cfg.model.torque_scale if nv == 14 else cfg.model.point_force)
    return t.astype(np.float32)
