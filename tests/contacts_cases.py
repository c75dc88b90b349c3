"""Shared by tests/test_contacts_emu.py and tests/test_gpu_contacts.py: the scenarios of the contact report (hrl_buffers_ext.contacts), the
emulator build that writes it, and the oracle's replay of a step.  Test infrastructure only.

A scenario is run ONCE by the fp32 oracle env (the driver); its trace keeps, per step, the inputs of the step -- state, items, aux, actions --
so that every implementation (emulator forward / reverse, the device) is handed identical inputs each step, and the oracle's own contact
data of that step: `orc_ant_substeps_items_f32` on the pre-step state for the step's substeps (its last substep's surfaces and impulses)."""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np

import capsule_cases
import emu_env
import orc
import textbook as tb
from hrl_pybullet_envs_amd import _capi as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE, HEAD, WIDTH, MAXC, MAXR = K.HRL_CONTACTS_STRIDE, K.HRL_CONTACTS_HEADER, K.HRL_CONTACT_WIDTH, K.HRL_CONTACT_MAX, 44
_LIB = None


def lib():
    """tests/emu/libhrl_emu_contacts.so: emu_lib.cpp + emu_step_contacts, built with the flags of tests/emu/Makefile."""
    global _LIB
    if _LIB is None and emu_env.coverage_dir():   # tests/tools/step_coverage.py: the Makefile's --coverage build of the same source
        d, cov = os.path.join(ROOT, 'tests', 'emu'), emu_env.coverage_dir()
        subprocess.check_call(['make', '-s', '-C', d, 'COVDIR=' + cov, os.path.join(cov, 'libhrl_emu_contacts_cov.so')])
        _LIB = C.CDLL(os.path.join(cov, 'libhrl_emu_contacts_cov.so'))
    if _LIB is None:
        d = os.path.join(ROOT, 'tests', 'emu')
        out, src = os.path.join(d, 'libhrl_emu_contacts.so'), os.path.join(d, 'emu_contacts.cpp')
        deps = [src, os.path.join(d, 'emu_lib.cpp'), os.path.join(ROOT, 'include', 'hrl_envs.h')] + \
               [os.path.join(ROOT, 'hrl_pybullet_envs_amd', 'csrc', f) for f in ('step_core.h', 'host_cfg.h')]
        if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
            with open('/proc/cpuinfo') as f:
                fma = ['-mfma'] if ' fma ' in f.read().replace('\n', ' ') else []
            subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-fPIC', '-std=c++17', '-ffp-contract=off'] + fma +
                                  ['-Wall', '-Wno-unknown-pragmas', '-shared', '-o', out, src, '-lm', '-lpthread'], cwd=d)
        _LIB = C.CDLL(out)
    return _LIB


class EmuContactsEnv(emu_env.EmuEnv):
    """The host executor with the contact report on: `contacts` [N, 256] is rewritten by every step."""

    def __init__(self, cfg, reverse=False):
        super().__init__(cfg, reverse=reverse)
        self.contacts = np.full((self.N, STRIDE), np.nan, np.float32)  # every float must be written by the step

    def step(self, actions):
        self.act[...] = np.asarray(actions, np.float32).reshape(self.N, self.ad)
        b = K.hrl_buffers_ext.of(self._bufs())
        b.contacts = emu_env.ptr(self.contacts)
        assert lib().emu_step_contacts(C.byref(self.cfg), C.byref(b), self.reverse) == 0
        return self.obs, self.rew, self.done, self.info


# ---------------------------------------------------------------------------------------------------------------- scenarios
SEED = 5
NAMES = ('random', 'items', 'walls', 'box', 'self', 'point')
# the states of tests/capsule_cases.py as two-step scenarios of the same machinery (mid-section and second-support contacts), set up at step 0
CAPSULE = ('cubes_under_the_feet', 'foot_across_the_maze_corner', 'feet_flat_against_the_maze_box', 'feet_flat_on_cubes')


def make_cfg(name, n=None, frame_skip=None, **over):
    kw = dict(seed=SEED, auto_reset=1)
    if name == 'random':
        kind, n0 = K.HRL_ANT_GATHER, 16
    elif name == 'items':
        kind, n0 = K.HRL_ANT_GATHER, 16; kw['robot_coll_dist'] = 0.0
    elif name == 'walls':
        kind, n0 = K.HRL_ANT_GATHER, 16
    elif name == 'box':
        kind, n0 = K.HRL_ANT_MAZE, 16
    elif name == 'self':
        kind, n0 = K.HRL_ANT_FLAT, 64; kw['model_frame_skip'] = 1
    elif name in ('cubes_under_the_feet', 'feet_flat_on_cubes'):
        kind, n0 = K.HRL_ANT_GATHER, 16; kw['robot_coll_dist'] = 0.0
    elif name in CAPSULE:
        kind, n0 = K.HRL_ANT_MAZE, 16
    else:
        kind, n0 = K.HRL_POINT_GATHER, 16; kw['robot_coll_dist'] = 0.0  # pickup by contact, as in 'items': placed cubes stay until touched
    if frame_skip is not None:
        kw['model_frame_skip'] = frame_skip
    kw.update(over)
    return orc.default_config(kind, num_envs=n or n0, **kw)


def n_steps(name):
    return 1 if name == 'self' else (2 if name in CAPSULE else 30)


def perturb(name, t, o, rng):
    """The scenario's edit of the driver's state before step t (draws come before the step's actions)."""
    n = o.N
    if name in ('items', 'point') and t >= 10 and t % 5 == 0:  # all 16 cubes around the torso / the cube
        o.items[:, :32] = (o.state[:, None, 0:2] + rng.uniform(-0.9, 0.9, (n, 16, 2)).astype(np.float32)).reshape(n, 32)
    if name == 'walls' and t == 10:
        o.state[:, 0] = (o.cfg.world_size[0] / 2 - 0.05 - rng.uniform(0.3, 0.8, n)).astype(np.float32)
    if name == 'box' and t == 10:
        o.state[:, 0] = (1 + rng.uniform(0.3, 0.8, n)).astype(np.float32)
        o.state[:, 1] = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    if name in CAPSULE and t == 0:
        getattr(capsule_cases, name)(o, rng)
    if name == 'self' and t == 0:  # the pose of tests/test_gpu_parity.py:593: legs thrown across one another in mid-air
        o.state[:, 2] = 1.5; o.state[:, 15:29] = 0
        o.state[:, 7:15:2] = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
        o.state[:, 8:15:2] = rng.uniform(-1.8, 1.8, (n, 4)).astype(np.float32)


def n_items(cfg):
    return cfg.n_food + cfg.n_poison if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) else 0


def pre_step(cfg, state, act):
    """(q, u, tau) of one env as the step kernel forms them from the record and the action, in fp32 (step_core.h, step_entry)."""
    f = np.float32
    qv = state[15:29]
    if cfg.env_kind == K.HRL_POINT_GATHER:  # point_bot.py:28-31: a / |a| * 500 N in the world xy plane
        a = act.astype(f)
        nrm = np.sqrt(f(a[0] * a[0]) + f(a[1] * a[1]), dtype=f)
        with np.errstate(all='ignore'):
            force = np.array([f(f(a[0] / nrm) * f(cfg.model.point_force)), f(f(a[1] / nrm) * f(cfg.model.point_force)), 0], f)
        return state[:7].astype(f), np.concatenate([qv[3:6], qv[0:3]]).astype(f), force
    tau = (f(cfg.model.torque_scale) * np.clip(act.astype(f), f(-1), f(1))).astype(f)
    return state[:15].astype(f), np.concatenate([qv[3:6], qv[0:3], qv[6:14]]).astype(f), tau


def oracle_replay(cfg, state, items, act):
    """The oracle's account of one env's step from its inputs: dict(q, u after the substeps; n_rows, n_limits, n_contacts; surf [n_contacts];
    lam [MAXR] -- the ant kinds; n_item_contacts -- the point bot)."""
    q, u, tau = pre_step(cfg, state, act)
    q, u = q.copy(), u.copy()
    ni = n_items(cfg)
    it = np.ascontiguousarray(items[:2 * ni], np.float32) if ni else None
    info = np.zeros(3, np.int32)
    if cfg.env_kind == K.HRL_POINT_GATHER:
        orc.lib().orc_point_substeps_items_f32(C.byref(cfg), orc.ptr(q), orc.ptr(u), orc.ptr(tau), cfg.model.frame_skip, orc.ptr(it), ni, orc.ptr(info))
        return dict(q=q, u=u, n_rows=int(info[0]), n_limits=0, n_contacts=int(info[2]), n_item_contacts=int(info[1]))
    dbg, lam = np.zeros(1 + MAXC, np.int32), np.zeros(MAXR, np.float32)
    orc.lib().orc_ant_substeps_items_f32(C.byref(cfg), orc.ptr(q), orc.ptr(u), orc.ptr(tau), cfg.model.frame_skip, orc.ptr(it), ni,
                                         orc.ptr(info), orc.ptr(dbg), orc.ptr(lam))
    return dict(q=q, u=u, n_rows=int(info[0]), n_limits=int(info[1]), n_contacts=int(info[2]), surf=dbg[1:1 + info[2]].copy(), lam=lam)


class Trace:
    pass


def trace(name, n=None, frame_skip=None, max_episode_steps=None):
    """The scenario run by the oracle env: per step the inputs, `done`, and the oracle's replay of every env's step.  Computed once per
    (scenario, shape) and shared by the tests: treat as read-only."""
    return _trace(name, n, frame_skip, max_episode_steps)   # (one cache key however the arguments were passed)


@functools.lru_cache(maxsize=None)
def _trace(name, n, frame_skip, max_episode_steps):
    over = {} if max_episode_steps is None else dict(max_episode_steps=max_episode_steps)
    cfg = make_cfg(name, n, frame_skip, **over)
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    rng = np.random.RandomState(SEED)
    tr = Trace()
    tr.name, tr.cfg, tr.steps = name, cfg, []
    for t in range(n_steps(name)):
        perturb(name, t, o, rng)
        a = rng.uniform(-1, 1, (o.N, o.ad)).astype(np.float32)
        s = dict(state=o.state.copy(), items=o.items.copy(), aux=o.aux.copy(), act=a)
        o.step(a)
        s['done'] = o.done.copy()
        s['after'] = o.state.copy()
        s['replay'] = [oracle_replay(cfg, s['state'][i], s['items'][i], a[i]) for i in range(o.N)]
        tr.steps.append(s)
    for k in tr.steps:
        for v in k.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tr


def run(tr, env, step, fetch=lambda e: e.contacts.copy(), push=None, after=None):
    """Hands `env` the trace's inputs step by step; returns the contact records [steps, N, 256] it wrote.  `after`: a list that receives the env's
    own state record after every step."""
    out = []
    for s in tr.steps:
        if push is None:
            env.state[...] = s['state']; env.items[...] = s['items']; env.aux[...] = s['aux']
        else:
            push(env, s)
        step(env, s['act'])
        out.append(fetch(env))
        if after is not None:
            after.append(np.array(env.state))
    return np.stack(out)


def emu_run(name, n=None, frame_skip=None, reverse=False, max_episode_steps=None):
    """The emulator's records of the scenario, [steps, N, 256], and its own state after every step, [steps, N, stride] (read-only, shared)."""
    return _emu_run(name, n, frame_skip, reverse, max_episode_steps)


@functools.lru_cache(maxsize=None)
def _emu_run(name, n, frame_skip, reverse, max_episode_steps):
    tr = trace(name, n, frame_skip, max_episode_steps)
    e = EmuContactsEnv(tr.cfg, reverse=reverse)
    e.reset()
    after = []
    r = run(tr, e, lambda env, a: env.step(a), after=after)
    after = np.stack(after)
    r.setflags(write=False); after.setflags(write=False)
    return r, after


def emu_records(name, n=None, frame_skip=None, reverse=False, max_episode_steps=None):
    """The emulator's records of the scenario, [steps, N, 256] (read-only, shared)."""
    return emu_run(name, n, frame_skip, reverse, max_episode_steps)[0]


# ---------------------------------------------------------------------------------------------------------------- record fields
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def contact(rec, i):
    return rec[HEAD + WIDTH * i: HEAD + WIDTH * (i + 1)]


def limit_lambdas(rec):
    """The limit rows' impulses in row order (ascending joint), rebuilt from the header: [4 + j] * sign for the joints of mask [12]."""
    held, neg = int(rec[12]), int(rec[13])
    return np.array([rec[4 + j] * np.float32(-1 if (neg >> j) & 1 else 1) for j in range(8) if (held >> j) & 1], np.float32)


def check_against_oracle(rec, rp, where):
    """Counts, surfaces and every impulse of one record == the oracle's replay of that step, bit for bit (the ant kinds)."""
    nC, nL = rp['n_contacts'], rp['n_limits']
    assert (int(rec[0]), int(rec[1]), int(rec[2])) == (nC, nL, rp['n_rows']), (where, rec[:3], rp)
    assert [int(contact(rec, i)[16]) for i in range(nC)] == [int(s) for s in rp['surf']], (where, rp['surf'])
    lam = rp['lam']
    got = np.concatenate([limit_lambdas(rec), [contact(rec, i)[7] for i in range(nC)],
                          np.array([[contact(rec, i)[11], contact(rec, i)[15]] for i in range(nC)], np.float32).reshape(-1)]).astype(np.float32)
    assert len(got) == rp['n_rows'] and np.array_equal(bits(got), bits(lam[:len(got)])), (where, got, lam[:len(got)])


# ---------------------------------------------------------------------------------------------------------------- fp64 physics of a record
# What tests/test_contacts_physics.py (the emulator) and tests/test_gpu_contacts.py (the device) hold a record against: plain numpy in fp64 on
# the record's own numbers, the textbook reference (tests/textbook.py) for everything else.  Nothing here reads the oracle or step_core.h.
R_CAPS, R_TORSO = 0.08, 0.25   # assets/ant.xml:16-55: the leg capsules; the torso sphere


def qvel_to_u(cfg, qv):
    """qvel of a state record (v, omega, joint rates) as the solver's u (omega, v, joint rates)"""
    qv = np.asarray(qv, np.float64)
    return np.concatenate([qv[3:6], qv[0:3]] + ([] if cfg.env_kind == K.HRL_POINT_GATHER else [qv[6:14]]))


def contact_impulse(c):
    """n lambda_n + t1 lambda_t1 + t2 lambda_t2 of one contact (fp64, N s, world frame)"""
    c = np.asarray(c, np.float64)
    return c[4:7] * c[7] + c[8:11] * c[11] + c[12:15] * c[15]


def external_impulse(rec):
    """(sum J, sum position x J) over the record's contacts with the world (link2 == -1), about the world origin"""
    J, T = np.zeros(3), np.zeros(3)
    for i in range(int(rec[0])):
        c = contact(rec, i).astype(np.float64)
        if c[18] == -1:
            j = contact_impulse(c)
            J += j; T += np.cross(c[0:3], j)
    return J, T


def free_params(p):
    """tb_params `p` with every external surface removed: no planes, no boxes, the ground 100 m below"""
    f = type(p).from_buffer_copy(p)
    f.n_planes = f.n_boxes = 0
    f.ground_z = -100.0
    return f


def tb_params_of(cfg, items):
    ni = n_items(cfg)
    return tb.params(cfg, items=np.asarray(items[:2 * ni], np.float64) if ni else None)


def clamped(p, u_full, u_free):
    """The leave-out criterion of the momentum balance, on the reference alone: the textbook's own substep -- with or without the surfaces --
    ends with a joint rate at the clamp (|rate| >= vmax (1 - 1e-3)): the one non-linearity between impulses and velocities."""
    return bool((np.abs(np.r_[u_full[6:], u_free[6:]]) >= p.vmax * (1 - 1e-3)).any())


def momentum_change(cfg, state_before, act, u_after, items):
    """(dP, dL, clamped): linear and angular momentum (about the world origin) of the robot at the step's INPUT pose q with the velocity
    `u_after` the step under test ended with, minus the same with the velocity of the textbook's substep from the same (q, u, tau) with
    every external surface removed -- what the world's contact impulses added (frame_skip = 1).  The ant: `textbook.ant_energy_momentum`,
    per-body sums.  The point bot: linear momentum only, m v with the textbook's mass (dL is None: textbook_ref.c keeps the cube's inertia
    to itself)."""
    q, u, tau = (a.astype(np.float64) for a in pre_step(cfg, state_before, act))
    p = tb_params_of(cfg, items)
    free = free_params(p)
    u_after = np.asarray(u_after, np.float64)
    if cfg.env_kind == K.HRL_POINT_GATHER:
        _, u_free, out = tb.point_substep(free, q, u, tau)
        return out.total_mass * (u_after[3:6] - u_free[3:6]), None, False
    u_full, u_free = tb.ant_substep(p, q, u, tau)[1], tb.ant_substep(free, q, u, tau)[1]
    a, b = tb.ant_energy_momentum(p, q, u_after), tb.ant_energy_momentum(p, q, u_free)
    return a[2:5] - b[2:5], a[5:8] - b[5:8], clamped(p, u_full, u_free)


def balance_residual(cfg, state_before, act, u_after, items, rec):
    """(|dP - sum J|, |dL - sum position x J|, clamped) of one env-step: largest component, N s and N m s"""
    dP, dL, cl = momentum_change(cfg, state_before, act, u_after, items)
    J, T = external_impulse(rec)
    return np.abs(dP - J).max(), (0.0 if dL is None else np.abs(dL - T).max()), cl


def after_u(tr, t, i, after):
    """u after step t of env i: from the implementation's own state `after` [steps, N, stride]; an env that ended in the step was reset, so
    the oracle's replay of the terminal substep speaks for it (the bit-for-bit tests show it equals the step wherever the env went on)."""
    s = tr.steps[t]
    return s['replay'][i]['u'].astype(np.float64) if s['done'][i] else qvel_to_u(tr.cfg, after[t, i, 15:29])


def balance(tr, rec, after, skip_done=False):
    """The momentum balance over a scenario.  Returns dict(total, compared, external -- compared env-steps with a contact with the world --,
    clamped, skipped -- done / no finite action --, worst_P, worst_L, at_P, at_L -- the (t, i) of the worst --, rows -- the (t, i) compared)."""
    n = dict(total=0, compared=0, external=0, clamped=0, skipped=0, worst_P=0.0, worst_L=0.0, at_P=None, at_L=None, rows=[])
    for t, s in enumerate(tr.steps):
        for i in range(tr.cfg.num_envs):
            if (skip_done and s['done'][i]) or not np.isfinite(pre_step(tr.cfg, s['state'][i], s['act'][i])[2]).all():
                n['skipped'] += 1
                continue
            n['total'] += 1
            eP, eL, cl = balance_residual(tr.cfg, s['state'][i], s['act'][i], after_u(tr, t, i, after), s['items'][i], rec[t, i])
            if cl:
                n['clamped'] += 1
                continue
            n['compared'] += 1
            n['rows'].append((t, i))
            n['external'] += any(contact(rec[t, i], k)[18] == -1 for k in range(int(rec[t, i, 0])))
            if eP > n['worst_P']:
                n['worst_P'], n['at_P'] = eP, (t, i)
            if eL > n['worst_L']:
                n['worst_L'], n['at_L'] = eL, (t, i)
    return n


def link_segment(q, legs, link):
    """The capsule axis of a link code `link = level | leg << 2` at pose q (legs = textbook.ant_points(p, q)[0]; assets/ant.xml:16-55):
        level 0  torso centre -> hip point of `leg`   (rigid with the torso; code 0 = level 0 of leg 0 is ALSO the torso sphere, radius 0.25)
        level 1  hip point -> ankle point             (the aux body)
        level 2  ankle point -> foot tip              (the foot)
    every capsule of radius 0.08."""
    level, leg = link & 3, link >> 2
    return (np.asarray(q[:3], np.float64) if level == 0 else legs[leg, level - 1]), legs[leg, level]


def seg_point(a, b, x):
    """the point of segment a-b closest to x"""
    d = b - a
    L = d @ d
    return a + d * (np.clip((x - a) @ d / L, 0, 1) if L > 0 else 0.0)


def seg_seg(p1, q1, p2, q2):
    """closest points of two segments (fp64; Ericson, Real-Time Collision Detection 5.1.9)"""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f, c, b = d1 @ d1, d2 @ d2, d2 @ r, d1 @ r, d1 @ d2
    den = a * e - b * b
    s = np.clip((b * f - c * e) / den, 0, 1) if den > 1e-14 else 0.0
    t = (b * s + f) / e
    if t < 0:
        t, s = 0.0, np.clip(-c / a, 0, 1)
    elif t > 1:
        t, s = 1.0, np.clip((b - c) / a, 0, 1)
    return p1 + d1 * s, p2 + d2 * t


def link_gap(q, legs, link, x):
    """distance of x to the surface of the shape(s) a link code names (<= 0: inside)"""
    a, b = link_segment(q, legs, link)
    g = np.linalg.norm(x - seg_point(a, b, x)) - R_CAPS
    return min(g, np.linalg.norm(x - q[:3]) - R_TORSO) if link == 0 else g


def box_of(cfg, p, c):
    """(lo, hi) of the box an external contact with surface code >= HRL_SURF_BOX names, from tb_params"""
    s = int(c[16])
    k = s - K.HRL_SURF_BOX if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ) else (s - K.HRL_SURF_ITEM if s < K.HRL_SURF_SELF else s - K.HRL_SURF_SELF)
    assert 0 <= k < p.n_boxes, (s, k)
    return np.array(p.box_lo[k][:]), np.array(p.box_hi[k][:])


def check_geometry(cfg, rec, state, items, where, n):
    """Every contact of one ant record against fp64 kinematics of the step's input pose (tolerances: 1e-5 m and 1e-6 on metre-scale fp32
    numbers as check_invariants has them, 1e-4 on a direction normalised from a vector of >= 1e-3 m -- shorter ones are counted in
    n['short'], not compared).  n: counters, updated in place (contacts, short, wall, box_out, box_face_out, box_edge, box_in, self, hand -- the set of
    signs of (t1 x t2) . normal seen)."""
    q = state[:15].astype(np.float64)
    p = tb_params_of(cfg, items)
    legs = tb.ant_points(p, q)[0]
    for i in range(int(rec[0])):
        c = contact(rec, i).astype(np.float64)
        w = where + (i,)
        x, dist, nrm, t1, t2, surf, link, link2 = c[0:3], c[3], c[4:7], c[8:11], c[12:15], int(c[16]), int(c[17]), int(c[18])
        n['contacts'] += 1
        hand = np.cross(t1, t2) @ nrm
        assert abs(abs(hand) - 1) <= 1e-5 and np.abs(np.cross(t1, t2) - np.sign(hand) * nrm).max() <= 1e-5, (w, 'frame', t1, t2, nrm)
        n['hand'].add(int(np.sign(hand)))
        assert 0 <= link < 16 and (link & 3) < 3, (w, link)
        assert link_gap(q, legs, link, x) <= 1e-5, (w, 'position is not on link', link, link_gap(q, legs, link, x))
        if link2 >= 0:
            n['self'] += 1
            assert contact(rec, i)[19] == np.float32(p.mu_self), (w, 'mu', c[19])
            assert 0 <= link2 < 16 and (link2 & 3) < 3 and (link >> 2) != (link2 >> 2), (w, link, link2)
            a2, b2 = link_segment(q, legs, link2)
            g2 = np.linalg.norm(x - seg_point(a2, b2, x)) - R_CAPS
            assert g2 <= max(dist, 0) + 1e-5, (w, 'position is not at link2', link2, g2, dist)
            c1, c2 = seg_seg(*link_segment(q, legs, link), a2, b2)
            gap = np.linalg.norm(c1 - c2)
            assert abs(gap - 2 * R_CAPS - dist) <= 1e-5, (w, 'self dist', gap - 2 * R_CAPS, dist)
            if gap < 1e-3:
                n['short'] += 1
            else:
                assert np.abs(nrm - (c1 - c2) / gap).max() <= 1e-4, (w, 'self normal', nrm, (c1 - c2) / gap)
            continue
        assert contact(rec, i)[19] == np.float32(p.mu), (w, 'mu', c[19])
        if surf == 0:
            continue   # the ground: check_invariants (normal (0, 0, 1) exactly, z - ground_z == dist)
        if surf < K.HRL_SURF_BOX:
            n['wall'] += 1
            assert surf - 1 < p.n_planes, (w, surf)
            pn, pd = np.array(p.plane_n[surf - 1][:]), p.plane_d[surf - 1]
            assert np.abs(nrm - pn).max() <= 1e-6 and abs(pn @ x - pd - dist) <= 1e-5, (w, 'wall', nrm, pn, pn @ x - pd, dist)
            continue
        lo, hi = box_of(cfg, p, c)
        k = int(np.argmax(np.abs(nrm)))
        if dist > 0:   # outside: the fp64 closest point of the box to the position is `dist` away
            gap = np.linalg.norm(x - np.clip(x, lo, hi))
            assert abs(gap - dist) <= 1e-5, (w, 'box dist', gap, dist)
        if abs(nrm[k]) == 1.0:   # a face of the box: its outward axis; the position over (dist > 0) or behind it by dist, within the face's outline
            n['box_face_out' if dist > 0 else 'box_in'] += 1
            height = x[k] - hi[k] if nrm[k] > 0 else lo[k] - x[k]
            assert abs(height - dist) <= 1e-5, (w, 'box face', height, dist)
            o = [j for j in range(3) if j != k]
            assert (x[o] >= lo[o] - 1e-5).all() and (x[o] <= hi[o] + 1e-5).all(), (w, 'beside the face', x, lo, hi)
            continue
        # An edge or a corner of the box (dist <= 0: the surface is in, the capsule's axis still outside).  The direction from the box's closest
        # point to the position is formed stably: box point, position and the capsule's axis point are collinear, and the axis point is a radius
        # or more away from the box where the position may be microns away (an fp32 world coordinate of +-8 m carries 5e-7 m: 1e-4 only on a
        # vector of >= 5e-3 m).  The axis point comes from fp64 kinematics: the point of the link's axis closest to the position (link 0: the
        # hip capsule of leg 0, or the torso's centre).  A surface far in with the axis less than 1 cm out leaves the same question on that
        # vector -- the step forms it from fp32 world coordinates, two roundings of 2.4e-7 m and the kinematics' own: 1e-6 m, 1e-4 of 1e-2 m --
        # and is counted as short.
        n['box_out' if dist > 0 else 'box_edge'] += 1
        best = None
        for ctr, rad in [(seg_point(*link_segment(q, legs, link), x), R_CAPS)] + ([(q[:3], R_TORSO)] if link == 0 else []):
            v = ctr - np.clip(ctr, lo, hi)
            g = np.linalg.norm(v)
            err = (abs(g - rad - dist), np.abs(nrm - v / g).max() if g >= 1e-2 else np.inf, g)
            best = err if best is None or err[:2] < best[:2] else best
        if best[2] < 1e-2:
            n['short'] += 1
            continue
        assert best[0] <= 1e-5 and best[1] <= 1e-4, (w, 'box distance / normal from the axis point', best, nrm, dist)


def geometry_counters():
    return dict(contacts=0, short=0, wall=0, box_out=0, box_face_out=0, box_edge=0, box_in=0, self=0, hand=set())


def geometry(tr, rec, skip_done=False):
    """check_geometry over a scenario; returns the counters.  One handedness for the whole run; at most 5 % of the contacts skipped for a
    direction too short to normalise."""
    n = geometry_counters()
    for t, s in enumerate(tr.steps):
        for i in range(tr.cfg.num_envs):
            if not (skip_done and s['done'][i]):
                check_geometry(tr.cfg, rec[t, i], s['state'][i], s['items'][i], (tr.name, t, i), n)
    assert len(n['hand']) <= 1, (tr.name, 'mixed handedness', n['hand'])
    assert n['short'] <= 0.05 * n['contacts'], (tr.name, n)
    return n


def body_of_link(link):
    """numpy twin of contacts.body_of_link: 0 the torso (level 0 of any leg), else 2 leg + level"""
    return 0 if link & 3 == 0 else 2 * (link >> 2) + (link & 3)


def link_impulses(rec):
    """[9, 3] fp64: the record regrouped by body -- external contacts on body(link); a self contact +J on body(link), -J on body(link2)"""
    out = np.zeros((9, 3))
    for i in range(int(rec[0])):
        c = contact(rec, i).astype(np.float64)
        j = contact_impulse(c)
        out[body_of_link(int(c[17]))] += j
        if c[18] >= 0:
            out[body_of_link(int(c[18]))] -= j
    return out


def check_link_force(rec, tol, device='cpu'):
    """contacts.decode / contacts.link_force on real records [M, 256] (torch, on `device`): link_force x h per body == the numpy regrouping of
    the record by link, its sum over bodies == sum J of the contacts with the world (a self contact cancels itself), within `tol` N s.
    Returns (the largest difference, the number of self contacts seen)."""
    import torch
    from hrl_pybullet_envs_amd import contacts
    raw = torch.tensor(np.ascontiguousarray(rec)).to(device)
    d = contacts.decode(raw)
    lf = (contacts.link_force(d).double() * d['h'].double()[:, None, None]).cpu().numpy()
    assert d['n'].cpu().numpy().tolist() == rec[:, 0].astype(int).tolist()
    worst = n_self = 0
    for m in range(len(rec)):
        want = link_impulses(rec[m])
        n_self += sum(contact(rec[m], i)[18] >= 0 for i in range(int(rec[m, 0])))
        worst = max(worst, np.abs(lf[m] - want).max(), np.abs(lf[m].sum(0) - external_impulse(rec[m])[0]).max())
        assert np.abs(lf[m] - want).max() <= tol and np.abs(lf[m].sum(0) - external_impulse(rec[m])[0]).max() <= tol, (m, lf[m], want)
    return worst, n_self


# ---------------------------------------------------------------------------------------------------------------- tolerances, floors
# The worst residuals of the momentum balance measured on the emulator over the scenarios of tests/test_contacts_physics.py (the device gives
# the same figures); the tolerance is 4 x that, and must stay under a ceiling that does not depend on the code under test: 1 % of the impulse one foot of a standing
# ant carries per substep, M g h / 4 = 182 kg x 9.8 m/s^2 x 0.004125 s / 4 = 1.8 N s.  Single impulses of these scenarios reach thousands of
# N s (feet teleported into cubes and walls), so the balance closes to about 1e-6 relative; a contact with the wrong sign, the wrong tangent
# or a misplaced point is off by its own impulse, or its impulse times centimetres.
P_MEASURED = 2.4e-3   # N s:   2.41e-3, scenario `box`, step 10, env 9
L_MEASURED = 2.3e-3   # N m s: 2.32e-3, scenario `box`, step 10, env 12
P_TOL, L_TOL = 4 * P_MEASURED, 4 * L_MEASURED
CEILING = 0.02        # N s and N m s
EXTERNAL_FLOOR = {'items': 50, 'walls': 25, 'box': 100}   # compared env-steps that carry a contact with the world


def check_balance(name, n, clamp_share=0.05, floors=True):
    print(f"{name}: compared {n['compared']} of {n['total']} env-steps ({n['external']} with external contacts, {n['clamped']} left out for the rate clamp); "
          f"worst |dP - sum J| {n['worst_P']:.2e} N s at {n['at_P']}, worst |dL - sum r x J| {n['worst_L']:.2e} N m s at {n['at_L']}")
    assert P_TOL <= CEILING and L_TOL <= CEILING
    assert n['clamped'] <= clamp_share * n['total'], (name, n)
    assert not floors or n['external'] >= EXTERNAL_FLOOR.get(name, 0), (name, n)
    assert n['worst_P'] <= P_TOL and n['worst_L'] <= L_TOL, (name, n)


def item_boxes(o, i):
    """{surface code: (lo, hi)} of env i's cubes"""
    ni = n_items(o.cfg)
    it = o.items[i, :2 * ni].reshape(ni, 2).astype(np.float64)
    return {(K.HRL_SURF_ITEM + k if k < 48 else K.HRL_SURF_SELF + k): (np.r_[it[k] - 0.125, -0.025], np.r_[it[k] + 0.125, 0.225]) for k in range(ni)}


def as_env(tr, s):
    return types.SimpleNamespace(cfg=tr.cfg, state=s['state'], items=s['items'], N=tr.cfg.num_envs)


def capsule_coverage(tr, rows_of):
    """(mid-section contacts, second support points) by the counting functions of tests/capsule_cases.py over the env-steps rows_of(t)"""
    box = {K.HRL_SURF_BOX: (np.array([-5., -2, 0]), np.array([1., 2, 2]))}
    mid = second = 0
    for t, s in enumerate(tr.steps):
        o = as_env(tr, s)
        mid += capsule_cases.count_mid_section_contacts(o, rows_of(t), (lambda i: item_boxes(o, i)) if n_items(tr.cfg) else (lambda i: box))
        second += capsule_cases.count_second_points(o, rows_of(t))
    return mid, second


def geometry_floor(name, n):
    """contacts of the scenario's own class that the geometry check must have seen (the free-falling random run meets no surface in 30 substeps)"""
    boxes = n['box_out'] + n['box_face_out'] + n['box_edge'] + n['box_in']
    return {'random': True, 'walls': n['wall'] >= 25, 'box': boxes >= 50, 'items': boxes >= 50, 'self': n['self'] >= 10}.get(name, boxes >= 1)
