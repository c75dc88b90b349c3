"""Shared by tests/test_contacts_emu.py and tests/test_gpu_contacts.py: the scenarios of the contact report (hrl_buffers_ext.contacts), the
emulator build that writes it, and the oracle's replay of a step.  Test infrastructure only.

A scenario is run ONCE by the fp32 oracle env (the driver); its trace keeps, per step, the inputs of the step -- state, items, aux, actions --
so that every implementation (emulator forward / reverse, the device) is handed identical inputs each step, and the oracle's own contact
data of that step: `orc_ant_substeps_items_f32` on the pre-step state for the step's substeps (its last substep's surfaces and impulses)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import emu_env
import orc
from hrl_pybullet_envs_amd import _capi as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE, HEAD, WIDTH, MAXC, MAXR = K.HRL_CONTACTS_STRIDE, K.HRL_CONTACTS_HEADER, K.HRL_CONTACT_WIDTH, K.HRL_CONTACT_MAX, 44
_LIB = None


def lib():
    """tests/emu/libhrl_emu_contacts.so: emu_lib.cpp + emu_step_contacts, built with the flags of tests/emu/Makefile."""
    global _LIB
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
    else:
        kind, n0 = K.HRL_POINT_GATHER, 16; kw['robot_coll_dist'] = 0.0  # pickup by contact, as in 'items': placed cubes stay until touched
    if frame_skip is not None:
        kw['model_frame_skip'] = frame_skip
    kw.update(over)
    return orc.default_config(kind, num_envs=n or n0, **kw)


def n_steps(name):
    return 1 if name == 'self' else 30


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


@functools.lru_cache(maxsize=None)
def trace(name, n=None, frame_skip=None, max_episode_steps=None):
    """The scenario run by the oracle env: per step the inputs, `done`, and the oracle's replay of every env's step.  Computed once per
    (scenario, shape) and shared by the tests: treat as read-only."""
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


def run(tr, env, step, fetch=lambda e: e.contacts.copy(), push=None):
    """Hands `env` the trace's inputs step by step; returns the contact records [steps, N, 256] it wrote."""
    out = []
    for s in tr.steps:
        if push is None:
            env.state[...] = s['state']; env.items[...] = s['items']; env.aux[...] = s['aux']
        else:
            push(env, s)
        step(env, s['act'])
        out.append(fetch(env))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def emu_records(name, n=None, frame_skip=None, reverse=False, max_episode_steps=None):
    """The emulator's records of the scenario, [steps, N, 256] (read-only, shared)."""
    tr = trace(name, n, frame_skip, max_episode_steps)
    e = EmuContactsEnv(tr.cfg, reverse=reverse)
    e.reset()
    r = run(tr, e, lambda env, a: env.step(a))
    r.setflags(write=False)
    return r


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
