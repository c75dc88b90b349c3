"""Shared by tests/test_emu_halfwave_rows.py and tests/test_gpu_halfwave_rows.py: poses that put every class of substep before the row build of
csrc/step_core.h -- the build on both half-waves (at most 32 rows, no self contact: phase_build_A_halves) and the one it falls back to
(build_A_blocks) -- the fp32 oracle's run of them, and the comparison of a side under test with it.  Test infrastructure only.

A case is (env kind, config overrides, pose function, classes it must show).  The oracle env is reset, the poses are written over its qpos / qvel,
and it then runs STEPS steps on its own; a side under test is reset, handed the same qpos / qvel through its own set-state call and runs on its
own too: after every step all nine buffers and the solver-row counter must equal the oracle's byte for byte.  Which classes occurred is read from
what the SIDE wrote: the contact report's header (n_contacts, n_limit_rows, n_rows of the step's last substep), its link2 fields (a self contact)
and the per-step `solver_rows`.  Every draw is made env by env and the actions come from one stream per step, so the first 16 envs of a 64-env run
are the 16-env run."""
import functools

import numpy as np

import contacts_cases as cc
import orc
from backends import ALL
from hrl_pybullet_envs_amd import _capi as K

STEPS = 8
JLO = np.radians([-40, 30, -40, -100, -40, -100, -40, 30])   # assets/ant.xml:18-54
JHI = np.radians([40, 100, 40, -30, 40, -30, 40, 100])

CLASSES = ('rows0', 'bounded_1_4_alone', 'nB_under', 'nB_on', 'nB_over', 'nF_under', 'nF_on', 'nF_over', 'standing20', 'rows32', 'rows33plus', 'self')


def classes_of(nL, nC, has_self):
    """the classes one substep with nL limit rows and nC contacts belongs to (nB = nL + nC bounded rows, nF = 2 nC friction rows)"""
    nB, nF, nR = nL + nC, 2 * nC, nL + 3 * nC
    if has_self:
        return {'self'}
    if nR > 32:
        return {'rows33plus'}
    out = set()   # everything below takes the build on both half-waves
    if nR == 0:
        out.add('rows0')
    if nC == 0 and 1 <= nL <= 4:
        out.add('bounded_1_4_alone')
    if nF > 0:   # a block "just under / on / just over" a multiple of four: its last group of four columns is nearly full, full, or holds one (two) columns
        if nB % 4 == 3:
            out.add('nB_under')
        if nB % 4 == 0:
            out.add('nB_on')
        if nB % 4 == 1 and nB > 4:
            out.add('nB_over')
        out.add('nF_on' if nF % 4 == 0 else 'nF_under')    # nF is even: 2, 6, 10 ... is two short of a multiple of four
        if nF % 4 == 2 and nF > 4:
            out.add('nF_over')                             # ... and 6, 10 ... is also two past one
    if (nL, nC) == (8, 4):
        out.add('standing20')
    if nR == 32:
        out.add('rows32')
    return out


def _quat(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.r_[axis * np.sin(ang / 2), np.cos(ang / 2)]


def _qmul(a, b):
    x1, y1, z1, w1 = a; x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def pose_air(i, rng):
    """in the air, level, joints at mid-range except the first i % 5, which sit ON a stop: 0 .. 4 limit rows and nothing else"""
    q = np.zeros(15); q[2] = 1.5; q[6] = 1.0
    q[7:] = 0.5 * (JLO + JHI)
    k = i % 5
    q[7:7 + k] = np.where(np.arange(k) % 2 == 0, JLO[:k], JHI[:k])
    return q


def _random_pose(rng, zlo, zhi, tilt, at_stop, xy):
    q = np.zeros(15)
    q[:2] = xy(rng)
    q[2] = rng.uniform(zlo, zhi)
    q[3:7] = _qmul(_quat([0, 0, 1], rng.uniform(-np.pi, np.pi)), _quat(rng.normal(size=3), rng.uniform(0, tilt)))
    u = rng.uniform(0, 1, 8)
    u = np.where(rng.rand(8) < at_stop, rng.randint(0, 2, 8).astype(float), u)
    q[7:] = JLO + u * (JHI - JLO)
    return q


def pose_low(i, rng):
    """dropped close to the ground at a small tilt, half of the joints on a stop: some feet down, some limits held"""
    return _random_pose(rng, 0.15, 0.6, 0.3, 0.5, lambda r: r.uniform(-1, 1, 2))


def pose_wall(i, rng):
    """low and tilted by up to a radian against the +x wall of the gather arena: ground and wall contacts of many spheres at once"""
    return _random_pose(rng, 0.1, 0.5, 1.0, 0.3, lambda r: np.r_[r.uniform(4.4, 4.9), r.uniform(-3, 3)])


def pose_stand(i, rng):
    """standing: level, the feet on the ground (z = 0.4), the ankles on the stop that stretches the leg and the hips on their lower stop -- four
    foot contacts and all eight joints at their stops, the 20 rows of DevCfg::hot_rows"""
    q = np.zeros(15); q[2] = 0.4; q[6] = 1.0
    q[7::2] = JLO[0::2]
    q[8::2] = [JLO[1], JHI[3], JHI[5], JLO[7]]
    return q


def pose_self(i, rng):
    """the pose of tests/contacts_cases.py `self`: in mid-air with the legs thrown across one another"""
    q = np.zeros(15); q[2] = 1.5; q[6] = 1.0
    q[7::2] = rng.uniform(-1.5, 1.5, 4)
    q[8::2] = rng.uniform(-1.8, 1.8, 4)
    return q


# name: (kind, overrides, pose, seed of the poses, classes the run must show).  One substep per step wherever the classes are counted per substep.
CASES = {
    'air': (K.HRL_ANT_FLAT, dict(model_frame_skip=1), pose_air, 0, {'rows0', 'bounded_1_4_alone'}),
    'low': (K.HRL_ANT_FLAT, dict(model_frame_skip=1), pose_low, 0, {'nB_under', 'nB_on', 'nB_over', 'nF_under', 'nF_on', 'nF_over'}),
    'stand': (K.HRL_ANT_FLAT, dict(), pose_stand, 0, {'standing20'}),   # four substeps per step, as shipped
    # limit_margin wider than every joint's range: all eight limit rows in every substep, so 8 contacts are 32 rows and 9 take the fallback
    'wall': (K.HRL_ANT_GATHER, dict(model_frame_skip=1, model_limit_margin=10.0), pose_wall, 1, {'rows32', 'rows33plus'}),
    'self': (K.HRL_ANT_FLAT, dict(model_frame_skip=1), pose_self, 0, {'self'}),
}
assert set().union(*(c[4] for c in CASES.values())) == set(CLASSES)
CPU_ENVS = {'air': 10, 'low': 16, 'stand': 4, 'wall': 16, 'self': 16}
NAMES = ALL + ('solver_rows',)


def make_cfg(name, n):
    kind, over, *_ = CASES[name]
    return orc.default_config(kind, num_envs=n, seed=5, auto_reset=1, **over)


def start_state(name, o):
    """(qpos [N, 15], qvel [N, 14]) of the case for the reset oracle env `o`, float32"""
    _, _, pose, seed, _ = CASES[name]
    rng = np.random.RandomState(seed)
    qpos, qvel = o.state[:, :15].copy(), np.zeros((o.N, 14), np.float32)
    for i in range(o.N):
        qpos[i] = pose(i, rng).astype(np.float32)
    return qpos, qvel


def actions(t, n, ad):
    return np.random.RandomState(1000 + t).uniform(-1, 1, (n, ad)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_run(name, n):
    """(cfg, qpos, qvel, per step a dict of the oracle's buffers after the step); computed once per (case, size), read-only"""
    cfg = make_cfg(name, n)
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    qpos, qvel = start_state(name, o)
    o.state[:, :15] = qpos; o.state[:, 15:29] = qvel
    steps = []
    for t in range(STEPS):
        o.step(actions(t, n, o.ad))
        snap = {k: getattr(o, k).copy() for k in NAMES}
        for v in snap.values():
            v.setflags(write=False)
        steps.append(snap)
    qpos.setflags(write=False); qvel.setflags(write=False)
    return cfg, qpos, qvel, steps


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_side(name, n, side, records, buffers):
    """Drives `side` (reset by the caller) through the case and holds it against the oracle after every step, byte for byte.  records(side) -> the
    contact records [N, 256] of the last step, buffers(side, name) -> a numpy copy of one buffer.  Returns the set of classes the side's own
    records showed."""
    cfg, qpos, qvel, steps = oracle_run(name, n)
    side.set(qpos.copy(), qvel.copy())
    seen, rows_before = set(), np.zeros(n, np.int64)
    for t, snap in enumerate(steps):
        side.step(actions(t, n, side.ad))
        for k in NAMES:
            got = buffers(side, k)
            assert got.dtype == snap[k].dtype and np.array_equal(raw(got), raw(snap[k])), (name, t, k, np.argwhere(got != snap[k])[:4].tolist())
        rec, rows = records(side), buffers(side, 'solver_rows').astype(np.int64)
        assert not np.isnan(rec).any()
        for i in range(n):
            nC, nL, nR = int(rec[i, 0]), int(rec[i, 1]), int(rec[i, 2])
            assert nR == nL + 3 * nC and 0 <= nC <= cc.MAXC and 0 <= nL <= 8, (name, t, i, rec[i, :3])
            if cfg.model.frame_skip == 1:   # one substep: the step's row count is the header's
                assert rows[i] - rows_before[i] == nR, (name, t, i, rows[i] - rows_before[i], nR)
            seen |= classes_of(nL, nC, any(cc.contact(rec[i], k)[18] >= 0 for k in range(nC)))
        rows_before = rows
    return seen
