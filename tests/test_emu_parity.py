"""Kernel logic on the CPU: the product's wave phases (csrc/step_core.h) run by the lock-step host executor
(tests/emu) against the independent scalar oracle.  Same compiler flags (-ffp-contract=off), same libm, and the
algorithm pins every operation order, so the two implementations must agree BIT FOR BIT.  This is what lets the GPU
tests attribute any difference to device arithmetic rather than to kernel logic."""
import ctypes as C

import numpy as np
import pytest

import emu_env
import orc
import parity_cases as P
from backends import Emu, same
from hrl_pybullet_envs_amd import _capi as K

KINDS = [K.HRL_ANT_FLAT, K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN]
REFUSED = dict(expected_exception=ValueError)   # what the adapter raises where the host executor refuses a goal list


def make(kind, count_rows=False, **over):
    """the sides tests/parity_cases.py drives: the host executor in both lane orders (it counts solver rows anyway)"""
    return [Emu(Emu.config(kind, **over)), Emu(Emu.config(kind, **over), reverse=True)]


@pytest.mark.parametrize('kind', KINDS)
def test_reset_bit_exact(kind):
    P.reset(make, kind, 64, every=3, seed=7)


@pytest.mark.parametrize('kind', KINDS)
def test_free_running_bit_exact(kind):
    """Both implementations run free (no state copying) for 120 steps with auto-reset and a short time limit."""
    P.free_running(make, kind, 24, 120, stream=kind, min_episodes=3, seed=3, max_episode_steps=50)   # every env went through at least two auto-resets


def test_gather_pickups_happen_and_match():
    """Drive the ants onto food: pickup, respawn draws and rewards must match exactly."""
    P.gather_pickups(make, 32, 40, need=dict(picked=51))


def test_maze_reaches_targets_and_matches():
    n = 32
    cfg = orc.default_config(K.HRL_ANT_MAZE, num_envs=n, seed=2, auto_reset=1)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    o.reset(); e.reset()
    rng = np.random.RandomState(9)
    hits = 0
    for t in range(20):
        tgt = np.array([[2, -3], [2, 0], [2, 3], [-2, 4]], np.float32)[o.aux[:, 3]]
        xy = tgt + rng.uniform(-2.5, 2.5, (n, 2)).astype(np.float32)
        xy[:, 0] = np.clip(xy[:, 0], 1.6, 4.5)  # stay out of the box
        o.state[:, 0:2] = xy; e.state[:, 0:2] = xy
        o.state[:, 2] = 0.6; e.state[:, 2] = 0.6
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        o.step(a); e.step(a)
        hits += int((o.rew > 0).sum())
        assert np.array_equal(o.rew, e.rew) and np.array_equal(o.done, e.done) and np.array_equal(o.state, e.state)
    assert hits > 20


@pytest.mark.parametrize('kind,n_bins,nf,npo', [(K.HRL_ANT_GATHER, 10, 8, 8), (K.HRL_POINT_GATHER, 5, 8, 8), (K.HRL_ANT_GATHER, 3, 5, 2)])
def test_abs_pos_observation_variant(kind, n_bins, nf, npo):
    """use_sensor=False (ant_gather_env.py:179-196): nearest-first item coordinates instead of the bin sensor."""
    cfg = orc.default_config(kind, num_envs=16, seed=3, auto_reset=1, use_sensor=0, n_bins=n_bins, n_food=nf, n_poison=npo)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    assert o.od == (26 if kind == K.HRL_ANT_GATHER else 8) + 2 * (min(nf, n_bins) + min(npo, n_bins))
    o.reset(); e.reset()
    assert np.array_equal(o.obs, e.obs)
    rng = np.random.RandomState(0)
    for t in range(40):
        a = rng.uniform(-1, 1, (16, o.ad)).astype(np.float32)
        o.step(a); e.step(a)
        assert np.array_equal(o.obs, e.obs) and np.array_equal(o.state, e.state) and np.array_equal(o.items, e.items)
    # nearest-first: consecutive squared distances of the reported food items are non-decreasing
    nb = 26 if kind == K.HRL_ANT_GATHER else 8
    mf = min(nf, n_bins)
    fxy = o.obs[:, nb:nb + 2 * mf].reshape(16, mf, 2)
    d2 = ((fxy - o.state[:, None, 0:2]) ** 2).sum(-1)
    assert np.all(np.diff(d2, axis=1) >= -1e-4)


def test_flagrun_goals_rewards_and_exhaustion():
    """Teleport the ants onto their goals: +5000 and a new goal each time, `done` once the 4 goals are used up."""
    import ctypes as C
    n = 16
    cfg = orc.default_config(K.HRL_ANT_FLAGRUN, num_envs=n, seed=6, auto_reset=1, flag_max_targets=4, use_sensor=1)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    o.reset(); e.reset()
    rng = np.random.RandomState(3)
    hits = dones = 0
    for t in range(24):
        if t % 2 == 1:
            for i in range(n):
                g = np.zeros(2, np.float32)
                orc.lib().orc_flag_goal_f32(C.byref(cfg), int(o.aux[i, 2]), int(o.aux[i, 3] & 0xffff), orc.ptr(g))
                # walk_target_dist is measured from the parts centroid (13 links + floor + wall at (-6, 0)): invert it
                o.state[i, 0:2] = np.clip([(15 * g[0] + 6) / 13, 15 * g[1] / 13], -5.5, 5.5); o.state[i, 2] = 0.6
            e.state[...] = o.state
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        o.step(a); e.step(a)
        hits += int((o.rew > 1000).sum()); dones += int(o.done.sum())
        for name in ('state', 'aux', 'obs', 'rew', 'done'):
            assert np.array_equal(getattr(o, name), getattr(e, name)), (t, name)
    assert o.obs.shape == (n, 36) and hits >= 4 * n and dones >= n


def test_flagrun_close_goal_mode():
    """max_target_dist mode (ant_flagrun_env.py:80-89,111-112): goals drawn around the robot, kept in items[0..1], never run out."""
    n = 16
    cfg = orc.default_config(K.HRL_ANT_FLAGRUN, num_envs=n, seed=11, auto_reset=1, flag_max_targets=0, flag_max_target_dist=3.0,
                             flag_timeout=7)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    o.reset(); e.reset()
    assert np.array_equal(o.items, e.items) and np.array_equal(o.obs, e.obs)
    g0 = o.items[:, 0:2].copy()
    # first goal: per axis tol <= |offset from the start pose (0, 0)| <= max_target_dist / 2, inside the arena
    assert np.all(np.abs(g0) >= 0.5 - 1e-6) and np.all(np.abs(g0) <= 1.5 + 1e-6) and len({tuple(r) for r in g0.tolist()}) > 1
    rng = np.random.RandomState(5)
    hits = retargets = 0
    for t in range(40):
        if t % 5 == 3:  # teleport onto the goal (walk_target_dist is measured from the parts centroid: 13 links + floor + wall at (-6, 0))
            g = o.items[:, 0:2]
            o.state[:, 0] = np.clip((15 * g[:, 0] + 6) / 13, -4.2, 4.2); o.state[:, 1] = np.clip(15 * g[:, 1] / 13, -4.2, 4.2)
            o.state[:, 2] = 0.75; o.state[:, 3:7] = (0, 0, 0, 1); o.state[:, 7:29] = 0  # a clean drop pose, clear of ground and walls
            e.state[...] = o.state
        before = o.items[:, 0:2].copy()
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        o.step(a); e.step(a)
        for name in ('state', 'items', 'aux', 'obs', 'rew', 'done'):
            assert np.array_equal(getattr(o, name), getattr(e, name)), (t, name)
        moved = np.any(o.items[:, 0:2] != before, axis=1) & ~o.done.astype(bool)
        retargets += int(moved.sum()); hits += int((o.rew > 1000).sum())
        # a fresh goal lies within max_target_dist / 2 per axis of the robot and strictly inside the arena
        d = np.abs(o.items[moved, 0:2] - o.state[moved, 0:2])
        assert np.all(d <= 1.5 + 1e-5) and np.all(d >= 0.5 - 1e-5) and np.all(np.abs(o.items[moved, 0:2]) < 5.0)
    assert hits >= n and retargets >= 4 * n  # reached goals + 7-step timeouts; the episode never ends for lack of goals
    bad = orc.default_config(K.HRL_ANT_FLAGRUN, flag_max_targets=5, flag_max_target_dist=2.0)
    import ctypes as C
    assert b'exactly one' in emu_env.lib().emu_validate(C.byref(bad))


def test_validation_errors():
    import ctypes as C
    L = emu_env.lib()
    bad = orc.default_config(K.HRL_ANT_GATHER, n_food=40, n_poison=25)
    assert b'n_food' in L.emu_validate(C.byref(bad))
    assert L.emu_validate(C.byref(orc.default_config(K.HRL_ANT_GATHER, n_food=40, n_poison=24, n_bins=64))) == b''   # 64 items, obs 154
    assert b'n_bins' in L.emu_validate(C.byref(orc.default_config(K.HRL_ANT_GATHER, n_bins=65)))
    assert b'flag_goal_capacity' in L.emu_validate(C.byref(orc.default_config(K.HRL_ANT_FLAGRUN, flag_manual_goals=1, flag_goal_capacity=64)))
    bad = orc.default_config(K.HRL_ANT_GATHER, robot_coll_dist=0, model_item_collision=0)
    assert b'robot_coll_dist' in L.emu_validate(C.byref(bad))  # contact pickup needs the cubes as colliders
    assert L.emu_validate(C.byref(orc.default_config(K.HRL_ANT_GATHER, robot_coll_dist=0))) == b''
    bad = orc.default_config(K.HRL_ANT_MAZE, n_bins=1, sensor_span=3.0)
    assert b'n_bins' in L.emu_validate(C.byref(bad))  # the wall sensor would divide by n_bins - 1
    bad = orc.default_config(K.HRL_ANT_MAZE, sense_walls=0, sense_target=1, sensor_span=0.0)
    assert b'sensor_span' in L.emu_validate(C.byref(bad))
    bad = orc.default_config(K.HRL_ANT_MAZE, n_targets=0)
    assert b'n_targets' in L.emu_validate(C.byref(bad))
    assert L.emu_validate(C.byref(orc.default_config(K.HRL_ANT_MAZE))) == b''
    assert L.emu_lds_bytes() <= 10240  # 16 waves per CU x 10 KB <= 160 KB LDS


def test_product_defaults_equal_oracle_defaults():
    import ctypes as C
    for kind in KINDS:
        a = K.hrl_config(); emu_env.lib().emu_default_config(kind, C.byref(a))
        assert bytes(a) == bytes(orc.default_config(kind))
        assert emu_env.lib().emu_obs_dim(C.byref(a)) == orc.obs_dim(a) == {0: 29, 1: 46, 2: 38, 3: 18, 4: 60, 5: 28}[kind]


# the emulator's own order of tests/parity_cases.py::CONFIG_MATRIX (the collected ids carry the position): the 25 entries it has always run, then the
# 11 that only the device ran
EMU_ORDER = [31, 1, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 17, 8, 19, 20, 32, 33, 34, 25, 35, 27, 28, 29, 30, 0, 2, 3, 7, 9, 18, 21, 22, 23, 24, 26]


@pytest.mark.parametrize('kind,n,kw', [(P.CONFIG_MATRIX[i][0], P.CONFIG_MATRIX[i][1], P.CONFIG_MATRIX[i][3]) for i in EMU_ORDER])
def test_non_default_configs_bit_exact(kind, n, kw):
    P.config_matrix(make, kind, n, kw)


@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER])
def test_item_cubes_collide_and_contact_pickup(kind):
    """The food / poison cubes are static boxes (food.xml:12,19): robots parked on top of / next to cubes are pushed by
    them, and with robot_coll_dist <= 0 every contact point with a cube pays +-1 and moves it (ant_gather_env.py:113-116).
    Both lane orders of the wave phases equal the oracle bit for bit."""
    P.item_cubes(make, kind, 32, 30, need={})
    P.item_cubes(make, kind, 32, 30, need=dict(paid=21, touched=21), robot_coll_dist=0.0)
    P.item_cubes(make, kind, 32, 30, need=dict(paid=21, touched=21), robot_coll_dist=0.0, use_sensor=0)
    P.cubes_matter_to_the_physics(kind, 32)


def test_pointbot_cube_corners_against_the_turned_player_box_bit_exact():
    """The second half of the player-vs-cube contacts (the cube's corners against the player's oriented box, orc_impl.h
    orc_point_substep): players turned by any yaw and slightly tipped, parked so that cubes sit under the middle of a face, under
    the body or beside an edge; both lane orders of the wave phases equal the oracle bit for bit, and such contacts do occur."""
    import ctypes as C
    n = 48
    cfg = orc.default_config(K.HRL_POINT_GATHER, num_envs=n, seed=21, auto_reset=1, robot_coll_dist=0.0)
    o, e, er = orc.OracleEnv(cfg, np.float32), Emu(cfg), Emu(cfg, reverse=True)
    o.reset(); e.reset(); er.reset()
    rng = np.random.RandomState(6)
    face_only = 0
    for t in range(40):
        if t % 2 == 0:
            k = rng.randint(0, 16, n)
            ang = rng.uniform(-np.pi, np.pi, n); dist = rng.uniform(0.0, 0.62, n)
            xy = o.items.reshape(n, 16, 2)[np.arange(n), k] + (np.stack([np.cos(ang), np.sin(ang)], 1) * dist[:, None]).astype(np.float32)
            yaw = rng.uniform(-np.pi, np.pi, n); tip = rng.uniform(-0.05, 0.05, (n, 2))
            quat = np.stack([tip[:, 0], tip[:, 1], np.sin(yaw / 2), np.cos(yaw / 2)], 1); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
            for env in (o, e, er):
                env.state[:, 0:2] = xy; env.state[:, 3:7] = quat.astype(np.float32)
            # contacts that only the cube's corners can make: the oracle sees contacts with this cube, yet no player corner is near it
            for i in range(0, n, 4):
                q = o.state[i, :7].astype(np.float64); info = np.zeros(3, np.int32)
                c0 = orc.default_config(K.HRL_POINT_GATHER, num_envs=1, seed=0)
                orc.lib().orc_point_substeps_items_f64(C.byref(c0), orc.ptr(q.copy()), orc.ptr(np.zeros(6)), orc.ptr(np.zeros(3)), 1,
                                                      orc.ptr(o.items[i].astype(np.float64)), 16, orc.ptr(info))
                R = np.array([[np.cos(yaw[i]), -np.sin(yaw[i])], [np.sin(yaw[i]), np.cos(yaw[i])]])
                corners = q[:2] + (R @ (np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]]).T * 0.35)).T
                far = np.all(np.abs(corners - o.items.reshape(n, 16, 2)[i, k[i]]).max(1) > 0.125 + 0.06)
                face_only += int(info[1] > 0 and far)
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        o.step(a); e.step(a); er.step(a)
        same(o, e, t); same(e, er, (t, 'lane order'))
    assert face_only > 10, face_only


def test_self_collision_rows_bit_exact_and_keep_legs_apart():
    """Hips forced far beyond their +-40 degree range so that capsules of different legs meet (within the range they
    cannot: step_core.h broad phase): the two-body rows of the wave phases equal the oracle's bit for bit in both lane
    orders, and the contacts push the legs apart again (with self-collision off they stay interpenetrated longer)."""
    P.self_collision(make, 48, 25, stride=8, need=dict(seen=10), auto_reset=0)


def test_self_collision_broad_phase_is_exact():
    """The wave phases skip the 48 capsule pairs while every |hip angle| <= 0.75 rad and |ankle angle| <= 2 rad; the oracle
    always tests them.  On random poses inside those bounds (any torso orientation) the oracle never finds a pair within
    reach; just outside the ankle bound it does (a foot folded back over the torso)."""
    import ctypes as C
    cfg = orc.default_config(K.HRL_ANT_FLAT)
    rng = np.random.RandomState(8)
    for i in range(4000):
        q = np.zeros(15); q[2] = 5.0
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(-3.1, 3.1)
        q[3:6], q[6] = ax * np.sin(ang / 2), np.cos(ang / 2)
        q[7::2] = rng.choice([-0.75, 0.75, 0.0], 4) if i % 3 == 0 else rng.uniform(-0.75, 0.75, 4)
        q[8::2] = rng.choice([-2.0, 2.0], 4) if i % 5 == 0 else rng.uniform(-2.0, 2.0, 4)
        info = np.zeros(3, np.int32); dbg = np.zeros(13, np.int32)
        orc.lib().orc_ant_substeps_items_f64(C.byref(cfg), orc.ptr(q), orc.ptr(np.zeros(14)), orc.ptr(np.zeros(8)), 1, None, 0, orc.ptr(info), orc.ptr(dbg), None)
        assert dbg[0] == 0 and info[2] == 0, (i, q[7:], dbg)
    found = 0
    for i in range(300):  # outside the ankle bound a foot can fold back over the torso onto another leg
        q = np.zeros(15); q[2] = 5.0; q[6] = 1
        q[7::2] = rng.uniform(-0.75, 0.75, 4); q[8::2] = rng.uniform(2.2, 3.1, 4) * rng.choice([-1, 1], 4)
        orc.lib().orc_ant_substeps_items_f64(C.byref(cfg), orc.ptr(q), orc.ptr(np.zeros(14)), orc.ptr(np.zeros(8)), 1, None, 0, orc.ptr(info), orc.ptr(dbg), None)
        found += int(dbg[0] > 0)
    assert found > 0


def test_flagrun_manual_goals():
    """manual_goal_creation (ant_flagrun_env.py:27,150-153): reset draws no goal; `env.goals = [...]; env.next_target()` comes
    through hrl_set_goals (emu_set_goals here): as in the reference the list is consumed from its BACK (`goals.pop()`, :116) and
    the episode ends when it runs out; next_target() alone (hrl_next_target) pops one more, IndexError -> ok = 0."""
    P.flagrun_manual_goals(make, 8, 3, skip=None, auto_reset=0)


def test_flagrun_manual_close_targets():
    """manual_goal_creation with max_targets < 1 (ant_flagrun_env.py:113-114): next_target() -- from step() on reaching the goal /
    timing out, or from outside -- draws a goal near the robot whatever env.goals holds; reset() draws nothing (:150-153) and
    the episode never runs out of goals.  hrl_set_goals is refused there (the list would never be read)."""
    P.flagrun_manual_close_targets(make, 8, 14, REFUSED, seed=9, auto_reset=0, flag_timeout=4)


def test_flagrun_open_field_and_no_switch_on_collision():
    """ant_flagrun_env.py:59-64 `enclosed=False` (and no sensor): upstream's stadium scene, no walls -- an ant beyond where the
    arena's walls would stand meets nothing lateral; :183-194 `switch_flag_on_collision=False`: reaching the goal pays the +5000
    once and keeps the goal until the timeout moves it."""
    P.flagrun_open_field_and_no_switch(make, 8, auto_reset=0)


def test_reset_potential_is_taken_before_the_target_switch():
    """ant_flagrun_env.py:116 / ant_maze_bullet_env.py:111: the potential a reset leaves behind belongs to the PREVIOUS
    target (first episode: upstream's default walk target (1e3, 0)), so the first step's `progress` carries the jump."""
    dt = np.float32(0.0165 / 4) * 4
    for kind, kw in ((K.HRL_ANT_FLAGRUN, dict()), (K.HRL_ANT_MAZE, dict(inner_rew_weight=1.0)), (K.HRL_ANT_MAZE_MJ, dict(inner_rew_weight=1.0))):
        cfg = orc.default_config(kind, num_envs=6, seed=2, auto_reset=0, **kw)
        o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
        o.reset(); e.reset()
        same(o, e, 'reset 1')
        pot1 = o.state[:, 31].copy()
        assert np.all(np.abs(pot1 * dt + 1000) < 8)   # distance to (1e3, 0) from the start area
        a = np.zeros((6, 8), np.float32)
        o.step(a); e.step(a)
        same(o, e, 'step 1')
        assert np.all(o.rew > 5e4)                    # the reference's first-step jump (~ +6e4)
        o.reset(); e.reset()
        same(o, e, 'reset 2')
        assert np.all(np.abs(o.state[:, 31] * dt) < 20)  # second episode: against the previous episode's goal / target


def test_specified_transcendentals_accuracy_and_agreement():
    """sin / cos / atan2 / asin of DESIGN.md 3.7: the product's and the oracle's implementations agree bit for bit, and both are
    within a few 1e-7 of the exact functions (what the fp32 observations inherit)."""
    import ctypes as C
    rng = np.random.RandomState(0)
    n = 400000
    def run(which, a, b=None):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(a if b is None else b, np.float32)
        o1 = np.zeros(len(a), np.float32); o2 = np.zeros(len(a), np.float32)
        orc.lib().orc_spec_math_f32(which, orc.ptr(a), orc.ptr(b), orc.ptr(o1), len(a))
        emu_env.lib().emu_spec_math(which, orc.ptr(a), orc.ptr(b), orc.ptr(o2), len(a))
        assert np.array_equal(o1, o2, equal_nan=True)
        return o1.astype(np.float64)
    x = rng.uniform(-20, 20, n)
    assert np.abs(run(0, x) - np.sin(x.astype(np.float32).astype(np.float64))).max() < 2e-7
    assert np.abs(run(1, x) - np.cos(x.astype(np.float32).astype(np.float64))).max() < 2e-7
    yy = np.concatenate([rng.normal(size=n), 10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n), [0, 0, 1, -1, 0.0, 3, -3]]).astype(np.float32)
    xx = np.concatenate([rng.normal(size=n), 10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1, 1], n), [0, 1, 0, 0, -1.0, 3, -3]]).astype(np.float32)
    assert np.abs(run(2, yy, xx) - np.arctan2(yy.astype(np.float64), xx.astype(np.float64))).max() < 3.5e-7
    s = rng.uniform(-0.99999, 0.99999, n).astype(np.float32)
    assert np.abs(run(3, s) - np.arcsin(s.astype(np.float64))).max() < 3e-7
    run(2, np.array([np.nan, 1, np.inf, -np.inf, np.inf], np.float32), np.array([1, np.nan, 1, np.inf, np.inf], np.float32))  # same bits, whatever they are


@pytest.mark.parametrize('auto_reset', [1, 0])
@pytest.mark.parametrize('kind', KINDS)
def test_envs_that_blow_up_match_too(kind, auto_reset):
    """Non-finite and absurd states -- velocities of 1e20 and inf, a NaN coordinate, a torso 1e19 m away, robots inside a wall, joint angles far
    out of range -- go through the same arithmetic in the wave phases and in the oracle: NaN, inf, done, the dying cost and the auto-reset that
    follows come out identical (NaNs compared as equal)."""
    P.blow_up(make, kind, 64, auto_reset)


@pytest.mark.parametrize('kind', KINDS)
def test_fuzzed_absurd_values_stay_bit_exact(kind):
    """tests/tools/fuzz_parity.py: NaN, +-inf, 1e20, 3e38, denormals and signed zeros written into positions, velocities, item coordinates and actions
    of running envs; every output of the wave phases equals the oracle's at every step (this found a cube at a NaN place being everywhere for the
    oracle and nowhere for the phases)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('fuzz_parity', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'fuzz_parity.py'))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    for seed in (0, 1):
        for ar in (0, 1):
            assert fz.run(fz.EmuSide, kind, seed, ar) is None


@pytest.mark.parametrize('kind', KINDS)
def test_terminal_observation_and_truncation_flag(kind):
    """ABI v6: `final_obs` = the observation of the step that ended an episode (what the reference's step() returns there,
    ant_gather_env.py:96,118-119, ant_maze_bullet_env.py:82,97) and `truncated` = ended by the step limit alone (gym TimeLimit:
    info['TimeLimit.truncated'] = not done).  Property, on the oracle: an auto-resetting env with a step limit against a twin without reset
    and without limit stepped from the same pre-step records -- the twin's observation IS the terminal one, its done the env's own.
    Then the wave phases (both lane orders) equal the oracle bit for bit, final_obs / truncated included (same())."""
    P.terminal_observation(make, kind, 24, 4, need=dict(n_trunc=20, n_term=5, n_both=1))


@pytest.mark.parametrize('kind,kw', [
    (K.HRL_ANT_GATHER, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_POINT_GATHER, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_ANT_GATHER, dict(n_food=40, n_poison=24, n_bins=64, robot_coll_dist=0.0)),
    (K.HRL_POINT_GATHER, dict(n_food=40, n_poison=24, n_bins=30, robot_coll_dist=-1.0)),
])
def test_more_than_16_items(kind, kw):
    """n_food + n_poison > 16 (ant_gather_env.py:16-17 takes any counts): the longer items record, the 16-item slices of the packed
    contact phase, the wider item field of the respawn key and the item codes beyond the capsule pairs.  Robots are parked at every slot in
    turn so that the items past the 16th (and past the 48th) are picked up, touched and sensed; both lane orders equal the oracle."""
    P.more_than_16_items(make, kind, 32, 36, need=dict(moved_hi=10, paid=20), **kw)


def test_manual_goal_lists_longer_than_15():
    """manual_goal_creation with flag_goal_capacity = 40 (`env.goals = [...]` takes any list, ant_flagrun_env.py:45): the pending list lives in a
    longer items record; 40 goals are consumed back to front, one per 3-step timeout."""
    P.manual_goal_lists_longer_than_15(make, 6, REFUSED, auto_reset=0)


def test_next_target_pops_the_shared_list_of_a_non_manual_env():
    """`env.next_target()` called from outside on a NON-manual env (ant_flagrun_env.py:112-116): `self.goals.pop()` of the list reset() made --
    here: the goal counter of the episode advances --, ok = 0 (IndexError in the reference) once max_targets goals are used up."""
    import ctypes as C
    n = 9
    cfg = orc.default_config(K.HRL_ANT_FLAGRUN, num_envs=n, seed=4, auto_reset=0, flag_max_targets=3)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    o.reset(); e.reset()
    mask = np.ones(n, np.uint8); mask[::4] = 0
    for k in range(4):
        ok_o, ok_e = o.next_target(mask), e.next_target(mask)
        same(o, e, k)
        assert np.array_equal(ok_o, ok_e) and np.all(ok_o[mask == 0] == 1) and np.all(ok_o[mask == 1] == (1 if k < 2 else 0))
        assert np.all((o.aux[mask == 1, 3] & 0xffff) == min(2 + k, 3)) and np.all((o.aux[mask == 0, 3] & 0xffff) == 1)
    a = np.zeros((n, 8), np.float32)
    o.step(a); e.step(a)
    same(o, e, 'step')


def test_random_legal_configs():
    """tests/tools/fuzz_configs.py, a slice of it: every constructor argument and engine parameter drawn at random (biased to the edges of the capacity
    ranges), teleports / masked resets / manual goals between the steps; the wave phases equal the oracle bit for bit after every step.
    (This fuzzer is what found that with robot_coll_dist <= 0 and use_sensor=0 the observation held the positions of touched items AFTER their
    move; the hand-picked matrix had both branches, never together.)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
    import fuzz_configs as F
    ended = 0
    for seed in range(5000, 5016):
        for kind in F.KINDS:
            r, e = F.run(F.EmuSide, kind, seed * 16 + kind, 25)
            assert r is None, r
            ended += e
    assert ended > 1000


def test_capsule_mid_sections_against_cubes_and_the_maze_box():
    """assets/ant.xml:16-55 capsules against assets/food.xml:12 cubes and the assets/box.xml:12 maze box: ants let down onto cubes with the
    MIDDLE of their feet (contact pickup, ant_gather_env.py:113-116: the touch is paid) and feet laid across the vertical edges of the maze
    box -- contacts no end-point sphere sees; wave phases == oracle bit for bit."""
    P.capsule_mid_sections(make, 32, rounds=6, steps=2, stride=4, need=dict(mid=20, paid=60, mid_box=25))


def test_feet_contact_flags_show_the_previous_step():
    """Upstream WalkerBaseBulletEnv.step (recalled): `state = robot.calc_state()` comes BEFORE the loop that refreshes
    `robot.feet_contact` from the step's contacts, so obs[22:26] of AntMaze / obs[24:28] of AntFlagrun are the flags of the step before
    (zeros in the first step after a reset: robot_specific_reset); AntGather never refreshes them (ant_gather_env.py:105-111).  The flags of
    a step ride in bits 28..31 of aux[1]."""
    for kind, lo in ((K.HRL_ANT_MAZE, 22), (K.HRL_ANT_FLAGRUN, 24)):
        cfg = orc.default_config(kind, num_envs=6, seed=2, auto_reset=1, max_episode_steps=30)
        o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
        o.reset(); e.reset()
        assert np.all(o.obs[:, lo:lo + 4] == 0) and np.all((o.aux[:, 1].view(np.uint32) >> 28) == 0)
        seen = 0
        for t in range(70):
            before = (o.aux[:, 1].view(np.uint32) >> 28) & 0xf
            a = np.zeros((6, 8), np.float32)
            o.step(a); e.step(a)
            assert np.array_equal(o.obs, e.obs, equal_nan=True) and np.array_equal(o.aux, e.aux)
            cont = o.done == 0   # an env that ended was reset in place: its row is the next episode's first observation, flags 0
            want = ((before[:, None] >> np.arange(4)) & 1).astype(np.float32)
            assert np.array_equal(o.obs[cont, lo:lo + 4], want[cont]) and np.all(o.obs[~cont, lo:lo + 4] == 0)
            assert np.all(((o.aux[~cont, 1].view(np.uint32) >> 28) & 0xf) == 0)
            assert np.all((o.aux[:, 1] & 0x0fffffff) == t + 1)   # the lifetime count underneath
            seen += int(want.sum())
        assert seen > 200   # standing ants: feet on the floor most of the time
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=4, seed=2, auto_reset=1)
    o = orc.OracleEnv(cfg, np.float32); o.reset()
    for t in range(20):
        o.step(np.zeros((4, 8), np.float32))
    assert np.all(o.obs[:, 22:26] == 0) and np.all(o.aux[:, 1] == 20)


def test_flagrun_path_reward_switched_on_for_a_live_env():
    """`AntFlagrunBulletEnv.path_rew_weight = 0.5` while an env runs (ant_flagrun_env.py:158,174-176): set_target() has kept `_goal_start_pos` and
    `_sq_dist_goal` all along (:98-103), so the very next step pays a finite path reward measured from where the robot stood when it got its
    CURRENT goal.  Every flagrun env keeps both in its items record whatever the weight is -- with the bookkeeping tied to the weight the record
    of a default env was all zeros and the first steps after the switch paid +-inf (x / 0) until the next goal or reset."""
    n = 12
    cfg = orc.default_config(K.HRL_ANT_FLAGRUN, num_envs=n, seed=9, auto_reset=1, flag_timeout=25, max_episode_steps=2000)
    o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
    o.reset(); e.reset()
    assert np.all(o.items[:, K.HRL_FLAG_SQDIST_OFF] >= 0.25) and np.all(o.items[:, K.HRL_FLAG_START_OFF:K.HRL_FLAG_START_OFF + 2] == 0)   # goals >= 0.5 from the start (:71-78)
    rng = np.random.RandomState(1)
    checked = 0
    for t in range(90):
        if t == 33:   # mid-episode, between two goal switches
            cfg.flag_path_rew_weight = 0.5
        if t == 70:   # off and on again: the start position is the CURRENT goal's, not a stale one
            cfg.flag_path_rew_weight = 0.0
        if t == 75:
            cfg.flag_path_rew_weight = 0.5
        xy0, start, sqd = o.state[:, 0:2].copy(), o.items[:, 2:4].copy(), o.items[:, 4].copy()
        goal = np.zeros((n, 2), np.float32)
        for i in range(n):
            orc.lib().orc_flag_goal_f32(C.byref(cfg), int(o.aux[i, 2]), int(o.aux[i, 3] & 0xffff), orc.ptr(goal[i]))
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        o.step(a); e.step(a)
        for name in ('state', 'items', 'aux', 'obs', 'rew', 'done', 'info', 'goal'):
            assert np.array_equal(getattr(o, name), getattr(e, name), equal_nan=True), (t, name)
        assert np.all(np.isfinite(o.rew)), (t, o.rew)
        keep = (o.done == 0) & (o.goal[:, 2] == 0) & (o.rew < 1000)   # the rows whose record was not rewritten by this step (no switch, no reset, no goal reward)
        xy = o.state[:, 0:2].astype(np.float64)
        path = ((xy - start) * (goal.astype(np.float64) - start)).sum(1) / sqd
        want = (o.info[:, 0].astype(np.float64) + o.info[:, 1]) + cfg.flag_path_rew_weight * path
        assert np.allclose(o.rew[keep], want[keep], rtol=1e-5, atol=1e-4), (t, o.rew[keep], want[keep])
        if cfg.flag_path_rew_weight:
            checked += int(keep.sum())
            assert not keep.any() or np.abs(path[keep]).max() < 50
    assert checked > 300


def test_straggler_threshold_follows_the_model():
    """DevCfg::hot_rows (host_cfg.h::standing_rows): the solver rows of an ant that STANDS under the config -- its feet's contacts x 3 as far as the
    contact cap lets them in, one limit row per joint at its stop, two where the margin spans the joint's whole range -- is what ant_env_block compares an
    env's rows with (scheduling only).  20 at the defaults, the literal of round 5."""
    L = emu_env.lib()
    for kind in (K.HRL_ANT_FLAT, K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN):
        assert L.emu_hot_rows(C.byref(orc.default_config(kind, num_envs=4))) == 20
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=4, model_max_contacts=2)
    assert L.emu_hot_rows(C.byref(cfg)) == 6 + 8
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=4, model_limit_margin=1.3)   # spans the ankles' 70 degrees, not the hips' 80
    assert L.emu_hot_rows(C.byref(cfg)) == 12 + 4 + 8
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=4, model_limit_margin=1.5)
    assert L.emu_hot_rows(C.byref(cfg)) == 12 + 16
    # ... and that is what an ant standing on its four feet holds AT MOST (all eight joints at their stops): the settled population under random
    # torques reaches it and does not pass it -- an env above it has more than its feet on something
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=128, seed=1, auto_reset=1)
    o = orc.OracleEnv(cfg, np.float32); o.reset()
    rng = np.random.RandomState(0)
    for t in range(200):
        o.step(rng.uniform(-1, 1, (128, 8)).astype(np.float32))
    rows = []
    for t in range(20):
        o.solver_rows[:] = 0
        o.step(rng.uniform(-1, 1, (128, 8)).astype(np.float32))
        rows.append(o.solver_rows / 4.0)
    rows = np.concatenate(rows)
    assert np.percentile(rows, 95) <= 20.0 and np.percentile(rows, 90) >= 19.0 and (rows > 20).mean() < 0.02, np.percentile(rows, [50, 90, 95, 99])


def test_second_support_points_of_capsules_lying_flat_on_a_box_face():
    """A capsule that rests flat on a face of the maze box (assets/box.xml:12) or on the top of an item cube (assets/food.xml:12) gets a SECOND support
    point (Bullet keeps a manifold there; with one point the capsule rocks): feet hanging alongside the box's vertical faces, legs stretched out level
    over cubes -- states full of such contacts, counted; wave phases == oracle bit for bit, the contact cap included."""
    P.second_support_points(make, 32, rounds=4, stride=1, maze=[(0, 12, dict(seconds=60)), (0, 5, dict(seconds=10))],
                            gather=[(0, dict(seconds=100, paid=60))])


def test_observe_shows_the_feet_flags_the_last_step_left():
    """hrl_observe (include/hrl_envs.h): the feet-contact entries of an AntMaze / AntFlagrun observation are what robot.feet_contact holds in the reference at
    that point -- the flags the LAST step left (bits 28..31 of aux[1]), zeros right after a reset; a replay that wants zeros clears the bits with the
    state it writes.  Wave phases == oracle, and both == the bits."""
    for kind, lo in ((K.HRL_ANT_MAZE, 22), (K.HRL_ANT_FLAGRUN, 24)):
        cfg = orc.default_config(kind, num_envs=8, seed=3, auto_reset=0, max_episode_steps=0)
        o, e = orc.OracleEnv(cfg, np.float32), Emu(cfg)
        o.reset(); e.reset()
        o.observe(); e.observe()
        assert np.array_equal(o.obs, e.obs) and np.all(o.obs[:, lo:lo + 4] == 0)
        for t in range(30):
            o.step(np.zeros((8, 8), np.float32)); e.step(np.zeros((8, 8), np.float32))
        bits = (o.aux[:, 1].view(np.uint32) >> 28) & 0xf
        want = ((bits[:, None] >> np.arange(4)) & 1).astype(np.float32)
        assert want.sum() >= 8   # standing ants: feet on the floor
        o.obs[...] = -7; e.obs[...] = -7
        o.observe(); e.observe()
        assert np.array_equal(o.obs, e.obs) and np.array_equal(o.obs[:, lo:lo + 4], want)
        o.aux[:, 1] &= 0x0fffffff; e.aux[...] = o.aux   # the replay's way to zeros
        o.observe(); e.observe()
        assert np.array_equal(o.obs, e.obs) and np.all(o.obs[:, lo:lo + 4] == 0)


# ------------------------------------------------------------------ directed scenarios for branches no rollout enters (tests/STEP_COVERAGE.md)
ANT_N, POINT_N = 5, 3   # one group of four plus a ragged one; the point bot


@pytest.mark.parametrize('kind', [K.HRL_ANT_FLAT, K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN, K.HRL_POINT_GATHER])
def test_gimbal_lock(kind):
    point = kind == K.HRL_POINT_GATHER
    P.gimbal_lock(make, kind, POINT_N if point else ANT_N, need=dict(exact=3, band=3, control=3) if point else dict(exact=6, band=6, control=3))


@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER, K.HRL_ANT_MAZE])
def test_angle_wraps_and_bin_edges(kind):
    P.angle_wraps_and_bin_edges(make, kind, POINT_N if kind == K.HRL_POINT_GATHER else ANT_N,
                                need=dict(tiny_negative=2, two_pi_or_more=1, below_minus_pi=1, top_edge=1, last_bin=1, lit=4, last_bin_lit=1))


@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER])
def test_nan_item_in_the_nearest_first_order(kind):
    point = kind == K.HRL_POINT_GATHER
    P.nan_item_in_the_nearest_first_order(make, kind, POINT_N if point else ANT_N, need=dict(nan_types=2 if point else 4, clean=1))


def test_collinear_segments():
    P.collinear_segments(make, ANT_N, need=dict(p2=1, q2=1, p1=2, collinear_apart=4, apart=1))


@pytest.mark.parametrize('kind', [K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ])
def test_target_index_outside_the_table(kind):
    P.target_index_outside_the_table(make, kind, ANT_N)


@pytest.mark.parametrize('auto_reset', [0, 1])
@pytest.mark.parametrize('kind', KINDS)
def test_time_limit_on_the_terminal_step(kind, auto_reset):
    P.time_limit_on_the_terminal_step(make, kind, POINT_N if kind == K.HRL_POINT_GATHER else ANT_N, auto_reset)


@pytest.mark.parametrize('kind', [K.HRL_ANT_FLAT, K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ])
def test_null_items(kind):
    P.null_items(make, kind, ANT_N)


@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER, K.HRL_ANT_FLAGRUN])
def test_sixty_four_redraws(kind):
    n = POINT_N if kind == K.HRL_POINT_GATHER else ANT_N
    P.sixty_four_redraws(make, kind, n, need=dict(exhausted=n))


@pytest.mark.parametrize('kind', KINDS)
def test_optional_outputs_may_be_null(kind):
    """final_obs, truncated, goal and solver_rows are optional in the buffer record (include/hrl_envs.h): a step without them -- through the time limit's
    in-step reset -- computes everything else as the oracle does (the device's side of this: test_terminal_observation_and_truncation_flag there)"""
    n = ANT_N
    over = dict(num_envs=n, seed=3, auto_reset=1, max_episode_steps=3)
    o, e = orc.OracleEnv(orc.default_config(kind, **over), np.float32), Emu(Emu.config(kind, **over))
    o.reset(); e.reset()
    e.final_obs = e.truncated = e.goal = e.solver_rows = None
    rng = np.random.RandomState(2)
    for t in range(4):
        a = P.uniform(rng, n, o.ad)
        o.step(a); e.step(a)
        same(o, e, t, names=('state', 'items', 'aux', 'obs', 'rew', 'done', 'info'))
    assert o.aux[:, 2].min() >= 2


def test_crossing_capsule_axes():
    P.crossing_capsule_axes(make, ANT_N, need=dict(self_contacts=ANT_N, crossing=ANT_N))


def test_exhausted_goal_draws():
    P.exhausted_goal_draws(make, ANT_N)


def test_nan_robot_with_the_target_on_a_wall():
    P.nan_robot_with_the_target_on_a_wall(make, ANT_N, need=dict(q1=4, apart=3))
