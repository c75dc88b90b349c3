"""The parity scenarios, once: every function builds the fp32 oracle, drives it and the sides under test from ONE random stream, writes the
oracle's edited pre-step buffers into every side (push), compares all nine buffers of every side with the oracle's after every step bit for bit
(NaNs as equal) and counts from the oracle's buffers that the scenario reached what it is about.

`make(kind, count_rows=False, **over) -> [sides]` is the suite's factory (tests/backends.py): tests/test_emu_parity.py hands back the host executor
in both lane orders (the second is also compared with the first), tests/test_gpu_parity.py the device.  Sizes and the coverage thresholds
(`need`: counter -> least value) are the suite's own; a threshold is a condition on the inputs.  Test infrastructure only."""
import ctypes as C

import numpy as np
import pytest

import capsule_cases as cc
import orc
from backends import ALL, same
from hrl_pybullet_envs_amd import _capi as K

GATHER = (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER)

# (kind, envs on the emulator, envs on the device -- chosen to leave ragged groups of four --, constructor arguments)
CONFIG_MATRIX = [
    (K.HRL_ANT_GATHER, 5, 37, dict(n_bins=7, n_food=5, n_poison=3, sensor_range=9.0, sensor_span=2.0, world_size=(9.0, 11.0), centroid_static_sum=(-4.5, 0.0))),
    (K.HRL_ANT_GATHER, 4, 64, dict(respawn=0, robot_coll_dist=4.0, dying_cost=-3.0)),
    (K.HRL_ANT_GATHER, 5, 33, dict(use_sensor=0)),
    (K.HRL_POINT_GATHER, 6, 50, dict(n_bins=9, robot_object_spacing=3.0)),
    (K.HRL_ANT_MAZE, 6, 65, dict(sense_target=1, n_bins=8)),
    (K.HRL_ANT_MAZE, 5, 31, dict(target_encoding=1, sense_walls=0, tol=3.0, targ_dist_rew=1, max_steps=20, done_at_target=0)),
    (K.HRL_ANT_MAZE_MJ, 4, 40, dict(inner_rew_weight=0.5, n_bins=6)),
    (K.HRL_ANT_FLAGRUN, 4, 48, dict(use_sensor=1, n_bins=8, flag_timeout=9, flag_max_targets=3)),
    (K.HRL_ANT_FLAGRUN, 7, 21, dict(flag_max_targets=0, flag_max_target_dist=2.5, flag_timeout=6, flag_size=3.0, world_size=(5.0, 5.0), centroid_static_sum=(-2.5, 0.0))),
    (K.HRL_ANT_FLAT, 1, 1, dict()),
    (K.HRL_ANT_GATHER, 3, 3, dict(model_solver_iters=2, model_frame_skip=2, model_limit_margin=0.1)),
    (K.HRL_ANT_GATHER, 6, 40, dict(model_self_collision=0, model_item_collision=0)),
    # hrl_model of ABI v7, all on at once: Bullet's per-body damping (pybullet's 0.04 and a strong one), restitution, a tight contact cap, joint damping + armature
    (K.HRL_ANT_GATHER, 6, 66, dict(model_linear_damping=0.04, model_angular_damping=0.04, model_restitution=0.3, model_max_contacts=6, model_joint_damping=1.0, model_joint_armature=1.0)),
    (K.HRL_ANT_MAZE, 5, 35, dict(model_linear_damping=3.0, model_angular_damping=8.0, model_restitution_threshold=0.0, model_restitution=0.8)),
    (K.HRL_POINT_GATHER, 6, 46, dict(model_linear_damping=0.04, model_angular_damping=2.0, model_restitution=0.5, model_max_contacts=3)),
    (K.HRL_ANT_GATHER, 6, 70, dict(robot_coll_dist=0.0)),
    (K.HRL_POINT_GATHER, 6, 45, dict(robot_coll_dist=-1.0, respawn=0)),
    (K.HRL_ANT_MAZE, 5, 33, dict(inner_rew_weight=1.0)),
    (K.HRL_ANT_MAZE_MJ, 4, 17, dict(inner_rew_weight=1.0)),
    (K.HRL_ANT_FLAGRUN, 6, 35, dict(flag_enclosed=0, centroid_n_static=1, centroid_static_sum=(0.0, 0.0), flag_timeout=8, flag_max_targets=5)),  # ant_flagrun_env.py:59-64: open field
    (K.HRL_ANT_FLAGRUN, 6, 29, dict(flag_switch_on_collision=0, flag_timeout=7, flag_max_targets=4)),                                           # :183-194
    (K.HRL_ANT_FLAGRUN, 5, 19, dict(flag_manual_goals=1, flag_max_targets=0, flag_max_target_dist=3.0, flag_timeout=5)),                        # manual + close targets (:113-114)
    # constructor arguments beyond the caps of ABI <= 5 (ant_gather_env.py:16-29 takes any n_food / n_poison / n_bins, ant_maze_bullet_env.py:23-25 and
    # ant_maze_mj_env.py:50 any targets): more than 16 items (longer items record, 16-item slices in the packed contact phase, 6-bit item field of the
    # respawn key), observations wider than the wave (several packing / store passes), more than 8 targets
    (K.HRL_ANT_GATHER, 6, 70, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_POINT_GATHER, 6, 41, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_ANT_GATHER, 5, 37, dict(n_food=40, n_poison=24, n_bins=64, robot_coll_dist=0.0, world_size=(8.0, 8.0), centroid_static_sum=(-4.0, 0.0))),
    (K.HRL_POINT_GATHER, 5, 33, dict(n_food=33, n_poison=31, n_bins=40, robot_coll_dist=-1.0, world_size=(8.0, 8.0))),
    (K.HRL_ANT_GATHER, 5, 21, dict(n_food=20, n_poison=12, n_bins=24, use_sensor=0)),
    (K.HRL_ANT_MAZE_MJ, 4, 35, dict(n_bins=16)),
    (K.HRL_ANT_MAZE_MJ, 4, 18, dict(n_bins=64)),
    (K.HRL_ANT_MAZE, 6, 45, dict(sense_target=1, n_bins=33, targets=[(-2.0 + 0.5 * i, -4.0 + 0.1 * i) for i in range(12)], tol=0.7)),
    (K.HRL_ANT_FLAGRUN, 4, 22, dict(use_sensor=1, n_bins=40, flag_timeout=9)),
    # the entries the emulator's list held in another form than the device's (no centroid_static_sum; a 9 x 9 world)
    (K.HRL_ANT_GATHER, 5, 39, dict(n_bins=7, n_food=5, n_poison=3, sensor_range=9.0, sensor_span=2.0, world_size=(9.0, 11.0))),
    (K.HRL_ANT_GATHER, 6, 43, dict(n_food=20, n_poison=12, n_bins=24, world_size=(9.0, 9.0))),
    (K.HRL_POINT_GATHER, 6, 47, dict(n_food=20, n_poison=12, n_bins=24, world_size=(9.0, 9.0))),
    (K.HRL_ANT_GATHER, 5, 38, dict(n_food=40, n_poison=24, n_bins=64, robot_coll_dist=0.0, world_size=(8.0, 8.0))),
    (K.HRL_ANT_GATHER, 5, 23, dict(n_food=20, n_poison=12, n_bins=24, use_sensor=0, world_size=(9.0, 9.0))),
]


def start(make, kind, count_rows=False, **over):
    """the oracle and every side under test on one config, all reset"""
    o, sides = orc.OracleEnv(orc.default_config(kind, **over), np.float32), make(kind, count_rows=count_rows, **over)
    o.reset()
    for s in sides:
        s.reset()
    return o, sides


def check(o, sides, tag, names=ALL):
    for s in sides:
        same(o, s, tag, names)
    for s in sides[1:]:
        same(sides[0], s, (tag, 'lane order'), names)


def step(o, sides, a, tag, push=True, names=ALL):
    """one step of all from identical inputs: the oracle's state / items / aux as they stand (edited or not) go into every side first"""
    for s in sides:
        if push:
            s.push(o)
        s.step(a)
    o.step(a)
    check(o, sides, tag, names)


def covered(need, **count):
    assert all(count[k] >= v for k, v in need.items()), (count, need)


def uniform(rng, n, d, scale=1.0):
    return (rng.uniform(-1, 1, (n, d)) * scale).astype(np.float32)


def park_against_a_cube_face(o, rng, xy, lat_max, gap_max):
    """point bots at rest, unturned, with a face against the cube at `xy` (gap -4 mm .. gap_max) at any offset along that face: a player teleported
    INTO a cube is thrown out within a substep and touches nothing at the step's last collision pass"""
    n = o.N
    side = rng.randint(0, 4, n); d = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)[side]
    lat = rng.uniform(-lat_max, lat_max, n).astype(np.float32); gap = rng.uniform(-0.004, gap_max, n).astype(np.float32)
    o.state[:, 0:2] = xy - d * (np.float32(0.475) + gap)[:, None] + d[:, ::-1] * lat[:, None]
    o.state[:, 2] = 0.35; o.state[:, 3:7] = [0, 0, 0, 1]; o.state[:, 7:13] = 0


def reset(make, kind, n, every, **over):
    o, sides = start(make, kind, num_envs=n, **over)
    check(o, sides, 'reset')
    mask = np.zeros(n, np.uint8); mask[::every] = 1   # a masked reset touches only the selected envs
    s0 = o.state.copy()
    o.reset(mask)
    for s in sides:
        s.reset(mask)
    check(o, sides, 'masked reset')
    assert np.array_equal(o.state[mask == 0], s0[mask == 0]) and np.all(o.aux[mask == 1, 2] == 2) and np.all(o.aux[mask == 0, 2] == 1)


def free_running(make, kind, n, steps, stream, min_episodes, **over):
    """no state copying: every side runs on its own from the same seed"""
    o, sides = start(make, kind, num_envs=n, auto_reset=1, **over)
    rng = np.random.RandomState(stream)
    for t in range(steps):
        a = uniform(rng, n, o.ad)
        if kind == K.HRL_POINT_GATHER and t == 7:
            a[0] = 0  # point_bot.py:29 divides by |a| -> NaN -> done -> auto-reset
        step(o, sides, a, t, push=False)
    assert o.aux[:, 2].min() >= min_episodes


def gather_pickups(make, n, steps, need):
    o, sides = start(make, K.HRL_ANT_GATHER, num_envs=n, seed=11, auto_reset=1)
    rng = np.random.RandomState(5)
    picked = 0
    for t in range(steps):
        k = rng.randint(0, 16, n)   # every torso next to one of its items
        o.state[:, 0:2] = o.items.reshape(n, 16, 2)[np.arange(n), k] + rng.uniform(-0.6, 0.6, (n, 2)).astype(np.float32)
        step(o, sides, uniform(rng, n, 8), t)
        picked += int((o.info[:, 0] != 0).sum())
    covered(need, picked=picked)


def config_matrix(make, kind, n, kw):
    o, sides = start(make, kind, num_envs=n, seed=17, auto_reset=1, max_episode_steps=25, **kw)
    check(o, sides, 'reset')
    rng = np.random.RandomState(4)
    for t in range(60):
        if kw.get('flag_manual_goals') and t == 20:
            # a manual_goal_creation env that was never given a goal pays NaN, as the reference does (`_sq_dist_goal` is still the constructor's 0:
            # path_rew = 0 / 0, ant_flagrun_env.py:48,174-176) until its first goal; next_target() is the documented way to give it one
            for s in [o] + sides:
                s.next_target()
            check(o, sides, 'next_target')
        step(o, sides, uniform(rng, n, o.ad), t, push=False)


def item_cubes(make, kind, n, steps, need, turned=False, **kw):
    """robots teleported onto / next to cubes; with robot_coll_dist <= 0 every contact point with a cube pays +-1 and moves it.  `turned`: every other
    round the point bots stand at any yaw, slightly tipped, the cube under the body, under a face or beside an edge (contacts made by the CUBE's
    corners against the player's box) instead of parked against a face.  use_sensor=0: the observation holds the items' positions from BEFORE the
    step moved them (get_food_obs, ant_gather_env.py:95-96, precedes reward_collision, :113-116)."""
    o, sides = start(make, kind, num_envs=n, seed=13, auto_reset=1, **kw)
    rng = np.random.RandomState(2)
    paid = touched = moved = 0
    for t in range(steps):
        k = rng.randint(0, 16, n)
        off = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32) * (1.4 if kind == K.HRL_ANT_GATHER else 0.45)
        if 'robot_coll_dist' in kw:  # contact mode: nothing is picked up by distance, so stand right next to / on the cube
            cube = o.items.reshape(n, 16, 2)[np.arange(n), k]
            o.state[:, 0:2] = cube + off
            if kind == K.HRL_POINT_GATHER and not (turned and t % 2):
                park_against_a_cube_face(o, rng, cube, 0.42, 0.012)
            elif kind == K.HRL_POINT_GATHER:
                yaw = rng.uniform(-np.pi, np.pi, n); tip = rng.uniform(-0.05, 0.05, (n, 2))
                quat = np.stack([tip[:, 0], tip[:, 1], np.sin(yaw / 2), np.cos(yaw / 2)], 1); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
                o.state[:, 3:7] = quat.astype(np.float32); o.state[:, 2] = 0.35; o.state[:, 7:13] = 0
        a = uniform(rng, n, o.ad)
        it0 = o.items.copy()
        step(o, sides, a, t)
        paid += int((o.info[:, 0] != 0).sum()); touched += int(np.any(o.items != it0, axis=1).sum())
        if not o.cfg.use_sensor:   # 8 + 8 items, 10 / 5 slots per type: the food slots hold the nearest foods' OLD positions, whether or not they moved
            live = np.isfinite(o.obs).all(axis=1) & (o.done == 0)
            m = min(8, o.cfg.n_bins); nb = o.od - 4 * m
            for i in np.nonzero(live)[0]:
                old = it0[i, :16].reshape(8, 2)
                assert all(any(np.array_equal(f, q) for q in old) for f in o.obs[i, nb:nb + 2 * m].reshape(m, 2)), (t, i)
            moved += int(np.any(it0[live, :16] != o.items[live, :16], axis=1).sum())
    covered(need, paid=paid, touched=touched, moved=moved)


def cubes_matter_to_the_physics(kind, n):
    """(the oracle alone) the same rollout without the cubes as colliders diverges"""
    c1 = orc.default_config(kind, num_envs=n, seed=13, robot_coll_dist=0.0)
    c0 = orc.default_config(kind, num_envs=n, seed=13, robot_coll_dist=4.0, respawn=0, model_item_collision=0)
    o1, o0 = orc.OracleEnv(c1, np.float32), orc.OracleEnv(c0, np.float32)
    o1.reset(); o0.reset()
    # ant: the torso over the cube; point bot: one of its bottom corners over the cube (its contact points are the 8 corners)
    xy = o1.items.reshape(n, 16, 2)[:, 3] + np.float32(0.05 if kind == K.HRL_ANT_GATHER else 0.33)
    o1.state[:, 0:2] = xy; o0.state[:, 0:2] = xy; o0.items[...] = o1.items
    if kind == K.HRL_ANT_GATHER:
        o1.state[:, 2] = 0.4; o0.state[:, 2] = 0.4  # torso low enough to sit on the 0.225 m high cube
    a = np.zeros((n, o1.ad), np.float32) + np.float32(0.3)
    o1.step(a); o0.step(a)
    assert np.abs(o1.state[:, :15] - o0.state[:, :15]).max() > 1e-3


def self_collision(make, n, steps, stride, need, **over):
    """hips forced far beyond their +-40 degree range so that capsules of different legs meet (within the range they cannot: step_core.h broad phase)"""
    o, sides = start(make, K.HRL_ANT_FLAT, num_envs=n, seed=5, **over)
    rng = np.random.RandomState(1)
    seen = 0
    for t in range(steps):
        if t % 5 == 0:
            o.state[:, 2] = 1.5; o.state[:, 15:29] = 0
            o.state[:, 7:15:2] = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
            o.state[:, 8:15:2] = rng.uniform(-1.8, 1.8, (n, 4)).astype(np.float32)
        for i in range(0, n, stride):   # how many self contacts does the oracle see in these poses?
            q = o.state[i, :15].astype(np.float64); info = np.zeros(3, np.int32); dbg = np.zeros(13, np.int32)
            orc.lib().orc_ant_substeps_items_f64(C.byref(o.cfg), orc.ptr(q), orc.ptr(np.zeros(14)), orc.ptr(np.zeros(8)), 1, None, 0, orc.ptr(info), orc.ptr(dbg), None)
            seen += int((dbg[1:] >= 64).sum())
        step(o, sides, uniform(rng, n, 8), t)
    covered(need, seen=seen)   # sampled rows only: the rollouts really contain self contacts


def on_the_goal(xy, n_static, static_sum):
    """walk_target_dist is measured from the parts centroid (13 robot parts + the static bodies of the scene): the torso place that puts it on xy"""
    return (((13 + n_static) * xy - np.asarray(static_sum, np.float32)) / 13).astype(np.float32)


def flagrun_manual_goals(make, n, G, skip, **over):
    """manual_goal_creation (ant_flagrun_env.py:27,45,112-120,150-153): reset draws no goal; `env.goals = [...]; env.next_target()` comes through
    set_goals: as in the reference the list is consumed from its BACK (`goals.pop()`, :116) and the episode ends when it runs out; next_target()
    alone pops one more, IndexError -> ok = 0.  `skip`: every skip-th env is masked out of set_goals (None: no mask)."""
    o, sides = start(make, K.HRL_ANT_FLAGRUN, num_envs=n, seed=6, flag_manual_goals=1, flag_timeout=0, **over)
    every = [o] + sides
    check(o, sides, 'reset')
    assert np.all(o.items[:, 0] == 1000) and np.all(o.items[:, 1:] == 0) and np.all(o.aux[:, 3] == 0)  # upstream default walk target
    goals = np.random.RandomState(0).uniform(-4, 4, (n, G, 2)).astype(np.float32)
    mask = None
    if skip:
        mask = np.ones(n, np.uint8); mask[::skip] = 0
    given = np.ones(n, bool) if mask is None else mask == 1
    for s in every:
        s.set_goals(goals, mask)
    check(o, sides, 'set_goals')
    assert np.array_equal(o.items[given, 0:2], goals[given, G - 1]) and np.all((o.aux[given, 3] & 0xffff) == G - 1)  # the LAST goal first
    P0 = K.HRL_FLAG_PENDING_OFF
    assert np.array_equal(o.items[given, P0:P0 + 2 * (G - 1)], goals[given, :G - 1].reshape(given.sum(), -1))       # the rest, in list order
    rng = np.random.RandomState(1)
    visited = np.zeros(n, int); done_at = np.full(n, -1)
    for t in range(4 * G):
        # (the masked-out envs still chase (1e3, 0): teleported outside the arena they blow up to NaN on all sides alike)
        o.state[:, 0:2] = on_the_goal(o.items[:, 0:2], 2, (-6.0, 0.0)); o.state[:, 2] = 0.5
        step(o, sides, uniform(rng, n, 8), t)
        for i in np.nonzero(given & (done_at < 0))[0]:
            if o.rew[i] > 1000:
                visited[i] += 1
                if visited[i] <= G - 1 and not o.done[i]:
                    assert np.array_equal(o.items[i, 0:2], goals[i, G - 1 - visited[i]])  # back to front
            if o.done[i]:
                done_at[i] = t
    assert np.all(visited[given] >= G) and np.all(done_at[given] >= 0)  # all goals reached, then the episode ends for lack of goals
    # next_target() alone: the first half of the envs gets one more goal as plain data (env.goals = [g]), the others have an empty list (ok 0,
    # unchanged); env 1 is masked out; a second call finds every list empty
    extra = np.random.RandomState(3).uniform(-4, 4, (n, 2)).astype(np.float32)
    has = np.arange(n) < n // 2
    o.state[:, 0:3] = np.array([0.5, -0.5, 0.5], np.float32)
    o.items[has, P0:P0 + 2] = extra[has]; o.aux[:, 3] &= ~0xffff; o.aux[has, 3] |= 1
    for s in sides:
        s.push(o)
    mask = np.ones(n, np.uint8); mask[1] = 0
    kept = o.items[1, 0:2].copy()
    for rep in range(2):
        oks = [s.next_target(mask) for s in every]
        check(o, sides, ('next_target', rep))
        assert all(np.array_equal(oks[0], ok) for ok in oks[1:])
        assert np.array_equal(oks[0], np.where(mask == 0, 1, has & (rep == 0)))
        assert np.array_equal(o.items[has & (mask == 1), 0:2], extra[has & (mask == 1)]) and np.all((o.aux[:, 3] & 0xffff)[mask == 1] == 0)
    assert np.array_equal(o.items[1, 0:2], kept) and not np.array_equal(kept, extra[1])  # the masked-out env kept its target
    return o, sides


def flagrun_manual_close_targets(make, n, steps, refused, **over):
    """manual_goal_creation with max_targets < 1 (ant_flagrun_env.py:113-114): next_target() -- from step() on reaching the goal / timing out, or
    from outside -- draws a goal near the robot whatever env.goals holds; reset() draws nothing (:150-153) and the episode never runs out of
    goals.  set_goals is refused there (the list would never be read): pytest.raises(**refused)."""
    o, sides = start(make, K.HRL_ANT_FLAGRUN, num_envs=n, flag_manual_goals=1, flag_max_targets=0, flag_max_target_dist=3.0, **over)
    check(o, sides, 'reset')
    assert np.all(o.items[:, 0] == 1000) and np.all(o.aux[:, 3] == 0)
    for s in sides:
        with pytest.raises(**refused):
            s.set_goals(np.zeros((n, 2, 2), np.float32))
    oks = [s.next_target() for s in [o] + sides]
    check(o, sides, 'next_target')
    assert all(ok.all() for ok in oks) and np.all((o.aux[:, 3] & 0xffff) == 1)
    d = np.abs(o.items[:, 0:2] - o.state[:, 0:2])
    assert np.all(d >= 0.5 - 1e-6) and np.all(d <= 1.5 + 1e-6) and np.all(np.abs(o.items[:, 0:2]) < 5)   # +-U(tol, mtd / 2) per axis, inside the arena
    rng = np.random.RandomState(2)
    seen = [set() for _ in range(n)]
    for t in range(steps):
        step(o, sides, uniform(rng, n, 8), t, push=False)
        for i in range(n):
            seen[i].add(tuple(o.items[i, 0:2]))
    k = steps // o.cfg.flag_timeout   # the timeout retargets k times; nobody runs out of goals
    assert not o.done.any() and all(len(sx) >= k for sx in seen) and np.all((o.aux[:, 3] & 0xffff) >= k + 1)


def flagrun_open_field_and_no_switch(make, n, **over):
    """ant_flagrun_env.py:59-64 `enclosed=False` (and no sensor): upstream's stadium scene, no walls -- an ant beyond where the arena's walls would
    stand meets nothing lateral; :183-194 `switch_flag_on_collision=False`: reaching the goal pays the +5000 once and keeps the goal until the
    timeout moves it."""
    kw = dict(num_envs=n, seed=3, flag_switch_on_collision=0, flag_timeout=6, flag_max_targets=3, **over)
    o, sides = start(make, K.HRL_ANT_FLAGRUN, flag_enclosed=0, centroid_n_static=1, centroid_static_sum=(0.0, 0.0), **kw)
    ow = orc.OracleEnv(orc.default_config(K.HRL_ANT_FLAGRUN, **kw), np.float32)   # the walled arena, the oracle alone
    ow.reset()
    check(o, sides, 'reset')
    for env in (o, ow):   # astride the line x = 6 where the enclosed arena's wall stands (world 12 x 12), feet on the ground
        env.state[:, 0] = 6.0; env.state[:, 2] = 0.3
    rng = np.random.RandomState(0)
    for t in range(5):
        a = uniform(rng, n, 8)
        step(o, sides, a, ('open', t)); ow.step(a)
    assert np.isfinite(o.state).all() and np.all(np.abs(o.state[:, 0] - 6.0) < 0.5)   # nothing pushed it away
    assert np.abs(ow.state[:, 0] - o.state[:, 0]).max() > 0.05                         # the walled arena did
    o.reset()
    for s in sides:
        s.reset()
    paid = np.zeros(n, int); goals_seen = [set() for _ in range(n)]
    episode = o.aux[:, 2].copy()
    for t in range(14):
        g = np.zeros((n, 2), np.float32)
        for i in range(n):
            orc.lib().orc_flag_goal_f32(C.byref(o.cfg), int(o.aux[i, 2]), int(o.aux[i, 3] & 0xffff), orc.ptr(g[i:i + 1]))
            goals_seen[i].add(tuple(g[i]))
        o.state[:, 0:2] = on_the_goal(g, 1, (0.0, 0.0)); o.state[:, 2] = 0.5   # the stadium's floor at the origin is the one static body
        step(o, sides, uniform(rng, n, 8), ('noswitch', t))
        paid += (o.rew > 1000).astype(int)
    # on the goal every step: paid once per goal, the goal only moves with the 6-step timeout (14 steps -> 3 goals), never `done` for it; with
    # auto-reset an env whose third goal timed out is out of goals -> done -> a new episode with a new list: its first goal is a fourth
    seen = np.array([len(sx) for sx in goals_seen])
    assert np.all(paid == seen) and np.all(seen[o.aux[:, 2] == episode] == 3) and np.all((seen >= 3) & (seen <= 4)), (paid, goals_seen)


def blow_up(make, kind, n, auto_reset):
    """velocities of 1e20 and inf, NaN coordinates of the robot or of an item, a torso 1e19 m away, robots inside a wall, joint angles far out of range"""
    o, sides = start(make, kind, num_envs=n, seed=31, auto_reset=auto_reset)
    rng = np.random.RandomState(9)
    nq = 7 if kind == K.HRL_POINT_GATHER else 15
    for t in range(15):
        a = uniform(rng, n, o.ad)
        if t % 3 == 0:
            rows = rng.permutation(n)[:48]
            o.state[rows[0:8], 15 + rng.randint(0, 6, 8)] = 1e20
            o.state[rows[8:16], 15 + rng.randint(0, 6, 8)] = np.inf
            o.state[rows[16:24], 15 + rng.randint(0, 6, 8)] = -3e38
            o.state[rows[20:24], 15 + rng.randint(0, 6, 4)] = np.nan
            o.state[rows[24:28], 0] = 1e19
            o.state[rows[26:28], 1] = -np.inf
            o.state[rows[28:32], 2] = -1e19
            o.state[rows[32:36], rng.randint(0, nq, 4)] = np.nan
            o.state[rows[36:40], 0:2] = [-2.0, 0.0] if kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ) else [7.6, 7.6]  # inside the maze box / the walls
            if kind != K.HRL_POINT_GATHER:
                o.state[rows[40:48], 7 + rng.randint(0, 8, 8)] = rng.choice([40.0, -1e6, 3e30], 8)  # joint angles far out of range
            if kind in GATHER:  # item coordinates too
                o.items[rows[0:4], rng.randint(0, 32, 4)] = np.nan
                o.items[rows[4:8], rng.randint(0, 32, 4)] = np.inf
                o.items[rows[24:26], rng.randint(0, 32, 2)] = 1e30
        step(o, sides, a, t)


def terminal_observation(make, kind, n, n_edit, need):
    """Property, on the oracle: an auto-resetting env with a step limit against a twin without reset and without limit stepped from the same pre-step
    records -- the twin's observation IS the terminal one, its done the env's own.  Then every side equals the oracle, final_obs / truncated
    included; rows of live envs keep what they held (-7 to begin with)."""
    limit = 9
    kw = dict(flag_timeout=4, flag_max_targets=3) if kind == K.HRL_ANT_FLAGRUN else {}
    o, sides = start(make, kind, num_envs=n, seed=5, auto_reset=1, max_episode_steps=limit, **kw)
    twin = orc.OracleEnv(orc.default_config(kind, num_envs=n, seed=5, auto_reset=0, max_episode_steps=0, **kw), np.float32)
    o.final_obs[...] = -7.0
    for s in sides:
        s.fill('final_obs', -7.0)
    rng = np.random.RandomState(8)
    n_trunc = n_term = n_both = 0
    for t in range(40):
        if t % 4 == 3 or t % 9 == 8:   # some episodes end on their own -- a numerical failure ends any kind's (ant_gather_env.py:101-103,
            rows = rng.permutation(n)[:n_edit]   # gather_base.py:91-93), an ant held under 0.26 m dies --, some of them exactly at the step limit
            o.state[rows[:n_edit // 2], 15] = np.nan
            if kind != K.HRL_POINT_GATHER:
                o.state[rows[n_edit // 2:], 2] = 0.05; o.state[rows[n_edit // 2:], 17] = -3.0
        twin.state[...] = o.state; twin.items[...] = o.items; twin.aux[...] = o.aux
        a = uniform(rng, n, o.ad)
        keep = o.final_obs.copy()
        step(o, sides, a, t); twin.step(a)
        d = o.done.astype(bool)
        hit_limit = twin.aux[:, 0] >= limit
        assert np.array_equal(d, twin.done.astype(bool) | hit_limit)
        assert np.array_equal(o.truncated.astype(bool), hit_limit & ~twin.done.astype(bool))
        assert np.array_equal(o.final_obs[d], twin.obs[d], equal_nan=True)         # the terminal observation
        assert np.array_equal(o.final_obs[~d], keep[~d], equal_nan=True)            # rows of live envs are left alone
        assert np.array_equal(o.rew, twin.rew, equal_nan=True)
        assert not np.array_equal(o.final_obs[d], o.obs[d], equal_nan=True) or not d.any()   # obs itself is already the next episode's first
        n_trunc += int(o.truncated.sum()); n_term += int((d & ~o.truncated.astype(bool)).sum()); n_both += int((hit_limit & twin.done.astype(bool)).sum())
    covered(need, n_trunc=n_trunc, n_term=n_term, n_both=n_both)   # n_both: ended on its own AT the limit -> not truncated
    assert (o.final_obs != -7.0).any(axis=1).all()   # every env has ended at least once
    return o, sides, rng


def more_than_16_items(make, kind, n, steps, need, **kw):
    """robots parked at every slot in turn so that the items past the 16th (and past the 48th) are picked up, touched and sensed"""
    n_items = kw['n_food'] + kw['n_poison']
    o, sides = start(make, kind, num_envs=n, seed=19, auto_reset=1, **kw)
    assert orc.items_stride(o.cfg) == (64 if n_items == 32 else 128)
    check(o, sides, 'reset')
    assert np.all(o.items[:, 2 * n_items:] == 0) and np.all(np.abs(o.items[:, :2 * n_items]) <= 7.0) and np.all(o.items[:, 2 * n_items - 2:2 * n_items] != 0)
    contact = 'robot_coll_dist' in kw
    rng = np.random.RandomState(3)
    paid = moved_hi = 0
    for t in range(steps):
        k = (np.arange(n) * 2 + t * 5) % n_items        # every slot gets its turn
        it = o.items[:, :2 * n_items].reshape(n, n_items, 2)[np.arange(n), k]
        if contact and kind == K.HRL_POINT_GATHER:
            park_against_a_cube_face(o, rng, it, 0.3, 0.01)
        else:
            o.state[:, 0:2] = it + rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32) * np.float32(0.5 if not contact else 1.2)
        a = uniform(rng, n, o.ad)
        it0 = o.items.copy()
        step(o, sides, a, t)
        moved = np.any((o.items != it0).reshape(n, -1, 2), axis=2) & ~o.done.astype(bool)[:, None]
        moved_hi += int(moved[:, 16:n_items].sum()) if n_items <= 48 else int(moved[:, 48:n_items].sum())
        paid += int((o.info[:, 0] != 0).sum())
    covered(need, moved_hi=moved_hi, paid=paid)
    if not contact:   # the sensor sees the items past the 16th: with only those in range, readings are non-zero
        o2, sides2 = start(make, kind, num_envs=4, seed=1, **kw)
        o2.items[:, :32] = 90.0       # the first 16 far out of range
        o2.items[:, 32:2 * n_items:2] = o2.state[:, 0:1] + 3.0; o2.items[:, 33:2 * n_items:2] = o2.state[:, 1:2] + np.linspace(-2, 2, n_items - 16, dtype=np.float32)
        step(o2, sides2, np.zeros((4, o2.ad), np.float32) + np.float32(0.1), 'sensor')
        assert (o2.obs[:, (26 if kind == K.HRL_ANT_GATHER else 8):] > 0).any(axis=1).all()
    return o, sides


def manual_goal_lists_longer_than_15(make, n, refused, **over):
    """flag_goal_capacity = 40 (`env.goals = [...]` takes any list, ant_flagrun_env.py:45): the pending list lives in a 96-float items record; 40
    goals are consumed back to front, one per 3-step timeout; one goal beyond the capacity is refused: pytest.raises(**refused)."""
    G = 40
    o, sides = start(make, K.HRL_ANT_FLAGRUN, num_envs=n, seed=2, flag_manual_goals=1, flag_goal_capacity=G, flag_timeout=3, max_episode_steps=0, **over)
    assert orc.items_stride(o.cfg) == 96
    goals = np.random.RandomState(0).uniform(-4, 4, (n, G, 2)).astype(np.float32)
    for s in [o] + sides:
        s.set_goals(goals)
    check(o, sides, 'set_goals')
    assert np.array_equal(o.items[:, 0:2], goals[:, G - 1]) and np.all((o.aux[:, 3] & 0xffff) == G - 1)
    for s in sides:
        with pytest.raises(**refused):
            s.set_goals(np.zeros((n, G + 1, 2), np.float32))
    rng = np.random.RandomState(1)
    for t in range(3 * G + 2):
        step(o, sides, rng.uniform(-0.3, 0.3, (n, 8)).astype(np.float32), t, push=False)
        left, cur = G - 1 - (t + 1) // 3, o.aux[:, 3] & 0xffff   # one goal per timeout, sooner where a goal happens to be reached
        live = ~o.done.astype(bool) & (o.aux[:, 2] == 1)        # (an auto-reset env starts over without a list)
        assert np.all(cur[live] <= max(left, 0)) and np.array_equal(o.items[live, 0:2], goals[np.arange(n)[live], cur[live]]), t
    assert (o.done | (o.aux[:, 2] > 1)).all()    # every list ran out (IndexError in the reference, :193-194)
    return o, sides


def item_boxes(o, i):
    ni = o.cfg.n_food + o.cfg.n_poison
    it = o.items[i, :2 * ni].reshape(ni, 2).astype(np.float64)
    return {(16 + k if k < 48 else 64 + k): (np.r_[it[k] - 0.125, -0.025], np.r_[it[k] + 0.125, 0.225]) for k in range(ni)}


def capsule_mid_sections(make, n, rounds, steps, stride, need):
    """ants let down onto cubes with the MIDDLE of their feet (contact pickup: the touch is paid) and feet laid across the vertical edges of the
    maze box -- contacts no end-point sphere sees.  `stride`: every stride-th env (gather) / every (stride / 2)-th (maze) is counted."""
    rng = np.random.RandomState(8)
    o, sides = start(make, K.HRL_ANT_GATHER, num_envs=n, seed=4, auto_reset=1, robot_coll_dist=0.0)
    paid = mid = 0
    for t in range(rounds):
        cc.cubes_under_the_feet(o, rng)
        mid += cc.count_mid_section_contacts(o, range(0, n, stride), lambda i: item_boxes(o, i))
        for k in range(steps):
            step(o, sides, uniform(rng, n, 8, 0.0 if k == 0 else 0.3), (t, k))
            paid += int((o.info[:, 0] != 0).sum())
    o, sides = start(make, K.HRL_ANT_MAZE, num_envs=n, seed=4, auto_reset=1)
    box = {8: (np.array([-5., -2, 0]), np.array([1., 2, 2]))}
    mid_box = 0
    for t in range(rounds):
        cc.foot_across_the_maze_corner(o, rng)
        mid_box += cc.count_mid_section_contacts(o, range(0, n, stride // 2), lambda i: box)
        for k in range(steps):
            step(o, sides, uniform(rng, n, 8, 0.3), ('box', t, k))
    covered(need, mid=mid, paid=paid, mid_box=mid_box)


def second_support_points(make, n, rounds, stride, maze, gather):
    """A capsule that rests flat on a face of the maze box (assets/box.xml:12) or on the top of an item cube (assets/food.xml:12) gets a SECOND support
    point (Bullet keeps a manifold there; with one point the capsule rocks): feet hanging alongside the box's vertical faces, legs stretched out
    level over cubes -- states full of such contacts, counted.  maze: [(step_group, contact cap, need)], gather: [(step_group, need)]; the solver's
    row counts are compared as well."""
    rng = np.random.RandomState(12)
    names = ALL + ('solver_rows',)
    for group, cap, need in maze:
        o, sides = start(make, K.HRL_ANT_MAZE, count_rows=True, num_envs=n, seed=4, auto_reset=1, model_step_group=group, model_max_contacts=cap)
        seconds = 0
        for t in range(rounds):
            cc.feet_flat_against_the_maze_box(o, rng)
            seconds += cc.count_second_points(o, range(0, n, stride))
            for k in range(2):
                step(o, sides, uniform(rng, n, 8, 0.3), (group, cap, t, k), names=names)
        covered(need, seconds=seconds)
    for group, need in gather:
        o, sides = start(make, K.HRL_ANT_GATHER, count_rows=True, num_envs=n, seed=4, auto_reset=1, robot_coll_dist=0.0, model_step_group=group)
        seconds = paid = 0
        for t in range(rounds):
            cc.feet_flat_on_cubes(o, rng)
            seconds += cc.count_second_points(o, range(0, n, stride))
            for k in range(2):
                step(o, sides, uniform(rng, n, 8, 0.2), (group, t, k), names=names)
                paid += int((o.info[:, 0] != 0).sum())
        covered(need, seconds=seconds, paid=paid)
