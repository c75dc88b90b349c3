"""GPU parity: HIP kernels (through the C-ABI) vs the fp32 CPU oracle on identical (state, items, action).

Stated tolerance for one env step from identical inputs: BIT-EXACT, for everything the step produces -- packed state
(qpos, qvel, episode return, potential), item positions, aux counters, reward, done, info AND observations.
The algorithm pins every fp32 operation (no FMA contraction; sin / cos / atan2 / asin specified operation by operation,
DESIGN.md 3.7; IEEE divide / sqrt / fmod), so the device and the host must produce the same bits.
(Against the reference's fp64 numpy arithmetic the fp32 observations are good to ~1e-6; that is checked on the CPU by the
golden-vector tests of the fp64 oracle and the fp32-vs-fp64 comparison in tests/test_oracle_golden.py.)
"""
import numpy as np
import pytest
import torch

import orc
import parity_cases as P
from backends import Device
from hrl_pybullet_envs_amd import _capi as K

pytestmark = pytest.mark.gpu
KINDS = [K.HRL_ANT_GATHER, K.HRL_ANT_FLAT, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN]
OBS_ATOL = 0.0  # observations are bit-exact as well


def make(kind, count_rows=False, **over):
    """the side tests/parity_cases.py drives: the device (product defaults == oracle defaults asserted on the way)"""
    return [Device(Device.config(kind, **over), count_rows=count_rows)]


def pair(kind, n, seed=3, **kw):
    """(BatchedEnv, oracle) of the tests that only the device runs"""
    over = dict(num_envs=n, seed=seed, auto_reset=1, **kw)
    return make(kind, **over)[0].env, orc.OracleEnv(orc.default_config(kind, **over), np.float32)


def obs_bad_rows(gobs, oobs):
    return ~((gobs == oobs) | (np.isnan(gobs) & np.isnan(oobs))).all(axis=1)


@pytest.mark.parametrize('kind', KINDS)
def test_reset_matches_oracle(kind):
    P.reset(make, kind, 512, every=5, seed=3, auto_reset=1)


@pytest.mark.parametrize('kind', KINDS)
def test_single_step_parity_along_trajectory(kind):
    """Identical inputs every step (the oracle's state is copied to the device), 80 steps of a random-action rollout
    with auto-reset and a short time limit so that resets, pickups and deaths are all exercised."""
    n, T = 256, 80
    over = dict(num_envs=n, seed=3, auto_reset=1, max_episode_steps=37)
    d, o = make(kind, **over)[0], orc.OracleEnv(orc.default_config(kind, **over), np.float32)
    g = d.env
    g.reset(); o.reset()
    rng = np.random.RandomState(0)
    obs_flips = 0
    for t in range(T):
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        if kind == K.HRL_POINT_GATHER and t == 5:
            a[3] = 0  # NaN force path (point_bot.py:29)
        d.push(o)
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda())
        o.step(a)
        torch.cuda.synchronize()
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), t
        assert np.array_equal(g.items.cpu().numpy(), o.items), t
        assert np.array_equal(g.aux.cpu().numpy(), o.aux), t
        assert np.array_equal(gd.cpu().numpy(), o.done), t
        assert np.array_equal(gr.cpu().numpy(), o.rew), t
        assert np.array_equal(g.info.cpu().numpy(), o.info), t
        gob = go.cpu().numpy()
        fin = np.isfinite(o.obs).all(axis=1)
        obs_flips += int(obs_bad_rows(gob[fin], o.obs[fin]).sum())
    assert obs_flips == 0, obs_flips
    assert o.aux[:, 2].min() >= 3     # every env was auto-reset at least twice


def test_free_running_stays_bit_exact():
    """No state copying: device and oracle run 150 steps independently from the same seed and stay identical."""
    P.free_running(make, K.HRL_ANT_GATHER, 256, 150, stream=1, min_episodes=1, seed=3)


@pytest.mark.parametrize('kind,n,steps', [(K.HRL_ANT_GATHER, 512, 2000), (K.HRL_ANT_MAZE, 256, 1200), (K.HRL_POINT_GATHER, 512, 2000),
                                          (K.HRL_ANT_FLAGRUN, 256, 1200), (K.HRL_ANT_MAZE_MJ, 256, 1200), (K.HRL_ANT_FLAT, 256, 1200)])
def test_long_free_run_stays_bit_exact(kind, n, steps):
    """A whole episode's worth of steps (the 2000-step time limit of the registration for the gather kinds) with no state copying: device and
    oracle each run on their own from the same seed -- pickups, respawns, deaths, time-limit resets on the way -- and end bit-identical
    (over a million env-steps for the gather kinds)."""
    g, o = pair(kind, n, seed=23)
    g.reset(); o.reset()
    gen = torch.Generator(device='cuda').manual_seed(5)
    acts = torch.rand(64, n, o.ad, device='cuda', generator=gen) * 2 - 1
    acts_np = acts.cpu().numpy()
    for t in range(steps):
        g.step(acts[t % 64]); o.step(acts_np[t % 64])
        if t % 500 == 499:
            torch.cuda.synchronize()
            assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), t
    torch.cuda.synchronize()
    assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(g.items.cpu().numpy(), o.items)
    assert np.array_equal(g.aux.cpu().numpy(), o.aux) and obs_bad_rows(g.obs.cpu().numpy(), o.obs).sum() == 0
    assert np.array_equal(g.info.cpu().numpy(), o.info)
    if kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
        assert o.aux[:, 2].min() >= 2   # every env ran into the time limit at least once


def test_pickups_and_respawn_match():
    P.gather_pickups(make, 256, 20, need=dict(picked=401))


def sampled_row_parity(kind, g, rows, st, it, au, a_np, rew, done, seed, **kw):
    """Re-runs the sampled rows of one full-size launch on the oracle from the device's own pre-step state.  The oracle
    keys its RNG by global env id, so every sampled row runs as its own 1-env shard at that id."""
    gs, gi, ga, go = g.state.cpu().numpy(), g.items.cpu().numpy(), g.aux.cpu().numpy(), g.obs.cpu().numpy()
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    off = int(g.cfg.env_id_offset)
    for r in rows:
        o = orc.OracleEnv(orc.default_config(kind, num_envs=1, seed=seed, auto_reset=1, env_id_offset=off + int(r), **kw), np.float32)
        o.state[0] = st[r]; o.items[0] = it[r]; o.aux[0] = au[r]
        o.step(a_np[r:r + 1])
        assert np.array_equal(gs[r], o.state[0], equal_nan=True), r
        assert np.array_equal(gi[r], o.items[0]) and np.array_equal(ga[r], o.aux[0]), r
        assert np.array_equal(go[r], o.obs[0], equal_nan=True), r
        assert float(rew[r]) == float(o.rew[0]) and int(done[r]) == int(o.done[0]), r


FULL_SIZE = [(K.HRL_ANT_GATHER, 4096), (K.HRL_ANT_FLAT, 4096), (K.HRL_ANT_MAZE, 8192), (K.HRL_POINT_GATHER, 4096),
             (K.HRL_ANT_MAZE_MJ, 4096), (K.HRL_ANT_FLAGRUN, 4096)]


@pytest.mark.parametrize('kind,n', FULL_SIZE)
def test_full_size_properties(kind, n):
    """BASELINE.json sizes: size-independent properties + oracle parity on 256 sampled rows (state, items, counters,
    observation, reward, done: bit-exact)."""
    g, o0 = pair(kind, n, seed=21)
    g.reset()
    gen = torch.Generator(device='cuda').manual_seed(0)
    acts = torch.rand(60, n, o0.ad, device='cuda', generator=gen) * 2 - 1
    for t in range(59):
        g.step(acts[t])
    rows = np.random.RandomState(3).choice(n, 256, replace=False)
    st, it, au = g.state.cpu().numpy(), g.items.cpu().numpy(), g.aux.cpu().numpy()
    obs, rew, done, _ = g.step(acts[59])
    torch.cuda.synchronize()
    sampled_row_parity(kind, g, rows, st, it, au, acts[59].cpu().numpy(), rew, done, seed=21)
    s = g.state.cpu().numpy()
    assert np.isfinite(s).all()
    assert np.abs(np.linalg.norm(s[:, 3:7], axis=1) - 1).max() < 1e-5          # unit quaternions
    assert np.all(np.abs(s[:, 21:29]) <= 100.0)                                 # joint-rate clamp
    ob = obs.cpu().numpy()
    assert np.isfinite(ob).all()
    if kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
        nb = 26 if kind == K.HRL_ANT_GATHER else 8
        itf = g.items.cpu().numpy().reshape(n, 16, 2)
        assert np.all(np.abs(itf) <= 7.0)                                       # gather_scene.py:52-62
        assert np.all(ob[:, nb:] >= 0) and np.all(ob[:, nb:] <= 1)             # sensor intensities
        assert np.all(np.abs(s[:, 0:2]) < 7.6)                                  # walls hold the robot in the arena
    if kind == K.HRL_ANT_GATHER:
        assert np.all(np.abs(ob[:, :26]) <= 5)                                  # upstream clip
    if kind == K.HRL_ANT_MAZE:
        assert np.all(ob[:, 28:] >= 0) and np.all(ob[:, 28:] <= 1)
        assert np.allclose(np.linalg.norm(ob[:, 26:28], axis=1), 1, atol=1e-5)  # normed target vector
    if kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        assert np.all(np.abs(s[:, 0]) < 5.1) and np.all(np.abs(s[:, 1]) < 9.1)
    if kind == K.HRL_ANT_MAZE_MJ:
        assert np.all(ob[:, 29:39] >= 0) and np.all(ob[:, 29:39] <= 1) and np.all(ob[:, 39:59] == 0)  # walls | pit, moveable zeros
    if kind == K.HRL_ANT_FLAGRUN:
        assert np.all(np.abs(ob[:, :28]) <= 5) and np.all(np.abs(s[:, 0:2]) < 6.1)


def test_mixed_shard_full_size_two_streams():
    """BASELINE.json configs[4] per GPU at full size: 2048 AntGather + 2048 PointGather (global ids 0..4095), the two
    hrl_step launches of a step issued on two HIP streams as bench.py --kind mixed does; 256 sampled rows of each half
    re-run on the oracle bit for bit, and the overlapped run equals a serialized run of the same shard."""
    n = 2048
    ant, _ = pair(K.HRL_ANT_GATHER, n, seed=31)
    pt, _ = pair(K.HRL_POINT_GATHER, n, seed=31, env_id_offset=n)
    ant_s, _ = pair(K.HRL_ANT_GATHER, n, seed=31)
    pt_s, _ = pair(K.HRL_POINT_GATHER, n, seed=31, env_id_offset=n)
    for e in (ant, pt, ant_s, pt_s):
        e.reset()
    torch.cuda.synchronize()
    gen = torch.Generator(device='cuda').manual_seed(7)
    a8 = torch.rand(41, n, 8, device='cuda', generator=gen) * 2 - 1
    a2 = torch.rand(41, n, 2, device='cuda', generator=gen) * 2 - 1
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for t in range(40):
        with torch.cuda.stream(s1):
            ant.step(a8[t])
        with torch.cuda.stream(s2):
            pt.step(a2[t])
        ant_s.step(a8[t]); pt_s.step(a2[t])
    torch.cuda.synchronize()
    assert torch.equal(ant.state, ant_s.state) and torch.equal(pt.state, pt_s.state) and torch.equal(pt.items, pt_s.items)
    rows = np.random.RandomState(4).choice(n, 256, replace=False)
    pre = [(e.state.cpu().numpy(), e.items.cpu().numpy(), e.aux.cpu().numpy()) for e in (ant, pt)]
    with torch.cuda.stream(s1):
        _, ra, da, _ = ant.step(a8[40])
    with torch.cuda.stream(s2):
        _, rp, dp, _ = pt.step(a2[40])
    torch.cuda.synchronize()
    sampled_row_parity(K.HRL_ANT_GATHER, ant, rows, *pre[0], a8[40].cpu().numpy(), ra, da, seed=31)
    sampled_row_parity(K.HRL_POINT_GATHER, pt, rows, *pre[1], a2[40].cpu().numpy(), rp, dp, seed=31)
    returns = torch.cat([ant.info[:, 2], pt.info[:, 2]])  # what the all-gather of a mixed shard carries
    assert returns.shape == (2 * n,) and bool(torch.isfinite(returns).all())


def test_rank7_shard_of_config5_global_ids():
    """BASELINE.json configs[4] = 32768 global ids over 8 ranks; rank 7 owns ids 28672..32767: its first half AntGather, its
    second half PointGather (bench.py --kind mixed).  One GPU runs that shard with `env_id_offset` as rank 7 would; 256 sampled
    rows of each half are re-run on the oracle at their GLOBAL ids (resets and respawns draw from streams keyed by them)."""
    n, off = 2048, 7 * 4096
    ant, _ = pair(K.HRL_ANT_GATHER, n, seed=0, env_id_offset=off, max_episode_steps=25)
    pt, _ = pair(K.HRL_POINT_GATHER, n, seed=0, env_id_offset=off + n, max_episode_steps=25)
    ant.reset(); pt.reset()
    # reset parity at the global ids (the oracle as one shard at the same offset)
    _, oa = pair(K.HRL_ANT_GATHER, 64, seed=0, env_id_offset=off + 1000, max_episode_steps=25)
    oa.reset()
    assert np.array_equal(ant.state[1000:1064].cpu().numpy(), oa.state) and np.array_equal(ant.items[1000:1064].cpu().numpy(), oa.items)
    gen = torch.Generator(device='cuda').manual_seed(9)
    a8 = torch.rand(31, n, 8, device='cuda', generator=gen) * 2 - 1
    a2 = torch.rand(31, n, 2, device='cuda', generator=gen) * 2 - 1
    for t in range(30):  # past the 25-step time limit: every env has been auto-reset from its global-id stream
        ant.step(a8[t]); pt.step(a2[t])
    rows = np.random.RandomState(6).choice(n, 256, replace=False)
    pre = [(e.state.cpu().numpy(), e.items.cpu().numpy(), e.aux.cpu().numpy()) for e in (ant, pt)]
    assert pre[0][2][:, 2].min() >= 2
    _, ra, da, _ = ant.step(a8[30])
    _, rp, dp, _ = pt.step(a2[30])
    torch.cuda.synchronize()
    sampled_row_parity(K.HRL_ANT_GATHER, ant, rows, *pre[0], a8[30].cpu().numpy(), ra, da, seed=0, max_episode_steps=25)
    sampled_row_parity(K.HRL_POINT_GATHER, pt, rows, *pre[1], a2[30].cpu().numpy(), rp, dp, seed=0, max_episode_steps=25)
    # the same ids inside a 32768-env single-GPU launch give the same trajectories (shard invariance at the top of the range)
    small, _ = pair(K.HRL_ANT_GATHER, 128, seed=0, env_id_offset=off + 500, max_episode_steps=25)
    small.reset()
    for t in range(31):
        small.step(a8[t][500:628].contiguous())
    assert torch.equal(small.state, ant.state[500:628]) and torch.equal(small.items, ant.items[500:628])


def test_32768_envs_on_one_gpu():
    """All of config 5's ids in one launch (8192 workgroups of four env-waves): size-independent properties + 256 sampled rows
    against the oracle at their own global ids, including rows of the last rank's range."""
    n = 32768
    g, o0 = pair(K.HRL_ANT_GATHER, n, seed=4)
    g.reset()
    gen = torch.Generator(device='cuda').manual_seed(2)
    acts = torch.rand(8, n, 8, device='cuda', generator=gen) * 2 - 1
    for t in range(40):
        g.step(acts[t % 8])
    rows = np.concatenate([np.random.RandomState(8).choice(n, 192, replace=False), np.arange(n - 64, n)])
    st, it, au = g.state.cpu().numpy(), g.items.cpu().numpy(), g.aux.cpu().numpy()
    obs, rew, done, _ = g.step(acts[3])
    torch.cuda.synchronize()
    sampled_row_parity(K.HRL_ANT_GATHER, g, rows, st, it, au, acts[3].cpu().numpy(), rew, done, seed=4)
    s = g.state.cpu().numpy()
    assert np.isfinite(s).all() and np.abs(np.linalg.norm(s[:, 3:7], axis=1) - 1).max() < 1e-5
    assert np.all(np.abs(s[:, 21:29]) <= 100.0) and np.all(np.abs(s[:, 0:2]) < 7.6)
    ob = obs.cpu().numpy()
    assert np.isfinite(ob).all() and np.all(ob[:, 26:] >= 0) and np.all(ob[:, 26:] <= 1) and np.all(np.abs(ob[:, :26]) <= 5)
    assert np.all(np.abs(g.items.cpu().numpy()) <= 7.0)


def test_batch_composition_invariance():
    """Env i's trajectory does not depend on which other envs share the launch (global-id RNG, no cross-env state)."""
    big, _ = pair(K.HRL_ANT_GATHER, 4096, seed=5)
    small, _ = pair(K.HRL_ANT_GATHER, 128, seed=5, env_id_offset=1000)
    big.reset(); small.reset()
    gen = torch.Generator(device='cuda').manual_seed(1)
    for t in range(40):
        a = torch.rand(4096, 8, device='cuda', generator=gen) * 2 - 1
        big.step(a); small.step(a[1000:1128].contiguous())
    assert torch.equal(big.state[1000:1128], small.state) and torch.equal(big.items[1000:1128], small.items)


@pytest.mark.parametrize('n', [1, 2, 3, 5, 7, 4093])
def test_env_counts_that_do_not_fill_the_last_group(n):
    """Four env-waves share a workgroup: the waves of the last group without an env of their own only take part in its barriers.
    Every count from one env up must match the oracle, and nothing outside the n rows of the caller's buffers may be written."""
    g, o = pair(K.HRL_ANT_GATHER, n, seed=11)
    # the caller's buffers become views into larger allocations: a write past row n - 1 lands in the guard rows behind them
    big = {}
    for k in ('state', 'items', 'aux', 'obs', 'reward', 'done', 'info', 'final_obs', 'truncated'):
        t = getattr(g, k)
        big[k] = torch.full((n + 8,) + tuple(t.shape[1:]), 7, dtype=t.dtype, device=t.device)
        big[k][:n] = t
        if k in g._out:
            g._out[k] = big[k][:n]   # the step's outputs are read through properties over this dict
        else:
            setattr(g, k, big[k][:n])
    g._bind()   # the buffer record of the library from the tensors as they are now
    g.reset(); o.reset()
    rng = np.random.RandomState(3)
    for t in range(25):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0, t
    assert all(bool((v[n:] == 7).all()) for v in big.values())


@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_ANT_MAZE])
def test_one_wave_per_env_launch_matches_too(kind):
    """hrl_model.step_group = 1 (kept for ABI v7 configs; it launches the same four-wave group as 0) is accepted and bit-exact against
    the oracle like the default."""
    n = 96
    g, o = pair(kind, n, seed=13, max_episode_steps=23, model_step_group=1)
    g.reset(); o.reset()
    rng = np.random.RandomState(4)
    for t in range(40):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state), t
        assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0, t


def test_mixed_ant_point_shard():
    """BASELINE config 5 shape on one GPU: first half AntGather, second half PointGather, two launches per step."""
    n = 512
    ant, oa = pair(K.HRL_ANT_GATHER, n, seed=8)
    pt, op = pair(K.HRL_POINT_GATHER, n, seed=8, env_id_offset=n)
    ant.reset(); pt.reset(); oa.reset(); op.reset()
    rng = np.random.RandomState(2)
    for t in range(30):
        a8 = rng.uniform(-1, 1, (n, 8)).astype(np.float32); a2 = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        ant.step(torch.from_numpy(a8).cuda()); pt.step(torch.from_numpy(a2).cuda())
        oa.step(a8); op.step(a2)
    assert np.array_equal(ant.state.cpu().numpy(), oa.state) and np.array_equal(pt.state.cpu().numpy(), op.state)
    returns = torch.cat([ant.info[:, 2], pt.info[:, 2]])
    assert returns.shape == (2 * n,) and bool(torch.isfinite(returns).all())


def test_get_set_state_roundtrip():
    g, o = pair(K.HRL_ANT_GATHER, 64)
    g.reset()
    qpos, qvel = g.get_state()
    assert torch.equal(qpos, g.state[:, :15]) and torch.equal(qvel, g.state[:, 15:29])
    qpos2 = qpos + 0.01
    g.set_state(qpos2, qvel)
    assert torch.equal(g.state[:, :15], qpos2)


def test_determinism_on_device():
    outs = []
    for rep in range(2):
        g, _ = pair(K.HRL_ANT_GATHER, 1024, seed=9)
        g.reset()
        gen = torch.Generator(device='cuda').manual_seed(0)
        for t in range(50):
            a = torch.rand(1024, 8, device='cuda', generator=gen) * 2 - 1
            g.step(a)
        torch.cuda.synchronize()
        outs.append((g.state.clone(), g.items.clone(), g.obs.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


@pytest.mark.parametrize('kind,n,kw', [(kind, n, kw) for kind, _, n, kw in P.CONFIG_MATRIX])
def test_non_default_configs_match_oracle(kind, n, kw):
    """Non-default constructor branches and odd batch sizes, free-running for 60 steps."""
    P.config_matrix(make, kind, n, kw)


@pytest.mark.parametrize('use_sensor', [1, 0])
@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER])
def test_contact_pickup_on_item_cubes(kind, use_sensor):
    """robot_coll_dist <= 0 (ant_gather_env.py:113-116): robots teleported onto / next to cubes touch them, are paid +-1 per
    contact point and the cube moves; device == oracle bit for bit (identical inputs every step).  The observation was taken before
    the cube moved (:95-96 precede :113): with use_sensor=0 it holds the positions the items had when the step began."""
    P.item_cubes(make, kind, 256, 25, need=dict(paid=151, moved=0 if use_sensor else 41), turned=True, robot_coll_dist=0.0, use_sensor=use_sensor)
    P.cubes_matter_to_the_physics(kind, 256)


def test_capsule_mid_sections_against_cubes_and_the_maze_box_on_device():
    """assets/ant.xml:16-55 capsules against assets/food.xml:12 cubes and the assets/box.xml:12 maze box: ants let down onto cubes with the
    MIDDLE of their feet (contact pickup, ant_gather_env.py:113-116: the touch is paid) and feet laid across the vertical edges of the maze
    box -- contacts no end-point sphere sees.  Device == oracle bit for bit, identical inputs every round."""
    P.capsule_mid_sections(make, 256, rounds=4, steps=3, stride=16, need=dict(mid=30, paid=400, mid_box=30))


def test_second_support_points_on_device():
    """A capsule that rests flat on a face of the maze box or on the top of an item cube gets a SECOND support point (Bullet keeps a manifold there):
    feet hanging alongside the box's vertical faces, legs stretched out level over cubes (tests/capsule_cases.py) -- states full of such contacts,
    counted; device == oracle bit for bit, with hrl_model.step_group 0 and 1 (both the four-wave group), a tight contact cap included."""
    P.second_support_points(make, 256, rounds=3, stride=4, maze=[(0, 12, dict(seconds=100)), (1, 12, dict(seconds=100)), (0, 5, dict(seconds=20))],
                            gather=[(group, dict(seconds=150, paid=300)) for group in (0, 1)])


def test_self_collision_rows_on_device():
    """Hips forced beyond their range so that capsules of different legs meet: the two-body rows (second impulse response,
    10-term row products) on the device equal the oracle's bit for bit."""
    P.self_collision(make, 256, 20, stride=16, need=dict(seen=10), auto_reset=1)


def test_flagrun_manual_goals_through_the_c_abi():
    """hrl_set_goals / hrl_next_target (manual_goal_creation, ant_flagrun_env.py:45,112-120): the list is consumed from its back
    (`goals.pop()`), the episode is over when it runs out; next_target() alone pops one goal, ok = 0 on an empty list."""
    from hrl_pybullet_envs_amd import _lib
    P.flagrun_manual_goals(make, 64, 4, skip=7, auto_reset=1)
    bad, _ = pair(K.HRL_ANT_FLAGRUN, 4)
    with pytest.raises(_lib.HrlError, match='manual'):
        bad.set_goals(torch.zeros(4, 2, 2).cuda())
    # max_targets < 1: next_target() never reads the list (:113-114)
    P.flagrun_manual_close_targets(make, 32, 12, dict(expected_exception=_lib.HrlError, match='hrl_next_target'), seed=4, auto_reset=1, flag_timeout=5)


def test_flagrun_open_field_and_no_switch_on_device():
    """The two flagrun branches the device had not run (ant_flagrun_env.py:59-64 `enclosed=False`, :183-194
    `switch_flag_on_collision=False`), with the robots put where the branches matter: astride the absent wall, and on the goal."""
    P.flagrun_open_field_and_no_switch(make, 64, auto_reset=1)


@pytest.mark.parametrize('auto_reset', [1, 0])
@pytest.mark.parametrize('kind', KINDS)
def test_envs_that_blow_up_match_too(kind, auto_reset):
    """Non-finite and absurd states -- velocities of 1e20 and inf, NaN coordinates of the robot or of an item, a torso 1e19 m away, robots inside
    a wall, joint angles far out of range -- go through the same arithmetic on both sides: what comes out (NaN, inf, done, the dying cost, the
    auto-reset that follows) is identical, bit for bit with NaNs compared as equal.  (A NaN item distance used to read 0 on the device and NaN
    in the oracle; a division replaced by a cheaper sequence that treats infinities differently shows up here too, not in a healthy run.)"""
    P.blow_up(make, kind, 128, auto_reset)


@pytest.mark.parametrize('kind', KINDS)
def test_fuzzed_absurd_values_stay_bit_exact(kind):
    """tests/tools/fuzz_parity.py on the device: NaN, +-inf, 1e20, 3e38, denormals and signed zeros in positions, velocities, item coordinates and
    actions of running envs; every output equals the oracle's at every step."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('fuzz_parity', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools', 'fuzz_parity.py'))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    for seed in (0, 1, 2):
        for ar in (0, 1):
            assert fz.run(fz.GpuSide, kind, seed, ar) is None


@pytest.mark.parametrize('kind', KINDS)
def test_terminal_observation_and_truncation_flag(kind):
    """ABI v6: hrl_buffers.final_obs = the observation of the step that ended an episode (ant_gather_env.py:96,118-119,
    ant_maze_bullet_env.py:82,97) -- which the in-kernel reset replaces in `obs` by the next episode's first --, hrl_buffers.truncated = ended by
    the step limit alone.  Device == oracle bit for bit (the oracle's semantics are pinned against a never-resetting twin in
    tests/test_emu_parity.py); rows of live envs keep what they held; a launch with NULL pointers writes neither."""
    import ctypes as C
    n = 192
    o, (d,), rng = P.terminal_observation(make, kind, n, 24, need=dict(n_trunc=100, n_term=40))
    g = d.env
    # NULL pointers: nothing is written (and nothing crashes)
    keep_f, keep_t = g.final_obs.clone(), g.truncated.clone()
    g._bufs.final_obs = None; g._bufs.truncated = None
    for t in range(12):
        g.step(torch.from_numpy(rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)).cuda())
    torch.cuda.synchronize()
    assert torch.equal(g.final_obs.view(torch.int32), keep_f.view(torch.int32)) and torch.equal(g.truncated, keep_t)   # bit patterns: rows hold NaNs
    assert int(g.done.sum()) >= 0 and C.sizeof(K.hrl_buffers) == 8 + 12 * 8


@pytest.mark.parametrize('kind,kw', [
    (K.HRL_ANT_GATHER, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_POINT_GATHER, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_ANT_GATHER, dict(n_food=40, n_poison=24, n_bins=64, robot_coll_dist=0.0)),
    (K.HRL_POINT_GATHER, dict(n_food=40, n_poison=24, n_bins=30, robot_coll_dist=-1.0)),
])
def test_more_than_16_items(kind, kw):
    """n_food + n_poison > 16 on the device (the reference's constructor takes any counts, ant_gather_env.py:16-17): robots parked at every slot in
    turn, identical inputs every step: pickups, cube contacts (the 16-item slices of the packed contact phase, item codes beyond the capsule
    pairs), respawns with the 6-bit item field and the sensor over all slots equal the oracle bit for bit."""
    o, (d,) = P.more_than_16_items(make, kind, 256, 30, need=dict(moved_hi=80, paid=200), **kw)
    assert d.env.items.shape[1] == orc.items_stride(o.cfg)


def test_manual_goal_lists_longer_than_15_through_the_c_abi():
    """flag_goal_capacity = 40: hrl_set_goals takes the 40-goal list (`env.goals = [...]` takes any, ant_flagrun_env.py:45), the pending list
    lives in a 96-float items record and is consumed back to front; one goal beyond the capacity is refused with a reason."""
    from hrl_pybullet_envs_amd import _lib
    o, (d,) = P.manual_goal_lists_longer_than_15(make, 48, dict(expected_exception=_lib.HrlError, match='flag_goal_capacity'), auto_reset=1)
    assert d.env.items.shape[1] == 96


def test_random_legal_configs_on_device():
    """tests/tools/fuzz_configs.py on the device: 600 random legal configs (constructor arguments, engine parameters, env counts that leave parked
    waves, global ids beyond 2^32) x 30 steps with teleports, masked resets, manual goals in between; every buffer equals the oracle's bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tools'))
    import fuzz_configs as F
    for seed in range(7000, 7100):
        for kind in F.KINDS:
            r, _ = F.run(F.GpuSide, kind, seed * 16 + kind, 30)
            assert r is None, r


def test_device_reproduces_the_committed_specification_fingerprint():
    """tests/golden/spec_fingerprint.json (sha256 of the buffers of 16 envs of every kind after the reset and 1, 10, 80 steps; the oracle and the host
    executor reproduce it in tests/test_spec_fingerprint.py): the device's bytes, read back through the C-ABI buffers, hash to the same digests."""
    import json
    import spec_fingerprint as S

    want = json.load(open(S.PATH))
    got = S.fingerprint(Device)
    assert got == want, [k for k in want if got.get(k) != want[k]]


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


def test_crossing_capsule_axes():
    P.crossing_capsule_axes(make, ANT_N, need=dict(self_contacts=ANT_N, crossing=ANT_N))


def test_exhausted_goal_draws():
    P.exhausted_goal_draws(make, ANT_N)


def test_nan_robot_with_the_target_on_a_wall():
    P.nan_robot_with_the_target_on_a_wall(make, ANT_N, need=dict(q1=4, apart=3))
