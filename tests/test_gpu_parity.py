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
from hrl_pybullet_envs_amd import _capi as K

pytestmark = pytest.mark.gpu
KINDS = [K.HRL_ANT_GATHER, K.HRL_ANT_FLAT, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER, K.HRL_ANT_MAZE_MJ, K.HRL_ANT_FLAGRUN]
OBS_ATOL = 0.0  # observations are bit-exact as well


def make(kind, n, seed=3, **kw):
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    cfg = _lib.default_config(kind, num_envs=n, seed=seed, auto_reset=1, **kw)
    ocfg = orc.default_config(kind, num_envs=n, seed=seed, auto_reset=1, **kw)
    assert bytes(cfg) == bytes(ocfg)  # product defaults == oracle defaults
    return BatchedEnv(cfg, 'cuda:0'), orc.OracleEnv(ocfg, np.float32)


def push(g, o):
    g.state.copy_(torch.from_numpy(o.state)); g.items.copy_(torch.from_numpy(o.items)); g.aux.copy_(torch.from_numpy(o.aux))


def obs_bad_rows(gobs, oobs):
    return ~((gobs == oobs) | (np.isnan(gobs) & np.isnan(oobs))).all(axis=1)


@pytest.mark.parametrize('kind', KINDS)
def test_reset_matches_oracle(kind):
    g, o = make(kind, 512)
    g.reset(); o.reset()
    torch.cuda.synchronize()
    assert np.array_equal(g.aux.cpu().numpy(), o.aux)
    assert np.array_equal(g.state.cpu().numpy(), o.state)
    assert np.array_equal(g.items.cpu().numpy(), o.items)
    assert obs_bad_rows(g.obs.cpu().numpy(), o.obs).sum() == 0
    mask = torch.zeros(512, dtype=torch.uint8); mask[::5] = 1
    g.reset(mask.cuda()); o.reset(mask.numpy())
    assert np.array_equal(g.state.cpu().numpy(), o.state) and np.array_equal(g.aux.cpu().numpy(), o.aux)


@pytest.mark.parametrize('kind', KINDS)
def test_single_step_parity_along_trajectory(kind):
    """Identical inputs every step (the oracle's state is copied to the device), 80 steps of a random-action rollout
    with auto-reset and a short time limit so that resets, pickups and deaths are all exercised."""
    n, T = 256, 80
    g, o = make(kind, n, max_episode_steps=37)
    g.reset(); o.reset()
    rng = np.random.RandomState(0)
    obs_flips = 0
    for t in range(T):
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        if kind == K.HRL_POINT_GATHER and t == 5:
            a[3] = 0  # NaN force path (point_bot.py:29)
        push(g, o)
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
    n = 256
    g, o = make(K.HRL_ANT_GATHER, n)
    g.reset(); o.reset()
    rng = np.random.RandomState(1)
    for t in range(150):
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        g.step(torch.from_numpy(a).cuda()); o.step(a)
    torch.cuda.synchronize()
    assert np.array_equal(g.state.cpu().numpy(), o.state) and np.array_equal(g.items.cpu().numpy(), o.items)


@pytest.mark.parametrize('kind,n,steps', [(K.HRL_ANT_GATHER, 512, 2000), (K.HRL_ANT_MAZE, 256, 1200), (K.HRL_POINT_GATHER, 512, 2000),
                                          (K.HRL_ANT_FLAGRUN, 256, 1200), (K.HRL_ANT_MAZE_MJ, 256, 1200), (K.HRL_ANT_FLAT, 256, 1200)])
def test_long_free_run_stays_bit_exact(kind, n, steps):
    """A whole episode's worth of steps (the 2000-step time limit of the registration for the gather kinds) with no state copying: device and
    oracle each run on their own from the same seed -- pickups, respawns, deaths, time-limit resets on the way -- and end bit-identical
    (over a million env-steps for the gather kinds)."""
    g, o = make(kind, n, seed=23)
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
    n = 256
    g, o = make(K.HRL_ANT_GATHER, n, seed=11)
    g.reset(); o.reset()
    rng = np.random.RandomState(5)
    picked = 0
    for t in range(20):
        k = rng.randint(0, 16, n)
        xy = o.items.reshape(n, 16, 2)[np.arange(n), k] + rng.uniform(-0.6, 0.6, (n, 2)).astype(np.float32)
        o.state[:, 0:2] = xy
        push(g, o)
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        _, gr, _, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        picked += int((o.info[:, 0] != 0).sum())
        assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(gr.cpu().numpy(), o.rew)
        assert np.array_equal(gi['food_rew'].cpu().numpy(), o.info[:, 0])
    assert picked > 400


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
    g, o0 = make(kind, n, seed=21)
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
    ant, _ = make(K.HRL_ANT_GATHER, n, seed=31)
    pt, _ = make(K.HRL_POINT_GATHER, n, seed=31, env_id_offset=n)
    ant_s, _ = make(K.HRL_ANT_GATHER, n, seed=31)
    pt_s, _ = make(K.HRL_POINT_GATHER, n, seed=31, env_id_offset=n)
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
    ant, _ = make(K.HRL_ANT_GATHER, n, seed=0, env_id_offset=off, max_episode_steps=25)
    pt, _ = make(K.HRL_POINT_GATHER, n, seed=0, env_id_offset=off + n, max_episode_steps=25)
    ant.reset(); pt.reset()
    # reset parity at the global ids (the oracle as one shard at the same offset)
    _, oa = make(K.HRL_ANT_GATHER, 64, seed=0, env_id_offset=off + 1000, max_episode_steps=25)
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
    small, _ = make(K.HRL_ANT_GATHER, 128, seed=0, env_id_offset=off + 500, max_episode_steps=25)
    small.reset()
    for t in range(31):
        small.step(a8[t][500:628].contiguous())
    assert torch.equal(small.state, ant.state[500:628]) and torch.equal(small.items, ant.items[500:628])


def test_32768_envs_on_one_gpu():
    """All of config 5's ids in one launch (8192 workgroups of four env-waves): size-independent properties + 256 sampled rows
    against the oracle at their own global ids, including rows of the last rank's range."""
    n = 32768
    g, o0 = make(K.HRL_ANT_GATHER, n, seed=4)
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
    big, _ = make(K.HRL_ANT_GATHER, 4096, seed=5)
    small, _ = make(K.HRL_ANT_GATHER, 128, seed=5, env_id_offset=1000)
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
    g, o = make(K.HRL_ANT_GATHER, n, seed=11)
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
    g, o = make(kind, n, seed=13, max_episode_steps=23, model_step_group=1)
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
    ant, oa = make(K.HRL_ANT_GATHER, n, seed=8)
    pt, op = make(K.HRL_POINT_GATHER, n, seed=8, env_id_offset=n)
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
    g, o = make(K.HRL_ANT_GATHER, 64)
    g.reset()
    qpos, qvel = g.get_state()
    assert torch.equal(qpos, g.state[:, :15]) and torch.equal(qvel, g.state[:, 15:29])
    qpos2 = qpos + 0.01
    g.set_state(qpos2, qvel)
    assert torch.equal(g.state[:, :15], qpos2)


def test_determinism_on_device():
    outs = []
    for rep in range(2):
        g, _ = make(K.HRL_ANT_GATHER, 1024, seed=9)
        g.reset()
        gen = torch.Generator(device='cuda').manual_seed(0)
        for t in range(50):
            a = torch.rand(1024, 8, device='cuda', generator=gen) * 2 - 1
            g.step(a)
        torch.cuda.synchronize()
        outs.append((g.state.clone(), g.items.clone(), g.obs.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


CONFIG_MATRIX = [
    (K.HRL_ANT_GATHER, 37, dict(n_bins=7, n_food=5, n_poison=3, sensor_range=9.0, sensor_span=2.0, world_size=(9.0, 11.0), centroid_static_sum=(-4.5, 0.0))),
    (K.HRL_ANT_GATHER, 64, dict(respawn=0, robot_coll_dist=4.0, dying_cost=-3.0)),
    (K.HRL_ANT_GATHER, 33, dict(use_sensor=0)),
    (K.HRL_POINT_GATHER, 50, dict(n_bins=9, robot_object_spacing=3.0)),
    (K.HRL_ANT_MAZE, 65, dict(sense_target=1, n_bins=8)),
    (K.HRL_ANT_MAZE, 31, dict(target_encoding=1, sense_walls=0, tol=3.0, targ_dist_rew=1, max_steps=20, done_at_target=0)),
    (K.HRL_ANT_MAZE_MJ, 40, dict(inner_rew_weight=0.5, n_bins=6)),
    (K.HRL_ANT_FLAGRUN, 48, dict(use_sensor=1, n_bins=8, flag_timeout=9, flag_max_targets=3)),
    (K.HRL_ANT_FLAGRUN, 21, dict(flag_max_targets=0, flag_max_target_dist=2.5, flag_timeout=6, flag_size=3.0, world_size=(5.0, 5.0), centroid_static_sum=(-2.5, 0.0))),
    (K.HRL_ANT_FLAT, 1, dict()),
    (K.HRL_ANT_GATHER, 3, dict(model_solver_iters=2, model_frame_skip=2, model_limit_margin=0.1)),
    (K.HRL_ANT_GATHER, 40, dict(model_self_collision=0, model_item_collision=0)),
    # hrl_model of ABI v7, all on at once: Bullet's per-body damping (pybullet's 0.04 and a strong one), restitution, a tight contact cap, joint damping + armature
    (K.HRL_ANT_GATHER, 66, dict(model_linear_damping=0.04, model_angular_damping=0.04, model_restitution=0.3, model_max_contacts=6, model_joint_damping=1.0, model_joint_armature=1.0)),
    (K.HRL_ANT_MAZE, 35, dict(model_linear_damping=3.0, model_angular_damping=8.0, model_restitution_threshold=0.0, model_restitution=0.8)),
    (K.HRL_POINT_GATHER, 46, dict(model_linear_damping=0.04, model_angular_damping=2.0, model_restitution=0.5, model_max_contacts=3)),
    (K.HRL_ANT_GATHER, 70, dict(robot_coll_dist=0.0)),
    (K.HRL_POINT_GATHER, 45, dict(robot_coll_dist=-1.0, respawn=0)),
    (K.HRL_ANT_MAZE, 33, dict(inner_rew_weight=1.0)),
    (K.HRL_ANT_MAZE_MJ, 17, dict(inner_rew_weight=1.0)),
    (K.HRL_ANT_FLAGRUN, 35, dict(flag_enclosed=0, centroid_n_static=1, centroid_static_sum=(0.0, 0.0), flag_timeout=8, flag_max_targets=5)),  # ant_flagrun_env.py:59-64: open field
    (K.HRL_ANT_FLAGRUN, 29, dict(flag_switch_on_collision=0, flag_timeout=7, flag_max_targets=4)),                                           # :183-194
    (K.HRL_ANT_FLAGRUN, 19, dict(flag_manual_goals=1, flag_max_targets=0, flag_max_target_dist=3.0, flag_timeout=5)),                        # manual + close targets (:113-114)
    # constructor arguments beyond the caps of ABI <= 5 (ant_gather_env.py:16-29, ant_maze_bullet_env.py:23-25, ant_maze_mj_env.py:50):
    # more than 16 items, observations wider than the wave, more than 8 targets
    (K.HRL_ANT_GATHER, 70, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_POINT_GATHER, 41, dict(n_food=20, n_poison=12, n_bins=24)),
    (K.HRL_ANT_GATHER, 37, dict(n_food=40, n_poison=24, n_bins=64, robot_coll_dist=0.0, world_size=(8.0, 8.0), centroid_static_sum=(-4.0, 0.0))),
    (K.HRL_POINT_GATHER, 33, dict(n_food=33, n_poison=31, n_bins=40, robot_coll_dist=-1.0, world_size=(8.0, 8.0))),
    (K.HRL_ANT_GATHER, 21, dict(n_food=20, n_poison=12, n_bins=24, use_sensor=0)),
    (K.HRL_ANT_MAZE_MJ, 35, dict(n_bins=16)),
    (K.HRL_ANT_MAZE_MJ, 18, dict(n_bins=64)),
    (K.HRL_ANT_MAZE, 45, dict(sense_target=1, n_bins=33, targets=[(-2.0 + 0.5 * i, -4.0 + 0.1 * i) for i in range(12)], tol=0.7)),
    (K.HRL_ANT_FLAGRUN, 22, dict(use_sensor=1, n_bins=40, flag_timeout=9)),
]


@pytest.mark.parametrize('kind,n,kw', CONFIG_MATRIX)
def test_non_default_configs_match_oracle(kind, n, kw):
    """Non-default constructor branches and odd batch sizes, free-running for 60 steps."""
    g, o = make(kind, n, seed=17, max_episode_steps=25, **kw)
    g.reset(); o.reset()
    assert np.array_equal(g.state.cpu().numpy(), o.state) and obs_bad_rows(g.obs.cpu().numpy(), o.obs).sum() == 0
    rng = np.random.RandomState(4)
    flips = 0
    for t in range(60):
        if kw.get('flag_manual_goals') and t == 20:
            # a manual_goal_creation env that was never given a goal pays NaN, as the reference does (`_sq_dist_goal` is still the constructor's 0:
            # path_rew = 0 / 0, ant_flagrun_env.py:48,174-176) until its first goal; next_target() is the documented way to give it one
            import ctypes as C
            g.next_target()
            orc.lib().orc_next_target_batch_f32(C.byref(o.cfg), orc.ptr(o.state), orc.ptr(o.items), orc.ptr(o.aux), None, orc.ptr(o.obs), None)
            assert np.array_equal(g.items.cpu().numpy(), o.items)
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), t
        assert np.array_equal(gr.cpu().numpy(), o.rew, equal_nan=True) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert np.array_equal(g.truncated.cpu().numpy(), o.truncated) and obs_bad_rows(g.final_obs.cpu().numpy(), o.final_obs).sum() == 0, t
        flips += int(obs_bad_rows(go.cpu().numpy(), o.obs).sum())
    assert flips == 0
    assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux)


@pytest.mark.parametrize('use_sensor', [1, 0])
@pytest.mark.parametrize('kind', [K.HRL_ANT_GATHER, K.HRL_POINT_GATHER])
def test_contact_pickup_on_item_cubes(kind, use_sensor):
    """robot_coll_dist <= 0 (ant_gather_env.py:113-116): robots teleported onto / next to cubes touch them, are paid +-1 per
    contact point and the cube moves; device == oracle bit for bit (identical inputs every step).  The observation was taken before
    the cube moved (:95-96 precede :113): with use_sensor=0 it holds the positions the items had when the step began."""
    n = 256
    g, o = make(kind, n, seed=13, robot_coll_dist=0.0, use_sensor=use_sensor)
    g.reset(); o.reset()
    rng = np.random.RandomState(2)
    paid = moved = 0
    for t in range(25):
        k = rng.randint(0, 16, n)
        off = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32) * (1.4 if kind == K.HRL_ANT_GATHER else 0.45)
        o.state[:, 0:2] = o.items.reshape(n, 16, 2)[np.arange(n), k] + off
        if kind == K.HRL_POINT_GATHER and t % 2 == 0:
            # parked at rest with a face against the cube (gap -4 .. 12 mm) anywhere along that face: contacts that last until the
            # step's final collision pass, most of them made by the CUBE's corners against the player's box
            side = rng.randint(0, 4, n); d = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)[side]
            lat = rng.uniform(-0.42, 0.42, n).astype(np.float32); gap = rng.uniform(-0.004, 0.012, n).astype(np.float32)
            o.state[:, 0:2] = o.items.reshape(n, 16, 2)[np.arange(n), k] - d * (np.float32(0.475) + gap)[:, None] + d[:, ::-1] * lat[:, None]
            o.state[:, 2] = 0.35; o.state[:, 3:7] = [0, 0, 0, 1]; o.state[:, 7:13] = 0
        elif kind == K.HRL_POINT_GATHER:  # any yaw, slightly tipped, the cube under the body, under a face or beside an edge
            yaw = rng.uniform(-np.pi, np.pi, n); tip = rng.uniform(-0.05, 0.05, (n, 2))
            quat = np.stack([tip[:, 0], tip[:, 1], np.sin(yaw / 2), np.cos(yaw / 2)], 1); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
            o.state[:, 3:7] = quat.astype(np.float32); o.state[:, 2] = 0.35; o.state[:, 7:13] = 0
        push(g, o)
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        it0 = o.items.copy()
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(g.items.cpu().numpy(), o.items), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(g.info.cpu().numpy(), o.info) and np.array_equal(gd.cpu().numpy(), o.done), t
        fin = np.isfinite(o.obs).all(axis=1)
        assert obs_bad_rows(go.cpu().numpy()[fin], o.obs[fin]).sum() == 0
        paid += int((o.info[:, 0] != 0).sum())
        if not use_sensor:   # 8 + 8 items, 10 / 5 slots per type: the food slots hold the nearest foods' OLD positions, whether or not they moved
            live = fin & (o.done == 0)
            nb = o.od - 2 * 2 * min(8, o.cfg.n_bins)
            food = go.cpu().numpy()[live, nb:nb + 2 * min(8, o.cfg.n_bins)].reshape(live.sum(), -1, 2)
            old = it0[live, :16].reshape(live.sum(), 8, 2)
            assert all(any(np.array_equal(f, q) for q in old[i]) for i in range(len(food)) for f in food[i]), t
            moved += int((np.any(it0[live, :16] != o.items[live, :16], axis=1)).sum())
    assert paid > 150, paid
    assert use_sensor or moved > 40, moved


def test_capsule_mid_sections_against_cubes_and_the_maze_box_on_device():
    """assets/ant.xml:16-55 capsules against assets/food.xml:12 cubes and the assets/box.xml:12 maze box: ants let down onto cubes with the
    MIDDLE of their feet (contact pickup, ant_gather_env.py:113-116: the touch is paid) and feet laid across the vertical edges of the maze
    box -- contacts no end-point sphere sees.  Device == oracle bit for bit, identical inputs every round."""
    import capsule_cases as cc
    n = 256
    g, o = make(K.HRL_ANT_GATHER, n, seed=4, robot_coll_dist=0.0)
    g.reset(); o.reset()
    rng = np.random.RandomState(8)
    paid = mid = 0

    def item_boxes(i):
        it = o.items[i, :32].reshape(16, 2).astype(np.float64)
        return {16 + k: (np.r_[it[k] - 0.125, -0.025], np.r_[it[k] + 0.125, 0.225]) for k in range(16)}
    for t in range(4):
        cc.cubes_under_the_feet(o, rng)
        mid += cc.count_mid_section_contacts(o, range(0, n, 16), item_boxes)
        push(g, o)
        for k in range(3):
            a = (rng.uniform(-1, 1, (n, 8)) * (0.0 if k == 0 else 0.3)).astype(np.float32)
            go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
            assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(g.items.cpu().numpy(), o.items), (t, k)
            assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(g.info.cpu().numpy(), o.info) and np.array_equal(gd.cpu().numpy(), o.done), (t, k)
            assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0
            paid += int((o.info[:, 0] != 0).sum())
    assert mid >= 30 and paid >= 400, (mid, paid)
    g, o = make(K.HRL_ANT_MAZE, n, seed=4)
    g.reset(); o.reset()
    box = {8: (np.array([-5., -2, 0]), np.array([1., 2, 2]))}
    mid = 0
    for t in range(4):
        cc.foot_across_the_maze_corner(o, rng)
        mid += cc.count_mid_section_contacts(o, range(0, n, 8), lambda i: box)
        push(g, o)
        for k in range(3):
            a = (rng.uniform(-1, 1, (n, 8)) * 0.3).astype(np.float32)
            go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
            assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), (t, k)
            assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done), (t, k)
            assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0
    assert mid >= 30, mid


def test_second_support_points_on_device():
    """A capsule that rests flat on a face of the maze box or on the top of an item cube gets a SECOND support point (Bullet keeps a manifold there):
    feet hanging alongside the box's vertical faces, legs stretched out level over cubes (tests/capsule_cases.py) -- states full of such contacts,
    counted; device == oracle bit for bit, with hrl_model.step_group 0 and 1 (both the four-wave group), a tight contact cap included."""
    import capsule_cases as cc
    n = 256
    rng = np.random.RandomState(12)
    for group, cap in ((0, 12), (1, 12), (0, 5)):
        g, o = make(K.HRL_ANT_MAZE, n, seed=4, model_step_group=group, model_max_contacts=cap)
        g.reset(); o.reset()
        g.count_solver_rows()
        seconds = 0
        for t in range(3):
            cc.feet_flat_against_the_maze_box(o, rng)
            seconds += cc.count_second_points(o, range(0, n, 4))
            push(g, o)
            for k in range(2):
                a = (rng.uniform(-1, 1, (n, 8)) * 0.3).astype(np.float32)
                go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
                assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), (group, cap, t, k)
                assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done) and np.array_equal(g.solver_rows.cpu().numpy(), o.solver_rows), (group, cap, t, k)
                assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0
        assert seconds >= (100 if cap == 12 else 20), (group, cap, seconds)
    for group in (0, 1):
        g, o = make(K.HRL_ANT_GATHER, n, seed=4, robot_coll_dist=0.0, model_step_group=group)
        g.reset(); o.reset()
        seconds = paid = 0
        for t in range(3):
            cc.feet_flat_on_cubes(o, rng)
            seconds += cc.count_second_points(o, range(0, n, 4))
            push(g, o)
            for k in range(2):
                a = (rng.uniform(-1, 1, (n, 8)) * 0.2).astype(np.float32)
                go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
                assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(g.items.cpu().numpy(), o.items), (group, t, k)
                assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(g.info.cpu().numpy(), o.info) and np.array_equal(gd.cpu().numpy(), o.done), (group, t, k)
                assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0
                paid += int((o.info[:, 0] != 0).sum())
        assert seconds >= 150 and paid >= 300, (group, seconds, paid)


def test_self_collision_rows_on_device():
    """Hips forced beyond their range so that capsules of different legs meet: the two-body rows (second impulse response,
    10-term row products) on the device equal the oracle's bit for bit."""
    import ctypes as C
    n = 256
    g, o = make(K.HRL_ANT_FLAT, n, seed=5)
    g.reset(); o.reset()
    rng = np.random.RandomState(1)
    seen = 0
    for t in range(20):
        if t % 5 == 0:
            o.state[:, 2] = 1.5; o.state[:, 15:29] = 0
            o.state[:, 7:15:2] = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
            o.state[:, 8:15:2] = rng.uniform(-1.8, 1.8, (n, 4)).astype(np.float32)
            for i in range(0, n, 16):
                q = o.state[i, :15].astype(np.float64); info = np.zeros(3, np.int32); dbg = np.zeros(13, np.int32)
                orc.lib().orc_ant_substeps_items_f64(C.byref(o.cfg), orc.ptr(q), orc.ptr(np.zeros(14)), orc.ptr(np.zeros(8)), 1, None, 0, orc.ptr(info), orc.ptr(dbg), None)
                seen += int((dbg[1:] >= 64).sum())
        push(g, o)
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done), t
    assert seen >= 10, seen


def test_flagrun_manual_goals_through_the_c_abi():
    """hrl_set_goals / hrl_next_target (manual_goal_creation, ant_flagrun_env.py:45,112-120): the list is consumed from its back
    (`goals.pop()`), the episode is over when it runs out; next_target() alone pops one goal, ok = 0 on an empty list."""
    import ctypes as C
    n, G = 64, 4
    g, o = make(K.HRL_ANT_FLAGRUN, n, seed=6, flag_manual_goals=1, flag_timeout=0)
    g.cfg.auto_reset = 0
    g.reset(); o.reset()
    assert np.array_equal(g.items.cpu().numpy(), o.items)
    goals = np.random.RandomState(0).uniform(-4, 4, (n, G, 2)).astype(np.float32)
    mask = np.ones(n, np.uint8); mask[::7] = 0
    gobs = g.set_goals(torch.from_numpy(goals).cuda(), torch.from_numpy(mask).cuda())
    orc.lib().orc_set_goals_batch_f32(C.byref(o.cfg), orc.ptr(o.state), orc.ptr(o.items), orc.ptr(o.aux), orc.ptr(goals), G, orc.ptr(mask), orc.ptr(o.obs))
    assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux)
    assert np.array_equal(o.items[mask == 1, 0:2], goals[mask == 1, G - 1])   # the LAST goal of the list is the first target
    assert obs_bad_rows(gobs.cpu().numpy(), o.obs).sum() == 0
    rng = np.random.RandomState(1)
    for t in range(10):
        o.state[:, 0:2] = ((15 * o.items[:, 0:2] - np.array([-6.0, 0.0], np.float32)) / 13).astype(np.float32)
        o.state[:, 2] = 0.5
        push(g, o)
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux), t
        # (the masked-out envs still chase (1e3, 0): teleported outside the arena they blow up to NaN on both sides alike)
        assert np.array_equal(gr.cpu().numpy(), o.rew, equal_nan=True) and np.array_equal(gd.cpu().numpy(), o.done), t
    # next_target() alone: envs 0..31 get one more goal as plain data, the others have an empty list (-> ok 0, unchanged)
    o.state[:, 0:3] = np.array([0.5, -0.5, 0.5], np.float32)
    o.items[:32, K.HRL_FLAG_PENDING_OFF:K.HRL_FLAG_PENDING_OFF + 2] = 1.25; o.aux[:32, 3] = (o.aux[:32, 3] & ~0xffff) | 1
    o.aux[32:, 3] &= ~0xffff
    push(g, o)
    gobs, ok = g.next_target()
    ok_o = np.zeros(n, np.uint8)
    orc.lib().orc_next_target_batch_f32(C.byref(o.cfg), orc.ptr(o.state), orc.ptr(o.items), orc.ptr(o.aux), None, orc.ptr(o.obs), orc.ptr(ok_o))
    assert np.array_equal(ok.cpu().numpy(), ok_o) and ok_o[:32].all() and not ok_o[32:].any()
    assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux)
    assert obs_bad_rows(gobs.cpu().numpy(), o.obs).sum() == 0
    from hrl_pybullet_envs_amd import _lib
    bad, _ = make(K.HRL_ANT_FLAGRUN, 4)
    with pytest.raises(_lib.HrlError, match='manual'):
        bad.set_goals(torch.zeros(4, 2, 2).cuda())
    close, oc = make(K.HRL_ANT_FLAGRUN, 32, seed=4, flag_manual_goals=1, flag_max_targets=0, flag_max_target_dist=3.0, flag_timeout=5)
    with pytest.raises(_lib.HrlError, match='hrl_next_target'):   # max_targets < 1: next_target() never reads the list (:113-114)
        close.set_goals(torch.zeros(32, 2, 2).cuda())
    close.reset(); oc.reset()
    gobs, ok = close.next_target()
    orc.lib().orc_next_target_batch_f32(C.byref(oc.cfg), orc.ptr(oc.state), orc.ptr(oc.items), orc.ptr(oc.aux), None, orc.ptr(oc.obs), None)
    assert bool(ok.all()) and np.array_equal(close.items.cpu().numpy(), oc.items) and obs_bad_rows(gobs.cpu().numpy(), oc.obs).sum() == 0
    for t in range(12):
        a = rng.uniform(-1, 1, (32, 8)).astype(np.float32)
        close.step(torch.from_numpy(a).cuda()); oc.step(a)
        assert np.array_equal(close.items.cpu().numpy(), oc.items) and np.array_equal(close.aux.cpu().numpy(), oc.aux), t
        assert np.array_equal(close.state.cpu().numpy(), oc.state), t


def test_flagrun_open_field_and_no_switch_on_device():
    """The two flagrun branches the device had not run (ant_flagrun_env.py:59-64 `enclosed=False`, :183-194
    `switch_flag_on_collision=False`), with the robots put where the branches matter: astride the absent wall, and on the goal."""
    import ctypes as C
    n = 64
    kw = dict(flag_enclosed=0, centroid_n_static=1, centroid_static_sum=(0.0, 0.0), flag_switch_on_collision=0, flag_timeout=6, flag_max_targets=3)
    g, o = make(K.HRL_ANT_FLAGRUN, n, seed=3, **kw)
    g.reset(); o.reset()
    o.state[:, 0] = 6.0; o.state[:, 2] = 0.3
    rng = np.random.RandomState(0)
    for t in range(5):
        push(g, o)
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state) and obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0, t
    assert np.all(np.abs(o.state[:, 0] - 6.0) < 0.5)
    g.reset(); o.reset()
    paid = np.zeros(n, int)
    for t in range(14):
        gl = np.zeros((n, 2), np.float32)
        for i in range(n):
            orc.lib().orc_flag_goal_f32(C.byref(o.cfg), int(o.aux[i, 2]), int(o.aux[i, 3] & 0xffff), orc.ptr(gl[i:i + 1]))
        o.state[:, 0:2] = ((14 * gl) / 13).astype(np.float32); o.state[:, 2] = 0.5
        push(g, o)
        a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state) and np.array_equal(g.aux.cpu().numpy(), o.aux), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0, t
        paid += (o.rew > 1000).astype(int)
    assert np.all(paid >= 3) and np.all(paid <= 4)   # once per goal (the goal only moves with the timeout); out of goals -> done -> auto-reset -> a new list


@pytest.mark.parametrize('auto_reset', [1, 0])
@pytest.mark.parametrize('kind', KINDS)
def test_envs_that_blow_up_match_too(kind, auto_reset):
    """Non-finite and absurd states -- velocities of 1e20 and inf, NaN coordinates of the robot or of an item, a torso 1e19 m away, robots inside
    a wall, joint angles far out of range -- go through the same arithmetic on both sides: what comes out (NaN, inf, done, the dying cost, the
    auto-reset that follows) is identical, bit for bit with NaNs compared as equal.  (A NaN item distance used to read 0 on the device and NaN
    in the oracle; a division replaced by a cheaper sequence that treats infinities differently shows up here too, not in a healthy run.)"""
    n = 128
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    g = BatchedEnv(_lib.default_config(kind, num_envs=n, seed=31, auto_reset=auto_reset), 'cuda:0')
    o = orc.OracleEnv(orc.default_config(kind, num_envs=n, seed=31, auto_reset=auto_reset), np.float32)
    g.reset(); o.reset()
    rng = np.random.RandomState(9)
    nq = 7 if kind == K.HRL_POINT_GATHER else 15
    for t in range(15):
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
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
            if kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
                o.items[rows[0:4], rng.randint(0, 32, 4)] = np.nan
                o.items[rows[4:8], rng.randint(0, 32, 4)] = np.inf
                o.items[rows[24:26], rng.randint(0, 32, 2)] = 1e30
            push(g, o)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True), t
        assert np.array_equal(g.aux.cpu().numpy(), o.aux) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert np.array_equal(gr.cpu().numpy(), o.rew, equal_nan=True) and np.array_equal(g.info.cpu().numpy(), o.info, equal_nan=True), t
        assert np.array_equal(go.cpu().numpy(), o.obs, equal_nan=True), t
        assert np.array_equal(g.items.cpu().numpy(), o.items, equal_nan=True), t
    assert int(o.done.sum()) >= 0


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
    from hrl_pybullet_envs_amd import _lib
    n, limit = 192, 9
    kw = dict(flag_timeout=4, flag_max_targets=3) if kind == K.HRL_ANT_FLAGRUN else {}
    g, o = make(kind, n, seed=5, max_episode_steps=limit, **kw)
    g.reset(); o.reset()
    g.final_obs.fill_(-7.0); o.final_obs[...] = -7.0
    rng = np.random.RandomState(8)
    n_trunc = n_term = 0
    for t in range(40):
        if t % 4 == 3 or t % 9 == 8:
            rows = rng.permutation(n)[:24]
            o.state[rows[:12], 15] = np.nan
            if kind != K.HRL_POINT_GATHER:
                o.state[rows[12:], 2] = 0.05; o.state[rows[12:], 17] = -3.0
            push(g, o)
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert np.array_equal(gi['TimeLimit.truncated'].cpu().numpy(), o.truncated), t
        assert np.array_equal(gi['final_observation'].cpu().numpy(), o.final_obs, equal_nan=True), t
        assert np.array_equal(go.cpu().numpy(), o.obs, equal_nan=True), t
        d = o.done.astype(bool)
        n_trunc += int(o.truncated.sum()); n_term += int((d & ~o.truncated.astype(bool)).sum())
    assert n_trunc >= 100 and n_term >= 40, (n_trunc, n_term)
    assert (o.final_obs != -7.0).any(axis=1).all()   # every env has ended at least once
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
    n = 256
    n_items = kw['n_food'] + kw['n_poison']
    g, o = make(kind, n, seed=19, **kw)
    assert g.items.shape[1] == orc.items_stride(o.cfg) == (64 if n_items == 32 else 128)
    g.reset(); o.reset()
    assert np.array_equal(g.items.cpu().numpy(), o.items) and obs_bad_rows(g.obs.cpu().numpy(), o.obs).sum() == 0
    contact = 'robot_coll_dist' in kw
    rng = np.random.RandomState(3)
    paid = moved_hi = 0
    for t in range(30):
        k = (np.arange(n) * 2 + t * 5) % n_items
        it = o.items[:, :2 * n_items].reshape(n, n_items, 2)[np.arange(n), k]
        if contact and kind == K.HRL_POINT_GATHER:
            side = rng.randint(0, 4, n); d = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)[side]
            lat = rng.uniform(-0.3, 0.3, n).astype(np.float32); gap = rng.uniform(-0.004, 0.01, n).astype(np.float32)
            o.state[:, 0:2] = it - d * (np.float32(0.475) + gap)[:, None] + d[:, ::-1] * lat[:, None]
            o.state[:, 2] = 0.35; o.state[:, 3:7] = [0, 0, 0, 1]; o.state[:, 7:13] = 0
        else:
            o.state[:, 0:2] = it + rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32) * np.float32(0.5 if not contact else 1.2)
        push(g, o)
        a = rng.uniform(-1, 1, (n, o.ad)).astype(np.float32)
        it0 = o.items.copy()
        go, gr, gd, gi = g.step(torch.from_numpy(a).cuda()); o.step(a)
        assert np.array_equal(g.state.cpu().numpy(), o.state, equal_nan=True) and np.array_equal(g.items.cpu().numpy(), o.items), t
        assert np.array_equal(gr.cpu().numpy(), o.rew) and np.array_equal(g.info.cpu().numpy(), o.info) and np.array_equal(gd.cpu().numpy(), o.done), t
        assert np.array_equal(go.cpu().numpy(), o.obs, equal_nan=True), t
        moved = np.any((o.items != it0).reshape(n, -1, 2), axis=2) & ~o.done.astype(bool)[:, None]
        moved_hi += int(moved[:, 16:n_items].sum()) if n_items <= 48 else int(moved[:, 48:n_items].sum())
        paid += int((o.info[:, 0] != 0).sum())
    assert moved_hi >= 80 and paid >= 200, (moved_hi, paid)


def test_manual_goal_lists_longer_than_15_through_the_c_abi():
    """flag_goal_capacity = 40: hrl_set_goals takes the 40-goal list (`env.goals = [...]` takes any, ant_flagrun_env.py:45), the pending list
    lives in a 96-float items record and is consumed back to front; one goal beyond the capacity is refused with a reason."""
    import ctypes as C
    from hrl_pybullet_envs_amd import _lib
    n, G = 48, 40
    g, o = make(K.HRL_ANT_FLAGRUN, n, seed=2, flag_manual_goals=1, flag_goal_capacity=G, flag_timeout=3, max_episode_steps=0)
    assert g.items.shape[1] == 96
    g.reset(); o.reset()
    goals = np.random.RandomState(0).uniform(-4, 4, (n, G, 2)).astype(np.float32)
    gobs = g.set_goals(torch.from_numpy(goals).cuda())
    orc.lib().orc_set_goals_batch_f32(C.byref(o.cfg), orc.ptr(o.state), orc.ptr(o.items), orc.ptr(o.aux), orc.ptr(goals), G, None, orc.ptr(o.obs))
    assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux) and obs_bad_rows(gobs.cpu().numpy(), o.obs).sum() == 0
    with pytest.raises(_lib.HrlError, match='flag_goal_capacity'):
        g.set_goals(torch.zeros(n, G + 1, 2).cuda())
    rng = np.random.RandomState(1)
    for t in range(3 * G + 2):
        a = rng.uniform(-0.3, 0.3, (n, 8)).astype(np.float32)
        go, gr, gd, _ = g.step(torch.from_numpy(a).cuda()); o.step(a)
        if t % 10 == 0 or t > 3 * G - 3:
            assert np.array_equal(g.items.cpu().numpy(), o.items) and np.array_equal(g.aux.cpu().numpy(), o.aux), t
            assert np.array_equal(g.state.cpu().numpy(), o.state) and obs_bad_rows(go.cpu().numpy(), o.obs).sum() == 0, t
    assert np.array_equal(gd.cpu().numpy(), o.done) and (o.done | (o.aux[:, 2] > 1)).all()   # every list ran out


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

    from hrl_pybullet_envs_amd.vec_env import BatchedEnv

    class Dev:   # the buffers of BatchedEnv under the names tests/orc.py::OracleEnv gives them, as numpy
        def __init__(self, cfg):
            self.e, self.ad = BatchedEnv(cfg, 'cuda:0'), orc.act_dim(cfg)

        def reset(self):
            self.e.reset()

        def step(self, a):
            self.e.step(torch.from_numpy(a).cuda())

        def __getattr__(self, name):
            t = getattr(self.e, {'rew': 'reward'}.get(name, name))
            a = t.cpu().numpy()
            if name == 'items' and not self.e._uses_items:   # kinds that keep nothing there hand the library NULL: the oracle's record stays zero
                a = np.zeros_like(a)
            return a
    want = json.load(open(S.PATH))
    got = S.fingerprint(Dev)
    assert got == want, [k for k in want if got.get(k) != want[k]]
