"""The sensor config matrix: the constructor configurations, other than the six defaults, on which the eight sensors (render, scan, probe,
field, route, see, frontier, camera) are checked -- the host build against fp64 in tests/test_<sensor>_host.py, the device against the
host build in tests/test_gpu_<sensor>.py.  It covers only what the sensors read from the config and the records: more than 16 items (an
items record of 64 or 128 floats, hit codes with an index above 15), a 96-float flagrun record, arenas that are not the default square
(and flagrun's open field, which has none), and a maze with a target list of its own.  The entries are spelled like those of
parity_cases.CONFIG_MATRIX.  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import orc
import render_cases as rc
from hrl_pybullet_envs_amd import _capi as K

N = 5
MATRIX = [
    ('gather-64', K.HRL_ANT_GATHER, dict(n_food=40, n_poison=24, n_bins=64, world_size=(8.0, 8.0))),
    ('point-64', K.HRL_POINT_GATHER, dict(n_food=33, n_poison=31, n_bins=40, world_size=(8.0, 8.0))),
    ('gather-32', K.HRL_ANT_GATHER, dict(n_food=20, n_poison=12, n_bins=24, world_size=(9.0, 9.0))),
    ('gather-tall', K.HRL_ANT_GATHER, dict(n_food=5, n_poison=3, world_size=(9.0, 11.0))),
    ('gather-wide', K.HRL_ANT_GATHER, dict(world_size=(14.0, 6.0))),
    ('gather-nofood', K.HRL_ANT_GATHER, dict(n_food=0, n_poison=3)),   # one item class empty: every item is poison, item 0 included
    ('maze-12', K.HRL_ANT_MAZE, dict(sense_target=1, targets=[(-2 + 0.5 * i, -4 + 0.1 * i) for i in range(12)])),
    ('mazemj-3', K.HRL_ANT_MAZE_MJ, dict(targets=[(3.0, 4.0), (-6.0, -6.0), (6.0, 0.0)])),
    ('flagrun-open', K.HRL_ANT_FLAGRUN, dict(flag_enclosed=0, centroid_n_static=1, centroid_static_sum=(0.0, 0.0))),   # no lateral plane at all
    ('flagrun-small', K.HRL_ANT_FLAGRUN, dict(world_size=(5.0, 5.0), flag_size=3.0, flag_max_targets=0, flag_max_target_dist=2.5)),
    ('flagrun-manual-40', K.HRL_ANT_FLAGRUN, dict(flag_manual_goals=1, flag_goal_capacity=40)),   # a 96-float record; 20 goals through set_goals
]
NAMES = tuple(m[0] for m in MATRIX)
_ENTRY = {m[0]: m for m in MATRIX}
MANUAL_GOALS = 20
MAZE_12_TARGETS = (0, 3, 7, 8, 11)   # aux[:, 3] of the maze-12 shard: the default mazes' lists end at 3 and 4
# where the tests that need every robot clear of the edges between cells put the centre of a library default grid: about the origin the
# spread robot at (3, 6) stands on an edge of flagrun's default grid (cells of 0.1875 m), and about field_cases.WORLD_CENTRE the one at
# (-2.37, 2.19) on one of the 8 x 8 arenas' (cells of 0.125 m); asserted on the reference alone wherever it matters
DEFAULT_CENTRE = (0.013, -0.021)
NEAR_ITEMS = ((1, 50, (0.6, 0.3)), (3, -1, (-0.4, 0.7)))   # (env, item (-1: the last), offset from the robot) on the entries of more than 48 items


def kind_of(name):
    return _ENTRY[name][1]


def overrides(name):
    return dict(_ENTRY[name][2])


def seed_of(name):
    return 31 + NAMES.index(name)


def many_items(cfg):
    """The entry has items 48..63: a record of 128 floats."""
    return cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER) and cfg.n_food + cfg.n_poison > 48


def goals_of(name):
    """The goals of a manual-goal entry, float32 [N, MANUAL_GOALS, 2] inside the arena; None for every other entry."""
    if not overrides(name).get('flag_manual_goals'):
        return None
    return np.random.RandomState(seed_of(name)).uniform(-4, 4, (N, MANUAL_GOALS, 2)).astype(np.float32)


def host_config(name, **more):
    """The entry's config from the oracle's defaults (orc.default_config sets scalars, world_size and targets; the other arrays here)."""
    over = overrides(name)
    over.update(more)
    for k in ('centroid_static_sum',):
        if k in over:
            over[k] = (C.c_float * 2)(*over[k])
    return orc.default_config(kind_of(name), **over)


@functools.lru_cache(None)
def shard(name):
    """(cfg, state, items, aux) of 5 envs of the entry on the fp32 oracle: reset (a manual-goal entry is then given its goals) + 30
    random-action steps.  Computed once, never modified.  maze-12: aux[:, 3] is then set to 0, 3, 7, 8 and 11; the entries of more than
    48 items: envs 1 and 3 get item 50 and the last item moved to within 1 m of the robot."""
    cfg = host_config(name, num_envs=N, seed=seed_of(name), auto_reset=1)
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    if goals_of(name) is not None:
        o.set_goals(goals_of(name))
    rng = np.random.RandomState(200 + seed_of(name))
    for _ in range(30):
        o.step(rng.uniform(-1, 1, (N, o.ad)))
    ar = rc.arena(cfg)
    assert (np.abs(o.state[:, :2]) <= (8.0 if ar is None else np.array(ar))).all()   # every robot stands inside its arena
    if name == 'maze-12':
        o.aux[:, 3] = MAZE_12_TARGETS
    if many_items(cfg):
        for e, i, (dx, dy) in NEAR_ITEMS:
            i %= cfg.n_food + cfg.n_poison
            assert i >= 48
            o.items[e, 2 * i:2 * i + 2] = (o.state[e, 0] + dx, o.state[e, 1] + dy)
            assert (np.abs(o.items[e, 2 * i:2 * i + 2]) < np.array(ar)).all()
    for a in (o.state, o.items, o.aux):
        a.setflags(write=False)
    return cfg, o.state, o.items, o.aux


def hostile(name, generator, records=None):
    """The hostile-state generator of a sensor's cases module (render_cases.hostile, scan_cases.hostile, probe_cases.hostile) applied to
    the entry's shard (or to `records` = (cfg, state, items, aux)): a list of (state, items, aux, cleaned state, cleaned items, cleaned
    aux, far, blind), `blind` empty where the generator names none.  On the entries of more than 48 items one more case puts NaN and
    +-inf into the LAST item of three envs; its clean twin has that item at an eaten one's place."""
    cfg, state, items, aux = records if records is not None else shard(name)
    out = [tuple(c[:7]) + (tuple(c[7]) if len(c) > 7 else (),) for c in generator(cfg, state, items, aux)]
    if many_items(cfg):
        last = 2 * (cfg.n_food + cfg.n_poison - 1)
        it, cit = np.array(items), np.array(items)
        it[4, last] = np.nan
        it[1, last + 1] = np.inf
        it[2, last:last + 2] = (-np.inf, np.nan)
        for e in (4, 1, 2):
            cit[e, last:last + 2] = (100.0, 0.0)
        out.append((np.array(state), it, np.array(aux), np.array(state), cit, np.array(aux), False, ()))
    return out


def saw_a_late_item(codes):
    """Some code of `codes` (class | index << 8 [| face << 16]; food is class 3, poison 4) names an item of index 48 or more."""
    codes = np.asarray(codes).astype(np.int64)
    return bool((np.isin(codes & 255, (3, 4)) & ((codes >> 8 & 255) >= 48)).any())


# ------------------------------------------------------------------------------------------------ the device side
def device_config(name, **more):
    from hrl_pybullet_envs_amd import _lib
    over = overrides(name)
    over.update(more)
    return _lib.default_config(kind_of(name), **over)


@functools.lru_cache(None)
def device_env(name):
    """The entry as a BatchedEnv of 5 on cuda:0 after reset (a manual-goal entry is then given its goals): made once; the tests write the
    shard's records into its tensors (test_gpu_render.put)."""
    import torch
    from test_gpu_render import make_env
    env = make_env(kind_of(name), seed=seed_of(name) - kind_of(name), **overrides(name))
    env.reset()
    if goals_of(name) is not None:
        env.set_goals(torch.from_numpy(goals_of(name)))
    torch.cuda.synchronize()
    assert env.items.shape[1] == shard(name)[2].shape[1] and bytes(env.cfg) == bytes(shard(name)[0])
    return env
