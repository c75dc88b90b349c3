"""Shared by tests/test_sensors_scale_host.py and tests/test_gpu_sensors_scale.py: the records of
thousands of envs the sensors are checked on at the workload's size -- the fp32 oracle's states of 30 seeded steps with a fixed, sparse pattern of spread, hostile and
hand-made envs written over them, so that neighbouring workgroups do unequal work --, one specification per sensor, and the host build
of every sensor on those records: the seven of SENSORS on SHAPES, and beside them the four of LATER (the chase camera, the ray test,
the closest points and the dynamics terms) on shapes of their own (LATER_SHAPES, DYN_CASES) (the device equals the oracle bit for bit, tests/test_gpu_parity.py: the whole expected side is
computable without a GPU).  Test infrastructure only."""
import collections
import functools
import math

import numpy as np

import cast_cases as cac
import chase_cases as chc
import closest_cases as clc
import dyn_cases as dc
import field_cases as fc
import frontier_cases as xc
import links_cases as lc
import orc
import probe_cases as pc
import render_cases as rc
import route_cases as rt
import scan_cases as sc
import see_cases as vc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import cast_device as Ca
from hrl_pybullet_envs_amd import chase_device as Ch
from hrl_pybullet_envs_amd import closest_device as Cl
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import frontier_device as X
from hrl_pybullet_envs_amd import probe_device as P
from hrl_pybullet_envs_amd import render_device as R
from hrl_pybullet_envs_amd import scan_device as S
from hrl_pybullet_envs_amd import see_device as V

SENSORS = ('render', 'scan', 'probe', 'field', 'route', 'see', 'frontier')
KINDS = (K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER)   # the three with BASELINE configs: items | the box and targets | the point bot
SHAPES = ((4096, (32, 32)), (1029, (64, 64)))   # (envs, grid): the benchmark's size | the longest relaxation; 1029 = 4 * 256 + 5: no multiple of 8 XCDs or 256 CUs
# the four sensors merged after the seven, beside them and not among them: (envs, size) per sensor -- chase: (width, height), 128 x 96 = 12
# chunks of 1024 pixels per workgroup | cast: rays per env, 129 = two full waves and one ray, 1024 = the maximum | closest: no size
LATER = ('chase', 'cast', 'closest', 'dyn')
LATER_SHAPES = {'chase': ((4096, (32, 16)), (1029, (128, 96))), 'cast': ((4096, 129), (1029, 1024)), 'closest': ((4096, None), (1029, None))}
# dyn reads the state and the model only, 16 envs per workgroup: (kind, envs, where the states come from) -- 4096 = 256 workgroups on
# records() | 16389 = 1024 workgroups and a tail of 5 envs, hand-made states (the oracle is not stepped at that size)
RECORDS, HAND_MADE = 'records', 'hand-made'
DYN_CASES = ((K.HRL_ANT_GATHER, 4096, RECORDS), (K.HRL_POINT_GATHER, 4096, RECORDS), (K.HRL_ANT_GATHER, 16389, HAND_MADE))
DYN_PLACES = (0, 4, 9, 16, 24)   # of a state record: x | a quaternion component | a joint angle | a velocity | a joint rate
STEPS, SEED = 30, 21
# every SPREAD_EVERY-th env (from SPREAD_AT) takes a placement of probe_cases.SPREAD, ...: three residues that never meet
SPREAD_EVERY, SPREAD_AT = 16, 3
HOSTILE_EVERY, HOSTILE_AT = 64, 21
HAND_EVERY, HAND_AT = 128, 77
CLEAR_EVERY, STILL_EVERY = 7, 5   # see: the envs whose memory starts over in the second launch | whose robot stands where it stood in the first
OUTSIDE = (1.0e3, 1.0e3)          # route: a start outside every grid


def uses_items(kind):
    return kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER, K.HRL_ANT_FLAGRUN)   # the library is handed NULL for the others (BatchedEnv._uses_items)


def config_args(n, seed=SEED):
    return dict(num_envs=n, seed=seed, auto_reset=1)


def actions(kind, n, seed=SEED):
    """The action stream [STEPS, n, act_dim] float32 both the oracle and a device env are given."""
    ad = orc.act_dim(orc.default_config(kind, **config_args(n, seed)))
    return np.random.RandomState(1000 * seed + kind).uniform(-1, 1, (STEPS, n, ad)).astype(np.float32)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(None)
def stepped(kind, n, seed=SEED):
    """(cfg, state, items, aux) of the fp32 oracle after reset + STEPS steps of actions(): what a device env holds after the same."""
    cfg = orc.default_config(kind, **config_args(n, seed))
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    for a in actions(kind, n, seed):
        o.step(a)
    return (cfg,) + frozen(o.state.copy(), o.items.copy(), o.aux.copy())


def turns(n, every, at):
    """(env, how many such envs came before it) of every `every`-th env from `at`."""
    return list(enumerate(range(at, n, every)))


def hostile_record(cfg, st, it, aux, turn):
    """Entry turn % 5 of scan_cases.hostile (NaN, +inf, -inf, 1e20 | a target index out of range) as its row (turn // 5) % 5 has it (the
    robot's x | its y | a food item | a poison item | the target alone), of one env's records."""
    shard = [np.repeat(a[None], 5, 0) for a in (st, it, aux)]
    s, i2, a = sc.hostile(cfg, *shard)[turn % 5][:3]
    row = (turn // 5) % 5
    return s[row], i2[row], a[row]


@functools.lru_cache(None)
def records(kind, n, seed=SEED):
    """(cfg, state, items, aux) for n envs: stepped() with the pattern of unequal envs written over it."""
    cfg, st, it, aux = stepped(kind, n, seed)
    st, it, aux = st.copy(), it.copy(), aux.copy()
    for k, e in turns(n, SPREAD_EVERY, SPREAD_AT):
        st[e] = pc.spread(cfg, np.repeat(st[e][None], 5, 0))[k % 5]
    for k, e in turns(n, HOSTILE_EVERY, HOSTILE_AT):
        st[e], it[e], aux[e] = hostile_record(cfg, st[e], it[e], aux[e], k)
    for k, e in turns(n, HAND_EVERY, HAND_AT):
        st[e] = rc.hand_made(cfg, np.repeat(st[e][None], 3, 0))[k % 3]
    return (cfg,) + frozen(st, it, aux)


@functools.lru_cache(None)
def hand_made_records(kind, n, seed=SEED):
    """(cfg, state, items, aux) for n ant envs whose states are blocks of dyn_cases.hand_made(seed + k, 12) -- tilted torsos, joints at
    and between their stops, velocities of the shards' scale --, columns 29..31, items and aux as the oracle's reset leaves them (what a
    device env of that size holds after reset()), and every HOSTILE_EVERY-th env with a NaN in place DYN_PLACES[turn % 5]."""
    cfg = orc.default_config(kind, **config_args(n, seed))
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    st = np.concatenate([dc.hand_made(seed + k, 12) for k in range((n + 11) // 12)])[:n].astype(np.float32)
    st[:, 29:32] = o.state[:, 29:32]
    for k, e in turns(n, HOSTILE_EVERY, HOSTILE_AT):
        st[e, DYN_PLACES[k % 5]] = np.nan
    return (cfg,) + frozen(st, o.items.copy(), o.aux.copy())


def records_of(sensor, kind, n, size, seed=SEED):
    """The records a case is built on: records(), but for dyn's hand-made case."""
    return hand_made_records(kind, n, seed) if (sensor, size) == ('dyn', HAND_MADE) else records(kind, n, seed)


def blind(state):
    """The envs whose robot has no finite place."""
    return ~np.isfinite(state[:, 0:2]).all(1)


# ------------------------------------------------------------------------------------------------ one specification per sensor
def margin_of(kind):
    return 0.35 if kind == K.HRL_POINT_GATHER else 0.4   # the point bot's half side | the torso's radius and a leg's


def field_spec(kind, size):
    """A grid that turns with the robot and spans the arena's width about it, towards the kind's goal: a blind env blocks every cell."""
    return fc.spec_of(size, F.HRL_VIEW_EGO_HEADING, margin_of(kind), F.FOOD | F.TARGET, half=fc.WORLD_HALF[kind])


def route_spec(kind, size):
    """The world grid of the whole arena, P = 5 starts given in world coordinates, K = 7, for a load of 0.8 m radius that every item is
    in the way of, towards the robot or the target: in the maze the routes go round the box, among 16 items grown by 0.8 m they wind
    (a torso-sized disc among the poison alone never needs more than 7 waypoints in these arenas: nothing would be truncated)."""
    fspec = fc.spec_of(size, F.HRL_VIEW_WORLD, 0.8, F.ROBOT | F.TARGET, blocking=F.WALL | F.BOX | F.FOOD | F.POISON, kind=kind, centre=fc.WORLD_CENTRE)
    return rt.spec_of(fspec, P.HRL_PROBE_WORLD, 5, 7)


def see_spec(kind, size):
    """The kind's default occluders, 200 degrees about the heading, 4 m, a slack of one cell, on the world grid the frontier shares."""
    return vc.spec_of(size, V.HRL_VIEW_WORLD, V.WALL | V.BOX, math.cos(math.radians(100.0)), 4.0, None, kind=kind, centre=fc.WORLD_CENTRE)


SPECS = {'render': lambda kind, size: rc.view_of(kind, R.HRL_VIEW_EGO_HEADING, (48, 32)),
         'scan': lambda kind, size: sc.spec_of(65, S.HRL_SCAN_HEADING, 20.0),
         'probe': lambda kind, size: pc.spec_of(65, P.HRL_PROBE_HEADING, 0.4),
         'field': field_spec,
         'route': route_spec,
         'see': see_spec,
         'frontier': lambda kind, size: xc.spec_of(size, margin_of(kind), X.EDGE, X.KNOWN_ONLY, kind=kind)}


def n_links(kind):
    return 1 if kind == K.HRL_POINT_GATHER else 13


# the four of LATER.  chase: the heading frame, the library's default orbit (3 m behind the torso, 30 degrees above it), every class, a
# ground checker of 1 m | cast: the link frame, which reads all 13 link frames of the env from LDS, every class | closest: every class |
# dyn: 16 sites over every link (and tau, of inputs())
SPECS.update({'chase': lambda kind, size: chc.spec_of(size, Ch.HRL_SCAN_HEADING, Ch.HRL_EYE_TORSO, 0.0, 0.0, -30.0, 3.0, Ch.EVERYTHING, tile=1.0),
              'cast': lambda kind, size: cac.spec_of(Ca.HRL_CAST_LINK, size, Ca.EVERYTHING),
              'closest': lambda kind, size: clc.spec_of(Cl.EVERYTHING),
              'dyn': lambda kind, size: dc.spec_of(lc.sixteen_sites(n_links(kind)))})
SHARED = ('ray_link',)   # the members of a case's `extra` that all envs share: no row per env


def cast_rays(kind, n, R, seed):
    """(rays [n, R, 6] float32, ray_link [R] int32) in link coordinates, built at once for all envs: one seeded pattern -- a lidar of 4
    rings x 16 from the torso (link 0), a range finder of 1 m at each foot tip (the ants), then random segments on random links up to R
    --, the same for every env but for a seeded move of every ray's `to` by at most 0.2 m along each axis."""
    rng = np.random.default_rng(seed)
    parts, links = [Ca.lidar_rays(16, (-30.0, -10.0, 0.0, 15.0), 8.0, 0.3).numpy()], [np.zeros(64, np.int32)]
    if kind != K.HRL_POINT_GATHER:
        feet, foot_links = Ca.down_rays(1.0)
        parts.append(feet.numpy()); links.append(foot_links.numpy())
    fill = R - sum(len(p) for p in parts)
    a = np.stack((rng.uniform(-2, 2, fill), rng.uniform(-2, 2, fill), rng.uniform(-0.4, 1.5, fill)), 1)
    b = np.stack((rng.uniform(-6, 6, fill), rng.uniform(-6, 6, fill), rng.uniform(-1.0, 0.5, fill)), 1)
    parts.append(np.concatenate((a, b), 1)); links.append(rng.integers(0, n_links(kind), fill))
    pattern = np.concatenate(parts).astype(np.float32)
    rays = np.ascontiguousarray(np.broadcast_to(pattern, (n, R, 6)))
    rays[:, :, 3:6] += rng.uniform(-0.2, 0.2, (n, R, 3)).astype(np.float32)
    return rays, np.concatenate(links).astype(np.int32)


def see_inputs(cfg, state, seed):
    """(first, clear): the states of the first launch -- every robot moved by up to 3 m along x and y, every STILL_EVERY-th left where it
    is -- and the envs whose memory the second launch clears."""
    n = len(state)
    first = np.array(state)
    move = np.random.RandomState(seed).uniform(-3, 3, (n, 2)).astype(np.float32)
    move[::STILL_EVERY] = 0
    first[:, 0:2] += move
    return first, (np.arange(n) % CLEAR_EVERY == 0).astype(np.uint8)


def see_first(cfg, items, aux, spec, first):
    """The map of the first launch: from `first`, every memory cleared."""
    n = len(first)
    out = vc.See(*(np.zeros(shape, dt) for shape, dt in zip(vc.shapes_of(n, spec), vc.DTYPES)))
    return vc.see_host(cfg, first, items if uses_items(cfg.env_kind) else None, aux, spec, clear=np.ones(n, np.uint8), out=out)


def see_host(cfg, state, items, aux, spec, first, clear):
    """The map after two launches: see_first(), then from `state` with `clear` on the memory that left."""
    return vc.see_host(cfg, state, items, aux, spec, clear=clear, out=see_first(cfg, items, aux, spec, first))


def inputs(sensor, kind, n, size, seed=SEED):
    """What the sensor is handed besides the records and its spec, as a dict of arrays with one row per env."""
    cfg, st, it, aux = records_of(sensor, kind, n, size, seed)
    spec = SPECS[sensor](kind, size)
    if sensor == 'cast':
        return dict(zip(('rays', 'ray_link'), cast_rays(kind, n, size, 31 + kind)))
    if sensor == 'dyn':
        return dict(tau=dc.taus(cfg, n))
    if sensor == 'probe':
        return dict(points=pc.draw_points(cfg, st, spec.frame, spec.n_points, pc.seed_of(cfg, spec)))
    if sensor == 'route':
        drawn, _ = rt.draw_starts(cfg, st, rt.R.field_spec(spec), spec.frame, 3, 11 + kind)
        starts = np.concatenate([st[:, None, 0:2], drawn, np.broadcast_to(np.float32(OUTSIDE), (n, 1, 2))], 1)   # the robot | three drawn | one outside
        return dict(starts=np.ascontiguousarray(starts, np.float32))
    if sensor == 'see':
        first, clear = see_inputs(cfg, st, 5 + kind)
        return dict(first=first, clear=clear)
    if sensor == 'frontier':   # on the memory the see case leaves
        return dict(seen=expected('see', kind, n, size, seed).want.seen)
    return {}


def sub_config(cfg, n):
    c = K.hrl_config.from_buffer_copy(bytes(cfg))
    c.num_envs = n
    return c


def host_build(sensor, cfg, state, items, aux, spec, extra):
    """The host build of `sensor` on these records, every output, as the namedtuple (render: the array; scan: the pair) of its suite."""
    items = items if uses_items(cfg.env_kind) else None
    if sensor == 'render':
        return rc.render_host(cfg, state, items, aux, spec)
    if sensor == 'scan':
        return sc.scan_host(cfg, state, items, aux, spec)
    if sensor == 'probe':
        return pc.probe_host(cfg, state, items, aux, spec, extra['points'])
    if sensor == 'field':
        return fc.field_host(cfg, state, items, aux, spec)
    if sensor == 'route':
        return rt.route_host(cfg, state, items, aux, spec, extra['starts'])
    if sensor == 'see':
        return see_host(cfg, state, items, aux, spec, extra['first'], extra['clear'])
    if sensor == 'chase':
        return chc.chase_host(cfg, state, items, aux, spec)
    if sensor == 'cast':
        return cac.cast_host(cfg, state, items, aux, spec, extra['rays'], extra['ray_link'])
    if sensor == 'closest':
        return clc.closest_host(cfg, state, items, aux, spec)
    if sensor == 'dyn':
        return dc.dyn_host(cfg, state, spec, tau=extra['tau'])
    return xc.frontier_host(cfg, state, items, aux, spec, np.ascontiguousarray(extra['seen']))


def host_build_rows(sensor, case, rows):
    """host_build of the envs `rows` (a slice) of a case alone, as a shard of their own."""
    st, it, aux = (np.ascontiguousarray(a[rows]) for a in (case.state, case.items, case.aux))
    return host_build(sensor, sub_config(case.cfg, len(st)), st, it, aux, case.spec, {k: v if k in SHARED else np.ascontiguousarray(v[rows]) for k, v in case.extra.items()})


def members(out):
    """The arrays of a host build's output, in order."""
    return [out] if isinstance(out, np.ndarray) else list(out)


Case = collections.namedtuple('Case', 'cfg state items aux spec extra want')


@functools.lru_cache(None)
def expected(sensor, kind, n, size, seed=SEED):
    """The case of (sensor, kind, batch shape): records, spec, further inputs and the host build's outputs (computed once, read-only)."""
    cfg, st, it, aux = records_of(sensor, kind, n, size, seed)
    spec, extra = SPECS[sensor](kind, size), inputs(sensor, kind, n, size, seed)
    frozen(*extra.values())
    want = host_build(sensor, cfg, st, it, aux, spec, extra)
    frozen(*members(want))
    return Case(cfg, st, it, aux, spec, extra, want)


def later_cases():
    """(sensor, kind, envs, size) of every case of the four of LATER."""
    out = [(s, kind, n, size) for s in LATER[:3] for kind in KINDS for n, size in LATER_SHAPES[s]]
    return out + [('dyn', kind, n, source) for kind, n, source in DYN_CASES]


# ------------------------------------------------------------------------------------------------ the comparison at scale
def host_rows(want):
    """Every output of a host build as bytes [n, bytes per env]."""
    return [np.ascontiguousarray(w).reshape(len(w), -1).view(np.uint8) for w in want]


def nan_for_nan(rows):
    """Rows of float32 as bytes with every NaN replaced by one NaN: the payload and the sign of a NaN are the processor's own (dyn's
    hostile envs; tests/test_gpu_dyn.py and tests/test_gpu_links_scale.py hold a NaN against a NaN likewise)."""
    out = []
    for r in rows:
        f = np.array(r).view(np.float32)
        f[np.isnan(f)] = np.float32(np.nan)
        out.append(f.view(np.uint8))
    return out


def differences(names, got, want, envs=None):
    """The first few (output, env, byte within the env's row, env % 8) where two lists of [rows, bytes] arrays differ (`envs`: the env
    of each row; None: row i is env i), and how the wrong envs fall on the eight residues (a pattern by XCD or by place in the batch
    shows here)."""
    first, by_residue = [], np.zeros(8, int)
    for name, g, w in zip(names, got, want):
        bad = np.nonzero((g != w).any(1))[0]
        ids = bad if envs is None else envs[bad]
        by_residue += np.bincount(ids % 8, minlength=8)
        first += [(name, int(e), int(np.nonzero(g[r] != w[r])[0][0]), int(e % 8)) for r, e in zip(bad[:4], ids[:4])]
    return dict(first=first, wrong_envs=int(by_residue.sum()), wrong_envs_by_residue=by_residue.tolist())


# ------------------------------------------------------------------------------------------------ what the records reach
def classes(codes):
    """The class codes (code & 0xff) that occur."""
    return set(np.unique(np.asarray(codes) & 0xff).tolist())


def colours(img):
    packed = np.unique(img.reshape(-1, 3).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32))
    return {(int(c) >> 16, int(c) >> 8 & 255, int(c) & 255) for c in packed}


def reached(sensor, kind, n, size, seed=SEED):
    """Counts, from the host build's outputs, of what the case is about (the floors of tests/test_sensors_scale_host.py are conditions
    on these)."""
    c = expected(sensor, kind, n, size, seed)
    w, dead = c.want, blind(c.state)
    if sensor in ('chase', 'cast'):   # seg [n, ...]: class | index << 8 | face << 16; the robot's index is the link
        seg = w.seg.reshape(n, -1)
        robot = (seg & 255) == Ch.HIT_ROBOT
        out = dict(classes=classes(seg), links=set(np.unique((seg[robot] >> 8) & 255).tolist()), robot_envs=int(robot.any(1).sum()), blind=int(dead.sum()))
        if sensor == 'cast':
            out.update(hits=int((seg != 0).sum()), misses=int((seg == 0).sum()), blind_hits=int((seg[dead] != 0).sum()))
        return out
    if sensor == 'closest':
        d = w.distance
        return dict(finite=np.isfinite(d).sum((0, 1)).tolist(), negative=(d < 0).sum((0, 1)).tolist(), none=(d == np.inf).sum((0, 1)).tolist(), nan=int(np.isnan(d).sum()),
                    blind=int(dead.sum()), blind_cells=int(np.isfinite(d[dead]).sum()))
    if sensor == 'dyn':
        hostile = np.zeros(n, bool)
        hostile[HOSTILE_AT::HOSTILE_EVERY] = True
        finite = {name: np.isfinite(a.reshape(n, -1)).all(1) for name, a in zip(dc.NAMES, w)}
        every = np.logical_and.reduce(list(finite.values()))
        return dict(hostile=int(hostile.sum()), hostile_not_finite=int((hostile & ~every).sum()), hostile_bias_or_accel=int((hostile & ~(finite['bias'] & finite['accel'])).sum()),
                    others_not_finite=int((~hostile & ~every).sum()))
    if sensor == 'render':
        return dict(colours=colours(w))
    if sensor == 'scan':
        return dict(hits=classes(w[1]), blind=int(dead.sum()))
    if sensor == 'probe':
        return dict(nearest=classes(w.nearest), blockers=classes(w.blocker), vias=set(np.unique(w.via).tolist()))
    if sensor == 'field':
        has_blocked, has_way = (w.parent == F.BLOCKED).any((1, 2)), (np.isfinite(w.dist) & (w.dist > 0)).any((1, 2))
        return dict(mixed=int((has_blocked & has_way).sum()), all_blocked=int((w.parent == F.BLOCKED).all((1, 2)).sum()), blind=int(dead.sum()))
    if sensor == 'route':
        return dict(bent=int((w.count >= 3).sum()), none=int((w.count == 0).sum()), truncated=int((w.count > c.spec.max_waypoints).sum()), routes=int((w.count > 0).sum()))
    if sensor == 'see':
        still = (c.extra['first'][:, 0:2] == c.state[:, 0:2]).all(1) & (c.extra['clear'] == 0)
        return dict(fresh=int((w.fresh > 0).sum()), stale=int((w.fresh == 0).sum()), still_and_stale=int((still & (w.fresh == 0) & ~dead).sum()), lit=int(w.visible.any((1, 2)).sum()))
    return dict(with_edge=int((w.count > 0).sum()), reached=int((w.cell >= 0).sum()), cut_off=int(((w.count > 0) & (w.cell < 0)).sum()), no_edge=int((w.count == 0).sum()))
