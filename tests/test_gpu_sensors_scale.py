"""The seven sensors of scale_cases.SENSORS (render, scan, probe, field, route, see, frontier; chase, cast, closest and dyn: under the same
protocol in the second half of this file, with sizes of their own; the camera and the link states: tests/test_gpu_camera_scale.py,
tests/test_gpu_links_scale.py) on the MI355X at the sizes they are run at: 4096 envs on 32 x 32 grids and 1029 envs on 64 x 64 grids, every output of
every env against the host build (tests/scale_cases.py; its expected side is checked in tests/test_sensors_scale_host.py), bit for bit.
Thousands of workgroups are then resident together and queue behind one another; a step of another env of the same size runs directly
before every sensor launch, as in the workload, and leaves its LDS behind; neighbouring envs do unequal work (spread, hostile and
hand-made envs in a sparse pattern).  Every case launches once, 20 more times into a second set of outputs, and once under a mask; all
outputs are views into allocations with 8 guard rows of sentinel behind them.  The per-sensor suites keep the breadth at N = 5."""
import functools
import time

import numpy as np
import pytest
import torch

import scale_cases as sx
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import cast_device as Ca
from hrl_pybullet_envs_amd import chase_device as Ch
from hrl_pybullet_envs_amd import closest_device as Cl
from hrl_pybullet_envs_amd import dyn_device as Dy
from scale_cases import differences, host_rows   # the byte-row comparison (tests/test_sensors_scale_host.py checks that it can fail)
from test_gpu_field import same as same_field
from test_gpu_frontier import same as same_frontier
from test_gpu_probe import same as same_probe
from test_gpu_render import put
from test_gpu_route import same as same_route
from test_gpu_scan import same as same_scan
from test_gpu_see import same as same_see

pytestmark = pytest.mark.gpu
SENTINEL, GUARD_ROWS, REPEATS = 0x7B, 8, 20
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}
SAME = {'render': lambda a, b: np.array_equal(a[0].cpu().numpy(), b[0]), 'scan': same_scan, 'probe': same_probe, 'field': same_field, 'route': same_route,
        'see': same_see, 'frontier': same_frontier}


@functools.lru_cache(None)
def device(kind, n):
    """(the env under test, a second env of the same kind and size, an action for it): the first after reset + 30 steps of
    scale_cases.actions(), its records equal to the oracle's of scale_cases.stepped() bit for bit -- the floors of
    tests/test_sensors_scale_host.py are computed from those.  Made once per kind and size."""
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    ocfg, st, it, aux = sx.stepped(kind, n)
    cfg = _lib.default_config(kind, **sx.config_args(n))
    assert bytes(cfg) == bytes(ocfg)
    env, other = BatchedEnv(cfg, 'cuda:0'), BatchedEnv(_lib.default_config(kind, **sx.config_args(n)), 'cuda:0')
    env.reset(); other.reset()
    acts = torch.from_numpy(sx.actions(kind, n)).cuda()
    for a in acts:
        env.step(a)
    torch.cuda.synchronize()
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), st.view(np.uint32)), (kind, n, 'state')
    assert np.array_equal(env.aux.cpu().numpy(), aux), (kind, n, 'aux')
    if sx.uses_items(kind):
        assert np.array_equal(env.items.cpu().numpy().view(np.uint32), it.view(np.uint32)), (kind, n, 'items')
    return env, other, acts[0]


def wrap(sensor, tensors):
    """The list of output tensors as the `out=` of the sensor's method."""
    from hrl_pybullet_envs_amd import field_device, frontier_device, probe_device, route_device, see_device
    return {'render': lambda t: t[0], 'scan': tuple, 'probe': lambda t: probe_device.Probe(*t), 'field': lambda t: field_device.Field(*t),
            'route': lambda t: route_device.Route(*t), 'see': lambda t: see_device.See(*t), 'frontier': lambda t: frontier_device.Frontier(*t)}[sensor](tensors)


class Arena:
    """One allocation per output, n + GUARD_ROWS env-rows of SENTINEL bytes each; `out`: the views of the first n rows."""

    def __init__(self, want):
        self.n = len(want[0])
        self.whole = [torch.full(((self.n + GUARD_ROWS) * w[0].nbytes,), SENTINEL, dtype=torch.uint8, device='cuda') for w in want]
        self.out = [b.view(TORCH[w.dtype]).view((self.n + GUARD_ROWS,) + w.shape[1:])[:self.n] for b, w in zip(self.whole, want)]

    def guards_intact(self):
        return all(bool((b.view(self.n + GUARD_ROWS, -1)[self.n:] == SENTINEL).all()) for b in self.whole)

    def rows(self):
        """Every output as bytes [n, bytes per env] on the host."""
        return [b.view(self.n + GUARD_ROWS, -1)[:self.n].cpu().numpy() for b in self.whole]


class Launcher:
    """The launches of one case: the overwritten records are put into the env, what the sensor is handed besides is on the device."""

    def __init__(self, sensor, case, env, other, action):
        self.sensor, self.case, self.env, self.other, self.action = sensor, case, env, other, action
        put(env, case.state, case.items, case.aux)
        self.dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in case.extra.items()}
        if sensor == 'see':
            self.dev['state'], self.dev['all'] = torch.from_numpy(np.array(case.state)).cuda(), torch.ones(len(case.state), dtype=torch.uint8, device='cuda')

    def sensor_launch(self, mask, out, **over):
        s, env, spec, dev = self.sensor, self.env, self.case.spec, dict(self.dev, **over)
        o = wrap(s, out)
        if s == 'render':
            env.render(spec, mask=mask, out=o)
        elif s == 'scan':
            env.scan(spec, mask=mask, out=o)
        elif s == 'probe':
            env.probe(dev['points'], spec, mask=mask, out=o)
        elif s == 'field':
            env.field(spec, mask=mask, out=o)
        elif s == 'route':
            env.route(dev['starts'], spec, mask=mask, out=o)
        elif s == 'see':
            env.see(spec, clear=dev['clear'], mask=mask, out=o)
        else:
            env.frontier(dev['seen'], spec, mask=mask, out=o)

    def __call__(self, mask, out):
        """A step of the second env, then the sensor, on one stream with no synchronisation between them (see: twice -- from the first
        states with every memory cleared, then from the records with `clear`)."""
        if self.sensor == 'see':
            self.env.state.copy_(self.dev['first'])
            self.other.step(self.action)
            self.sensor_launch(mask, out, clear=self.dev['all'])
            self.env.state.copy_(self.dev['state'])
        self.other.step(self.action)
        self.sensor_launch(mask, out)


def check(sensor, arena, want, keep, tag):
    """The env-rows `keep` (None: all) of the arena's outputs equal the host build's, by the sensor suite's same()."""
    names = getattr(want, '_fields', None)
    want = sx.members(want)
    names = names or [str(i) for i in range(len(want))]
    got = arena.out
    if keep is not None:
        got, want = [t[torch.from_numpy(keep).cuda()] for t in got], [w[keep] for w in want]
    if not SAME[sensor](got, want):
        rows = arena.rows()
        pytest.fail(f'{tag}: {differences(names, rows if keep is None else [r[keep] for r in rows], host_rows(want), None if keep is None else np.nonzero(keep)[0])}')


CASES = [(sensor, kind, shape) for sensor in sx.SENSORS for kind in sx.KINDS for shape in range(len(sx.SHAPES))]


@pytest.mark.parametrize('sensor,kind,shape', CASES)
def test_device_equals_the_host_build_at_scale(sensor, kind, shape):
    n, size = sx.SHAPES[shape]
    case = sx.expected(sensor, kind, n, size)
    want = sx.members(case.want)
    go = Launcher(sensor, case, *device(kind, n))
    try:
        once, again, masked = Arena(want), Arena(want), Arena(want)
        go(None, once.out)
        torch.cuda.synchronize()
        check(sensor, once, case.want, None, (sensor, kind, n, size, 'after a step'))
        assert once.guards_intact()
        for _ in range(REPEATS):
            go(None, again.out)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(once.out, again.out)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (sensor, kind, n, 'launch 21 differs from the first', differences([str(i)], [again.rows()[i]], [once.rows()[i]]))
        assert again.guards_intact()
        mask = np.arange(n) % 3 != 0
        go(torch.from_numpy(mask.astype(np.uint8)).cuda(), masked.out)
        torch.cuda.synchronize()
        check(sensor, masked, case.want, mask, (sensor, kind, n, size, 'masked'))
        assert all((r[~mask] == SENTINEL).all() for r in masked.rows()), (sensor, kind, n, 'a masked env was written')
        assert masked.guards_intact()
    finally:
        put(go.env, *sx.stepped(kind, n)[1:])


def test_three_sensors_on_three_streams_at_once():
    """Field, route and see of 4096 maze envs launched on three streams with nothing between the launches (plain launches, no graph):
    different kernels share compute units and LDS, and each result equals the host build.  (see: its second launch, on the memory the
    host build's first leaves.)"""
    kind, (n, size) = K.HRL_ANT_MAZE, sx.SHAPES[0]
    env, other, action = device(kind, n)
    cases = {s: sx.expected(s, kind, n, size) for s in ('field', 'route', 'see')}
    see = cases['see']
    seen = sx.see_first(see.cfg, see.items, see.aux, see.spec, see.extra['first']).seen
    try:
        launchers = {s: Launcher(s, c, env, other, action) for s, c in cases.items()}   # (each puts the same records)
        arenas = {s: Arena(sx.members(c.want)) for s, c in cases.items()}
        arenas['see'].out[1].copy_(torch.from_numpy(seen).cuda())
        streams = [torch.cuda.Stream() for _ in cases]
        other.step(action)
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for s, stream in zip(cases, streams):
            with torch.cuda.stream(stream):
                launchers[s].sensor_launch(None, arenas[s].out)
        torch.cuda.synchronize()
        for s, c in cases.items():
            check(s, arenas[s], c.want, None, (s, 'of three streams'))
            assert arenas[s].guards_intact()
    finally:
        put(env, *sx.stepped(kind, n)[1:])


# ------------------------------------------------------------------------------------------------ the four of scale_cases.LATER
FRONT = 4096   # the size of the env whose step runs in front of every launch of the four
WRAP = {'chase': Ch.Chase, 'cast': Ca.Cast, 'closest': Cl.Closest, 'dyn': Dy.Dynamics}


class LaterLauncher:
    """The launches of one case of the four: the records are put into the env, what the sensor is handed besides is on the device."""

    def __init__(self, sensor, case, env, front, action):
        self.sensor, self.case, self.env, self.front, self.action = sensor, case, env, front, action
        put(env, case.state, case.items, case.aux)
        self.dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in case.extra.items()}

    def sensor_launch(self, mask, out):
        s, env, spec, dev, o = self.sensor, self.env, self.case.spec, self.dev, WRAP[self.sensor](*out)
        if s == 'chase':
            env.chase(spec, mask=mask, out=o)
        elif s == 'cast':
            env.cast(dev['rays'], spec, mask=mask, out=o, ray_link=dev['ray_link'])
        elif s == 'closest':
            env.closest(spec, mask=mask, out=o)
        else:
            env.dynamics(spec, tau=dev['tau'], mask=mask, out=o)

    def __call__(self, mask, out):
        """A step of the 4096-env second env, then the sensor, on one stream with no synchronisation between them."""
        self.front.step(self.action)
        self.sensor_launch(mask, out)


def check_rows(sensor, arena, want, keep, tag):
    """The env-rows `keep` (None: all) of the arena's outputs equal the host build's, as bytes (dyn: a NaN for a NaN on its hostile envs,
    whose payload is the processor's own)."""
    got, rows = arena.rows(), host_rows(want)
    if sensor == 'dyn':
        got, rows = sx.nan_for_nan(got), sx.nan_for_nan(rows)
    if keep is not None:
        got, rows = [g[keep] for g in got], [r[keep] for r in rows]
    if not all(np.array_equal(g, r) for g, r in zip(got, rows)):
        pytest.fail(f'{tag}: {differences(want._fields, got, rows, None if keep is None else np.nonzero(keep)[0])}')


def env_of(kind, n):
    """(the env under test, whether it is this test's own to close): device(kind, n)'s first env at the cached sizes, else a fresh one
    after reset()."""
    if n in (FRONT, 1029):
        return device(kind, n)[0], False
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    env = BatchedEnv(_lib.default_config(kind, **sx.config_args(n)), 'cuda:0')
    env.reset()
    return env, True


@pytest.mark.parametrize('sensor,kind,n,size', sx.later_cases())
def test_the_later_four_equal_the_host_build_at_scale(sensor, kind, n, size):
    """The chase camera, the ray test, the closest points and the dynamics terms at the sizes they are run at (scale_cases.LATER_SHAPES,
    DYN_CASES), every output of every env against the host build, byte for byte:

        chase    4096 envs of 32 x 16 pixels | 1029 envs of 128 x 96 (12 chunks of 1024 pixels: the rgb staging runs 12 times per workgroup)
        cast     4096 envs of 129 rays (two full waves and one ray) | 1029 envs of 1024 rays (the maximum), the link frame
        closest  4096 | 1029 envs, every class
        dyn      4096 ant and 4096 point envs on the records | 16389 ant envs (1024 workgroups and a tail of 5 envs) on hand-made states

    The protocol is the seven sensors', unchanged: every output is a view into an allocation with 8 guard rows of sentinel bytes behind
    it; the case's records are put into the env; ONCE: a step, then the sensor on the same stream with nothing between them -- every
    output equals the host build, the guards are intact; AGAIN: 20 more step-and-sensor pairs into a second arena, which equals the
    first byte for byte (a missing barrier or an order-dependent minimum in LDS shows as launch 21 differing from launch 1); MASKED:
    under arange(n) % 3 != 0 the kept envs equal the host build and the others still hold the sentinel.

    The step in front is ALWAYS that of the second env of device(kind, 4096), also for the 1029- and 16389-env shapes: it is the launch
    that fills the machine (4096 workgroups of 256 threads) and leaves its LDS behind on every compute unit, so that a table slot one
    of these kernels reads without having written it holds the step's bytes and not a fresh process's zeros.

    Why these sizes -- what is resident at once on 256 compute units, from the kernels' resource figures (SRC=<file>
    tools/kernel_resources.sh; workgroups of 256 threads, one wave per SIMD):

        kernel          limiting resource             workgroups per compute unit   envs resident at once
        closest_kernel  123 VGPRs, 4 waves per SIMD   4                             1024
        chase_kernel    80 VGPRs, 6 waves per SIMD    6                             1536
        cast_kernel     55 VGPRs, 8 waves per SIMD    8                             2048
        dyn_kernel      58816 B of LDS (78 VGPRs)     2, of 16 envs each            8192

    At 4096 envs (dyn: 16389) workgroups wait for others to retire and start in the LDS a workgroup of the same launch left behind; at
    the 1029 envs of the per-sensor suites none does."""
    began = time.perf_counter()
    case = sx.expected(sensor, kind, n, size)
    want = case.want
    expected_s = time.perf_counter() - began
    _, front, action = device(kind, FRONT)
    env, own = env_of(kind, n)
    try:
        if own:   # the case's columns 29..31, items and aux are the oracle's after reset: what this env holds
            assert np.array_equal(env.state[:, 29:32].cpu().numpy().view(np.uint32), case.state[:, 29:32].view(np.uint32)) and np.array_equal(env.aux.cpu().numpy(), case.aux)
        go = LaterLauncher(sensor, case, env, front, action)
        once, again, masked = Arena(want), Arena(want), Arena(want)
        go(None, once.out)
        torch.cuda.synchronize()
        check_rows(sensor, once, want, None, (sensor, kind, n, size, 'after a step'))
        assert once.guards_intact()
        for _ in range(REPEATS):
            go(None, again.out)
        torch.cuda.synchronize()
        for i, (name, a, b) in enumerate(zip(want._fields, once.out, again.out)):
            if not torch.equal(a.view(torch.uint8), b.view(torch.uint8)):
                pytest.fail(f'{(sensor, kind, n, size)}: launch 21 differs from the first: {differences([name], [again.rows()[i]], [once.rows()[i]])}')
        assert again.guards_intact()
        mask = np.arange(n) % 3 != 0
        go(torch.from_numpy(mask.astype(np.uint8)).cuda(), masked.out)
        torch.cuda.synchronize()
        check_rows(sensor, masked, want, mask, (sensor, kind, n, size, 'masked'))
        assert all((r[~mask] == SENTINEL).all() for r in masked.rows()), (sensor, kind, n, 'a masked env was written')
        assert masked.guards_intact()
    finally:
        if own:
            env.close()
        else:
            put(env, *sx.stepped(kind, n)[1:])
    print(sensor, kind, n, size, f'expected side {expected_s:.2f} s, the whole case {time.perf_counter() - began:.2f} s')


def test_chase_cast_and_closest_on_three_streams_at_once():
    """Chase, cast and closest of 4096 gather envs launched on three streams with nothing between the launches (plain launches, no
    graph), after one step of the second env that all three streams wait on: different kernels share compute units and LDS, each result
    equals the host build and its guards are intact."""
    kind, n = K.HRL_ANT_GATHER, FRONT
    env, front, action = device(kind, n)
    cases = {s: sx.expected(s, kind, *sx.LATER_SHAPES[s][0]) for s in sx.LATER[:3]}
    try:
        launchers = {s: LaterLauncher(s, c, env, front, action) for s, c in cases.items()}   # (each puts the same records)
        arenas = {s: Arena(c.want) for s, c in cases.items()}
        streams = [torch.cuda.Stream() for _ in cases]
        front.step(action)
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for s, stream in zip(cases, streams):
            with torch.cuda.stream(stream):
                launchers[s].sensor_launch(None, arenas[s].out)
        torch.cuda.synchronize()
        for s, c in cases.items():
            check_rows(s, arenas[s], c.want, None, (s, 'of three streams'))
            assert arenas[s].guards_intact()
    finally:
        put(env, *sx.stepped(kind, n)[1:])
