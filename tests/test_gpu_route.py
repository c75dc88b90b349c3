"""The batched routes on the MI355X (csrc/route_hip.hip, include/hrl_route.h) against the host build of their specification
(tests/route_host, csrc/route_core.h), bit for bit, and their surface: the chain of the device's own field, None members, masks, streams
and graph replay, `out=`, the gym classes' route_batch(), and that the step does not notice them.  At most 16 envs per test."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_cases as fc
import probe_cases as pc
import route_cases as rt
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import route_device as R
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5
ALL_SOURCES = F.ROBOT | F.FOOD | F.POISON | F.TARGET


def host_of(route):
    out = []
    for x, dt in zip(route, rt.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return rt.Route(*out)


def same(a, b):
    """cells and count compared as integers, waypoints and length as uint32."""
    return rt.same(host_of(a), host_of(b))


def dev_starts(starts):
    return None if starts is None else torch.from_numpy(starts).cuda()


def both(env, st, it, aux, spec, starts):
    """(device routes, host-build routes) of the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    return env.route(dev_starts(starts), spec), rt.route_host(env.cfg, st, host_items(env, it), aux, spec, starts)


@pytest.mark.parametrize('kind', rt.KINDS)
def test_device_routes_equal_the_host_build_bit_for_bit(kind):
    """Six kinds x three modes x 8 x 8 (64 cells: three waves idle in the field phases), 24 x 40, 64 x 8 and 64 x 64 at N = 5, on the states
    of 30 steps and with the robots spread about the arena; P = 1, 5 (a wave wraps to a second start) and 64, K = 2 and 32, the three
    frames and the source sets taken in turn, and starts = None once per grid; then the hostile states and hostile starts.  cells and
    count as integers, waypoints and length as uint32 equal the host build of route_core.h."""
    env, st, it, aux = stepped(kind)
    turn, routes = 0, 0
    try:
        for mode in rt.MODES:
            for size in rt.GPU_SIZES:
                for s in (st, fc.spread(env.cfg, st)):
                    p, frame, k = (1, 5, 64)[turn % 3], rt.FRAMES[(turn // 3) % 3], (2, 32)[(turn // 2) % 2]
                    fspec = fc.spec_of(size, mode, 0.25, fc.SOURCE_SETS[turn % len(fc.SOURCE_SETS)], kind=kind, centre=fc.WORLD_CENTRE)
                    turn += 1
                    spec = rt.spec_of(fspec, frame, p, k)
                    starts, _ = rt.draw_starts(env.cfg, s, fspec, frame, p, 11 * turn + kind)
                    dev, host = both(env, s, it, aux, spec, starts)
                    assert all(tuple(x.shape) == shape and x.dtype == dt for x, shape, (_, dt) in zip(dev, rt.shapes(N, spec), R.FIELDS))
                    assert same(dev, host), (kind, mode, size, p, frame, k, fspec.sources)
                    routes += int((host.count > 0).sum())
                spec = rt.spec_of(fspec, frame, 1, k)
                dev, host = both(env, s, it, aux, spec, None)
                assert same(dev, host), (kind, mode, size, 'robot')
        assert routes > 50
        for mode in rt.MODES:
            for size, frame in (((24, 40), R.HRL_PROBE_HEADING), ((64, 64), R.HRL_PROBE_WORLD)):
                fspec = fc.spec_of(size, mode, 0.4, ALL_SOURCES, kind=kind)
                spec = rt.spec_of(fspec, frame, 8, 7)
                starts, _ = rt.draw_starts(env.cfg, st, fspec, frame, 8, 5)
                for s, i2, a, _, _, _, _, blind in fc.hostile(env.cfg, st, it, aux):
                    dev, host = both(env, s, i2, a, spec, starts)
                    assert same(dev, host), (kind, mode, size, 'hostile')
                    assert all(bool((dev.count[e] == 0).all()) for e in blind)
                bad, blank, huge = pc.hostile_points(starts)
                dev, host = both(env, st, it, aux, spec, bad)
                assert same(dev, host), (kind, mode, size, 'hostile starts')
                assert bool((dev.count[:, list(blank) + list(huge)] == 0).all())
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_routes_equal_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: 16 x 16 grids in the three modes
    with 1 and 64 starts, K = 2 and 32, the frames and the source sets taken in turn, on the shard and with the robots spread about the
    entry's arena, starts = None once per mode, and the library's default spec; then the hostile states (on the entries of 64 items:
    NaN and inf in the last item).  cells and count as integers, waypoints and length as uint32 equal the host build of route_core.h."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    turn, routes = 0, 0
    for mode in rt.MODES:
        for p in (1, 64):
            for s in (st, fc.spread(cfg, st)):
                frame, k = rt.FRAMES[turn % 3], (2, 32)[(turn // 2) % 2]
                fspec = fc.spec_of((16, 16), mode, 0.25, fc.SOURCE_SETS[(4 * turn + 2) % len(fc.SOURCE_SETS)], kind=cfg, centre=fc.WORLD_CENTRE)
                turn += 1
                spec = rt.spec_of(fspec, frame, p, k)
                starts, _ = rt.draw_starts(cfg, s, fspec, frame, p, 11 * turn + scfg.seed_of(name))
                dev, host = both(env, s, it, aux, spec, starts)
                assert same(dev, host), (name, mode, p, frame, k, fspec.sources)
                routes += int((host.count > 0).sum())
        dev, host = both(env, s, it, aux, rt.spec_of(fspec, frame, 1, k), None)
        assert same(dev, host), (name, mode, 'robot')
    assert routes > 0
    put(env, st, it, aux)
    assert same(env.route(), rt.route_host(env.cfg, st, host_items(env, it), aux, R.default_spec(env.cfg), None)), (name, 'default')
    fspec = fc.spec_of((16, 16), F.HRL_VIEW_EGO_HEADING, 0.4, ALL_SOURCES, kind=cfg)
    spec = rt.spec_of(fspec, R.HRL_PROBE_HEADING, 8, 7)
    starts, _ = rt.draw_starts(cfg, st, fspec, R.HRL_PROBE_HEADING, 8, 5)
    for s, i2, a, _, _, _, _, _ in scfg.hostile(name, fc.hostile):
        dev, host = both(env, s, i2, a, spec, starts)
        assert same(dev, host), (name, 'hostile')


def test_the_routes_follow_the_chain_of_the_devices_own_field():
    """cells[..., 0] chained by env.field(field part).parent ends on the cell the route ends on, count is at most the chain's length + 1,
    and length lies between the straight line and the field's dist of the start cell."""
    for kind, sources in ((K.HRL_ANT_MAZE, F.TARGET), (K.HRL_ANT_GATHER, F.FOOD), (K.HRL_ANT_FLAGRUN, F.TARGET | F.ROBOT)):
        env, st, it, aux = stepped(kind)
        s = fc.spread(env.cfg, st)
        put(env, s, it, aux)
        try:
            walked = 0
            for mode in rt.MODES:
                fspec = fc.spec_of((64, 64), mode, 0.25, sources, blocking=F.WALL | F.BOX, half=10.0)
                spec = rt.spec_of(fspec, R.HRL_PROBE_WORLD, 16, 32)
                starts, _ = rt.draw_starts(env.cfg, s, fspec, R.HRL_PROBE_WORLD, 16, 3)
                got = host_of(env.route(dev_starts(starts), spec))
                field = fc.Field(*(x.cpu().numpy() for x in env.field(R.field_spec(spec))))
                size = fc.cell_size(fspec)
                for e in range(N):
                    for p in range(16):
                        n = int(got.count[e, p])
                        if n == 0:
                            continue
                        assert n <= 32
                        first, last = (divmod(int(got.cells[e, p, k]), 64) for k in (0, n - 1))
                        ch = rt.chain(field.parent[e], first)
                        assert ch[-1] == last and n <= len(ch) and field.parent[e][last] == F.SOURCE
                        straight = size * np.hypot(last[0] - first[0], last[1] - first[1])
                        assert straight - 1e-4 <= got.length[e, p] <= field.dist[e][first] + 1e-4   # (the two fp32 sums' tolerances, 5.4e-6 and 6.1e-5 m, together)
                        walked += 1
            assert walked >= 30, kind
        finally:
            put(env, st, it, aux)


def arena_of(spec, n, fill=0x7B):
    """One allocation that holds guard | waypoints | guard | count | guard | length | guard | cells | guard, and the four views."""
    sizes = [4 * int(np.prod(shape)) for shape in rt.shapes(n, spec)]
    guard = 256
    arena = torch.full((sum(sizes) + 5 * guard,), fill, dtype=torch.uint8, device='cuda')
    views, spans, at = [], [], guard
    for size, shape, (_, dt) in zip(sizes, rt.shapes(n, spec), R.FIELDS):
        views.append(arena[at:at + size].view(dt).view(shape))
        spans.append((at, at + size))
        at += size + guard
    return arena, views, spans


def test_none_members_write_nothing_beyond_the_requested_tensors():
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    fspec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.TARGET | F.ROBOT, kind=K.HRL_ANT_MAZE)
    spec = rt.spec_of(fspec, R.HRL_PROBE_WORLD, 5, 7)
    starts, _ = rt.draw_starts(env.cfg, st, fspec, R.HRL_PROBE_WORLD, 5, 2)
    full = rt.route_host(env.cfg, st, host_items(env, it), aux, spec, starts)
    for want in (('waypoints',), ('count',), ('length',), ('cells',), ('count', 'length'), rt.NAMES):
        arena, views, spans = arena_of(spec, N)
        out = R.Route(*(v if name in want else None for name, v in zip(rt.NAMES, views)))
        got = env.route(dev_starts(starts), spec, out=out)
        assert got is out
        a = arena.cpu().numpy()
        keep = np.ones(len(a), bool)
        for name, (lo, hi), ref, dt in zip(rt.NAMES, spans, rt.bits(full), rt.DTYPES):
            if name in want:
                keep[lo:hi] = False
                assert np.array_equal(a[lo:hi].view(np.uint32 if dt == np.float32 else dt).reshape(ref.shape), ref), (want, name)
        assert (a[keep] == 0x7B).all(), want


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    fspec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.4, F.TARGET | F.ROBOT, half=6.0)
    spec = rt.spec_of(fspec, R.HRL_PROBE_EGO, 5, 7)
    starts = torch.from_numpy(rt.draw_starts(env.cfg, env.state.cpu().numpy(), fspec, R.HRL_PROBE_EGO, 5, 4)[0]).cuda()
    full = host_of(env.route(starts, spec))
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = R.Route(*(torch.full(shape, -7, dtype=dt, device='cuda') for shape, (_, dt) in zip(rt.shapes(7, spec), R.FIELDS)))
    got = env.route(starts, spec, mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        for x, y in zip(rt.bits(o), rt.bits(full)):
            assert np.array_equal(x[e], y[e]) if mask[e] else all((m[e] == -7).all() for m in o)
    fresh = host_of(env.route(starts, spec, mask=mask))
    assert all((m[1] == 0).all() for m in fresh) and np.array_equal(fresh.cells[0], full.cells[0])
    env.close()


def test_route_follows_the_stream_and_replays_in_a_graph():
    """step + route captured once (the first route call ran before the capture, on a side stream) and replayed three times give the routes
    of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    fspec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, F.FOOD, half=5.0)
    spec = rt.spec_of(fspec, R.HRL_PROBE_HEADING, 5, 7)
    starts = (torch.rand(n, 5, 2, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6)) * 2 - 1) * 4
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    eager, eager_routes = make_env(kind, n), []
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager_routes.append(R.Route(*(x.clone() for x in eager.route(starts, spec))))
    env = make_env(kind, n)
    env.reset()
    static_a = acts[0].clone()
    out = R.Route(*(torch.zeros(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(rt.shapes(n, spec), R.FIELDS)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the route's constants are uploaded here, outside the capture
        env.step(static_a)
        env.route(starts, spec, out=out)
        first = R.Route(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_routes[0]) and bool((first.count > 0).any())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.route(starts, spec, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert same(out, eager_routes[r]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    fspec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.35, F.FOOD, kind=K.HRL_POINT_GATHER)
    spec = rt.spec_of(fspec, R.HRL_PROBE_WORLD, 5, 7)
    starts_h, _ = rt.draw_starts(env.cfg, st, fspec, R.HRL_PROBE_WORLD, 5, 9)
    starts = dev_starts(starts_h)
    out = R.Route(*(torch.zeros(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(rt.shapes(N, spec), R.FIELDS)))
    ptrs = [x.data_ptr() for x in out]
    got = env.route(starts, spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, rt.route_host(env.cfg, st, it, aux, spec, starts_h))
    with pytest.raises(TypeError):
        env.route(starts, spec, out=out._replace(length=out.length.double()))
    with pytest.raises(TypeError):
        env.route(starts, spec, out=out._replace(cells=out.cells.long()))
    with pytest.raises(TypeError):
        env.route(starts, spec, out=tuple(out))
    with pytest.raises(TypeError):
        env.route(starts.double(), spec)
    with pytest.raises(ValueError):
        env.route(starts, spec, out=out._replace(cells=torch.zeros(N, 7, 5, dtype=torch.int32, device='cuda')))   # P and K swapped
    with pytest.raises(ValueError):
        env.route(starts, spec, out=out._replace(count=torch.zeros(N, 5, dtype=torch.int32)))   # on the host
    with pytest.raises(ValueError):
        env.route(starts, spec, out=out._replace(length=torch.zeros(N, 10, device='cuda')[:, ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.route(starts, spec, out=R.Route())
    with pytest.raises(ValueError):
        env.route(starts[:, :3].contiguous(), spec)   # three starts, a spec of five
    with pytest.raises(ValueError):
        env.route(None, spec)   # the robot is one start
    with pytest.raises(ValueError):
        env.route(starts.cpu(), spec)
    bad = spec.copy()
    bad.max_waypoints = 40
    with pytest.raises(ValueError):
        env.route(starts, bad)


def test_route_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntGatherBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    records = (b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy())
    spec = R.default_spec(b.cfg, 'ego', 24, 40, 'ego', 5, 7)
    starts = (torch.rand(5, 5, 2, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)) * 2 - 1) * 3
    a, c = env.route_batch(starts, spec), b.route(starts, spec)
    assert isinstance(a, R.Route) and [tuple(x.shape) for x in a] == [(5, 5, 7, 2), (5, 5), (5, 5), (5, 5, 7)] and same(a, c)
    assert same(a, rt.route_host(b.cfg, *records, spec, starts.cpu().numpy()))
    d = env.route_batch()   # the default: from the robot to the nearest food on the 64 x 64 world grid, 16 waypoints
    assert [tuple(x.shape) for x in d] == [(5, 1, 16, 2), (5, 1), (5, 1), (5, 1, 16)]
    assert same(d, rt.route_host(b.cfg, *records, R.default_spec(b.cfg)))
    assert bool((d.count > 0).any())
    env.close()


def test_the_step_does_not_notice_the_routes():
    """20 steps of a 16-env gather shard with route calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = [rt.spec_of(fc.spec_of(size, m, 0.25, ALL_SOURCES, kind=kind), f, 5, 7) for size in ((24, 40), (64, 64)) for m, f in zip(rt.MODES, rt.FRAMES)]
    starts = (torch.rand(n, 5, 2, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8)) * 2 - 1) * 5
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.route(starts, specs[t % len(specs)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.route(None if t % 2 else starts, specs[(t + 1) % len(specs)] if t % 2 == 0 else None)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 12), ('height', 72), ('mode', 3), ('sources', 0), ('margin', 3.0), ('n_starts', 65), ('frame', 3), ('max_waypoints', 1),
                                         ('max_waypoints', 33), ('struct_size', 16), ('out', None)])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = rt.spec_of(fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.ROBOT, kind=K.HRL_ANT_FLAT), R.HRL_PROBE_WORLD, 5, 7)
    if field != 'out':
        setattr(spec, field, value)
    out = R.Route(*(torch.full((N, 64, 32, 2)[:len(shape)], -7, dtype=dt, device='cuda') for shape, (_, dt) in zip(rt.shapes(N, spec), R.FIELDS)))
    handed = R.Route() if field == 'out' else out
    starts = torch.zeros(N, 64, 2, device='cuda')
    with pytest.raises(HrlError) as e:
        R.route(env.cfg, env._bufs_ref, spec, starts, None, handed, None)
    hout = rt.Route(*((None if field == 'out' else np.zeros((N, 64, 32, 2)[:len(shape)], dt)) for shape, dt in zip(rt.shapes(N, spec), rt.DTYPES)))
    hst, haux, hstarts = np.array(st), np.array(aux), np.zeros((N, 64, 2), np.float32)
    b = K.make_buffers(rt.ptr(hst), None, rt.ptr(haux), None, None, None, None, None)
    o = R.hrl_route_out(**{name: rt.ptr(x) for name, x in zip(rt.NAMES, hout)})
    code = rt.lib().route_host(C.byref(env.cfg), C.byref(b), C.byref(spec), rt.ptr(hstarts), None, C.byref(o), rt.WALK)
    assert code == K.HRL_ERR_BAD_ARG and rt.lib().route_host_last_error().decode() in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((x == -7).all()) for x in out)
