"""The batched navigation field on the MI355X (csrc/field_hip.hip, include/hrl_field.h) against the host build of its specification
(tests/field_host, csrc/field_core.h), bit for bit, and its surface: source and blocking subsets, None members, masks, streams and graph
replay, `out=`, the gym classes' field_batch(), that the step does not notice it, and the helpers that turn `parent` into a walk.  At most
16 envs per test."""
import numpy as np
import pytest
import torch

import field_cases as fc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5
ALL_SOURCES = F.ROBOT | F.FOOD | F.POISON | F.TARGET


def host_of(field):
    out = []
    for x, dt in zip(field, fc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return fc.Field(*out)


def same(a, b):
    """dist compared as uint32, parent as bytes."""
    return fc.same(host_of(a), host_of(b))


def both(env, st, it, aux, spec):
    """(device field, host-build field) of the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    return env.field(spec), fc.field_host(env.cfg, st, host_items(env, it), aux, spec)


@pytest.mark.parametrize('kind', fc.KINDS)
def test_device_field_equals_the_host_build_bit_for_bit(kind):
    """Six kinds x three modes x margin 0 and 0.4 x 8 x 8 (64 cells: three waves idle), 24 x 40 (960 cells, no multiple of 256), 64 x 8 and
    8 x 64 (edge shapes) and 64 x 64 (the maximum) at N = 5, on the states of 30 steps, with the robots spread about the arena, on the
    hand-made poses (through set_state) and on the hostile states: dist as uint32 and parent as bytes equal the host build of
    field_core.h.  The source sets are taken in turn."""
    env, st, it, aux = stepped(kind)
    turn = 0
    try:
        for mode in fc.MODES:
            for margin in (0.0, 0.4):
                for size in fc.GPU_SIZES:
                    for s in (st, fc.spread(env.cfg, st)):
                        spec = fc.spec_of(size, mode, margin, fc.SOURCE_SETS[turn % len(fc.SOURCE_SETS)], kind=kind, centre=fc.WORLD_CENTRE)
                        turn += 1
                        dev, host = both(env, s, it, aux, spec)
                        assert all(tuple(x.shape) == (N, size[1], size[0]) and x.dtype == dt for x, (_, dt) in zip(dev, F.FIELDS))
                        assert same(dev, host), (kind, mode, margin, size, spec.sources)
        hm = fc.hand_made(env.cfg, st)
        put(env, st, it, aux)
        env.set_state(torch.from_numpy(hm[:, :15].copy()), torch.from_numpy(hm[:, 15:29].copy()))
        torch.cuda.synchronize()
        got = env.state.cpu().numpy()
        assert np.array_equal(got[:, :15], hm[:, :15])
        for mode in fc.MODES:
            for size in ((24, 40), (64, 64)):
                spec = fc.spec_of(size, mode, 0.4, ALL_SOURCES, kind=kind)
                assert same(env.field(spec), fc.field_host(env.cfg, got, host_items(env, it), aux, spec)), (kind, mode, size, 'hand-made')
        for mode in fc.MODES:
            for size in ((24, 40), (64, 64)):
                spec = fc.spec_of(size, mode, 0.4, ALL_SOURCES, kind=kind)
                for s, i2, a, _, _, _, _, blind in fc.hostile(env.cfg, st, it, aux):
                    dev, host = both(env, s, i2, a, spec)
                    assert same(dev, host), (kind, mode, size, 'hostile')
                    if mode != F.HRL_VIEW_WORLD:
                        assert all(bool((dev.parent[e] == F.BLOCKED).all()) for e in blind)
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_field_equals_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: the three modes at 8 x 8 (64 cells)
    and 24 x 40, margins 0 and 0.4 and the source sets taken in turn, on the shard and with the robots spread about the entry's arena,
    and the library's default spec; then the hostile states (on the entries of 64 items: NaN and inf in the last item): dist as uint32
    and parent as bytes equal the host build of field_core.h."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    turn = 0
    for mode in fc.MODES:
        for size in ((8, 8), (24, 40)):
            for s in (st, fc.spread(cfg, st)):
                spec = fc.spec_of(size, mode, (0.0, 0.4)[turn % 2], fc.SOURCE_SETS[(4 * turn + 2) % len(fc.SOURCE_SETS)], kind=cfg, centre=fc.WORLD_CENTRE)
                turn += 1
                dev, host = both(env, s, it, aux, spec)
                assert same(dev, host), (name, mode, size, spec.margin, spec.sources)
    put(env, st, it, aux)
    assert same(env.field(), fc.field_host(env.cfg, st, host_items(env, it), aux, F.default_spec(env.cfg))), (name, 'default')
    for mode in (F.HRL_VIEW_WORLD, F.HRL_VIEW_EGO_HEADING):
        spec = fc.spec_of((24, 40), mode, 0.4, ALL_SOURCES, kind=cfg)
        for s, i2, a, _, _, _, _, _ in scfg.hostile(name, fc.hostile):
            dev, host = both(env, s, i2, a, spec)
            assert same(dev, host), (name, mode, 'hostile')


def test_source_and_blocking_subsets_and_the_default_spec():
    for kind in fc.KINDS:
        env, st, it, aux = stepped(kind)
        put(env, st, it, aux)
        got = env.field()   # the kind's default: 64 x 64 world grid, WALL | BOX | POISON in the way, towards the kind's goal
        assert isinstance(got, F.Field) and all(tuple(x.shape) == (N, 64, 64) and x.device == env.device for x in got)
        assert same(got, fc.field_host(env.cfg, st, host_items(env, it), aux, F.default_spec(env.cfg))), kind
        assert bool((got.parent == F.SOURCE).any()) and bool(torch.isfinite(got.dist).any())
    env, st, it, aux = stepped(K.HRL_ANT_GATHER)
    for blocking in (F.WALL, F.FOOD, F.POISON, F.FOOD | F.POISON, F.WALL | F.TARGET | F.BOX, F.ALL):
        for sources in (F.ROBOT, F.FOOD, F.POISON | F.TARGET, ALL_SOURCES):
            spec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, sources, blocking=blocking, half=5.0)
            dev, host = both(env, st, it, aux, spec)
            assert same(dev, host), (blocking, sources)


def test_none_members_write_nothing_beyond_the_requested_tensor():
    """One allocation holds sentinel | dist | sentinel | parent | sentinel; a Field `out` with a None member fills the other tensor and
    leaves every other byte, the unrequested tensor's included."""
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    spec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.TARGET | F.ROBOT, kind=K.HRL_ANT_MAZE)
    full = fc.field_host(env.cfg, st, host_items(env, it), aux, spec)
    n = N * 40 * 24   # cells; the arena is laid out in bytes: 4n of dist between guards of n, n of parent
    for want in (('dist',), ('parent',), ('dist', 'parent')):
        arena = torch.full((8 * n,), 0x7B, dtype=torch.uint8, device='cuda')
        d, p = arena[n:5 * n].view(torch.float32).view(N, 40, 24), arena[6 * n:7 * n].view(N, 40, 24)
        out = F.Field(d if 'dist' in want else None, p if 'parent' in want else None)
        got = env.field(spec, out=out)
        assert got is out
        a = arena.cpu().numpy()
        assert (a[:n] == 0x7B).all() and (a[5 * n:6 * n] == 0x7B).all() and (a[7 * n:] == 0x7B).all()
        assert np.array_equal(a[n:5 * n].view(np.uint32).reshape(N, 40, 24), full.dist.view(np.uint32)) if 'dist' in want else (a[n:5 * n] == 0x7B).all(), want
        assert np.array_equal(a[6 * n:7 * n].reshape(N, 40, 24), full.parent) if 'parent' in want else (a[6 * n:7 * n] == 0x7B).all(), want


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    spec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.4, F.TARGET | F.ROBOT, half=6.0)
    full = host_of(env.field(spec))
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = F.Field(torch.full((7, 40, 24), -7.0, device='cuda'), torch.full((7, 40, 24), 77, dtype=torch.uint8, device='cuda'))
    got = env.field(spec, mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        if mask[e]:
            assert np.array_equal(o.dist[e].view(np.uint32), full.dist[e].view(np.uint32)) and np.array_equal(o.parent[e], full.parent[e])
        else:
            assert (o.dist[e] == -7).all() and (o.parent[e] == 77).all()
    fresh = host_of(env.field(spec, mask=mask))
    assert (fresh.dist[1] == 0).all() and (fresh.parent[1] == 0).all() and np.array_equal(fresh.parent[0], full.parent[0])
    env.close()


def test_field_follows_the_stream_and_replays_in_a_graph():
    """step + field captured once (the first field call ran before the capture, on a side stream) and replayed three times give the fields
    of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    spec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, F.FOOD, half=5.0)
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    eager, eager_fields = make_env(kind, n), []
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager_fields.append(F.Field(*(x.clone() for x in eager.field(spec))))
    env = make_env(kind, n)
    env.reset()
    static_a = acts[0].clone()
    out = F.Field(*(torch.zeros(n, 40, 24, dtype=dt, device='cuda') for _, dt in F.FIELDS))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the field's constants are uploaded here, outside the capture
        env.step(static_a)
        env.field(spec, out=out)
        first = F.Field(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_fields[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.field(spec, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert same(out, eager_fields[r]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    spec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.35, F.FOOD, kind=K.HRL_POINT_GATHER)
    out = F.Field(*(torch.zeros(N, 40, 24, dtype=dt, device='cuda') for _, dt in F.FIELDS))
    ptrs = [x.data_ptr() for x in out]
    got = env.field(spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, fc.field_host(env.cfg, st, it, aux, spec))
    with pytest.raises(TypeError):
        env.field(spec, out=out._replace(dist=out.dist.double()))
    with pytest.raises(TypeError):
        env.field(spec, out=out._replace(parent=out.parent.int()))
    with pytest.raises(TypeError):
        env.field(spec, out=tuple(out))
    with pytest.raises(ValueError):
        env.field(spec, out=out._replace(dist=torch.zeros(N, 24, 40, device='cuda')))   # width and height swapped
    with pytest.raises(ValueError):
        env.field(spec, out=out._replace(parent=torch.zeros(N, 40, 24, dtype=torch.uint8)))   # on the host
    with pytest.raises(ValueError):
        env.field(spec, out=out._replace(dist=torch.zeros(N, 40, 48, device='cuda')[:, :, ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.field(spec, out=F.Field())
    bad = spec.copy()
    bad.width = 72
    with pytest.raises(ValueError):
        env.field(bad)


def test_field_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntGatherBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    spec = F.default_spec(b.cfg, 'ego', 24, 40)
    a, c = env.field_batch(spec), b.field(spec)
    assert isinstance(a, F.Field) and all(tuple(x.shape) == (5, 40, 24) for x in a) and same(a, c)
    assert same(a, fc.field_host(b.cfg, b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy(), spec))
    assert same(env.field_batch(), fc.field_host(b.cfg, b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy(), F.default_spec(b.cfg)))
    env.close()


def test_the_step_does_not_notice_the_field():
    """20 steps of a 16-env gather shard with field calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = [fc.spec_of(size, m, 0.25, ALL_SOURCES, kind=kind) for size in ((24, 40), (64, 64)) for m in fc.MODES]
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.field(specs[t % len(specs)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.field(specs[(t + 1) % len(specs)])
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 0), ('width', 12), ('height', 72), ('mode', 3), ('blocking', 0), ('blocking', 32), ('sources', 0), ('sources', F.BOX),
                                         ('margin', float('nan')), ('margin', 3.0), ('half_extent', 0.0), ('half_extent', float('inf')), ('struct_size', 16), ('out', None)])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.ROBOT, kind=K.HRL_ANT_FLAT)
    if field != 'out':
        setattr(spec, field, value)
    out = F.Field(torch.full((N, 80, 80), -7.0, device='cuda'), torch.full((N, 80, 80), 77, dtype=torch.uint8, device='cuda'))
    handed = F.Field() if field == 'out' else out
    with pytest.raises(HrlError) as e:
        F.field(env.cfg, env._bufs_ref, spec, None, handed, None)
    hout = fc.Field(*((None if field == 'out' else np.zeros((N, 80, 80), dt)) for dt in fc.DTYPES))
    want = fc.field_host(env.cfg, st, None, aux, spec, out=hout, expect_ok=False)
    assert want[0] == K.HRL_ERR_BAD_ARG and want[1] in str(e.value)
    torch.cuda.synchronize()
    assert bool((out.dist == -7).all()) and bool((out.parent == 77).all())


def test_walking_down_the_field_reaches_a_source():
    """cell_index() and direction_vectors() agree with the kernel's geometry: a source sits in the cell cell_index() names for it, and
    following `parent` from the robot's cell reaches a source cell in dist / w1 steps or fewer (every step costs at least w1), each step
    moving the cell's centre along direction_vectors()[parent]."""
    for kind, sources in ((K.HRL_ANT_MAZE, F.TARGET), (K.HRL_ANT_GATHER, F.FOOD), (K.HRL_ANT_FLAGRUN, F.TARGET)):
        env, st, it, aux = stepped(kind)
        s = fc.spread(env.cfg, st)
        put(env, s, it, aux)
        try:
            for mode in fc.MODES:
                spec = fc.spec_of((64, 64), mode, 0.25, sources, blocking=F.WALL | F.BOX, half=10.0)
                got = env.field(spec)
                dist, parent = host_of(got)
                row, col = F.cell_index(spec, env.state, env.state[:, None, 0:2])
                dv = F.direction_vectors(spec, env.state).cpu().numpy()
                w1 = fc.cell_size(spec)
                walked = 0
                for e in range(N):
                    r, c = int(row[e, 0]), int(col[e, 0])
                    assert 0 <= r < 64 and 0 <= c < 64
                    pos = fc.centres(s[e], spec)[0]
                    assert np.abs(pos[r, c] - s[e, 0:2]).max() <= 0.5 * w1 * 1.42 + 1e-4   # the robot is in the cell cell_index() names
                    if not np.isfinite(dist[e, r, c]):
                        continue   # (a robot leaning on the box stands in a blocked cell)
                    steps = fc.follow(parent[e], r, c, 64 * 64)
                    assert 0 <= steps <= dist[e, r, c] / w1 + 1e-3, (kind, mode, e, steps, dist[e, r, c] / w1)
                    k = int(parent[e, r, c])
                    if k < 8:
                        nr, nc = r + F.DIRECTIONS[k][1], c + F.DIRECTIONS[k][0]
                        step = pos[nr, nc] - pos[r, c]
                        assert np.allclose(step / np.linalg.norm(step), dv[e, k], atol=1e-5) and dist[e, nr, nc] < dist[e, r, c]
                    walked += 1
                assert walked >= 3, (kind, mode)
        finally:
            put(env, st, it, aux)
