"""The batched visibility map on the MI355X (csrc/see_hip.hip, include/hrl_see.h) against the host build of its specification
(tests/see_host, csrc/see_core.h), bit for bit, and its surface: the memory over real steps, None members, masks, streams and graph
replay, `out=`, the gym classes' see_batch(), and that the step does not notice it.  At most 16 envs per test."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_cases as fc
import see_cases as vc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import see_device as V
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5


def host_of(see):
    out = []
    for x, dt in zip(see, vc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return vc.See(*out)


def same(a, b):
    return vc.same(host_of(a), host_of(b))


def dirty_memory(n, spec, seed):
    """A memory with arbitrary bytes in a third of its cells."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (n, spec.height, spec.width)) * (rng.randint(0, 3, (n, spec.height, spec.width)) == 0)).astype(np.uint8)


def both(env, st, it, aux, spec, turn):
    """(device map, host-build map) of the records st / it / aux, written into the env's tensors first: all three outputs in the world
    mode (from a dirty memory, some envs cleared), `visible` alone in the ego modes."""
    put(env, st, it, aux)
    n = env.num_envs
    if spec.mode != V.HRL_VIEW_WORLD:
        return env.see(spec), vc.see_host(env.cfg, st, host_items(env, it), aux, spec)
    mem = dirty_memory(n, spec, turn)
    clear = None if turn % 3 == 0 else (np.arange(n) % 2 == turn % 2).astype(np.uint8) * 5
    out = V.See(torch.full((n, spec.height, spec.width), 9, dtype=torch.uint8, device='cuda'), torch.from_numpy(mem).cuda(), torch.full((n,), -7, dtype=torch.int32, device='cuda'))
    dev = env.see(spec, None if clear is None else torch.from_numpy(clear).cuda(), out=out)
    host = vc.See(np.full((n, spec.height, spec.width), 9, np.uint8), mem.copy(), np.full(n, -7, np.int32))
    vc.see_host(env.cfg, st, host_items(env, it), aux, spec, clear=clear, out=host)
    return dev, host


@pytest.mark.parametrize('kind', vc.KINDS)
def test_device_map_equals_the_host_build_bit_for_bit(kind):
    """Six kinds x three modes x 8 x 8 (64 cells: three waves idle), 24 x 40, 64 x 8 and 64 x 64 at N = 5, the three specs of
    see_cases.sweep_specs taken in turn, on the states of 30 steps and with the robots spread about the arena; then the hostile states.
    visible, seen and fresh equal the host build of see_core.h."""
    env, st, it, aux = stepped(kind)
    turn, lit = 0, 0
    try:
        for mode in vc.MODES:
            for size in vc.SIZES:
                for s in (st, vc.spread(env.cfg, st)):
                    spec = vc.sweep_specs(size, mode, kind)[turn % 3]
                    turn += 1
                    dev, host = both(env, s, it, aux, spec, turn)
                    assert tuple(dev.visible.shape) == (N, size[1], size[0]) and dev.visible.dtype == torch.uint8
                    assert same(dev, host), (kind, mode, size, turn)
                    lit += int(host.visible.sum())
        assert lit > 1000
        for mode in vc.MODES:
            for size in ((24, 40), (64, 64)):
                spec = vc.spec_of(size, mode, V.ALL, slack=0.1, kind=kind)
                for s, i2, a, _, _, _, _, blind in fc.hostile(env.cfg, st, it, aux):
                    turn += 1
                    dev, host = both(env, s, i2, a, spec, turn)
                    assert same(dev, host), (kind, mode, size, 'hostile')
                    assert all(not bool(dev.visible[e].any()) for e in blind)
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_map_equals_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: the three modes at 8 x 8 (one wave
    of cells) and 24 x 40, the three specs of see_cases.sweep_specs taken in turn, on the shard and with the robots spread about the
    entry's arena, and the library's default spec; then the hostile states (on the entries of 64 items: NaN and inf in the last item).
    visible, seen and fresh equal the host build of see_core.h."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    turn, lit = 0, 0
    for mode in vc.MODES:
        for size in ((8, 8), (24, 40)):
            for s in (st, vc.spread(cfg, st)):
                spec = vc.sweep_specs(size, mode, cfg)[turn % 3]
                turn += 1
                dev, host = both(env, s, it, aux, spec, turn)
                assert same(dev, host), (name, mode, size, turn)
                lit += int(host.visible.sum())
    assert lit > 100
    dev, host = both(env, st, it, aux, V.default_spec(env.cfg), 1)
    assert same(dev, host), (name, 'default')
    assert np.array_equal(env.see().visible.cpu().numpy(), host.visible), (name, 'default, none given')
    for mode in (V.HRL_VIEW_WORLD, V.HRL_VIEW_EGO_HEADING):
        spec = vc.spec_of((24, 40), mode, V.ALL, slack=0.1, kind=cfg)
        for s, i2, a, _, _, _, _, blind in scfg.hostile(name, fc.hostile):
            turn += 1
            dev, host = both(env, s, i2, a, spec, turn)
            assert same(dev, host), (name, mode, 'hostile')
            assert all(not bool(dev.visible[e].any()) for e in blind)


def test_memory_over_real_steps():
    """Six real steps of a 16-env maze shard whose episodes end after 4 steps, the step's `done` as `clear`: `seen` and `fresh` equal
    the host build fed the same states, step by step."""
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    n = 16
    env = BatchedEnv(_lib.default_config(K.HRL_ANT_MAZE, num_envs=n, seed=5, auto_reset=1, max_episode_steps=4), 'cuda:0')
    env.reset()
    spec = V.default_spec(env.cfg, 'world', 64, 64, fov_degrees=200, max_range=8.0)
    out = V.See(None, V.memory(n, spec, 'cuda'), torch.zeros(n, dtype=torch.int32, device='cuda'))
    host = vc.See(None, np.zeros((n, 64, 64), np.uint8), np.zeros(n, np.int32))
    acts = torch.rand(6, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)) * 2 - 1
    cleared = 0
    for t in range(6):
        _, _, done, _ = env.step(acts[t])
        env.see(spec, clear=done, out=out)
        st, aux, d = env.state.cpu().numpy(), env.aux.cpu().numpy(), done.cpu().numpy()
        vc.see_host(env.cfg, st, None, aux, spec, clear=d, out=host)
        assert same(out, host), t
        cleared += int(d.sum())
    assert cleared >= n and bool(out.seen.any())
    env.close()


def arena_of(spec, n, fill=0x7B):
    """One allocation that holds guard | visible | guard | seen | guard | fresh | guard, and the three views."""
    sizes = [n * spec.height * spec.width, n * spec.height * spec.width, 4 * n]
    guard = 256
    arena = torch.full((sum(sizes) + 4 * guard,), fill, dtype=torch.uint8, device='cuda')
    views, spans, at = [], [], guard
    for size, shape, (_, dt) in zip(sizes, vc.shapes_of(n, spec), V.FIELDS):
        views.append(arena[at:at + size].view(dt).view(shape))
        spans.append((at, at + size))
        at += size + guard
    return arena, views, spans


def test_none_members_write_nothing_beyond_the_requested_tensors():
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    spec = vc.spec_of((24, 40), V.HRL_VIEW_WORLD, V.WALL | V.BOX, slack=None, kind=K.HRL_ANT_MAZE)
    full = vc.See(np.zeros((N, 40, 24), np.uint8), np.full((N, 40, 24), 0x7B, np.uint8), np.zeros(N, np.int32))
    vc.see_host(env.cfg, st, host_items(env, it), aux, spec, out=full)
    assert (full.seen == 1).all() and (full.fresh == 0).all() and full.visible.any()   # (the memory found is the arena's fill: every cell counts as seen)
    for want in (('visible',), ('seen',), ('seen', 'fresh'), ('visible', 'seen'), vc.NAMES):
        arena, views, spans = arena_of(spec, N)
        out = V.See(*(v if name in want else None for name, v in zip(vc.NAMES, views)))
        got = env.see(spec, out=out)
        assert got is out
        a = arena.cpu().numpy()
        keep = np.ones(len(a), bool)
        for name, (lo, hi), ref, dt in zip(vc.NAMES, spans, full, vc.DTYPES):
            if name in want:
                keep[lo:hi] = False
                assert np.array_equal(a[lo:hi].view(dt).reshape(ref.shape), ref), (want, name)
        assert (a[keep] == 0x7B).all(), want


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    spec = vc.spec_of((24, 40), V.HRL_VIEW_WORLD, V.WALL | V.BOX, slack=None, kind=K.HRL_ANT_MAZE)
    full = host_of(env.see(spec, out=V.See(torch.zeros(7, 40, 24, dtype=torch.uint8, device='cuda'), V.memory(7, spec, 'cuda'), torch.zeros(7, dtype=torch.int32, device='cuda'))))
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = V.See(torch.full((7, 40, 24), 9, dtype=torch.uint8, device='cuda'), torch.full((7, 40, 24), 0, dtype=torch.uint8, device='cuda'), torch.full((7,), -7, dtype=torch.int32, device='cuda'))
    out.seen[1] = 0x33
    got = env.see(spec, clear=torch.ones(7, dtype=torch.uint8), mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        if mask[e]:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(o, full)), e
        else:
            assert (o.visible[e] == 9).all() and (o.seen[e] == (0x33 if e == 1 else 0)).all() and o.fresh[e] == -7
    fresh = host_of(env.see(spec, mask=mask))
    assert fresh.seen is None and fresh.fresh is None and (fresh.visible[1] == 0).all() and np.array_equal(fresh.visible[0], full.visible[0])
    env.close()


def test_see_follows_the_stream_and_replays_in_a_graph():
    """step + see captured once (the first see call ran before the capture, on a side stream) and replayed three times give the maps and
    the memory of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    spec = vc.spec_of((24, 40), V.HRL_VIEW_WORLD, V.ALL, fov_cos=0.3, max_range=9.0, slack=0.2, kind=kind)
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    fresh_out = lambda: V.See(torch.zeros(n, 40, 24, dtype=torch.uint8, device='cuda'), V.memory(n, spec, 'cuda'), torch.zeros(n, dtype=torch.int32, device='cuda'))
    eager, eager_maps, eout = make_env(kind, n), [], fresh_out()
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager.see(spec, clear=eager.done, out=eout)
        eager_maps.append(V.See(*(x.clone() for x in eout)))
    env = make_env(kind, n)
    env.reset()
    static_a = acts[0].clone()
    out = fresh_out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the map's constants are uploaded here, outside the capture
        env.step(static_a)
        done = env.done
        env.see(spec, clear=done, out=out)
        first = V.See(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_maps[0]) and bool(first.visible.any()) and bool((first.fresh > 0).any())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.see(spec, clear=done, out=out)   # (`done` is the env's own output tensor: the step of the graph rewrites it)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert same(out, eager_maps[r]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    spec = vc.spec_of((24, 40), V.HRL_VIEW_WORLD, V.ALL, slack=None, kind=K.HRL_POINT_GATHER)
    out = V.See(torch.zeros(N, 40, 24, dtype=torch.uint8, device='cuda'), V.memory(N, spec, 'cuda'), torch.zeros(N, dtype=torch.int32, device='cuda'))
    ptrs = [x.data_ptr() for x in out]
    got = env.see(spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    host = vc.See(np.zeros((N, 40, 24), np.uint8), np.zeros((N, 40, 24), np.uint8), np.zeros(N, np.int32))
    assert same(out, vc.see_host(env.cfg, st, it, aux, spec, out=host))
    alone = env.see(spec)
    assert isinstance(alone, V.See) and alone.seen is None and alone.fresh is None and torch.equal(alone.visible, out.visible)
    with pytest.raises(TypeError):
        env.see(spec, out=out._replace(visible=out.visible.float()))
    with pytest.raises(TypeError):
        env.see(spec, out=out._replace(fresh=out.fresh.long()))
    with pytest.raises(TypeError):
        env.see(spec, out=tuple(out))
    with pytest.raises(ValueError):
        env.see(spec, out=out._replace(seen=torch.zeros(N, 24, 40, dtype=torch.uint8, device='cuda')))   # W and H swapped
    with pytest.raises(ValueError):
        env.see(spec, out=out._replace(fresh=torch.zeros(N, dtype=torch.int32)))   # on the host
    with pytest.raises(ValueError):
        env.see(spec, out=out._replace(visible=torch.zeros(N, 40, 48, dtype=torch.uint8, device='cuda')[..., ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.see(spec, out=V.See())
    with pytest.raises(ValueError):
        env.see(spec, out=out._replace(seen=None))   # fresh without seen
    with pytest.raises(ValueError):
        env.see(spec, out=out._replace(seen=out.visible))   # aliased
    with pytest.raises(ValueError):
        env.see(vc.spec_of((24, 40), V.HRL_VIEW_EGO, kind=K.HRL_POINT_GATHER), out=out)   # a memory on an ego grid
    with pytest.raises(ValueError):
        env.see(spec, clear=torch.zeros(N + 1, dtype=torch.uint8), out=out)
    bad = spec.copy()
    bad.width = 72
    with pytest.raises(ValueError):
        env.see(bad)


def test_see_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntMazeBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    records = (b.state.cpu().numpy(), host_items(b, b.items.cpu().numpy()), b.aux.cpu().numpy())
    spec = V.default_spec(b.cfg, 'ego_heading', 24, 40, fov_degrees=120)
    a, c = env.see_batch(spec), b.see(spec)
    assert isinstance(a, V.See) and tuple(a.visible.shape) == (5, 40, 24) and same(a, c)
    assert same(a, vc.see_host(b.cfg, *records, spec))
    d = env.see_batch()   # the default: the 64 x 64 world grid, walls and the box occlude, all round, a slack of one cell
    assert tuple(d.visible.shape) == (5, 64, 64) and d.seen is None and d.fresh is None
    assert same(d, vc.see_host(b.cfg, *records, V.default_spec(b.cfg)))
    assert bool((d.visible == 1).any()) and bool((d.visible == 0).any())
    env.close()


def test_the_step_does_not_notice_the_map():
    """20 steps of a 16-env gather shard with see calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = [vc.sweep_specs(size, m, kind)[k] for k, size in enumerate(((24, 40), (64, 64), (8, 8))) for m in vc.MODES]
    wspec = vc.spec_of((64, 64), V.HRL_VIEW_WORLD, V.ALL, slack=None, kind=kind)
    out = V.See(None, V.memory(n, wspec, 'cuda'), torch.zeros(n, dtype=torch.int32, device='cuda'))
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.see(specs[t % len(specs)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.see(wspec, clear=b.done, out=out) if t % 2 else b.see()
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 12), ('height', 72), ('mode', 3), ('occluders', 32), ('max_range', 0.0), ('fov_cos', 1.5), ('slack', 3.0), ('struct_size', 16),
                                         ('out', 'empty'), ('out', 'seen in ego'), ('out', 'fresh alone'), ('out', 'aliased')])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = vc.spec_of((24, 40), V.HRL_VIEW_EGO if value == 'seen in ego' else V.HRL_VIEW_WORLD, kind=K.HRL_ANT_FLAT)
    if field != 'out':
        setattr(spec, field, value)
    out = V.See(torch.full((N, 64, 64), 0x7B, dtype=torch.uint8, device='cuda'), torch.full((N, 64, 64), 0x7B, dtype=torch.uint8, device='cuda'),
                torch.full((N,), -7, dtype=torch.int32, device='cuda'))
    pick = {'empty': lambda o: type(o)(None, None, None), 'seen in ego': lambda o: o, 'fresh alone': lambda o: o._replace(seen=None), 'aliased': lambda o: o._replace(seen=o.visible)}
    handed = pick[value](out) if field == 'out' else out
    with pytest.raises(HrlError) as e:
        V.see(env.cfg, env._bufs_ref, spec, None, None, handed, None)
    hout = vc.See(np.zeros((N, 64, 64), np.uint8), np.zeros((N, 64, 64), np.uint8), np.zeros(N, np.int32))
    hhanded = pick[value](hout) if field == 'out' else hout
    hst, haux = np.array(st), np.array(aux)
    b = K.make_buffers(vc.ptr(hst), None, vc.ptr(haux), None, None, None, None, None)
    o = V.hrl_see_out(**{name: vc.ptr(x) for name, x in zip(vc.NAMES, hhanded)})
    code = vc.lib().see_host(C.byref(env.cfg), C.byref(b), C.byref(spec), None, None, C.byref(o), None)
    assert code == K.HRL_ERR_BAD_ARG and vc.lib().see_host_last_error().decode() in str(e.value)
    torch.cuda.synchronize()
    assert bool((out.visible == 0x7B).all()) and bool((out.seen == 0x7B).all()) and bool((out.fresh == -7).all())
