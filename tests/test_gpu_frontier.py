"""The batched frontier map on the MI355X (csrc/frontier_hip.hip, include/hrl_frontier.h) against the host build of its specification
(tests/frontier_host, csrc/frontier_core.h), bit for bit, and its surface: the chain step -> see -> frontier over real steps, None
members, masks, graph replay, `out=`, the gym classes' frontier_batch(), and that the step does not notice it.  At most 16 envs per
test."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_cases as fc
import frontier_cases as xc
import see_cases as vc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import frontier_device as X
from hrl_pybullet_envs_amd import see_device as V
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5


def host_of(fr):
    out = []
    for x, dt in zip(fr, xc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return xc.Frontier(*out)


def same(a, b):
    return xc.same(host_of(a), host_of(b))


def both(env, st, it, aux, spec, seen):
    """(device map, host-build map) of the records st / it / aux, written into the env's tensors first, and the memory `seen`."""
    put(env, st, it, aux)
    mem = torch.from_numpy(seen).cuda()
    dev = env.frontier(mem, spec)
    assert np.array_equal(mem.cpu().numpy(), seen)   # only read
    return dev, xc.frontier_host(env.cfg, st, host_items(env, it), aux, spec, seen)


@pytest.mark.parametrize('kind', xc.KINDS)
def test_device_map_equals_the_host_build_bit_for_bit(kind):
    """Six kinds x 8 x 8 (one wave of cells), 24 x 40 (960, no multiple of 256), 64 x 8, 8 x 64 and 64 x 64 x both meanings of `unknown`
    at N = 5, the 31 source sets and the margins taken in turn, on the states of 30 steps and with the robots spread about the arena,
    with real memories made by the host visibility map and with arbitrary bytes; then the hostile states.  All seven outputs equal the
    host build of frontier_core.h."""
    env, st, it, aux = stepped(kind)
    turn, edges, reached = 0, 0, 0
    try:
        for size in xc.GPU_SIZES:
            for unknown in xc.UNKNOWNS:
                for s in (st, xc.spread(env.cfg, st)):
                    for which in ('real', 'dirty'):
                        spec = xc.spec_of(size, xc.MARGINS[turn % 3], xc.SOURCE_SETS[(7 * turn) % 31], unknown, kind=kind)
                        turn += 1
                        seen = xc.memory(which, env.cfg, np.array(s), host_items(env, it), aux, spec, turn)
                        dev, host = both(env, s, it, aux, spec, seen)
                        assert tuple(dev.edge.shape) == (N, size[1], size[0]) and tuple(dev.goal.shape) == (N, 2)
                        assert same(dev, host), (kind, size, unknown, which, turn)
                        edges += int(host.count.sum())
                        reached += int((host.cell >= 0).sum())
        assert edges > 1000 and reached > 20
        for size in ((24, 40), (64, 64)):
            for unknown in xc.UNKNOWNS:
                spec = xc.spec_of(size, 0.25, X.EDGE | xc.CLASS_SOURCES, unknown, kind=kind)
                for s, i2, a, _, _, _, _, blind in xc.hostile(env.cfg, st, it, aux):
                    turn += 1
                    seen = xc.memory('dirty', env.cfg, st, None, aux, spec, turn)
                    dev, host = both(env, s, i2, a, spec, seen)
                    assert same(dev, host), (kind, size, unknown, 'hostile')
                    assert all(int(dev.cell[e]) == -1 for e in blind)
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_map_equals_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: 8 x 8 (one wave of cells) and
    24 x 40 x both meanings of `unknown`, the source sets and the margins taken in turn, on the shard and with the robots spread about
    the entry's arena, with real and dirty memories, and the library's default spec; then the hostile states (on the entries of 64
    items: NaN and inf in the last item).  All seven outputs equal the host build of frontier_core.h."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    turn, edges = 0, 0
    for size in ((8, 8), (24, 40)):
        for unknown in xc.UNKNOWNS:
            for s, which in ((st, 'real'), (xc.spread(cfg, st), 'dirty')):
                spec = xc.spec_of(size, xc.MARGINS[turn % 3], xc.SOURCE_SETS[(7 * turn) % 31], unknown, kind=cfg)
                turn += 1
                seen = xc.memory(which, env.cfg, np.array(s), host_items(env, it), aux, spec, turn)
                dev, host = both(env, s, it, aux, spec, seen)
                assert same(dev, host), (name, size, unknown, which, turn)
                edges += int(host.count.sum())
    assert edges > 100
    spec = X.default_spec(env.cfg)
    dev, host = both(env, st, it, aux, spec, xc.memory('real', env.cfg, np.array(st), host_items(env, it), aux, spec, 2))
    assert same(dev, host), (name, 'default')
    spec = xc.spec_of((24, 40), 0.25, X.EDGE | xc.CLASS_SOURCES, X.OPTIMISTIC, kind=cfg)
    seen = xc.memory('dirty', env.cfg, np.array(st), None, aux, spec, 3)
    for s, i2, a, _, _, _, _, blind in scfg.hostile(name, xc.hostile):
        dev, host = both(env, s, i2, a, spec, seen)
        assert same(dev, host), (name, 'hostile')
        assert all(int(dev.cell[e]) == -1 for e in blind)


def test_the_chain_over_real_steps():
    """step, see(clear=done), frontier(seen) for six steps of a 16-env maze shard whose episodes end after 4 steps: the memory and the
    map equal the host chain fed the same states, step by step."""
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    n = 16
    env = BatchedEnv(_lib.default_config(K.HRL_ANT_MAZE, num_envs=n, seed=5, auto_reset=1, max_episode_steps=4), 'cuda:0')
    env.reset()
    sspec = V.default_spec(env.cfg, 'world', 32, 32, fov_degrees=200, max_range=6.0)
    spec = X.spec_like(env.cfg, sspec, sources=X.EDGE | X.TARGET)
    mem = V.See(None, V.memory(n, sspec, 'cuda'), None)
    hmem = vc.See(None, np.zeros((n, 32, 32), np.uint8), None)
    acts = torch.rand(6, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)) * 2 - 1
    cleared = 0
    for t in range(6):
        _, _, done, _ = env.step(acts[t])
        env.see(sspec, clear=done, out=mem)
        got = env.frontier(mem.seen, spec)
        st, aux, d = env.state.cpu().numpy(), env.aux.cpu().numpy(), done.cpu().numpy()
        vc.see_host(env.cfg, st, None, aux, sspec, clear=d, out=hmem)
        assert np.array_equal(mem.seen.cpu().numpy(), hmem.seen), t
        assert same(got, xc.frontier_host(env.cfg, st, None, aux, spec, hmem.seen)), t
        cleared += int(d.sum())
    assert cleared >= n and bool((got.count > 0).all()) and bool(torch.isfinite(got.length).any())
    env.close()


def arena_of(spec, n, fill=0x7B):
    """One allocation that holds guard | edge | guard | dist | ... | cell | guard, and the seven views."""
    sizes = [int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in zip(xc.shapes_of(n, spec), xc.DTYPES)]
    guard = 256
    arena = torch.full((sum(sizes) + (len(sizes) + 1) * guard,), fill, dtype=torch.uint8, device='cuda')
    views, spans, at = [], [], guard
    for size, shape, (_, dt) in zip(sizes, xc.shapes_of(n, spec), X.FIELDS):
        views.append(arena[at:at + size].view(dt).view(shape))
        spans.append((at, at + size))
        at += size + guard
    return arena, views, spans


def test_none_members_write_nothing_beyond_the_requested_tensors():
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    spec = xc.spec_of((24, 40), 0.25, X.EDGE | X.TARGET, kind=K.HRL_ANT_MAZE)
    seen = xc.memory('real', env.cfg, np.array(st), host_items(env, it), aux, spec, 1)
    full = xc.frontier_host(env.cfg, st, host_items(env, it), aux, spec, seen)
    assert full.edge.any() and np.isfinite(full.length).any()
    mem = torch.from_numpy(seen).cuda()
    for want in (('edge',), ('dist',), ('parent',), ('count',), ('length',), ('goal', 'cell'), ('edge', 'parent', 'count'), ('dist', 'goal'), xc.NAMES):
        arena, views, spans = arena_of(spec, N)
        out = X.Frontier(*(v if name in want else None for name, v in zip(xc.NAMES, views)))
        got = env.frontier(mem, spec, out=out)
        assert got is out
        a = arena.cpu().numpy()
        keep = np.ones(len(a), bool)
        for name, (lo, hi), ref, dt in zip(xc.NAMES, spans, full, xc.DTYPES):
            if name in want:
                keep[lo:hi] = False
                assert np.array_equal(a[lo:hi], ref.reshape(-1).view(np.uint8)), (want, name)
        assert (a[keep] == 0x7B).all(), want
        assert np.array_equal(mem.cpu().numpy(), seen)   # byte-identical afterwards


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    spec = xc.spec_of((24, 40), 0.25, X.EDGE, kind=K.HRL_ANT_MAZE)
    st, aux = env.state.cpu().numpy(), env.aux.cpu().numpy()
    seen = xc.memory('real', env.cfg, st, None, aux, spec, 2)
    mem = torch.from_numpy(seen).cuda()
    full = host_of(env.frontier(mem, spec))
    assert full.count.min() > 0
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    fills = (9, -7.0, 9, -7, -7.0, -7.0, -7)
    out = X.Frontier(*(torch.full(shape, fill, dtype=dt, device='cuda') for shape, fill, (_, dt) in zip(xc.shapes_of(7, spec), fills, X.FIELDS)))
    got = env.frontier(mem, spec, mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        for x, y, fill in zip(o, full, fills):
            assert np.array_equal(xc.bits(x[e]), xc.bits(y[e])) if mask[e] else (x[e] == fill).all(), e
    fresh = host_of(env.frontier(mem, spec, mask=mask))
    assert (fresh.edge[1] == 0).all() and fresh.count[1] == 0 and np.array_equal(fresh.edge[0], full.edge[0])
    env.close()


def test_step_see_frontier_replay_in_a_graph():
    """step + see + frontier captured once on one stream (the first calls ran before the capture, on that side stream) and replayed three
    times give the memory and the maps of the eager sequence."""
    kind, n = K.HRL_ANT_GATHER, 16
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1

    def outs(env):
        sspec = V.default_spec(env.cfg, 'world', 24, 40, fov_degrees=150, max_range=5.0)
        spec = X.spec_like(env.cfg, sspec, sources=X.EDGE | X.FOOD)
        mem = V.See(None, V.memory(n, sspec, 'cuda'), None)
        out = X.Frontier(*(torch.zeros(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(xc.shapes_of(n, spec), X.FIELDS)))
        return sspec, spec, mem, out

    eager, eager_maps = make_env(kind, n), []
    eager.reset()
    sspec, spec, emem, eout = outs(eager)
    for r in range(4):
        eager.step(acts[r])
        eager.see(sspec, clear=eager.done, out=emem)
        eager.frontier(emem.seen, spec, out=eout)
        eager_maps.append((emem.seen.clone(), X.Frontier(*(x.clone() for x in eout))))
    env = make_env(kind, n)
    env.reset()
    sspec, spec, mem, out = outs(env)
    static_a = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the libraries' constants are uploaded here, outside the capture
        env.step(static_a)
        done = env.done
        env.see(sspec, clear=done, out=mem)
        env.frontier(mem.seen, spec, out=out)
        first = X.Frontier(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_maps[0][1]) and bool((first.count > 0).any())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.see(sspec, clear=done, out=mem)   # (`done` is the env's own output tensor: the step of the graph rewrites it)
        env.frontier(mem.seen, spec, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert torch.equal(mem.seen, eager_maps[r][0]) and same(out, eager_maps[r][1]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    spec = xc.spec_of((24, 40), 0.35, X.EDGE | X.FOOD, kind=K.HRL_POINT_GATHER)
    seen = xc.memory('real', env.cfg, np.array(st), it, aux, spec, 3)
    mem = torch.from_numpy(seen).cuda()
    out = X.Frontier(*(torch.zeros(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(xc.shapes_of(N, spec), X.FIELDS)))
    ptrs = [x.data_ptr() for x in out]
    got = env.frontier(mem, spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, xc.frontier_host(env.cfg, st, it, aux, spec, seen))
    alone = env.frontier(mem, spec)
    assert isinstance(alone, X.Frontier) and same(alone, out)
    with pytest.raises(TypeError):
        env.frontier(mem, spec, out=out._replace(edge=out.edge.float()))
    with pytest.raises(TypeError):
        env.frontier(mem, spec, out=out._replace(cell=out.cell.long()))
    with pytest.raises(TypeError):
        env.frontier(mem, spec, out=tuple(out))
    with pytest.raises(TypeError):
        env.frontier(mem.float(), spec)
    with pytest.raises(TypeError):
        env.frontier(None, spec)
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=out._replace(parent=torch.zeros(N, 24, 40, dtype=torch.uint8, device='cuda')))   # W and H swapped
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=out._replace(length=torch.zeros(N)))   # on the host
    with pytest.raises(ValueError):
        env.frontier(mem.cpu(), spec)
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=out._replace(dist=torch.zeros(N, 40, 48, device='cuda')[..., ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=X.Frontier())
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=out._replace(edge=mem))   # aliased
    with pytest.raises(ValueError):
        env.frontier(mem, spec, out=out._replace(parent=mem))
    with pytest.raises(ValueError):
        env.frontier(mem[:, :32], spec)   # another grid
    bad = spec.copy()
    bad.width = 72
    with pytest.raises(ValueError):
        env.frontier(mem, bad)


def test_frontier_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntMazeBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    records = (b.state.cpu().numpy(), host_items(b, b.items.cpu().numpy()), b.aux.cpu().numpy())
    mem = V.See(None, V.memory(5, V.default_spec(b.cfg), 'cuda'), None)
    env.see_batch(out=mem)   # the default memory: the 64 x 64 world grid ...
    d, c = env.frontier_batch(mem.seen), b.frontier(mem.seen)   # ... lines up with the default map
    assert isinstance(d, X.Frontier) and tuple(d.edge.shape) == (5, 64, 64) and same(d, c)
    assert same(d, xc.frontier_host(b.cfg, *records, X.default_spec(b.cfg), mem.seen.cpu().numpy()))
    assert bool((d.count > 0).all()) and bool(torch.isfinite(d.length).all()) and bool((d.cell >= 0).all())
    seen = mem.seen.bool()
    assert bool((d.edge.bool() <= seen).all())   # an edge cell has been seen (the robot's own cell has: it is visible to itself)
    spec = X.default_spec(b.cfg, 24, 40, sources=X.TARGET, unknown='optimistic')
    small = V.See(None, V.memory(5, V.default_spec(b.cfg, 'world', 24, 40), 'cuda'), None)
    env.see_batch(V.default_spec(b.cfg, 'world', 24, 40), out=small)
    a = env.frontier_batch(small.seen, spec)
    assert same(a, b.frontier(small.seen, spec)) and same(a, xc.frontier_host(b.cfg, *records, spec, small.seen.cpu().numpy()))
    env.close()


def test_the_step_does_not_notice_the_map():
    """20 steps of a 16-env gather shard with see and frontier calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    sspec = V.default_spec(b.cfg, 'world', 64, 64, max_range=4.0)
    mem = V.See(None, V.memory(n, sspec, 'cuda'), None)
    specs = [X.spec_like(b.cfg, sspec, sources=s, unknown=u) for s, u in ((X.EDGE, 'known'), (X.FOOD | X.EDGE, 'optimistic'), (X.ROBOT, 'known'))]
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.frontier(mem.seen, specs[t % 3])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.see(sspec, clear=b.done, out=mem)
        b.frontier(mem.seen)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 12), ('height', 72), ('blocking', 0), ('sources', 128), ('sources', 0), ('margin', 3.0), ('unknown', 2), ('struct_size', 16),
                                         ('out', 'empty'), ('out', 'no seen'), ('out', 'seen is edge'), ('out', 'seen is parent')])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = xc.spec_of((24, 40), 0.25, kind=K.HRL_ANT_FLAT)
    if field != 'out':
        setattr(spec, field, value)
    fills = (0x7B, -7.0, 0x7B, -7, -7.0, -7.0, -7)
    out = X.Frontier(*(torch.full(shape, fill, dtype=dt, device='cuda') for shape, fill, (_, dt) in zip(xc.shapes_of(N, xc.spec_of((64, 64), 0.25, kind=K.HRL_ANT_FLAT)), fills, X.FIELDS)))
    mem = torch.full((N, 64, 64), 0x7B, dtype=torch.uint8, device='cuda')
    pick_out = lambda o: type(o)(*(None,) * 7) if value == 'empty' else o
    pick_mem = lambda o, m: {'no seen': None, 'seen is edge': o.edge, 'seen is parent': o.parent}.get(value, m)
    handed, seen = (pick_out(out), pick_mem(out, mem)) if field == 'out' else (out, mem)
    with pytest.raises(HrlError) as e:
        X.frontier(env.cfg, env._bufs_ref, spec, None if seen is None else seen.data_ptr(), None, handed, None)
    hout = xc.Frontier(*(np.zeros(tuple(x.shape), dt) for x, dt in zip(out, xc.DTYPES)))
    hmem = np.zeros((N, 64, 64), np.uint8)
    hhanded, hseen = (pick_out(hout), pick_mem(hout, hmem)) if field == 'out' else (hout, hmem)
    code, why = xc.frontier_host(env.cfg, np.array(st), None, np.array(aux), spec, hseen, out=hhanded, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and why in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((x == fill).all()) for x, fill in zip(out, fills)) and bool((mem == 0x7B).all())
