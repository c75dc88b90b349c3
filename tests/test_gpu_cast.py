"""The batched ray test on the MI355X (csrc/cast_hip.hip, include/hrl_cast.h) against the host build of its specification
(tests/cast_host, csrc/cast_core.h), bit for bit in all four outputs, and its surface: None members, masks, streams and graph replay,
`out=`, ray patterns and ray_link, the gym classes' cast_batch(), and that the step does not notice it.  At most 37 envs per test, except
one of 1029."""
import ctypes as C

import numpy as np
import pytest
import torch

import cast_cases as hc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import cast_device as Ca
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5
COUNTS = (1, 63, 64, 65, 257, 1024)   # one lane live | the wave's edge | a second pass with one lane | the maximum


def host_of(got):
    out = []
    for x, dt in zip(got, hc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return hc.Cast(*out)


def same(a, b):
    """Every member equal, floats compared as uint32."""
    return hc.same(host_of(a), host_of(b))


def dev_links(links):
    return None if links is None else torch.from_numpy(links).cuda()


def both(env, st, it, aux, spec, rays, links):
    """(device answers, host-build answers) on the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    return env.cast(torch.from_numpy(rays).cuda(), spec, ray_link=dev_links(links)), hc.cast_host(env.cfg, st, host_items(env, it), aux, spec, rays, links)


@pytest.mark.parametrize('kind', hc.KINDS)
def test_device_answers_equal_the_host_build_bit_for_bit(kind):
    """Six kinds x the four frames x R = 1, 63, 64, 65, 257 and 1024 at N = 5, on the states of 30 steps and with the robots spread about
    the arena, the rays of cast_cases.sized_ray_set (lidar, foot rays, random segments, rays from inside solids and from under the
    ground, in the link frame with links 0..12); then the hostile states, a torso without a finite height and joints without a finite
    angle, null and non-finite rays and links out of range at R = 65.  fraction, point and normal (as uint32) and seg equal the host
    build of cast_core.h."""
    env, st, it, aux = stepped(kind)
    items = host_items(env, it)
    hits = set()
    try:
        for frame in hc.FRAMES:
            for R in COUNTS:
                spec = hc.spec_of(frame, R)
                for k, s in enumerate((st, hc.spread(env.cfg, st))):
                    rays, links = hc.sized_ray_set(env.cfg, s, items, frame, R, 1000 * int(kind) + 10 * R + k)
                    dev, host = both(env, s, it, aux, spec, rays, links)
                    assert tuple(dev.fraction.shape) == tuple(dev.seg.shape) == (N, R) and tuple(dev.point.shape) == tuple(dev.normal.shape) == (N, R, 3)
                    assert (dev.fraction.dtype, dev.seg.dtype, dev.point.dtype, dev.normal.dtype) == (torch.float32, torch.int32, torch.float32, torch.float32)
                    assert same(dev, host), (kind, frame, R, k)
                    hits |= set(np.unique(host.seg & 255).tolist())
            spec = hc.spec_of(frame, 65)
            rays, links = hc.sized_ray_set(env.cfg, st, items, frame, 65, 77)
            for s, i2, a, _, _, _, _, _ in hc.hostile(env.cfg, st, it, aux):
                dev, host = both(env, s, i2, a, spec, rays, links)
                assert same(dev, host), (kind, frame, 'hostile')
                assert all(not bool(dev.seg[e].any()) for e in range(N) if not np.isfinite(s[e, 0:2]).all())
            s = np.array(st)
            s[4, 2], s[3, 7], s[2, 10] = np.nan, np.nan, np.inf   # a torso without a finite height; a hip and an ankle without a finite angle
            r = np.array(rays)
            r[:, 5] = r[:, 5, 0:1]          # null
            r[:, 9, 4], r[:, 11, 0], r[:, 13, 2] = np.nan, np.inf, -np.inf
            wild = None if links is None else np.array(links)
            if wild is not None:
                wild[0::6], wild[1::6] = 13, -1
            dev, host = both(env, s, it, aux, spec, r, wild)
            assert same(dev, host) and not bool(dev.seg[4].any()) and not bool(dev.seg[:, [5, 9, 11, 13]].any())
        assert {Ca.HIT_NONE, Ca.HIT_GROUND, Ca.HIT_ROBOT} <= hits and (kind == K.HRL_ANT_FLAT or Ca.HIT_WALL in hits)
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_answers_equal_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5 and R = 65, its shard's records written into the device env: the four frames, on
    the shard and with the robots spread about the entry's arena; then the hostile states under world-frame rays.  All four outputs equal
    the host build of cast_core.h."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    items = host_items(env, it)
    kinds = set()
    for frame in hc.FRAMES:
        spec = hc.spec_of(frame, 65)
        for k, s in enumerate((st, hc.spread(cfg, st))):
            rays, links = hc.sized_ray_set(cfg, s, items, frame, 65, 300 + k)
            dev, host = both(env, s, it, aux, spec, rays, links)
            assert same(dev, host), (name, frame, k)
            kinds |= set(np.unique(host.seg & 255).tolist())
    assert Ca.HIT_GROUND in kinds and (Ca.HIT_ROBOT in kinds or cfg.env_kind == K.HRL_POINT_GATHER)   # (the lidar starts 0.3 m from O: inside the point bot's cube)
    spec = hc.spec_of(Ca.HRL_CAST_WORLD, 65)
    rays, _ = hc.sized_ray_set(cfg, st, items, Ca.HRL_CAST_WORLD, 65, 301)
    for s, i2, a, _, _, _, _, _ in scfg.hostile(name, hc.hostile):
        dev, host = both(env, s, i2, a, spec, rays, None)
        assert same(dev, host), (name, 'hostile')
    put(env, st, it, aux)


@pytest.mark.parametrize('n,R', [(1, 64), (37, 65), (1029, 16)])
def test_other_batch_sizes(n, R):
    """N = 1 and 37, and once 1029 at R = 16: the env index past one wave of workgroups and the size_t bases of the rays and the outputs.
    The device equals the host build on the env's own records after reset + 3 steps, in the link frame."""
    env = make_env(K.HRL_ANT_GATHER, n=n)
    env.reset()
    g = torch.Generator(device='cpu').manual_seed(n)
    for _ in range(3):
        env.step((torch.rand(n, env.act_dim, generator=g) * 2 - 1).cuda())
    torch.cuda.synchronize()
    st, it, aux = env.state.cpu().numpy(), env.items.cpu().numpy(), env.aux.cpu().numpy()
    base, links = hc.sized_ray_set(env.cfg, st[:1], host_items(env, it[:1]), Ca.HRL_CAST_LINK, R, n)
    rays = np.ascontiguousarray(np.broadcast_to(base, (n, R, 6))) + np.random.default_rng(n).uniform(-0.05, 0.05, (n, R, 6)).astype(np.float32)
    spec = hc.spec_of(Ca.HRL_CAST_LINK, R)
    dev = env.cast(torch.from_numpy(rays).cuda(), spec, ray_link=dev_links(links))
    host = hc.cast_host(env.cfg, st, host_items(env, it), aux, spec, rays, links)
    assert tuple(dev.point.shape) == (n, R, 3) and same(dev, host)
    assert bool(dev.seg[n - 1].any())
    env.close()


def arena_of(spec, n, fill=0x7B):
    """One allocation that holds guard | fraction | guard | seg | guard | point | guard | normal | guard, and the four views."""
    rays = n * spec.n_rays
    sizes = [4 * rays, 4 * rays, 12 * rays, 12 * rays]
    guard = 256
    arena = torch.full((sum(sizes) + 5 * guard,), fill, dtype=torch.uint8, device='cuda')
    views, spans, at = [], [], guard
    for size, shape, (_, dt) in zip(sizes, hc.shapes_of(n, spec), Ca.FIELDS):
        views.append(arena[at:at + size].view(dt).view(shape))
        spans.append((at, at + size))
        at += size + guard
    return arena, views, spans


def test_none_members_write_nothing_beyond_the_requested_tensors():
    """Each single output alone, pairs and all four: the bytes written equal the full call's slice, and not a byte beside them changes."""
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    for R in (65, 1024):
        spec = hc.spec_of(Ca.HRL_CAST_HEADING, R)
        rays, _ = hc.sized_ray_set(env.cfg, st, host_items(env, it), Ca.HRL_CAST_HEADING, R, 4)
        full = hc.cast_host(env.cfg, st, host_items(env, it), aux, spec, rays)
        drays = torch.from_numpy(rays).cuda()
        for want in (('fraction',), ('seg',), ('point',), ('normal',), ('fraction', 'seg'), ('seg', 'normal'), hc.NAMES):
            arena, views, spans = arena_of(spec, N)
            out = Ca.Cast(*(v if name in want else None for name, v in zip(hc.NAMES, views)))
            got = env.cast(drays, spec, out=out)
            assert got is out
            a = arena.cpu().numpy()
            keep = np.ones(len(a), bool)
            for name, (lo, hi), ref in zip(hc.NAMES, spans, full):
                if name in want:
                    keep[lo:hi] = False
                    assert np.array_equal(a[lo:hi], np.ascontiguousarray(ref).reshape(-1).view(np.uint8)), (R, want, name)
            assert (a[keep] == 0x7B).all(), (R, want)


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    pattern = Ca.lidar_rays(16, (-20.0, 0.0), 6.0, 0.3)
    rays = Ca.expand(pattern, 7, 'cuda')
    full = host_of(env.cast(rays))
    assert (full.seg != 0).any()
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = Ca.Cast(torch.full((7, 32), -3.0, device='cuda'), torch.full((7, 32), -7, dtype=torch.int32, device='cuda'), torch.full((7, 32, 3), -5.0, device='cuda'),
                  torch.full((7, 32, 3), -9.0, device='cuda'))
    got = env.cast(rays, mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        if mask[e]:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(hc.bits(o), hc.bits(full))), e
        else:
            assert (o.fraction[e] == -3).all() and (o.seg[e] == -7).all() and (o.point[e] == -5).all() and (o.normal[e] == -9).all()
    fresh = host_of(env.cast(rays, mask=mask))
    assert (fresh.seg[1] == 0).all() and (fresh.point[1] == 0).all() and np.array_equal(fresh.seg[0], full.seg[0])
    assert same(env.cast(pattern.cuda()), full)   # a pattern [R, 6] is expanded for the caller
    env.close()


def test_cast_follows_the_stream_and_replays_in_a_graph():
    """The single cast launch captured once (the first cast call ran before the capture, on a side stream) and replayed after each of three
    eager steps gives the answers of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    rays = Ca.expand(Ca.lidar_rays(16, (-30.0, -10.0, 0.0), 9.0), n, 'cuda')
    spec = hc.spec_of(Ca.HRL_CAST_HEADING, 48)
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    fresh_out = lambda: Ca.Cast(torch.zeros(n, 48, device='cuda'), torch.zeros(n, 48, dtype=torch.int32, device='cuda'), torch.zeros(n, 48, 3, device='cuda'), torch.zeros(n, 48, 3, device='cuda'))
    eager, eager_answers, eout = make_env(kind, n), [], fresh_out()
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager.cast(rays, spec, out=eout)
        eager_answers.append(Ca.Cast(*(x.clone() for x in eout)))
    env = make_env(kind, n)
    env.reset()
    out = fresh_out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the library's constants are uploaded here, outside the capture
        env.step(acts[0])
        env.cast(rays, spec, out=out)
        first = Ca.Cast(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_answers[0]) and bool(((first.seg & 255) == Ca.HIT_GROUND).any())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.cast(rays, spec, out=out)
    for r in range(1, 4):
        env.step(acts[r])
        g.replay()
        assert same(out, eager_answers[r]), r
    assert not same(eager_answers[1], eager_answers[3])   # the robots moved: the answers are not the same
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    R = 24
    spec = hc.spec_of(Ca.HRL_CAST_WORLD, R)
    hrays, _ = hc.sized_ray_set(env.cfg, st, host_items(env, it), Ca.HRL_CAST_WORLD, R, 8)
    rays = torch.from_numpy(hrays).cuda()
    out = Ca.Cast(torch.zeros(N, R, device='cuda'), torch.zeros(N, R, dtype=torch.int32, device='cuda'), torch.zeros(N, R, 3, device='cuda'), torch.zeros(N, R, 3, device='cuda'))
    ptrs = [x.data_ptr() for x in out]
    got = env.cast(rays, spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, hc.cast_host(env.cfg, st, it, aux, spec, hrays))
    alone = env.cast(rays, spec, out=Ca.Cast(fraction=torch.zeros(N, R, device='cuda')))
    assert isinstance(alone, Ca.Cast) and alone.seg is None and alone.point is None and alone.normal is None and torch.equal(alone.fraction, out.fraction)
    with pytest.raises(TypeError):
        env.cast(rays, spec, out=out._replace(fraction=out.fraction.double()))
    with pytest.raises(TypeError):
        env.cast(rays, spec, out=tuple(out))
    with pytest.raises(TypeError):
        env.cast(rays.double(), spec)
    with pytest.raises(ValueError):
        env.cast(rays, spec, out=out._replace(seg=torch.zeros(N, R + 1, dtype=torch.int32, device='cuda')))
    with pytest.raises(ValueError):
        env.cast(rays, spec, out=out._replace(seg=torch.zeros(N, R, dtype=torch.int32)))   # on the host
    with pytest.raises(ValueError):
        env.cast(rays, spec, out=out._replace(point=torch.zeros(N, R, 4, device='cuda')[..., :3]))   # not contiguous
    with pytest.raises(ValueError):
        env.cast(rays, spec, out=Ca.Cast())
    with pytest.raises(ValueError):
        env.cast(rays, spec, out=out._replace(normal=out.point))   # aliased
    with pytest.raises(ValueError):
        env.cast(rays[:, :R - 1].contiguous(), spec)   # fewer rays than the spec says
    with pytest.raises(ValueError):
        env.cast(rays.cpu(), spec)
    with pytest.raises(ValueError):
        env.cast(rays, hc.spec_of(Ca.HRL_CAST_LINK, R), ray_link=torch.zeros(R + 1, dtype=torch.int32, device='cuda'))
    with pytest.raises(TypeError):
        env.cast(rays, hc.spec_of(Ca.HRL_CAST_LINK, R), ray_link=torch.zeros(R, dtype=torch.int64, device='cuda'))
    bad = spec.copy()
    bad.n_rays = 1025
    with pytest.raises(ValueError):
        env.cast(rays, bad)


def test_cast_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntMazeBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    records = (b.state.cpu().numpy(), host_items(b, b.items.cpu().numpy()), b.aux.cpu().numpy())
    pattern = Ca.lidar_rays(16, (-45.0, -15.0, 0.0, 15.0), 8.0, 0.3)
    rays = Ca.expand(pattern, 5, 'cuda')
    spec = Ca.default_spec(b.cfg, 'link', 64)
    a, c = env.cast_batch(rays, spec), b.cast(rays, spec)
    assert isinstance(a, Ca.Cast) and tuple(a.point.shape) == (5, 64, 3) and same(a, c)
    assert same(a, hc.cast_host(b.cfg, *records, spec, rays.cpu().numpy()))
    d = env.cast_batch(rays)   # the default: the heading frame, every class
    assert tuple(d.fraction.shape) == (5, 64) and same(d, hc.cast_host(b.cfg, *records, Ca.default_spec(b.cfg, n_rays=64), rays.cpu().numpy()))
    kinds, index, faces = Ca.decode(d.seg)
    assert bool((kinds == Ca.HIT_GROUND).any()) and bool((kinds == Ca.HIT_ROBOT).any()) and int(faces.max()) <= Ca.FACE_GROUND
    hit = kinds != Ca.HIT_NONE
    assert bool((d.normal[hit].norm(dim=1) - 1).abs().max() <= 1e-6) and bool((d.normal[~hit] == 0).all()) and bool((d.fraction[~hit] == 1).all())
    ground = kinds == Ca.HIT_GROUND
    assert bool((d.point[ground][:, 2] - float(b.cfg.model.ground_z)).abs().max() <= 1e-4)
    feet, links = Ca.down_rays(0.6)
    f = env.cast_batch(feet.cuda(), Ca.default_spec(b.cfg, 'link', 4), ray_link=links.cuda())
    assert tuple(f.seg.shape) == (5, 4) and same(f, hc.cast_host(b.cfg, *records, Ca.default_spec(b.cfg, 'link', 4), Ca.expand(feet, 5).numpy(), links.numpy()))
    env.close()


def test_the_step_does_not_notice_the_ray_test():
    """20 steps of a 16-env gather shard with cast calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    rays = [Ca.expand(Ca.lidar_rays(az, el, 7.0, 0.2), n, 'cuda') for az, el in ((16, (-30.0, 0.0)), (65, (-10.0,)), (64, tuple(np.linspace(-60, 20, 16))))]
    feet, links = (x.cuda() for x in Ca.down_rays(0.5))
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.cast(rays[t % 3], Ca.default_spec(b.cfg, ('world', 'ego', 'heading', 'link')[t % 4], rays[t % 3].shape[1]))
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.cast(feet, Ca.default_spec(b.cfg, 'link', 4), ray_link=links) if t % 2 else b.cast(rays[(t + 1) % 3], mask=torch.arange(n) % 2)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('n_rays', 0), ('n_rays', 1025), ('frame', 4), ('classes', 0), ('classes', 128), ('reserved', 1), ('struct_size', 16), ('out', 'empty')])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = hc.spec_of(Ca.HRL_CAST_HEADING, 24)
    if field != 'out':
        setattr(spec, field, value)
    rays = torch.zeros(N, 24, 6, device='cuda')
    out = Ca.Cast(torch.full((N, 24), -3.0, device='cuda'), torch.full((N, 24), -7, dtype=torch.int32, device='cuda'), torch.full((N, 24, 3), -5.0, device='cuda'),
                  torch.full((N, 24, 3), -9.0, device='cuda'))
    handed = Ca.Cast() if field == 'out' else out
    with pytest.raises(HrlError) as e:
        Ca.cast(env.cfg, env._bufs_ref, spec, rays.data_ptr(), None, None, handed, None)
    hout = hc.Cast(np.zeros((N, 24), np.float32), np.zeros((N, 24), np.int32), np.zeros((N, 24, 3), np.float32), np.zeros((N, 24, 3), np.float32))
    hst, haux, hrays = np.array(st), np.array(aux), np.zeros((N, 24, 6), np.float32)
    b = K.make_buffers(hc.ptr(hst), None, hc.ptr(haux), None, None, None, None, None)
    o = Ca.hrl_cast_out(**({} if field == 'out' else {name: hc.ptr(x) for name, x in zip(hc.NAMES, hout)}))
    code = hc.lib().cast_host(C.byref(env.cfg), C.byref(b), C.byref(spec), hc.ptr(hrays), None, None, C.byref(o))
    assert code == K.HRL_ERR_BAD_ARG and hc.lib().cast_host_last_error().decode() in str(e.value)
    torch.cuda.synchronize()
    assert bool((out.fraction == -3).all()) and bool((out.seg == -7).all()) and bool((out.point == -5).all()) and bool((out.normal == -9).all())
