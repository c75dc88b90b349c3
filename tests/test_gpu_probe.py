"""The batched point probes on the MI355X (csrc/probe_hip.hip, include/hrl_probe.h) against the host build of their specification
(tests/probe_host, csrc/probe_core.h), bit for bit, and their surface: class subsets, None fields, masks, streams and graph replay, `out=`,
the gym classes' probe_batch(), and that the step does not notice them.  At most 16 envs per test."""
import numpy as np
import pytest
import torch

import probe_cases as pc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import probe_device as P
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5


def bits(probe):
    out = []
    for x, dt in zip(probe, pc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x.dtype == dt
        out.append(x.view(np.uint32))
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def dev_points(pts):
    return torch.from_numpy(np.ascontiguousarray(pts)).cuda()


def both(env, st, it, aux, spec, pts):
    """(device probes, host-build probes) of the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    return env.probe(dev_points(pts), spec), pc.probe_host(env.cfg, st, host_items(env, it), aux, spec, pts)


@pytest.mark.parametrize('kind', pc.KINDS)
def test_device_probes_equal_the_host_build_bit_for_bit(kind):
    """Six kinds x three frames x 1, 37, 64, 65 and 512 points x margin 0 and 0.4 at N = 5, on the states of 30 steps, with the robots
    spread about the arena, on the hand-made poses (through set_state) and on the hostile states and points: every float as uint32 and
    every int32 equal the host build of probe_core.h."""
    env, st, it, aux = stepped(kind)
    try:
        for spec in pc.all_specs():
            for s in (st, pc.spread(env.cfg, st)):
                pts = pc.draw_points(env.cfg, s, spec.frame, spec.n_points, pc.seed_of(env.cfg, spec))
                dev, host = both(env, s, it, aux, spec, pts)
                assert all(tuple(x.shape) == (N, spec.n_points) and x.dtype == dt for x, (_, dt) in zip(dev, P.FIELDS))
                assert same(dev, host), (kind, spec.n_points, spec.frame, spec.margin)
        hm = pc.hand_made(env.cfg, st)
        put(env, st, it, aux)
        env.set_state(torch.from_numpy(hm[:, :15].copy()), torch.from_numpy(hm[:, 15:29].copy()))
        torch.cuda.synchronize()
        got = env.state.cpu().numpy()
        assert np.array_equal(got[:, :15], hm[:, :15])
        for frame in pc.FRAMES:
            for n in (65, 512):
                spec = pc.spec_of(n, frame, 0.4)
                pts = pc.draw_points(env.cfg, got, frame, n, 11)
                assert same(env.probe(dev_points(pts), spec), pc.probe_host(env.cfg, got, host_items(env, it), aux, spec, pts)), (kind, frame, n, 'hand-made')
        for frame in pc.FRAMES:
            spec = pc.spec_of(65, frame, 0.4)
            pts = pc.hostile_points(pc.draw_points(env.cfg, st, frame, 65, 5))[0]
            for s, i2, a, _, _, _, _, _ in pc.hostile(env.cfg, st, it, aux):
                dev, host = both(env, s, i2, a, spec, pts)
                assert same(dev, host), (kind, frame, 'hostile')
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_probes_equal_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: 1 point (a block of 64 threads, which
    stages a record of 96 or 128 floats in two trips), 65 and 512 points in the three frames, margins 0 and 0.4 in turn, and the
    library's default spec on the shard and with the robots spread about the entry's arena; 1 and 65 points on the hostile states (on
    the entries of 64 items: NaN and inf in the last item) and hostile points: every float as uint32 and every int32 equal the host
    build of probe_core.h.  On the entries of 64 items the device names an item of index 48 or more, on maze-12 the targets 8 and 11."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    codes, turn = set(), 0
    for n in (1, 65, 512):
        for frame in pc.FRAMES:
            for s in (st, pc.spread(cfg, st)):
                spec = pc.spec_of(n, frame, pc.MARGINS[turn % 2])
                turn += 1
                pts = pc.draw_points(cfg, s, frame, n, pc.seed_of(cfg, spec))
                dev, host = both(env, s, it, aux, spec, pts)
                assert same(dev, host), (name, n, frame, spec.margin)
                codes |= set(np.unique(dev.nearest.cpu().numpy()).tolist()) | set(np.unique(dev.blocker.cpu().numpy()).tolist())
    pts = pc.draw_points(cfg, st, P.HRL_PROBE_WORLD, 64, 13)
    put(env, st, it, aux)
    assert same(env.probe(dev_points(pts)), pc.probe_host(env.cfg, st, host_items(env, it), aux, P.default_spec(env.cfg, 'world', 64), pts)), (name, 'default')
    for n in (1, 65):
        spec = pc.spec_of(n, P.HRL_PROBE_HEADING, 0.4)
        pts = pc.hostile_points(pc.draw_points(cfg, st, spec.frame, 65, 5))[0][:, 65 - n:].copy()
        for s, i2, a, _, _, _, _, _ in scfg.hostile(name, pc.hostile):
            dev, host = both(env, s, i2, a, spec, pts)
            assert same(dev, host), (name, n, 'hostile')
    pts = pc.hostile_points(pc.draw_points(cfg, st, P.HRL_PROBE_EGO, 65, 5))[0]
    dev, host = both(env, st, it, aux, pc.spec_of(65, P.HRL_PROBE_EGO, 0.0), pts)
    assert same(dev, host), (name, 'hostile points')
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(sorted(codes))
    if name == 'maze-12':
        assert {P.HIT_TARGET | t << 8 for t in (8, 11)} <= codes


def test_class_subsets_and_the_default_spec():
    env, st, it, aux = stepped(K.HRL_ANT_GATHER)
    pts = pc.draw_points(env.cfg, st, P.HRL_PROBE_HEADING, 37, 12)
    for classes in (P.WALL, P.FOOD, P.POISON, P.FOOD | P.POISON, P.WALL | P.TARGET | P.BOX):
        spec = pc.spec_of(37, P.HRL_PROBE_HEADING, 0.25, classes)
        dev, host = both(env, st, it, aux, spec, pts)
        assert same(dev, host), classes
    pts = pc.draw_points(env.cfg, st, P.HRL_PROBE_WORLD, 64, 13)
    got = env.probe(dev_points(pts))   # world points, all classes, margin = the torso's radius
    assert isinstance(got, P.Probe) and all(tuple(x.shape) == (N, 64) and x.device == env.device for x in got)
    assert same(got, pc.probe_host(env.cfg, st, it, aux, P.default_spec(env.cfg), pts))
    cls, _ = P.decode(got.nearest)
    assert int(cls.max()) <= P.HIT_TARGET and bool((cls != 0).all()) and bool((got.via <= 1).all())
    got = env.probe(dev_points(pts[:, :37].copy()))   # the default spec follows the points
    assert same(got, pc.probe_host(env.cfg, st, it, aux, P.default_spec(env.cfg, 'world', 37), pts[:, :37]))


def test_none_fields_write_nothing_beyond_the_requested_tensors():
    """One allocation holds sentinel | clearance | sentinel | ... | via | sentinel; a Probe `out` with None fields fills the requested
    tensors and leaves every other byte, the unrequested tensors' included."""
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    spec = pc.spec_of(65, P.HRL_PROBE_WORLD, 0.4)
    pts = pc.draw_points(env.cfg, st, spec.frame, 65, 14)
    full = bits(pc.probe_host(env.cfg, st, host_items(env, it), aux, spec, pts))
    n = N * 65
    for want in (('path',), ('via', 'nearest'), ('clearance', 'sight', 'blocker'), ('blocker',)):
        arena = torch.full((13 * n,), 0x7B7B7B7B, dtype=torch.int32, device='cuda')
        views = [arena[(2 * i + 1) * n:(2 * i + 2) * n].view(N, 65) for i in range(6)]
        out = P.Probe(*((v.view(dt) if name in want else None) for v, (name, dt) in zip(views, P.FIELDS)))
        got = env.probe(dev_points(pts), spec, out=out)
        assert got is out
        a = arena.cpu().numpy().view(np.uint32)
        for i, (name, _) in enumerate(P.FIELDS):
            seg = a[(2 * i + 1) * n:(2 * i + 2) * n].reshape(N, 65)
            assert np.array_equal(seg, full[i]) if name in want else (seg == 0x7B7B7B7B).all(), (want, name)
            assert (a[2 * i * n:(2 * i + 1) * n] == 0x7B7B7B7B).all()
        assert (a[12 * n:] == 0x7B7B7B7B).all()


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    spec = pc.spec_of(65, P.HRL_PROBE_HEADING, 0.4)
    pts = dev_points(pc.draw_points(env.cfg, env.state.cpu().numpy(), spec.frame, 65, 15))
    full = bits(env.probe(pts, spec))
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = P.Probe(*(torch.full((7, 65), -7, dtype=dt, device='cuda') for _, dt in P.FIELDS))
    got = env.probe(pts, spec, mask=mask, out=out)
    assert got is out
    for x, y, o in zip(bits(out), full, out):
        for e in range(7):
            assert np.array_equal(x[e], y[e]) if mask[e] else bool((o[e] == -7).all())
    fresh = bits(env.probe(pts, spec, mask=mask))
    assert all((x[1] == 0).all() and np.array_equal(x[0], y[0]) for x, y in zip(fresh, full))
    env.close()


def test_probe_follows_the_stream_and_replays_in_a_graph():
    """step + probe captured once (the first probe call ran before the capture, on a side stream) and replayed three times give the probes
    of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    spec = pc.spec_of(65, P.HRL_PROBE_HEADING, 0.25)
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    eager, eager_probes = make_env(kind, n), []
    eager.reset()
    pts = dev_points(pc.draw_points(eager.cfg, eager.state.cpu().numpy(), P.HRL_PROBE_EGO, 65, 16))
    for r in range(4):
        eager.step(acts[r])
        eager_probes.append(P.Probe(*(x.clone() for x in eager.probe(pts, spec))))
    env = make_env(kind, n)
    env.reset()
    static_a = acts[0].clone()
    out = P.Probe(*(torch.zeros(n, 65, dtype=dt, device='cuda') for _, dt in P.FIELDS))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the probe's constants are uploaded here, outside the capture
        env.step(static_a)
        env.probe(pts, spec, out=out)
        first = P.Probe(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_probes[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.probe(pts, spec, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert same(out, eager_probes[r]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_and_points_are_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    spec = pc.spec_of(37, P.HRL_PROBE_WORLD, 0.35)
    hp = pc.draw_points(env.cfg, st, spec.frame, 37, 17)
    pts = dev_points(hp)
    out = P.Probe(*(torch.zeros(N, 37, dtype=dt, device='cuda') for _, dt in P.FIELDS))
    ptrs = [x.data_ptr() for x in out]
    got = env.probe(pts, spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, pc.probe_host(env.cfg, st, it, aux, spec, hp))
    with pytest.raises(TypeError):
        env.probe(pts, spec, out=out._replace(nearest=out.nearest.float()))
    with pytest.raises(TypeError):
        env.probe(pts, spec, out=out._replace(path=out.path.int()))
    with pytest.raises(TypeError):
        env.probe(pts, spec, out=tuple(out))
    with pytest.raises(ValueError):
        env.probe(pts, spec, out=out._replace(sight=torch.zeros(N, 64, device='cuda')))
    with pytest.raises(ValueError):
        env.probe(pts, spec, out=out._replace(via=torch.zeros(N, 37, dtype=torch.int32)))
    with pytest.raises(ValueError):
        env.probe(pts, spec, out=P.Probe())
    with pytest.raises(TypeError):
        env.probe(pts.double(), spec)
    with pytest.raises(ValueError):
        env.probe(pts[:, :, :1], spec)
    with pytest.raises(ValueError):
        env.probe(pts.transpose(0, 1), spec)
    with pytest.raises(ValueError):
        env.probe(pts.cpu(), spec)
    with pytest.raises(ValueError):
        env.probe(pts[:, :36].contiguous(), spec)   # spec.n_points is 37
    with pytest.raises(ValueError):
        env.probe(torch.zeros(N, 513, 2, device='cuda'))


def test_probe_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntGatherBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    spec = P.default_spec(b.cfg, 'ego', 37)
    hp = pc.draw_points(b.cfg, b.state.cpu().numpy(), P.HRL_PROBE_EGO, 37, 18)
    a, c = env.probe_batch(dev_points(hp), spec), b.probe(dev_points(hp), spec)
    assert isinstance(a, P.Probe) and all(tuple(x.shape) == (5, 37) for x in a) and same(a, c)
    assert same(a, pc.probe_host(b.cfg, b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy(), spec, hp))
    env.close()


def test_the_step_does_not_notice_the_probe():
    """20 steps of a 16-env gather shard with probe calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = [pc.spec_of(p, f, 0.25) for p in (37, 512) for f in pc.FRAMES]
    pts = {p: dev_points(pc.draw_points(b.cfg, b.state.cpu().numpy(), P.HRL_PROBE_WORLD, p, 19)) for p in (37, 512)}
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        s = specs[t % len(specs)]
        b.probe(pts[s.n_points], s)
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        s = specs[(t + 1) % len(specs)]
        b.probe(pts[s.n_points], s)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('n_points', 0), ('n_points', 513), ('frame', 3), ('classes', 0), ('classes', 32), ('margin', float('nan')), ('margin', -1.0),
                                         ('margin', 3.0), ('struct_size', 16), ('out', None)])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = pc.spec_of(37, P.HRL_PROBE_WORLD, 0.4)
    if field != 'out':
        setattr(spec, field, value)
    pts = torch.zeros(N, 600, 2, device='cuda')
    out = P.Probe(*(torch.full((N, 600), -7, dtype=dt, device='cuda') for _, dt in P.FIELDS))
    handed = P.Probe() if field == 'out' else out
    with pytest.raises(HrlError) as e:
        P.probe(env.cfg, env._bufs_ref, spec, pts, None, handed, None)
    hout = pc.Probe(*((None if field == 'out' else np.zeros((N, 600), dt)) for dt in pc.DTYPES))
    want = pc.probe_host(env.cfg, st, None, aux, spec, np.zeros((N, 600, 2), np.float32), out=hout, expect_ok=False)
    assert want[0] == K.HRL_ERR_BAD_ARG and want[1] in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((x == -7).all()) for x in out)
