"""The batched first-person camera on the MI355X (csrc/camera_hip.hip, include/hrl_camera.h) against the host build of its specification
(tests/camera_host, csrc/camera_core.h), bit for bit, and its surface: None members, masks, streams and graph replay, `out=`, the gym
classes' camera_batch(), and that the step does not notice it.  At most 16 envs per test."""
import ctypes as C

import numpy as np
import pytest
import torch

import camera_cases as cc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import camera_device as Cm
from test_gpu_render import host_items, make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5


def host_of(cam):
    out = []
    for x, dt in zip(cam, cc.DTYPES):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        assert x is None or x.dtype == dt
        out.append(x)
    return cc.Camera(*out)


def same(a, b):
    """Every member equal, depth compared as uint32."""
    return cc.same(host_of(a), host_of(b))


def both(env, st, it, aux, spec):
    """(device images, host-build images) of the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    return env.camera(spec), cc.camera_host(env.cfg, st, host_items(env, it), aux, spec)


@pytest.mark.parametrize('kind', cc.KINDS)
def test_device_images_equal_the_host_build_bit_for_bit(kind):
    """Six kinds x both frames x both eye modes x 16 x 8 (128 pixels: two waves idle), 48 x 24 (1152: the last pass half full), 64 x 40
    and 128 x 128 (every rgb chunk boundary, the longest loop) at N = 5, the eye heights, class sets, ranges and fields of view of
    camera_cases.sweep taken in turn, on the states of 30 steps and with the robots spread about the arena; then the hostile states.
    depth (as uint32), seg and rgb equal the host build of camera_core.h."""
    env, st, it, aux = stepped(kind)
    hits = set()
    try:
        for spec in cc.sweep(kind):
            for s in (st, cc.spread(env.cfg, st)):
                dev, host = both(env, s, it, aux, spec)
                assert tuple(dev.depth.shape) == tuple(dev.seg.shape) == (N, spec.height, spec.width) and tuple(dev.rgb.shape) == (N, spec.height, spec.width, 3)
                assert (dev.depth.dtype, dev.seg.dtype, dev.rgb.dtype) == (torch.float32, torch.int32, torch.uint8)
                assert same(dev, host), (kind, spec.width, spec.height, spec.frame, spec.eye_mode, spec.classes)
                hits |= set(np.unique(host.seg & 255).tolist())
        assert {Cm.HIT_NONE, Cm.HIT_GROUND} <= hits and (kind == K.HRL_ANT_FLAT or Cm.HIT_WALL in hits)
        for frame in cc.FRAMES:
            for size, eye_mode in (((48, 24), Cm.HRL_EYE_TORSO), ((128, 128), Cm.HRL_EYE_GROUND)):
                spec = cc.spec_of(size, frame, eye_mode, 0.6)
                for s, i2, a, _, _, _, _, blind in cc.hostile(env.cfg, st, it, aux):
                    dev, host = both(env, s, i2, a, spec)
                    assert same(dev, host), (kind, frame, size, 'hostile')
                    assert all(not bool(dev.seg[e].any()) for e in blind)
                s = np.array(st)
                s[4, 2] = np.nan   # a torso without a finite height: blind from the torso, not from the ground
                dev, host = both(env, s, it, aux, spec)
                assert same(dev, host) and bool(dev.seg[4].any()) == (eye_mode == Cm.HRL_EYE_GROUND)
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_images_equal_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: 16 x 8 (128 pixels: two waves idle)
    and 64 x 48 in both frames and both eye modes, the eye heights, class sets, ranges and fields of view of camera_cases.sweep taken
    in turn, on the shard and with the robots spread about the entry's arena, and the library's default spec; then the hostile states
    (on the entries of 64 items: NaN and inf in the last item).  depth (as uint32), seg and rgb equal the host build of camera_core.h.
    On the entries of 64 items the device shows an item of index 48 or more, on maze-12 the posts 8 and 11."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    codes, turn = set(), 0
    for frame in cc.FRAMES:
        for eye_mode in cc.EYE_MODES:
            for size in ((16, 8), (64, 48)):
                spec = cc.spec_of(size, frame, eye_mode, cc.EYE_HEIGHTS[turn % 3], cc.CLASS_SETS[(turn // 3 + turn) % 3], (30.0, 7.0)[turn % 2], cc.TANS[(turn // 2) % 2])
                turn += 1
                for s in (st, cc.spread(cfg, st)):
                    dev, host = both(env, s, it, aux, spec)
                    assert same(dev, host), (name, size, frame, eye_mode, spec.classes)
                    codes |= set(np.unique(dev.seg.cpu().numpy() & 0xFFFF).tolist())
    put(env, st, it, aux)
    dev = env.camera()
    assert same(dev, cc.camera_host(env.cfg, st, host_items(env, it), aux, Cm.default_spec(env.cfg))), (name, 'default')
    codes |= set(np.unique(dev.seg.cpu().numpy() & 0xFFFF).tolist())
    assert {Cm.HIT_NONE, Cm.HIT_GROUND} <= {c & 255 for c in codes}
    spec = cc.spec_of((64, 48), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6)
    for s, i2, a, _, _, _, _, blind in scfg.hostile(name, cc.hostile):
        dev, host = both(env, s, i2, a, spec)
        assert same(dev, host), (name, 'hostile')
        assert all(not bool(dev.seg[e].any()) for e in blind)
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(sorted(codes))
    if name == 'maze-12':
        assert {Cm.HIT_TARGET | t << 8 for t in (8, 11)} <= codes


def arena_of(spec, n, fill=0x7B):
    """One allocation that holds guard | depth | guard | seg | guard | rgb | guard, and the three views."""
    px = n * spec.height * spec.width
    sizes = [4 * px, 4 * px, 3 * px]
    guard = 256
    arena = torch.full((sum(sizes) + 4 * guard,), fill, dtype=torch.uint8, device='cuda')
    views, spans, at = [], [], guard
    for size, shape, (_, dt) in zip(sizes, cc.shapes_of(n, spec), Cm.FIELDS):
        views.append(arena[at:at + size].view(dt).view(shape))
        spans.append((at, at + size))
        at += size + guard
    return arena, views, spans


def test_none_members_write_nothing_beyond_the_requested_tensors():
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    for size in ((48, 24), (128, 128)):   # one partial chunk of rgb | sixteen whole ones
        spec = cc.spec_of(size, Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6)
        full = cc.camera_host(env.cfg, st, host_items(env, it), aux, spec)
        for want in (('depth',), ('seg',), ('rgb',), ('depth', 'seg'), ('seg', 'rgb'), cc.NAMES):
            arena, views, spans = arena_of(spec, N)
            out = Cm.Camera(*(v if name in want else None for name, v in zip(cc.NAMES, views)))
            got = env.camera(spec, out=out)
            assert got is out
            a = arena.cpu().numpy()
            keep = np.ones(len(a), bool)
            for name, (lo, hi), ref, dt in zip(cc.NAMES, spans, full, cc.DTYPES):
                if name in want:
                    keep[lo:hi] = False
                    assert np.array_equal(a[lo:hi], np.ascontiguousarray(ref).reshape(-1).view(np.uint8)), (size, want, name)
            assert (a[keep] == 0x7B).all(), (size, want)


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6)
    full = host_of(env.camera(spec))
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = Cm.Camera(torch.full((7, 24, 48), -3.0, device='cuda'), torch.full((7, 24, 48), -7, dtype=torch.int32, device='cuda'), torch.full((7, 24, 48, 3), 9, dtype=torch.uint8, device='cuda'))
    got = env.camera(spec, mask=mask, out=out)
    assert got is out
    o = host_of(out)
    for e in range(7):
        if mask[e]:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(cc.bits(o), cc.bits(full))), e
        else:
            assert (o.depth[e] == -3).all() and (o.seg[e] == -7).all() and (o.rgb[e] == 9).all()
    fresh = host_of(env.camera(spec, mask=mask))
    assert (fresh.seg[1] == 0).all() and (fresh.rgb[1] == 0).all() and np.array_equal(fresh.seg[0], full.seg[0])
    env.close()


def test_camera_follows_the_stream_and_replays_in_a_graph():
    """step + camera captured once (the first camera call ran before the capture, on a side stream) and replayed three times give the
    images of the eager sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6, max_range=9.0)
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    fresh_out = lambda: Cm.Camera(torch.zeros(n, 24, 48, device='cuda'), torch.zeros(n, 24, 48, dtype=torch.int32, device='cuda'), torch.zeros(n, 24, 48, 3, dtype=torch.uint8, device='cuda'))
    eager, eager_images, eout = make_env(kind, n), [], fresh_out()
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager.camera(spec, out=eout)
        eager_images.append(Cm.Camera(*(x.clone() for x in eout)))
    env = make_env(kind, n)
    env.reset()
    static_a = acts[0].clone()
    out = fresh_out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the camera's constants are uploaded here, outside the capture
        env.step(static_a)
        env.camera(spec, out=out)
        first = Cm.Camera(*(x.clone() for x in out))
    torch.cuda.current_stream().wait_stream(side)
    assert same(first, eager_images[0]) and bool(first.seg.any())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.camera(spec, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert same(out, eager_images[r]), r
    assert not same(eager_images[1], eager_images[3])   # the robots moved: the images are not one picture
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    put(env, st, it, aux)
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_TORSO, 0.6)
    out = Cm.Camera(torch.zeros(N, 24, 48, device='cuda'), torch.zeros(N, 24, 48, dtype=torch.int32, device='cuda'), torch.zeros(N, 24, 48, 3, dtype=torch.uint8, device='cuda'))
    ptrs = [x.data_ptr() for x in out]
    got = env.camera(spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, cc.camera_host(env.cfg, st, it, aux, spec))
    alone = env.camera(spec, out=Cm.Camera(depth=torch.zeros(N, 24, 48, device='cuda')))
    assert isinstance(alone, Cm.Camera) and alone.seg is None and alone.rgb is None and torch.equal(alone.depth, out.depth)
    with pytest.raises(TypeError):
        env.camera(spec, out=out._replace(depth=out.depth.double()))
    with pytest.raises(TypeError):
        env.camera(spec, out=out._replace(rgb=out.rgb.float()))
    with pytest.raises(TypeError):
        env.camera(spec, out=tuple(out))
    with pytest.raises(ValueError):
        env.camera(spec, out=out._replace(seg=torch.zeros(N, 48, 24, dtype=torch.int32, device='cuda')))   # W and H swapped
    with pytest.raises(ValueError):
        env.camera(spec, out=out._replace(seg=torch.zeros(N, 24, 48, dtype=torch.int32)))   # on the host
    with pytest.raises(ValueError):
        env.camera(spec, out=out._replace(depth=torch.zeros(N, 24, 96, device='cuda')[..., ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.camera(spec, out=Cm.Camera())
    with pytest.raises(ValueError):
        env.camera(spec, out=out._replace(seg=out.depth.view(torch.int32)))   # aliased
    bad = spec.copy()
    bad.width = 144
    with pytest.raises(ValueError):
        env.camera(bad)


def test_camera_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntMazeBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    b = env._backend()
    records = (b.state.cpu().numpy(), host_items(b, b.items.cpu().numpy()), b.aux.cpu().numpy())
    spec = Cm.default_spec(b.cfg, 'world', 48, 24, hfov_degrees=70, eye='ground', eye_height=1.3)
    a, c = env.camera_batch(spec), b.camera(spec)
    assert isinstance(a, Cm.Camera) and tuple(a.rgb.shape) == (5, 24, 48, 3) and same(a, c)
    assert same(a, cc.camera_host(b.cfg, *records, spec))
    d = env.camera_batch()   # the default: 64 x 48 pixels, 90 degrees, from the torso, turning with the heading
    assert tuple(d.depth.shape) == (5, 48, 64) and same(d, cc.camera_host(b.cfg, *records, Cm.default_spec(b.cfg)))
    kinds, _, faces = Cm.decode(d.seg)
    assert bool((kinds == Cm.HIT_GROUND).any()) and bool((kinds == Cm.HIT_WALL).any()) and bool((kinds == Cm.HIT_NONE).any()) and int(faces.max()) <= Cm.FACE_GROUND
    env.close()


def test_the_step_does_not_notice_the_camera():
    """20 steps of a 16-env gather shard with camera calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = cc.sweep(kind)
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.camera(specs[t % len(specs)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.camera() if t % 2 else b.camera(specs[(t + 5) % len(specs)], mask=torch.arange(n) % 2)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 24), ('height', 132), ('frame', 2), ('eye_mode', 2), ('eye_height', 11.0), ('tan_half_h', 0.0), ('tan_half_v', 2e3), ('max_range', 0.0),
                                         ('classes', 0), ('classes', 32), ('struct_size', 16), ('out', 'empty')])
def test_bad_specs_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING)
    if field != 'out':
        setattr(spec, field, value)
    out = Cm.Camera(torch.full((N, 128, 128), -3.0, device='cuda'), torch.full((N, 128, 128), -7, dtype=torch.int32, device='cuda'), torch.full((N, 128, 128, 3), 0x7B, dtype=torch.uint8, device='cuda'))
    handed = Cm.Camera() if field == 'out' else out
    with pytest.raises(HrlError) as e:
        Cm.camera(env.cfg, env._bufs_ref, spec, None, handed, None)
    hout = cc.Camera(np.zeros((N, 128, 128), np.float32), np.zeros((N, 128, 128), np.int32), np.zeros((N, 128, 128, 3), np.uint8))
    hst, haux = np.array(st), np.array(aux)
    b = K.make_buffers(cc.ptr(hst), None, cc.ptr(haux), None, None, None, None, None)
    o = Cm.hrl_camera_out(**({} if field == 'out' else {name: cc.ptr(x) for name, x in zip(cc.NAMES, hout)}))
    code = cc.lib().camera_host(C.byref(env.cfg), C.byref(b), C.byref(spec), None, C.byref(o))
    assert code == K.HRL_ERR_BAD_ARG and cc.lib().camera_host_last_error().decode() in str(e.value)
    torch.cuda.synchronize()
    assert bool((out.depth == -3).all()) and bool((out.seg == -7).all()) and bool((out.rgb == 0x7B).all())
