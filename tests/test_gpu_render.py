"""The batched renderer on the MI355X (csrc/render_hip.hip, include/hrl_render.h) against the host build of its specification
(tests/render_host, csrc/render_core.h), byte for byte, and its surface: masks, streams and graph replay, `out=`, the gym classes'
render_batch(), and that the step does not notice it.  At most 16 envs per test; images 32 x 32 and 48 x 32, one 256 x 256."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import render_cases as rc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import render_device as R

pytestmark = pytest.mark.gpu
N = 5


def make_env(kind, n=N, seed=21, **over):
    """`over`: constructor overrides of the kind's default config (tests/sensor_configs.py)."""
    from hrl_pybullet_envs_amd import _lib
    from hrl_pybullet_envs_amd.vec_env import BatchedEnv
    return BatchedEnv(_lib.default_config(kind, num_envs=n, seed=seed + kind, auto_reset=1, **over), 'cuda:0')


@functools.lru_cache(None)
def stepped(kind):
    """An env of 5 after reset + 30 random-action steps, and host copies of its records (computed once; the tests that write into the env's
    tensors put these back)."""
    env = make_env(kind)
    env.reset()
    g = torch.Generator(device='cpu').manual_seed(kind)
    for _ in range(30):
        env.step((torch.rand(N, env.act_dim, generator=g) * 2 - 1).cuda())
    torch.cuda.synchronize()
    st, it, aux = env.state.cpu().numpy(), env.items.cpu().numpy(), env.aux.cpu().numpy()
    for a in (st, it, aux):
        a.setflags(write=False)
    return env, st, it, aux


def host_items(env, it):
    return it if env._uses_items else None   # the library is handed NULL for the kinds that keep nothing there


def put(env, st, it, aux):
    env.state.copy_(torch.from_numpy(np.array(st)))
    env.items.copy_(torch.from_numpy(np.array(it)))
    env.aux.copy_(torch.from_numpy(np.array(aux)))


def both(env, st, it, aux, view):
    """(device image, host-build image) of the records st / it / aux, written into the env's tensors first."""
    put(env, st, it, aux)
    dev = env.render(view).cpu().numpy()
    return dev, rc.render_host(env.cfg, st, host_items(env, it), aux, view)


@pytest.mark.parametrize('kind', rc.KINDS)
def test_device_image_equals_the_host_build_byte_for_byte(kind):
    """Six kinds x three modes x two sizes at N = 5, on the states of 30 steps, on the hand-made poses (through set_state) and on the
    hostile states: every byte equals the host build of render_core.h."""
    env, st, it, aux = stepped(kind)
    try:
        for mode in rc.MODES:
            for size in rc.SIZES:
                v = rc.view_of(kind, mode, size)
                dev, host = both(env, st, it, aux, v)
                assert dev.shape == (N, size[1], size[0], 3) and dev.dtype == np.uint8
                assert np.array_equal(dev, host), (kind, mode, size, np.argwhere((dev != host).any(-1))[:4])
        hm = rc.hand_made(env.cfg, st)
        put(env, st, it, aux)
        env.set_state(torch.from_numpy(hm[:, :15].copy()), torch.from_numpy(hm[:, 15:29].copy()))
        torch.cuda.synchronize()
        got = env.state.cpu().numpy()
        assert np.array_equal(got[:, :15], hm[:, :15])
        for mode in rc.MODES:
            v = rc.view_of(kind, mode, (48, 32))
            assert np.array_equal(env.render(v).cpu().numpy(), rc.render_host(env.cfg, got, host_items(env, it), aux, v)), (kind, mode, 'hand-made')
        for s, i2, a, _, _, _, _ in rc.hostile(env.cfg, st, it, aux):
            for mode in rc.MODES:
                v = rc.view_of(kind, mode, (32, 32))
                dev, host = both(env, s, i2, a, v)
                assert np.array_equal(dev, host), (kind, mode, 'hostile')
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_image_equals_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: the three modes at 16 x 16 (the smallest
    view the library takes) and 48 x 32 and the library's default view on the shard, the world mode on the hostile states (on the entries of 64 items: NaN and inf in the
    last item): every byte equals the host build of render_core.h.  On the entries of 64 items the device paints the items 50 and 63."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    views = [rc.view_of(cfg, mode, size) for mode in rc.MODES for size in ((16, 16), (48, 32))] + [R.default_view(env.cfg)]
    for v in views:
        dev, host = both(env, st, it, aux, v)
        assert np.array_equal(dev, host), (name, v.mode, v.width, np.argwhere((dev != host).any(-1))[:4])
    put(env, st, it, aux)
    assert np.array_equal(env.render().cpu().numpy(), rc.render_host(env.cfg, st, host_items(env, it), aux, views[-1])), (name, 'default')
    for s, i2, a, _, _, _, _, _ in scfg.hostile(name, rc.hostile):
        dev, host = both(env, s, i2, a, rc.view_of(cfg, R.HRL_VIEW_WORLD, (48, 32)))
        assert np.array_equal(dev, host), (name, 'hostile')
    if scfg.many_items(cfg):
        gone = np.array(it)
        for e, i, _ in scfg.NEAR_ITEMS:
            gone[e, 2 * (i % (cfg.n_food + cfg.n_poison)):][:2] = (100.0, 0.0)
        v = rc.view_of(cfg, R.HRL_VIEW_EGO_HEADING, (48, 32))
        a, b = both(env, st, it, aux, v)[0], both(env, st, gone, aux, v)[0]
        assert all((a[e] != b[e]).any() for e, _, _ in scfg.NEAR_ITEMS)


def test_one_large_image_and_the_default_view():
    env, st, it, aux = stepped(K.HRL_ANT_GATHER)
    v = rc.view_of(K.HRL_ANT_GATHER, R.HRL_VIEW_WORLD, (256, 256))
    dev, host = both(env, st, it, aux, v)
    assert np.array_equal(dev, host)
    img = env.render()   # the 64 x 64 world view of the whole arena
    assert tuple(img.shape) == (N, 64, 64, 3) and img.dtype == torch.uint8 and img.device == env.device
    assert np.array_equal(img.cpu().numpy(), rc.render_host(env.cfg, st, it, aux, R.default_view(env.cfg)))


def test_masked_envs_are_untouched():
    env = make_env(K.HRL_ANT_MAZE, n=7)
    env.reset()
    v = rc.view_of(K.HRL_ANT_MAZE, R.HRL_VIEW_WORLD, (48, 32))
    full = env.render(v).cpu().numpy()
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8)
    out = torch.full((7, 32, 48, 3), 0xAB, dtype=torch.uint8, device='cuda')
    assert env.render(v, mask=mask, out=out) is out
    got = out.cpu().numpy()
    for e in range(7):
        assert np.array_equal(got[e], full[e]) if mask[e] else (got[e] == 0xAB).all()
    fresh = env.render(v, mask=mask).cpu().numpy()
    assert (fresh[1] == 0).all() and np.array_equal(fresh[0], full[0])
    env.close()


def test_render_follows_the_stream_and_replays_in_a_graph():
    """step + render captured once (the first render call ran before the capture) and replayed three times give the images of the eager
    sequence; the launch goes to the env's current stream."""
    kind, n = K.HRL_ANT_GATHER, 16
    v = rc.view_of(kind, R.HRL_VIEW_EGO_HEADING, (48, 32))
    acts = torch.rand(4, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 2 - 1
    eager, eager_imgs = make_env(kind, n), []
    eager.reset()
    for r in range(4):
        eager.step(acts[r])
        eager_imgs.append(eager.render(v).clone())
    env = make_env(kind, n)
    env.reset()
    static_a, out = acts[0].clone(), torch.zeros(n, 32, 48, 3, dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up torch asks for; the render's constants are uploaded here, outside the capture
        env.step(static_a)
        env.render(v, out=out)
        first = out.clone()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(first, eager_imgs[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(static_a)
        env.render(v, out=out)
    for r in range(1, 4):
        static_a.copy_(acts[r])
        g.replay()
        assert torch.equal(out, eager_imgs[r]), r
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager.state)
    del g
    env.close(); eager.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_POINT_GATHER)
    v = rc.view_of(K.HRL_POINT_GATHER, R.HRL_VIEW_EGO, (32, 32))
    out = torch.zeros(N, 32, 32, 3, dtype=torch.uint8, device='cuda')
    p = out.data_ptr()
    got = env.render(v, out=out)
    assert got is out and got.data_ptr() == p
    assert np.array_equal(out.cpu().numpy(), rc.render_host(env.cfg, st, it, aux, v))
    with pytest.raises(TypeError):
        env.render(v, out=torch.zeros(N, 32, 32, 3, device='cuda'))
    with pytest.raises(ValueError):
        env.render(v, out=torch.zeros(N, 32, 48, 3, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        env.render(v, out=torch.zeros(N, 32, 32, 3, dtype=torch.uint8))


def test_render_batch_of_a_gym_class_equals_the_batched_env():
    import hrl_pybullet_envs_amd as H
    env = H.AntGatherBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(5, 8, device='cuda'))
    v = R.default_view(env._backend().cfg, 'ego', 48, 32)
    a, b = env.render_batch(v), env._backend().render(v)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (5, 32, 48, 3) and torch.equal(a, b)
    b = env._backend()
    assert np.array_equal(a.cpu().numpy(), rc.render_host(b.cfg, b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy(), v))
    one = env.render(mode='rgb_array')   # the host-drawn picture of one env is what it was
    assert one.shape == (256, 256, 3)
    env.close()


def test_the_step_does_not_notice_the_renderer():
    """20 steps of a 16-env gather shard with render calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    views = [rc.view_of(kind, m, s) for m in rc.MODES for s in rc.SIZES]
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.render(views[t % len(views)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.render(views[(t + 1) % len(views)])
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()


@pytest.mark.parametrize('field,value', [('width', 40), ('height', 0), ('half_extent', float('nan')), ('half_extent', 0.0), ('half_extent', -2.0),
                                         ('mode', 7), ('struct_size', 16)])
def test_bad_views_are_refused_by_the_library(field, value):
    from hrl_pybullet_envs_amd._lib import HrlError
    env, st, it, aux = stepped(K.HRL_ANT_FLAT)
    v = rc.view_of(K.HRL_ANT_FLAT, R.HRL_VIEW_WORLD, (32, 32))
    setattr(v, field, value)
    out = torch.full((N, max(v.height, 16), max(v.width, 16), 3), 0xAB, dtype=torch.uint8, device='cuda')
    with pytest.raises(HrlError) as e:
        R.render(env.cfg, env._bufs_ref, v, None, out, None)
    want = rc.render_host(env.cfg, st, None, aux, v, expect_ok=False)
    assert want[0] == K.HRL_ERR_BAD_ARG and want[1] in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
