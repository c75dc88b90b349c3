"""The batched link states on the MI355X (csrc/links_hip.hip, include/hrl_links.h) against the host build of their specification
(tests/links_host, csrc/links_core.h), bit for bit in all seven outputs, and their surface: None members, masks, streams and graph
replay, `out=`, the gym classes' links_batch(), `robot.parts` / `robot.feet`, and that the step does not notice them.  At most 37 envs
per test."""
import numpy as np
import pytest
import torch

import links_cases as lc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import links_device as Lk
from test_gpu_render import make_env, put, stepped   # the envs of 5 after reset + 30 steps: made once, shared with the renderer's tests

pytestmark = pytest.mark.gpu
N = 5
SIZES = (1, 5, 16, 17, 37)   # a lone env | a part of a group | a full group | a group and a lone env | two groups and a tail of 5


def host_of(links):
    return lc.Links(*(x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in links))


def same(a, b, nan_ok=False):
    """Every member the same bits."""
    return lc.same(host_of(a), host_of(b), nan_ok)


def site_sets(kind):
    """0 sites, the library's default ones (4; the point bot: 1) and 16 over every link."""
    b = Lk.n_links(kind)
    return ((), lc.foot_sites() if b > 1 else ((0, (0.0, 0.0, 0.0)),), lc.sixteen_sites(b))


def states_of(n, seed=0):
    """n hand-made ant states: tilted torsos, joints at and between their stops, x and y out to +-10 m, every velocity set."""
    return np.concatenate([lc.hand_made(seed + k, 12) for k in range((n + 11) // 12)])[:n]


def both(env, st, spec, mask=None):
    """(device link states, host-build link states) of the state records st, written into the env's tensor first."""
    env.state.copy_(torch.from_numpy(np.array(st)))
    return env.links(spec, mask=mask), lc.links_host(env.cfg, st, spec, mask=None if mask is None else mask.cpu().numpy())


@pytest.mark.parametrize('kind', lc.KINDS)
def test_device_equals_the_host_build_bit_for_bit(kind):
    """Six kinds x both frames x 0, 4 (1) and 16 sites at N = 5, on the states of 30 steps and (the ants) on hand-made poses: origin, com,
    quat, lin_vel, ang_vel, site_pos and site_vel equal the host build of links_core.h as uint32.  Then a NaN in another place of every
    env's record: the same, a NaN for a NaN."""
    env, st, it, aux = stepped(kind)
    b = Lk.n_links(kind)
    try:
        for s in (st,) + ((states_of(N, 20),) if b > 1 else ()):
            for frame in lc.FRAMES:
                for sites in site_sets(kind):
                    spec = lc.spec_of(frame, sites)
                    dev, host = both(env, s, spec)
                    assert tuple(dev.origin.shape) == (N, b, 3) and tuple(dev.quat.shape) == (N, b, 4) and dev.com.dtype == torch.float32
                    assert (dev.site_pos is None) == (not sites) and (not sites or tuple(dev.site_vel.shape) == (N, len(sites), 3))
                    assert same(dev, host), (kind, frame, len(sites))
        bad = np.array(st)
        for e, place in enumerate((0, 4, 9, 16, 24)):
            bad[e, place] = np.nan
        dev, host = both(env, bad, lc.spec_of(Lk.HRL_LINKS_WORLD, site_sets(kind)[2]))
        assert same(dev, host, nan_ok=True) and not bool(torch.isfinite(dev.origin[0]).all())
    finally:
        put(env, st, it, aux)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_device_equals_the_host_build_on_the_sensor_config_matrix(name):
    """Every entry of sensor_configs.MATRIX at N = 5, its shard's records written into the device env: both frames with 16 sites, and the
    library's default spec."""
    cfg, st, it, aux = scfg.shard(name)
    env = scfg.device_env(name)
    put(env, st, it, aux)
    for frame in lc.FRAMES:
        dev, host = both(env, st, lc.spec_of(frame, lc.sixteen_sites(Lk.n_links(cfg))))
        assert same(dev, host), (name, frame)
    assert same(env.links(), lc.links_host(env.cfg, st, Lk.default_spec(env.cfg))), (name, 'default')


@pytest.mark.parametrize('n', SIZES)
def test_batch_sizes_masks_and_single_outputs(n):
    """N = 1, 5, 16, 17 and 37 ant envs in both frames with 16 sites: every output equals the host build; each output alone (the others
    NULL) equals it too and nothing else is written; under a random mask, with the first env masked and with the whole last group masked
    the masked envs keep the bytes the tensors were filled with."""
    env = make_env(K.HRL_ANT_GATHER, n)
    env.reset()
    st = states_of(n, 40 + n)
    st[:, 29:32] = env.state[:, 29:32].cpu().numpy()
    sites = lc.sixteen_sites(13)
    for frame in lc.FRAMES:
        spec = lc.spec_of(frame, sites)
        dev, host = both(env, st, spec)
        assert same(dev, host), (n, frame)
    for name in lc.NAMES:
        filled = Lk.Links(*(torch.full((n,) + shape, -3.0, device='cuda') for shape in Lk.shapes(env.cfg, spec)))
        got = env.links(spec, out=Lk.Links(**{name: getattr(filled, name)}))
        assert all((x is None) == (k != name) for k, x in zip(lc.NAMES, got))
        torch.cuda.synchronize()
        assert np.array_equal(lc.bits(getattr(filled, name).cpu().numpy()), lc.bits(getattr(host, name))), (n, name)
        assert all(bool((x == -3).all()) for k, x in zip(lc.NAMES, filled) if k != name), (n, name)
    rng = np.random.RandomState(n)
    last_group = np.arange(n) < (n - 1) // 16 * 16
    masks = [rng.randint(0, 2, n), np.arange(n) != 0] + ([last_group] if n > 16 else [])
    for m in masks:
        mask = torch.from_numpy(np.asarray(m).astype(np.uint8) * 7)
        out = Lk.Links(*(torch.full((n,) + shape, -3.0, device='cuda') for shape in Lk.shapes(env.cfg, spec)))
        assert env.links(spec, mask=mask, out=out) is out
        o, on = host_of(out), np.asarray(m).astype(bool)
        for x, y in zip(o, host):
            assert np.array_equal(lc.bits(x[on]), lc.bits(y[on])) and (x[~on] == -3).all(), (n, m)
    fresh = env.links(spec, mask=torch.zeros(n, dtype=torch.uint8))
    assert all(not bool(x.any()) for x in fresh)   # fresh tensors are zeros where the mask leaves envs unwritten
    env.close()


def test_links_follow_the_stream_and_replay_in_a_graph():
    """After 30 step launches with nothing between them, on the env's stream and on a second stream, the link states are those of the
    state the steps left; one launch captured into a graph and replayed twice gives the link states of the state as it is at each
    replay."""
    kind, n = K.HRL_ANT_GATHER, 17
    env = make_env(kind, n)
    env.reset()
    spec = lc.spec_of(Lk.HRL_LINKS_HEADING, lc.sixteen_sites(13))
    acts = torch.rand(30, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6)) * 2 - 1
    env.links(spec)   # the constants are uploaded here
    for t in range(30):
        env.step(acts[t])
    dev = env.links(spec)
    torch.cuda.synchronize()
    assert same(dev, lc.links_host(env.cfg, env.state.cpu().numpy(), spec))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(30):
            env.step(acts[29 - t])
        dev = env.links(spec)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(dev, lc.links_host(env.cfg, env.state.cpu().numpy(), spec))
    out = Lk.Links(*(torch.zeros((n,) + shape, device='cuda') for shape in Lk.shapes(env.cfg, spec)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.links(spec, out=out)
    for r in range(2):
        st = states_of(n, 60 + r)
        env.state.copy_(torch.from_numpy(st))
        g.replay()
        torch.cuda.synchronize()
        assert same(out, lc.links_host(env.cfg, st, spec)), r
    del g
    env.close()


def test_out_is_reused_and_checked():
    env, st, it, aux = stepped(K.HRL_ANT_MAZE)
    put(env, st, it, aux)
    spec = lc.spec_of(Lk.HRL_LINKS_WORLD, lc.foot_sites())
    out = Lk.Links(*(torch.zeros((N,) + shape, device='cuda') for shape in Lk.shapes(env.cfg, spec)))
    ptrs = [x.data_ptr() for x in out]
    got = env.links(spec, out=out)
    assert got is out and [x.data_ptr() for x in got] == ptrs
    assert same(out, lc.links_host(env.cfg, st, spec))
    alone = env.links(spec, out=Lk.Links(com=torch.zeros(N, 13, 3, device='cuda')))
    assert isinstance(alone, Lk.Links) and alone.origin is None and alone.site_pos is None and torch.equal(alone.com, out.com)
    with pytest.raises(TypeError):
        env.links(spec, out=out._replace(com=out.com.double()))
    with pytest.raises(TypeError):
        env.links(spec, out=tuple(out))
    with pytest.raises(ValueError):
        env.links(spec, out=out._replace(quat=torch.zeros(N, 13, 3, device='cuda')))
    with pytest.raises(ValueError):
        env.links(spec, out=out._replace(com=torch.zeros(N, 13, 3)))   # on the host
    with pytest.raises(ValueError):
        env.links(spec, out=out._replace(origin=torch.zeros(N, 13, 6, device='cuda')[..., ::2]))   # not contiguous
    with pytest.raises(ValueError):
        env.links(spec, out=Lk.Links())
    with pytest.raises(ValueError):
        env.links(spec, out=out._replace(com=out.origin))   # aliased
    bad = spec.copy()
    bad.n_sites = 17
    with pytest.raises(ValueError):
        env.links(bad)
    from hrl_pybullet_envs_amd._lib import HrlError
    bad = spec.copy()
    bad.site_link[1] = 13
    filled = Lk.Links(*(torch.full((N,) + shape, -3.0, device='cuda') for shape in Lk.shapes(env.cfg, spec)))
    with pytest.raises(HrlError) as e:
        env.links(bad, out=filled)
    assert lc.links_host(env.cfg, st, bad, expect_ok=False)[1] in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((x == -3).all()) for x in filled)


def test_parts_and_feet_of_a_batched_and_of_a_single_env_equal_the_tensors():
    """`env.robot.parts` / `feet` (one links() launch, one copy) against links_batch(): batched [N, ...] rows, single-env numpy rows;
    `robot_body` and the torso part agree; the point bot has its cube and no feet."""
    import hrl_pybullet_envs_amd as H
    env = H.AntMazeBulletEnv(num_envs=5, device='cuda:0', seed=3)
    env.reset()
    for _ in range(3):
        env.step(torch.rand(5, 8, device='cuda') * 2 - 1)
    b = env._backend()
    st = b.state.cpu().numpy()
    t = env.links_batch()
    assert isinstance(t, Lk.Links) and same(t, b.links()) and same(t, lc.links_host(b.cfg, st, Lk.default_spec(b.cfg)))
    h = host_of(t)
    parts, feet = env.robot.parts, env.robot.feet
    assert tuple(parts) == Lk.NAMES(b.cfg) and len(feet) == 4
    for i, name in enumerate(Lk.NAMES(b.cfg)):
        p = parts[name]
        assert np.array_equal(p.get_position(), h.com[:, i]) and np.array_equal(p.pose().xyz(), h.com[:, i]) and np.array_equal(p.get_orientation(), h.quat[:, i])
        assert np.array_equal(p.speed(), h.lin_vel[:, i]) and np.array_equal(p.get_pose(), np.concatenate([h.com[:, i], h.quat[:, i]], 1)) and np.array_equal(p.origin(), h.origin[:, i])
        assert p.get_position().shape == (5, 3) and p.get_position().dtype == np.float64
    for l, f in enumerate(feet):
        assert np.array_equal(f.get_position(), h.com[:, Lk.FEET[l]])
    assert np.array_equal(parts['torso'].get_position(), env.robot.robot_body.get_position()) and np.array_equal(parts['torso'].get_pose(), env.robot.robot_body.get_pose())
    assert np.array_equal(parts['torso'].speed(), env.robot.robot_body.speed()) and np.allclose(parts['torso'].pose().rpy(), env.robot.body_rpy)
    env.close()
    one = H.AntGatherBulletEnv(seed=4)
    one.reset()
    one.step(np.zeros(8))
    b = one._backend()
    h = host_of(b.links())
    parts = one.robot.parts
    for i, name in enumerate(Lk.NAMES(b.cfg)):
        assert parts[name].get_position().shape == (3,) and np.array_equal(parts[name].get_position(), h.com[0, i]) and np.array_equal(parts[name].get_pose(), np.concatenate([h.com[0, i], h.quat[0, i]]))
    assert [np.array_equal(f.speed(), h.lin_vel[0, Lk.FEET[l]]) for l, f in enumerate(one.robot.feet)] == [True] * 4
    one.close()
    point = H.PointGatherBulletEnv(seed=5)
    point.reset()
    assert tuple(point.robot.parts) == ('cube',) and np.array_equal(point.robot.parts['cube'].get_position(), point.robot.body_real_xyz)
    with pytest.raises(AttributeError):
        point.robot.feet
    point.close()


def test_the_step_does_not_notice_the_links():
    """20 steps of a 16-env gather shard with links calls interleaved are bit-identical to the same steps without them."""
    kind, n = K.HRL_ANT_GATHER, 16
    a, b = make_env(kind, n), make_env(kind, n)
    a.reset(); b.reset()
    acts = torch.rand(20, n, 8, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9)) * 2 - 1
    specs = [lc.spec_of(f, s) for f in lc.FRAMES for s in site_sets(kind)]
    for t in range(20):
        oa = [x.clone() for x in a.step(acts[t])[:3]]
        b.links(specs[t % len(specs)])
        ob = [x.clone() for x in b.step(acts[t])[:3]]
        b.links() if t % 2 else b.links(specs[(t + 2) % len(specs)], mask=torch.arange(n) % 2)
        for x, y in zip(oa, ob):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), t
    for name in ('state', 'items', 'aux'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close(); b.close()
