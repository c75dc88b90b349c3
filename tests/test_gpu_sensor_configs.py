"""The sensor config matrix seen from the API, on the MI355X: a gym class built with non-default arguments hands its sensors the config it
was built with, and a config changed on a live env reaches the next sensor launch (the sensors' device constants are cached per config
bytes, csrc/sensor_launch.h).  The matrix itself runs in tests/test_gpu_<sensor>.py."""
import numpy as np
import pytest
import torch

import camera_cases as cc
import field_cases as fc
import render_cases as rc
import scan_cases as sc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import camera_device as Cm
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import render_device as R
from hrl_pybullet_envs_amd import scan_device as S
from test_gpu_camera import same as same_camera
from test_gpu_field import same as same_field
from test_gpu_render import make_env
from test_gpu_scan import same as same_scan

pytestmark = pytest.mark.gpu


def records(b):
    torch.cuda.synchronize()
    return b.state.cpu().numpy(), b.items.cpu().numpy(), b.aux.cpu().numpy()


def test_a_gym_class_with_non_default_arguments_hands_them_to_its_sensors():
    """AntGatherBulletEnv(n_food=40, n_poison=24, n_bins=64, world_size=(8, 8)) at N = 5 after 20 steps: scan_batch(), render_batch() and
    camera_batch(), with the library's default specs and with given ones, equal the host build on the env's own records of 128 floats --
    which differs from the host build under the class's default arguments."""
    import hrl_pybullet_envs_amd as H
    env = H.AntGatherBulletEnv(num_envs=5, device='cuda:0', seed=3, n_food=40, n_poison=24, n_bins=64, world_size=(8, 8))
    env.reset()
    g = torch.Generator(device='cpu').manual_seed(4)
    for _ in range(20):
        env.step((torch.rand(5, 8, generator=g) * 2 - 1).cuda())
    b = env._backend()
    cfg = b.cfg
    assert (cfg.n_food, cfg.n_poison, cfg.n_bins, tuple(cfg.world_size)) == (40, 24, 64, (8.0, 8.0)) and b.items.shape[1] == 128
    st, it, aux = records(b)
    for spec in (None, sc.spec_of(65, S.HRL_SCAN_HEADING, 20.0), sc.spec_of(1, S.HRL_SCAN_WORLD, 6.0)):
        want = sc.scan_host(cfg, st, it, aux, spec if spec is not None else S.default_spec(cfg))
        assert same_scan(env.scan_batch(spec), want), spec
    full = sc.scan_host(cfg, st, it, aux, sc.spec_of(512, S.HRL_SCAN_HEADING, 20.0))
    assert same_scan(env.scan_batch(sc.spec_of(512, S.HRL_SCAN_HEADING, 20.0)), full)
    assert (S.decode(full[1])[1][np.isin(S.decode(full[1])[0], (S.HIT_FOOD, S.HIT_POISON))] >= 16).any()   # an item the default arguments do not have
    for view in (None, rc.view_of(cfg, R.HRL_VIEW_EGO_HEADING, (48, 32))):
        want = rc.render_host(cfg, st, it, aux, view if view is not None else R.default_view(cfg))
        assert np.array_equal(env.render_batch(view).cpu().numpy(), want)
    assert R.default_view(cfg).half_extent == 4.0
    for spec in (None, cc.spec_of((16, 8), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 1.3)):
        want = cc.camera_host(cfg, st, it, aux, spec if spec is not None else Cm.default_spec(cfg))
        assert same_camera(env.camera_batch(spec), want)
    env.close()


def test_a_live_config_change_reaches_the_next_sensor_launch():
    """A gather env of 5 whose sensors have run (their constants are on the device) is handed another world_size through update_config: the
    next eager scan, field and render -- with given specs and with the library's defaults, which are derived from the config -- equal the
    host build under the NEW config, and that differs from the host build under the old one."""
    env = make_env(K.HRL_ANT_GATHER)
    env.reset()
    g = torch.Generator(device='cpu').manual_seed(6)
    for _ in range(5):
        env.step((torch.rand(5, 8, generator=g) * 2 - 1).cuda())
    old = env.cfg.copy()
    st, it, aux = records(env)

    def device():
        spec, fspec, view = sc.spec_of(65, S.HRL_SCAN_HEADING, 20.0), fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.25, F.FOOD, half=7.7), rc.view_of(K.HRL_ANT_GATHER, R.HRL_VIEW_WORLD, (48, 32))
        return (env.scan(spec), env.scan()), (env.field(fspec), env.field()), (env.render(view).cpu().numpy(), env.render().cpu().numpy())

    def host(cfg):
        spec, fspec, view = sc.spec_of(65, S.HRL_SCAN_HEADING, 20.0), fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.25, F.FOOD, half=7.7), rc.view_of(K.HRL_ANT_GATHER, R.HRL_VIEW_WORLD, (48, 32))
        return ((sc.scan_host(cfg, st, it, aux, spec), sc.scan_host(cfg, st, it, aux, S.default_spec(cfg))),
                (fc.field_host(cfg, st, it, aux, fspec), fc.field_host(cfg, st, it, aux, F.default_spec(cfg))),
                (rc.render_host(cfg, st, it, aux, view), rc.render_host(cfg, st, it, aux, R.default_view(cfg))))

    def check(cfg, when):
        (s, f, r), (hs, hf, hr) = device(), host(cfg)
        for k in range(2):
            assert same_scan(s[k], hs[k]), (when, 'scan', k)
            assert same_field(f[k], hf[k]), (when, 'field', k)
            assert np.array_equal(r[k], hr[k]), (when, 'render', k)

    check(old, 'before')
    new = old.copy()
    new.world_size[0], new.world_size[1] = 9.0, 11.0
    env.update_config(new)
    check(new, 'after')
    a, b = host(old), host(new)
    assert not same_scan(a[0][0], b[0][0]) and not fc.same(a[1][0], b[1][0]) and not np.array_equal(a[2][0], b[2][0])   # the test can tell the two configs apart
    assert S.default_spec(new).max_range != S.default_spec(old).max_range and R.default_view(new).half_extent != R.default_view(old).half_extent
    torch.cuda.synchronize()
    assert np.array_equal(env.state.cpu().numpy(), st) and np.array_equal(env.items.cpu().numpy(), it)   # the sensors only read
    env.close()
