"""The first-person camera on the MI355X at the sizes it is run at: 4096 envs of 32 x 16 pixels and 1029 envs of 128 x 128, gather and maze,
every output of every env against the host build (tests/camera_host, computed in C++), bit for bit.  Thousands of workgroups are then
resident together and queue behind one another; a step of another env of the same size runs directly before the camera launch on the same
stream, as in the workload, and leaves its LDS behind; neighbouring envs do unequal work (the spread, hostile and hand-made envs of
scale_cases.records, which is read and not touched).  Every case launches once after a step and once under a mask of every third env
into outputs full of sentinel bytes, with 8 guard rows behind them."""
import functools

import numpy as np
import pytest
import torch

import camera_cases as cc
import scale_cases as sx
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import camera_device as Cm
from test_gpu_render import put
from test_gpu_sensors_scale import SENTINEL, Arena, device, differences, host_rows   # the envs of 4096 and 1029 after 30 steps: made once, shared with the seven sensors' scale check

pytestmark = pytest.mark.gpu
KINDS = (K.HRL_ANT_GATHER, K.HRL_ANT_MAZE)
SHAPES = ((4096, (32, 16)), (1029, (128, 128)))   # (envs, (width, height)): the benchmark's size | the largest image; 1029 = 4 * 256 + 5


def spec_of(kind, size):
    """Everything and the ground, turning with the heading, 1.3 m over the torso (the maze: over the ground), out to 20 m."""
    return cc.spec_of(size, Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND if kind == K.HRL_ANT_MAZE else Cm.HRL_EYE_TORSO, 1.3, Cm.EVERYTHING, max_range=20.0, tan_half_h=cc.TANS[0])


@functools.lru_cache(None)
def expected(kind, n, size):
    """(cfg, state, items, aux, spec, the host build's Camera) on scale_cases.records: computed once, read-only."""
    cfg, st, it, aux = sx.records(kind, n)
    spec = spec_of(kind, size)
    want = cc.camera_host(cfg, st, it if sx.uses_items(kind) else None, aux, spec)
    sx.frozen(*want)
    return cfg, st, it, aux, spec, want


def check(arena, want, keep, tag):
    got = arena.rows()
    rows = host_rows(want)
    if keep is not None:
        got, rows = [g[keep] for g in got], [r[keep] for r in rows]
    if not all(np.array_equal(g, r) for g, r in zip(got, rows)):
        pytest.fail(f'{tag}: {differences(cc.NAMES, got, rows, None if keep is None else np.nonzero(keep)[0])}')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', range(len(SHAPES)))
def test_device_equals_the_host_build_at_scale(kind, shape):
    n, size = SHAPES[shape]
    cfg, st, it, aux, spec, want = expected(kind, n, size)
    assert {Cm.HIT_NONE, Cm.HIT_WALL, Cm.HIT_GROUND} <= set(np.unique(want.seg & 255).tolist()) and int(sx.blind(st).sum()) > 0
    env, other, action = device(kind, n)
    try:
        put(env, st, it, aux)
        once, masked = Arena(list(want)), Arena(list(want))
        other.step(action)   # on the same stream, nothing between the two launches
        env.camera(spec, out=Cm.Camera(*once.out))
        torch.cuda.synchronize()
        check(once, want, None, (kind, n, size, 'after a step'))
        assert once.guards_intact()
        mask = np.arange(n) % 3 != 0
        other.step(action)
        env.camera(spec, mask=torch.from_numpy(mask.astype(np.uint8)).cuda(), out=Cm.Camera(*masked.out))
        torch.cuda.synchronize()
        check(masked, want, mask, (kind, n, size, 'masked'))
        assert all((r[~mask] == SENTINEL).all() for r in masked.rows()), (kind, n, 'a masked env was written')
        assert masked.guards_intact()
    finally:
        put(env, *sx.stepped(kind, n)[1:])
