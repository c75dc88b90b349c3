"""The link states on the MI355X at the sizes they are run at: 4096 and 1029 envs (256 workgroups of 16 envs | 64 and a tail of 5), gather
and maze, every output of every env against the host build (tests/links_host, computed in C++), bit for bit -- a NaN for a NaN on the
hostile envs of scale_cases.records, whose payload is the processor's own.  A step of another env of the same size runs directly before
the launch on the same stream, as in the workload, and leaves its LDS behind.  Each case launches once, into outputs full of sentinel
bytes with 8 guard rows behind them."""
import functools

import numpy as np
import pytest
import torch

import links_cases as lc
import scale_cases as sx
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import links_device as Lk
from test_gpu_render import put
from test_gpu_sensors_scale import Arena, device   # the envs of 4096 and 1029 after 30 steps: made once, shared with the other sensors' scale checks

pytestmark = pytest.mark.gpu
CASES = ((K.HRL_ANT_GATHER, 4096, Lk.HRL_LINKS_HEADING), (K.HRL_ANT_MAZE, 1029, Lk.HRL_LINKS_WORLD))


@functools.lru_cache(None)
def expected(kind, n, frame):
    """(cfg, state, items, aux, spec, the host build's Links) on scale_cases.records: computed once, read-only."""
    cfg, st, it, aux = sx.records(kind, n)
    spec = lc.spec_of(frame, lc.sixteen_sites(13))
    want = lc.links_host(cfg, st, spec)
    sx.frozen(*want)
    return cfg, st, it, aux, spec, want


@pytest.mark.parametrize('kind,n,frame', CASES)
def test_device_equals_the_host_build_at_scale(kind, n, frame):
    cfg, st, it, aux, spec, want = expected(kind, n, frame)
    assert int(sx.blind(st).sum()) > 0   # some envs hold no finite place: their outputs are not finite either
    env, other, action = device(kind, n)
    try:
        put(env, st, it, aux)
        arena = Arena(list(want))
        other.step(action)   # on the same stream, nothing between the two launches
        env.links(spec, out=Lk.Links(*arena.out))
        torch.cuda.synchronize()
        got = lc.Links(*(t.cpu().numpy() for t in arena.out))
        for name, g, w in zip(lc.NAMES, got, want):
            bad = np.nonzero(~((lc.bits(g) == lc.bits(w)) | (np.isnan(g) & np.isnan(w))).reshape(n, -1).all(1))[0]
            assert bad.size == 0, (kind, n, name, bad[:8].tolist(), np.bincount(bad % 16, minlength=16).tolist())
        assert arena.guards_intact()
    finally:
        put(env, *sx.stepped(kind, n)[1:])
