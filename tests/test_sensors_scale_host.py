"""What tests/test_gpu_sensors_scale.py leans on, checked without a GPU: an env's expected output depends on its own records only (the
host build of 256 envs in one call equals the build of the same envs five at a time), and the records of tests/scale_cases.py reach what
the checks at scale are about (floors on the host build's outputs at 4096 envs, conditions on the inputs in the style of
parity_cases.covered; the counts are printed)."""
import numpy as np
import pytest

import scale_cases as sx
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import render_device as R
from hrl_pybullet_envs_amd import scan_device as S
from parity_cases import covered

N, SIZE = sx.SHAPES[0]
GATHER = (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER)
# 64 hostile envs take the 25 (entry, row) pairs of scale_cases.hostile_record in turn; 6 pairs put NaN or +-inf into the robot's place
BLIND = 64 // 25 * 6


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize('kind', sx.KINDS)
@pytest.mark.parametrize('sensor', sx.SENSORS)
def test_expected_values_do_not_depend_on_the_batch(sensor, kind):
    """The first 256 of the 4096 records (16 spread, 4 hostile and 2 hand-made envs among them) built by the host in one call and in
    chunks of 5 (the last of 1): every output of every env is the same, bit for bit."""
    case = sx.expected(sensor, kind, N, SIZE)
    whole = sx.members(sx.host_build_rows(sensor, case, slice(0, 256)))
    chunks = [sx.members(sx.host_build_rows(sensor, case, slice(at, min(at + 5, 256)))) for at in range(0, 256, 5)]
    for m, (a, full) in enumerate(zip(whole, sx.members(case.want))):
        b = np.concatenate([c[m] for c in chunks])
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (sensor, kind, m)
        assert np.array_equal(bits(a), bits(full[:256])), (sensor, kind, m, 'against the build of all 4096')


def test_the_pattern_of_unequal_envs():
    """Spread, hostile and hand-made envs never coincide, every other env holds the oracle's records, and the blind envs are there."""
    for kind in sx.KINDS:
        for n, _ in sx.SHAPES:
            _, st0, it0, aux0 = sx.stepped(kind, n)
            _, st, it, aux = sx.records(kind, n)
            rows = [set(e for _, e in sx.turns(n, every, at)) for every, at in ((sx.SPREAD_EVERY, sx.SPREAD_AT), (sx.HOSTILE_EVERY, sx.HOSTILE_AT), (sx.HAND_EVERY, sx.HAND_AT))]
            assert not (rows[0] & rows[1] or rows[0] & rows[2] or rows[1] & rows[2])
            assert [len(r) for r in rows] == [(n - at + every - 1) // every for every, at in ((16, 3), (64, 21), (128, 77))]
            changed = (bits(st) != bits(st0)).any(1) | (bits(it) != bits(it0)).any(1) | (aux != aux0).any(1)
            assert set(np.nonzero(changed)[0]) <= rows[0] | rows[1] | rows[2] and changed.sum() >= len(rows[0])
            assert np.isfinite(st0).all() and sx.blind(st).sum() >= (n // 64) // 25 * 6 and set(np.nonzero(sx.blind(st))[0]) <= rows[1]


LAYERS = {K.HRL_ANT_GATHER: ('ground', 'wall', 'food', 'poison', 'leg1', 'leg2', 'torso'), K.HRL_ANT_MAZE: ('ground', 'wall', 'box', 'target', 'leg1', 'leg2', 'torso'),
          K.HRL_POINT_GATHER: ('ground', 'wall', 'food', 'poison', 'torso')}
HITS = {K.HRL_ANT_GATHER: {S.HIT_WALL, S.HIT_FOOD, S.HIT_POISON}, K.HRL_ANT_MAZE: {S.HIT_WALL, S.HIT_BOX, S.HIT_TARGET}, K.HRL_POINT_GATHER: {S.HIT_WALL, S.HIT_FOOD, S.HIT_POISON}}


@pytest.mark.parametrize('kind', sx.KINDS)
def test_the_records_reach_what_the_checks_at_scale_are_about(kind):
    """Floors on the host build's outputs at 4096 envs; each is a condition on the inputs.
    Render: the colour of every layer of the kind -- but leg0: the torso's disc and the capsule of leg1 cover the first leg segment but
    for a sliver a few millimetres wide, which no 0.13 m pixel of these pictures samples.
    Route: with K = 7 some routes among the gather kinds' 16 grown items are truncated; round the maze's one box no pulled route has more
    than 7 waypoints, so none is truncated there (the floor is 0 and says so)."""
    got = {s: sx.reached(s, kind, N, SIZE) for s in sx.SENSORS}
    print(kind, got)
    assert got['render']['colours'] >= {R.PALETTE[name] for name in LAYERS[kind]}
    assert got['scan']['hits'] >= HITS[kind] | {0} and got['scan']['blind'] >= BLIND        # (a blind robot's rays hit nothing: 0)
    assert got['probe']['nearest'] >= HITS[kind] and got['probe']['blockers'] >= HITS[kind] | {0}
    assert got['probe']['vias'] >= {0, 1} and (kind in GATHER or max(got['probe']['vias']) > 1)   # no way | straight | in the maze: round a corner
    covered(dict(mixed=N // 2, all_blocked=BLIND, blind=BLIND), **got['field'])                   # BLOCKED cells and finite ways | the blind envs: every cell BLOCKED
    covered(dict(bent=256, none=N, truncated=1 if kind in GATHER else 0, routes=N), **got['route'])   # none: every env has a start outside the grid
    covered(dict(fresh=N // 2, still_and_stale=N // 10, lit=N // 2), **got['see'])                # fresh > 0 in most envs | fresh == 0 where nothing moved
    covered(dict(with_edge=N // 2, reached=N // 2, cut_off=1, no_edge=BLIND), **got['frontier'])  # cut_off: edge cells, none of them reachable
