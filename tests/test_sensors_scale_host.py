"""What tests/test_gpu_sensors_scale.py leans on, checked without a GPU: an env's expected output
depends on its own records only (the host build of 256 envs in one call equals the build of the same envs five at a time), the records of
tests/scale_cases.py reach what the checks at scale are about (floors on the host build's outputs, conditions on the inputs in the style
of parity_cases.covered; the counts are printed), and the byte-row comparison used at scale can fail.  The seven sensors of
scale_cases.SENSORS at 4096 envs; the four of scale_cases.LATER (chase, cast, closest, dyn) at the sizes of their own cases."""
import numpy as np
import pytest

import scale_cases as sx
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import cast_device as Ca
from hrl_pybullet_envs_amd import chase_device as Ch
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


# ------------------------------------------------------------------------------------------------ the four of scale_cases.LATER
LATER_FIRST = [(s, kind) + sx.LATER_SHAPES[s][0] for s in sx.LATER[:3] for kind in sx.KINDS] + [('dyn',) + c for c in sx.DYN_CASES]
BLIND_AT = {4096: 18, 1029: 6}   # the hostile envs whose (entry, row) pair leaves the robot no finite place: 64 and 16 envs take the 25 pairs in turn
SEEN = {kind: HITS[kind] | {Ch.HIT_NONE, Ch.HIT_GROUND, Ch.HIT_ROBOT} for kind in sx.KINDS}   # the sky or a miss | the scene of the kind | the ground | the robot itself
GROUND, WALL, BOX, FOOD, POISON, SELF = range(6)   # closest: the class axis
HAS = {K.HRL_ANT_GATHER: (GROUND, WALL, FOOD, POISON, SELF), K.HRL_ANT_MAZE: (GROUND, WALL, BOX, SELF), K.HRL_POINT_GATHER: (GROUND, WALL, FOOD, POISON)}


@pytest.mark.parametrize('sensor,kind,n,size', LATER_FIRST)
def test_expected_values_of_the_later_four_do_not_depend_on_the_batch(sensor, kind, n, size):
    """Chase, cast and closest at their 4096-env shape and every dyn case: the first 256 envs built by the host in one call and in
    chunks of 5 (cast: the rays sliced with the envs, ray_link shared) give the same bits, and those of the build of all envs."""
    case = sx.expected(sensor, kind, n, size)
    whole = sx.members(sx.host_build_rows(sensor, case, slice(0, 256)))
    chunks = [sx.members(sx.host_build_rows(sensor, case, slice(at, min(at + 5, 256)))) for at in range(0, 256, 5)]
    assert len(whole) == len(sx.members(case.want)) == {'chase': 3, 'cast': 4, 'closest': 5, 'dyn': 7}[sensor]
    for m, (a, full) in enumerate(zip(whole, sx.members(case.want))):
        b = np.concatenate([c[m] for c in chunks])
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (sensor, kind, m)
        assert np.array_equal(bits(a), bits(full[:256])), (sensor, kind, m, 'against the build of all envs')


def test_the_rays_and_the_hand_made_states_of_the_later_four():
    """Cast: [n, R, 6] rays of one pattern, every `to` moved by at most 0.2 m per axis and no two envs' rays the same; ray_link [R] names
    every link of the kind, the lidar on the torso and (the ants) the range finders on the feet.  Dyn's 16389 envs: 1024 groups of 16
    and 5, every 64th with a NaN in place 0, 4, 9, 16 or 24 in turn, all others finite."""
    for kind in sx.KINDS:
        for n, R in sx.LATER_SHAPES['cast']:
            x = sx.expected('cast', kind, n, R).extra
            rays, link = x['rays'], x['ray_link']
            assert rays.shape == (n, R, 6) and rays.dtype == np.float32 and link.shape == (R,) and link.dtype == np.int32
            assert (rays[:, :, 0:3] == rays[0, :, 0:3]).all() and float(np.abs(rays[:, :, 3:6] - rays[0, :, 3:6]).max()) <= 0.4 + 1e-6
            assert (rays[1:, :, 3:6] != rays[0, :, 3:6]).any((1, 2)).all()
            assert set(link.tolist()) == set(range(sx.n_links(kind))) and not link[:64].any()
            assert kind == K.HRL_POINT_GATHER or tuple(link[64:68]) == Ca.FOOT_LINKS
    kind, n, source = sx.DYN_CASES[2]
    cfg, st, it, aux = sx.hand_made_records(kind, n)
    assert n == 1024 * 16 + 5 and st.shape == (n, K.HRL_STATE_STRIDE) and st.dtype == np.float32
    bad = np.nonzero(~np.isfinite(st).all(1))[0]
    assert bad.tolist() == [e for _, e in sx.turns(n, sx.HOSTILE_EVERY, sx.HOSTILE_AT)]
    assert all(np.isnan(st[e, sx.DYN_PLACES[k % 5]]) and np.isnan(st[e]).sum() == 1 for k, e in enumerate(bad))


@pytest.mark.parametrize('kind', sx.KINDS)
def test_the_records_reach_what_the_later_four_are_about(kind):
    """Floors on the host build's outputs at both shapes of chase, cast and closest; each is a condition on the inputs, set at or under
    the host build's own counts (printed).
    Chase: every class of the kind, the sky, the ground and the robot; the robot in all but a fortieth of the envs (4076 | 4025 |
    4078 of 4096 show it; the 18 blind envs cannot); at 32 x 16 no pixel of a gather env samples
    the hip capsules 9 and 12 (11 of 13 links, the floor there), at 128 x 96 all 13 links are seen.
    Cast, the link frame: every class and a fifth of the rays each hitting and missing (the miss rate is 26 .. 65 %); at R = 1024 all
    13 links are hit; a blind env's rays are not finite in the world and hit nothing.
    Closest: finite cells in every class the kind has for every link of all but the hostile envs, +inf in the classes it lacks, no NaN;
    links in the ground (gather 3234 | maze 2097 | point 4041 of the cells at 4096), in a wall (741 | 90 | 57) and in the maze's box (353)."""
    B = sx.n_links(kind)
    for shape in (0, 1):
        got = {s: sx.reached(s, kind, *sx.LATER_SHAPES[s][shape]) for s in sx.LATER[:3]}
        n = sx.LATER_SHAPES['chase'][shape][0]
        print(kind, n, got)
        for s in ('chase', 'cast'):
            assert got[s]['classes'] >= SEEN[kind] and got[s]['blind'] >= BLIND_AT[n], s
            covered(dict(robot_envs=n - n // 40), **{k: v for k, v in got[s].items() if isinstance(v, int)})
            assert got[s]['links'] <= set(range(B)) and len(got[s]['links']) >= (B if shape else min(B, 11)), s
        rays = n * sx.LATER_SHAPES['cast'][shape][1]
        covered(dict(hits=rays // 5, misses=rays // 5), **{k: v for k, v in got['cast'].items() if isinstance(v, int)})
        c = got['closest']
        assert c['nan'] == 0 and c['blind'] >= BLIND_AT[n] and c['blind_cells'] == 0 and got['cast']['blind_hits'] == 0
        for cls in range(6):
            links = B - 1 if cls == SELF else B   # (the torso is in no pair of capsules)
            assert c['finite'][cls] + c['none'][cls] == B * n
            assert c['finite'][cls] >= links * (n - n // 64) if cls in HAS[kind] else c['finite'][cls] == 0, (cls, c)
        assert c['negative'][GROUND] >= n // 4 and c['negative'][WALL] >= n // 100 and (kind != K.HRL_ANT_MAZE or c['negative'][BOX] >= n // 30), c


@pytest.mark.parametrize('kind,n,source', sx.DYN_CASES)
def test_the_hostile_envs_of_the_dynamics_cases(kind, n, source):
    """On records() the blind envs have no finite centre of mass; on the hand-made states every hostile env has a non-finite output, and
    non-finite bias or accel unless its NaN is the robot's x (which only com reads).  Every other env is finite in all seven outputs."""
    got = sx.reached('dyn', kind, n, source)
    print(kind, n, source, got)
    assert got['others_not_finite'] == 0 and got['hostile'] == len(sx.turns(n, sx.HOSTILE_EVERY, sx.HOSTILE_AT))
    if source == sx.HAND_MADE:
        assert got['hostile_not_finite'] == got['hostile'] >= 256
        assert got['hostile_bias_or_accel'] == sum(1 for k, _ in sx.turns(n, sx.HOSTILE_EVERY, sx.HOSTILE_AT) if sx.DYN_PLACES[k % 5] != 0)
    else:
        assert got['hostile_not_finite'] >= BLIND_AT[n]


@pytest.mark.parametrize('sensor,kind,n,size', [('chase', K.HRL_POINT_GATHER) + sx.LATER_SHAPES['chase'][0], ('cast', K.HRL_ANT_MAZE) + sx.LATER_SHAPES['cast'][0],
                                                ('closest', K.HRL_ANT_GATHER) + sx.LATER_SHAPES['closest'][1], ('dyn',) + sx.DYN_CASES[2]])
def test_the_comparison_at_scale_can_fail(sensor, kind, n, size):
    """One bit of one env's row flipped in a COPY of an expected output (nothing in a kernel or a host build is touched): the byte-row
    comparison the GPU tests use (scale_cases.host_rows, differences) names exactly that output, that env and that byte -- the lowest
    and the highest bit, the first and the last env, under a `keep` selection too.  nan_for_nan hides the payload of a NaN and nothing
    else."""
    want = sx.members(sx.expected(sensor, kind, n, size).want)
    names = [str(i) for i in range(len(want))]
    rows = sx.host_rows(want)
    assert sx.differences(names, rows, rows) == dict(first=[], wrong_envs=0, wrong_envs_by_residue=[0] * 8)
    for m, (env, bit) in zip(range(len(want)), ((0, 0), (n - 1, 7), (n // 2 + 3, 3), (1, 31), (n - 2, 8), (77, 1), (n - 1, 0))):
        got = [np.array(r) for r in rows]
        byte = (got[m].shape[1] - 1) - bit // 8 if env else bit // 8
        got[m][env, byte] ^= 1 << (bit % 8)
        d = sx.differences(names, got, rows)
        assert d['first'] == [(names[m], env, byte, env % 8)] and d['wrong_envs'] == 1 and d['wrong_envs_by_residue'][env % 8] == 1, (m, d)
        keep = np.arange(n) % 3 != 0
        keep[env] = True
        d = sx.differences(names, [g[keep] for g in got], [r[keep] for r in rows], np.nonzero(keep)[0])
        assert d['first'] == [(names[m], env, byte, env % 8)] and d['wrong_envs'] == 1, (m, d)
        keep[env] = False
        assert sx.differences(names, [g[keep] for g in got], [r[keep] for r in rows], np.nonzero(keep)[0])['wrong_envs'] == 0
    if sensor == 'dyn':
        hostile = sx.HOSTILE_AT + sx.HOSTILE_EVERY   # the second hostile env, a NaN in place 4 (a quaternion component): its bias holds NaNs
        f = np.array(rows[1]).view(np.float32)
        assert np.isnan(f[hostile]).any()
        at = int(np.nonzero(np.isnan(f[hostile]))[0][0])
        other = f.view(np.uint32).copy()
        other[hostile, at] ^= 0x80000001   # the same NaN with another sign and payload
        assert np.isnan(other.view(np.float32)[hostile, at])
        assert sx.differences(['bias'], [other.view(np.uint8)], [rows[1]])['wrong_envs'] == 1
        assert sx.differences(['bias'], sx.nan_for_nan([other.view(np.uint8)]), sx.nan_for_nan([rows[1]]))['wrong_envs'] == 0
        other[hostile, at] = np.float32(1.0).view(np.uint32)   # a number for a NaN
        other[0, 0] ^= 1                                       # and a last bit of a finite number
        d = sx.differences(['bias'], sx.nan_for_nan([other.view(np.uint8)]), sx.nan_for_nan([rows[1]]))
        assert d['wrong_envs'] == 2 and [x[1] for x in d['first']] == [0, hostile], d
