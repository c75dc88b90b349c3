"""The batched chase camera's specification (csrc/chase_core.h) on the CPU: its host build (tests/chase_host) against an independent fp64
reference written from include/hrl_chase.h alone (tests/chase_cases.py: world-coordinate rays against spheres, cylinders, a box, prisms
and the plane, its own forward kinematics, no cull), known answers, totality on hostile states, spec validation, the sanitised
stand-alone program and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import chase_cases as hc
import orc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import chase_device as Ch
from hrl_pybullet_envs_amd import scan_device as S
from test_camera_host import gather_env
from test_field_host import maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
EXEMPT_CAP = 0.01      # of the pixels of a case (a spec on a set of 5 states): asserted on the reference alone
DEPTH_WORST = 1.79e-5  # metres: the worst |host build - reference| measured over the sweep below (see the test's docstring)
DEPTH_TOL = 4 * DEPTH_WORST
ROUND = Ch.FACE_ROUND << 16


def states_of(cfg, state):
    return (('shard', state), ('spread', hc.spread(cfg, state)))


def pitch_of(spec):
    return float(np.degrees(np.arctan2(spec.pitch[1], spec.pitch[0])))


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states and with the robots spread about the arena;
    returns (the worst depth error in metres, every seg word of the reference)."""
    runs = []
    for spec in specs:
        for label, st in states_of(cfg, state):
            refs = [hc.reference(cfg, st[e], None if items is None else items[e], aux[e], spec) for e in range(N)]
            share = sum(int(x.sum()) for _, _, x in refs) / (N * spec.width * spec.height)
            where = (tag, spec.width, spec.height, spec.frame, spec.target_mode, round(pitch_of(spec)), spec.distance, spec.classes, spec.tile, label)
            print(f'{where}: {100 * share:.3f} % exempt')
            assert share <= EXEMPT_CAP, (where, share)   # on the reference alone
            runs.append((spec, where, st, refs))
    worst, words = 0.0, set()
    for spec, where, st, refs in runs:
        got = hc.chase_host(cfg, st, items, aux, spec)
        assert np.array_equal(got.rgb, hc.colour_of(got.seg))
        for e, (depth, seg, exempt) in enumerate(refs):
            wrong = (got.seg[e] != seg) & ~exempt
            assert not wrong.any(), (where, e, np.argwhere(wrong)[:5].tolist(), got.seg[e][wrong][:5], seg[wrong][:5])
            err = np.abs(got.depth[e].astype(float) - depth)[~exempt]
            print(f'{where} env {e}: depth error {err.max():.3e}')
            worst = max(worst, float(err.max()))
            assert err.max() <= DEPTH_TOL, (where, e, float(err.max()))
            assert np.array_equal(got.rgb[e][~exempt], hc.colour_of(seg)[~exempt])
            words |= set(np.unique(seg).tolist())
    return worst, words


@pytest.mark.parametrize('kind', hc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Six kinds x both frames x both target modes x 16 x 8, 48 x 24, 64 x 48 and 256 x 256 pixels, with the pitches -85, -60, -30, -10
    and +20 degrees (and -90 once per kind), the distances 1.5, 3 and 6 m, the yaws 0, 75 and 200 degrees, the class sets (everything |
    the robot alone | everything but the robot | the ground alone), tiles of 0 and 1 m, max_range 30 and 7 m and fields of view of 60
    and 87 degrees taken in turn (chase_cases.sweep), on the shard's states and with the robots spread about the arena.  A pixel is
    exempt where a comparison the reference made is within 1e-4 m of changing (chase_cases.reference); at most 1 % of the pixels of a
    case may be, asserted on the reference alone before the build is looked at.  On every other pixel seg equals the reference exactly,
    depth is within DEPTH_TOL, and rgb is the header's colour of the reference's seg; on every pixel rgb is the header's colour of the
    build's seg.  Every ant kind's sweep sees all 13 links, the point bot's at least three faces of the cube.

    Measured over this sweep (the printed lines): at most 0.56 % of a case's pixels exempt (point gather, 48 x 24, the robots spread,
    +20 degrees from 3 m: silhouettes of the cube and of item cubes); 0.0 - 0.47 % in the other kinds, the robot filling up to 33 % of
    an image.  The worst |depth - reference| on the other pixels is 1.781e-5 m (gather, 256 x 256, heading frame, -60 degrees from 3 m,
    everything: a ray grazing a leg's cylinder), 1.54e-5 m on the ground near the horizon (maze, -10 degrees), under 6e-6 m in most
    cases; DEPTH_TOL is four times the worst."""
    cfg, state, items, aux = shard(kind)
    worst, words = compare_with_the_reference(cfg, state, items, aux, hc.sweep(kind), f'kind {kind}')
    print(f'kind {kind}: worst depth error {worst:.3e} m')
    kinds_seen = {w & 255 for w in words}
    assert {Ch.HIT_NONE, Ch.HIT_GROUND, Ch.HIT_ROBOT} <= kinds_seen and (kind == K.HRL_ANT_FLAT or Ch.HIT_WALL in kinds_seen)
    robot = {w for w in words if w & 255 == Ch.HIT_ROBOT}
    if kind == K.HRL_POINT_GATHER:
        assert {w >> 8 & 255 for w in robot} == {0} and len({w >> 16 for w in robot}) >= 3, sorted(robot)
    else:
        assert {w >> 8 & 255 for w in robot} == set(range(13)) and {w >> 16 for w in robot} == {Ch.FACE_ROUND}, sorted(robot)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its DEPTH_TOL and its cap of 1 % exempt pixels, on every entry of sensor_configs.MATRIX: 48 x 24 pixels
    in the heading frame from 3 m and -30 degrees, 64 x 48 in the world frame from 6 m, -60 degrees and a yaw of 75 degrees out to 7 m
    over a ground of 0.5 m tiles, and the library's default spec, whose range is derived from the entry's own arena.  On the entry's
    hostile states the images of the envs whose robot stands at a finite place equal, bit for bit, those of the clean twin, and an env
    without a finite place sees nothing.  On the entries of 64 items some pixel shows an item of index 48 or more.

    Measured here: at most 0.63 % of a case's pixels exempt (gather-64 at 48 x 24: 64 cubes' corners), the worst depth error 2.0e-5 m
    (gather-wide), under 4e-6 m on nine of the eleven entries."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [hc.spec_of((48, 24), Ch.HRL_SCAN_HEADING), hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, Ch.HRL_EYE_GROUND, 0.3, 75.0, -60.0, 6.0, max_range=7.0, tile=0.5),
             Ch.default_spec(cfg)]
    worst, words = compare_with_the_reference(cfg, state, items, aux, specs, name)
    print(f'{name}: worst depth error {worst:.3e} m')
    assert {Ch.HIT_GROUND, Ch.HIT_ROBOT} <= {w & 255 for w in words}
    for spec in specs[:2]:
        check_hostile(cfg, spec, scfg.hostile(name, hc.hostile), name)
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(sorted(w & 0xFFFF for w in words)), sorted(words)


def check_hostile(cfg, spec, cases, tag):
    for s, it, a, cs, cit, ca, far, _ in cases:
        got = hc.chase_host(cfg, s, it, a, spec)
        want = hc.chase_host(hc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
        moved = [e for e in range(N) if not np.array_equal(s[e, 0:2].view(np.uint32), cs[e, 0:2].view(np.uint32))]   # the twin's robot stands elsewhere: another picture
        rows = [e for e in range(N) if e not in moved]
        assert hc.same(hc.Chase(*(x[rows] for x in got)), hc.Chase(*(x[rows] for x in want))), (tag, spec.width)
        blind = [e for e in range(N) if not np.isfinite(s[e, 0:2]).all()]
        assert (got.seg[blind] == 0).all() and (got.depth[blind] == np.float32(spec.max_range)).all() and (got.rgb[blind] == Ch.RGB_SKY).all()
        assert (want.seg != 0).any()


@pytest.mark.parametrize('kind', hc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range (the camera's hostile states):
    an env whose x or y is not finite sees nothing at all -- NONE, max_range and the sky on every pixel; a shape with a non-finite
    parameter is not seen -- the image equals, bit for bit, that of the clean twin without the shape.  A torso whose z is not finite is
    blind when the torso is the target; with the ground as target the scene is seen as ever and the robot, which has no finite place, is
    not."""
    cfg, state, items, aux = shard(kind)
    for frame in hc.FRAMES:
        for size, mode in (((48, 24), Ch.HRL_EYE_TORSO), ((64, 48), Ch.HRL_EYE_GROUND)):
            spec = hc.spec_of(size, frame, mode, 0.3)
            check_hostile(cfg, spec, hc.hostile(cfg, state, items, aux), kind)
            for bad in (np.nan, np.inf, -np.inf):
                s = np.array(state)
                s[4, 2] = bad
                got, clean = hc.chase_host(cfg, s, items, aux, spec), hc.chase_host(cfg, state, items, aux, spec)
                assert hc.same(hc.Chase(*(x[:4] for x in got)), hc.Chase(*(x[:4] for x in clean)))
                if mode == Ch.HRL_EYE_TORSO:
                    assert (got.seg[4] == 0).all() and (got.depth[4] == np.float32(spec.max_range)).all() and (got.rgb[4] == Ch.RGB_SKY).all()
                else:
                    no_robot = spec.copy()
                    no_robot.classes = Ch.EVERYTHING & ~Ch.ROBOT
                    want = hc.chase_host(cfg, state, items, aux, no_robot)
                    assert all(np.array_equal(x[4], y[4]) for x, y in zip(hc.bits(got), hc.bits(want))) and (want.seg[4] != 0).any()


def standing_ant(n=1, z=0.55, xy=(0.0, 0.0), yaw=0.0, kind=K.HRL_ANT_FLAT):
    """A shard of n ants with level torsos and straight legs."""
    cfg = orc.default_config(kind, num_envs=n)
    st = np.zeros((n, K.HRL_STATE_STRIDE), np.float32)
    st[:, 0:2], st[:, 2], st[:, 5], st[:, 6] = xy, z, np.sin(yaw / 2), np.cos(yaw / 2)
    items = None if kind == K.HRL_ANT_FLAT else np.full((n, orc.items_stride(cfg)), 100.0, np.float32)
    return cfg, st, items, np.zeros((n, K.HRL_AUX_STRIDE), np.int32)


def unproject(cfg, st, spec):
    """(E [3], D [H, W, 3]) of env 0 in fp64 from the binding's eye() and pixel_rays()."""
    E, F, L, U = (x[0].numpy() for x in Ch.eye(cfg, torch.from_numpy(st), spec))
    u, s = (x.numpy().astype(float) for x in Ch.pixel_rays(spec))
    return E, F[None, None] + u[None, :, None] * L[None, None] + s[:, None, None] * U[None, None]


def test_ground_alone_from_straight_above():
    """The ground alone at pitch -90: the depth is the eye's height over the ground on every pixel, 3.3 m from 3 m over a target 0.3 m
    up; with tiles of 1 m the parity is that of the hit point and flips across x = 1."""
    cfg, st, items, aux = standing_ant(xy=(1.0, 0.5))
    spec = hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, Ch.HRL_EYE_GROUND, 0.3, 0.0, -90.0, 3.0, Ch.GROUND, tile=0.0)
    got = hc.chase_host(cfg, st, items, aux, spec)
    assert (got.seg == (Ch.HIT_GROUND | Ch.FACE_GROUND << 16)).all() and np.abs(got.depth - 3.3).max() <= DEPTH_TOL and (got.rgb == 240).all()
    spec.tile = 1.0
    got = hc.chase_host(cfg, st, items, aux, spec)
    E, D = unproject(cfg, st, spec)
    assert abs(E[2] - hc.ground_z(cfg) - 3.3) < 1e-7 and np.abs(E[:2] - (1.0, 0.5)).max() < 1e-12   # (0.3 as a float32)
    P = E + got.depth[0][..., None] * D
    assert np.abs(P[..., 2] - hc.ground_z(cfg)).max() <= 1e-4
    sure = (np.abs(P[..., 0] - np.rint(P[..., 0])) > 1e-3) & (np.abs(P[..., 1] - np.rint(P[..., 1])) > 1e-3)
    kinds, parity, face = Ch.decode(got.seg[0].astype(np.int64))
    want = (np.floor(P[..., 0]) + np.floor(P[..., 1])).astype(np.int64) & 1
    assert (kinds == Ch.HIT_GROUND).all() and np.array_equal(parity[sure], want[sure]) and sure.mean() > 0.9
    row = (P[..., 1] > 0.1) & (P[..., 1] < 0.9)
    left, right = row & (P[..., 0] > 0.1) & (P[..., 0] < 0.9), row & (P[..., 0] > 1.1) & (P[..., 0] < 1.9)
    assert left.any() and right.any() and (parity[left] == 0).all() and (parity[right] == 1).all()   # across x = 1
    assert (got.rgb[0][left] == 240).all() and (got.rgb[0][right] == 240 * Ch.TILE_SHADE >> 8).all()


def test_a_standing_ant_from_straight_above():
    """Pitch -90 from 3 m over the torso's centre through a field of view of half a degree: the four centre pixels show link 0, the
    torso, at depth 3 - r_torso (their rays meet the sphere 0.7 mm off its top: 1e-6 m lower)."""
    cfg, st, items, aux = standing_ant()
    got = hc.chase_host(cfg, st, items, aux, hc.spec_of((16, 8), Ch.HRL_SCAN_HEADING, pitch=-90.0, tan_half_h=4e-3))
    centre = (slice(0, 1), slice(3, 5), slice(7, 9))
    assert (got.seg[centre] == (Ch.HIT_ROBOT | 0 << 8 | ROUND)).all() and np.abs(got.depth[centre] - (3.0 - hc.R_TORSO)).max() <= DEPTH_TOL
    assert (got.rgb[centre] == tuple(c * Ch.SHADES[Ch.FACE_ROUND] >> 8 for c in Ch.RGB_TORSO)).all()
    wide = hc.chase_host(cfg, st, items, aux, hc.spec_of((64, 48), Ch.HRL_SCAN_HEADING, pitch=-90.0))
    kinds, index, _ = Ch.decode(wide.seg[0].astype(np.int64))
    assert set(np.unique(index[kinds == Ch.HIT_ROBOT])) == set(range(13))   # straight legs: every link is seen from above


def bent_leg_env(cube):
    """A gather env whose ant bends the ankle of leg 0 by 1 rad, the foot pointing down to the ground, with food item 0 at `cube`."""
    cfg, st, items, aux = gather_env(((0.0, 0.0),), (cube,))
    st[0, 8] = 1.0
    return cfg, st, items, aux


def test_a_foot_hides_a_cube_behind_it_and_a_cube_the_foot():
    """World frame, the camera 3 m behind the ant and 5 degrees above the ground: with a food cube 0.6 m beyond the front left foot's tip
    on the line of sight, every pixel of the foot still shows the foot and some of them would show the cube without the robot; with the
    cube 0.6 m before the tip, every pixel of the cube shows the cube and some of them would show the foot without it."""
    cfg, st, items, aux = bent_leg_env((100.0, 0.0))
    tip = dict((link, p1) for link, _, p1 in hc.ant_capsules(st[0]))[2]
    assert -0.01 < tip[2] - hc.R_CAPS and tip[2] + hc.R_CAPS < 0.225   # the foot's ball is within the cube's z-interval
    spec = hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, Ch.HRL_EYE_GROUND, 0.0, 0.0, -5.0, 3.0, tan_half_h=0.3, tile=0.0)
    E = Ch.eye(cfg, torch.from_numpy(st), spec)[0][0].numpy()
    along = (tip[:2] - E[:2]) / np.linalg.norm(tip[:2] - E[:2])
    robot_only, cube_only = spec.copy(), spec.copy()
    robot_only.classes, cube_only.classes = Ch.ROBOT | Ch.GROUND, Ch.FOOD | Ch.GROUND
    foot = (hc.chase_host(cfg, st, items, aux, robot_only).seg[0] & 0xFFFF) == (Ch.HIT_ROBOT | 2 << 8)
    assert foot.sum() > 20
    for offset, hidden in ((0.6, 'cube'), (-0.6, 'foot')):
        items[0, 0:2] = tip[:2] + offset * along
        both = hc.chase_host(cfg, st, items, aux, spec).seg[0] & 0xFFFF
        cube = (hc.chase_host(cfg, st, items, aux, cube_only).seg[0] & 0xFFFF) == Ch.HIT_FOOD
        assert (foot & cube).sum() > 5, hidden
        if hidden == 'cube':
            assert (both[foot] == (Ch.HIT_ROBOT | 2 << 8)).all()
        else:
            assert (both[cube] == Ch.HIT_FOOD).all()


def test_an_eye_inside_a_solid_looks_out_through_it():
    """From (1.8, 0) in the maze the default camera's eye lies inside the box, and from (4.2, 0) with a yaw of 180 degrees beyond the +x
    wall's bounding line: the robot is seen all the same, and the containing solid appears in no pixel.  With the eye over the box
    (pitch -60: 2.6 m over the torso) the box is seen, from above."""
    cfg, st, aux = maze_env(((1.8, 0.0), (4.2, 0.0)))
    inside = hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, pitch=-10.0)
    E = Ch.eye(cfg, torch.from_numpy(st), inside)[0].numpy()
    assert -5 < E[0, 0] < 1 and abs(E[0, 1]) < 2 and 0 < E[0, 2] < 2
    got = hc.chase_host(cfg, st, None, aux, inside)
    kinds = got.seg & 255
    assert (kinds[0] != Ch.HIT_BOX).all() and (kinds[0] == Ch.HIT_ROBOT).sum() > 50 and (kinds[0] == Ch.HIT_WALL).any()
    front = hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, yaw=180.0, pitch=-10.0)
    E = Ch.eye(cfg, torch.from_numpy(st), front)[0].numpy()
    assert E[1, 0] > 5.0 and 0 < E[1, 2] < 2.5
    got = hc.chase_host(cfg, st, None, aux, front)
    walls = got.seg[1][(got.seg[1] & 255) == Ch.HIT_WALL] >> 8 & 255
    assert 0 not in walls and 1 in walls and ((got.seg[1] & 255) == Ch.HIT_ROBOT).sum() > 50   # the far wall, not the one the eye is in
    above = hc.chase_host(cfg, st, None, aux, hc.spec_of((64, 48), Ch.HRL_SCAN_WORLD, pitch=-60.0))
    assert (above.seg[0] == (Ch.HIT_BOX | Ch.FACE_TOP << 16)).any()


def test_a_joint_ball_names_the_proximal_link():
    """Leg 0 with its ankle bent by 1 rad, seen from straight above: the point of the ankle's ball 0.05 m beyond the end of aux_1's
    cylinder lies on neither cylinder; it is link 1's, aux_1 -- the proximal link of the ankle joint -- and not the foot's."""
    cfg, st, items, aux = bent_leg_env((100.0, 0.0))
    caps = dict((link, (p0, p1)) for link, p0, p1 in hc.ant_capsules(st[0]))
    pa = caps[1][1]
    e1 = (caps[1][1] - caps[1][0]) / np.linalg.norm(caps[1][1] - caps[1][0])
    q = pa + 0.05 * e1 + np.sqrt(hc.R_CAPS ** 2 - 0.05 ** 2) * np.array([0.0, 0.0, 1.0])
    spec = hc.spec_of((256, 256), Ch.HRL_SCAN_WORLD, pitch=-90.0, classes=Ch.ROBOT, tan_half_h=0.4)
    got = hc.chase_host(cfg, st, items, aux, spec)
    E, D = unproject(cfg, st, spec)
    X = E + ((q[2] - E[2]) / D[..., 2])[..., None] * D
    i, j = np.unravel_index(np.argmin(((X - q) ** 2).sum(-1)), X.shape[:2])
    assert np.linalg.norm(X[i, j] - q) < 0.01
    assert got.seg[0, i, j] == (Ch.HIT_ROBOT | 1 << 8 | ROUND) and abs(got.depth[0, i, j] - (E[2] - q[2])) < 6e-3   # (the pixel's ray passes within 6 mm of q)
    assert got.seg[0][(got.seg[0] & 0xFFFF) == (Ch.HIT_ROBOT | 2 << 8)].size > 0   # the foot itself is in the picture


def test_a_nan_joint_angle_removes_the_links_beyond_it():
    """A NaN ankle angle removes that leg's foot, a NaN hip angle its aux link and its foot; every other link and the scene stay where
    they were: outside the pixels that showed the removed links the image is the clean one's, bit for bit.  (Ants with their ankles
    bent by 0.6 rad, from 1.5 m and 80 degrees above: all 13 links are in the clean picture.)"""
    cfg, state, items, aux = gather_env(((0.0, 0.0),) * 3, ((2.0, 1.0),) * 3, yaw=0.4)
    state[:, 8:15:2] = (0.6, -0.6, -0.6, 0.6)
    spec = hc.spec_of((64, 48), Ch.HRL_SCAN_HEADING, pitch=-80.0, distance=1.5)
    clean = hc.chase_host(cfg, state, items, aux, spec)
    was = set(np.unique(clean.seg[2][(clean.seg[2] & 255) == Ch.HIT_ROBOT] >> 8 & 255))
    assert was == set(range(13))
    for leg in range(4):
        for joint, gone in ((8 + 2 * leg, {2 + 2 * leg}), (7 + 2 * leg, {1 + 2 * leg, 2 + 2 * leg})):
            s = np.array(state)
            s[2, joint] = np.nan
            got = hc.chase_host(cfg, s, items, aux, spec)
            assert hc.same(hc.Chase(*(x[:2] for x in got)), hc.Chase(*(x[:2] for x in clean)))
            seen = set(np.unique(got.seg[2][(got.seg[2] & 255) == Ch.HIT_ROBOT] >> 8 & 255))
            assert seen == was - gone, (leg, joint, sorted(seen))
            keep = ~(((clean.seg[2] & 255) == Ch.HIT_ROBOT) & np.isin(clean.seg[2] >> 8 & 255, sorted(gone)))
            assert all(np.array_equal(x[2][keep], y[2][keep]) for x, y in zip(hc.bits(got), hc.bits(clean)))


def test_an_env_does_not_depend_on_its_batch():
    """Env e of a shard of 5, alone in a shard of 1, and under a mask of its own: the same bytes; a masked env keeps its bytes; a NULL
    member is not written."""
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    spec = hc.spec_of((48, 24), Ch.HRL_SCAN_HEADING)
    full = hc.chase_host(cfg, state, items, aux, spec)
    one = orc.default_config(K.HRL_ANT_GATHER, num_envs=1, seed=cfg.seed, auto_reset=1)
    for e in range(N):
        alone = hc.chase_host(one, state[e:e + 1], items[e:e + 1], aux[e:e + 1], spec)
        assert hc.same(alone, hc.Chase(*(x[e:e + 1] for x in full))), e
    out = hc.Chase(np.full((N, 24, 48), -3, np.float32), np.full((N, 24, 48), -7, np.int32), np.full((N, 24, 48, 3), 0x7B, np.uint8))
    hc.chase_host(cfg, state, items, aux, spec, mask=np.array([1, 0, 5, 0, 1], np.uint8), out=out)
    for e in range(N):
        if e in (1, 3):
            assert (out.depth[e] == -3).all() and (out.seg[e] == -7).all() and (out.rgb[e] == 0x7B).all()
        else:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(hc.bits(out), hc.bits(full)))
    for want in (('depth',), ('seg',), ('rgb',), ('depth', 'rgb')):
        part = hc.chase_host(cfg, state, items, aux, spec, want=want)
        assert all((x is None) == (name not in want) and (x is None or np.array_equal(x, y)) for name, x, y in zip(hc.NAMES, hc.bits(part), hc.bits(full)))


def test_shades_and_unprojection():
    """shade_rgb equals the header's table for every class, link, parity and face; E + depth * D lies on the surface seen."""
    for cls, col in list(hc.COLOURS.items()) + [(0, Ch.RGB_SKY)]:
        for face in range(7):
            for index in (0, 1):
                word = hc.lib().chase_shade_rgb(cls | index << 8 | face << 16)
                k = Ch.SHADES[face] if cls else 256
                want = tuple(c * k >> 8 for c in col)
                if cls == Ch.HIT_GROUND and index:
                    want = tuple(c * Ch.TILE_SHADE >> 8 for c in want)
                assert (word & 255, word >> 8 & 255, word >> 16 & 255, word >> 24) == want + (0,), (cls, face, index)
    for link in range(13):
        for face in range(7):
            word = hc.lib().chase_shade_rgb(Ch.HIT_ROBOT | link << 8 | face << 16)
            assert (word & 255, word >> 8 & 255, word >> 16 & 255) == tuple(c * Ch.SHADES[face] >> 8 for c in hc.LINK_COLOURS[link]), (link, face)
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    spec = hc.spec_of((64, 48), Ch.HRL_SCAN_HEADING, yaw=75.0, pitch=-30.0)
    got = hc.chase_host(cfg, state, None, aux, spec)
    E, D = unproject(cfg, np.array(state), spec)
    P = E + got.depth[0][..., None] * D
    kinds, index, face = Ch.decode(got.seg[0].astype(np.int64))
    assert (kinds == Ch.HIT_GROUND).any() and np.abs(P[..., 2][kinds == Ch.HIT_GROUND] - hc.ground_z(cfg)).max() <= 1e-4
    torso = (kinds == Ch.HIT_ROBOT) & (index == 0)
    assert torso.any() and np.abs(np.linalg.norm(P[torso] - state[0, 0:3].astype(float), axis=-1) - hc.R_TORSO).max() <= 1e-4


SPEC_BAD = [('width', 0), ('width', 24), ('width', 272), ('height', 4), ('height', 12), ('height', 264), ('frame', 2), ('frame', -1), ('target_mode', 2), ('target_mode', -1),
            ('target_height', -0.1), ('target_height', 10.5), ('target_height', float('nan')), ('yaw', (0.9, 0.0)), ('yaw', (float('nan'), 0.0)), ('yaw', (1.0, 0.1)),
            ('pitch', (-0.5, -0.8660254)), ('pitch', (1.1, 0.0)), ('pitch', (0.0, float('nan'))), ('distance', 0.4), ('distance', 51.0), ('distance', float('nan')),
            ('tan_half_h', 1e-3), ('tan_half_h', 2e3), ('tan_half_h', float('nan')), ('tan_half_h', float('inf')), ('tan_half_v', 0.0), ('tan_half_v', -1.0),
            ('tan_half_v', float('nan')), ('max_range', 0.0), ('max_range', -1.0), ('max_range', float('inf')), ('max_range', float('nan')), ('classes', 0), ('classes', 128),
            ('classes', 256 | 1), ('tile', -1.0), ('tile', float('nan')), ('tile', 2e6), ('struct_size', 16), ('struct_size', 0), ('out', 'empty'), ('out', 'null')]
REASONS = {'width': 'chase width must be a multiple of 16 within 16..256', 'height': 'chase height must be a multiple of 8 within 8..256', 'frame': 'unknown chase frame',
           'target_mode': 'unknown chase target_mode', 'target_height': 'chase target_height must be finite and within 0..10', 'yaw': 'chase yaw must be a (cos, sin) pair',
           'pitch': 'chase pitch must be a (cos, sin) pair with cos >= 0', 'distance': 'chase distance must be within 0.5..50',
           'tan_half_h': 'chase tan_half_h must be finite and within (1e-3, 1e3]', 'tan_half_v': 'chase tan_half_v must be finite and within (1e-3, 1e3]',
           'max_range': 'chase max_range must be finite and positive', 'classes': 'chase classes must be a non-empty mask of', 'tile': 'chase tile must be within 0..1e6',
           'struct_size': 'struct_size is not sizeof', 'empty': 'chase out holds no pointer: at least one output must be given', 'null': 'null chase out'}


@pytest.mark.parametrize('field,value', SPEC_BAD)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = hc.spec_of((48, 24), Ch.HRL_SCAN_HEADING)
    out = hc.Chase(np.full((N, 24, 48), -3, np.float32), np.full((N, 24, 48), -7, np.int32), np.full((N, 24, 48, 3), 0x7B, np.uint8))
    if field in ('yaw', 'pitch'):
        getattr(spec, field)[0], getattr(spec, field)[1] = value
    elif field != 'out':
        setattr(spec, field, value)
    b = K.make_buffers(hc.ptr(state), hc.ptr(items), hc.ptr(aux), None, None, None, None, None)
    o = Ch.hrl_chase_out(**({} if value == 'empty' else {name: hc.ptr(a) for name, a in zip(hc.NAMES, out)}))
    ref = None if value == 'null' else C.byref(o)
    code = hc.lib().chase_host(C.byref(cfg), C.byref(b), C.byref(spec), None, ref)
    why = hc.lib().chase_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and REASONS[value if field == 'out' else field] in why, why
    untouched = lambda: (out.depth == -3).all() and (out.seg == -7).all() and (out.rgb == 0x7B).all()
    assert untouched()
    # the device library runs the same checks before it looks for a device
    L = Ch.lib()
    assert L.hrl_chase(C.byref(cfg), C.byref(b), C.byref(spec), None, ref, None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_chase_last_error() == b'hrl_chase: ' + why.encode()
    assert untouched()


def test_default_spec_and_the_mirrors():
    for kind in hc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, frame in Ch.FRAMES.items():
            s, h, r = Ch.default_spec(cfg, name), Ch.hrl_chase_spec(), S.default_spec(cfg)
            assert hc.lib().chase_host_default_spec(C.byref(cfg), frame, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.width, s.height, s.frame, s.target_mode, s.target_height, s.distance, s.tile) == (C.sizeof(Ch.hrl_chase_spec), 64, 48, frame, Ch.HRL_EYE_TORSO, 0.0, 3.0, 1.0)
            assert tuple(s.yaw) == (1.0, 0.0) and tuple(s.pitch) == (np.float32(np.cos(np.pi / 6)), -0.5)
            assert s.tan_half_h == np.float32(np.tan(np.pi / 6)) and s.tan_half_v == np.float32(np.tan(np.pi / 6) * 0.75)
            assert s.max_range == np.float32(r.max_range) + np.float32(3.0) and s.classes == Ch.EVERYTHING == 127
            assert hc.lib().chase_validate_spec(C.byref(s)) == b''
    s = Ch.default_spec(cfg, 'world', 128, 64, yaw_degrees=90, pitch_degrees=-90, distance=5.0, hfov_degrees=90, target='ground', target_height=0.5, max_range=6.0,
                        classes=Ch.ROBOT | Ch.GROUND, tile=0.0)
    assert (s.width, s.height, s.frame, s.target_mode, s.target_height, s.distance, s.max_range, s.classes, s.tile) == (128, 64, 0, Ch.HRL_EYE_GROUND, 0.5, 5.0, 6.0, 96, 0.0)
    assert s.yaw[1] == 1.0 and abs(s.yaw[0]) < 1e-7 and s.pitch[1] == -1.0 and 0 <= s.pitch[0] < 1e-7 and hc.lib().chase_validate_spec(C.byref(s)) == b''
    assert s.tan_half_h == np.float32(1.0) and s.tan_half_v == np.float32(0.5)   # float64, rounded once
    assert Ch.default_spec(cfg, vfov_degrees=90).tan_half_v == np.float32(np.tan(np.pi / 4))
    assert Ch.default_spec(cfg, distance=6.0).max_range == np.float32(float(np.float32(S.default_spec(cfg).max_range) + np.float32(3.0)) - 3.0 + 6.0)   # the scanner's range + the distance
    for pitch in (90, 45, -45):
        assert hc.lib().chase_validate_spec(C.byref(Ch.default_spec(cfg, pitch_degrees=pitch, yaw_degrees=123.4))) == b''
    with pytest.raises(ValueError):
        Ch.default_spec(cfg, 'sideways')
    with pytest.raises(ValueError):
        Ch.default_spec(cfg, target='hip')
    with pytest.raises(ValueError):
        Ch.default_spec(cfg, pitch_degrees=-91)
    assert hc.lib().chase_sizeof_spec() == C.sizeof(Ch.hrl_chase_spec) == 72 and hc.lib().chase_sizeof_out() == C.sizeof(Ch.hrl_chase_out) == 24
    assert Ch.Chase() == (None,) * 3 and Ch.Chase._fields == hc.NAMES
    u, v = Ch.pixel_rays(s)
    assert u.dtype == v.dtype and tuple(u.shape) == (128,) and tuple(v.shape) == (64,) and float(u[0]) == -float(u[-1]) > 0 and float(v[0]) == -float(v[-1]) > 0
    hdr = open(os.path.join(hc.ROOT, 'include', 'hrl_chase.h')).read()
    for name, value in (('HRL_CHASE_ROBOT', Ch.ROBOT), ('HRL_HIT_ROBOT', Ch.HIT_ROBOT), ('HRL_CHASE_MAX_SIZE', Ch.MAX_SIZE), ('HRL_CHASE_MIN_WIDTH', Ch.MIN_WIDTH),
                        ('HRL_CHASE_MIN_HEIGHT', Ch.MIN_HEIGHT), ('HRL_CHASE_TILE_SHADE', Ch.TILE_SHADE)):
        assert int(re.search(rf'#define {name} (\d+)', hdr).group(1)) == value
    assert 'RECALLED, UNPINNED' in hdr
    field = open(os.path.join(hc.ROOT, 'include', 'hrl_field.h')).read()
    assert int(re.search(r'#define HRL_FIELD_ROBOT (\d+)u', field).group(1)) == Ch.ROBOT
    render = open(os.path.join(hc.ROOT, 'include', 'hrl_render.h')).read()
    for name, col in (('TORSO', Ch.RGB_TORSO), ('LEG0', Ch.RGB_LEG0), ('LEG1', Ch.RGB_LEG1), ('LEG2', Ch.RGB_LEG2)):
        assert re.search(rf'#define HRL_RGB_{name} (\d+), (\d+), (\d+)', render).groups() == tuple(str(x) for x in col)


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """chase_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the images of every kind in both frames
    from reset-like and hostile states: exit status 0, sizeof(hrl_chase_spec) == the ctypes mirror's, checksums == the unsanitised host
    build's."""
    p = subprocess.run([hc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_chase_spec {C.sizeof(Ch.hrl_chase_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = hc.lib().chase_check_n_cases()
    assert n == len(sums) == 6 * 2 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert hc.lib().chase_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different images


def test_chase_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_chase_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the kernel and an LDS footprint of at most 8 KB; the header's symbols are SYMBOLS; the chase camera is an entry of
    build.py of its own, built by build() after the link states, and SENSORS stays the four."""
    code = 'from hrl_pybullet_envs_amd.build import build_chase, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_chase(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=hc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(hc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_chase_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*chase_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 8192
    hdr = open(os.path.join(hc.ROOT, 'include', 'hrl_chase.h')).read()
    assert set(re.findall(r'\b(hrl_chase(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_chase_out', 'hrl_chase_spec'} == set(Ch.SYMBOLS)
    for s in Ch.SYMBOLS:
        assert hasattr(Ch.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.CHASE == ('chase', 'libhrl_chase_hip.so', 'chase_hip.hip', 'chase_core.h', 'hrl_chase.h')
    assert [name for name, *_ in build.SENSORS] == ['render', 'scan', 'probe', 'field'] and 'chase' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_links(force, verbose)\n    build_chase(force, verbose)') > 0
