"""The batched first-person camera's specification (csrc/camera_core.h) on the CPU: its host build (tests/camera_host) against an
independent fp64 reference written from include/hrl_camera.h alone (tests/camera_cases.py: 3-D rays in world coordinates), known
answers, totality on hostile states, spec validation, the sanitised stand-alone program and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import camera_cases as cc
import orc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import camera_device as Cm
from hrl_pybullet_envs_amd import scan_device as S
from test_field_host import maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
EXEMPT_CAP = 0.01      # of the pixels of a case (a spec on a set of 5 states): asserted on the reference alone
DEPTH_WORST = 1.74e-5  # metres: the worst |host build - reference| measured over the sweep below (see the test's docstring)
DEPTH_TOL = 4 * DEPTH_WORST


def states_of(cfg, state):
    return (('shard', state), ('spread', cc.spread(cfg, state)))


@pytest.mark.parametrize('kind', cc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Six kinds x both frames x both eye modes x 16 x 8, 48 x 24, 64 x 40 and 128 x 128 pixels, with the eye heights 0.6, 1.3 and 2.2 m,
    the class sets (everything | the ground alone | every shape without the ground), max_range 30 and 7 m and fields of view of 87 and
    58 degrees taken in turn (camera_cases.sweep), on the shard's states and with the robots spread about the arena.  A pixel is exempt
    where a comparison the reference made is within 1e-4 m of changing (camera_cases.reference); at most 1 % of the pixels of a case may
    be, asserted on the reference alone before the build is looked at.  On every other pixel seg equals the reference exactly, depth is
    within DEPTH_TOL, and rgb is the header's colour of the reference's seg; on every pixel rgb is the header's colour of the build's seg.

    Measured over this sweep (the printed lines): at most 0.51 % of a case's pixels exempt (65 of 12 800: gather and flagrun at 64 x 40,
    where a column's ray passes within 1e-4 m of a cube's corner or the post's rim and the whole column is exempted -- a column shares
    its ground-plan ray); none at all in 133 of the 192 cases.  The worst |depth - reference| on the other pixels is 1.731e-5 m (gather,
    48 x 24, heading frame, 2.2 m over the torso: the first row under the horizon comes down on a wall's top 22.6 m away), between
    4.1e-6 and 1.2e-5 m in the other kinds; DEPTH_TOL is four times the worst."""
    cfg, state, items, aux = shard(kind)
    worst, codes = compare_with_the_reference(cfg, state, items, aux, cc.sweep(kind), f'kind {kind}')
    kinds_seen = {c & 255 for c in codes}
    print(f'kind {kind}: worst depth error {worst:.3e} m')
    assert {Cm.HIT_NONE, Cm.HIT_GROUND} <= kinds_seen and (kind == K.HRL_ANT_FLAT or Cm.HIT_WALL in kinds_seen)


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states and with the robots spread about the arena;
    returns (the worst depth error in metres, every code of the reference's seg)."""
    runs = []
    for spec in specs:
        for label, st in states_of(cfg, state):
            refs = [cc.reference(cfg, st[e], None if items is None else items[e], aux[e], spec) for e in range(N)]
            share = sum(int(x.sum()) for _, _, x in refs) / (N * spec.width * spec.height)
            print(f'{tag} {spec.width} x {spec.height} frame {spec.frame} eye {spec.eye_mode} classes {spec.classes} {label}: {100 * share:.3f} % exempt')
            assert share <= EXEMPT_CAP, (tag, spec.width, spec.height, spec.frame, spec.eye_mode, label, share)   # on the reference alone
            runs.append((spec, label, st, refs))
    worst, codes = 0.0, set()
    for spec, label, st, refs in runs:
        got = cc.camera_host(cfg, st, items, aux, spec)
        assert np.array_equal(got.rgb, cc.colour_of(got.seg))
        for e, (depth, seg, exempt) in enumerate(refs):
            where = (tag, spec.width, spec.height, spec.frame, spec.eye_mode, spec.classes, label, e)
            wrong = (got.seg[e] != seg) & ~exempt
            assert not wrong.any(), (where, np.argwhere(wrong)[:5].tolist(), got.seg[e][wrong][:5], seg[wrong][:5])
            err = np.abs(got.depth[e].astype(float) - depth)[~exempt]
            print(f'{where}: depth error {err.max():.3e}')
            worst = max(worst, float(err.max()))
            assert err.max() <= DEPTH_TOL, (where, float(err.max()))
            assert np.array_equal(got.rgb[e][~exempt], cc.colour_of(seg)[~exempt])
            codes |= set(np.unique(seg & 0xFFFF).tolist())
    return worst, codes


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its DEPTH_TOL and its cap of 1 % exempt pixels, on every entry of sensor_configs.MATRIX: 48 x 24 pixels
    in the heading frame from 0.6 m over the torso, 64 x 40 in the world frame from 1.3 m over the ground out to 7 m (both 87 degrees wide:
    at 58 degrees four columns of point-64's spread robots pass a cube's corner within 1e-4 m and 1.27 % of the reference's pixels are
    exempt, over the cap; measured here at most 0.99 %, point-64 under the default spec), and the library's
    default spec, whose range is derived from the entry's own arena (flagrun's open field has none).  On the entry's hostile states
    the images equal, bit for bit, those of the clean twin and an env without a finite place sees nothing.  On the entries of 64 items
    some pixel shows an item of index 48 or more; on maze-12 the posts 8 and 11 are seen."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6, tan_half_h=cc.TANS[0]),
             cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 1.3, max_range=7.0, tan_half_h=cc.TANS[0]), Cm.default_spec(cfg)]
    worst, codes = compare_with_the_reference(cfg, state, items, aux, specs, name)
    print(f'{name}: worst depth error {worst:.3e} m')
    assert {Cm.HIT_NONE, Cm.HIT_GROUND} <= {c & 255 for c in codes}
    for spec in specs[:2]:
        for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, cc.hostile):
            got = cc.camera_host(cfg, s, it, a, spec)
            want = cc.camera_host(cc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
            rows = [e for e in range(N) if e not in blind]
            assert cc.same(cc.Camera(*(x[rows] for x in got)), cc.Camera(*(x[rows] for x in want))), (name, spec.width)
            b = list(blind)
            assert (got.seg[b] == 0).all() and (got.depth[b] == np.float32(spec.max_range)).all() and (got.rgb[b] == Cm.RGB_SKY).all()
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(sorted(codes)), sorted(codes)
    if name == 'maze-12':
        assert {Cm.HIT_TARGET | t << 8 for t in (8, 11)} <= codes


def gather_env(robots, cubes, yaw=0.0, z=0.55):
    """A gather shard with hand-placed robots; env e's food item 0 stands at cubes[e], every other item far away."""
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=len(robots))
    st = np.zeros((len(robots), K.HRL_STATE_STRIDE), np.float32)
    st[:, 2], st[:, 5], st[:, 6] = z, np.sin(yaw / 2), np.cos(yaw / 2)
    st[:, 0:2] = robots
    items = np.zeros((len(robots), orc.items_stride(cfg)), np.float32)
    items[:, 0:2 * (cfg.n_food + cfg.n_poison):2] = 100.0
    items[:, 0:2] = cubes
    return cfg, st, items, np.zeros((len(robots), K.HRL_AUX_STRIDE), np.int32)


def test_flat_ground_alone():
    """The ground alone from 0.6 m: the depth of row i is eye_height / -s_i in every column, and the sky is above the horizon."""
    cfg, st, aux = maze_env(((-2.0, -5.0),))
    spec = cc.spec_of((64, 40), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 0.6, Cm.GROUND, max_range=1e6)
    got = cc.camera_host(cfg, st, None, aux, spec)
    u, s = (x.numpy().astype(float) for x in Cm.pixel_rays(spec))
    assert (s[:20] > 0).all() and (s[20:] < 0).all() and u[0] > 0 > u[-1]
    assert (got.seg[0, :20] == Cm.HIT_NONE).all() and (got.depth[0, :20] == np.float32(1e6)).all() and (got.rgb[0, :20] == Cm.RGB_SKY).all()
    assert (got.seg[0, 20:] == (Cm.HIT_GROUND | Cm.FACE_GROUND << 16)).all() and (got.rgb[0, 20:] == (240, 240, 240)).all()
    want = (0.6 / -s[20:])[:, None] * np.ones(64)
    assert np.abs(got.depth[0, 20:] - want).max() <= 1e-5 * want.max()
    near = cc.camera_host(cfg, st, None, aux, cc.spec_of((64, 40), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 0.6, Cm.GROUND, max_range=5.0))
    t = (0.6 / -s[20:])[:, None] * np.sqrt(1 + u * u)[None, :]   # the horizontal range decides, not the depth
    sure = np.abs(t - 5.0) > 1e-3
    assert np.array_equal((near.seg[0, 20:] != 0)[sure], (t <= 5.0)[sure]) and (near.seg[0, 20:] == 0).any() and (near.seg[0, 20:] != 0).any()


def test_a_wall_faced_squarely():
    """World frame in a gather arena of 15 x 15: from (1.5, 0) the +x wall's centre line is D = 6 m ahead.  Every pixel of the wall has
    depth D, and its top edge lies at s = (ground_z + 2.5 - ez) / D: the rows above it see the sky (the ground is off)."""
    cfg, st, items, aux = gather_env(((1.5, 0.0),), ((100.0, 0.0),))
    spec = cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 0.6, Cm.WALL, tan_half_h=0.5, tan_half_v=0.6)
    got = cc.camera_host(cfg, st, items, aux, spec)
    u, s = (x.numpy().astype(float) for x in Cm.pixel_rays(spec))
    edge = (cc.ground_z(cfg) + 2.5 - (cc.ground_z(cfg) + 0.6)) / 6.0
    below_ground = (cc.ground_z(cfg) - (cc.ground_z(cfg) + 0.6)) / 6.0
    wall = (s < edge) & (s > below_ground)
    assert 0 < edge < s[0] and wall.any() and (~wall).any() and np.abs(s - edge).min() > 1e-3
    assert (got.seg[0][wall] == (Cm.HIT_WALL | 0 << 8 | Cm.FACE_SIDE_X << 16)).all()
    assert np.abs(got.depth[0][wall] - 6.0).max() <= 2e-6 * 6.0   # one depth: t * cj with t = D / cos and cj = cos, two roundings
    assert (got.seg[0][s > edge] == Cm.HIT_NONE).all()
    assert (got.seg[0][s < below_ground] == Cm.HIT_NONE).all()   # below the wall's foot, with the ground off
    assert (got.rgb[0][wall] == (60 * 224 >> 8,) * 3).all()


def test_cubes_tops_and_what_they_hide():
    """An item cube seen from above shows its TOP; from the side, its SIDE_X face.  In the maze, a marker post in front of the box hides
    the box only on the rows and columns it covers: beside and above it the box's face is seen.  (No kind has both cubes and the box --
    the cubes are the gather kinds', the box the maze kinds' -- so the low shape before the box is the 1 m post.)"""
    cfg, st, items, aux = gather_env(((0.0, 0.0), (0.0, 0.0)), ((3.0, 0.0), (3.0, 0.0)))
    high = cc.camera_host(cfg, st, items, aux, cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 1.3, Cm.FOOD | Cm.GROUND))
    kinds, index, face = (np.asarray(x) for x in Cm.decode(high.seg[0].astype(np.int64)))
    cube = kinds == Cm.HIT_FOOD
    assert cube.any() and (index[cube] == 0).all() and (face[cube] == Cm.FACE_TOP).any() and set(np.unique(face[cube])) <= {Cm.FACE_TOP, Cm.FACE_SIDE_X}
    top = cube & (face == Cm.FACE_TOP)
    u, s = (x.numpy().astype(float) for x in Cm.pixel_rays(cc.spec_of((64, 40), 0)))
    want = (0.225 - (cc.ground_z(cfg) + 1.3)) / s[:, None] * np.ones(64)   # depth of the plane z = 0.225
    assert np.abs(high.depth[0][top] - want[top]).max() <= 1e-5
    low = cc.camera_host(cfg, st, items, aux, cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 0.1, Cm.FOOD | Cm.GROUND))
    kinds, index, face = (np.asarray(x) for x in Cm.decode(low.seg[0].astype(np.int64)))
    assert (kinds == Cm.HIT_FOOD).any() and (face[kinds == Cm.HIT_FOOD] == Cm.FACE_SIDE_X).all()
    assert np.abs(low.depth[0][kinds == Cm.HIT_FOOD] - 2.875).max() <= 5e-6
    mcfg, mst, maux = maze_env(((-2.0, -8.0),))
    mst[:, 5], mst[:, 6] = np.sin(np.pi / 4), np.cos(np.pi / 4)   # heading +y: the box's y = -2 face is 6 m ahead
    mcfg.targets[0][0], mcfg.targets[0][1] = -2.0, -5.0            # the post 3 m ahead, 1 m tall
    spec = cc.spec_of((64, 40), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 0.6, Cm.BOX | Cm.TARGET | Cm.GROUND)
    got = cc.camera_host(mcfg, mst, None, maux, spec)
    kinds, index, face = (np.asarray(x) for x in Cm.decode(got.seg[0].astype(np.int64)))
    post = kinds == Cm.HIT_TARGET
    rows, cols = np.nonzero(post)
    assert post.any() and (face[post] == Cm.FACE_ROUND).all() and set(cols) == {30, 31, 32, 33}   # a radius of 0.2 m at 3 m: columns of 2 / 64 * 3 m = 0.094 m, centred 0.047 and 0.14 m off the axis
    top_row = rows.min()
    assert (kinds[top_row - 1, 30:34] == Cm.HIT_BOX).all() and (face[top_row - 1, 30:34] == Cm.FACE_SIDE_Y).all()   # above the post: the box's face again
    assert (kinds[top_row:rows.max() + 1, 29] != Cm.HIT_TARGET).all() and (kinds[top_row, 29] == Cm.HIT_BOX)
    assert np.abs(got.depth[0][kinds == Cm.HIT_BOX] - 6.0).max() <= 2e-5
    without = cc.camera_host(mcfg, mst, None, maux, cc.spec_of((64, 40), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 0.6, Cm.BOX | Cm.GROUND))
    assert np.array_equal(without.seg[0][~post], got.seg[0][~post]) and (without.seg[0][post] & 255 != Cm.HIT_TARGET).all()


def test_inside_ties_and_range():
    """An eye inside the box gives BOX | INSIDE << 16 at depth 0 everywhere.  Two cubes at the same place tie on every ray: the lower
    slot wins.  A shape beyond max_range is not drawn while the ground in front of it is."""
    cfg, st, aux = maze_env(((-2.0, 0.0),))
    got = cc.camera_host(cfg, st, None, aux, cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 0.6))
    assert (got.seg == (Cm.HIT_BOX | Cm.FACE_INSIDE << 16)).all() and (got.depth == 0).all() and (got.rgb == 170 * 128 >> 8).all()
    above = cc.camera_host(cfg, st, None, aux, cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_GROUND, 2.2))   # over the box's roof
    u, s = (x.numpy().astype(float) for x in Cm.pixel_rays(cc.spec_of((48, 24), 0)))
    roof = 0.205 / -s[18:]   # the depth at which the six lowest rows come down on the roof, 0.205 m under the eye: at most 0.76 m, inside the box's outline in every column
    assert (above.seg[0, 18:] == (Cm.HIT_BOX | Cm.FACE_TOP << 16)).all() and np.abs(above.depth[0, 18:] - roof[:, None]).max() <= 1e-5
    assert ((above.seg[0, :12] & 255) != Cm.HIT_BOX).all()   # nothing of the box above the horizon
    gcfg, gst, items, gaux = gather_env(((0.0, 0.0),), ((2.0, 0.3),))
    items[0, 2:4] = (2.0, 0.3)                                 # food item 1 on top of item 0
    items[0, 2 * gcfg.n_food:2 * gcfg.n_food + 2] = (2.0, 0.3)   # ... and the first poison cube
    tie = cc.camera_host(gcfg, gst, items, gaux, cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 0.6, Cm.FOOD | Cm.POISON | Cm.GROUND))
    kinds, index, _ = (np.asarray(x) for x in Cm.decode(tie.seg[0].astype(np.int64)))
    assert (kinds == Cm.HIT_FOOD).any() and (index[kinds == Cm.HIT_FOOD] == 0).all() and (kinds != Cm.HIT_POISON).all()
    only_poison = cc.camera_host(gcfg, gst, items, gaux, cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 0.6, Cm.POISON | Cm.GROUND))
    assert np.array_equal(only_poison.seg[0] & 255 == Cm.HIT_POISON, kinds == Cm.HIT_FOOD) and np.array_equal(only_poison.depth, tie.depth)
    # a cube resting on the ground plane's level ties with nothing; a cube 2 m away is not drawn at max_range 1.5 while the ground before it is
    short = cc.camera_host(gcfg, gst, items, gaux, cc.spec_of((64, 40), Cm.HRL_SCAN_WORLD, Cm.HRL_EYE_GROUND, 0.6, Cm.EVERYTHING, max_range=1.5))
    kinds = short.seg[0] & 255
    assert set(np.unique(kinds)) == {Cm.HIT_NONE, Cm.HIT_GROUND} and (short.depth[0][kinds == Cm.HIT_NONE] == np.float32(1.5)).all()
    assert (short.depth[0][kinds == Cm.HIT_GROUND] <= 1.5).all()


@pytest.mark.parametrize('kind', cc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range (field_cases.hostile): an env
    whose x or y is not finite sees nothing at all -- NONE, max_range and the sky on every pixel; a shape with a non-finite parameter is
    not seen -- the image equals, bit for bit, that of the clean twin without the shape.  A torso whose z is not finite is blind under
    HRL_EYE_TORSO and sees as ever under HRL_EYE_GROUND."""
    cfg, state, items, aux = shard(kind)
    for frame in cc.FRAMES:
        for size, eye_mode in (((48, 24), Cm.HRL_EYE_TORSO), ((128, 128), Cm.HRL_EYE_GROUND)):
            spec = cc.spec_of(size, frame, eye_mode, 0.6)
            for s, it, a, cs, cit, ca, far, blind in cc.hostile(cfg, state, items, aux):
                got = cc.camera_host(cfg, s, it, a, spec)
                want = cc.camera_host(cc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
                rows = [e for e in range(N) if e not in blind]
                assert cc.same(cc.Camera(*(x[rows] for x in got)), cc.Camera(*(x[rows] for x in want))), (kind, frame, size)
                b = list(blind)
                assert (got.seg[b] == 0).all() and (got.depth[b] == np.float32(spec.max_range)).all() and (got.rgb[b] == Cm.RGB_SKY).all()
                assert (want.seg != 0).any()
            for bad in (np.nan, np.inf, -np.inf):
                s = np.array(state)
                s[4, 2] = bad
                got, clean = cc.camera_host(cfg, s, items, aux, spec), cc.camera_host(cfg, state, items, aux, spec)
                assert cc.same(cc.Camera(*(x[:4] for x in got)), cc.Camera(*(x[:4] for x in clean)))
                if eye_mode == Cm.HRL_EYE_TORSO:
                    assert (got.seg[4] == 0).all() and (got.depth[4] == np.float32(spec.max_range)).all() and (got.rgb[4] == Cm.RGB_SKY).all()
                else:
                    assert all(np.array_equal(x[4], y[4]) for x, y in zip(cc.bits(got), cc.bits(clean)))


def test_an_env_does_not_depend_on_its_batch():
    """Env e of a shard of 5, alone in a shard of 1, and under a mask of its own: the same bytes; a masked env keeps its bytes; a NULL
    member is not written."""
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6)
    full = cc.camera_host(cfg, state, items, aux, spec)
    one = orc.default_config(K.HRL_ANT_GATHER, num_envs=1, seed=cfg.seed, auto_reset=1)
    for e in range(N):
        alone = cc.camera_host(one, state[e:e + 1], items[e:e + 1], aux[e:e + 1], spec)
        assert cc.same(alone, cc.Camera(*(x[e:e + 1] for x in full))), e
    out = cc.Camera(np.full((N, 24, 48), -3, np.float32), np.full((N, 24, 48), -7, np.int32), np.full((N, 24, 48, 3), 0x7B, np.uint8))
    cc.camera_host(cfg, state, items, aux, spec, mask=np.array([1, 0, 5, 0, 1], np.uint8), out=out)
    for e in range(N):
        if e in (1, 3):
            assert (out.depth[e] == -3).all() and (out.seg[e] == -7).all() and (out.rgb[e] == 0x7B).all()
        else:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(cc.bits(out), cc.bits(full)))
    for want in (('depth',), ('seg',), ('rgb',), ('depth', 'rgb')):
        part = cc.camera_host(cfg, state, items, aux, spec, want=want)
        assert all((x is None) == (name not in want) and (x is None or np.array_equal(x, y)) for name, x, y in zip(cc.NAMES, cc.bits(part), cc.bits(full)))


def test_shades_and_unprojection():
    """shade_rgb equals the header's table for every class and face; eye + depth * (forward + u left + s up) lies on the surface seen."""
    for cls, col in list(cc.COLOURS.items()) + [(0, Cm.RGB_SKY)]:
        for face in range(7):
            word = cc.lib().camera_shade_rgb(cls | face << 16)
            k = Cm.SHADES[face] if cls else 256
            assert (word & 255, word >> 8 & 255, word >> 16 & 255, word >> 24) == (col[0] * k >> 8, col[1] * k >> 8, col[2] * k >> 8, 0)
    cfg, st, aux = maze_env(((3.0, -6.0),))
    st[:, 5], st[:, 6] = np.sin(1.0), np.cos(1.0)   # a yaw of 2 rad
    spec = cc.spec_of((64, 40), Cm.HRL_SCAN_HEADING, Cm.HRL_EYE_TORSO, 0.6, Cm.WALL | Cm.BOX | Cm.GROUND)
    got = cc.camera_host(cfg, st, None, aux, spec)
    u, s = (x.numpy().astype(float) for x in Cm.pixel_rays(spec))
    f = np.array([np.cos(2.0), np.sin(2.0)])
    eye = np.array([3.0, -6.0, 0.55 + 0.6])
    P = eye + got.depth[0][..., None] * np.dstack([f[0] - u[None, :] * f[1] + 0 * s[:, None], f[1] + u[None, :] * f[0] + 0 * s[:, None], s[:, None] + 0 * u[None, :]])
    kinds, index, face = (np.asarray(x) for x in Cm.decode(got.seg[0].astype(np.int64)))
    assert np.abs(P[..., 2][kinds == Cm.HIT_GROUND] - cc.ground_z(cfg)).max() <= 1e-4
    for k, (axis, value) in enumerate(((0, 5.0), (0, -5.0), (1, 9.0), (1, -9.0))):
        sel = (kinds == Cm.HIT_WALL) & (index == k) & (face != Cm.FACE_TOP)
        assert not sel.any() or np.abs(P[..., axis][sel] - value).max() <= 1e-4, k
    assert (kinds == Cm.HIT_WALL).any() and (kinds == Cm.HIT_GROUND).any()


SPEC_BAD = [('width', 0), ('width', 24), ('width', 144), ('height', 4), ('height', 12), ('height', 136), ('frame', 2), ('frame', -1), ('eye_mode', 2), ('eye_mode', -1),
            ('eye_height', -0.1), ('eye_height', 10.5), ('eye_height', float('nan')), ('tan_half_h', 1e-3), ('tan_half_h', 2e3), ('tan_half_h', float('nan')), ('tan_half_h', float('inf')),
            ('tan_half_v', 0.0), ('tan_half_v', -1.0), ('tan_half_v', float('nan')), ('max_range', 0.0), ('max_range', -1.0), ('max_range', float('inf')), ('max_range', float('nan')),
            ('classes', 0), ('classes', 32), ('classes', 128 | 1), ('struct_size', 16), ('struct_size', 0), ('out', 'empty'), ('out', 'null')]
REASONS = {'width': 'camera width must be a multiple of 16 within 16..128', 'height': 'camera height must be a multiple of 8 within 8..128', 'frame': 'unknown camera frame',
           'eye_mode': 'unknown camera eye_mode', 'eye_height': 'camera eye_height must be finite and within 0..10', 'tan_half_h': 'camera tan_half_h must be finite and within (1e-3, 1e3]',
           'tan_half_v': 'camera tan_half_v must be finite and within (1e-3, 1e3]', 'max_range': 'camera max_range must be finite and positive',
           'classes': 'camera classes must be a non-empty mask of', 'struct_size': 'struct_size is not sizeof', 'empty': 'camera out holds no pointer: at least one output must be given',
           'null': 'null camera out'}


@pytest.mark.parametrize('field,value', SPEC_BAD)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = cc.spec_of((48, 24), Cm.HRL_SCAN_HEADING)
    out = cc.Camera(np.full((N, 128, 128), -3, np.float32), np.full((N, 128, 128), -7, np.int32), np.full((N, 128, 128, 3), 0x7B, np.uint8))
    if field != 'out':
        setattr(spec, field, value)
    b = K.make_buffers(cc.ptr(state), cc.ptr(items), cc.ptr(aux), None, None, None, None, None)
    o = Cm.hrl_camera_out(**({} if value == 'empty' else {name: cc.ptr(a) for name, a in zip(cc.NAMES, out)}))
    ref = None if value == 'null' else C.byref(o)
    code = cc.lib().camera_host(C.byref(cfg), C.byref(b), C.byref(spec), None, ref)
    why = cc.lib().camera_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and REASONS[value if field == 'out' else field] in why, why
    untouched = lambda: (out.depth == -3).all() and (out.seg == -7).all() and (out.rgb == 0x7B).all()
    assert untouched()
    # the device library runs the same checks before it looks for a device
    L = Cm.lib()
    assert L.hrl_camera(C.byref(cfg), C.byref(b), C.byref(spec), None, ref, None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_camera_last_error() == b'hrl_camera: ' + why.encode()
    assert untouched()


def test_default_spec_and_the_mirrors():
    for kind in cc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, frame in Cm.FRAMES.items():
            s, h, r = Cm.default_spec(cfg, name), Cm.hrl_camera_spec(), S.default_spec(cfg)
            assert cc.lib().camera_host_default_spec(C.byref(cfg), frame, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.width, s.height, s.frame, s.eye_mode, s.tan_half_h, s.tan_half_v) == (C.sizeof(Cm.hrl_camera_spec), 64, 48, frame, Cm.HRL_EYE_TORSO, 1.0, 0.75)
            assert s.eye_height == np.float32(0.4 if kind == K.HRL_POINT_GATHER else 0.3) and s.max_range == r.max_range and s.classes == Cm.ALL | Cm.GROUND == 95
            assert cc.lib().camera_validate_spec(C.byref(s)) == b''
    s = Cm.default_spec(cfg, 'world', 128, 64, hfov_degrees=60, eye='ground', eye_height=1.5, max_range=6.0, classes=Cm.WALL | Cm.GROUND)
    assert (s.width, s.height, s.frame, s.eye_mode, s.eye_height, s.max_range, s.classes) == (128, 64, 0, Cm.HRL_EYE_GROUND, 1.5, 6.0, 65)
    assert s.tan_half_h == np.float32(np.tan(np.pi / 6)) and s.tan_half_v == np.float32(np.tan(np.pi / 6) * 64 / 128)   # float64, rounded once
    assert Cm.default_spec(cfg, vfov_degrees=90).tan_half_v == np.float32(np.tan(np.pi / 4))
    with pytest.raises(ValueError):
        Cm.default_spec(cfg, 'sideways')
    with pytest.raises(ValueError):
        Cm.default_spec(cfg, eye='hip')
    assert cc.lib().camera_sizeof_spec() == C.sizeof(Cm.hrl_camera_spec) == 48 and cc.lib().camera_sizeof_out() == C.sizeof(Cm.hrl_camera_out) == 24
    assert Cm.Camera() == (None,) * 3 and Cm.Camera._fields == cc.NAMES
    u, v = Cm.pixel_rays(s)
    assert u.dtype == v.dtype and tuple(u.shape) == (128,) and tuple(v.shape) == (64,) and float(u[0]) == -float(u[-1]) > 0 and float(v[0]) == -float(v[-1]) > 0
    hdr = open(os.path.join(cc.ROOT, 'include', 'hrl_camera.h')).read()
    for name, value in (('HRL_CAMERA_GROUND', Cm.GROUND), ('HRL_HIT_GROUND', Cm.HIT_GROUND), ('HRL_FACE_TOP', Cm.FACE_TOP), ('HRL_FACE_GROUND', Cm.FACE_GROUND),
                        ('HRL_EYE_TORSO', Cm.HRL_EYE_TORSO), ('HRL_CAMERA_MAX_SIZE', Cm.MAX_SIZE)):
        assert int(re.search(rf'#define {name} (\d+)', hdr).group(1)) == value
    assert re.search(r'#define HRL_RGB_SKY (\d+), (\d+), (\d+)', hdr).groups() == tuple(str(x) for x in Cm.RGB_SKY)


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """camera_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the images of every kind in both frames
    from reset-like and hostile states, and holds span_* to scan::isect_* bit for bit over 2 x 4096 rays: exit status 0,
    sizeof(hrl_camera_spec) == the ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([cc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_camera_spec {C.sizeof(Cm.hrl_camera_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = cc.lib().camera_check_n_cases()
    assert n == len(sums) == 6 * 2 * 7 + 2 and 'spans0' in sums and 'spans1' in sums
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert cc.lib().camera_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different images


def test_camera_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_camera_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the kernel and an LDS footprint of at most 8 KB; the header's symbols are SYMBOLS; the camera is an entry of build.py of
    its own, built by build() after the frontier map."""
    code = 'from hrl_pybullet_envs_amd.build import build_camera, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_camera(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=cc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(cc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_camera_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*camera_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 8192
    hdr = open(os.path.join(cc.ROOT, 'include', 'hrl_camera.h')).read()
    assert set(re.findall(r'\b(hrl_camera(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_camera_out', 'hrl_camera_spec'} == set(Cm.SYMBOLS)
    for s in Cm.SYMBOLS:
        assert hasattr(Cm.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.CAMERA == ('camera', 'libhrl_camera_hip.so', 'camera_hip.hip', 'camera_core.h', 'hrl_camera.h') and 'camera' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_frontier(force, verbose)\n    build_camera(force, verbose)') > 0
