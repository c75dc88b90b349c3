"""The batched closest points' specification (csrc/closest_core.h) on the CPU: its host build (tests/closest_host) against an independent
fp64 reference written from include/hrl_closest.h alone (tests/closest_cases.py), by certificate; against the step's own contacts (the
emulator's contact records); known answers on hand-made poses; totality on hostile states; the sanitised stand-alone program and the
gfx950 cross-compile.  No GPU."""
import collections
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as hc
import contacts_cases as cs
import orc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import closest_device as Cl
from test_camera_host import gather_env
from test_chase_host import standing_ant
from test_field_host import maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
# The worst figures of the certificate over the two sweeps below (the six default shards and sensor_configs.MATRIX, each as it is and with
# the robots spread), measured against the fp64 reference (the printed lines); the tolerances are four times these.
DIST_WORST = 6.07e-7     # metres: |distance - the fp64 gap of the surface named by which| (gather-nofood, spread)
POINT_WORST = 7.16e-7    # metres: on_link / on_surface off their surfaces, ||on_link - on_surface| - |distance|| (maze-12, spread)
NORMAL_WORST = 4.27e-6   # |normal -+ (on_link - on_surface) / |...||, per component (gather-nofood, spread)
DIST_TOL, POINT_TOL, NORMAL_TOL = 4 * DIST_WORST, 4 * POINT_WORST, 4 * NORMAL_WORST
TOL = (DIST_TOL, POINT_TOL, NORMAL_TOL)
CONTACT_TOL = 1e-5       # metres: contacts_cases.check_geometry's tolerance


def sweep(cfg, state, items, aux, tag):
    worst, seen = dict(a=0.0, b=0.0, c=0.0, d=0.0), collections.Counter()
    for label, st in (('shard', state), ('spread', hc.spread(cfg, state))):
        got = hc.closest_host(cfg, st, items, aux)
        w, n = hc.certificate(cfg, st, items, got, tol=TOL, where=(tag, label))
        print(f'{tag} {label}: distance {w["a"]:.3e} m, lead of the named surface {w["b"]:.3e} m, points {w["c"]:.3e} m, normal {w["d"]:.3e}; finite cells {dict(n)}')
        worst = {k: max(worst[k], w[k]) for k in worst}
        seen.update(n)
    return worst, seen


@pytest.mark.parametrize('kind', hc.KINDS)
def test_host_build_holds_the_fp64_certificate(kind):
    """The six default shards, as they are and with the robots spread about the arena (probe_cases.spread: one leans into the maze box).
    On EVERY finite cell, with no exemption:
      (a) |distance - the fp64 gap of the surface named by which| <= DIST_TOL where the fp64 axis gap is positive; where the axis meets
          the solid, distance <= -r + DIST_TOL;
      (b) the fp64 gap of the named surface is within DIST_TOL of the fp64 minimum over the class;
      (c) on_link lies on the link's surface and on_surface on the other shape's within POINT_TOL, and |on_link - on_surface| equals
          |distance| within POINT_TOL.  WHERE THE AXIS RUNS THROUGH A BOX the header's on_link = x - r n lies on the sphere of radius r
          about the axis point x that stands in for the capsule (as in the step), which is the capsule's surface only if the face's normal
          is square to the axis: there on_link is held to that sphere about the fp64 middle of the stretch, at the same tolerance
          (closest_cases.on_shape) -- measured before this was written: 7.0e-2 m off the capsule's surface on the maze's leaning robot;
      (d) where |distance| >= 1e-3, normal = sign(distance) (on_link - on_surface) / |...| within NORMAL_TOL; its length is 1 within 1e-6.
    Every class that has a surface reports a finite cell for every link; which is NONE exactly where distance is +inf.

    Measured over this sweep and the matrix's: (a) 6.07e-7 m, (b) 1.9e-9 m, (c) 7.16e-7 m, (d) 4.27e-6."""
    cfg, state, items, aux = shard(kind)
    worst, seen = sweep(cfg, state, items, aux, f'kind {kind}')
    B = hc.n_links(cfg)
    assert seen[hc.GROUND] == 2 * N * B and (kind == K.HRL_POINT_GATHER or seen[hc.SELF] == 2 * N * 12)
    assert (seen[hc.WALL] > 0) == (kind != K.HRL_ANT_FLAT) and (seen[hc.BOX] > 0) == (kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ))
    assert (seen[hc.FOOD] > 0) == (seen[hc.POISON] > 0) == (kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER))


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_holds_the_fp64_certificate_on_the_sensor_config_matrix(name):
    """The certificate above, with its tolerances, on every entry of sensor_configs.MATRIX; gather-64 and point-64 name items past 47."""
    cfg, state, items, aux = scfg.shard(name)
    sweep(cfg, state, items, aux, name)
    got = hc.closest_host(cfg, state, items, aux)
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(got.which)
    if name == 'flagrun-open':    # no lateral plane at all
        assert (got.distance[:, :, hc.WALL] == np.inf).all() and (got.which[:, :, hc.WALL] == Cl.HIT_NONE).all()
    if name == 'gather-nofood':   # every item is poison
        assert (got.distance[:, :, hc.FOOD] == np.inf).all() and (got.which[:, :, hc.FOOD] == Cl.HIT_NONE).all()
        assert np.isfinite(got.distance[:, :, hc.POISON]).all() and (got.which[:, :, hc.POISON] & 255 == Cl.HIT_POISON).all()


# ------------------------------------------------------------------------------------------------ the step's own contacts
FLOORS = {'items': {'food': 30, 'poison': 30}, 'walls': {'wall': 25}, 'box': {'box': 50, 'ground': 100}, 'self': {'self': 20}, 'cubes_under_the_feet': {'food': 8},
          'foot_across_the_maze_corner': {'box': 40, 'wall': 40}, 'feet_flat_against_the_maze_box': {'box': 80}, 'feet_flat_on_cubes': {'food': 60}}


@pytest.mark.parametrize('name', ('items', 'walls', 'box', 'self') + cs.CAPSULE)
def test_a_pair_the_step_holds_in_contact_reports_the_steps_distance(name):
    """The scenarios of tests/contacts_cases.py with frame_skip = 1, so the record's collision pass is at the step's input pose.  For
    every contact of the emulator's record the cell of that link and class at the input state names a surface whose distance is at most
    the record's + 1e-5 m, and equals the record's within 1e-5 m where which names the contact's surface.  A link code `level | leg << 2`
    names a link by closest_cases.links_of_code; code 0 is the torso's sphere or leg 0's hip capsule, and one of the two must hold.  A
    self contact is held against the cells of both of its links.

    Two properties of the record decide what can be asked of a contact, both read off the reference alone:
      * against a plane the step's contact of a link is the sphere at the link's FAR end p1; the cell is the lower of both ends (the
        header).  Where fp64 kinematics put the near end p0 lower than p1, the cell is below the record's distance and equality is not
        asked (counted as `near_end`; measured: the robots of foot_across_the_maze_corner that stand in a wall, up to 0.34 m);
      * a second support point (a later contact of the same link and surface) is a manifold point, not the pair's closest point.
        Where the pair's first contact is at -r or less (the axis runs through the solid, where the step takes the middle of the
        stretch) the second point may lie deeper than the first, and it is not compared (counted as `deep_second`; measured: 4 contacts
        of scenario `box`, up to 0.21 m); every other second point is held to the `at most` clause.
    Floors on the contacts compared per class are asserted."""
    tr = cs.trace(name, frame_skip=1)
    rec = cs.emu_records(name, frame_skip=1)
    cfg = tr.cfg
    n = collections.Counter()
    for t, s in enumerate(tr.steps):
        got = hc.closest_host(cfg, s['state'], s['items'], s['aux'])
        for i in range(cfg.num_envs):
            first, segs = {}, hc.link_segments(s['state'][i])
            for k in range(int(rec[t, i, 0])):
                c = cs.contact(rec[t, i], k)
                dist, surf, link, link2 = float(c[3]), int(c[16]), int(c[17]), int(c[18])
                w = (name, t, i, k)
                if link2 >= 0:
                    a, b = hc.links_of_code(link, True)[0], hc.links_of_code(link2, True)[0]
                    for mine, other in ((a, b), (b, a)):
                        d, which = float(got.distance[i, mine, hc.SELF]), int(got.which[i, mine, hc.SELF])
                        assert d <= dist + CONTACT_TOL, (w, mine, d, dist)
                        assert which != hc.word_of(hc.SELF, other) or abs(d - dist) <= CONTACT_TOL, (w, mine, d, dist)
                    n['self'] += 1
                    continue
                cls, idx = hc.class_of_surface(cfg, surf)
                second = (link, surf) in first
                if second and first[(link, surf)] <= -hc.R_CAPS:
                    n['deep_second'] += 1
                    continue
                first.setdefault((link, surf), dist)
                held = False
                for l in hc.links_of_code(link):
                    d, which = float(got.distance[i, l, cls]), int(got.which[i, l, cls])
                    equal = second or which != hc.word_of(cls, idx) or abs(d - dist) <= CONTACT_TOL
                    if not equal and cls in (hc.GROUND, hc.WALL):
                        _, _, plane_n, plane_d = [x for x in hc.surfaces(cfg, s['items'][i])[cls] if x[0] == idx][0]
                        p0, p1, _ = segs[l]
                        if plane_n @ p0 < plane_n @ p1:
                            equal = True
                            n['near_end'] += 1
                    held = held or (d <= dist + CONTACT_TOL and equal)
                assert held, (w, link, surf, dist, [(float(got.distance[i, l, cls]), int(got.which[i, l, cls])) for l in hc.links_of_code(link)])
                n[Cl.CLASS_NAMES[cls]] += 1
    print(name, dict(n))
    for cls, floor in FLOORS[name].items():
        assert n[cls] >= floor, (name, dict(n))


# ------------------------------------------------------------------------------------------------ known answers
def cell(got, link, cls, e=0):
    return float(got.distance[e, link, cls]), int(got.which[e, link, cls]), got.on_link[e, link, cls].astype(float), got.on_surface[e, link, cls].astype(float), got.normal[e, link, cls].astype(float)


def test_a_level_ants_feet_over_the_ground():
    """A level ant with straight legs at height z: every link's axis lies at z, so each foot's ground distance is z - ground_z - 0.08 and
    the torso's z - ground_z - 0.25, the normal (0, 0, 1), on_surface on the plane under the end that won (a tie: the far end p1, the
    tip).  With the ankles bent by 1 rad the feet point down and the tips are 0.4 sqrt 2 sin 1 lower."""
    for z in (0.55, 0.75, 0.05):
        cfg, st, items, aux = standing_ant(z=z, xy=(0.5, -0.25), yaw=0.7)
        gz = hc.ground_z(cfg)
        got = hc.closest_host(cfg, st, items, aux)
        tips = {link: p1 for link, (_, p1, _) in enumerate(hc.link_segments(st[0]))}
        for foot in (2, 4, 6, 8):
            d, which, a, b, n = cell(got, foot, hc.GROUND)
            assert abs(d - (z - gz - 0.08)) <= DIST_TOL and which == Cl.HIT_GROUND and tuple(n) == (0.0, 0.0, 1.0)
            assert np.abs(a - (tips[foot] - (0, 0, 0.08))).max() <= POINT_TOL and np.abs(b - (tips[foot][0], tips[foot][1], gz)).max() <= POINT_TOL
        assert abs(got.distance[0, 0, hc.GROUND] - (z - gz - 0.25)) <= DIST_TOL
        assert (got.distance[0, :, 1:5] == np.inf).all() and (got.which[0, :, 1:5] == Cl.HIT_NONE).all() and not got.normal[0, :, 1:5].any()   # the flat kind: ground and self alone
        st[0, 8:15:2] = (1.0, -1.0, -1.0, 1.0)
        got = hc.closest_host(cfg, st, items, aux)
        for foot in (2, 4, 6, 8):
            assert abs(got.distance[0, foot, hc.GROUND] - (z - 0.4 * math.sqrt(2) * math.sin(1.0) - gz - 0.08)) <= DIST_TOL


def test_a_foot_tip_by_a_wall():
    """The gather arena's +x plane is the wall's inner face at 7.45.  A level ant at x = 6.35 has leg 0's foot tip at x = 7.15, 0.3 m
    from it: distance 0.3 - 0.08, plane 0, the inward normal (-1, 0, 0), on_surface on the plane."""
    cfg, st, items, aux = standing_ant(z=0.55, xy=(6.35, 0.0), kind=K.HRL_ANT_GATHER)
    d, which, a, b, n = cell(hc.closest_host(cfg, st, items, aux), 2, hc.WALL)
    assert abs(d - 0.22) <= DIST_TOL and which == (Cl.HIT_WALL | 0 << 8) and tuple(n) == (-1.0, 0.0, 0.0)
    assert np.abs(a - (7.23, 0.8, 0.55)).max() <= POINT_TOL and np.abs(b - (7.45, 0.8, 0.55)).max() <= POINT_TOL
    cfg, st, items, aux = standing_ant(z=0.55, xy=(0.0, -6.35), kind=K.HRL_ANT_GATHER)   # leg 2 points to (-1, -1): the -y wall is plane 3
    d, which, a, b, n = cell(hc.closest_host(cfg, st, items, aux), 6, hc.WALL)
    assert abs(d - 0.22) <= DIST_TOL and which == (Cl.HIT_WALL | 3 << 8) and tuple(n) == (0.0, 1.0, 0.0)


def test_a_cube_under_a_foot():
    """Food cube 0 under the middle of leg 0's level foot: the cube's top is at 0.225, the distance z - 0.225 - 0.08, the normal (0, 0, 1),
    and -- the axis runs alongside the face -- the points lie under the middle of the stretch over the cube."""
    cfg, st, items, aux = gather_env(((1.0, 2.0),), ((1.6, 2.6),), z=0.5)
    got = hc.closest_host(cfg, st, items, aux)
    d, which, a, b, n = cell(got, 2, hc.FOOD)
    assert abs(d - (0.5 - 0.225 - 0.08)) <= DIST_TOL and which == (Cl.HIT_FOOD | 0 << 8) and tuple(n) == (0.0, 0.0, 1.0)
    assert np.abs(a - (1.6, 2.6, 0.42)).max() <= POINT_TOL and np.abs(b - (1.6, 2.6, 0.225)).max() <= POINT_TOL
    assert (got.which[0, :, hc.POISON] >> 8 >= cfg.n_food).all()   # the poison cubes stand far away and are still named
    st[0, 2] = 0.25   # the foot's sphere reaches into the cube, the axis does not
    d, which, a, b, n = cell(hc.closest_host(cfg, st, items, aux), 2, hc.FOOD)
    assert abs(d - (0.25 - 0.225 - 0.08)) <= DIST_TOL and d < 0 and tuple(n) == (0.0, 0.0, 1.0) and abs(a[2] - 0.17) <= POINT_TOL and abs(b[2] - 0.225) <= POINT_TOL


def test_an_axis_through_the_maze_box():
    """A level ant at (1.3, 0) by the maze box's +x face (x = 1): leg 1's foot (0.9, 0.4) - (0.5, 0.8) lies inside the box, the middle of
    the stretch is 0.3 m behind the face: distance -0.3 - 0.08 and the face's normal (1, 0, 0); its aux body (1.1, 0.2) - (0.9, 0.4)
    crosses the face half way: the middle of the stretch is 0.05 m in: -0.05 - 0.08."""
    cfg, st, aux = maze_env(((1.3, 0.0),))
    got = hc.closest_host(cfg, st, None, aux)
    d, which, a, b, n = cell(got, 4, hc.BOX)
    assert abs(d + 0.38) <= DIST_TOL and which == Cl.HIT_BOX and tuple(n) == (1.0, 0.0, 0.0)
    assert np.abs(a - (0.62, 0.6, 0.55)).max() <= POINT_TOL and np.abs(b - (1.0, 0.6, 0.55)).max() <= POINT_TOL
    d, which, a, b, n = cell(got, 3, hc.BOX)
    assert abs(d + 0.13) <= DIST_TOL and tuple(n) == (1.0, 0.0, 0.0) and np.abs(b - (1.0, 0.35, 0.55)).max() <= POINT_TOL
    d, which, a, b, n = cell(got, 0, hc.BOX)   # the torso's sphere: 0.3 m from the face
    assert abs(d - 0.05) <= DIST_TOL and tuple(n) == (1.0, 0.0, 0.0)
    assert (got.distance[0, :, hc.FOOD:hc.POISON + 1] == np.inf).all()


def test_two_legs_folded_towards_each_other():
    """Legs 0 and 1 turned towards each other about their hips: every capsule's self cell names a link of another leg, the two links of
    the nearest pair of all name each other with THE SAME distance to the bit (the pair is evaluated in the step's order), opposite normals
    and each other's points; the distance equals the fp64 segment - segment distance - 0.16."""
    cfg, st, items, aux = standing_ant(z=1.0)
    st[0, 7], st[0, 9] = 0.6, -0.6
    got = hc.closest_host(cfg, st, items, aux)
    segs = hc.link_segments(st[0])
    for link in range(1, 13):
        d, which, a, b, n = cell(got, link, hc.SELF)
        other = which >> 8
        assert which & 255 == Cl.HIT_ROBOT and other in hc.self_pairs(link)
        want = min(hc.seg_seg(*segs[link][:2], *segs[o][:2]) for o in hc.self_pairs(link)) - 0.16
        assert abs(d - want) <= DIST_TOL, (link, d, want)
    mine = 1 + int(np.argmin(got.distance[0, 1:, hc.SELF]))   # a link of the nearest pair of all
    d2, w2, a2, b2, n2 = cell(got, mine, hc.SELF)
    other = w2 >> 8
    d4, w4, a4, b4, n4 = cell(got, other, hc.SELF)
    assert w4 == (Cl.HIT_ROBOT | mine << 8) and np.float32(d2).view(np.uint32) == np.float32(d4).view(np.uint32)
    assert np.array_equal(n2, -n4) and np.abs(a2 - b4).max() <= POINT_TOL and np.abs(b2 - a4).max() <= POINT_TOL
    neutral = hc.closest_host(*standing_ant(z=1.0))
    for foot in (2, 4):   # the folded legs' feet are nearer to another leg than with the legs as they were
        assert got.distance[0, foot, hc.SELF] < neutral.distance[0, foot, hc.SELF] - 0.05 and hc.leg_of(int(got.which[0, foot, hc.SELF]) >> 8)[0] in (0, 1)
    assert (got.distance[0, 0, hc.SELF] == np.inf) and got.which[0, 0, hc.SELF] == Cl.HIT_NONE   # the torso has no self class


def test_the_point_bot_on_the_ground_by_a_cube():
    """The cube upright with its bottom on the ground: ground distance 0 at the first corner, normal (0, 0, 1).  Food cube 0 with its
    near face 0.2 m from the player's +x face: the cube's corner (0.55, -0.125, -0.025..0.225) against the player's box gives 0.2 with
    the normal (-1, 0, 0) towards the player; the player's own corners are farther (0.301 m).  No box class, no self class."""
    cfg = orc.default_config(K.HRL_POINT_GATHER, num_envs=1)
    gz = hc.ground_z(cfg)
    st = np.zeros((1, K.HRL_STATE_STRIDE), np.float32)
    st[0, 2], st[0, 6] = gz + 0.35, 1.0
    items = np.full((1, orc.items_stride(cfg)), 100.0, np.float32)
    items[0, 0:2] = (0.675, 0.0)
    got = hc.closest_host(cfg, st, items, np.zeros((1, K.HRL_AUX_STRIDE), np.int32))
    d, which, a, b, n = cell(got, 0, hc.GROUND)
    assert abs(d) <= DIST_TOL and which == Cl.HIT_GROUND and tuple(n) == (0.0, 0.0, 1.0) and np.abs(a - (-0.35, -0.35, gz)).max() <= POINT_TOL
    d, which, a, b, n = cell(got, 0, hc.FOOD)
    assert abs(d - 0.2) <= DIST_TOL and which == (Cl.HIT_FOOD | 0 << 8) and np.abs(n - (-1.0, 0.0, 0.0)).max() <= NORMAL_TOL
    assert abs(a[0] - 0.35) <= POINT_TOL and abs(b[0] - 0.55) <= POINT_TOL and np.abs(a[1:] - b[1:]).max() <= POINT_TOL
    d, which, a, b, n = cell(got, 0, hc.WALL)
    assert abs(d - (7.45 - 0.35)) <= DIST_TOL * 8 and which & 255 == Cl.HIT_WALL   # (a number of 7 m carries 4.8e-7 m)
    assert got.distance[0, 0, hc.BOX] == np.inf and got.distance[0, 0, hc.SELF] == np.inf
    assert got.distance.shape == (1, 1, 6)


def test_classes_that_are_not_asked_for_report_nothing():
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    full = hc.closest_host(cfg, state, items, aux)
    for cls, bit in enumerate(Cl.CLASS_BITS):
        got = hc.closest_host(cfg, state, items, aux, hc.spec_of(bit))
        for k in range(6):
            if k == cls:
                assert all(np.array_equal(x[:, :, k], y[:, :, k]) for x, y in zip(hc.bits(got), hc.bits(full)))
            else:
                assert (got.distance[:, :, k] == np.inf).all() and (got.which[:, :, k] == 0).all() and not got.on_link[:, :, k].any() and not got.normal[:, :, k].any()
    hc.certificate(cfg, state, items, hc.closest_host(cfg, state, items, aux, hc.spec_of(Cl.GROUND | Cl.FOOD)), classes=Cl.GROUND | Cl.FOOD, tol=TOL)
    assert (hc.closest_host(cfg, state, None, aux).distance[:, :, hc.FOOD:hc.POISON + 1] == np.inf).all()   # no items record: no items


# ------------------------------------------------------------------------------------------------ totality
NAN_BITS = 0x7FC00000


def assert_contract(got, tag):
    for name, x in zip(hc.NAMES, got):
        if x.dtype == np.float32:
            ok = np.isfinite(x) | (x == np.inf) | (x.view(np.uint32) == NAN_BITS)
            assert ok.all(), (tag, name, x[~ok][:4])
    assert np.isfinite(got.distance[got.which != 0]).all() and (got.distance[got.which == 0] == np.inf).all(), tag
    none = got.which == 0
    assert not got.on_link[none].any() and not got.on_surface[none].any() and not got.normal[none].any(), tag
    assert ((got.which & 255) == np.where(none, 0, np.array(Cl.CLASS_HITS)[None, None, :])).all(), tag


def check_hostile(cfg, cases, state, items, aux, tag):
    """Every output is finite, +inf or the one quiet NaN; which is NONE exactly where distance is +inf; an env whose records the case
    leaves alone answers as in the clean shard, bit for bit; an env without a finite place reports nothing at all."""
    clean = hc.closest_host(cfg, state, items, aux)
    for k, (s, it, a, *_rest) in enumerate(cases):
        got = hc.closest_host(cfg, s, it, a)
        assert_contract(got, (tag, k))
        for e in range(N):
            untouched = np.array_equal(s[e].view(np.uint32), state[e].view(np.uint32)) and (items is None or np.array_equal(it[e].view(np.uint32), items[e].view(np.uint32)))
            if untouched:
                assert all(np.array_equal(x[e], y[e]) for x, y in zip(hc.bits(got), hc.bits(clean))), (tag, k, e)
            if not np.isfinite(s[e, 0:3]).all():
                assert (got.which[e] == 0).all(), (tag, k, e)


@pytest.mark.parametrize('name', scfg.NAMES)
def test_hostile_states_get_the_contract_on_the_sensor_config_matrix(name):
    cfg, state, items, aux = scfg.shard(name)
    check_hostile(cfg, scfg.hostile(name, hc.hostile), state, items, aux, name)


@pytest.mark.parametrize('kind', hc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """The camera's hostile states (NaN, +-inf and 1e20 in the robot's position and the items), then NaN, +-inf and 1e20 in the height,
    each component of the quaternion and each joint angle of env 2: the contract; a non-finite height takes every cell of
    the env, a non-finite quaternion every capsule's and the cube's (the torso is a sphere about O), a non-finite ankle angle the foot's cells alone, a non-finite hip angle the aux body's and the foot's; the other envs are
    unchanged.  An item with a non-finite or huge coordinate is no candidate: the cell names another item, as the clean twin without it
    does."""
    cfg, state, items, aux = shard(kind)
    check_hostile(cfg, hc.hostile(cfg, state, items, aux), state, items, aux, kind)
    clean = hc.closest_host(cfg, state, items, aux)
    B = hc.n_links(cfg)
    for bad in (np.nan, np.inf, -np.inf, 1e20):
        for at in [2, 3, 4, 5, 6] + ([] if B == 1 else list(range(7, 15))):
            s = np.array(state)
            s[2, at] = bad
            got = hc.closest_host(cfg, s, items, aux)
            assert_contract(got, (kind, bad, at))
            rows = [0, 1, 3, 4]
            assert all(np.array_equal(x[rows], y[rows]) for x, y in zip(hc.bits(got), hc.bits(clean)))
            if not np.isfinite(bad) and at < 7:   # (the torso is a sphere about O: the quaternion is nothing to it)
                gone = slice(None) if at == 2 or B == 1 else slice(1, None)
                assert (got.which[2, gone] == 0).all() and (at == 2 or B == 1 or (got.which[2, 0, hc.GROUND] != 0)), (kind, bad, at)
            if not np.isfinite(bad) and at >= 7:
                leg, ankle = (at - 7) // 2, (at - 7) % 2
                lost = [2 + 2 * leg] if ankle else [1 + 2 * leg, 2 + 2 * leg]
                kept = [l for l in range(B) if l not in lost]
                assert (got.which[2, lost] == 0).all() and (got.which[2, kept, hc.GROUND] != 0).all(), (kind, bad, at)
                scene = slice(hc.GROUND, hc.POISON + 1)   # (the lost links leave the others' self class too)
                assert all(np.array_equal(x[2, kept, scene], y[2, kept, scene]) for x, y in zip(hc.bits(got), hc.bits(clean)))
    if items is not None and kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
        for bad in (np.nan, np.inf, -np.inf, 1e20):
            it, twin = np.array(items), np.array(items)
            named = int(clean.which[1, 0, hc.FOOD]) >> 8
            it[1, 2 * named] = bad
            twin[1, 2 * named:2 * named + 2] = (100.0, 0.0)
            got, want = hc.closest_host(cfg, state, it, aux), hc.closest_host(cfg, state, twin, aux)
            assert_contract(got, (kind, bad, 'item'))
            assert (got.which[1, :, hc.FOOD] >> 8 != named).all() and hc.same(got, want)


def test_an_env_does_not_depend_on_its_batch():
    """Env e of a shard of 5, alone in a shard of 1: the same bytes; a masked env keeps its bytes; a NULL member is not written."""
    for kind in (K.HRL_ANT_GATHER, K.HRL_ANT_MAZE, K.HRL_POINT_GATHER):
        cfg, state, items, aux = shard(kind)
        one_cfg = orc.default_config(kind, num_envs=1, seed=cfg.seed, auto_reset=1)
        full = hc.closest_host(cfg, state, items, aux)
        for e in range(N):
            alone = hc.closest_host(one_cfg, state[e:e + 1], None if items is None else items[e:e + 1], aux[e:e + 1])
            assert hc.same(alone, hc.Closest(*(x[e:e + 1] for x in full))), (kind, e)
    out = hc.Closest(*(np.full(shape, fill, dt) for shape, fill, dt in zip(hc.shapes_of(N, cfg), (-3, -7, -5, -6, -9), hc.DTYPES)))
    hc.closest_host(cfg, state, items, aux, mask=np.array([1, 0, 5, 0, 1], np.uint8), out=out)
    for e in range(N):
        if e in (1, 3):
            assert all((x[e] == fill).all() for x, fill in zip(out, (-3, -7, -5, -6, -9)))
        else:
            assert all(np.array_equal(x[e], y[e]) for x, y in zip(hc.bits(out), hc.bits(full)))
    for want in (('distance',), ('which',), ('on_link',), ('on_surface',), ('normal',), ('distance', 'normal')):
        part = hc.closest_host(cfg, state, items, aux, want=want)
        assert all((x is None) == (name not in want) and (x is None or np.array_equal(x, y)) for name, x, y in zip(hc.NAMES, hc.bits(part), hc.bits(full)))


def test_default_spec_the_mirrors_and_the_header():
    for kind in hc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        s, h = Cl.default_spec(cfg), Cl.hrl_closest_spec()
        assert hc.lib().closest_host_default_spec(C.byref(cfg), C.byref(h)) == 0 and bytes(s) == bytes(h)
        assert (s.struct_size, s.classes, s.reserved) == (C.sizeof(Cl.hrl_closest_spec), Cl.EVERYTHING, 0) and hc.lib().closest_validate_spec(C.byref(s)) == b''
        assert Cl.shapes(cfg, s, (7,))[0] == (7, hc.n_links(cfg), 6) and Cl.shapes(cfg, s, (7,))[4] == (7, hc.n_links(cfg), 6, 3)
    s = Cl.default_spec(cfg, Cl.ROBOT | Cl.GROUND)
    assert s.classes == 96 and hc.lib().closest_validate_spec(C.byref(s)) == b''
    assert Cl.EVERYTHING == 111 and not Cl.EVERYTHING & Cl.TARGET
    assert hc.lib().closest_sizeof_spec() == C.sizeof(Cl.hrl_closest_spec) == 16 and hc.lib().closest_sizeof_out() == C.sizeof(Cl.hrl_closest_out) == 40
    assert Cl.Closest() == (None,) * 5 and Cl.Closest._fields == hc.NAMES == ('distance', 'which', 'on_link', 'on_surface', 'normal')
    hdr = open(os.path.join(hc.ROOT, 'include', 'hrl_closest.h')).read()
    for k, name in enumerate(Cl.CLASS_NAMES):
        assert int(re.search(rf'#define HRL_CLOSEST_{name.upper()} (\d+)', hdr).group(1)) == k
    assert int(re.search(r'#define HRL_CLOSEST_CLASSES (\d+)', hdr).group(1)) == Cl.CLASSES == 6
    assert 'INNER FACES' in hdr and '0.05 m nearer' in hdr and 'THEN IT IS AN UPPER BOUND' in hdr
    cells = Cl.within((np.array([[0.5, np.inf, -0.1, 2.0, np.inf, 0.2]], np.float32), np.array([[6, 0, 2, 3 | 5 << 8, 0, 7 | 4 << 8]], np.int32),
                       np.zeros((1, 6, 3), np.float32), np.ones((1, 6, 3), np.float32), np.zeros((1, 6, 3), np.float32)), 0.5)
    assert [(c[0], c[1], c[2], c[3]) for c in cells] == [(0, 6, 0, 0.5), (0, 2, 0, pytest.approx(-0.1)), (0, 7, 4, pytest.approx(0.2))] and cells[0][5] == (1.0, 1.0, 1.0)


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """closest_check_main (address + undefined-behaviour sanitisers, a program of its own) answers every kind from reset-like states, with
    robots on the ground, at items and in the maze box, and from hostile ones, with subsets of the classes and of the outputs: exit
    status 0, sizeof(hrl_closest_spec) == the ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([hc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_closest_spec {C.sizeof(Cl.hrl_closest_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = hc.lib().closest_check_n_cases()
    assert n == len(sums) == 6 * 4 * 6
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert hc.lib().closest_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different answers


def test_closest_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_closest_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the kernel and an LDS footprint of at most 8 KB; the header's symbols are SYMBOLS; the closest points are an entry of
    build.py of their own, built by build() after the ray test, and SENSORS stays the four."""
    code = 'from hrl_pybullet_envs_amd.build import build_closest, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_closest(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=hc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(hc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_closest_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*closest_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 8192
    hdr = open(os.path.join(hc.ROOT, 'include', 'hrl_closest.h')).read()
    assert set(re.findall(r'\b(hrl_closest(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_closest_out', 'hrl_closest_spec'} == set(Cl.SYMBOLS)
    for s in Cl.SYMBOLS:
        assert hasattr(Cl.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.CLOSEST == ('closest', 'libhrl_closest_hip.so', 'closest_hip.hip', 'closest_core.h', 'hrl_closest.h')
    assert [name for name, *_ in build.SENSORS] == ['render', 'scan', 'probe', 'field'] and 'closest' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_cast(force, verbose)\n    build_closest(force, verbose)') > 0 and 'fourteen libraries' in src
