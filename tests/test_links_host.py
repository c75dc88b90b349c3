"""The batched link states' specification (csrc/links_core.h) on the CPU: its host build (tests/links_host) pinned bit for bit to the
step's own leg points (the CPU oracle's orc_ant_leg_points_f32), and held against two independent fp64 references -- the textbook
reference (tests/textbook.py: ant_points) and a numpy one written from include/hrl_links.h alone (tests/links_cases.py) -- in positions,
orientations, velocities (also against a finite difference of the fp64 positions), sites and frames; consistency with what the package
already says about the bodies, the sensor config matrix, spec validation, mask and batch invariance, the sanitised stand-alone program
and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import links_cases as lc
import orc
import sensor_configs as scfg
import textbook as tb
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import contacts
from hrl_pybullet_envs_amd import links_device as Lk
from hrl_pybullet_envs_amd.envs import robot_view
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
ANTS = tuple(k for k in lc.KINDS if k != K.HRL_POINT_GATHER)
# The worst deviations measured over the sweeps of this file (every test below prints its own), and the tolerances: four times the
# worst, rounded up to one digit -- the margin is for states the sweeps do not visit.
POS_WORST = 1.43e-6   # metres, |x|, |y| <= 10 m: origin, com, the far end 2 com - origin and sites against both fp64 references (the issue's condition: below 1e-5)
POS_TOL = 6e-6
ROT_WORST = 4.97e-7   # entries of the rotation matrix of quat against the reference's
ROT_TOL = 2e-6
AIM_WORST = 5.91e-6   # components of quat's image of the capsule's unit fromto direction against (far end - origin) / L: positions at 10 m, two units in their last place, over L = 0.28 m
AIM_TOL = 3e-5
VEL_WORST = 1.09e-7   # m/s and rad/s, relative to the state's speed scale (scale_of: shard states turn their joints at tens of rad/s)
VEL_TOL = 5e-7
FD_H = 1e-6


def leg_points_f32(cfg, st):
    """orc_ant_leg_points_f32 of every env: [n, leg, (hip point, ankle point, foot tip), xyz] float32 -- the step's own points."""
    out = np.zeros((st.shape[0], 36), np.float32)
    for e in range(st.shape[0]):
        orc.lib().orc_ant_leg_points_f32(C.byref(cfg.model), orc.ptr(np.ascontiguousarray(st[e, :15], np.float32)), orc.ptr(out[e]))
    return out.reshape(-1, 4, 3, 3)


def state_sets(kind, state):
    """(label, states, unit quaternions) of a kind: its shard, and for the ants the hand-made poses."""
    sets = [('shard', np.asarray(state), True)]
    if kind != K.HRL_POINT_GATHER:
        sets += [('hand-made', lc.hand_made(), True), ('non-unit', lc.hand_made(4, unit=False), False)]
    return sets


def pinned_to_the_step(cfg, st):
    """Item 1 on states st: origin of aux / foot == the oracle's hip / ankle point, com == the fp32 midpoint of the oracle's two ends, bit
    for bit; returns the worst |2 com - origin - tip|."""
    c = lc.config_of(cfg, st.shape[0])
    got = lc.links_host(c, st, lc.spec_of())
    P = leg_points_f32(c, st)
    half, worst = np.float32(0.5), 0.0
    for l in range(4):
        assert np.array_equal(lc.bits(got.origin[:, Lk.AUX[l]]), lc.bits(P[:, l, 0])) and np.array_equal(lc.bits(got.origin[:, Lk.FEET[l]]), lc.bits(P[:, l, 1]))
        assert np.array_equal(lc.bits(got.com[:, Lk.AUX[l]]), lc.bits(half * (P[:, l, 0] + P[:, l, 1])))
        assert np.array_equal(lc.bits(got.com[:, Lk.FEET[l]]), lc.bits(half * (P[:, l, 1] + P[:, l, 2])))
        assert np.array_equal(lc.bits(got.com[:, Lk.HIPS[l]]), lc.bits(half * (st[:, 0:3] + P[:, l, 0])))
        assert np.array_equal(lc.bits(got.origin[:, Lk.HIPS[l]]), lc.bits(st[:, 0:3]))
        tips = Lk.tip(got)
        worst = max(worst, float(np.abs(tips[:, Lk.FEET[l]].astype(float) - P[:, l, 2]).max()), float(np.abs(tips[:, Lk.AUX[l]].astype(float) - P[:, l, 1]).max()))
    assert np.array_equal(lc.bits(got.origin[:, 0]), lc.bits(st[:, 0:3])) and np.array_equal(lc.bits(got.com[:, 0]), lc.bits(st[:, 0:3]))
    return worst


@pytest.mark.parametrize('kind', ANTS)
def test_origin_and_com_are_the_steps_points_bit_for_bit(kind):
    """The pin to the step.  On the kind's shard, on hand-made poses (tilted torsos, joints at both stops, x and y up to +-10 m) and on
    quaternions up to 1 % off unit length: `origin` of every aux body and foot equals the hip and the ankle point of
    orc_ant_leg_points_f32 BIT FOR BIT (the device step equals that oracle bit for bit), `origin` of the torso and the hip capsules is
    the state's position, and `com` equals the fp32 midpoint 0.5f * (p0 + p1) of the oracle's two ends bit for bit -- which holds the
    foot tip too, through the one rounding of that sum.

    THE MIDPOINT IDENTITY 2 com - origin == tip DOES NOT HOLD BIT FOR BIT: the sum p0 + p1 is rounded (at x = 10 m its last bit is
    9.5e-7 m and the tip's offset from the ankle does not survive it exactly), so the tip is compared within that rounding instead --
    measured 9.54e-7 m, one unit in the last place of 10 m -- and `origin` and `com` carry the bit-for-bit pin."""
    cfg, state, _, _ = shard(kind)
    worst = max(pinned_to_the_step(cfg, st) for _, st, _ in state_sets(kind, state))
    print(f'kind {kind}: worst |2 com - origin - tip| {worst:.3e} m')
    assert worst <= 2.0 ** -20 * 1.0001   # one ulp of a coordinate below 16 m


def scale_of(st):
    """1 + the largest speed of a state's bodies, roughly: |v| + 1.2 m * (|omega| + the fastest hip + the fastest ankle)."""
    return 1.0 + np.linalg.norm(st[15:18]) + 1.2 * (np.linalg.norm(st[18:21]) + np.abs(st[21:29:2]).max() + np.abs(st[22:29:2]).max())


def fd_bound(st, h=FD_H):
    """What the central difference of the fp64 positions may differ by from the velocity: the truncation h^2 / 6 * |third derivative| of a
    point at r <= 1.2 m on a chain turning at W = |omega| + hip rate + ankle rate, |x'''| <= r W^3 + 3 |v| W^2 (the product rule's cross
    terms, bounded generously), plus the rounding of fp64 positions of up to 16 m over 2 h, 2^-52 * 16 / h -- and a term that is no step
    error: the stored quaternion is a unit one only to fp32 rounding, |q|^2 = 1 + d with |d| up to 2.4e-7; the header's matrix of such a
    quaternion is no rotation, and its derivative along the pose integration differs from omega x r by O(d) of the speed (measured
    4e-8 m/s at d = 5e-8, whatever h is): 2 |d| r W is allowed for it."""
    W = np.linalg.norm(st[18:21]) + np.abs(st[21:29:2]).max() + np.abs(st[22:29:2]).max()
    d = abs(st[3:7] @ st[3:7] - 1.0)
    return h * h / 6 * (1.2 * W ** 3 + 3 * np.linalg.norm(st[15:18]) * W ** 2) + 2.0 ** -52 * 16 / h + 2 * d * 1.2 * W


def against_fp64(cfg, kind, st, sites, frame=Lk.HRL_LINKS_WORLD):
    """Items 2 to 5 on unit-quaternion states st: returns the worst (position, rotation matrix, capsule direction, velocity / scale)
    deviations."""
    c = lc.config_of(cfg, st.shape[0])
    got = lc.links_host(c, st, lc.spec_of(frame, sites))
    b = Lk.n_links(kind)
    R32 = lc.quat_axes_f32(got.quat)
    far = Lk.tip(got).astype(np.float64)
    pos = rot = aim = vel = 0.0
    for e in range(st.shape[0]):
        ref = lc.reference(kind, st[e], frame, sites)
        pos = max(pos, np.abs(got.origin[e] - ref['origin']).max(), np.abs(got.com[e] - ref['com']).max(), np.abs(far[e] - ref['far']).max(),
                  np.abs(got.site_pos[e] - ref['site_pos']).max() if sites else 0.0)
        rot = max(rot, np.abs(R32[e] - ref['R']).max())
        for link in range(1, b):   # quat carries the capsule's local fromto direction onto (far end - origin) / L
            d = lc.fromto(link)
            L = np.linalg.norm(d)
            aim = max(aim, np.abs(R32[e, link] @ (d / L) - (far[e, link] - got.origin[e, link].astype(float)) / L).max())
        s = scale_of(st[e].astype(float))
        vel = max(vel, np.abs(got.lin_vel[e] - ref['lin_vel']).max() / s, np.abs(got.ang_vel[e] - ref['ang_vel']).max() / s,
                  np.abs(got.site_vel[e] - ref['site_vel']).max() / s if sites else 0.0)
        if frame == Lk.HRL_LINKS_WORLD:
            if kind != K.HRL_POINT_GATHER:   # the textbook reference: an fp64 implementation of its own
                legs, coms = tb.ant_points(tb.params(c), st[e, :15].astype(np.float64))
                pos = max(pos, np.abs(got.com[e, :9] - coms).max(), np.abs(got.origin[e, 1:9:2] - legs[:, 0]).max(), np.abs(got.origin[e, 2:9:2] - legs[:, 1]).max(),
                          np.abs(far[e, 2:9:2] - legs[:, 2]).max())
                assert np.abs(ref['com'][:9] - coms).max() < 1e-12 and np.abs(ref['far'][2:9:2] - legs[:, 2]).max() < 1e-12   # the two references agree
            # the central difference of the fp64 positions under the fp64 pose integration
            a, z = lc.reference(kind, lc.advance(st[e], FD_H), frame, sites), lc.reference(kind, lc.advance(st[e], -FD_H), frame, sites)
            for name, key in (('lin_vel', 'com'), ('site_vel', 'site_pos')):
                if key == 'site_pos' and not sites:
                    continue
                fd = (a[key] - z[key]) / (2 * FD_H)
                assert np.abs(fd - ref[name]).max() <= fd_bound(st[e].astype(float)), (name, e)   # the reference's own velocities are derivatives
                assert np.abs(getattr(got, name)[e] - fd).max() <= VEL_TOL * s + fd_bound(st[e].astype(float)), (name, e)
    return float(pos), float(rot), float(aim), float(vel)


def check_against_fp64(cfg, kind, sets, tag):
    worst = np.zeros(4)
    for label, st, unit in sets:
        if not unit:
            continue
        sites = lc.sixteen_sites(Lk.n_links(kind))
        for frame in lc.FRAMES:
            worst = np.maximum(worst, against_fp64(cfg, kind, st, sites, frame))
    print(f'{tag}: worst position {worst[0]:.3e} m, rotation {worst[1]:.3e}, direction {worst[2]:.3e}, velocity / scale {worst[3]:.3e}')
    assert worst[0] <= POS_TOL and worst[1] <= ROT_TOL and worst[2] <= AIM_TOL and worst[3] <= VEL_TOL, (tag, worst)
    return worst


@pytest.mark.parametrize('kind', lc.KINDS)
def test_positions_orientations_and_velocities_against_fp64(kind):
    """Items 2 to 4, in both frames, with 16 sites spread over every link.  origin, com, the far end 2 com - origin and the sites agree
    with the numpy reference written from the header and (world frame, links 0..8) with textbook.ant_points' legs36 / coms27;
    quat_axes(quat) agrees with the reference's rotation matrix and carries the capsule's local fromto direction onto (far end - origin)
    / L; lin_vel, ang_vel and site_vel agree with the reference, and with the central difference at h = 1e-6 of the fp64 positions
    under the fp64 pose integration (quaternion exponential, joint angles + h * rate) within VEL_TOL * scale + fd_bound -- fd_bound is
    the step error allowed for, h^2 / 6 (1.2 W^3 + 3 |v| W^2) + 2^-52 * 16 / h + 2.4 |q.q - 1| W with W the chain's total turning rate, and the fp64
    reference's own velocities are asserted to lie within it.  ang_vel of a hip capsule is the torso's, bit for bit.

    Measured over this file's sweeps (six kinds, the shards and the hand-made poses out to +-10 m, the sensor config matrix; the printed
    lines): position 1.422e-6 m at worst (the far end 2 com - origin at |x| = 10 m, where a unit in the last place is 9.5e-7 m; origin
    and com alone 9.1e-7 m), under the issue's condition of 1e-5 m; rotation matrix 4.97e-7; the capsule's direction 5.90e-6 (fp32
    positions at 10 m divided by L = 0.28 m; 3.3e-6 within the mazes' +-5 m); velocities 1.09e-7 of the state's speed scale (the
    deviation is relative to scale_of, not absolute: shard states turn their joints at tens of rad/s).  The tolerances are four times
    those, rounded up to one digit."""
    cfg, state, _, _ = shard(kind)
    sets = state_sets(kind, state)
    worst = check_against_fp64(cfg, kind, sets, f'kind {kind}')
    assert worst[0] < 1e-5   # the issue's condition on the specification itself
    for _, st, _ in sets:
        got = lc.links_host(lc.config_of(cfg, st.shape[0]), st, lc.spec_of())
        if kind != K.HRL_POINT_GATHER:
            for l in range(4):
                assert np.array_equal(lc.bits(got.ang_vel[:, Lk.HIPS[l]]), lc.bits(got.ang_vel[:, 0])) and np.array_equal(lc.bits(got.quat[:, Lk.HIPS[l]]), lc.bits(got.quat[:, 0]))
        assert np.array_equal(lc.bits(got.ang_vel[:, 0]), lc.bits(st[:, 18:21])) and np.array_equal(lc.bits(got.lin_vel[:, 0]), lc.bits(st[:, 15:18]))


@pytest.mark.parametrize('kind', ANTS)
def test_sites(kind):
    """The default sites equal the foot tips within POS_TOL; a site with local = 0 equals its link's origin exactly; site_vel at the
    centre of mass's local offset equals lin_vel within VEL_TOL."""
    cfg, state, _, _ = shard(kind)
    for _, st, unit in state_sets(kind, state):
        if not unit:
            continue
        c = lc.config_of(cfg, st.shape[0])
        default = Lk.hrl_links_spec()
        assert lc.lib().links_host_default_spec(C.byref(c), Lk.HRL_LINKS_WORLD, C.byref(default)) == 0 and bytes(default) == bytes(lc.spec_of(0, lc.foot_sites()))
        got = lc.links_host(c, st, default)
        assert np.abs(got.site_pos.astype(float) - Lk.tip(got)[:, Lk.FEET, :]).max() <= POS_TOL
        zero = lc.links_host(c, st, lc.spec_of(0, tuple((k, (0.0, 0.0, 0.0)) for k in range(13))))
        assert np.array_equal(zero.site_pos, zero.origin)
        at_com = lc.links_host(c, st, lc.spec_of(0, tuple((k, tuple(0.5 * lc.fromto(k))) for k in range(13))))
        scale = np.array([scale_of(s.astype(float)) for s in st])[:, None, None]
        assert (np.abs(at_com.site_vel.astype(float) - at_com.lin_vel) <= VEL_TOL * scale).all() and np.abs(at_com.site_pos.astype(float) - at_com.com).max() <= POS_TOL


@pytest.mark.parametrize('kind', lc.KINDS)
def test_heading_frame_is_the_world_frame_turned(kind):
    """HEADING outputs turned back by the fp64 yaw (and moved back to the torso) equal the WORLD outputs within the tolerances; the
    torso's origin and com are exactly 0 in HEADING; velocities are only turned, not made relative."""
    cfg, state, _, _ = shard(kind)
    sites = lc.sixteen_sites(Lk.n_links(kind))
    for _, st, unit in state_sets(kind, state):
        if not unit:
            continue
        c = lc.config_of(cfg, st.shape[0])
        world, head = lc.links_host(c, st, lc.spec_of(Lk.HRL_LINKS_WORLD, sites)), lc.links_host(c, st, lc.spec_of(Lk.HRL_LINKS_HEADING, sites))
        assert (head.origin[:, 0] == 0).all() and (head.com[:, 0] == 0).all()
        Rw, Rh = lc.quat_axes_f32(world.quat), lc.quat_axes_f32(head.quat)
        for e in range(st.shape[0]):
            T = lc.yaw_matrix(lc.rot_of_quat(st[e, 3:7].astype(float)))
            O, s = st[e, 0:3].astype(float), scale_of(st[e].astype(float))
            for name in ('origin', 'com', 'site_pos'):
                assert np.abs(getattr(head, name)[e] @ T + O - getattr(world, name)[e]).max() <= POS_TOL, (name, e)
            for name in ('lin_vel', 'ang_vel', 'site_vel'):
                assert np.abs(getattr(head, name)[e] @ T - getattr(world, name)[e]).max() <= VEL_TOL * s, (name, e)
            assert np.abs(np.einsum('ji,bjk->bik', T, Rh[e]) - Rw[e]).max() <= ROT_TOL


def test_consistency_with_what_exists():
    """The mean of the 13 com's xy equals robot_view.ant_parts_centroid (fp64 numpy; no static bodies); links 0..8 are in the body order
    of contacts.body_of_link, and the names are the asset's; the point bot has one link whose pose and velocity are the state's bits, in
    the world frame whatever the state holds."""
    for kind in ANTS:
        cfg, state, _, _ = shard(kind)
        for _, st, unit in state_sets(kind, state):
            got = lc.links_host(lc.config_of(cfg, st.shape[0]), st, lc.spec_of())
            if unit:
                cen = robot_view.ant_parts_centroid(st[:, :15], 0, (0.0, 0.0))
                assert np.abs(got.com[:, :, :2].astype(float).mean(1) - cen).max() <= POS_TOL
    for l in range(4):
        for level, table in ((1, Lk.AUX), (2, Lk.FEET)):
            assert int(contacts.body_of_link(torch.tensor(level | l << 2))) == table[l]
        assert int(contacts.body_of_link(torch.tensor(0 | l << 2))) == Lk.TORSO   # a hip capsule's contacts are the torso's
    names = Lk.NAMES(K.HRL_ANT_GATHER)
    assert names == tuple(lc.lib().links_host_name(K.HRL_ANT_GATHER, i).decode() for i in range(13)) and lc.lib().links_host_name(K.HRL_ANT_GATHER, 13) is None
    assert names[0] == 'torso' and tuple(names[i] for i in Lk.AUX) == ('aux_1', 'aux_2', 'aux_3', 'aux_4') and tuple(names[i] for i in Lk.FEET) == Lk.FOOT_LIST
    assert tuple(names[i] for i in Lk.HIPS) == ('front_left_leg', 'front_right_leg', 'left_back_leg', 'right_back_leg')
    assert Lk.NAMES(K.HRL_POINT_GATHER) == ('cube',) and Lk.n_links(K.HRL_POINT_GATHER) == 1 and Lk.n_links(K.HRL_ANT_MAZE) == 13
    cfg, state, _, _ = shard(K.HRL_POINT_GATHER)
    st = np.array(state)
    st[1, 18], st[2, 15], st[3, 0] = np.inf, -np.inf, -0.0
    got = lc.links_host(cfg, st, Lk.default_spec(cfg))
    assert got.origin.shape == (N, 1, 3) and got.site_pos.shape == (N, 1, 3)
    for name, lo in (('origin', 0), ('com', 0), ('quat', 3), ('lin_vel', 15), ('ang_vel', 18)):
        a = getattr(got, name)
        assert np.array_equal(lc.bits(a[:, 0]), lc.bits(st[:, lo:lo + a.shape[2]])), name


def nan_states(state):
    """(states with a NaN in another place of the record per env, the envs, the places)"""
    places = (0, 4, 9, 16, 24)   # x, a quaternion component, a joint angle, a velocity, a joint rate
    out = []
    for e, place in enumerate(places):
        s = np.array(state)
        s[e, place] = np.nan
        out.append((s, e, place))
    return out


@pytest.mark.parametrize('name', scfg.NAMES)
def test_the_sensor_config_matrix(name):
    """Items 1 and 2 (the pin to the step and the fp64 comparison, with this file's tolerances) on every entry of
    sensor_configs.MATRIX.  A NaN in an env's record -- x, a quaternion component, a joint angle, a velocity, a joint rate -- makes
    outputs of that env non-finite in the world frame, leaves every other env's bits what they were, and never crashes."""
    cfg, state, _, _ = scfg.shard(name)
    kind = scfg.kind_of(name)
    if kind != K.HRL_POINT_GATHER:
        pinned_to_the_step(cfg, np.asarray(state))
    check_against_fp64(cfg, kind, [('shard', np.asarray(state), True)], name)
    spec = Lk.default_spec(cfg)
    clean = lc.links_host(cfg, state, spec)
    assert all(np.isfinite(x).all() for x in clean)
    for s, e, place in nan_states(state):
        if kind == K.HRL_POINT_GATHER and place in (9, 24):
            continue   # the cube has no joints: nothing reads those slots
        got = lc.links_host(cfg, s, spec)
        others = [i for i in range(N) if i != e]
        assert lc.same(lc.Links(*(x[others] for x in got)), lc.Links(*(x[others] for x in clean))), (name, e)
        assert any(not np.isfinite(x[e]).all() for x in got), (name, e, place)


SPEC_BAD = [('struct_size', 16), ('struct_size', 0), ('n_sites', -1), ('n_sites', 17), ('site_link', 13), ('site_link', -1), ('site_local', float('nan')), ('site_local', float('inf')),
            ('frame', 2), ('frame', -1), ('out', 'empty'), ('out', 'sites-only'), ('out', 'null')]
REASONS = {'struct_size': 'hrl_links_spec.struct_size is not sizeof(hrl_links_spec)', 'n_sites': 'links n_sites must be within 0..16', 'site_link': 'links site_link must be within 0..B-1',
           'site_local': 'links site_local must be finite', 'frame': 'unknown links frame', 'empty': 'links out holds no pointer: at least one output must be given',
           'sites-only': 'links out holds no pointer: at least one output must be given', 'null': 'null links out'}


@pytest.mark.parametrize('field,value', SPEC_BAD)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, _, aux = shard(K.HRL_ANT_FLAT)
    spec = lc.spec_of(Lk.HRL_LINKS_HEADING, lc.foot_sites())
    out = lc.Links(*(np.full(shape, -3, np.float32) for shape in lc.shapes_of(cfg, N, lc.spec_of(0, lc.sixteen_sites(13)))))
    if field == 'site_link':
        spec.site_link[3] = value
    elif field == 'site_local':
        spec.site_local[2][1] = value
    elif field != 'out':
        setattr(spec, field, value)
    if value == 'sites-only':
        spec.n_sites = 0
    b = K.make_buffers(lc.ptr(np.asarray(state)), None, lc.ptr(np.asarray(aux)), None, None, None, None, None)
    given = {} if value == 'empty' else ({'site_pos': lc.ptr(out.site_pos), 'site_vel': lc.ptr(out.site_vel)} if value == 'sites-only' else {n: lc.ptr(a) for n, a in zip(lc.NAMES, out)})
    o = Lk.hrl_links_out(**given)
    ref = None if value == 'null' else C.byref(o)
    code = lc.lib().links_host(C.byref(cfg), C.byref(b), C.byref(spec), None, ref)
    why = lc.lib().links_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and REASONS[value if field == 'out' else field] in why, why
    untouched = lambda: all((a == -3).all() for a in out)
    assert untouched()
    # the device library runs the same checks before it looks for a device
    L = Lk.lib()
    assert L.hrl_links(C.byref(cfg), C.byref(b), C.byref(spec), None, ref, None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_links_last_error() == b'hrl_links: ' + why.encode()
    assert untouched()


def test_a_site_on_the_point_bots_second_link_is_refused():
    cfg, state, _, _ = shard(K.HRL_POINT_GATHER)
    code, why = lc.links_host(cfg, state, lc.spec_of(0, ((1, (0.0, 0.0, 0.0)),)), expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and 'links site_link must be within 0..B-1' in why


def test_default_spec_and_the_mirrors():
    for kind in lc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, frame in Lk.FRAMES.items():
            s, h = Lk.default_spec(cfg, name), Lk.hrl_links_spec()
            assert lc.lib().links_host_default_spec(C.byref(cfg), frame, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.frame, s.n_sites) == (C.sizeof(Lk.hrl_links_spec), frame, 1 if kind == K.HRL_POINT_GATHER else 4)
            assert lc.lib().links_validate_spec(C.byref(cfg), C.byref(s)) == b''
    s = Lk.default_spec(cfg, 'heading', [(2, (0.1, 0.2, 0.3)), (12, (0, 0, -1))])
    assert (s.frame, s.n_sites, s.site_link[0], s.site_link[1], s.site_link[2]) == (1, 2, 2, 12, 0) and tuple(s.site_local[0]) == tuple(np.float32((0.1, 0.2, 0.3)))
    assert Lk.default_spec(cfg, sites=()).n_sites == 0
    with pytest.raises(ValueError):
        Lk.default_spec(cfg, 'sideways')
    with pytest.raises(ValueError):
        Lk.default_spec(cfg, sites=[(0, (0, 0, 0))] * 17)
    assert lc.lib().links_sizeof_spec() == C.sizeof(Lk.hrl_links_spec) == 272 and lc.lib().links_sizeof_out() == C.sizeof(Lk.hrl_links_out) == 56
    assert Lk.Links() == (None,) * 7 and Lk.Links._fields == lc.NAMES
    hdr = open(os.path.join(lc.ROOT, 'include', 'hrl_links.h')).read()
    for name, value in (('HRL_LINKS_ANT', Lk.LINKS_ANT), ('HRL_LINKS_POINT', Lk.LINKS_POINT), ('HRL_LINKS_MAX_SITES', Lk.MAX_SITES), ('HRL_LINKS_WORLD', Lk.HRL_LINKS_WORLD),
                        ('HRL_LINKS_HEADING', Lk.HRL_LINKS_HEADING)):
        assert int(re.search(rf'#define {name} (\d+)', hdr).group(1)) == value
    assert 'INERTIAL' in hdr   # the header says what quat is not


def test_an_env_does_not_depend_on_its_batch():
    """N = 17 with every other env masked: env e equals the same env alone in a batch of 1; a masked env keeps its bytes; a NULL member
    is not written."""
    n = 17
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=n)
    st = np.concatenate([lc.hand_made(7, 12), lc.hand_made(8, 5)])
    spec = lc.spec_of(Lk.HRL_LINKS_HEADING, lc.sixteen_sites(13))
    full = lc.links_host(cfg, st, spec)
    one = lc.config_of(cfg, 1)
    for e in range(n):
        alone = lc.links_host(one, st[e:e + 1], spec)
        assert lc.same(alone, lc.Links(*(x[e:e + 1] for x in full))), e
    out = lc.Links(*(np.full(shape, -3, np.float32) for shape in lc.shapes_of(cfg, n, spec)))
    mask = (np.arange(n) % 2 == 0).astype(np.uint8) * 3
    lc.links_host(cfg, st, spec, mask=mask, out=out)
    for e in range(n):
        if mask[e]:
            assert all(np.array_equal(lc.bits(x[e]), lc.bits(y[e])) for x, y in zip(out, full))
        else:
            assert all((x[e] == -3).all() for x in out)
    for want in [(name,) for name in lc.NAMES] + [('com', 'site_vel')]:
        part = lc.links_host(cfg, st, spec, want=want)
        assert all((x is None) == (name not in want) and (x is None or np.array_equal(lc.bits(x), lc.bits(y))) for name, x, y in zip(lc.NAMES, part, full))


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """links_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the link states of every kind in both
    frames from reset-like and hostile states at 5, 16, 17 and 37 envs with 0, 1, 4 and 16 sites: exit status 0,
    sizeof(hrl_links_spec) == the ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([lc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_links_spec {C.sizeof(Lk.hrl_links_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = lc.lib().links_check_n_cases()
    assert n == len(sums) == 6 * 2 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert lc.lib().links_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different states


def test_links_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_links_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the kernel and an LDS footprint under 8 KB; the source holds no inline assembly; the header's symbols are SYMBOLS; the
    link states are an entry of build.py of their own, built by build() after the camera."""
    code = 'from hrl_pybullet_envs_amd.build import build_links, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_links(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=lc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(lc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_links_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*links_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) < 8192
    csrc = os.path.join(lc.ROOT, 'hrl_pybullet_envs_amd', 'csrc')
    for name in ('links_hip.hip', 'links_core.h'):
        assert not re.search(r'\basm\b|__asm__', open(os.path.join(csrc, name)).read()), name
    hdr = open(os.path.join(lc.ROOT, 'include', 'hrl_links.h')).read()
    assert set(re.findall(r'\b(hrl_links(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_links_out', 'hrl_links_spec'} == set(Lk.SYMBOLS)
    for s in Lk.SYMBOLS:
        assert hasattr(Lk.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.LINKS == ('links', 'libhrl_links_hip.so', 'links_hip.hip', 'links_core.h', 'hrl_links.h') and 'links' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_camera(force, verbose)\n    build_links(force, verbose)') > 0
