"""The batched point probes' specification (csrc/probe_core.h) on the CPU: its host build (tests/probe_host) against an independent fp64
numpy reference written from include/hrl_probe.h alone (tests/probe_cases.py), known answers in the maze, the tie to the reference's own
occlusion test, totality on hostile states and points, spec validation, the sanitised stand-alone program and the gfx950 cross-compile.
No GPU."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import orc
import probe_cases as pc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import probe_device as P
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
# metres: the worst |host build - fp64 reference| measured over the sweep of test_host_build_equals_the_fp64_reference, per output
WORST = dict(clearance=2.9e-6, sight=8.9e-6, path=3.2e-6)
TOLS = {k: 4 * v for k, v in WORST.items()}   # asserted at four times that, the scanner's convention
TOL = TOLS['path']                            # routes closer than this are the same route to `via`
assert max(TOLS.values()) <= 1e-4


@pytest.mark.parametrize('kind', pc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Six kinds x three frames x 1, 37, 64, 65 and 512 points x margin 0 and 0.4, on the shard's states, on the hand-made poses and with the robots spread
    about the arena (probe_cases.spread); the points are drawn uniformly (seeded) from the arena's box grown by 1 m.  An identity (nearest, blocker, via == 0) is exempt on a point
    where the reference's changes when the point moves by +-1e-4 m along x or y; at most 1 % of the points of a (kind, spec) are, which
    is asserted on the reference alone first (measured: at most 0.54 %).  On every other point the identity equals the reference's and
    the length (clearance, sight, path) lies within its tolerance of the reference's; `via` equals the reference's where its best and
    second-best routes differ by more than the path's tolerance.  Measured over this sweep, the worst |host build - reference|:
    clearance 2.9e-6 m, path 3.2e-6 m (an ulp of 16 m is 1.9e-6 m) and sight 8.9e-6 m (a segment grazing the flagrun goal's disc; 3.2e-6 m
    elsewhere); asserted at 4 x that: 1.2e-5, 1.3e-5 and 3.6e-5 m, under the ceiling of 1e-4 m."""
    cfg, state, items, aux = shard(kind)
    worst, vias, _ = compare_with_the_reference(cfg, state, items, aux, pc.all_specs(), kind)
    print(f'kind {kind}: worst errors {worst}')
    if pc.is_maze(cfg):   # the sweep goes round the box
        assert {0, 1, 2, 5} <= vias, vias


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states, their hand-made poses and with the robots spread
    about the arena; returns (the worst error per output in metres, the values of `via` met, every code of `nearest` and `blocker` met)."""
    worst = dict(clearance=0.0, sight=0.0, path=0.0)
    vias, codes = set(), set()
    for spec in specs:
        runs = []
        for st in (state, pc.hand_made(cfg, state), pc.spread(cfg, state)):
            pts = pc.draw_points(cfg, st, spec.frame, spec.n_points, pc.seed_of(cfg, spec))
            runs.append((st, pts))
        where = (tag, spec.n_points, spec.frame, spec.margin)
        results = []
        for st, pts in runs:
            got = pc.probe_host(cfg, st, items, aux, spec, pts)
            results.append(pc.compare(cfg, st, items, aux, spec, pts, got, TOL))
            vias |= set(np.unique(got.via))
            codes |= set(np.unique(got.nearest).tolist()) | set(np.unique(got.blocker).tolist())
        for name in ('nearest', 'blocker', 'via0'):   # on the reference alone, before the build is looked at
            ex = sum(r['exempt_' + name].sum() for r in results)
            assert ex <= 0.01 * sum(r['exempt_' + name].size for r in results), (where, name, ex)
        for r in results:
            for name in ('nearest', 'blocker', 'via0', 'via'):
                assert not r['wrong_' + name].any(), (where, name, np.argwhere(r['wrong_' + name])[:4])
            for name in worst:
                worst[name] = max(worst[name], float(r['err_' + name].max()))
                assert r['err_' + name].max() <= TOLS[name], (where, name, r['err_' + name].max())
    return worst, vias, codes


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its tolerances and its cap of 1 % exempt points, on every entry of sensor_configs.MATRIX: 65 points in
    the heading frame at margin 0.4, 512 in the world frame at margin 0 (drawn from the entry's own arena grown by 1 m) and the
    library's default spec at 37 points.  On the entry's hostile states the probes equal, bit for bit, those of the clean twin and a
    robot at a non-finite place gets the blank answers.  On the entries of 64 items an item of index 48 or more is some point's
    nearest shape or blocker; on maze-12 the targets 8 and 11 are."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [pc.spec_of(65, P.HRL_PROBE_HEADING, 0.4), pc.spec_of(512, P.HRL_PROBE_WORLD, 0.0), P.default_spec(cfg, 'world', 37)]
    worst, _, codes = compare_with_the_reference(cfg, state, items, aux, specs, name)
    print(f'{name}: worst errors {worst}')
    for spec in specs[:2]:
        pts = pc.draw_points(cfg, state, spec.frame, spec.n_points, 5)
        for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, pc.hostile):
            got = pc.probe_host(cfg, s, it, a, spec, pts)
            want = pc.probe_host(pc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, pts)
            rows = [e for e in range(N) if e not in blind]
            for x, y in zip(got, want):
                assert np.array_equal(x[rows].view(np.uint32), y[rows].view(np.uint32)), (name, spec.n_points)
            assert pc.is_blank(got, rows=blind)
    if scfg.many_items(cfg):
        assert scfg.saw_a_late_item(sorted(codes)), sorted(codes)
    if name == 'maze-12':
        assert {P.HIT_TARGET | t << 8 for t in (8, 11)} <= codes


def maze_env(robots, n=None):
    cfg = orc.default_config(K.HRL_ANT_MAZE, num_envs=len(robots))
    st = np.zeros((len(robots), K.HRL_STATE_STRIDE), np.float32)
    st[:, 2], st[:, 6] = 0.55, 1.0
    st[:, 0:2] = robots
    return cfg, st, np.zeros((len(robots), K.HRL_AUX_STRIDE), np.int32)


def test_known_answers_in_the_maze():
    """At margin 0.4: from the start (-2, -5) to the evaluation target (-2, 4) the way leads round both +x corners of the grown box,
    (1.401, -2.401) and (1.401, 2.401): 4.2803 + 4.802 + 3.7581 = 12.8405 m, first turning at corner 3; from (4.9, -2.1), which is past
    the wall's margin (the plane is at 4.95), the start is snapped to (4.55, -2.1) and the way to (2, 3) is straight, 0.35 + 5.7020 m; a
    point inside the grown box is unreachable.  The straight line start -> target is blocked by the box (`sight`)."""
    cfg, st, aux = maze_env([(-2.0, -5.0), (4.9, -2.1), (-2.0, -5.0)])
    pts = np.array([[(-2.0, 4.0), (-2.0, -2.3)], [(2.0, 3.0), (2.0, 3.0)], [(1.3, 0.0), (1.5, 0.0)]], np.float32)
    got = pc.probe_host(cfg, st, None, aux, pc.spec_of(2, P.HRL_PROBE_WORLD, 0.4), pts)
    c3, c0 = (1.401, -2.401), (1.401, 2.401)
    want = math.dist((-2, -5), c3) + math.dist(c3, c0) + math.dist(c0, (-2, 4))
    assert abs(want - 12.8405) < 1e-4 and abs(got.path[0, 0] - want) <= pc_tol() and got.via[0, 0] == 2 + 3
    assert got.blocker[0, 0] == P.HIT_BOX and abs(got.sight[0, 0] - 3.0) <= pc_tol()
    assert got.path[0, 1] == np.inf and got.via[0, 1] == 0            # (-2, -2.3) is 0.1 inside the grown box
    assert got.via[1, 0] == 1 and abs(got.path[1, 0] - (0.35 + math.dist((4.55, -2.1), (2, 3)))) <= pc_tol()
    assert got.path[2, 0] == np.inf and got.via[2, 0] == 0            # (1.3, 0): inside the grown box
    assert got.via[2, 1] == 2 + 3 and abs(got.path[2, 1] - (math.dist((-2, -5), c3) + math.dist(c3, (1.5, 0)))) <= pc_tol()
    table = P.corner_table(cfg, 0.4).numpy()
    assert np.isnan(table[:2]).all() and np.allclose(table[2 + 3], c3) and np.allclose(table[2 + 0], c0) and np.allclose(table[2 + 1], (-5.401, 2.401))
    # ego and heading points name the same places: a robot turned by 90 degrees has (-2, 4) at 9 m ahead
    st[0, 3:7] = (0, 0, math.sin(math.pi / 4), math.cos(math.pi / 4))
    for frame, p in ((P.HRL_PROBE_EGO, (0.0, 9.0)), (P.HRL_PROBE_HEADING, (9.0, 0.0))):
        pts[0, 0] = p
        g2 = pc.probe_host(cfg, st, None, aux, pc.spec_of(2, frame, 0.4), pts)
        assert abs(g2.path[0, 0] - want) <= pc_tol() and g2.via[0, 0] == 5 and g2.blocker[0, 0] == P.HIT_BOX
    # a robot leaning on the box is moved out through the nearest side and still reaches everything
    cfg, st, aux = maze_env([(1.2, 0.5)])
    got = pc.probe_host(cfg, st, None, aux, pc.spec_of(1, P.HRL_PROBE_WORLD, 0.4), np.array([[(3.0, 0.5)]], np.float32))
    assert got.via[0, 0] == 1 and abs(got.path[0, 0] - (0.201 + 1.599)) <= pc_tol()


def pc_tol():
    return TOL


def test_flat_kind_has_nothing_in_the_way():
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = pc.spec_of(37, P.HRL_PROBE_WORLD, 0.4)
    pts = pc.draw_points(cfg, state, spec.frame, 37, 3)
    got = pc.probe_host(cfg, state, items, aux, spec, pts)
    straight = np.hypot(*(pts.astype(float) - state[:, None, 0:2].astype(float)).transpose(2, 0, 1))
    assert (got.clearance == np.inf).all() and (got.nearest == 0).all() and (got.blocker == 0).all() and (got.via == 1).all()
    assert np.abs(got.path - straight).max() <= TOL and np.array_equal(got.path, got.sight)
    # ego points do not depend on where the robot is: at 1e20 the answers are the same bits
    ego = pc.spec_of(37, P.HRL_PROBE_EGO, 0.4)
    far = state.copy()
    far[:, 0:2] = (1e20, -1e20)
    a, b = pc.probe_host(cfg, state, items, aux, ego, pts), pc.probe_host(cfg, far, items, aux, ego, pts)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_probe_reproduces_the_references_occlusion_test():
    """tests/golden/maze_step.json, every case with walk_target_dist <= 5 (44): the case's target probed from its torso_xy with
    classes = BOX.  blocker != 0 holds exactly when target_sensor_obs is all zeros on every case whose torso is outside the box (35)
    and on every case inside it (9) except the three whose segment to the target leaves the box through its y = +2 side -- the
    reference's box_bounds has no edge there (maze_scene.py:19-21) and sees through it.  41 cases agree: 7 occluded, 34 visible."""
    with open(os.path.join(pc.ROOT, 'tests', 'golden', 'maze_step.json')) as f:
        cases = [c for c in json.load(f) if c['walk_target_dist'] <= 5]
    assert len(cases) == 44
    cfg, st, aux = maze_env([c['torso_xy'] for c in cases])
    pts = np.array([[c['target']] for c in cases], np.float32)
    got = pc.probe_host(cfg, st, None, aux, pc.spec_of(1, P.HRL_PROBE_WORLD, 0.25, P.BOX), pts, want=('sight', 'blocker'))
    assert got.clearance is None and set(np.unique(got.blocker)) == {0, P.HIT_BOX}
    agree = occluded = 0
    for c, b in zip(cases, got.blocker[:, 0]):
        (x, y), (tx, ty) = c['torso_xy'], c['target']
        inside = -5 <= x <= 1 and -2 <= y <= 2
        through_top = inside and ty > 2 and -5 <= x + (tx - x) * (2 - y) / (ty - y) <= 1
        zeros = not any(c['target_sensor_obs'])
        assert ((b != 0) == zeros) == (not through_top), c
        if not inside:
            assert (b != 0) == zeros
        agree += not through_top
        occluded += (not through_top) and zeros
    assert (agree, occluded) == (41, 7)


@pytest.mark.parametrize('kind', pc.KINDS)
def test_hostile_states_and_points_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range: the probes equal, bit for
    bit, those of the same env with that shape where nothing meets it (an eaten item's place; no goal; a far target), and a robot at a
    non-finite place gets clearance +inf, nearest 0, sight 0, blocker 0, path +inf, via 0.  NaN and +-inf query points get the same
    blank answers and leave their neighbours' bits alone; points at 1e20 and 3.2e38 are finite, and either overflow in the frame's
    arithmetic (blank) or lie outside the arena."""
    cfg, state, items, aux = shard(kind)
    for frame in pc.FRAMES:
        spec = pc.spec_of(65, frame, 0.4)
        pts = pc.draw_points(cfg, state, frame, 65, 5)
        for s, it, a, cs, cit, ca, far, blind in pc.hostile(cfg, state, items, aux):
            got = pc.probe_host(cfg, s, it, a, spec, pts)
            want = pc.probe_host(pc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, pts)
            rows = [e for e in range(N) if e not in blind]
            for x, y in zip(got, want):
                assert np.array_equal(x[rows].view(np.uint32), y[rows].view(np.uint32)), (kind, frame)
            assert pc.is_blank(got, rows=blind)
        clean = pc.probe_host(cfg, state, items, aux, spec, pts)
        bad, blank, huge = pc.hostile_points(pts)
        got = pc.probe_host(cfg, state, items, aux, spec, bad)
        assert pc.is_blank(got, cols=blank)
        rest = [k for k in range(65) if k not in blank + huge]
        for x, y in zip(got, clean):
            assert np.array_equal(x[:, rest].view(np.uint32), y[:, rest].view(np.uint32))
        for k in huge:
            sub = pc.Probe(*(x[:, k:k + 1] for x in got))
            if pc.arena(cfg) is not None:
                assert pc.is_blank(sub) or ((sub.path == np.inf).all() and (sub.via == 0).all() and (sub.clearance <= -1e19).all() and (sub.nearest & 0xFF == P.HIT_WALL).all())
            else:
                assert (sub.path == np.inf).all() and (sub.via == 0).all() and (sub.nearest == 0).all()   # (the square of the distance overflows)
    s = state.copy(); s[:, 3:7] = np.nan   # no heading: forward = world +x, the ego frame's answers
    pts = pc.draw_points(cfg, state, P.HRL_PROBE_EGO, 37, 6)
    a, b = (pc.probe_host(cfg, s, items, aux, pc.spec_of(37, f, 0.4), pts) for f in (P.HRL_PROBE_EGO, P.HRL_PROBE_HEADING))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_none_fields_and_a_mask_leave_the_other_bytes_alone():
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    spec = pc.spec_of(37, P.HRL_PROBE_HEADING, 0.4)
    pts = pc.draw_points(cfg, state, spec.frame, 37, 8)
    full = pc.probe_host(cfg, state, items, aux, spec, pts)
    for want in (('path',), ('via', 'nearest'), ('clearance', 'sight', 'blocker')):
        part = pc.probe_host(cfg, state, items, aux, spec, pts, want=want)
        for name, x, y in zip(pc.NAMES, part, full):
            assert (x is None) if name not in want else np.array_equal(x.view(np.uint32), y.view(np.uint32)), (want, name)
    out = pc.Probe(*(np.full((N, 37), -7, dt) for dt in pc.DTYPES))
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    pc.probe_host(cfg, state, items, aux, spec, pts, mask=mask, out=out)
    for e in range(N):
        for x, y in zip(out, full):
            assert np.array_equal(x[e], y[e]) if mask[e] else (x[e] == -7).all()


def test_class_subsets_pick_among_the_single_class_answers():
    """Clearance and sight under all classes are the minimum over the single-class answers, ties to the class whose slots come first;
    path does not depend on the classes."""
    for kind in (K.HRL_ANT_GATHER, K.HRL_ANT_MAZE):
        cfg, state, items, aux = shard(kind)
        pts = pc.draw_points(cfg, state, P.HRL_PROBE_WORLD, 65, 9)
        full = pc.probe_host(cfg, state, items, aux, pc.spec_of(65, P.HRL_PROBE_WORLD, 0.4), pts)
        best = [np.full((N, 65), np.inf, np.float32), np.zeros((N, 65), np.int32), None, np.zeros((N, 65), np.int32)]
        tbest = np.full((N, 65), np.inf, np.float32)
        for cls in (P.WALL, P.BOX, P.TARGET, P.FOOD, P.POISON):
            one = pc.probe_host(cfg, state, items, aux, pc.spec_of(65, P.HRL_PROBE_WORLD, 0.4, cls), pts)
            take = one.clearance < best[0]
            best[0], best[1] = np.where(take, one.clearance, best[0]), np.where(take, one.nearest, best[1])
            take = (one.blocker != 0) & (one.sight < tbest)
            tbest, best[3] = np.where(take, one.sight, tbest), np.where(take, one.blocker, best[3])
            assert np.array_equal(one.path.view(np.uint32), full.path.view(np.uint32)) and np.array_equal(one.via, full.via)
        assert np.array_equal(best[0].view(np.uint32), full.clearance.view(np.uint32)) and np.array_equal(best[1], full.nearest)
        assert np.array_equal(best[3], full.blocker) and np.array_equal(tbest[best[3] != 0], full.sight[full.blocker != 0])


BAD_SPECS = [('n_points', 0), ('n_points', 513), ('n_points', -1), ('frame', 3), ('frame', -1), ('classes', 0), ('classes', 32), ('margin', float('nan')),
             ('margin', -1.0), ('margin', 3.0), ('margin', float('inf')), ('struct_size', 16), ('struct_size', 0), ('out', None), ('points', None)]


@pytest.mark.parametrize('field,value', BAD_SPECS)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = pc.spec_of(37, P.HRL_PROBE_WORLD, 0.4)
    pts = np.zeros((N, 600, 2), np.float32)
    out = pc.Probe(*(np.full((N, 600), -7, dt) for dt in pc.DTYPES))
    handed = out
    if field == 'out':
        handed = pc.Probe(*(None,) * 6)   # all six outputs NULL
    elif field == 'points':
        pts = None
    else:
        setattr(spec, field, value)
    code, why = pc.probe_host(cfg, state, items, aux, spec, pts, out=handed, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and why
    assert all((x == -7).all() for x in out)
    # the device library runs the same checks before it looks for a device
    L = P.lib()
    b = K.make_buffers(pc.ptr(state), pc.ptr(items), pc.ptr(aux), None, None, None, None, None)
    o = P.hrl_probe_out(**{name: pc.ptr(a) for name, a in zip(pc.NAMES, handed)})
    assert L.hrl_probe(C.byref(cfg), C.byref(b), C.byref(spec), pc.ptr(pts), None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
    assert why.encode() in L.hrl_probe_last_error()
    assert all((x == -7).all() for x in out)


def test_default_spec_and_the_mirrors():
    for kind in pc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, frame in P.FRAMES.items():
            s, h = P.default_spec(cfg, name), P.hrl_probe_spec()
            assert pc.lib().probe_host_default_spec(C.byref(cfg), frame, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.n_points, s.frame, s.classes) == (C.sizeof(P.hrl_probe_spec), 64, frame, P.ALL)
            assert s.margin == np.float32(0.35 if kind == K.HRL_POINT_GATHER else 0.25)
            assert pc.lib().probe_validate_spec(C.byref(s)) == b''
    s = P.default_spec(cfg, 'ego', 37)
    assert (s.n_points, s.frame) == (37, 1) and P.default_spec(cfg).frame == P.HRL_PROBE_WORLD
    with pytest.raises(ValueError):
        P.default_spec(cfg, 'sideways')
    assert pc.lib().probe_sizeof_spec() == C.sizeof(P.hrl_probe_spec) and pc.lib().probe_sizeof_out() == C.sizeof(P.hrl_probe_out)
    assert P.Probe() == (None,) * 6 and P.Probe._fields == pc.NAMES
    assert np.isnan(P.corner_table(orc.default_config(K.HRL_ANT_GATHER, num_envs=1), 0.25).numpy()).all()


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """probe_check_main (address + undefined-behaviour sanitisers, a program of its own) probes every kind in the three frames from
    reset-like and hostile states and points: exit status 0, sizeof(hrl_probe_spec) == the ctypes mirror's, checksums == the unsanitised
    host build's."""
    p = subprocess.run([pc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_probe_spec {C.sizeof(P.hrl_probe_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = pc.lib().probe_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert pc.lib().probe_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different probes


def test_probe_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_probe_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the probe kernel and an LDS footprint under 8 KB; the header's symbols are SYMBOLS."""
    code = 'from hrl_pybullet_envs_amd.build import build_probe, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_probe(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=pc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(pc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_probe_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*probe_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) < 8192
    hdr = open(os.path.join(pc.ROOT, 'include', 'hrl_probe.h')).read()
    assert set(re.findall(r'\b(hrl_probe(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_probe_out', 'hrl_probe_spec'} == set(P.SYMBOLS)
    for s in P.SYMBOLS:
        assert hasattr(P.lib(), s)
