"""The batched range scanner's specification (csrc/scan_core.h) on the CPU: its host build (tests/scan_host) against an independent fp64
numpy ray caster written from include/hrl_scan.h alone (tests/scan_cases.py), the tie to the reference's own sense_walls numbers, the
invariants of a scan, totality on hostile states, spec validation, the sanitised stand-alone program and the gfx950 cross-compile.
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
import scan_cases as sc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import scan_device as S
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
SLACK = 4 * 8.3e-7          # metres: four times the worst excess measured below
assert SLACK <= 1e-4
GOLDEN_TOL = 4 * 4.4e-6     # metres: four times the worst error measured against the reference's sense_walls numbers
assert GOLDEN_TOL <= 1e-4


@pytest.mark.parametrize('kind', sc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Specs: 1, 37, 64, 65 and 512 rays x both frames x max_range 6 and 20, on the shard's states and on the hand-made poses.
    A ray is exempt when the reference's hit identity differs at theta - 1e-4, theta or theta + 1e-4 rad; exempt rays are at most 1 %
    per (kind, spec).  On every other ray `hit` equals the reference's and `range` lies within [min, max] of the reference at
    theta - 1e-5, theta, theta + 1e-5 rad (two orders above sincos_spec's error: the bracket follows the incidence) widened by SLACK.
    Measured: the worst excess of the host build over the bare bracket is 8.3e-7 m (under half an ulp of 20 m); asserted at
    4 x that = 3.3e-6 m, under the ceiling of 1e-4 m."""
    cfg, state, items, aux = shard(kind)
    worst, _ = compare_with_the_reference(cfg, state, items, aux, sc.all_specs(), kind)
    print(f'kind {kind}: worst excess over the bracket {worst:.3e} m')
    if kind != K.HRL_ANT_FLAT:   # the scans are not blank
        assert (sc.scan_host(cfg, state, items, aux, sc.spec_of(64, S.HRL_SCAN_HEADING, 20.0))[1] != 0).any()


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states and their hand-made poses; returns (the worst
    excess over the bracket in metres, the largest share of exempt rays of a spec)."""
    worst, share = 0.0, 0.0
    for spec in specs:
        n_exempt = total = 0
        where = (tag, spec.n_rays, spec.frame, spec.max_range)
        for st in (state, sc.hand_made(cfg, state)):
            got = sc.scan_host(cfg, st, items, aux, spec)
            exempt, wrong, excess = sc.compare(cfg, st, items, aux, spec, got)
            n_exempt += exempt.sum(); total += exempt.size
            assert not wrong.any(), (where, np.argwhere(wrong)[:4])
            worst = max(worst, float(np.where(exempt, 0.0, excess).max()))
            assert np.where(exempt, 0.0, excess).max() <= SLACK, (where, worst)
        assert n_exempt <= 0.01 * total, (where, n_exempt, total)
        share = max(share, n_exempt / total)
    return worst, share


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its SLACK, its bracket and its cap of 1 % exempt rays, on every entry of sensor_configs.MATRIX: 65 rays
    in the heading frame out to 20 m, 512 in the world frame out to 6 m, and the library's default spec, whose range is the diagonal of
    the entry's own arena (flagrun's open field has none).  On the entry's hostile states the scan equals, bit for bit, that of the
    clean twin; a robot at a NaN place sees nothing.  On the entries of 64 items some ray reports an item of index 48 or more; on
    maze-12 the targets 8 and 11 are reported.  Measured: the worst excess over the bare bracket is 8.5e-7 m (gather-tall), under SLACK;
    at most 0.47 % of a spec's rays exempt (gather-tall; 0.31 % on the entries of 32 and 64 items)."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [sc.spec_of(65, S.HRL_SCAN_HEADING, 20.0), sc.spec_of(512, S.HRL_SCAN_WORLD, 6.0), S.default_spec(cfg)]
    worst, share = compare_with_the_reference(cfg, state, items, aux, specs, name)
    print(f'{name}: worst excess over the bracket {worst:.3e} m, at most {100 * share:.2f} % of a spec\'s rays exempt')
    for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, sc.hostile):
        for spec in specs[::2]:
            got = sc.scan_host(cfg, s, it, a, spec)
            want = sc.scan_host(sc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
            rows = [e for e in range(N) if e not in blind]
            assert np.array_equal(got[0][rows].view(np.uint32), want[0][rows].view(np.uint32)) and np.array_equal(got[1][rows], want[1][rows]), (name, spec.n_rays)
            for e in blind:
                assert (got[0][e] == np.float32(spec.max_range)).all() and (got[1][e] == 0).all()
    hit = sc.scan_host(cfg, state, items, aux, specs[1])[1]
    assert (hit != 0).any()
    if scfg.many_items(cfg):
        assert all(scfg.saw_a_late_item(hit[e]) for e, _, _ in scfg.NEAR_ITEMS)
    if name == 'maze-12':
        assert {S.HIT_TARGET | t << 8 for t in (8, 11)} <= set(hit.ravel().tolist())


def golden_arena(world):
    """(cfg, state, aux, out [30, 10]) of the 30 `arena` cases of tests/golden/sense_walls.json in a gather config of world_size
    (world, world): the torso at `pos`, a quaternion of `yaw`."""
    with open(os.path.join(sc.ROOT, 'tests', 'golden', 'sense_walls.json')) as f:
        cases = [c for c in json.load(f)['cases'] if c['scene'] == 'arena']
    assert len(cases) == 30 and all((c['bins'], c['span'], c['range']) == (10, 2 * math.pi, 5.0) for c in cases)
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=len(cases), world_size=(world, world))
    st = np.zeros((len(cases), K.HRL_STATE_STRIDE), np.float32)
    st[:, 2] = 0.55
    for i, c in enumerate(cases):
        st[i, 0:2] = c['pos']
        st[i, 3:7] = (0.0, 0.0, math.sin(c['yaw'] / 2), math.cos(c['yaw'] / 2))
    return cfg, st, np.zeros((len(cases), K.HRL_AUX_STRIDE), np.int32), np.array([c['out'] for c in cases], float)


def golden_errors(world):
    cfg, st, aux, out = golden_arena(world)
    rng, hit = sc.scan_host(cfg, st, None, aux, S.sensor_spec(10, 2 * math.pi, 5.0, S.WALL))
    cls, _ = S.decode(hit)
    seen = out > 0
    assert seen.sum() > 100
    return np.abs(rng - np.where(seen, (1 - out) * 5, 5.0)), cls, seen


def test_scan_reproduces_the_references_sense_walls_numbers():
    """The 30 `arena` cases of tests/golden/sense_walls.json in a gather config with world_size (15, 15), sensor_spec(10, 2 pi, 5),
    classes = WALL: where out[i] > 0, range[i] = (1 - out[i]) * 5 and the class is wall; elsewhere no hit and range == 5.  (The `maze`
    cases are not used: the reference intersects infinite lines there, the scanner finite shapes.)  The scanner's walls are the
    arena's bounding lines at +-world_size / 2, where the reference meets them (scan_core.h: WALL_HALF beyond the collision planes).
    Measured worst |range - (1 - out) * 5| = 4.4e-6 m; asserted at 4 x that = 1.8e-5 m, under the ceiling of 1e-4 m."""
    err, cls, seen = golden_errors(15.0)
    print(f'world_size 15: worst error {err.max():.3e} m')
    assert np.array_equal(cls, np.where(seen, S.HIT_WALL, S.HIT_NONE))
    assert err[~seen].max() == 0.0 and err.max() <= GOLDEN_TOL


def in_bracket(cfg, state, items, aux, spec, rng):
    exempt, _, excess = sc.compare(cfg, state, items, aux, spec, (rng, np.zeros_like(rng, np.int32)))
    return np.where(exempt, 0.0, excess).max() <= SLACK


def test_heading_frame_turns_with_the_robot():
    """Turning robot and world together leaves `range` unchanged, within the bracket test of the unturned scan.  Discs turn with
    anything: flagrun's goal and the maze's targets by 0.9 rad; the square gather arena with its items turns onto itself by 90 degrees
    (the classes seen stay, the planes' indices permute)."""
    for kind, angle, classes in ((K.HRL_ANT_FLAGRUN, 0.9, S.TARGET), (K.HRL_ANT_MAZE, 0.9, S.TARGET), (K.HRL_ANT_GATHER, math.pi / 2, S.ALL),
                                 (K.HRL_POINT_GATHER, math.pi / 2, S.ALL)):
        cfg, state, items, aux = shard(kind)
        c, s = math.cos(angle), math.sin(angle)
        turned_cfg, it = cfg.copy(), items.copy()
        if kind == K.HRL_ANT_MAZE:
            for t in range(cfg.n_targets):
                x, y = cfg.targets[t][0], cfg.targets[t][1]
                turned_cfg.targets[t][0], turned_cfg.targets[t][1] = c * x - s * y, s * x + c * y
        else:
            n = 1 if kind == K.HRL_ANT_FLAGRUN else cfg.n_food + cfg.n_poison
            x, y = items[:, 0:2 * n:2].astype(float), items[:, 1:2 * n:2].astype(float)
            it[:, 0:2 * n:2], it[:, 1:2 * n:2] = c * x - s * y, s * x + c * y
        for n_rays in (64, 512):
            spec = sc.spec_of(n_rays, S.HRL_SCAN_HEADING, 20.0, classes)
            a = sc.scan_host(cfg, state, items, aux, spec)
            b = sc.scan_host(turned_cfg, sc.yawed(state, items, cfg, angle), it, aux, spec)
            assert in_bracket(cfg, state, items, aux, spec, b[0]), (kind, n_rays)
            assert (a[1] != 0).any() and (b[1] != 0).any()
    # the fallback: a torso whose X axis points straight up has no heading -- forward = world +x, the world frame's scan
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    s = state.copy()
    s[:, 3:7] = (0, -np.sqrt(0.5), 0, np.sqrt(0.5))
    a, b = (sc.scan_host(cfg, s, items, aux, sc.spec_of(65, f, 20.0)) for f in sc.FRAMES)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('kind', sc.KINDS)
def test_the_full_scan_is_the_nearest_of_the_single_class_scans(kind):
    """Bit for bit, ties to the class whose slots come first; and a class whose bit is off is never reported."""
    cfg, state, items, aux = shard(kind)
    code_of = {S.WALL: S.HIT_WALL, S.BOX: S.HIT_BOX, S.TARGET: S.HIT_TARGET, S.FOOD: S.HIT_FOOD, S.POISON: S.HIT_POISON}
    for frame in sc.FRAMES:
        for rmax in sc.RANGES:
            full = sc.scan_host(cfg, state, items, aux, sc.spec_of(65, frame, rmax))
            best, hit = np.full((N, 65), np.inf, np.float32), np.zeros((N, 65), np.int32)
            for cls in sc.SLOT_ORDER:
                r, h = sc.scan_host(cfg, state, items, aux, sc.spec_of(65, frame, rmax, cls))
                assert set(np.unique(S.decode(h)[0])) <= {S.HIT_NONE, code_of[cls]}, (kind, cls)
                assert (r[h == 0] == np.float32(rmax)).all()
                take = (h != 0) & (r < best)
                best, hit = np.where(take, r, best), np.where(take, h, hit)
            assert np.array_equal(hit, full[1]) and np.array_equal(np.where(hit != 0, best, np.float32(rmax)).view(np.uint32), full[0].view(np.uint32)), (kind, frame, rmax)
            two = sc.scan_host(cfg, state, items, aux, sc.spec_of(65, frame, rmax, S.WALL | S.POISON))
            assert set(np.unique(S.decode(two[1])[0])) <= {S.HIT_NONE, S.HIT_WALL, S.HIT_POISON}


def test_standing_on_an_item_and_standing_outside_the_arena():
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    s = state.copy()
    slots = (0, 3, cfg.n_food, cfg.n_food + 2, cfg.n_food + cfg.n_poison - 1)
    it = items.copy()
    for e, i in enumerate(slots):   # the item well inside the arena, clear of the others; the robot 0.05 off its centre
        it[e, 2 * i:2 * i + 2] = (-6.0 + e, 6.5)
        s[e, 0:2] = (-6.0 + e + 0.05, 6.5 - 0.05)
    for frame in sc.FRAMES:
        rng, hit = sc.scan_host(cfg, s, it, aux, sc.spec_of(37, frame, 6.0))
        cls, idx = S.decode(hit)
        for e, i in enumerate(slots):
            assert (rng[e] == 0).all() and (cls[e] == (S.HIT_FOOD if i < cfg.n_food else S.HIT_POISON)).all() and (idx[e] == i).all()
    # beyond the wall on the +x side (plane 0), the -y side (plane 3), and both: range 0, wall, the lower plane
    s = state.copy()
    s[0, 0:2] = (9.0, 1.0); s[1, 0:2] = (1.0, -7.51); s[2, 0:2] = (8.0, -8.0); s[3, 0:2] = (-7.51, 0.0); s[4, 0:2] = (0.0, 30.0)
    for frame in sc.FRAMES:
        rng, hit = sc.scan_host(cfg, s, items, aux, sc.spec_of(37, frame, 6.0))
        cls, idx = S.decode(hit)
        assert (rng == 0).all() and (cls == S.HIT_WALL).all()
        assert [set(idx[e]) for e in range(N)] == [{0}, {3}, {0}, {1}, {2}]
    # maze: standing on the target, standing in the box
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    s, a = state.copy(), aux.copy()
    a[:, 3] = (0, 1, 2, 3, 0)
    for e in range(4):
        s[e, 0:2] = (cfg.targets[a[e, 3]][0] + 0.1, cfg.targets[a[e, 3]][1] - 0.1)
    s[4, 0:2] = (-3.0, 1.0)
    rng, hit = sc.scan_host(cfg, s, items, a, sc.spec_of(64, S.HRL_SCAN_HEADING, 20.0))
    assert (rng == 0).all() and [set(hit[e]) for e in range(N)] == [{S.HIT_TARGET | t << 8} for t in range(4)] + [{S.HIT_BOX}]


def test_a_mask_leaves_the_other_rows_alone():
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    spec = sc.spec_of(37, S.HRL_SCAN_HEADING, 20.0)
    full = sc.scan_host(cfg, state, items, aux, spec)
    out = np.full((N, 37), -7.0, np.float32), np.full((N, 37), -7, np.int32)
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    sc.scan_host(cfg, state, items, aux, spec, mask=mask, out=out)
    for e in range(N):
        for got, want in zip(out, full):
            assert np.array_equal(got[e], want[e]) if mask[e] else (got[e] == -7).all()


@pytest.mark.parametrize('kind', sc.KINDS)
def test_hostile_states_scan_as_if_the_offending_shape_were_out_of_reach(kind):
    """NaN, +-inf and 1e20 in the robot's position, an item or the flagrun goal, and target indices out of range: the scan equals, bit
    for bit, the one of the same env with that shape moved out of reach; a robot at a NaN place sees nothing."""
    cfg, state, items, aux = shard(kind)
    for s, it, a, cs, cit, ca, far, blind in sc.hostile(cfg, state, items, aux):
        for frame in sc.FRAMES:
            spec = sc.spec_of(65, frame, 20.0)
            got = sc.scan_host(cfg, s, it, a, spec)
            want = sc.scan_host(sc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
            rows = [e for e in range(N) if e not in blind]
            assert np.array_equal(got[0][rows].view(np.uint32), want[0][rows].view(np.uint32)) and np.array_equal(got[1][rows], want[1][rows]), (kind, frame)
            for e in blind:
                assert (got[0][e] == np.float32(20.0)).all() and (got[1][e] == 0).all()
    s = state.copy(); s[:, 3:7] = np.nan   # no heading: the world frame's scan
    a, b = (sc.scan_host(cfg, s, items, aux, sc.spec_of(37, f, 20.0)) for f in sc.FRAMES)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


BAD_SPECS = [('n_rays', 0), ('n_rays', 513), ('n_rays', -1), ('max_range', float('nan')), ('max_range', 0.0), ('max_range', -1.0), ('max_range', float('inf')),
             ('classes', 0), ('classes', 32), ('classes', 33), ('frame', 2), ('frame', -1), ('first_angle', 65.0), ('first_angle', float('nan')),
             ('step_angle', 2.0), ('step_angle', float('inf')), ('struct_size', 24), ('struct_size', 0)]


@pytest.mark.parametrize('field,value', BAD_SPECS)
def test_bad_specs_are_refused_with_a_reason(field, value):
    """(step_angle 2 over 37 rays from -pi: the last ray at 68.9 rad.)"""
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = sc.spec_of(37, S.HRL_SCAN_WORLD, 6.0)
    setattr(spec, field, value)
    out = np.full((N, 600), -7.0, np.float32), np.full((N, 600), -7, np.int32)
    code, why = sc.scan_host(cfg, state, items, aux, spec, out=out, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and why
    assert (out[0] == -7).all() and (out[1] == -7).all()
    # the device library runs the same checks before it looks for a device
    L = S.lib()
    b = K.make_buffers(sc.ptr(state), sc.ptr(items), sc.ptr(aux), None, None, None, None, None)
    assert L.hrl_scan(C.byref(cfg), C.byref(b), C.byref(spec), None, sc.ptr(out[0]), sc.ptr(out[1]), None) == K.HRL_ERR_BAD_ARG
    assert why.encode() in L.hrl_scan_last_error()
    assert (out[0] == -7).all() and (out[1] == -7).all()


def test_default_and_sensor_specs():
    want = {K.HRL_ANT_FLAT: 10.0, K.HRL_ANT_GATHER: math.hypot(15, 15), K.HRL_POINT_GATHER: math.hypot(15, 15), K.HRL_ANT_MAZE: math.hypot(10, 18),
            K.HRL_ANT_MAZE_MJ: math.hypot(10, 18), K.HRL_ANT_FLAGRUN: 12 * math.sqrt(2)}
    for kind in sc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, frame in S.FRAMES.items():
            s, h = S.default_spec(cfg, name), S.hrl_scan_spec()
            assert sc.lib().scan_host_default_spec(C.byref(cfg), frame, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.n_rays, s.frame, s.classes) == (C.sizeof(S.hrl_scan_spec), 64, frame, S.ALL)
            assert s.max_range == np.float32(want[kind]) and s.first_angle == np.float32(-math.pi + math.pi / 64) and s.step_angle == np.float32(2 * math.pi / 64)
            assert sc.lib().scan_validate_spec(C.byref(s)) == b''
    s = S.default_spec(cfg, 'world', 37)
    assert (s.n_rays, s.frame) == (37, 0) and bytes(s) == bytes(sc.spec_of(37, 0, s.max_range))
    with pytest.raises(ValueError):
        S.default_spec(cfg, 'sideways')
    a = S.sensor_spec(10, 2 * math.pi, 5.0)
    assert (a.n_rays, a.frame, a.classes, a.max_range) == (10, S.HRL_SCAN_HEADING, S.WALL, 5.0)
    assert a.first_angle == np.float32(math.pi / 2 + 2 * math.pi / 10) and a.step_angle == np.float32(2 * math.pi / 10)
    b = S.sensor_spec(8, math.pi, 4.0)
    assert b.first_angle == np.float32(math.pi / 2) and b.step_angle == np.float32(math.pi / 7)
    cls, idx = S.decode(np.array([S.HIT_POISON | 9 << 8, 0, S.HIT_WALL | 3 << 8], np.int32))
    assert cls.tolist() == [4, 0, 1] and idx.tolist() == [9, 0, 3]


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """scan_check_main (address + undefined-behaviour sanitisers, a program of its own) scans every kind in both frames from reset-like
    and hostile states: exit status 0, sizeof(hrl_scan_spec) == the ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([sc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_scan_spec {C.sizeof(S.hrl_scan_spec)}'
    assert sc.lib().scan_sizeof_spec() == C.sizeof(S.hrl_scan_spec)
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = sc.lib().scan_check_n_cases()
    assert n == len(sums) == 6 * 2 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert sc.lib().scan_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different scans


def test_scan_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_scan_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the scan kernel and an LDS footprint under 8 KB; the header's symbols are SYMBOLS."""
    code = 'from hrl_pybullet_envs_amd.build import build_scan, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_scan(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=sc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(sc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_scan_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*scan_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) < 8192
    hdr = open(os.path.join(sc.ROOT, 'include', 'hrl_scan.h')).read()
    assert set(re.findall(r'\b(hrl_scan[a-z_]*)\s*\(', hdr)) == set(S.SYMBOLS)
    for s in S.SYMBOLS:
        assert hasattr(S.lib(), s)
