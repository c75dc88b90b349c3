"""The batched renderer's specification (csrc/render_core.h) on the CPU: its host build (tests/render_host) against an independent fp64
numpy reference written from include/hrl_render.h alone (tests/render_cases.py), the invariants of the picture, totality on hostile
states, the sanitised stand-alone program, view validation and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import orc
import render_cases as rc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import render_device as R

N = 5
ROBOT = [R.PALETTE[k] for k in ('leg0', 'leg1', 'leg2', 'torso')]


@functools.lru_cache(None)
def shard(kind):
    """(cfg, state, items, aux) of 5 envs on the CPU oracle: reset + 30 random-action steps.  Computed once, never modified."""
    cfg = orc.default_config(kind, num_envs=N, seed=11 + kind, auto_reset=1)
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    rng = np.random.RandomState(100 + kind)
    for _ in range(30):
        o.step(rng.uniform(-1, 1, (N, o.ad)))
    assert np.abs(o.state[:, :2]).max() <= 8.0
    for a in (o.state, o.items, o.aux):
        a.setflags(write=False)
    return cfg, o.state, o.items, o.aux


def is_colour(img, cols):
    m = np.zeros(img.shape[:-1], bool)
    for c in cols:
        m |= (img == np.array(c, np.uint8)).all(-1)
    return m


@pytest.mark.parametrize('kind', rc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Every pixel of every env, mode and size equals the fp64 reference, except pixels whose centre lies within 1e-4 m of the boundary
    of a drawn shape in the reference (two orders above what < 32 fp32 operations lose on coordinates below 16 m, three below the
    coarsest pixel); those are at most 0.5 % of any image."""
    cfg, state, items, aux = shard(kind)
    compare_with_the_reference(cfg, state, items, aux, [rc.view_of(kind, mode, size) for mode in rc.MODES for size in rc.SIZES], kind)


def compare_with_the_reference(cfg, state, items, aux, views, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states and their hand-made poses; returns the largest
    share of exempt pixels of an image."""
    worst = 0.0
    for st in (state, rc.hand_made(cfg, state)):
        for v in views:
            where = (tag, v.mode, v.width, v.height)
            img = rc.render_host(cfg, st, items, aux, v)
            for e in range(N):
                ref, near = rc.reference(cfg, st[e], items[e], aux[e], v)
                worst = max(worst, float(near.mean()))
                assert near.mean() <= 0.005, (where, e, near.mean())
                diff = (img[e] != ref).any(-1) & ~near
                assert not diff.any(), (where, e, np.argwhere(diff)[:4])
                assert len(np.unique(ref.reshape(-1, 3), axis=0)) >= 2   # the picture is not blank
    return worst


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its band and its cap of 0.5 %, on every entry of sensor_configs.MATRIX: the heading mode at 48 x 32, the
    world mode at 32 x 32 about the entry's own arena and the library's default view, whose extent is derived from the config (flagrun's
    open field has no walls to derive it from).  On the entry's hostile states the picture equals, byte for byte, that of the clean
    twin.  On the entries of 64 items the two items moved next to the robot (indices 50 and 63) are painted in the heading view."""
    cfg, state, items, aux = scfg.shard(name)
    views = [rc.view_of(cfg, R.HRL_VIEW_EGO_HEADING, (48, 32)), rc.view_of(cfg, R.HRL_VIEW_WORLD, (32, 32)), R.default_view(cfg, 'world')]
    worst = compare_with_the_reference(cfg, state, items, aux, views, name)
    print(f'{name}: at most {100 * worst:.3f} % of an image exempt')
    for s, it, a, cs, cit, ca, far, _ in scfg.hostile(name, rc.hostile):
        for v in views[1:]:
            assert np.array_equal(rc.render_host(cfg, s, it, a, v), rc.render_host(rc.far_targets(cfg) if far else cfg, cs, cit, ca, v)), (name, v.width)
    if scfg.many_items(cfg):
        gone = np.array(items)
        for e, i, _ in scfg.NEAR_ITEMS:
            gone[e, 2 * (i % (cfg.n_food + cfg.n_poison)):][:2] = (100.0, 0.0)
        a, b = rc.render_host(cfg, state, items, aux, views[0]), rc.render_host(cfg, state, gone, aux, views[0])
        assert all((a[e] != b[e]).any() for e, _, _ in scfg.NEAR_ITEMS) and all(np.array_equal(a[e], b[e]) for e in (0, 2, 4))


@pytest.mark.parametrize('kind', rc.KINDS)
def test_ego_modes_centre_on_the_robot_and_heading_mode_turns_with_it(kind):
    cfg, state, items, aux = shard(kind)
    turned = rc.yawed(state, items, cfg, 0.9)
    for size in rc.SIZES:
        w, h = size
        for mode in (R.HRL_VIEW_EGO, R.HRL_VIEW_EGO_HEADING):
            img = rc.render_host(cfg, state, items, aux, rc.view_of(kind, mode, size))
            assert (img[:, h // 2, w // 2] == np.array(R.PALETTE['torso'], np.uint8)).all()
        v = rc.view_of(kind, R.HRL_VIEW_EGO_HEADING, size)
        a, b = rc.render_host(cfg, state, items, aux, v), rc.render_host(cfg, turned, items, aux, v)
        assert np.array_equal(is_colour(a, ROBOT), is_colour(b, ROBOT))
        assert is_colour(a, ROBOT).reshape(N, -1).sum(1).min() > 4
    # the heading fallback: a torso whose X axis points straight up has no heading -- world axes
    s = state.copy()
    s[:, 3:7] = (0, -np.sqrt(0.5), 0, np.sqrt(0.5))
    v = rc.view_of(kind, R.HRL_VIEW_EGO_HEADING, (32, 32))
    e = rc.view_of(kind, R.HRL_VIEW_EGO, (32, 32))
    assert np.array_equal(rc.render_host(cfg, s, items, aux, v), rc.render_host(cfg, s, items, aux, e))


def regions(mask):
    """4-connected regions of a boolean image."""
    seen, n = np.zeros_like(mask), 0
    for i, j in np.argwhere(mask):
        if seen[i, j]:
            continue
        n += 1
        stack = [(i, j)]
        seen[i, j] = True
        while stack:
            a, b = stack.pop()
            for p, q in ((a + 1, b), (a - 1, b), (a, b + 1), (a, b - 1)):
                if 0 <= p < mask.shape[0] and 0 <= q < mask.shape[1] and mask[p, q] and not seen[p, q]:
                    seen[p, q] = True
                    stack.append((p, q))
    return n


def test_food_regions_equal_the_food_items_in_sight():
    """World mode at 256 x 256 (an item is four pixels wide): one food-coloured region per food item that lies in the arena and clear of
    the robot; an eaten item at (100, 0) falls outside the image, one under the torso is painted over."""
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    it = items.copy()
    expect = []
    for e in range(N):
        food = [(-5.0 + 1.7 * i, 5.0 - 1.5 * ((i + e) % 3)) for i in range(cfg.n_food)]
        food[1] = (100.0, 0.0)
        food[2] = (float(state[e, 0]) + 0.02, float(state[e, 1]) - 0.03)
        for i, (x, y) in enumerate(food):
            it[e, 2 * i:2 * i + 2] = (x, y)
        for k in range(cfg.n_poison):
            it[e, 2 * (cfg.n_food + k):2 * (cfg.n_food + k) + 2] = (-2.0 + 0.6 * k, -6.5)
        clear = [k for k, (x, y) in enumerate(food) if k not in (1, 2) and np.hypot(x - state[e, 0], y - state[e, 1]) > 1.6]
        assert len(clear) + 2 == cfg.n_food, 'every food item is either clear of the robot or one of the two special ones'
        expect.append(len(clear))
    v = rc.view_of(K.HRL_ANT_GATHER, R.HRL_VIEW_WORLD, (256, 256))
    img = rc.render_host(cfg, state, it, aux, v)
    for e in range(N):
        assert regions(is_colour(img[e], [R.PALETTE['food']])) == expect[e]
        ref, near = rc.reference(cfg, state[e], it[e], aux[e], v)
        assert not ((img[e] != ref).any(-1) & ~near).any()


def test_a_mask_leaves_the_other_images_alone():
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    v = rc.view_of(K.HRL_ANT_MAZE, R.HRL_VIEW_WORLD, (48, 32))
    full = rc.render_host(cfg, state, items, aux, v)
    out = np.full_like(full, 0xAB)
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    rc.render_host(cfg, state, items, aux, v, mask=mask, out=out)
    for e in range(N):
        assert np.array_equal(out[e], full[e]) if mask[e] else (out[e] == 0xAB).all()


@pytest.mark.parametrize('kind', rc.KINDS)
def test_hostile_states_draw_the_picture_without_the_offending_shape(kind):
    """NaN, +-inf and 1e20 in the robot's position, an item or the flagrun goal, and target indices out of range: the image equals the
    one of the same env with that shape moved out of sight; nothing else changes."""
    cfg, state, items, aux = shard(kind)
    for s, it, a, cs, cit, ca, far in rc.hostile(cfg, state, items, aux):
        for mode in (R.HRL_VIEW_WORLD,) if not far else rc.MODES:
            v = rc.view_of(kind, mode, (48, 32))
            got = rc.render_host(cfg, s, it, a, v)
            want = rc.render_host(rc.far_targets(cfg) if far else cfg, cs, cit, ca, v)
            assert np.array_equal(got, want), (kind, mode)
        # the ego modes centre on the robot: a robot at a NaN place has no view, the picture is bare ground
        for mode in (R.HRL_VIEW_EGO, R.HRL_VIEW_EGO_HEADING):
            if not far and np.isnan(s[0, 0]):
                got = rc.render_host(cfg, s, it, a, rc.view_of(kind, mode, (32, 32)))
                assert (got[0] == np.array(R.PALETTE['ground'], np.uint8)).all()
    # no robot layers at all where the robot's x is NaN
    s = state.copy(); s[:, 0] = np.nan
    got = rc.render_host(cfg, s, items, aux, rc.view_of(kind, R.HRL_VIEW_WORLD, (32, 32)))
    assert not is_colour(got, ROBOT).any()


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """render_check_main (address + undefined-behaviour sanitisers, a program of its own) renders every kind in every mode from reset-like
    and hostile states: exit status 0, sizeof(hrl_view) == the ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([rc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_view {C.sizeof(R.hrl_view)}'
    assert rc.lib().render_sizeof_view() == C.sizeof(R.hrl_view)
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = rc.lib().render_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert rc.lib().render_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different pictures


BAD_VIEWS = [('width', 40), ('width', 0), ('width', 272), ('height', 0), ('height', 24), ('half_extent', float('nan')), ('half_extent', 0.0),
             ('half_extent', -1.0), ('half_extent', float('inf')), ('mode', 3), ('mode', -1), ('struct_size', 24), ('struct_size', 0)]


@pytest.mark.parametrize('field,value', BAD_VIEWS)
def test_bad_views_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    v = rc.view_of(K.HRL_ANT_FLAT, R.HRL_VIEW_WORLD, (32, 32))
    setattr(v, field, value)
    out = np.full((N, 32, 32, 3), 0xAB, np.uint8)
    code, why = rc.render_host(cfg, state, items, aux, v, out=out, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and why
    assert (out == 0xAB).all()
    # the device library runs the same checks before it looks for a device
    L = R.lib()
    b = K.make_buffers(rc.ptr(state), rc.ptr(items), rc.ptr(aux), None, None, None, None, None)
    assert L.hrl_render(C.byref(cfg), C.byref(b), C.byref(v), None, rc.ptr(out), None) == K.HRL_ERR_BAD_ARG
    assert why.encode() in L.hrl_render_last_error()


def test_default_views():
    for kind in rc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        want = {K.HRL_ANT_FLAT: 6.0, K.HRL_ANT_GATHER: 7.5, K.HRL_POINT_GATHER: 7.5, K.HRL_ANT_MAZE: 9.0, K.HRL_ANT_MAZE_MJ: 9.0, K.HRL_ANT_FLAGRUN: 6.0}[kind]
        for mode in rc.MODES:
            v, h = R.default_view(cfg, mode), R.hrl_view()
            assert rc.lib().render_host_default_view(C.byref(cfg), mode, C.byref(h)) == 0 and bytes(v) == bytes(h)
            assert (v.struct_size, v.width, v.height, v.mode) == (C.sizeof(R.hrl_view), 64, 64, mode)
            assert v.half_extent == (want if mode == R.HRL_VIEW_WORLD else 3.0) and tuple(v.centre) == (0.0, 0.0)
    assert R.default_view(cfg, 'ego', 48, 32).width == 48
    assert R.default_view(orc.default_config(K.HRL_ANT_MAZE), 'world', 64, 32).half_extent == 18.0   # 9 m up and down still fit
    with pytest.raises(ValueError):
        R.default_view(cfg, 'sideways')


def test_render_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_render_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch for the
    render kernel, and an LDS footprint well under the step kernel's 31 KB."""
    code = 'from hrl_pybullet_envs_amd.build import build_render, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_render(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=rc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(rc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_render_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*render_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) < 8192
    hdr = open(os.path.join(rc.ROOT, 'include', 'hrl_render.h')).read()
    assert set(re.findall(r'\b(hrl_render[a-z_]*)\s*\(', hdr)) == set(R.SYMBOLS)
    for s in R.SYMBOLS:
        assert hasattr(R.lib(), s)
