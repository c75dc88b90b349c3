"""The batched navigation field's specification (csrc/field_core.h) on the CPU: its host build (tests/field_host) against an independent
fp64 numpy reference written from include/hrl_field.h alone (tests/field_cases.py: textbook signed distances in world coordinates,
Dijkstra with heapq), schedule independence, the tie to the point probes' exact `path`, known answers, totality on hostile states, spec
validation, the sanitised stand-alone program and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_cases as fc
import orc
import probe_cases as pc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import probe_device as P
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
# metres: the worst |host build - fp64 Dijkstra on the same mask| measured over the sweep of test_host_build_equals_the_fp64_reference
# (a way of up to ninety fp32 additions that ends at 30 m, where an ulp is 1.9e-6 m)
WORST = 1.53e-5
TOL = 4 * WORST   # asserted at four times that, the siblings' convention
assert TOL <= 2e-4


def states_of(cfg, state):
    return (('shard', state), ('hand-made', fc.hand_made(cfg, state)), ('spread', fc.spread(cfg, state)))


@pytest.mark.parametrize('kind', fc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Six kinds x three modes x 8 x 8, 24 x 40, 64 x 8 and 64 x 64 cells x margin 0, 0.25 and 0.4, on the shard's states, on the hand-made
    poses and with the robots spread about the arena, the fifteen admissible source sets taken in turn (each several times per kind).

    Mask: on every cell whose reference clearances all lie further than 1e-4 m from the margin and whose centre lies further than 1e-4 m
    from every source's half-cell bound, parent == BLOCKED equals the reference's blocked mask and parent == SOURCE its source set.  At
    most 1 % of a case's cells are exempt, asserted on the reference alone first (measured: at most 0.62 % of a case, two cells of an 8 x 8
    ego grid over five envs).  The world grids have half extents 6.1, 7.7 and 9.3 about (0.13, -0.21): no contour and no default target
    runs along their cell centres or edges.

    Propagation, apart from the geometry: fp64 Dijkstra on the host build's OWN mask and source set gives the same +inf and UNREACHED
    cells exactly, dist within TOL, and a parent whose step is within TOL of the reference's best.  Measured worst |dist - reference|
    over this sweep: 1.53e-5 m (the maze kinds; 4.9e-6 .. 8.2e-6 m elsewhere); asserted at 4 x that, 6.1e-5 m.  Most Jacobi rounds: 89
    (maze), 60 .. 65 elsewhere."""
    cfg, state, items, aux = shard(kind)
    specs = [(fc.spec_of(size, mode, margin, F.ROBOT, kind=kind, centre=fc.WORLD_CENTRE), None) for mode in fc.MODES for size in fc.SIZES for margin in fc.MARGINS]
    worst, exempt_worst, rounds_worst = compare_with_the_reference(cfg, state, items, aux, specs, kind)
    print(f'kind {kind}: worst |dist - reference| {worst:.3g} m, most exempt cells {100 * exempt_worst:.2f} %, most Jacobi rounds {rounds_worst}')


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference on the given states, their hand-made poses and with the robots spread
    about the arena.  `specs`: pairs (spec, sources); sources None = the admissible source sets taken in turn.  Returns (the worst
    |dist - reference| in metres, the largest share of exempt cells of a case, the most Jacobi rounds)."""
    worst, turn, exempt_worst, rounds_worst = 0.0, 0, 0.0, 0
    for base, fixed in specs:
        for label, st in states_of(cfg, state):
            spec = base.copy()
            spec.sources = fixed if fixed is not None else fc.SOURCE_SETS[turn % len(fc.SOURCE_SETS)]
            turn += 1
            where = (tag, spec.mode, (spec.width, spec.height), spec.margin, label, spec.sources)
            refs = [fc.geometry(cfg, st[e], None if items is None else items[e], aux[e], spec) for e in range(N)]
            exempt = sum(r[2].sum() for r in refs) / (N * spec.width * spec.height)   # on the reference alone, before the build is looked at
            assert exempt <= 0.01, (where, exempt)
            exempt_worst = max(exempt_worst, exempt)
            rounds = np.zeros(N, np.int32)
            got = fc.field_host(cfg, st, items, aux, spec, rounds=rounds)
            rounds_worst = max(rounds_worst, int(rounds.max()))
            for e, (blocked, source, near) in enumerate(refs):
                par = got.parent[e]
                bad = ((par == F.BLOCKED) != blocked) & ~near
                assert not bad.any(), (where, e, 'blocked', np.argwhere(bad)[:4])
                bad = ((par == F.SOURCE) != source) & ~near
                assert not bad.any(), (where, e, 'source', np.argwhere(bad)[:4])
                worst = max(worst, fc.check_propagation(fc.Field(got.dist[e], par), spec, TOL))
    return worst, exempt_worst, rounds_worst


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its TOL, its band and its cap of 1 % exempt cells, on every entry of sensor_configs.MATRIX: a 24 x 40
    grid in the heading mode at margin 0.25 towards every source class, a 24 x 40 world grid at margin 0.4 about the entry's own arena,
    the source sets taken in turn, and the library's default spec, whose extent, blocking and sources are derived from the config
    (flagrun's open field has no walls).  On the entry's hostile states the field equals, bit for bit, that of the clean twin."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [(fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, ALL_SOURCES, kind=cfg), ALL_SOURCES),
             (fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.ROBOT, kind=cfg, centre=fc.WORLD_CENTRE), None), (F.default_spec(cfg), F.default_spec(cfg).sources)]
    worst, exempt_worst, rounds_worst = compare_with_the_reference(cfg, state, items, aux, specs, name)
    print(f'{name}: worst |dist - reference| {worst:.3g} m, most exempt cells {100 * exempt_worst:.2f} %, most Jacobi rounds {rounds_worst}')
    for spec, _ in specs[:2]:
        spec = spec.copy()
        spec.sources = ALL_SOURCES
        for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, fc.hostile):
            got = fc.field_host(cfg, s, it, a, spec)
            want = fc.field_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
            rows = [e for e in range(N) if e not in blind]
            assert fc.same(fc.Field(*(x[rows] for x in got)), fc.Field(*(x[rows] for x in want))), (name, spec.mode)
            if spec.mode != F.HRL_VIEW_WORLD:
                assert all((got.parent[e] == F.BLOCKED).all() for e in blind)


@pytest.mark.parametrize('kind', (K.HRL_ANT_MAZE, K.HRL_ANT_GATHER, K.HRL_ANT_FLAGRUN))
def test_the_schedule_does_not_matter(kind):
    """Jacobi rounds, in-place sweeps in raster order and in reverse raster order give the same bits of dist and parent: the fixed point
    is unique (csrc/field_core.h).  The sweeps need far fewer passes than Jacobi needs rounds."""
    cfg, state, items, aux = shard(kind)
    st = fc.spread(cfg, state)
    for mode in fc.MODES:
        for size in ((24, 40), (64, 64)):
            spec = fc.spec_of(size, mode, 0.25, F.ROBOT | F.TARGET | F.FOOD, kind=kind)
            r = [np.zeros(N, np.int32) for _ in range(3)]
            a, b, c = (fc.field_host(cfg, st, items, aux, spec, schedule=s, rounds=r[s]) for s in (fc.JACOBI, fc.FORWARD, fc.REVERSE))
            assert fc.same(a, b) and fc.same(a, c), (kind, mode, size)
            assert (r[0] <= size[0] * size[1]).all() and (r[1] <= r[0]).all() and (r[2] <= r[0]).all()
            assert np.isfinite(a.dist).any()


def maze_env(robots):
    cfg = orc.default_config(K.HRL_ANT_MAZE, num_envs=len(robots))
    st = np.zeros((len(robots), K.HRL_STATE_STRIDE), np.float32)
    st[:, 2], st[:, 6] = 0.55, 1.0
    st[:, 0:2] = robots
    return cfg, st, np.zeros((len(robots), K.HRL_AUX_STRIDE), np.int32)


FREE_ROBOTS = ((-2.0, -5.0), (3.0, 6.0), (-3.0, 5.0), (4.0, -8.0), (0.5, -3.0))   # the start and probe_cases.SPREAD without the robot leaning on the box


@pytest.mark.parametrize('cells', (16, 32, 64))
def test_field_brackets_the_probes_exact_path(cells):
    """Maze, blocking = WALL | BOX, sources = ROBOT, five robots standing free, cells x cells world grids of half extent 9, margins 0, 0.25
    and 0.4: at every cell centre that both the field and the host probe (probe_cases.probe_host, world frame, same margin) reach,
        path - cell <= dist <= 1.0824 path + 3 cell
    (1.0824 = the octile bound; the robot stands at most 0.71 cell from its cell's centre).  The bracket holds for the fp64 reference
    (field_cases.reference against probe_cases.ref_path) first: measured there, dist - path >= -0.48 cell (the field rounds the box's
    corners, the probe's blocking rectangle has square ones) and dist - 1.0824 path <= 1.9 cell.  From the start (-2, -5) to the cell of (-2, 4) at 64 x 64: 13.28 m at margin 0.25 and 13.84 m at 0.4, where the probe's exact
    figure is 12.84 m."""
    cfg, st, aux = maze_env(FREE_ROBOTS)
    lo_worst, hi_worst = np.inf, -np.inf
    for margin in fc.MARGINS:
        spec = fc.spec_of((cells, cells), F.HRL_VIEW_WORLD, margin, F.ROBOT, blocking=F.WALL | F.BOX, half=9.0)
        cell = fc.cell_size(spec)
        got = fc.field_host(cfg, st, None, aux, spec)
        for e in range(len(FREE_ROBOTS)):
            pos = fc.centres(st[e], spec)[0].reshape(-1, 2)
            rpath = pc.ref_path(cfg, st[e, 0:2].astype(float), pos, margin)[0]
            rdist = fc.reference(cfg, st[e], None, aux[e], spec)[0].reshape(-1)
            both = np.isfinite(rpath) & np.isfinite(rdist)
            assert both.sum() > 0.3 * cells * cells
            assert (rdist[both] >= rpath[both] - cell).all() and (rdist[both] <= 1.0824 * rpath[both] + 3 * cell).all()   # the reference alone
            lo_worst, hi_worst = min(lo_worst, ((rdist[both] - rpath[both]) / cell).min()), max(hi_worst, ((rdist[both] - 1.0824 * rpath[both]) / cell).max())
            pts = pos.astype(np.float32)[None]
            one = orc.default_config(K.HRL_ANT_MAZE, num_envs=1)
            path = pc.probe_host(one, st[e:e + 1], None, aux[e:e + 1], pc.spec_of(1, P.HRL_PROBE_WORLD, margin), pts[:, :1]).path   # (warms the binding)
            path = np.concatenate([pc.probe_host(one, st[e:e + 1], None, aux[e:e + 1], pc.spec_of(min(512, len(pos) - k), P.HRL_PROBE_WORLD, margin), pts[:, k:k + 512]).path[0]
                                   for k in range(0, len(pos), 512)])
            dist = got.dist[e].reshape(-1)
            both = np.isfinite(path) & np.isfinite(dist)
            assert both.sum() > 0.3 * cells * cells
            assert (dist[both] >= path[both] - cell).all(), (margin, e, (dist[both] - path[both]).min() / cell)
            assert (dist[both] <= 1.0824 * path[both] + 3 * cell).all(), (margin, e, ((dist[both] - 1.0824 * path[both]) / cell).max())
        if cells == 64 and margin > 0:
            row, col = (int(x[0, 0]) for x in F.cell_index(spec, _t(st[:1]), _t(np.array([[[-2.0, 4.0]]], np.float32))))
            assert abs(float(got.dist[0, row, col]) - {0.25: 13.28, 0.4: 13.84}[margin]) < 0.01
    print(f'{cells} x {cells}: reference dist - path >= {lo_worst:.3f} cell, dist - 1.0824 path <= {hi_worst:.3f} cell')


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def gather_env(robot, food=(), poison=()):
    """One gather env with the robot at `robot`, food and poison where given; every other item far away, as an eaten one."""
    cfg = orc.default_config(K.HRL_ANT_GATHER, num_envs=1)
    assert len(food) <= cfg.n_food and len(poison) <= cfg.n_poison
    st = np.zeros((1, K.HRL_STATE_STRIDE), np.float32)
    st[0, 0:2], st[0, 2], st[0, 6] = robot, 0.55, 1.0
    items = np.zeros((1, shard(K.HRL_ANT_GATHER)[2].shape[1]), np.float32)
    items[0, :2 * (cfg.n_food + cfg.n_poison)] = np.tile((100.0, 0.0), cfg.n_food + cfg.n_poison)
    for i, p in enumerate(food):
        items[0, 2 * i:2 * i + 2] = p
    for i, p in enumerate(poison):
        items[0, 2 * (cfg.n_food + i):2 * (cfg.n_food + i) + 2] = p
    return cfg, st, items, np.zeros((1, K.HRL_AUX_STRIDE), np.int32)


def test_known_answers():
    """Cells of 0.25 m (64 columns, half extent 8; 8 or 16 columns, half extent 1 or 2), so cell centres lie at odd multiples of 0.125 m.

    An empty arena with one source: the octile distance w1 (max - min) + w2 min in cell steps -- bit for bit the fp32 lattice sum
    D[a][b] = min(fl(D[a-1][b] + w2), fl(D[a][b-1] + w1)) over a diagonal and b straight steps.  A wall of poison with a one-cell gap:
    every way leads through the gap.  A source fenced in by poison: UNREACHED outside the fence.  A source on a cell edge, on a cell
    corner and outside the grid: two, four and no source cells."""
    cfg, st, items, aux = gather_env((0.125, -0.375))
    spec = fc.spec_of((64, 48), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, blocking=F.WALL, half=8.0)
    got = fc.field_host(cfg, st, items, aux, spec)
    w1, w2 = np.float32(0.25), np.float32(0.25) * np.float32(1.41421354)
    lat = np.zeros((64, 64), np.float32)   # lat[a][b]
    for a in range(64):
        for b in range(64):
            if a or b:
                lat[a, b] = min(lat[a - 1, b] + w2 if a else np.inf, lat[a, b - 1] + w1 if b else np.inf)
    r0, c0 = np.argwhere(got.parent[0] == F.SOURCE)[0]
    assert (got.parent[0] == F.SOURCE).sum() == 1 and (r0, c0) == (25, 32)   # v = 5.875 - 0.25 row, u = -7.875 + 0.25 col
    rows, cols = np.abs(np.arange(48) - r0)[:, None], np.abs(np.arange(64) - c0)[None, :]
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    inside = got.parent[0] != F.BLOCKED
    assert inside.sum() == 48 * 58   # the planes at +-7.45 grown by 0.25 leave columns 3..60 (|u| <= 7.125)
    assert np.array_equal(got.dist[0][inside].view(np.uint32), lat[lo, hi - lo][inside].view(np.uint32))
    assert np.abs(got.dist[0][inside] - (0.25 * (hi - lo) + 0.25 * math.sqrt(2) * lo)[inside]).max() <= TOL
    assert (got.parent[0][r0, c0 + 1:61] == 4).all() and (got.parent[0][r0 + 1:, c0] == 2).all() and got.parent[0][r0 + 3, c0 + 3] == 3   # W, N, NW lead back

    # a wall of poison along the column u = 0.125 of an 8 x 8 grid, rows 0..7 but row 5; the robot (the source) to its left
    cell, gap, rows_in = 0.25, 5, range(8)
    ys = [0.875 - cell * i for i in rows_in]
    cfg, st, items, aux = gather_env((-0.625, -0.625), poison=[(0.125, y) for i, y in enumerate(ys) if i != gap])
    spec = fc.spec_of((8, 8), F.HRL_VIEW_WORLD, 0.1, F.ROBOT, blocking=F.POISON, half=1.0)
    got = fc.field_host(cfg, st, items, aux, spec)
    n, wall = len(rows_in), spec.width // 2
    par, dist = got.parent[0], got.dist[0]
    assert [int(par[i, wall]) == F.BLOCKED for i in rows_in] == [i != gap for i in rows_in] and (par == F.BLOCKED).sum() == n - 1
    assert np.isfinite(dist[par != F.BLOCKED]).all()
    src = np.argwhere(par == F.SOURCE)[0]
    for i in rows_in:   # every way from the right of the wall leads through the gap: no corner is cut, so it enters and leaves the gap along its row
        j = n - 1
        steps = fc.follow(par, i, j, n * n)
        assert steps > 0
        r, c, seen = i, j, False
        while par[r, c] != F.SOURCE:
            seen |= (r, c) == (gap, wall)
            k = int(par[r, c])
            r, c = r + F.DIRECTIONS[k][1], c + F.DIRECTIONS[k][0]
        assert seen and (r, c) == tuple(src)
    assert par[gap, wall] == 4 and par[gap, wall + 1] == 4   # W, W

    # a food source fenced in by eight poison squares; the robot outside is no source
    ring = [(0.125 + cell * dc, 0.125 + cell * dr) for dc in (-1, 0, 1) for dr in (-1, 0, 1) if dc or dr]
    cfg, st, items, aux = gather_env((0.9, 0.9), food=[(0.125, 0.125)], poison=ring)
    spec = fc.spec_of((8, 8), F.HRL_VIEW_WORLD, 0.1, F.FOOD, blocking=F.POISON, half=1.0)
    got = fc.field_host(cfg, st, items, aux, spec)
    par = got.parent[0]
    assert (par == F.SOURCE).sum() == 1 and par[3, 4] == F.SOURCE and (par == F.BLOCKED).sum() == 8 and (par == F.UNREACHED).sum() == 64 - 9
    assert np.isinf(got.dist[0][par != F.SOURCE]).all() and got.dist[0][3, 4] == 0
    # ... and reached once the robot's cell is a source too; a blocked source cell stays a source (the fence's corner)
    spec.sources = F.FOOD | F.POISON
    par = fc.field_host(cfg, st, items, aux, spec).parent[0]
    assert (par == F.SOURCE).sum() == 9 and (par < 8).sum() == 64 - 9

    # ties: food on a cell edge, on a cell corner, and outside the grid
    for food, cells_ in (((0.25, 0.125), {(3, 4), (3, 5)}), ((0.125, 0.5), {(2, 4), (1, 4)}), ((0.25, 0.25), {(3, 4), (3, 5), (2, 4), (2, 5)}), ((1.2, 0.1), set()),
                         ((1.0, 0.125), {(3, 7)})):   # (on the grid's own edge: the last column's half-cell bound)
        cfg, st, items, aux = gather_env((0.9, 0.9), food=[food])
        spec = fc.spec_of((8, 8), F.HRL_VIEW_WORLD, 0.0, F.FOOD, blocking=F.WALL, half=1.0)
        got = fc.field_host(cfg, st, items, aux, spec)
        assert {tuple(int(v) for v in x) for x in np.argwhere(got.parent[0] == F.SOURCE)} == cells_, food
        if not cells_:
            assert (got.parent[0] == F.UNREACHED).all() and np.isinf(got.dist[0]).all()
        else:
            assert np.isfinite(got.dist[0]).all() and got.dist[0].max() > 1.0


ALL_SOURCES = F.ROBOT | F.FOOD | F.POISON | F.TARGET


@pytest.mark.parametrize('kind', fc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range: the field equals, bit for
    bit, that of the same env with that shape where it touches no cell (an eaten item's place; no goal; a far target).  A robot at a
    non-finite place blocks every cell in the ego modes; in the world mode it is no source and the grid is computed about the world's
    origin: the field of a robot at (0, 0) that is no source.  A NaN quaternion leaves the heading mode with the ego mode's field."""
    cfg, state, items, aux = shard(kind)
    for mode in fc.MODES:
        for size, margin in (((24, 40), 0.4), ((64, 64), 0.0)):
            spec = fc.spec_of(size, mode, margin, ALL_SOURCES, kind=kind)
            for s, it, a, cs, cit, ca, far, blind in fc.hostile(cfg, state, items, aux):
                got = fc.field_host(cfg, s, it, a, spec)
                want = fc.field_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec)
                rows = [e for e in range(N) if e not in blind]
                assert fc.same(fc.Field(*(x[rows] for x in got)), fc.Field(*(x[rows] for x in want))), (kind, mode, size)
                for e in blind:
                    if mode != F.HRL_VIEW_WORLD:
                        assert (got.parent[e] == F.BLOCKED).all() and np.isinf(got.dist[e]).all()
                    else:
                        z = cs.copy()
                        z[e, 0:2] = 0.0
                        nosrc = spec.copy()
                        nosrc.sources = ALL_SOURCES & ~F.ROBOT
                        w = fc.field_host(cfg, z, cit, ca, nosrc)
                        assert fc.same(fc.Field(got.dist[e], got.parent[e]), fc.Field(w.dist[e], w.parent[e])), (kind, size, e)
                        only = spec.copy()
                        only.sources = F.ROBOT   # the robot alone: no source at all
                        g2 = fc.field_host(cfg, s, it, a, only)
                        assert np.isin(g2.parent[e], (F.UNREACHED, F.BLOCKED)).all() and np.isinf(g2.dist[e]).all() and ((got.parent[e] == F.BLOCKED) <= (g2.parent[e] == F.BLOCKED)).all()
    s = state.copy(); s[:, 3:7] = np.nan
    a, b = (fc.field_host(cfg, s, items, aux, fc.spec_of((24, 40), m, 0.25, ALL_SOURCES, kind=kind)) for m in (F.HRL_VIEW_EGO, F.HRL_VIEW_EGO_HEADING))
    assert fc.same(a, b)


def test_none_members_and_a_mask_leave_the_other_bytes_alone():
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    spec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, F.TARGET | F.ROBOT, kind=K.HRL_ANT_MAZE)
    full = fc.field_host(cfg, state, items, aux, spec)
    for want in (('dist',), ('parent',)):
        part = fc.field_host(cfg, state, items, aux, spec, want=want)
        for name, x, y in zip(fc.NAMES, part, full):
            assert (x is None) if name not in want else np.array_equal(x, y), (want, name)
    out = fc.Field(np.full((N, 40, 24), -7, np.float32), np.full((N, 40, 24), 77, np.uint8))
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    fc.field_host(cfg, state, items, aux, spec, mask=mask, out=out)
    for e in range(N):
        assert (np.array_equal(out.dist[e], full.dist[e]) and np.array_equal(out.parent[e], full.parent[e])) if mask[e] else ((out.dist[e] == -7).all() and (out.parent[e] == 77).all())


def test_blocking_and_source_subsets_compose():
    """More obstacles never shorten a way and never free a cell; the field of a union of source sets is the cell-wise minimum of the
    single sets' fields (within rounding: the same ways, summed from another end)."""
    for kind in (K.HRL_ANT_GATHER, K.HRL_ANT_MAZE):
        cfg, state, items, aux = shard(kind)
        st = fc.spread(cfg, state)
        few = fc.field_host(cfg, st, items, aux, fc.spec_of((64, 64), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, blocking=F.WALL, kind=kind))
        many = fc.field_host(cfg, st, items, aux, fc.spec_of((64, 64), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, blocking=F.ALL, kind=kind))
        assert (many.dist >= few.dist).all() and ((few.parent == F.BLOCKED) <= (many.parent == F.BLOCKED)).all() and (many.dist > few.dist).any()
        singles = [fc.field_host(cfg, st, items, aux, fc.spec_of((64, 64), F.HRL_VIEW_WORLD, 0.25, b, kind=kind)) for b in fc.SOURCE_BITS]
        union = fc.field_host(cfg, st, items, aux, fc.spec_of((64, 64), F.HRL_VIEW_WORLD, 0.25, ALL_SOURCES, kind=kind))
        low = np.minimum.reduce([x.dist for x in singles])
        ok = np.isfinite(low)
        blocked_everywhere = np.logical_and.reduce([x.parent == F.BLOCKED for x in singles])
        assert np.array_equal(np.isfinite(union.dist), ok) and np.abs(union.dist[ok] - low[ok]).max() <= TOL and np.array_equal(union.parent == F.BLOCKED, blocked_everywhere)


BAD_SPECS = [('width', 0), ('width', 4), ('width', 12), ('width', 72), ('height', 0), ('height', 4), ('height', 12), ('height', 72), ('mode', 3), ('mode', -1),
             ('blocking', 0), ('blocking', 32), ('blocking', 64), ('sources', 0), ('sources', F.ROBOT | F.WALL), ('sources', F.BOX), ('sources', 64),
             ('margin', float('nan')), ('margin', -1.0), ('margin', 3.0), ('half_extent', 0.0), ('half_extent', float('nan')), ('half_extent', float('inf')),
             ('half_extent', 1e-3), ('half_extent', 2e4), ('struct_size', 16), ('struct_size', 0), ('out', None)]
REASONS = {'width': 'width must be a multiple of 8', 'height': 'height must be a multiple of 8', 'mode': 'unknown field mode', 'blocking': 'blocking must be a non-empty mask',
           'sources': 'sources must be a non-empty mask', 'margin': 'margin must be finite', 'half_extent': 'half_extent must be finite', 'struct_size': 'struct_size is not sizeof',
           'out': 'holds no pointer'}


@pytest.mark.parametrize('field,value', BAD_SPECS)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.ROBOT, kind=K.HRL_ANT_FLAT)
    out = fc.Field(np.full((N, 80, 80), -7, np.float32), np.full((N, 80, 80), 77, np.uint8))
    handed = out
    if field == 'out':
        handed = fc.Field(None, None)
    else:
        setattr(spec, field, value)
    code, why = fc.field_host(cfg, state, items, aux, spec, out=handed, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and REASONS[field] in why
    assert (out.dist == -7).all() and (out.parent == 77).all()
    # the device library runs the same checks before it looks for a device
    L = F.lib()
    b = K.make_buffers(fc.ptr(state), fc.ptr(items), fc.ptr(aux), None, None, None, None, None)
    o = F.hrl_field_out(**{name: fc.ptr(a) for name, a in zip(fc.NAMES, handed)})
    assert L.hrl_field(C.byref(cfg), C.byref(b), C.byref(spec), None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
    assert why.encode() in L.hrl_field_last_error()
    assert (out.dist == -7).all() and (out.parent == 77).all()


def test_default_spec_and_the_mirrors():
    from hrl_pybullet_envs_amd import render_device as R
    want_sources = {K.HRL_ANT_FLAT: F.ROBOT, K.HRL_ANT_GATHER: F.FOOD, K.HRL_POINT_GATHER: F.FOOD, K.HRL_ANT_MAZE: F.TARGET, K.HRL_ANT_MAZE_MJ: F.TARGET, K.HRL_ANT_FLAGRUN: F.TARGET}
    for kind in fc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, mode in F.MODES.items():
            s, h, v = F.default_spec(cfg, name), F.hrl_field_spec(), R.default_view(cfg, mode)
            assert fc.lib().field_host_default_spec(C.byref(cfg), mode, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.struct_size, s.width, s.height, s.mode) == (C.sizeof(F.hrl_field_spec), 64, 64, mode)
            assert (s.half_extent, tuple(s.centre)) == (v.half_extent, tuple(v.centre)) and (v.width, v.height) == (64, 64)
            assert s.blocking == F.WALL | F.BOX | F.POISON and s.sources == want_sources[kind]
            assert s.margin == np.float32(0.35 if kind == K.HRL_POINT_GATHER else 0.25)
            assert fc.lib().field_validate_spec(C.byref(s)) == b''
    s = F.default_spec(cfg, 'ego', 24, 40)
    assert (s.width, s.height, s.mode) == (24, 40, 1) and F.default_spec(cfg).mode == F.HRL_VIEW_WORLD
    assert F.default_spec(cfg, 'world', 64, 32).half_extent == 2 * F.default_spec(cfg).half_extent
    with pytest.raises(ValueError):
        F.default_spec(cfg, 'sideways')
    assert fc.lib().field_sizeof_spec() == C.sizeof(F.hrl_field_spec) and fc.lib().field_sizeof_out() == C.sizeof(F.hrl_field_out)
    assert F.Field() == (None, None) and F.Field._fields == fc.NAMES
    assert (F.ROBOT, F.SOURCE, F.UNREACHED, F.BLOCKED) == (32, 8, 9, 10) and len(F.DIRECTIONS) == 8 and F.DIRECTIONS[2] == (0, -1)


def test_helpers_agree_with_the_grid():
    """cell_index() names the cell whose centre the host build puts a source on, in the three modes; direction_vectors() are the unit
    steps between neighbouring cell centres in world axes."""
    cfg, state, items, aux = shard(K.HRL_ANT_GATHER)
    st = fc.hand_made(cfg, state)
    for mode in fc.MODES:
        spec = fc.spec_of((24, 40), mode, 0.0, F.ROBOT, blocking=F.WALL, kind=K.HRL_ANT_GATHER, centre=(0.3, -0.2))
        got = fc.field_host(cfg, st, items, aux, spec)
        row, col = F.cell_index(spec, _t(st), _t(st[:, None, 0:2]))
        dv = F.direction_vectors(spec, _t(st)).numpy()
        assert dv.shape == (N, 8, 2) and np.allclose(np.linalg.norm(dv, axis=2), 1.0, atol=1e-6)
        for e in range(N):
            r, c = int(row[e, 0]), int(col[e, 0])
            src = {tuple(int(v) for v in x) for x in np.argwhere(got.parent[e] == F.SOURCE)}
            assert (r, c) in src and len(src) == (1 if mode == F.HRL_VIEW_WORLD else 4), (mode, e)   # (an ego grid's robot stands on a cell corner)
            pos = fc.centres(st[e], spec)[0]
            for k, (dc, dr) in enumerate(F.DIRECTIONS):
                step = pos[20 + dr, 12 + dc] - pos[20, 12]
                assert np.allclose(step / np.linalg.norm(step), dv[e, k], atol=1e-5), (mode, e, k)
    assert F.cell_index(spec, _t(st), _t(np.full((N, 1, 2), np.nan, np.float32)))[0].eq(-1).all()


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """field_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the field of every kind in the three
    modes from reset-like and hostile states under the three schedules: exit status 0, sizeof(hrl_field_spec) == the ctypes mirror's,
    checksums == the unsanitised host build's."""
    p = subprocess.run([fc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_field_spec {C.sizeof(F.hrl_field_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = fc.lib().field_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert fc.lib().field_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different fields


def test_field_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_field_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the field kernel and an LDS footprint of at most 40 KB (four workgroups per CU); the header's symbols are SYMBOLS."""
    code = 'from hrl_pybullet_envs_amd.build import build_field, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_field(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=fc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(fc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_field_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*field_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 40960
    hdr = open(os.path.join(fc.ROOT, 'include', 'hrl_field.h')).read()
    assert set(re.findall(r'\b(hrl_field(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_field_out', 'hrl_field_spec'} == set(F.SYMBOLS)
    for s in F.SYMBOLS:
        assert hasattr(F.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert [name for name, *_ in build.SENSORS] == ['render', 'scan', 'probe', 'field']   # built fifth, after the probes: build() walks the table behind the step library
