"""The batched routes' specification (csrc/route_core.h) on the CPU: its host build (tests/route_host) against an independent reference
written from include/hrl_route.h alone (tests/route_cases.py: `clear` by exact rational segment-square intersection, chain and pull in
plain Python on the field's parent, fp64 lengths), the header's integer inequality against that intersection on every pair of cells,
properties, known answers, truncation, totality on hostile states and starts, spec validation, the sanitised stand-alone program and the
gfx950 cross-compile.  No GPU."""
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
import route_cases as rt
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import probe_device as P
from hrl_pybullet_envs_amd import route_device as R
from test_field_host import TOL as FIELD_TOL   # how far the field's fp32 dist may lie from its fp64 sum
from test_field_host import gather_env, maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
# metres: the worst |host build - fp64 sum| of `length` measured over the sweep of test_host_build_equals_the_reference (at most 32 fp32
# additions of fl(cell * sqrtf(n)) that end below 30 m, where an ulp is 1.9e-6 m)
WORST = 1.36e-6
TOL = 4 * WORST   # asserted at four times that, the siblings' convention
assert TOL <= 2e-4


def states_of(cfg, state):
    return (('shard', state), ('hand-made', fc.hand_made(cfg, state)), ('spread', fc.spread(cfg, state)))


def test_the_integer_inequality_is_the_exact_intersection():
    """Every pair of cells a, b of an 8 x 8 grid and every cell c of it: the header's inequality (for c in the bounding box; no cell outside
    it is met) says what the exact rational intersection of the segment a b with the closed square of c says; the reference's row-wise
    `touched` says the same; and so do the host build's masks of touched columns, row by row."""
    L = rt.lib()
    for a in np.ndindex(8, 8):
        for b in np.ndindex(8, 8):
            ri, rj = rt.touched(b[0] - a[0], b[1] - a[1])
            fast = set(zip((ri + a[0]).tolist(), (rj + a[1]).tolist()))
            lo, hi = (min(a[0], b[0]), min(a[1], b[1])), (max(a[0], b[0]), max(a[1], b[1]))
            exact = set()
            for c in np.ndindex(8, 8):
                inside = lo[0] <= c[0] <= hi[0] and lo[1] <= c[1] <= hi[1]
                m = rt.meets(a, b, c)
                assert m == (inside and rt.inequality(a, b, c)), (a, b, c)
                if m:
                    exact.add(c)
            assert exact == {c for c in fast if 0 <= c[0] < 8 and 0 <= c[1] < 8} and fast <= {(i, j) for i in range(lo[0], hi[0] + 1) for j in range(lo[1], hi[1] + 1)}, (a, b)
            for i in range(8):
                mask = L.route_row_touch(a[0], a[1], b[0], b[1], i)
                assert {(i, j) for j in range(64) if mask >> j & 1} == {c for c in exact if c[0] == i}, (a, b, i)
    rng = np.random.RandomState(3)   # and the two ways the host build decides clear, on random blocked cells of a 64-row grid
    for _ in range(600):
        rows = (C.c_ulonglong * 64)(*[int(x) for x in rng.randint(0, 2 ** 62, 64) & rng.randint(0, 2 ** 62, 64) & rng.randint(0, 2 ** 62, 64)])
        i0, j0, i1, j1 = (int(x) for x in rng.randint(0, 64, 4))
        got = L.route_clear(rows, 64, i0, j0, i1, j1)
        assert got in (0, 3), (i0, j0, i1, j1)
        blocked = np.array([[rows[i] >> j & 1 for j in range(64)] for i in range(64)], bool)
        assert (got == 3) == rt.clear(blocked, (i0, j0), (i1, j1))


def check_properties(ref, blocked, parent, dist, size, length, tol):
    """What holds for every route: of the reference `ref` with its own fp64 length, or with the build's `length` in its place."""
    if ref.count == 0:
        return
    for a, b in zip(ref.way, ref.way[1:]):
        assert rt.clear(blocked, a, b)
    a, b = ref.way[0], ref.way[-1]
    assert size * math.hypot(b[0] - a[0], b[1] - a[1]) - tol <= length <= float(dist[a]) + tol
    assert ref.count <= ref.steps + 1 and parent[b] == F.SOURCE


@pytest.mark.parametrize('kind', rt.KINDS)
def test_host_build_equals_the_reference(kind):
    """Six kinds x three modes x 8 x 8, 24 x 40 and 64 x 64 cells on the shard's states, the hand-made poses and the robots spread about
    the arena; the frames, P in (1, 5, 64), K in (2, 7, 32) and the source sets taken in turn; every third case has starts = None.  The
    starts lie at most 0.3 cell from a cell's centre, some outside the grid (asserted on the reference alone: none within 1e-4 m of an
    edge between cells).

    count and cells equal the reference run on field_cases.field_host's parent exactly, no cell exempt; waypoints equal the fp64 cell
    centres to fp32's precision at that magnitude; length equals the fp64 sum within TOL.  Measured worst |length - reference| over
    this sweep: 1.36e-6 m (the maze kind; 4.6e-7 .. 1.1e-6 m elsewhere); asserted at 4 x that, 5.4e-6 m.  The properties of a route hold for the reference alone and with the build's length.
    Both ways the host build decides `clear` give the same bytes."""
    cfg, state, items, aux = shard(kind)
    fspecs = [(fc.spec_of(size, mode, 0.25, F.ROBOT, kind=kind, centre=fc.WORLD_CENTRE), None) for mode in rt.MODES for size in rt.SIZES]
    worst, routes, none = compare_with_the_reference(cfg, state, items, aux, fspecs, kind, kind)
    assert routes > 100 and none > 10, (routes, none)   # both answers occur
    print(f'kind {kind}: worst |length - reference| {worst:.3g} m over {routes} routes ({none} starts without one)')


def compare_with_the_reference(cfg, state, items, aux, fspecs, tag, seed):
    """The comparison of test_host_build_equals_the_reference on the given states, their hand-made poses and with the robots spread about
    the arena.  `fspecs`: pairs (field spec, sources); sources None = the admissible source sets taken in turn.  Returns (the worst
    |length - reference| in metres, the routes found, the starts without one)."""
    worst, turn, routes, none = 0.0, 0, 0, 0
    for base, fixed in fspecs:
        for label, st in states_of(cfg, state):
            sources = fixed if fixed is not None else fc.SOURCE_SETS[turn % len(fc.SOURCE_SETS)]
            frame, p, k = rt.FRAMES[turn % 3], (1, 5, 64)[(turn // 3) % 3], (2, 7, 32)[(turn // 2) % 3]
            robot = turn % 3 == 2
            turn += 1
            fspec = base.copy()
            fspec.sources = sources
            spec = rt.spec_of(fspec, frame, 1 if robot else p, k)
            where = (tag, fspec.mode, (fspec.width, fspec.height), label, sources, frame, p, k, robot)
            field = fc.field_host(cfg, st, items, aux, fspec)
            starts, world = (None, None) if robot else rt.draw_starts(cfg, st, fspec, frame, p, 7 * turn + seed)
            got = rt.route_host(cfg, st, items, aux, spec, starts)
            assert rt.same(got, rt.route_host(cfg, st, items, aux, spec, starts, how=rt.ROWS)), where
            for e in range(N):
                if robot:
                    cells = [rt.robot_cell(st[e], fspec, field.parent[e])]
                else:
                    found = [rt.start_cell(st[e], fspec, pc.world_points(st[e], frame, starts[e])[q]) for q in range(p)]
                    assert not any(near for _, near in found), where   # on the reference alone
                    cells = [c for c, _ in found]
                blocked = field.parent[e] == F.BLOCKED
                for q, c in enumerate(cells):   # the properties, on the reference alone first
                    ref = rt.reference(field.parent[e], c, k, fc.cell_size(fspec))
                    check_properties(ref, blocked, field.parent[e], field.dist[e], fc.cell_size(fspec), ref.length, FIELD_TOL)
                w, refs = rt.check_env(got, e, field.parent[e], st[e], fspec, spec, cells, TOL)
                worst = max(worst, w)
                for q, ref in enumerate(refs):
                    check_properties(ref, blocked, field.parent[e], field.dist[e], fc.cell_size(fspec), float(got.length[e, q]), FIELD_TOL + TOL)
                    routes += ref.count > 0
                    none += ref.count == 0
    return worst, routes, none


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its TOL and no cell exempt, on every entry of sensor_configs.MATRIX: a 24 x 40 grid in the heading mode,
    a 24 x 40 world grid about the entry's own arena, the source sets taken in turn, and the field part of the library's default spec,
    whose extent, blocking and sources are derived from the config (moved to sensor_configs.DEFAULT_CENTRE).  Both answers (a route, none) occur.  On the entry's hostile states
    the routes equal, bit for bit, those of the clean twin, and a robot at a non-finite place has none."""
    cfg, state, items, aux = scfg.shard(name)
    fspecs = [(fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, F.ROBOT, kind=cfg), None), (fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, kind=cfg, centre=fc.WORLD_CENTRE), None)]
    default = R.field_spec(R.default_spec(cfg))
    default.centre[0], default.centre[1] = scfg.DEFAULT_CENTRE
    fspecs.append((default, default.sources))
    worst, routes, none = compare_with_the_reference(cfg, state, items, aux, fspecs, name, scfg.seed_of(name))
    assert routes > 0 and none > 0, (routes, none)
    print(f'{name}: worst |length - reference| {worst:.3g} m over {routes} routes ({none} starts without one)')
    fspec = fspecs[0][0].copy()
    fspec.sources = F.ROBOT | F.FOOD | F.POISON | F.TARGET
    spec = rt.spec_of(fspec, R.HRL_PROBE_HEADING, 8, 7)
    starts, _ = rt.draw_starts(cfg, state, fspec, R.HRL_PROBE_HEADING, 8, 5)
    for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, fc.hostile):
        got = rt.route_host(cfg, s, it, a, spec, starts)
        want = rt.route_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, starts)
        rows = [e for e in range(N) if e not in blind]
        assert rt.same(rt.Route(*(x[rows] for x in got)), rt.Route(*(x[rows] for x in want))), name
        assert all((got.count[e] == 0).all() for e in blind)


def test_known_answers():
    """Cells of 0.25 m, as in test_field_host.test_known_answers.  An empty arena: two waypoints and the Euclidean distance between the two
    cell centres.  The wall of poison with a one-cell gap: from every row but the gap's own the way's interior waypoints lie in or next to the gap (from
    the gap's row it runs straight through).  A source fenced in by
    poison: no route.  A start on a source: one waypoint, length 0."""
    cfg, st, items, aux = gather_env((0.125, -0.375))
    fspec = fc.spec_of((64, 48), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, blocking=F.WALL, half=8.0)
    starts = np.array([[[5.125, 3.375], [-6.875, -4.125], [0.125, 2.125], [0.125, -0.375]]], np.float32)   # cell centres: (10, 52), (40, 4), (15, 32), the robot's (25, 32)
    got = rt.route_host(cfg, st, items, aux, rt.spec_of(fspec, R.HRL_PROBE_WORLD, 4, 16), starts)
    assert got.count[0].tolist() == [2, 2, 2, 1]
    assert got.cells[0, :, 0].tolist() == [10 * 64 + 52, 40 * 64 + 4, 15 * 64 + 32, 25 * 64 + 32] and (got.cells[0, :, 1:] == 25 * 64 + 32).all()
    want = [0.25 * math.hypot(15, 20), 0.25 * math.hypot(15, 28), 2.5, 0.0]
    assert np.abs(got.length[0] - want).max() <= TOL and got.length[0, 3] == 0
    assert np.array_equal(got.waypoints[0, :, 0], starts[0]) and (got.waypoints[0, :, 1:] == np.float32([0.125, -0.375])).all()
    dist = fc.field_host(cfg, st, items, aux, fspec).dist[0]
    assert dist[10, 52] > got.length[0, 0] + 0.25   # the field's chain zig-zags: 15 diagonal and 5 straight steps

    # the wall of poison along the column u = 0.125 of an 8 x 8 grid with the gap in row 5; the robot (the source) to its left
    cell, gap, wall = 0.25, 5, 4
    ys = [0.875 - cell * i for i in range(8)]
    cfg, st, items, aux = gather_env((-0.625, -0.625), poison=[(0.125, y) for i, y in enumerate(ys) if i != gap])
    fspec = fc.spec_of((8, 8), F.HRL_VIEW_WORLD, 0.1, F.ROBOT, blocking=F.POISON, half=1.0)
    starts = np.array([[[0.875, y] for y in ys]], np.float32)   # the last column, every row
    got = rt.route_host(cfg, st, items, aux, rt.spec_of(fspec, R.HRL_PROBE_WORLD, 8, 16), starts)
    parent = fc.field_host(cfg, st, items, aux, fspec).parent[0]
    src = tuple(int(x) for x in np.argwhere(parent == F.SOURCE)[0])
    for i in range(8):
        n = int(got.count[0, i])
        assert 3 <= n <= 16, (i, n)   # no straight line leads through the wall
        way = [(c // 8, c % 8) for c in got.cells[0, i, :n].tolist()]
        assert way[0] == (i, 7) and way[-1] == src
        if i != gap:
            assert all(abs(r - gap) <= 1 and abs(c - wall) <= 1 for r, c in way[1:-1]), (i, way)
        else:   # along the gap's own row the way runs straight through it: it turns only beyond the wall, towards the source's row
            assert way[1][0] == gap and way[1][1] < wall, way
        assert all(rt.clear(parent == F.BLOCKED, a, b) for a, b in zip(way, way[1:]))

    # a food source fenced in by eight poison squares: no route from outside; from the source itself one waypoint
    ring = [(0.125 + cell * dc, 0.125 + cell * dr) for dc in (-1, 0, 1) for dr in (-1, 0, 1) if dc or dr]
    cfg, st, items, aux = gather_env((0.9, 0.9), food=[(0.125, 0.125)], poison=ring)
    fspec = fc.spec_of((8, 8), F.HRL_VIEW_WORLD, 0.1, F.FOOD, blocking=F.POISON, half=1.0)
    starts = np.array([[[0.9, 0.9], [0.125, 0.125], [0.375, 0.125]]], np.float32)   # outside the fence, on the source, on the fence
    got = rt.route_host(cfg, st, items, aux, rt.spec_of(fspec, R.HRL_PROBE_WORLD, 3, 4), starts)
    assert got.count[0].tolist() == [0, 1, 0] and np.isposinf(got.length[0, [0, 2]]).all() and got.length[0, 1] == 0
    assert (got.cells[0, [0, 2]] == -1).all() and np.isnan(got.waypoints[0, [0, 2]]).all() and (got.cells[0, 1] == 3 * 8 + 4).all()
    robot = rt.route_host(cfg, st, items, aux, rt.spec_of(fspec, R.HRL_PROBE_EGO, 1, 4))   # starts = None: the robot, outside the fence
    assert robot.count[0, 0] == 0 and np.isposinf(robot.length[0, 0])


def test_the_maze_route_lies_between_the_exact_path_and_the_field():
    """The maze's start (-2, -5) to the evaluation target (-2, 4) on the 64 x 64 world grid of half extent 9, WALL | BOX in the way.  At
    margin 0.25 the field says 13.28 m and the probe's exact way is 12.45 m; at margin 0.4 they say 13.84 m and 12.84 m (the figure the
    README quotes).  The route's length lies between path - cell and the field's value at either margin -- measured 12.77 m in 4
    waypoints at 0.25 and 13.26 m at 0.4 -- and the route at 0.25 also lies above the quoted 12.84 m - cell."""
    cfg, st, aux = maze_env(((-2.0, -5.0),))
    cfg.targets[0][0], cfg.targets[0][1] = -2.0, 4.0
    aux[0, 3] = 0
    figures = {}
    for margin, want_dist, want_path, want_length in ((0.25, 13.28, 12.45, 12.77), (0.4, 13.84, 12.84, 13.26)):
        fspec = fc.spec_of((64, 64), F.HRL_VIEW_WORLD, margin, F.TARGET, blocking=F.WALL | F.BOX, half=9.0)
        spec = rt.spec_of(fspec, R.HRL_PROBE_EGO, 1, 16)
        got = rt.route_host(cfg, st, None, aux, spec)
        field = fc.field_host(cfg, st, None, aux, fspec)
        cell = rt.robot_cell(st[0], fspec, field.parent[0])
        path = float(pc.probe_host(cfg, st, None, aux, pc.spec_of(1, P.HRL_PROBE_WORLD, margin), np.array([[[-2.0, 4.0]]], np.float32)).path[0, 0])
        length, dist = float(got.length[0, 0]), float(field.dist[0][cell])
        print(f'maze start to the evaluation target at margin {margin}: route {length:.2f} m in {int(got.count[0, 0])} waypoints, field {dist:.2f} m, probe {path:.2f} m')
        assert abs(dist - want_dist) < 0.01 and abs(path - want_path) < 0.01
        assert path - fc.cell_size(fspec) <= length <= dist
        assert abs(length - want_length) < 0.01 and 3 <= got.count[0, 0] <= 16
        rt.check_env(got, 0, field.parent[0], st[0], fspec, spec, [cell], TOL)
        figures[margin] = (length, path)
    assert figures[0.4][1] - fc.cell_size(fspec) <= figures[0.25][0]   # the route at 0.25 against the 12.84 m the README sets next to 13.28 m


def test_truncation_keeps_the_whole_routes_count_and_length():
    cfg, st, aux = maze_env(((-2.0, -5.0), (3.0, 6.0), (4.0, -8.0)))
    fspec = fc.spec_of((64, 64), F.HRL_VIEW_WORLD, 0.25, F.ROBOT, blocking=F.WALL | F.BOX, half=9.0)
    starts = np.tile(np.array([[-2.0, 4.0], [-4.0, 7.0], [0.5, -3.0], [3.0, 0.0]], np.float32), (3, 1, 1))
    full = rt.route_host(cfg, st, None, aux, rt.spec_of(fspec, R.HRL_PROBE_WORLD, 4, 32), starts)
    two = rt.route_host(cfg, st, None, aux, rt.spec_of(fspec, R.HRL_PROBE_WORLD, 4, 2), starts)
    assert (full.count > 2).any() and (full.count <= 32).all()
    assert np.array_equal(two.count, full.count) and np.array_equal(two.length.view(np.uint32), full.length.view(np.uint32))
    assert two.cells.shape == (3, 4, 2) and np.array_equal(two.cells, full.cells[:, :, :2]) and np.array_equal(two.waypoints, full.waypoints[:, :, :2])


@pytest.mark.parametrize('kind', rt.KINDS)
def test_hostile_states_and_starts_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range: the routes equal, bit for bit,
    those of the clean twin (field_cases.hostile); a robot at a non-finite place has no route from anywhere.  Starts with NaN, +-inf or
    3.2e38 in a coordinate have no route, and the other starts of the env keep their bits."""
    cfg, state, items, aux = shard(kind)
    for mode in rt.MODES:
        for size, frame in (((24, 40), R.HRL_PROBE_HEADING), ((64, 64), R.HRL_PROBE_WORLD)):
            fspec = fc.spec_of(size, mode, 0.25, F.ROBOT | F.FOOD | F.POISON | F.TARGET, kind=kind)
            spec = rt.spec_of(fspec, frame, 8, 7)
            starts, _ = rt.draw_starts(cfg, state, fspec, frame, 8, 5)
            for s, it, a, cs, cit, ca, far, blind in fc.hostile(cfg, state, items, aux):
                got = rt.route_host(cfg, s, it, a, spec, starts)
                want = rt.route_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, starts)
                rows = [e for e in range(N) if e not in blind]
                assert rt.same(rt.Route(*(x[rows] for x in got)), rt.Route(*(x[rows] for x in want))), (kind, mode, size)
                for e in blind:
                    assert (got.count[e] == 0).all() and np.isposinf(got.length[e]).all() and (got.cells[e] == -1).all() and np.isnan(got.waypoints[e]).all()
                robot = rt.route_host(cfg, s, it, a, rt.spec_of(fspec, frame, 1, 7))
                assert all(robot.count[e, 0] == 0 for e in blind)
            clean = rt.route_host(cfg, state, items, aux, spec, starts)
            bad, blank, huge = pc.hostile_points(starts)
            got = rt.route_host(cfg, state, items, aux, spec, bad)
            gone = list(blank) + list(huge)
            assert (got.count[:, gone] == 0).all() and np.isposinf(got.length[:, gone]).all() and (got.cells[:, gone] == -1).all() and np.isnan(got.waypoints[:, gone]).all()
            keep = [q for q in range(8) if q not in gone]
            assert rt.same(rt.Route(*(x[:, keep] for x in got)), rt.Route(*(x[:, keep] for x in clean)))


def test_none_members_and_a_mask_leave_the_other_bytes_alone():
    cfg, state, items, aux = shard(K.HRL_ANT_MAZE)
    fspec = fc.spec_of((24, 40), F.HRL_VIEW_EGO_HEADING, 0.25, F.TARGET | F.ROBOT, kind=K.HRL_ANT_MAZE)
    spec = rt.spec_of(fspec, R.HRL_PROBE_EGO, 5, 7)
    starts, _ = rt.draw_starts(cfg, state, fspec, R.HRL_PROBE_EGO, 5, 1)
    full = rt.route_host(cfg, state, items, aux, spec, starts)
    for want in (('waypoints',), ('count',), ('length',), ('cells',), ('count', 'length')):
        part = rt.route_host(cfg, state, items, aux, spec, starts, want=want)
        for name, x, y in zip(rt.NAMES, rt.bits(part), rt.bits(full)):
            assert (x is None) if name not in want else np.array_equal(x, y), (want, name)
    out = rt.Route(*(np.full(shape, -7, dt) for dt, shape in zip(rt.DTYPES, rt.shapes(N, spec))))
    mask = np.array([1, 0, 1, 0, 0], np.uint8)
    rt.route_host(cfg, state, items, aux, spec, starts, mask=mask, out=out)
    for e in range(N):
        for x, y in zip(rt.bits(out), rt.bits(full)):
            assert np.array_equal(x[e], y[e]) if mask[e] else (out[0][e] == -7).all() and (out[1][e] == -7).all() and (out[2][e] == -7).all() and (out[3][e] == -7).all()


BAD_SPECS = [('width', 0), ('width', 12), ('width', 72), ('height', 4), ('height', 72), ('mode', 3), ('blocking', 0), ('blocking', 32), ('sources', 0), ('sources', F.BOX),
             ('margin', float('nan')), ('margin', 3.0), ('half_extent', 0.0), ('half_extent', float('inf')), ('n_starts', 0), ('n_starts', 65), ('n_starts', -1),
             ('frame', 3), ('frame', -1), ('max_waypoints', 1), ('max_waypoints', 33), ('max_waypoints', 0), ('struct_size', 16), ('struct_size', 0), ('out', None)]
REASONS = {'width': 'width must be a multiple of 8', 'height': 'height must be a multiple of 8', 'mode': 'unknown field mode', 'blocking': 'blocking must be a non-empty mask',
           'sources': 'sources must be a non-empty mask', 'margin': 'margin must be finite', 'half_extent': 'half_extent must be finite', 'n_starts': 'n_starts must be within 1..64',
           'frame': 'unknown route frame', 'max_waypoints': 'max_waypoints must be within 2..32', 'struct_size': 'struct_size is not sizeof', 'out': 'holds no pointer'}


@pytest.mark.parametrize('field,value', BAD_SPECS)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = rt.spec_of(fc.spec_of((24, 40), F.HRL_VIEW_WORLD, 0.4, F.ROBOT, kind=K.HRL_ANT_FLAT), R.HRL_PROBE_WORLD, 5, 7)
    out = rt.Route(*(np.full((N, 64, 32, 2)[:len(shape)], -7, dt) for dt, shape in zip(rt.DTYPES, rt.shapes(N, spec))))
    starts = np.zeros((N, 64, 2), np.float32)
    handed = out
    if field == 'out':
        handed = rt.Route(None, None, None, None)
    else:
        setattr(spec, field, value)
    m = None
    b = K.make_buffers(rt.ptr(state), rt.ptr(items), rt.ptr(aux), None, None, None, None, None)
    o = R.hrl_route_out(**{name: rt.ptr(a) for name, a in zip(rt.NAMES, handed)})
    code = rt.lib().route_host(C.byref(cfg), C.byref(b), C.byref(spec), rt.ptr(starts), m, C.byref(o), rt.WALK)
    why = rt.lib().route_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and REASONS[field] in why
    assert all((x == -7).all() for x in out)
    # the device library runs the same checks before it looks for a device
    L = R.lib()
    assert L.hrl_route(C.byref(cfg), C.byref(b), C.byref(spec), rt.ptr(starts), None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
    assert why.encode() in L.hrl_route_last_error()
    assert all((x == -7).all() for x in out)


def test_two_misaligned_pointers_name_the_first():
    """The outputs are looked at in the record's order and `starts` after them: of two misaligned pointers the first is named."""
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = R.default_spec(cfg, n_starts=2)
    b = K.make_buffers(rt.ptr(state), rt.ptr(items), rt.ptr(aux), None, None, None, None, None)
    room = {name: np.zeros(N * 2 * 16 * 2 * 4 + 64, np.uint8) for name in rt.NAMES + ('starts',)}
    at = {name: (a.ctypes.data + 63) // 64 * 64 for name, a in room.items()}
    L = R.lib()
    for first, second in (('waypoints', 'starts'), ('count', 'cells'), ('cells', 'starts')):
        addr = dict(at)
        addr[first] += 2
        addr[second] += 1
        o = R.hrl_route_out(**{name: addr[name] for name in rt.NAMES})
        assert L.hrl_route(C.byref(cfg), C.byref(b), C.byref(spec), addr['starts'], None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
        assert L.hrl_route_last_error().decode() == f'hrl_route: {first} must be 4-byte aligned'
    assert all((a == 0).all() for a in room.values())


def test_default_spec_and_the_mirrors():
    for kind in rt.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, mode in R.MODES.items():
            s, h, f = R.default_spec(cfg, name), R.hrl_route_spec(), F.default_spec(cfg, name)
            assert rt.lib().route_host_default_spec(C.byref(cfg), mode, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert bytes(R.field_spec(s)) == bytes(f) and bytes(R.from_field_spec(f)) == bytes(s)
            assert (s.struct_size, s.n_starts, s.frame, s.max_waypoints) == (C.sizeof(R.hrl_route_spec), 1, R.HRL_PROBE_EGO, 16)
            assert rt.lib().route_validate_spec(C.byref(s)) == b''
    s = R.default_spec(cfg, 'ego', 24, 40, 'heading', 5, 7)
    assert (s.width, s.height, s.mode, s.frame, s.n_starts, s.max_waypoints) == (24, 40, 1, 2, 5, 7)
    assert R.default_spec(cfg, 'world', 64, 32).half_extent == 2 * R.default_spec(cfg).half_extent
    with pytest.raises(ValueError):
        R.default_spec(cfg, 'sideways')
    with pytest.raises(ValueError):
        R.default_spec(cfg, frame='sideways')
    assert rt.lib().route_sizeof_spec() == C.sizeof(R.hrl_route_spec) == 56 and rt.lib().route_sizeof_out() == C.sizeof(R.hrl_route_out)
    assert R.Route() == (None,) * 4 and R.Route._fields == rt.NAMES
    assert (R.MAX_STARTS, R.MIN_WAYPOINTS, R.MAX_WAYPOINTS) == (64, 2, 32)


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """route_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the routes of every kind in the three
    modes from reset-like and hostile states and starts, both ways to decide clear: exit status 0, sizeof(hrl_route_spec) == the ctypes
    mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([rt.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_route_spec {C.sizeof(R.hrl_route_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = rt.lib().route_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert rt.lib().route_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different routes


def test_route_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_route_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the route kernel and an LDS footprint of at most 40 KB (four workgroups per CU); the header's symbols are SYMBOLS; the
    route is an entry of build.py of its own, built by build() after the four sensors."""
    code = 'from hrl_pybullet_envs_amd.build import build_route, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_route(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=rt.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(rt.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_route_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*route_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 40960
    hdr = open(os.path.join(rt.ROOT, 'include', 'hrl_route.h')).read()
    assert set(re.findall(r'\b(hrl_route(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_route_out', 'hrl_route_spec'} == set(R.SYMBOLS)
    for s in R.SYMBOLS:
        assert hasattr(R.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.ROUTE[0] == 'route' and 'route' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_sensor(name, force, verbose)\n    build_route(force, verbose)') > 0
