"""The batched frontier map's specification (csrc/frontier_core.h) on the CPU: its host build (tests/frontier_host) against the integer
logic of include/hrl_frontier.h applied to the host field's own verdicts and to the memory (tests/frontier_cases.py), fp64 Dijkstra on the
build's own mask, the tie to the field, schedule independence, the summary, a scripted explorer that explores the whole reachable arena,
totality on hostile states, spec validation, the sanitised stand-alone program and the gfx950 cross-compile.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_cases as fc
import frontier_cases as xc
import orc
import see_cases as vc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import frontier_device as X
from hrl_pybullet_envs_amd import see_device as V
from test_field_host import maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
# metres: the worst |host build - fp64 Dijkstra on the same mask| measured over the sweep of test_classification_exactly_and_propagation
WORST = 1.84e-5
TOL = 4 * WORST   # asserted at four times that, the siblings' convention
assert TOL <= 2e-4


def states_of(cfg, state):
    return (('shard', state), ('hand-made', xc.hand_made(cfg, state)), ('spread', xc.spread(cfg, state)))


def cells_of(cfg, st, spec):
    """The robots' cells in fp64, after asserting on the reference alone that no robot stands within BAND of a cell edge."""
    out = []
    for e in range(cfg.num_envs):
        cell, gap = xc.robot_cell(st[e], spec)
        assert gap > fc.BAND, (e, gap)
        out.append(cell)
    return out


@pytest.mark.parametrize('kind', xc.KINDS)
def test_classification_exactly_and_propagation(kind):
    """Six kinds x 8 x 8, 24 x 40, 64 x 8 and 64 x 64 cells x margin 0, 0.25 and 0.4 x the shard's states, the hand-made poses and the
    robots spread about the arena x both meanings of `unknown` x five memories (real ones from the host visibility map over one to three
    places of the robot, all ones, all zeros, arbitrary bytes in a third of the cells, a checkerboard), the 31 admissible source sets
    taken in turn, on the world grids about field_cases.WORLD_CENTRE.

    Classification: `edge` and the BLOCKED and SOURCE cells of `parent` equal frontier_cases.classify -- integer numpy logic on the host
    field's own verdicts on the same grid, the memory and the robot's cell found in fp64 -- on every cell, none exempt.  No robot stands
    within 1e-4 m of a cell edge: asserted on the reference alone first.

    Propagation: fp64 Dijkstra on the host build's OWN mask and source set (field_cases.check_propagation) gives the same +inf and
    UNREACHED cells exactly, dist within TOL, and a parent whose step is within TOL of the reference's best.  Measured worst
    |dist - reference| over this sweep: 1.84e-5 m (the maze kinds; 7.9e-6 .. 9.3e-6 m elsewhere; the field's own sweep gives
    1.53e-5 m -- ways through known space wind more); asserted at 4 x that, 7.4e-5 m."""
    cfg, state, items, aux = shard(kind)
    bases = [xc.spec_of(size, margin, kind=kind) for size in xc.SIZES for margin in xc.MARGINS]
    worst, turn, edges, unknown_cells = compare_with_the_reference(cfg, state, items, aux, bases, xc.MEMORIES, kind)
    assert edges > 1000 and unknown_cells > 1000
    print(f'kind {kind}: worst |dist - reference| {worst:.3g} m over {turn} cases')


def compare_with_the_reference(cfg, state, items, aux, bases, memories, tag):
    """The comparison of test_classification_exactly_and_propagation on the grids of `bases` (their sources and `unknown` are replaced:
    both meanings of `unknown`, the source sets taken in turn) with the memories `memories`, on the given states, their hand-made poses
    and with the robots spread about the arena.  Returns (the worst |dist - reference| in metres, the cases, the edge cells, the
    unknown cells)."""
    worst, turn, edges, unknown_cells = 0.0, 0, 0, 0
    for base in bases:
        for label, st in states_of(cfg, state):
            robots = cells_of(cfg, st, base)
            for which in memories:
                seen = xc.memory(which, cfg, st, items, aux, base, turn)
                for unknown in xc.UNKNOWNS:
                    sources = xc.SOURCE_SETS[turn % len(xc.SOURCE_SETS)]
                    turn += 1
                    spec = base.copy()
                    spec.sources, spec.unknown = sources, unknown
                    where = (tag, (spec.width, spec.height), spec.margin, label, which, unknown, sources)
                    blocked, source = xc.geometry(cfg, st, items, aux, spec)
                    before = seen.copy()
                    got = xc.frontier_host(cfg, st, items, aux, spec, seen)
                    assert np.array_equal(seen, before)   # only read
                    for e in range(N):
                        edge, v_blocked, v_source = xc.classify(blocked[e], source[e], seen[e], robots[e], sources, unknown)
                        assert np.array_equal(got.edge[e].astype(bool), edge) and got.edge[e].max() <= 1, (where, e, 'edge')
                        assert np.array_equal(got.parent[e] == F.BLOCKED, v_blocked), (where, e, 'blocked', np.argwhere((got.parent[e] == F.BLOCKED) != v_blocked)[:4])
                        assert np.array_equal(got.parent[e] == F.SOURCE, v_source), (where, e, 'source', np.argwhere((got.parent[e] == F.SOURCE) != v_source)[:4])
                        worst = max(worst, fc.check_propagation(fc.Field(got.dist[e], got.parent[e]), spec, TOL))
                        edges += int(edge.sum())
                        unknown_cells += int((seen[e] == 0).sum())
    return worst, turn, edges, unknown_cells


@pytest.mark.parametrize('name', scfg.NAMES)
def test_classification_exactly_and_propagation_on_the_sensor_config_matrix(name):
    """The comparison above, no cell exempt and with its TOL, on every entry of sensor_configs.MATRIX: a 24 x 40 grid at margin 0.25 about
    the entry's own arena and the grid of the library's default spec, whose extent, blocking and margin are derived from the config
    (moved to sensor_configs.DEFAULT_CENTRE: no robot within 1e-4 m of a cell edge, asserted on the reference alone), with a real and a
    dirty memory.  On the entry's hostile states the map equals, bit for bit, that of the clean twin, and a robot without a finite
    place has no cell."""
    cfg, state, items, aux = scfg.shard(name)
    default = X.default_spec(cfg)
    default.centre[0], default.centre[1] = scfg.DEFAULT_CENTRE
    bases = [xc.spec_of((24, 40), 0.25, kind=cfg), default]
    worst, turn, edges, unknown_cells = compare_with_the_reference(cfg, state, items, aux, bases, ('real', 'dirty'), name)
    assert edges > 100 and unknown_cells > 1000   # (the smallest arena's 24 x 40 grid holds some 300 free cells)
    print(f'{name}: worst |dist - reference| {worst:.3g} m over {turn} cases')
    spec = xc.spec_of((24, 40), 0.25, X.EDGE | xc.CLASS_SOURCES, X.OPTIMISTIC, kind=cfg)
    seen = xc.memory('dirty', cfg, state, items, aux, spec, 1)
    for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, xc.hostile):
        got = xc.frontier_host(cfg, s, it, a, spec, seen)
        want = xc.frontier_host(xc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, seen)
        rows = [e for e in range(N) if e not in blind]
        assert xc.same(xc.Frontier(*(x[rows] for x in got)), xc.Frontier(*(x[rows] for x in want))), name
        b = list(blind)
        assert np.isinf(got.length[b]).all() and (got.cell[b] == -1).all() and np.isnan(got.goal[b]).all()


@pytest.mark.parametrize('kind', (K.HRL_ANT_MAZE, K.HRL_ANT_GATHER, K.HRL_ANT_FLAGRUN))
def test_tie_to_the_field(kind):
    """Fully seen and without EDGE, dist and parent are the host field's bit for bit, in both modes.  Fully seen and towards EDGE alone
    nothing is an edge: count 0, every free cell +inf, length +inf, goal NaN.  Nothing seen and KNOWN_ONLY: the one edge cell is the
    robot's own, exactly where it stands on a free cell inside the grid: length 0 and cell = r."""
    cfg, state, items, aux = shard(kind)
    for label, st in states_of(cfg, state):
        for size, margin in (((24, 40), 0.25), ((64, 64), 0.4), ((8, 8), 0.0)):
            ones, zeros = np.ones((N, size[1], size[0]), np.uint8), np.zeros((N, size[1], size[0]), np.uint8)
            for unknown in xc.UNKNOWNS:
                for sources in (F.ROBOT, F.TARGET | F.FOOD, F.ROBOT | F.POISON | F.TARGET):
                    spec = xc.spec_of(size, margin, sources, unknown, kind=kind)
                    got = xc.frontier_host(cfg, st, items, aux, spec, ones)
                    want = fc.field_host(cfg, st, items, aux, xc.field_spec(spec, sources))
                    assert fc.same(fc.Field(got.dist, got.parent), want), (kind, label, size, unknown, sources)
                    assert (got.count == 0).all() and not got.edge.any()
                spec = xc.spec_of(size, margin, X.EDGE, unknown, kind=kind)
                got = xc.frontier_host(cfg, st, items, aux, spec, ones)
                assert (got.count == 0).all() and np.isinf(got.dist).all() and np.isin(got.parent, (F.UNREACHED, F.BLOCKED)).all()
                assert np.isinf(got.length).all() and np.isnan(got.goal).all() and (got.cell == -1).all()
            spec = xc.spec_of(size, margin, X.EDGE, X.KNOWN_ONLY, kind=kind)
            got = xc.frontier_host(cfg, st, items, aux, spec, zeros)
            robots = cells_of(cfg, st, spec)
            blocked, _ = xc.geometry(cfg, st, items, aux, spec)
            for e in range(N):
                alone = robots[e] is not None and not blocked[e][robots[e]]
                assert got.count[e] == int(alone) and got.edge[e].sum() == int(alone), (kind, label, size, e)
                if alone:
                    assert got.edge[e][robots[e]] == 1 and got.length[e] == 0 and got.cell[e] == robots[e][0] * size[0] + robots[e][1]
                else:
                    assert np.isinf(got.length[e]) and got.cell[e] == -1 and np.isnan(got.goal[e]).all()


@pytest.mark.parametrize('kind', (K.HRL_ANT_MAZE, K.HRL_ANT_GATHER))
def test_the_schedule_does_not_matter(kind):
    """Jacobi rounds, in-place sweeps in raster order and in reverse raster order give the same bits of all seven outputs."""
    cfg, state, items, aux = shard(kind)
    st = xc.spread(cfg, state)
    for t, size in enumerate(((24, 40), (64, 64))):
        for unknown in xc.UNKNOWNS:
            for which in ('real', 'dirty'):
                spec = xc.spec_of(size, 0.25, X.EDGE | X.TARGET | X.FOOD, unknown, kind=kind)
                seen = xc.memory(which, cfg, st, items, aux, spec, t)
                r = [np.zeros(N, np.int32) for _ in range(3)]
                a, b, c = (xc.frontier_host(cfg, st, items, aux, spec, seen, schedule=s, rounds=r[s]) for s in (fc.JACOBI, fc.FORWARD, fc.REVERSE))
                assert xc.same(a, b) and xc.same(a, c), (kind, size, unknown, which)
                assert (r[0] <= size[0] * size[1]).all() and (r[1] <= r[0]).all() and (r[2] <= r[0]).all()
                assert np.isfinite(a.dist).any()


def end_of(parent, row, col):
    """The cell the walk along `parent` from (row, col) ends on (field_cases.follow counts its steps), or None."""
    n = fc.follow(parent, row, col, parent.size)
    if n < 0:
        return None
    for _ in range(n):
        k = int(parent[row, col])
        row, col = row + fc.STEPS[k][1], col + fc.STEPS[k][0]
    return row, col


@pytest.mark.parametrize('kind', xc.KINDS)
def test_summary(kind):
    """count == edge.sum(); the bits of length are those of dist at the robot's cell (+inf without one, or on a blocked or unreached one);
    field_cases.follow from the robot's cell ends on `cell`; goal is that cell's centre."""
    cfg, state, items, aux = shard(kind)
    reached = lost = 0
    for t, (label, st) in enumerate(states_of(cfg, state)):
        for size in xc.SIZES:
            for unknown in xc.UNKNOWNS:
                for which in ('real', 'dirty', 'checkerboard'):
                    t += 1
                    spec = xc.spec_of(size, 0.25, xc.SOURCE_SETS[(5 * t) % 31], unknown, kind=kind)
                    seen = xc.memory(which, cfg, st, items, aux, spec, t)
                    got = xc.frontier_host(cfg, st, items, aux, spec, seen)
                    robots = cells_of(cfg, st, spec)
                    assert np.array_equal(got.count, got.edge.reshape(N, -1).sum(1))
                    for e in range(N):
                        r = robots[e]
                        if r is None or got.parent[e][r] > F.SOURCE:
                            assert np.isinf(got.length[e]) and got.length[e] > 0 and got.cell[e] == -1 and np.isnan(got.goal[e]).all()
                            lost += 1
                            continue
                        assert got.length[e].view(np.uint32) == got.dist[e][r].view(np.uint32)
                        end = end_of(got.parent[e], *r)
                        assert end is not None and got.cell[e] == end[0] * size[0] + end[1] and got.parent[e][end] == F.SOURCE
                        centre = fc.centres(st[e], xc.field_spec(spec, F.ROBOT))[0][end]
                        assert np.abs(got.goal[e] - centre).max() <= 1e-5
                        reached += 1
    assert reached > 50 and (lost > 0 or kind == K.HRL_ANT_FLAT)


def test_two_documented_answers():
    """A robot at the maze's start looking along +x through a field of view of 50 degrees has not seen the cell behind it: its own cell,
    known because it stands there, is an edge cell, so length is 0 and cell is its own.  A robot outside the grid has no cell: length
    +inf, cell -1, goal NaN, while count still counts the memory's edges."""
    cfg, st, aux = maze_env(((-2.0, -5.0),))
    spec = xc.spec_of((32, 32), 0.25, X.EDGE, blocking=F.WALL | F.BOX, half=9.3)
    mem = vc.See(None, np.zeros((1, 32, 32), np.uint8), None)
    vc.see_host(cfg, st, None, aux, xc.see_spec(spec, fov_cos=float(np.cos(np.radians(25)))), out=mem)
    (r, gap) = xc.robot_cell(st[0], spec)
    assert gap > fc.BAND and mem.seen[0][r[0], r[1] - 1] == 0 and mem.seen[0][r[0], r[1] + 1] == 1   # on the memory alone: behind unseen, ahead seen
    got = xc.frontier_host(cfg, st, None, aux, spec, mem.seen)
    assert got.edge[0][r] == 1 and got.length[0] == 0 and got.cell[0] == r[0] * 32 + r[1] and got.count[0] == got.edge[0].sum() > 1
    assert np.abs(got.goal[0] - fc.centres(st[0], xc.field_spec(spec, F.ROBOT))[0][r]).max() <= 1e-5
    small = xc.spec_of((32, 32), 0.25, X.EDGE, blocking=F.WALL | F.BOX, half=3.0, centre=(0.0, 0.0))
    assert xc.robot_cell(st[0], small)[0] is None
    seen = xc.memory('checkerboard', cfg, st, None, aux, small, 0)
    got = xc.frontier_host(cfg, st, None, aux, small, seen)
    assert np.isinf(got.length[0]) and got.cell[0] == -1 and np.isnan(got.goal[0]).all() and got.count[0] == got.edge[0].sum() > 100


def explore(cfg, st, items, aux, spec, max_range):
    """see, frontier, move to the goal, until length is +inf: (iterations, the last map, the memory)."""
    st = st.copy()
    ss = xc.see_spec(spec, occluders=spec.blocking, max_range=max_range)
    mem = vc.See(None, np.zeros((1, spec.height, spec.width), np.uint8), None)
    for it in range(1, spec.width * spec.height + 1):
        vc.see_host(cfg, st, items, aux, ss, out=mem)
        got = xc.frontier_host(cfg, st, items, aux, spec, mem.seen)
        if np.isinf(got.length[0]):
            return it, got, mem.seen[0]
        st[0, 0:2] = got.goal[0]
    raise AssertionError('the explorer did not finish within W * H iterations')


EXPLORERS = [(K.HRL_ANT_MAZE, cells, margin, rng) for cells in (16, 24, 32) for margin in (0.25, 0.4) for rng in (vc.HUGE, 4.0, 2.5)] + [(K.HRL_ANT_GATHER, 24, 0.25, 3.0)]


@pytest.mark.parametrize('kind,cells,margin,max_range', EXPLORERS)
def test_the_explorer_explores_everything_it_can_reach(kind, cells, margin, max_range):
    """From the start (-2, -5), blocking = occluders = WALL | BOX, all round, a slack of one cell: look (the host visibility map), ask the
    host frontier map, go to `goal`, until length is +inf -- within W * H iterations (a condition; the numpy model of the definition
    needed 3 to 42).  Then no edge cell is left, and every cell the host field reaches from the start (sources = ROBOT, the same
    blocking and margin) has been seen."""
    cfg = orc.default_config(kind, num_envs=1)
    st = np.zeros((1, K.HRL_STATE_STRIDE), np.float32)
    st[0, 0:2], st[0, 2], st[0, 6] = (-2.0, -5.0), 0.55, 1.0
    aux = np.zeros((1, K.HRL_AUX_STRIDE), np.int32)
    spec = xc.spec_of((cells, cells), margin, X.EDGE, blocking=F.WALL | F.BOX, kind=kind)
    its, got, seen = explore(cfg, st, None, aux, spec, max_range)
    print(f'kind {kind} {cells} x {cells} margin {margin} range {max_range:g}: {its} iterations')
    assert got.count[0] == 0 and not got.edge.any()
    reach = fc.field_host(cfg, st, None, aux, xc.field_spec(spec, F.ROBOT)).dist[0]
    assert np.isfinite(reach).sum() > cells * cells // 4 and (seen[np.isfinite(reach)] != 0).all()


@pytest.mark.parametrize('kind', xc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range (field_cases.hostile): the map
    equals, bit for bit, that of the clean twin without the shape.  A robot without a finite place has no cell -- length +inf, cell -1,
    goal NaN -- and its grids are those of a robot at the world's origin that is no source, on a fully seen memory."""
    cfg, state, items, aux = shard(kind)
    for t, (size, margin) in enumerate((((24, 40), 0.4), ((64, 64), 0.0))):
        for unknown in xc.UNKNOWNS:
            spec = xc.spec_of(size, margin, X.EDGE | xc.CLASS_SOURCES, unknown, kind=kind)
            seen = xc.memory('dirty', cfg, state, items, aux, spec, t)
            ones = np.ones_like(seen)
            for s, it, a, cs, cit, ca, far, blind in xc.hostile(cfg, state, items, aux):
                got = xc.frontier_host(cfg, s, it, a, spec, seen)
                want = xc.frontier_host(xc.far_targets(cfg) if far else cfg, cs, cit, ca, spec, seen)
                rows = [e for e in range(N) if e not in blind]
                assert xc.same(xc.Frontier(*(x[rows] for x in got)), xc.Frontier(*(x[rows] for x in want))), (kind, size, unknown)
                if blind:
                    b = list(blind)
                    assert np.isinf(got.length[b]).all() and (got.cell[b] == -1).all() and np.isnan(got.goal[b]).all()
                    assert np.array_equal(got.count[b], got.edge[b].reshape(len(b), -1).sum(1))
                    nosrc = spec.copy()
                    nosrc.sources = X.EDGE | (xc.CLASS_SOURCES & ~X.ROBOT)
                    z = cs.copy()
                    z[b, 0:2] = 0.0
                    g1, g0 = xc.frontier_host(cfg, s, it, a, spec, ones), xc.frontier_host(cfg, z, cit, ca, nosrc, ones)
                    assert all(np.array_equal(xc.bits(x[b]), xc.bits(y[b])) for x, y in zip(g1[:4], g0[:4])), (kind, size, unknown)


BAD = [('width', 0), ('width', 12), ('width', 72), ('height', 4), ('height', 72), ('half_extent', 0.0), ('half_extent', float('inf')), ('half_extent', float('nan')),
       ('blocking', 0), ('blocking', 32), ('sources', 0), ('sources', 128), ('sources', X.EDGE | F.WALL), ('sources', F.BOX), ('margin', float('nan')), ('margin', -1.0), ('margin', 3.0),
       ('unknown', 2), ('unknown', -1), ('struct_size', 16), ('struct_size', 0), ('out', 'empty'), ('out', 'no seen'), ('out', 'seen is edge'), ('out', 'seen is parent')]
REASONS = {'width': 'width must be a multiple of 8', 'height': 'height must be a multiple of 8', 'half_extent': 'half_extent must be finite', 'blocking': 'blocking must be a non-empty mask',
           'sources': 'frontier sources must be a non-empty mask of HRL_FRONTIER_EDGE', 'margin': 'margin must be finite', 'unknown': 'unknown must be HRL_FRONTIER_KNOWN_ONLY or',
           'struct_size': 'struct_size is not sizeof', 'empty': 'holds no pointer', 'no seen': 'seen is null', 'seen is edge': 'seen must not be the memory of edge or parent',
           'seen is parent': 'seen must not be the memory of edge or parent'}


def guarded(n, side=64):
    return xc.Frontier(np.full((n, side, side), 0x7B, np.uint8), np.full((n, side, side), -7, np.float32), np.full((n, side, side), 0x7B, np.uint8), np.full(n, -7, np.int32),
                       np.full(n, -7, np.float32), np.full((n, 2), -7, np.float32), np.full(n, -7, np.int32))


def untouched(out):
    return all((x == (0x7B if x.dtype == np.uint8 else -7)).all() for x in out)


@pytest.mark.parametrize('field,value', BAD)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = xc.spec_of((24, 40), 0.25, kind=K.HRL_ANT_FLAT)
    out = guarded(N)
    seen = np.full((N, 64, 64), 0x7B, np.uint8)
    handed, mem = out, seen
    if field == 'out':
        handed = xc.Frontier(*(None,) * 7) if value == 'empty' else out
        mem = {'empty': seen, 'no seen': None, 'seen is edge': out.edge, 'seen is parent': out.parent}[value]
    else:
        setattr(spec, field, value)
    code, why = xc.frontier_host(cfg, state, items, aux, spec, mem, out=handed, expect_ok=False)
    assert code == K.HRL_ERR_BAD_ARG and REASONS[value if field == 'out' else field] in why, why
    assert untouched(out) and (seen == 0x7B).all()
    # the device library runs the same checks before it looks for a device
    L = X.lib()
    b = K.make_buffers(xc.ptr(state), xc.ptr(items), xc.ptr(aux), None, None, None, None, None)
    o = X.hrl_frontier_out(**{name: xc.ptr(a) for name, a in zip(xc.NAMES, handed)})
    assert L.hrl_frontier(C.byref(cfg), C.byref(b), C.byref(spec), xc.ptr(mem), None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_frontier_last_error() == b'hrl_frontier: ' + why.encode()
    assert untouched(out) and (seen == 0x7B).all()


def test_default_spec_and_the_mirrors():
    for kind in xc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        s, h, f, v = X.default_spec(cfg), X.hrl_frontier_spec(), F.default_spec(cfg, 'world'), V.default_spec(cfg, 'world')
        assert xc.lib().frontier_host_default_spec(C.byref(cfg), C.byref(h)) == 0 and bytes(s) == bytes(h)
        assert (s.width, s.height, s.centre[0], s.centre[1], s.half_extent) == (v.width, v.height, v.centre[0], v.centre[1], v.half_extent)   # the grid of hrl_see_default_spec
        assert (s.struct_size, s.blocking, s.margin, s.sources, s.unknown) == (C.sizeof(X.hrl_frontier_spec), f.blocking, f.margin, X.EDGE, X.KNOWN_ONLY)
        assert xc.lib().frontier_validate_spec(C.byref(s)) == b''
        like = X.spec_like(cfg, V.default_spec(cfg, 'world', 24, 40), sources=X.EDGE | X.TARGET, unknown='optimistic', margin=0.4)
        w = V.default_spec(cfg, 'world', 24, 40)
        assert (like.width, like.height, like.half_extent, tuple(like.centre)) == (24, 40, w.half_extent, tuple(w.centre))
        assert (like.sources, like.unknown, like.blocking) == (X.EDGE | X.TARGET, X.OPTIMISTIC, f.blocking) and like.margin == np.float32(0.4)
        assert xc.lib().frontier_validate_spec(C.byref(like)) == b''
    s = X.default_spec(cfg, 24, 40, sources=X.ROBOT, unknown=X.OPTIMISTIC, margin=0.1)
    assert (s.width, s.height, s.sources, s.unknown) == (24, 40, X.ROBOT, 1) and s.margin == np.float32(0.1)
    assert X.default_spec(cfg, 64, 32).half_extent == 2 * X.default_spec(cfg).half_extent == V.default_spec(cfg, 'world', 64, 32).half_extent
    with pytest.raises(ValueError):
        X.default_spec(cfg, unknown='maybe')
    with pytest.raises(ValueError):
        X.spec_like(cfg, V.default_spec(cfg, 'ego'))
    assert xc.lib().frontier_sizeof_spec() == C.sizeof(X.hrl_frontier_spec) == 48 and xc.lib().frontier_sizeof_out() == C.sizeof(X.hrl_frontier_out) == 56
    assert X.Frontier() == (None,) * 7 and X.Frontier._fields == xc.NAMES
    assert (X.EDGE, X.KNOWN_ONLY, X.OPTIMISTIC) == (64, 0, 1) and X.EDGE & (X.ALL | X.ROBOT) == 0


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """frontier_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the maps of every kind from
    reset-like and hostile states, on three kinds of memory, under the three schedules: exit status 0, sizeof(hrl_frontier_spec) == the
    ctypes mirror's, checksums == the unsanitised host build's."""
    p = subprocess.run([xc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_frontier_spec {C.sizeof(X.hrl_frontier_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = xc.lib().frontier_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert xc.lib().frontier_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different maps


def test_frontier_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_frontier_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no
    spills for the kernel and an LDS footprint of at most 32 KB (five workgroups per CU); the header's symbols are SYMBOLS; the map is
    an entry of build.py of its own, built by build() after the visibility map."""
    code = 'from hrl_pybullet_envs_amd.build import build_frontier, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_frontier(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=xc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(xc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_frontier_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*frontier_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 32768
    hdr = open(os.path.join(xc.ROOT, 'include', 'hrl_frontier.h')).read()
    assert set(re.findall(r'\b(hrl_frontier(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_frontier_out', 'hrl_frontier_spec'} == set(X.SYMBOLS)
    for s in X.SYMBOLS:
        assert hasattr(X.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.FRONTIER == ('frontier', 'libhrl_frontier_hip.so', 'frontier_hip.hip', 'frontier_core.h', 'hrl_frontier.h')
    assert 'frontier' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_see(force, verbose)\n    build_frontier(force, verbose)') > 0
