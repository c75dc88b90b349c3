"""Shared by tests/test_route_host.py and tests/test_gpu_route.py: the ctypes binding of tests/route_host/libroute_host.so (the host build
of csrc/route_core.h), an independent reference written from include/hrl_route.h alone (`clear` by exact rational segment-square
intersection with fractions.Fraction, chain and pull in plain Python on a given `parent`, lengths in fp64), and the starts and specs the
tests compute routes of.  Test infrastructure only."""
import collections
import ctypes as C
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

import field_cases as fc
import probe_cases as pc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import route_device as R

ROOT = fc.ROOT
DIR = os.path.join(ROOT, 'tests', 'route_host')
KINDS = fc.KINDS
MODES = fc.MODES
FRAMES = pc.FRAMES
SIZES = ((8, 8), (24, 40), (64, 64))                 # width, height of the host sweep
GPU_SIZES = ((8, 8), (24, 40), (64, 8), (64, 64))    # 8 x 8: three waves idle in the field phases
WALK, ROWS = 0, 1                                    # how the host build decides clear: by its definition | a row at a time, as the device does
NAMES = tuple(n for n, _ in R.FIELDS)
DTYPES = (np.float32, np.int32, np.float32, np.int32)
Route = collections.namedtuple('Route', NAMES)       # of numpy arrays
HALF = Fraction(1, 2)
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libroute_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libroute_host.so'))
        L.route_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(R.hrl_route_spec), C.c_void_p, C.c_void_p, C.POINTER(R.hrl_route_out), C.c_int]
        L.route_host_last_error.restype = C.c_char_p
        L.route_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(R.hrl_route_spec)]
        L.route_sizeof_spec.restype = C.c_ulonglong
        L.route_sizeof_out.restype = C.c_ulonglong
        L.route_validate_spec.argtypes, L.route_validate_spec.restype = [C.POINTER(R.hrl_route_spec)], C.c_char_p
        L.route_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        L.route_clear.argtypes = [C.c_void_p] + [C.c_int] * 5
        L.route_row_touch.argtypes, L.route_row_touch.restype = [C.c_int] * 5, C.c_ulonglong
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'route_check_main'])
    return os.path.join(DIR, 'route_check_main')


ptr = fc.ptr


def spec_of(fspec, frame=R.HRL_PROBE_WORLD, n_starts=1, max_waypoints=16):
    """The route spec on the field of `fspec` (a field_cases.spec_of record)."""
    return R.from_field_spec(fspec, frame, n_starts, max_waypoints)


def shapes(n, spec):
    p, k = min(max(spec.n_starts, 1), 64), min(max(spec.max_waypoints, 1), 32)
    return ((n, p, k, 2), (n, p), (n, p), (n, p, k))


def route_host(cfg, state, items, aux, spec, starts=None, mask=None, out=None, want=NAMES, how=WALK, expect_ok=True):
    """The host build's routes of (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32) from starts [N, P, 2] f32 (None: the
    robot): a Route of arrays; the members not in `want` are None.  `out`: a Route of arrays (None members are passed as NULL)."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    starts = None if starts is None else np.ascontiguousarray(starts, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    assert starts is None or starts.shape == (n, spec.n_starts, 2)
    if out is None:
        out = Route(*(np.zeros(shape, dt) if name in want else None for name, dt, shape in zip(NAMES, DTYPES, shapes(n, spec))))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = R.hrl_route_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().route_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(starts), ptr(m), C.byref(o), how)
    if expect_ok:
        assert code == K.HRL_OK, lib().route_host_last_error()
        return out
    return code, lib().route_host_last_error().decode()


def bits(route):
    return [None if x is None else (x.view(np.uint32) if x.dtype == np.float32 else x) for x in route]


def same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ clear, exactly
def meets(a, b, c):
    """The segment between the points a and b meets the CLOSED unit square centred on c (pairs of integers; rational arithmetic): the
    parameters t of a + t (b - a) within the square on both axes and within 0..1 form a non-empty interval."""
    t0, t1 = Fraction(0), Fraction(1)
    for x in (0, 1):
        p, d = Fraction(a[x] - c[x]), Fraction(b[x] - a[x])
        if d == 0:
            if abs(p) > HALF:
                return False
            continue
        lo, hi = sorted(((-HALF - p) / d, (HALF - p) / d))
        t0, t1 = max(t0, lo), min(t1, hi)
    return t0 <= t1


@functools.lru_cache(maxsize=None)
def touched(di, dj):
    """The cells (ri, rj), relative to the first, whose closed square the segment from (0, 0) to (di, dj) meets, as two index arrays:
    per row the stretch of the segment inside the row's band (rational) and the columns whose band it overlaps.  Agrees with meets() on
    every cell (asserted for every pair of cells of an 8 x 8 grid by the tests)."""
    rows, cols = [], []
    for ri in range(min(0, di) - 1, max(0, di) + 2):
        if di == 0:
            if ri != 0:
                continue
            t0, t1 = Fraction(0), Fraction(1)
        else:
            lo, hi = sorted(((ri - HALF) / di, (ri + HALF) / di))
            t0, t1 = max(Fraction(0), lo), min(Fraction(1), hi)
            if t0 > t1:
                continue
        xa, xb = sorted((t0 * dj, t1 * dj))
        for rj in range(min(0, dj) - 1, max(0, dj) + 2):
            if rj - HALF <= xb and rj + HALF >= xa:
                rows.append(ri)
                cols.append(rj)
    return np.array(rows), np.array(cols)


def clear(blocked, a, b):
    """No blocked cell of the grid `blocked` [H, W] is met by the segment between the centres of the cells a and b (row, column)."""
    ri, rj = touched(b[0] - a[0], b[1] - a[1])
    i, j = ri + a[0], rj + a[1]
    h, w = blocked.shape
    ok = (i >= 0) & (i < h) & (j >= 0) & (j < w)
    return not blocked[i[ok], j[ok]].any()


def inequality(a, b, c):
    """The header's integer test for a cell c of the bounding box of a and b."""
    di, dj = b[0] - a[0], b[1] - a[1]
    return 2 * abs(dj * (c[0] - a[0]) - di * (c[1] - a[1])) <= abs(di) + abs(dj)


# ------------------------------------------------------------------------------------------------ chain, pull, outputs
def chain(parent, cell):
    """The cells c_0 .. c_L from `cell` down `parent` [H, W]."""
    h, w = parent.shape
    out = [tuple(cell)]
    while parent[out[-1]] != F.SOURCE:
        k = int(parent[out[-1]])
        assert k < 8 and len(out) < h * w
        out.append((out[-1][0] + F.DIRECTIONS[k][1], out[-1][1] + F.DIRECTIONS[k][0]))
        assert 0 <= out[-1][0] < h and 0 <= out[-1][1] < w
    return out


def pull(blocked, cells):
    way, anchor = [cells[0]], cells[0]
    for t in range(1, len(cells)):
        if not clear(blocked, anchor, cells[t]):
            way.append(cells[t - 1])
            anchor = cells[t - 1]
    if len(cells) > 1:
        way.append(cells[-1])
    return way


Ref = collections.namedtuple('Ref', 'count cells length way steps')   # way: every waypoint as (row, col); steps: L


def reference(parent, cell, k, size):
    """The route from `cell` ((row, col), or None for `no route`) on `parent` [H, W] with K = k and cells of `size` metres."""
    w = parent.shape[1]
    if cell is None or parent[cell] > F.SOURCE:
        return Ref(0, [-1] * k, math.inf, [], 0)
    ch = chain(parent, cell)
    way = pull(parent == F.BLOCKED, ch)
    idx = [i * w + j for i, j in way]
    written = idx[:k]
    length = sum(size * math.hypot(b[0] - a[0], b[1] - a[1]) for a, b in zip(way, way[1:]))
    return Ref(len(way), written + [written[-1]] * (k - len(written)), length, way, len(ch) - 1)


BAND = 1e-4   # metres: a start this close to the edge between two cells (or to the grid's) is no case of the sweep


def start_cell(st, fspec, world):
    """(cell or None, near) of a world point: the lowest row and column whose centre lies within half a cell of it on the grid's axes
    (fp64); near = some |distance - cell / 2| is below BAND, so fp32 may decide otherwise."""
    if not (np.isfinite(world).all() and np.isfinite(st[0:2]).all()):
        return None, False
    _, u, v, (c, right, up) = fc.centres(st, fspec)
    half = fc.cell_size(fspec) / 2
    su, sv = (world - c) @ right, (world - c) @ up
    du, dv = np.abs(u - su), np.abs(v - sv)
    near = bool((np.abs(du - half) < BAND).any() or (np.abs(dv - half) < BAND).any())
    cols, rows = np.nonzero(du <= half)[0], np.nonzero(dv <= half)[0]
    if not len(cols) or not len(rows):
        return None, near
    return (int(rows[0]), int(cols[0])), near


def robot_cell(st, fspec, parent):
    """The cell of `starts=None`.  In an ego grid the robot stands on the common corner of the four central cells, an exact tie in fp32
    (field_cases.geometry): the lowest row and column of them."""
    if not np.isfinite(st[0:2]).all():
        return None
    if fspec.mode != F.HRL_VIEW_WORLD:
        return (fspec.height // 2 - 1, fspec.width // 2 - 1)
    cell, near = start_cell(st, fspec, np.array(st[0:2], float))
    assert not near
    return cell


def draw_starts(cfg, state, fspec, frame, n_starts, seed):
    """(starts [N, P, 2] float32 in `frame`, world [N, P, 2] fp64): points at most 0.3 cell from the centre of a cell drawn uniformly from
    the grid grown by two cells on every side (so some lie outside), handed over in the frame's coordinates."""
    rng = np.random.RandomState(seed)
    n, size = cfg.num_envs, fc.cell_size(fspec)
    starts, world = np.zeros((n, n_starts, 2), np.float32), np.zeros((n, n_starts, 2))
    for e in range(n):
        st = state[e] if np.isfinite(state[e][:7]).all() else np.r_[0.0, 0.0, 0.5, 0, 0, 0, 1]
        _, u, v, (c, right, up) = fc.centres(st, fspec)
        j, i = rng.randint(-2, fspec.width + 2, n_starts), rng.randint(-2, fspec.height + 2, n_starts)
        du, dv = rng.uniform(-0.3, 0.3, (2, n_starts)) * size
        uu = u[0] + size * j + du
        vv = v[0] - size * i + dv
        world[e] = c + uu[:, None] * right + vv[:, None] * up
        starts[e] = pc.given_points(st, frame, world[e])
    return starts, world


def check_env(got, e, parent, st, fspec, spec, cells_of_starts, tol):
    """Env e of the host build's (or the device's) Route `got` against the reference on `parent` [H, W]: count and cells exactly,
    waypoints against the fp64 cell centres, length within tol.  Returns (the worst |length - reference|, the references)."""
    pos = fc.centres(st, fspec)[0]
    size = fc.cell_size(fspec)
    k, w = spec.max_waypoints, fspec.width
    worst, refs = 0.0, []
    for p, cell in enumerate(cells_of_starts):
        ref = reference(parent, cell, k, size)
        refs.append(ref)
        assert got.count[e, p] == ref.count, (e, p, cell, got.count[e, p], ref.count)
        assert got.cells[e, p].tolist() == ref.cells, (e, p, cell, got.cells[e, p].tolist(), ref.cells)
        if ref.count == 0:
            assert np.isposinf(got.length[e, p]) and np.isnan(got.waypoints[e, p]).all()
            continue
        want = np.array([pos[c // w, c % w] for c in ref.cells])
        assert np.abs(got.waypoints[e, p] - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (e, p)
        err = abs(float(got.length[e, p]) - ref.length)
        assert err <= tol, (e, p, err)
        worst = max(worst, err)
    return worst, refs
