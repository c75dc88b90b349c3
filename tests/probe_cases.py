"""Shared by tests/test_probe_host.py and tests/test_gpu_probe.py: the ctypes binding of tests/probe_host/libprobe_host.so (the host build
of csrc/probe_core.h), an independent fp64 numpy reference written from include/hrl_probe.h alone (world coordinates, textbook signed
distances, ray tests, Liang-Barsky clipping and a shortest-path relaxation over the corner graph), and the states, points and specs the
tests probe.  Test infrastructure only."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

import render_cases as rc
import scan_cases as sc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import probe_device as P

ROOT = rc.ROOT
DIR = os.path.join(ROOT, 'tests', 'probe_host')
KINDS = rc.KINDS
FRAMES = (P.HRL_PROBE_WORLD, P.HRL_PROBE_EGO, P.HRL_PROBE_HEADING)
COUNTS = (1, 37, 64, 65, 512)    # 65 crosses a wave's run of 64; 1 and 37 leave idle lanes; 512 is the four-wave maximum
MARGINS = (0.0, 0.4)
NAMES = tuple(n for n, _ in P.FIELDS)
DTYPES = (np.float32, np.int32, np.float32, np.int32, np.float32, np.int32)
Probe = collections.namedtuple('Probe', NAMES)   # of numpy arrays
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(['make', '-s', '-C', DIR, 'libprobe_host.so'])
        L = C.CDLL(os.path.join(DIR, 'libprobe_host.so'))
        L.probe_host.argtypes = [C.POINTER(K.hrl_config), C.POINTER(K.hrl_buffers), C.POINTER(P.hrl_probe_spec), C.c_void_p, C.c_void_p, C.POINTER(P.hrl_probe_out)]
        L.probe_host_last_error.restype = C.c_char_p
        L.probe_host_default_spec.argtypes = [C.POINTER(K.hrl_config), C.c_int32, C.POINTER(P.hrl_probe_spec)]
        L.probe_sizeof_spec.restype = C.c_ulonglong
        L.probe_sizeof_out.restype = C.c_ulonglong
        L.probe_validate_spec.argtypes, L.probe_validate_spec.restype = [C.POINTER(P.hrl_probe_spec)], C.c_char_p
        L.probe_check_case.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def check_program():
    subprocess.check_call(['make', '-s', '-C', DIR, 'probe_check_main'])
    return os.path.join(DIR, 'probe_check_main')


ptr = rc.ptr


def spec_of(n_points, frame, margin, classes=P.ALL):
    return P.hrl_probe_spec(n_points=n_points, frame=frame, classes=classes, margin=margin)


def all_specs():
    return [spec_of(n, f, m) for n in COUNTS for f in FRAMES for m in MARGINS]


def probe_host(cfg, state, items, aux, spec, points, mask=None, out=None, want=NAMES, expect_ok=True):
    """The host build's probes of (state [N, 32] f32, items [N, stride] f32 or None, aux [N, 4] i32, points [N, P, 2] f32): a Probe of
    arrays [N, n_points]; the fields not in `want` are None.  `out`: a Probe of arrays (None fields are passed as NULL) to write into."""
    state, aux = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(aux, np.int32)
    items = None if items is None else np.ascontiguousarray(items, np.float32)
    points = None if points is None else np.ascontiguousarray(points, np.float32)
    n = cfg.num_envs
    assert state.shape == (n, K.HRL_STATE_STRIDE) and aux.shape == (n, K.HRL_AUX_STRIDE)
    if out is None:
        out = Probe(*(np.zeros((n, max(spec.n_points, 1)), dt) if name in want else None for name, dt in zip(NAMES, DTYPES)))
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    b = K.make_buffers(ptr(state), ptr(items), ptr(aux), None, None, None, None, None)
    o = P.hrl_probe_out(**{name: ptr(a) for name, a in zip(NAMES, out)})
    code = lib().probe_host(C.byref(cfg), C.byref(b), C.byref(spec), ptr(points), ptr(m), C.byref(o))
    if expect_ok:
        assert code == K.HRL_OK, lib().probe_host_last_error()
        return out
    return code, lib().probe_host_last_error().decode()


# ------------------------------------------------------------------------------------------------ the fp64 reference
arena = rc.arena   # half sizes of the planes the robot collides with (the walls' inner faces), or None
BOX_C, BOX_H = np.array([-2.0, 0.0]), np.array([3.0, 2.0])
CORNER_SIGNS = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], float)
PLANES = (((-1.0, 0.0), 0), ((1.0, 0.0), 0), ((0.0, -1.0), 1), ((0.0, 1.0), 1))   # normal, which half size is the offset


def is_maze(cfg):
    return cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ)


def shapes(cfg, items, aux):
    """The env's shapes in table order, world coordinates: (class bit, code, type, parameters)."""
    out = [s for s in sc.shapes(cfg, items, aux) if s[2] != 'half']
    ar = arena(cfg)
    walls = [] if ar is None else [(P.WALL, P.HIT_WALL | i << 8, 'half', (n, ar[a])) for i, (n, a) in enumerate(PLANES)]
    return walls + out


def world_points(st, frame, pts):
    """Query points as given (fp32 values) -> world positions, fp64."""
    pts = np.asarray(pts, float)
    o = np.array([st[0], st[1]], float)
    if frame == P.HRL_PROBE_WORLD:
        return pts.copy()
    f = sc.forward(st, sc.S.HRL_SCAN_HEADING if frame == P.HRL_PROBE_HEADING else sc.S.HRL_SCAN_WORLD)
    left = np.array([-f[1], f[0]])
    return o + pts[:, :1] * f + pts[:, 1:] * left


def given_points(st, frame, world):
    """World positions -> the query points to hand over in `frame`, float32."""
    world = np.asarray(world, float)
    o = np.array([st[0], st[1]], float)
    if frame == P.HRL_PROBE_WORLD:
        return world.astype(np.float32)
    f = sc.forward(st, sc.S.HRL_SCAN_HEADING if frame == P.HRL_PROBE_HEADING else sc.S.HRL_SCAN_WORLD)
    left = np.array([-f[1], f[0]])
    d = world - o
    return np.stack([d @ f, d @ left], 1).astype(np.float32)


def ref_clearance(shp, classes, w):
    best, who = np.full(len(w), np.inf), np.zeros(len(w), np.int64)
    for cls, code, typ, p in shp:
        if not classes & cls:
            continue
        if typ == 'half':
            (nx, ny), off = p
            d = nx * w[:, 0] + ny * w[:, 1] + off
        elif typ == 'rect':
            (cx, cy), (hx, hy) = p
            d = rc._sd_rect(w[:, 0], w[:, 1], (cx, cy), hx, hy)
        else:
            (cx, cy), r = p
            d = np.hypot(w[:, 0] - cx, w[:, 1] - cy) - r
        if not np.isfinite([v for q in p for v in np.ravel(q)]).all():
            continue
        take = d < best
        best, who = np.where(take, d, best), np.where(take, code, who)
    return best, who


def ref_sight(shp, classes, o, w):
    d = w - o
    L = np.hypot(d[:, 0], d[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        dx, dy = d[:, 0] / L, d[:, 1] / L
    best, who = np.full(len(w), np.inf), np.zeros(len(w), np.int64)
    for cls, code, typ, p in shp:
        if not classes & cls or not np.isfinite([v for q in p for v in np.ravel(q)]).all():
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            if typ == 'half':
                (nx, ny), off0 = p
                off, den = nx * o[0] + ny * o[1] + off0, nx * dx + ny * dy
                t = np.zeros_like(dx) if off < 0 else np.where(den < 0, off / -np.where(den < 0, den, -1.0), np.inf)
            elif typ == 'rect':
                (cx, cy), (hx, hy) = p
                ts = []
                for lo, hi, oo, dd in ((cx - hx, cx + hx, o[0], dx), (cy - hy, cy + hy, o[1], dy)):
                    a, b = (lo - oo) / dd, (hi - oo) / dd
                    par, inside = dd == 0, lo <= oo <= hi
                    ts.append((np.where(par, -np.inf if inside else np.inf, np.minimum(a, b)), np.where(par, np.inf if inside else -np.inf, np.maximum(a, b))))
                tn, tf = np.maximum(ts[0][0], ts[1][0]), np.minimum(ts[0][1], ts[1][1])
                t = np.where((tn <= tf) & (tf >= 0), np.maximum(tn, 0.0), np.inf)
            else:
                (cx, cy), r = p
                ex, ey = cx - o[0], cy - o[1]
                b, cc = ex * dx + ey * dy, ex * ex + ey * ey
                h = b * b - cc + r * r
                t = np.zeros_like(dx) if cc <= r * r else np.where((h >= 0) & (b > 0), b - np.sqrt(np.maximum(h, 0.0)), np.inf)
        take = (t < L) & (t < best)
        best, who = np.where(take, t, best), np.where(take, code, who)
    return np.where(who != 0, best, np.where(L > 0, L, 0.0)), who


def crosses(a, b, c, h):
    """Liang-Barsky: the segments a -> b[i] overlap the open rectangle c +- h over a stretch of positive length.  a [2], b [n, 2]."""
    t0, t1 = np.zeros(len(b)), np.ones(len(b))
    ok = np.ones(len(b), bool)
    for ax in range(2):
        d = b[:, ax] - a[ax]
        lo, hi = c[ax] - h[ax] - a[ax], c[ax] + h[ax] - a[ax]
        par = d == 0
        with np.errstate(divide='ignore', invalid='ignore'):
            ta, tb = lo / d, hi / d
        t0 = np.where(par, t0, np.maximum(t0, np.minimum(ta, tb)))
        t1 = np.where(par, t1, np.minimum(t1, np.maximum(ta, tb)))
        ok &= ~par | ((lo < 0) & (0 < hi))
    return ok & (t0 < t1)


def ref_path(cfg, o, w, margin):
    """(path [n], via [n], gap [n]): gap = how much longer the best route with another `via` is (inf when there is none)."""
    ar = arena(cfg)
    planes = [] if ar is None else [(np.array(n), ar[a]) for n, a in PLANES]
    box = is_maze(cfg)
    s, d0 = np.array(o, float), 0.0
    for n, off in planes:
        lack = margin - (n @ s + off)
        if lack > 0:
            s, d0 = s + n * lack, d0 + lack
    hb = BOX_H + margin
    if box and (np.abs(s - BOX_C) < hb).all():
        hn = hb + P.SKIN
        moves = [BOX_C[0] + hn[0] - s[0], s[0] - (BOX_C[0] - hn[0]), BOX_C[1] + hn[1] - s[1], s[1] - (BOX_C[1] - hn[1])]
        k = int(np.argmin(moves))   # (the first of equal ones)
        d0 += moves[k]
        s = np.array([(BOX_C[0] + hn[0], BOX_C[0] - hn[0], s[0], s[0])[k], (s[1], s[1], BOX_C[1] + hn[1], BOX_C[1] - hn[1])[k]])
    free = np.ones(len(w), bool)
    for n, off in planes:
        free &= w @ n + off >= margin
    cross = (lambda a, b: crosses(a, b, BOX_C, hb)) if box else (lambda a, b: np.zeros(len(b), bool))
    if box:
        free &= ~(np.abs(w - BOX_C) < hb).all(1)
    routes = [np.where(cross(s, w), np.inf, np.hypot(*(w - s).T))]   # route 0: straight; route 1 + k: first turns at corner k
    if box:
        nodes = BOX_C + CORNER_SIGNS * (hb + P.SKIN)
        counts = np.array([all(n @ q + off >= margin for n, off in planes) for q in nodes])
        g = np.where(counts & ~cross(s, nodes), np.hypot(*(nodes - s).T), np.inf)
        first = np.arange(4)
        for _ in range(3):
            g2, f2 = g.copy(), first.copy()
            for k in range(4):
                for j in range(4):
                    if j != k and counts[k] and np.isfinite(g[j]) and not cross(nodes[j], nodes[k:k + 1])[0]:
                        cand = g[j] + np.hypot(*(nodes[k] - nodes[j]))
                        if cand < g2[k]:
                            g2[k], f2[k] = cand, first[j]
            g, first = g2, f2
        per_first = [np.full(len(w), np.inf) for _ in range(4)]
        for k in range(4):
            if np.isfinite(g[k]):
                r = np.where(cross(nodes[k], w), np.inf, g[k] + np.hypot(*(w - nodes[k]).T))
                per_first[first[k]] = np.minimum(per_first[first[k]], r)
        routes += per_first
    r = np.stack(routes, 1)
    best = r.min(1)
    via = np.where(np.isfinite(best), r.argmin(1) + 1, 0)
    second = np.sort(r, 1)[:, 1] if r.shape[1] > 1 else np.full(len(w), np.inf)
    with np.errstate(invalid='ignore'):
        gap = np.where(np.isfinite(second), second - best, np.inf)
    path = np.where(free & np.isfinite(best), d0 + best, np.inf)
    return path, np.where(free, via, 0), gap


def reference(cfg, st, items, aux, spec, pts, shift=(0.0, 0.0)):
    """The six answers of one env in fp64 (and `gap`, see ref_path), with every query point moved by `shift` in world coordinates."""
    o = np.array([st[0], st[1]], float)
    w = world_points(st, spec.frame, pts) + np.asarray(shift, float)
    shp = shapes(cfg, items, aux)
    c, n = ref_clearance(shp, spec.classes, w)
    s, b = ref_sight(shp, spec.classes, o, w)
    p, v, gap = ref_path(cfg, o, w, float(spec.margin))
    bad = ~(np.isfinite(o).all() & np.isfinite(np.asarray(pts, float)).all(1) & np.isfinite(w).all(1))
    c, n, s, b, p, v = (np.where(bad, blank, x) for x, blank in zip((c, n, s, b, p, v), (np.inf, 0, 0.0, 0, np.inf, 0)))
    return Probe(c, n, s, b, p, v), gap


SHIFTS = ((1e-4, 0.0), (-1e-4, 0.0), (0.0, 1e-4), (0.0, -1e-4))


def _err(got, want):
    with np.errstate(invalid='ignore'):
        return np.where(got == want, 0.0, np.abs(got.astype(float) - want))   # (inf against inf: 0; inf against a number: inf)


def compare(cfg, state, items, aux, spec, points, got, tol):
    """The host build (or anything else) against the reference, env by env.  Returns a dict of [N, P] arrays:
    exempt_nearest / exempt_blocker / exempt_via0: the reference's identity changes when the point moves by +-1e-4 m along x or y;
    wrong_nearest / wrong_blocker / wrong_via0: identity mismatches among the others; wrong_via: `via` differs where both are reachable,
    the identity is stable and the reference's best and second-best routes differ by more than `tol`;
    err_clearance / err_sight / err_path: |got - reference| where the identity is compared (0 elsewhere)."""
    n, p = cfg.num_envs, spec.n_points
    keys = ('exempt_nearest', 'exempt_blocker', 'exempt_via0', 'wrong_nearest', 'wrong_blocker', 'wrong_via0', 'wrong_via')
    out = {k: np.zeros((n, p), bool) for k in keys}
    out.update({k: np.zeros((n, p)) for k in ('err_clearance', 'err_sight', 'err_path')})
    for e in range(n):
        it = None if items is None else items[e]
        ref, gap = reference(cfg, state[e], it, aux[e], spec, points[e])
        for sh in SHIFTS:
            r2, _ = reference(cfg, state[e], it, aux[e], spec, points[e], sh)
            out['exempt_nearest'][e] |= r2.nearest != ref.nearest
            out['exempt_blocker'][e] |= r2.blocker != ref.blocker
            out['exempt_via0'][e] |= (r2.via == 0) != (ref.via == 0)
        out['wrong_nearest'][e] = (got.nearest[e] != ref.nearest) & ~out['exempt_nearest'][e]
        out['wrong_blocker'][e] = (got.blocker[e] != ref.blocker) & ~out['exempt_blocker'][e]
        out['wrong_via0'][e] = ((got.via[e] == 0) != (ref.via == 0)) & ~out['exempt_via0'][e]
        out['wrong_via'][e] = (got.via[e] != ref.via) & (ref.via != 0) & (got.via[e] != 0) & ~out['exempt_via0'][e] & (gap > tol)
        out['err_clearance'][e] = np.where(out['exempt_nearest'][e], 0.0, _err(got.clearance[e], ref.clearance))
        out['err_sight'][e] = np.where(out['exempt_blocker'][e], 0.0, _err(got.sight[e], ref.sight))
        out['err_path'][e] = np.where(out['exempt_via0'][e], 0.0, _err(got.path[e], ref.path))
    return out


# ------------------------------------------------------------------------------------------------ states and points
hand_made = rc.hand_made
far_targets = rc.far_targets


SPREAD = ((3.0, 6.0), (1.2, 0.5), (-3.0, 5.0), (4.0, -8.0), (0.5, -3.0))


def spread(cfg, state):
    """A copy of a state array [N >= 5, 32] with the robots of envs 0..4 put about the arena: above the maze box, leaning on its +x
    side, in the far corner behind it, a metre from two walls, and below the box (the shards' robots all stand near the start)."""
    s = state.copy()
    s[:5, 0:2] = SPREAD
    ar = arena(cfg)
    if ar is not None and ar != rc.DEFAULT_ARENA[cfg.env_kind]:   # another arena than the kind's default: the same places, scaled from the maze's 5 x 9 into it
        s[:5, 0:2] = np.array(SPREAD) * (ar[0] / 5.0, ar[1] / 9.0)
    return s


def extent(cfg):
    """Half sizes of the box the query points are drawn from: the arena's (6 x 6 where there is none) grown by 1 m."""
    ar = arena(cfg)
    return (7.0, 7.0) if ar is None else (ar[0] + 1.0, ar[1] + 1.0)


def draw_points(cfg, state, frame, n_points, seed):
    """[N, n_points, 2] float32 in `frame`: world positions drawn from a seeded uniform distribution over extent(cfg) (no grid: grid
    lines fall on the box's edges), handed over in the frame's coordinates."""
    rng = np.random.RandomState(seed)
    hx, hy = extent(cfg)
    out = np.zeros((cfg.num_envs, n_points, 2), np.float32)
    for e in range(cfg.num_envs):
        w = rng.uniform(-1, 1, (n_points, 2)) * (hx, hy)
        st = state[e] if np.isfinite(state[e][:7]).all() else np.r_[0.0, 0.0, 0.5, 0, 0, 0, 1]
        out[e] = given_points(st, frame, w)
    return out


def seed_of(cfg, spec):
    return 1000 * cfg.env_kind + 100 * spec.frame + spec.n_points + (7 if spec.margin else 0)


def hostile(cfg, state, items, aux):
    """Hostile copies of a shard of >= 5 envs: a list of (state, items, aux, cleaned state, cleaned items, cleaned aux, far, blind).  The
    cleaned record has the offending shape where no probe of the arena meets it (an item at (100, 0) as an eaten one is; a flagrun goal:
    no items record at all, which leaves out the goal alone); far: probe the cleaned record with far_targets(cfg) and classes without
    TARGET; blind: the rows whose robot stands at a non-finite place and must get the blank answers."""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        s, it, a = state.copy(), None if items is None else items.copy(), aux.copy()
        cs, cit, ca = state.copy(), None if items is None else items.copy(), aux.copy()
        s[0, 0] = bad
        s[1, 1] = bad
        if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
            it[2, 0] = bad; cit[2, 0:2] = (100.0, 0.0)
            it[3, 2 * cfg.n_food + 1] = bad; cit[3, 2 * cfg.n_food:2 * cfg.n_food + 2] = (100.0, 0.0)
        if cfg.env_kind == K.HRL_ANT_FLAGRUN:
            it[:, 1] = bad; cit = None
        out.append((s, it, a, cs, cit, ca, False, (0, 1)))
    if cfg.env_kind != K.HRL_ANT_FLAGRUN:
        s, it, a = state.copy(), None if items is None else items.copy(), aux.copy()
        a[:, 3] = (1000, -5, 2 ** 31 - 1, -2 ** 31, 64)[:len(a)]
        ca = a.copy()
        ca[:, 3] = 0
        out.append((s, it, a, s.copy(), None if it is None else it.copy(), ca, True, ()))
    return out


def hostile_points(points):
    """A copy of points [N, P >= 8, 2] with NaN, +-inf and 1e20 in some coordinates, and the rows (point indices) that must be blank."""
    p = points.copy()
    p[:, 0, 0] = np.nan
    p[:, 1, 1] = np.inf
    p[:, 2, 0] = -np.inf
    p[:, 3] = (np.nan, np.inf)
    p[:, 5] = (1e20, -1e20)
    p[:, 6, 0] = 3.2e38
    return p, (0, 1, 2, 3), (5, 6)


def is_blank(got, rows=None, cols=None):
    sel = (slice(None) if rows is None else list(rows), slice(None) if cols is None else list(cols))
    if rows is not None and cols is not None:
        sel = np.ix_(list(rows), list(cols))
    return all((x[sel] == v).all() for x, v in zip(got, (np.inf, 0, 0.0, 0, np.inf, 0)) if x is not None)
