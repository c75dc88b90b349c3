/*
 * route_core.h -- specification of the batched routes (include/hrl_route.h), written once as plain C++: the device kernel
 * (route_hip.hip) and the host build of the tests (tests/route_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The route of one (env, start) is a pure function of (DevCfg, the env's state / items / aux record, hrl_route_spec, the start point):
 *
 *   field       field_core.h's, for field_part(spec): the padded image and the bytes of admissible steps from field::cell_init, cell_adm
 *               and cell_relax, parent = field::cell_parent.  Nothing of it is restated here
 *   start_uv    the start in the view's coordinates: probe::locate (the probe's frames, its tests for a finite point and robot) and
 *               field::table_to_view
 *   col_holds / the tests that name the start's column and row: the LOWEST j with |pix_u(j) - u| <= half, the lowest i likewise --
 *   row_holds   cell_init's test for a source cell, so a start on a source's point lies on a source cell.  No float becomes an integer
 *   trace       chain and pull in one walk: c_{t+1} = c_t moved by parent[c_t], at most W H cells (the field's bound on a way, an integer
 *               of the spec); whenever the anchor is not clear of c_t, c_{t-1} is emitted and becomes the anchor; c_L is emitted last
 *   clear       integers only.  clear_walk is the definition: every cell of the bounding box is asked `touches` and `blocked`.
 *               row_touch gives the same set a row at a time, as an interval of columns, for rows kept as 64-bit masks of blocked cells:
 *               the device asks one row per lane and decides with one ballot.  The host build computes both and the tests compare them
 *               on every pair of cells
 *
 * clear(c_{t-1}, c_t) ALWAYS HOLDS: the bounding box of an orthogonal step is the two cells themselves, both free; that of a diagonal
 * step holds the two cells orthogonally adjacent to both as well, which the segment touches in a corner (2 |dj . 0 - di dj| = 2 = |di| +
 * |dj|) and which field::cell_adm demands free.  So after an emit the new anchor c_{t-1} is clear of c_t, and consecutive waypoints are
 * clear of each other.
 *
 * Totality: the field's.  The walk's addresses derive from the parent bytes and from cell indices found by comparisons; a start that is
 * not finite, outside the grid or on a cell without a way gets `no route` (count 0, length +inf, cells -1, waypoints NaN).
 */
#pragma once
#include "../../include/hrl_route.h"
#include "field_core.h" /* Grid, Frames, table_to_view, cell_centre, dcol, drow (and through it probe_core.h: ProbeSet, build_frame, locate) */

#ifdef HRL_EMU
#define HRL_BOTH inline
#else
#define HRL_BOTH __host__ __device__ __forceinline__
#endif

namespace hrl {
namespace route {

using field::Frames;
using field::Grid;
using probe::ProbeSet;
using render::inf_;

constexpr int MAX_STARTS = HRL_ROUTE_MAX_STARTS, MAX_WAYPOINTS = HRL_ROUTE_MAX_WAYPOINTS, MAX_SIZE = field::MAX_SIZE, MAX_CELLS = field::MAX_CELLS;
static_assert(MAX_SIZE <= 64, "a row of blocked cells is one 64-bit mask; a lane per row or column");
static_assert(2 * MAX_WAYPOINTS <= 64, "one wave stores the waypoints of a start");

/* the spec's field part as the field's own record */
HRL_BOTH hrl_field_spec field_part(const hrl_route_spec &sp) {
    hrl_field_spec f = {};
    f.struct_size = sizeof f; f.width = sp.width; f.height = sp.height; f.mode = sp.mode;
    f.centre[0] = sp.centre[0]; f.centre[1] = sp.centre[1]; f.half_extent = sp.half_extent;
    f.blocking = sp.blocking; f.sources = sp.sources; f.margin = sp.margin;
    return f;
}
/* what probe::build_frame and locate read of a probe spec */
HRL_DEV hrl_probe_spec frame_spec(int frame) {
    hrl_probe_spec p = {};
    p.struct_size = sizeof p; p.n_points = 1; p.frame = frame; p.classes = HRL_SCAN_ALL;
    return p;
}

/* a wave-uniform integer: on the device in a scalar register, so the walk below branches uniformly */
#if defined(__HIP_DEVICE_COMPILE__)
HRL_DEV int uniform_(int x) { return __builtin_amdgcn_readfirstlane(x); }
#else
HRL_DEV int uniform_(int x) { return x; }
#endif

/* ------------------------------------------------------------------------------------------------ the start */
/* S: fwd, org and robot_ok are read (probe::build_frame).  False = no route. */
HRL_DEV bool start_uv(const ProbeSet &S, const Frames &f, int frame, float px, float py, float *u, float *v) {
    float qx, qy;
    const bool ok = probe::locate(S, frame, px, py, &qx, &qy);
    field::table_to_view(f, qx, qy, u, v);
    return ok;
}
HRL_DEV bool col_holds(const Grid &g, float u, int j) { return fabsf(render::pix_u(j, g.W, g.inv_w, g.he) - u) <= g.half; }
HRL_DEV bool row_holds(const Grid &g, float v, int i) { return fabsf(render::pix_v(i, g.H, g.inv_w, g.he) - v) <= g.half; }

/* ------------------------------------------------------------------------------------------------ clear */
HRL_DEV int abs_(int x) { return x < 0 ? -x : x; }
HRL_DEV int floor_div(int n, int d) { /* d > 0 */
    const int q = n / d;
    return n - q * d < 0 ? q - 1 : q;
}
/* the closed square of the cell at (ri, rj) from a meets the segment from a to a + (di, dj) -- for a cell of their bounding box */
HRL_DEV bool touches(int di, int dj, int ri, int rj) { return 2 * abs_(dj * ri - di * rj) <= abs_(di) + abs_(dj); }
/* rows[i]: bit j set = cell (i, j) is blocked */
HRL_DEV bool clear_walk(const unsigned long long *rows, int i0, int j0, int i1, int j1) {
    const int di = i1 - i0, dj = j1 - j0;
    const int ia = i0 < i1 ? i0 : i1, ib = i0 < i1 ? i1 : i0, ja = j0 < j1 ? j0 : j1, jb = j0 < j1 ? j1 : j0;
    bool ok = true;
    for (int i = ia; i <= ib; ++i)
        for (int j = ja; j <= jb; ++j) ok = ok && !(touches(di, dj, i - i0, j - j0) && ((rows[i] >> j) & 1ull) != 0ull);
    return ok;
}
/* the cells of row i that clear_walk asks `blocked`, as a mask of columns; 0 for a row outside the bounding box.  With x = j - j0,
 * A = 2 dj (i - i0) and s = |di| + |dj| the test is |A - 2 di x| <= s: for di != 0 the integers x of [(A' - s) / D, (A' + s) / D] with
 * D = 2 |di| and A' = A sign(di); for di = 0 the one row i0, whole. */
HRL_DEV unsigned long long row_touch(int i0, int j0, int i1, int j1, int i) {
    const int di = i1 - i0, dj = j1 - j0;
    const int ia = i0 < i1 ? i0 : i1, ib = i0 < i1 ? i1 : i0, ja = j0 < j1 ? j0 : j1, jb = j0 < j1 ? j1 : j0;
    int lo = ja, hi = jb;
    if (di != 0) {
        const int D = 2 * abs_(di), A = (di < 0 ? -2 : 2) * dj * (i - i0), s = abs_(di) + abs_(dj);
        const int xlo = -floor_div(s - A, D), xhi = floor_div(A + s, D); /* ceil((A - s) / D), floor((A + s) / D) */
        lo = j0 + xlo > ja ? j0 + xlo : ja;
        hi = j0 + xhi < jb ? j0 + xhi : jb;
    }
    const bool any = i >= ia && i <= ib && lo <= hi;
    const int l = any ? lo : 0, h = any ? hi : 0; /* (shift counts within 0..63 whatever i is) */
    const unsigned long long m = (~0ull >> (63 - (h - l))) << l;
    return any ? m : 0ull;
}

/* ------------------------------------------------------------------------------------------------ chain and pull */
HRL_DEV float seg_len(const Grid &g, int di, int dj) { return g.cell * sqrtf((float)(di * di + dj * dj)); }

/* The route from the cell (i, j), which has a way (parent <= HRL_FIELD_SOURCE): its cells into stage[0 .. min(count, K) - 1], its count
 * and length.  par: the parent bytes [H][W].  clear(ai, aj, i, j): the anchor is clear of the cell.  Everything here is the same in
 * every lane of a wave. */
template <class Clear>
HRL_DEV void trace(const uint8_t *par, const Grid &g, int i, int j, int K, int32_t *stage, Clear clear, int *count, float *length) {
    int ai = i, aj = j, n = 1;
    float len = 0.f;
    stage[0] = i * g.W + j;
    const int cap = g.W * g.H;
    bool moved = false;
    for (int t = 0; t < cap; ++t) {
        const int k = uniform_((int)par[i * g.W + j]);
        if (k > 7) break; /* SOURCE: c_L */
        const int ni = i + field::drow(k), nj = j + field::dcol(k);
        if (!clear(ai, aj, ni, nj)) {
            len += seg_len(g, i - ai, j - aj);
            if (n < K) stage[n] = i * g.W + j;
            ++n; ai = i; aj = j;
        }
        i = ni; j = nj; moved = true;
    }
    if (moved) {
        len += seg_len(g, i - ai, j - aj);
        if (n < K) stage[n] = i * g.W + j;
        ++n;
    }
    *count = n; *length = len;
}
/* the world position of a cell's centre: cell_centre's q plus the table frame's centre */
HRL_DEV void waypoint_of(const Grid &g, const Frames &f, int cell, float *x, float *y) {
    const int i = cell / g.W, j = cell - i * g.W;
    float u, v, qx, qy;
    field::cell_centre(g, f, i, j, &u, &v, &qx, &qy);
    *x = qx + f.T.cx; *y = qy + f.T.cy;
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_route_spec *s) {
    if (!s) return "null route spec";
    if (s->struct_size != sizeof(hrl_route_spec)) return "hrl_route_spec.struct_size is not sizeof(hrl_route_spec): initialise the record with hrl_route_default_spec()";
    const hrl_field_spec f = field_part(*s);
    const std::string why = field::validate_spec(&f);
    if (!why.empty()) return "route " + why;
    if (s->n_starts < 1 || s->n_starts > MAX_STARTS) return "route n_starts must be within 1..64";
    if (s->frame != HRL_PROBE_WORLD && s->frame != HRL_PROBE_EGO && s->frame != HRL_PROBE_HEADING) return "unknown route frame";
    if (s->max_waypoints < HRL_ROUTE_MIN_WAYPOINTS || s->max_waypoints > MAX_WAYPOINTS) return "route max_waypoints must be within 2..32";
    return "";
}
inline std::string validate_out(const hrl_route_out *o) {
    if (!o) return "null route out";
    if (!o->waypoints && !o->count && !o->length && !o->cells) return "route out holds no pointer: at least one output must be given";
    return "";
}
inline int default_spec(const hrl_config *c, int32_t mode, hrl_route_spec *s) {
    hrl_field_spec f;
    if (!s || field::default_spec(c, mode, &f) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->width = f.width; s->height = f.height; s->mode = f.mode;
    s->centre[0] = f.centre[0]; s->centre[1] = f.centre[1]; s->half_extent = f.half_extent;
    s->blocking = f.blocking; s->sources = f.sources; s->margin = f.margin;
    s->n_starts = 1; s->frame = HRL_PROBE_EGO; s->max_waypoints = 16;
    return HRL_OK;
}

#ifdef HRL_EMU
constexpr int CLEAR_WALK = 0, CLEAR_ROWS = 1; /* clear by its definition | a row at a time through row_touch, as the device decides it */

/* the answers of one start into the outputs: n = 0 is `no route` */
inline void store_route(const Grid &g, const Frames &f, int K, const int32_t *stage, int n, float len, const hrl_route_out &out, size_t at) {
    if (out.count) out.count[at] = n;
    if (out.length) out.length[at] = n > 0 ? len : inf_();
    const int written = n < K ? n : K;
    for (int k = 0; k < K; ++k) {
        const int cell = n > 0 ? stage[k < written ? k : written - 1] : -1;
        float x = __builtin_nanf(""), y = __builtin_nanf("");
        if (n > 0) waypoint_of(g, f, cell, &x, &y);
        if (out.cells) out.cells[at * K + k] = cell;
        if (out.waypoints) { out.waypoints[(at * K + k) * 2] = x; out.waypoints[(at * K + k) * 2 + 1] = y; }
    }
}
/* One env on the host.  starts: [n_starts][2] or null (the robot). */
inline void route_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_route_spec &sp, const float *starts, int how, const hrl_route_out &out,
                           size_t at) {
    static thread_local uint8_t par[MAX_CELLS];
    static thread_local ProbeSet S;
    const hrl_field_spec fs = field_part(sp);
    const hrl_field_out fo = {nullptr, par};
    field::field_env_host(c, st, items, aux, fs, field::SCHED_JACOBI, fo, 0);
    const Grid g = field::grid_of(fs);
    const Frames f = field::frames_of(st, fs);
    probe::build_frame(S, st, frame_spec(sp.frame));
    unsigned long long rows[MAX_SIZE];
    for (int i = 0; i < g.H; ++i) {
        rows[i] = 0ull;
        for (int j = 0; j < g.W; ++j) rows[i] |= par[i * g.W + j] == HRL_FIELD_BLOCKED ? 1ull << j : 0ull;
    }
    const int K = sp.max_waypoints;
    for (int p = 0; p < sp.n_starts; ++p) {
        float u, v;
        const bool ok = starts ? start_uv(S, f, sp.frame, starts[2 * p], starts[2 * p + 1], &u, &v) : start_uv(S, f, HRL_PROBE_EGO, 0.f, 0.f, &u, &v);
        int i = -1, j = -1;
        for (int k = g.W - 1; k >= 0; --k) j = col_holds(g, u, k) ? k : j;
        for (int k = g.H - 1; k >= 0; --k) i = row_holds(g, v, k) ? k : i;
        int32_t stage[MAX_WAYPOINTS];
        int n = 0;
        float len = 0.f;
        if (ok && i >= 0 && j >= 0 && par[i * g.W + j] <= HRL_FIELD_SOURCE) {
            auto clear = [&](int ai, int aj, int bi, int bj) {
                if (how == CLEAR_WALK) return clear_walk(rows, ai, aj, bi, bj);
                bool hit = false;
                for (int r = 0; r < g.H; ++r) hit = hit || (row_touch(ai, aj, bi, bj, r) & rows[r]) != 0ull;
                return !hit;
            };
            trace(par, g, i, j, K, stage, clear, &n, &len);
        }
        store_route(g, f, K, stage, n, len, out, at + (size_t)p);
    }
}
/* hrl_route on host pointers; returns the status and leaves the reason in `why` */
inline int route_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_route_spec *sp, const float *starts, const uint8_t *mask, const hrl_route_out *out, int how,
                            std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (why.empty() && how != CLEAR_WALK && how != CLEAR_ROWS) why = "unknown way to decide clear";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        route_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp,
                       starts ? starts + (size_t)e * sp->n_starts * 2 : nullptr, how, *out, (size_t)e * sp->n_starts);
    }
    return HRL_OK;
}
#endif

}  // namespace route
}  // namespace hrl
