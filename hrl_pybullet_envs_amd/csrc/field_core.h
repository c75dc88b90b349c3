/*
 * field_core.h -- specification of the batched navigation field (include/hrl_field.h), written once as plain C++: the device kernel
 * (field_hip.hip) and the host build of the tests (tests/field_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The field of one env is a pure function of (DevCfg, its state / items / aux record, hrl_field_spec):
 *
 *   frames        V = the renderer's camera of (mode, centre) (render_core.h: view_frame); T = the probe's table frame, centred on the
 *                 robot with WORLD axes (scan_core.h: table_frame) -- on the world's origin when the robot's place is not finite;
 *                 off = V's centre - T's centre, exactly (0, 0) in the ego modes
 *   build_entry   entry s < S_SLOTS of the table: the probe's slot s (probe_core.h: build_slot, so make_prim's primitive with a plane
 *                 where the robot collides with it) in T, whether it BLOCKS (kept, class in spec.blocking) and whether it is a SOURCE
 *                 (kept, class in spec.sources), and its centre in V's coordinates (to_view's operations).  Entry S_SLOTS is the robot:
 *                 a source when HRL_FIELD_ROBOT is asked for and its x, y are finite
 *   cell_centre   (u, v) of cell (i, j) = the renderer's pixel centre (pix_u, pix_v), and the same point in T:
 *                 q = off + u right + v up
 *   cell_init     the cell's first value: 0 on a source cell (|u - su| <= cell / 2 and |v - sv| <= cell / 2 for a source entry), else
 *                 +inf on a free cell (q finite and probe::sdist(entry, q) >= margin for every blocking entry), else BLOCKED_ (-1)
 *   cell_adm      bit k of a free cell that is no source = step k is admissible: the neighbour is not blocked and, for a diagonal step,
 *                 neither is either of the two cells orthogonally adjacent to both.  0 on source and blocked cells: they never change
 *   cell_relax    min(d(c), min over admissible k of d(neighbour_k) + w_k)
 *   cell_parent   the code of hrl_field_out.parent from the converged values
 *
 * The values live in a padded image of (H + 2) x (W + 2) floats whose outer ring is blocked, so no step tests the grid's edge.
 *
 * THE FIXED POINT IS UNIQUE AND DOES NOT DEPEND ON THE ORDER OF RELAXATION.  Every value starts at +inf (sources at 0) and only ever
 * decreases; a value is at any time the fp32 length fl(...fl(fl(0 + w_a) + w_b)... + w_z) of some way to a source, summed from the source
 * outwards.  fl(d + w) is non-decreasing in d, and it is strictly larger than d for every d that can occur: d <= W H w2 < 5800 cell, whose
 * ulp is below 5e-4 cell, and w >= cell.  So the usual argument for Bellman-Ford holds in fp32: by induction over the number of steps the
 * smallest such length D(c) is reached by every schedule that relaxes every cell until nothing changes, no value can fall below it, and D
 * satisfies d(c) = min_k fl(d(neighbour_k) + w_k) with equality.  A way has fewer than W H cells, so W H Jacobi rounds always suffice;
 * that integer of the spec caps the loop.  The host build runs Jacobi rounds or in-place sweeps in either raster order (`schedule`), the
 * device relaxes in place with the lanes of a workgroup racing (field_hip.hip): the same bits.
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items.  Every acceptance test is a
 * float comparison that is false for NaN.
 */
#pragma once
#include "../../include/hrl_field.h"
#include "probe_core.h" /* ProbeSet, build_slot, sdist, fin_ (and through it scan_core.h: table_frame, slot_identity; render_core.h: view_frame, pix_u, pix_v) */

namespace hrl {
namespace field {

using probe::ProbeSet;
using probe::fin_;
using render::Frame;
using render::inf_;

constexpr int S_SLOTS = probe::S_SLOTS; /* 70 */
constexpr int E_ROBOT = S_SLOTS;        /* the robot's entry */
constexpr int N_ENTRIES = S_SLOTS + 1;
static_assert(N_ENTRIES <= 128, "two 64-bit lists hold the entries");
constexpr int MAX_SIZE = HRL_FIELD_MAX_SIZE, MAX_CELLS = MAX_SIZE * MAX_SIZE, MAX_PADDED = (MAX_SIZE + 2) * (MAX_SIZE + 2);
constexpr float SQRT2 = 1.41421354f;
constexpr float BLOCKED_ = -1.f; /* the value of a blocked cell in the padded image (every other value is >= 0) */
constexpr uint32_t F_BLOCKS = 1u, F_SOURCE = 2u;

struct alignas(16) FieldSet { /* 2.7 KB; on the device in LDS.  Built lane = entry, walked one entry wave-wide */
    ProbeSet S;
    float su[N_ENTRIES], sv[N_ENTRIES]; /* the entry's centre in V's coordinates */
    uint32_t flags[N_ENTRIES];          /* F_BLOCKS | F_SOURCE */
};

struct Grid { int W, H, PW; float inv_w, he, cell, half, w1, w2; };
HRL_DEV Grid grid_of(const hrl_field_spec &sp) {
    Grid g;
    g.W = sp.width; g.H = sp.height; g.PW = sp.width + 2;
    g.inv_w = 1.f / (float)sp.width; g.he = sp.half_extent;
    g.cell = (2.0f / (float)sp.width) * sp.half_extent;
    g.half = 0.5f * g.cell; g.w1 = g.cell; g.w2 = g.cell * SQRT2;
    return g;
}

/* ------------------------------------------------------------------------------------------------ frames and the table */
struct Frames { Frame V, T; float off[2]; bool robot_ok, dead; }; /* dead: an ego mode whose robot has no finite place -- every cell is blocked */
HRL_DEV Frames frames_of(const float *st, const hrl_field_spec &sp) {
    Frames f;
    hrl_view v = {};
    v.mode = sp.mode; v.centre[0] = sp.centre[0]; v.centre[1] = sp.centre[1];
    f.V = render::view_frame(v, st);
    f.T = scan::table_frame(st);
    f.robot_ok = fin_(f.T.cx) && fin_(f.T.cy);
    if (!f.robot_ok) { f.T.cx = 0.f; f.T.cy = 0.f; }
    f.off[0] = f.V.cx - f.T.cx; f.off[1] = f.V.cy - f.T.cy;
    f.dead = sp.mode != HRL_VIEW_WORLD && !f.robot_ok;
    return f;
}
/* a point of T in V's coordinates: render::to_view's operations on (x, y) - off */
HRL_DEV void table_to_view(const Frames &f, float x, float y, float *u, float *v) {
    const float dx = x - f.off[0], dy = y - f.off[1];
    *u = fma_(dx, f.V.rx, dy * f.V.ry);
    *v = fma_(dx, f.V.ux, dy * f.V.uy);
}
HRL_DEV hrl_probe_spec table_spec(const hrl_field_spec &sp) { /* what probe::build_slot keeps: every class the field looks at */
    hrl_probe_spec p = {};
    p.struct_size = sizeof p; p.n_points = 1; p.frame = HRL_PROBE_WORLD; p.classes = (sp.blocking | sp.sources) & HRL_SCAN_ALL; p.margin = sp.margin;
    return p;
}
HRL_DEV void build_entry(FieldSet &F, int e, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frames &f, const hrl_field_spec &sp) {
    uint32_t flags = 0u;
    float x = 0.f, y = 0.f; /* (the robot: the origin of T) */
    if (e < S_SLOTS) {
        probe::build_slot(F.S, e, c, st, items, aux, f.T, table_spec(sp));
        uint32_t cls;
        int32_t code;
        scan::slot_identity(e, c, aux, &cls, &code);
        const int type = probe::type_of(F.S, e);
        const bool kept = probe::kept(F.S, e), has_centre = type == render::P_RECT || type == render::P_DISC;
        flags = (kept && (sp.blocking & cls) != 0u ? F_BLOCKS : 0u) | (kept && has_centre && (sp.sources & cls) != 0u ? F_SOURCE : 0u);
        x = F.S.p[0][e]; y = F.S.p[1][e];
    } else {
        flags = (sp.sources & HRL_FIELD_ROBOT) != 0u && f.robot_ok ? F_SOURCE : 0u;
    }
    table_to_view(f, x, y, &F.su[e], &F.sv[e]);
    F.flags[e] = flags;
}

/* ------------------------------------------------------------------------------------------------ cells */
HRL_DEV int padded(const Grid &g, int i, int j) { return (i + 1) * g.PW + (j + 1); }
HRL_DEV void cell_centre(const Grid &g, const Frames &f, int i, int j, float *u, float *v, float *qx, float *qy) {
    *u = render::pix_u(j, g.W, g.inv_w, g.he);
    *v = render::pix_v(i, g.H, g.inv_w, g.he);
    *qx = f.off[0] + fma_(*u, f.V.rx, *v * f.V.ux);
    *qy = f.off[1] + fma_(*u, f.V.ry, *v * f.V.uy);
}
/* b0 / b1, s0 / s1: bit i set = entry i / 64 + i blocks / is a source */
HRL_DEV float cell_init(const FieldSet &F, unsigned long long b0, unsigned long long b1, unsigned long long s0, unsigned long long s1, const Grid &g, const Frames &f,
                        float margin, int i, int j) {
    float u, v, qx, qy;
    cell_centre(g, f, i, j, &u, &v, &qx, &qy);
    bool source = false;
    for (unsigned long long m = s0; m; m &= m - 1) {
        const int e = __builtin_ctzll(m);
        source = source || (fabsf(u - F.su[e]) <= g.half && fabsf(v - F.sv[e]) <= g.half);
    }
    for (unsigned long long m = s1; m; m &= m - 1) {
        const int e = 64 + __builtin_ctzll(m);
        source = source || (fabsf(u - F.su[e]) <= g.half && fabsf(v - F.sv[e]) <= g.half);
    }
    bool free = !f.dead && fin_(qx) && fin_(qy);
    for (unsigned long long m = b0; m; m &= m - 1) free = probe::sdist(F.S, __builtin_ctzll(m), qx, qy) >= margin && free;
    for (unsigned long long m = b1; m; m &= m - 1) free = probe::sdist(F.S, 64 + __builtin_ctzll(m), qx, qy) >= margin && free;
    return source ? 0.f : (free ? inf_() : BLOCKED_);
}
/* direction k = E, NE, N, NW, W, SW, S, SE: columns and rows it moves by, and its offset in the padded image */
HRL_DEV int dcol(int k) { return (k == 0 || k == 1 || k == 7) ? 1 : ((k >= 3 && k <= 5) ? -1 : 0); }
HRL_DEV int drow(int k) { return (k >= 1 && k <= 3) ? -1 : (k >= 5 ? 1 : 0); }
HRL_DEV int step_of(int k, int PW) { return drow(k) * PW + dcol(k); }
HRL_DEV uint32_t cell_adm(const float *img, int p, int PW) {
    uint32_t open = 0u, a = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) open |= img[p + step_of(k, PW)] >= 0.f ? 1u << k : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t need = (k & 1) ? ((1u << k) | (1u << (k - 1)) | (1u << ((k + 1) & 7))) : (1u << k);
        a |= (open & need) == need ? 1u << k : 0u;
    }
    return img[p] > 0.f ? a : 0u; /* (a source, 0, and a blocked cell, -1, are fixed) */
}
HRL_DEV float cell_relax(const float *img, int p, int PW, uint32_t a, float w1, float w2) {
    float best = img[p];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float cand = img[p + step_of(k, PW)] + ((k & 1) ? w2 : w1);
        best = ((a >> k) & 1u) != 0u && cand < best ? cand : best;
    }
    return best;
}
HRL_DEV uint32_t cell_parent(const float *img, int p, int PW, uint32_t a, float w1, float w2) {
    const float d = img[p];
    uint32_t par = HRL_FIELD_UNREACHED;
#pragma unroll
    for (int k = 7; k >= 0; --k) { /* (downwards: the lowest k stays) */
        const float cand = img[p + step_of(k, PW)] + ((k & 1) ? w2 : w1);
        par = ((a >> k) & 1u) != 0u && cand == d && d <= 3.0e38f ? (uint32_t)k : par;
    }
    return d < 0.f ? (uint32_t)HRL_FIELD_BLOCKED : (d == 0.f ? (uint32_t)HRL_FIELD_SOURCE : par);
}
HRL_DEV float cell_dist(const float *img, int p) { return img[p] < 0.f ? inf_() : img[p]; }

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_field_spec *s) {
    if (!s) return "null field spec";
    if (s->struct_size != sizeof(hrl_field_spec)) return "hrl_field_spec.struct_size is not sizeof(hrl_field_spec): initialise the record with hrl_field_default_spec()";
    if (s->width < HRL_FIELD_MIN_SIZE || s->width > HRL_FIELD_MAX_SIZE || s->width % 8 != 0) return "field width must be a multiple of 8 within 8..64";
    if (s->height < HRL_FIELD_MIN_SIZE || s->height > HRL_FIELD_MAX_SIZE || s->height % 8 != 0) return "field height must be a multiple of 8 within 8..64";
    if (s->mode != HRL_VIEW_WORLD && s->mode != HRL_VIEW_EGO && s->mode != HRL_VIEW_EGO_HEADING) return "unknown field mode";
    if (!(s->half_extent > HRL_FIELD_MIN_HALF_EXTENT) || !(s->half_extent <= HRL_FIELD_MAX_HALF_EXTENT)) return "field half_extent must be finite and within (1e-3, 1e4]";
    if (s->blocking == 0u || (s->blocking & ~HRL_SCAN_ALL) != 0u) return "field blocking must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET";
    if (s->sources == 0u || (s->sources & ~(HRL_FIELD_ROBOT | HRL_SCAN_FOOD | HRL_SCAN_POISON | HRL_SCAN_TARGET)) != 0u)
        return "field sources must be a non-empty mask of HRL_FIELD_ROBOT | HRL_SCAN_FOOD | POISON | TARGET (a wall or the box is no source)";
    if (!(s->margin >= 0.f) || !(s->margin <= HRL_PROBE_MAX_MARGIN)) return "field margin must be finite and within 0..2";
    return "";
}
inline std::string validate_out(const hrl_field_out *o) {
    if (!o) return "null field out";
    if (!o->dist && !o->parent) return "field out holds no pointer: at least one output must be given";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t mode, hrl_field_spec *s) {
    hrl_view v;
    if (!s || render::default_view(c, mode, &v) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    DevCfg dc;
    build_devcfg(*c, dc);
    s->struct_size = sizeof(*s); s->width = v.width; s->height = v.height; s->mode = mode;
    s->centre[0] = v.centre[0]; s->centre[1] = v.centre[1]; s->half_extent = v.half_extent;
    s->blocking = HRL_SCAN_WALL | HRL_SCAN_BOX | HRL_SCAN_POISON;
    s->margin = c->env_kind == HRL_POINT_GATHER ? render::POINT_HALF : dc.r_torso;
    switch (c->env_kind) {
        case HRL_ANT_GATHER: case HRL_POINT_GATHER: s->sources = HRL_SCAN_FOOD; break;
        case HRL_ANT_MAZE: case HRL_ANT_MAZE_MJ: case HRL_ANT_FLAGRUN: s->sources = HRL_SCAN_TARGET; break;
        default: s->sources = HRL_FIELD_ROBOT;
    }
    return HRL_OK;
}

#ifdef HRL_EMU
constexpr int SCHED_JACOBI = 0, SCHED_FORWARD = 1, SCHED_REVERSE = 2; /* rounds over two images | in-place sweeps in raster order | in reverse raster order */

/* One env on the host.  Returns the number of rounds (sweeps) it ran, the one that changed nothing included. */
inline int field_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_field_spec &sp, int schedule, const hrl_field_out &out, size_t at) {
    static thread_local FieldSet F;
    static thread_local float img[2][MAX_PADDED];
    static thread_local uint8_t adm[MAX_PADDED];
    const Grid g = grid_of(sp);
    const Frames f = frames_of(st, sp);
    for (int e = 0; e < N_ENTRIES; ++e) build_entry(F, e, c, st, items, aux, f, sp);
    unsigned long long b0 = 0, b1 = 0, s0 = 0, s1 = 0;
    for (int e = 0; e < N_ENTRIES; ++e) {
        if (F.flags[e] & F_BLOCKS) (e < 64 ? b0 : b1) |= 1ull << (e & 63);
        if (F.flags[e] & F_SOURCE) (e < 64 ? s0 : s1) |= 1ull << (e & 63);
    }
    const int n_padded = g.PW * (g.H + 2);
    for (int p = 0; p < n_padded; ++p) { img[0][p] = BLOCKED_; adm[p] = 0; }
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) img[0][padded(g, i, j)] = cell_init(F, b0, b1, s0, s1, g, f, sp.margin, i, j);
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) adm[padded(g, i, j)] = (uint8_t)cell_adm(img[0], padded(g, i, j), g.PW);
    memcpy(img[1], img[0], sizeof(float) * (size_t)n_padded);
    int cur = 0, rounds = 0;
    const int cap = g.W * g.H;
    for (int r = 0; r < cap; ++r) {
        bool changed = false;
        ++rounds;
        if (schedule == SCHED_JACOBI) {
            for (int p = 0; p < n_padded; ++p)
                if (adm[p]) {
                    const float old = img[cur][p], d = cell_relax(img[cur], p, g.PW, adm[p], g.w1, g.w2);
                    img[cur ^ 1][p] = d; changed = changed || d != old;
                }
            cur ^= 1;
        } else {
            for (int q = 0; q < n_padded; ++q) {
                const int p = schedule == SCHED_FORWARD ? q : n_padded - 1 - q;
                if (adm[p]) {
                    const float old = img[cur][p], d = cell_relax(img[cur], p, g.PW, adm[p], g.w1, g.w2);
                    img[cur][p] = d; changed = changed || d != old;
                }
            }
        }
        if (!changed) break;
    }
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) {
            const int p = padded(g, i, j);
            const size_t k = at + (size_t)(i * g.W + j);
            if (out.dist) out.dist[k] = cell_dist(img[cur], p);
            if (out.parent) out.parent[k] = (uint8_t)cell_parent(img[cur], p, g.PW, adm[p], g.w1, g.w2);
        }
    return rounds;
}
/* hrl_field on host pointers; returns the status and leaves the reason in `why`; rounds (may be null): [num_envs], the rounds each env ran */
inline int field_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_field_spec *sp, const uint8_t *mask, const hrl_field_out *out, int schedule, int32_t *rounds,
                            std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (why.empty() && (schedule < SCHED_JACOBI || schedule > SCHED_REVERSE)) why = "unknown schedule";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    const size_t cells = (size_t)sp->width * (size_t)sp->height;
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        const int r = field_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp,
                                     schedule, *out, (size_t)e * cells);
        if (rounds) rounds[e] = r;
    }
    return HRL_OK;
}
#endif

}  // namespace field
}  // namespace hrl
