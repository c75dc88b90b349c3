/*
 * probe_core.h -- specification of the batched point probes (include/hrl_probe.h), written once as plain C++: the device kernel
 * (probe_hip.hip) and the host build of the tests (tests/probe_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The probes of one env are a pure function of (DevCfg, its state / items / aux record, hrl_probe_spec, its points):
 *
 *   build_slot    slot s < S_SLOTS of the table: the renderer's primitive of that slot (render_core.h: make_prim, as scan_core.h reads
 *                 it) in the scanner's frame -- centred on the robot, WORLD axes -- with its code and the verdict `kept`: its class bit
 *                 is on and its parameters are finite.  A PLANE STAYS WHERE DevCfg HAS IT, the face the robot collides with and the
 *                 renderer paints: the probe answers what the robot can touch.  (scan_core.h makes the opposite choice and moves a
 *                 plane out by WALL_HALF to the wall's centre line, where the reference's sense_walls meets it.)
 *   build_start   the robot's end of `path`, snapped into free space, and the blocking rectangle (the box grown by margin)
 *   node_init /   corner node k, whether it counts, and the shortest length g[k] from the snapped start to it: the direct segment, then
 *   node_round    three Jacobi rounds over the four nodes (a route has at most four corners); first[k] = the first corner of that route
 *   to_robot      a query point in the table's frame
 *   point_*       the three answers of one point: walk the bit list of the kept slots in slot order for clearance and for sight (the
 *                 smallest value wins, equal values stay with the lower slot), and the four nodes for path
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state, the items or the points.  Every acceptance
 * test is a float comparison that is false for NaN; a robot or a point that is not finite gets the answers of `blank`.
 */
#pragma once
#include "../../include/hrl_probe.h"
#include "scan_core.h" /* forward, slot_identity, isect_* (and through it render_core.h: Frame, Prim, make_prim; step_core.h: fma_, DevCfg) */

namespace hrl {
namespace probe {

using render::Frame;
using render::Prim;
using render::inf_;
using render::max_;
using render::min_;

constexpr int S_SLOTS = scan::S_SLOTS; /* 70: planes 0..3, the box, the target, 64 items */
constexpr int MAX_POINTS = HRL_PROBE_MAX_POINTS;
constexpr float SKIN = HRL_PROBE_SKIN;

HRL_DEV bool fin_(float x) { return fabsf(x) <= 3.0e38f; } /* (false for NaN) */

struct alignas(16) ProbeSet { /* 1.8 KB; on the device in LDS.  Structure of arrays: built lane = slot, walked one slot wave-wide */
    float p[4][S_SLOTS];     /* P_HALF: nx, ny, offset (inside where nx x + ny y + offset >= 0) | P_RECT: centre x, y, half sizes | P_DISC: centre, r^2 */
    uint32_t meta[S_SLOTS];  /* type | kept << 8 */
    int32_t code[S_SLOTS];   /* what `nearest` / `blocker` report for this slot */
    float fwd[2], org[2];    /* forward; the robot's world (x, y) */
    float start[2], d0;      /* the snapped start in the table's frame and the length of the moves that took it there */
    float bc[2], bh[2];      /* the blocking rectangle: centre, half sizes */
    float node[4][2], g[4];  /* corner nodes; g = +inf for a node that does not count or cannot be reached */
    int32_t first[4];
    int32_t has_box, robot_ok;
};

struct Answer { float clearance, sight, path; int32_t nearest, blocker, via; };
HRL_DEV void blank(Answer &a) { a.clearance = inf_(); a.nearest = 0; a.sight = 0.f; a.blocker = 0; a.path = inf_(); a.via = HRL_VIA_NONE; }

/* ------------------------------------------------------------------------------------------------ the table */
HRL_DEV void build_slot(ProbeSet &S, int slot, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frame &f, const hrl_probe_spec &sp) {
    Prim P;
    render::make_prim(P, slot, c, st, items, aux, f); /* (a plane as it is: see the head of this file) */
    uint32_t cls;
    int32_t code;
    scan::slot_identity(slot, c, aux, &cls, &code);
    const bool kept = (sp.classes & cls) != 0u && P.type != render::P_NONE && fin_(P.p[0]) && fin_(P.p[1]) && fin_(P.p[2]) && fin_(P.p[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) S.p[k][slot] = P.p[k];
    S.meta[slot] = (uint32_t)P.type | (kept ? 256u : 0u);
    S.code[slot] = code;
}
HRL_DEV bool kept(const ProbeSet &S, int slot) { return (S.meta[slot] & 256u) != 0u; }
HRL_DEV int type_of(const ProbeSet &S, int slot) { return (int)(S.meta[slot] & 255u); }
HRL_DEV void build_frame(ProbeSet &S, const float *st, const hrl_probe_spec &sp) {
    scan::forward(sp.frame == HRL_PROBE_HEADING ? HRL_SCAN_HEADING : HRL_SCAN_WORLD, st, &S.fwd[0], &S.fwd[1]);
    S.org[0] = st[HRL_QPOS_OFF]; S.org[1] = st[HRL_QPOS_OFF + 1];
    S.robot_ok = fin_(S.org[0]) && fin_(S.org[1]);
}

/* ------------------------------------------------------------------------------------------------ path: planes, the blocking rectangle, nodes */
HRL_DEV float plane_val(const ProbeSet &S, int k, float x, float y) { return fma_(S.p[0][k], x, fma_(S.p[1][k], y, S.p[2][k])); }
/* every lateral plane the env has leaves `margin` of room at (x, y) (false for NaN) */
HRL_DEV bool in_arena(const ProbeSet &S, float x, float y, float margin) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < render::R_BOX; ++k) ok = ok && (type_of(S, k) != render::P_HALF || plane_val(S, k, x, y) >= margin);
    return ok;
}
HRL_DEV bool in_block(const ProbeSet &S, float x, float y) { return S.has_box && fabsf(x - S.bc[0]) < S.bh[0] && fabsf(y - S.bc[1]) < S.bh[1]; }
HRL_DEV float dist_(float ax, float ay, float bx, float by) {
    const float dx = bx - ax, dy = by - ay;
    return sqrtf(fma_(dx, dx, dy * dy));
}
/* one axis of the blocked test: the interval of the segment's parameter in which a + t d is strictly within c +- h (c relative to a).
 * A component whose reciprocal is not finite runs parallel to the slab. */
HRL_DEV void slab_open(float c, float h, float d, float *lo, float *hi) {
    const float id = 1.f / d;
    if (fabsf(id) <= 3.0e38f) {
        const float a = (c - h) * id, b = (c + h) * id;
        *lo = min_(a, b); *hi = max_(a, b);
    } else {
        const bool in = fabsf(c) < h;
        *lo = in ? -inf_() : inf_(); *hi = in ? inf_() : -inf_();
    }
}
/* the segment a b overlaps the interior of the blocking rectangle over a stretch of positive length */
HRL_DEV bool blocked(const ProbeSet &S, float ax, float ay, float bx, float by) {
    float lox, hix, loy, hiy;
    slab_open(S.bc[0] - ax, S.bh[0], bx - ax, &lox, &hix);
    slab_open(S.bc[1] - ay, S.bh[1], by - ay, &loy, &hiy);
    const float tn = max_(max_(lox, loy), 0.f), tf = min_(min_(hix, hiy), 1.f);
    return S.has_box && lox <= hix && loy <= hiy && tn < tf;
}
/* start, d0, has_box, bc, bh: the same values on whichever lane computes them */
HRL_DEV void build_start(ProbeSet &S, float margin) {
    float sx = 0.f, sy = 0.f, d0 = 0.f;
#pragma unroll
    for (int k = 0; k < render::R_BOX; ++k) {
        const float def = margin - plane_val(S, k, sx, sy);
        if (type_of(S, k) == render::P_HALF && def > 0.f) { sx = fma_(S.p[0][k], def, sx); sy = fma_(S.p[1][k], def, sy); d0 += def; }
    }
    const bool has_box = type_of(S, render::R_BOX) == render::P_RECT;
    const float cx = S.p[0][render::R_BOX], cy = S.p[1][render::R_BOX];
    const float hx = S.p[2][render::R_BOX] + margin, hy = S.p[3][render::R_BOX] + margin;
    if (has_box && fabsf(sx - cx) < hx && fabsf(sy - cy) < hy) { /* out through the nearest side, to the nodes' rectangle */
        const float x1 = cx + (hx + SKIN), x0 = cx - (hx + SKIN), y1 = cy + (hy + SKIN), y0 = cy - (hy + SKIN);
        const float m0 = x1 - sx, m1 = sx - x0, m2 = y1 - sy, m3 = sy - y0;
        float m = m0;
        int side = 0;
        if (m1 < m) { m = m1; side = 1; }
        if (m2 < m) { m = m2; side = 2; }
        if (m3 < m) { m = m3; side = 3; }
        sx = side == 0 ? x1 : (side == 1 ? x0 : sx);
        sy = side == 2 ? y1 : (side == 3 ? y0 : sy);
        d0 += m;
    }
    S.start[0] = sx; S.start[1] = sy; S.d0 = d0;
    S.has_box = has_box; S.bc[0] = cx; S.bc[1] = cy; S.bh[0] = hx; S.bh[1] = hy;
}
/* corner k = (+x, +y), (-x, +y), (-x, -y), (+x, -y) of the blocking rectangle grown by SKIN */
HRL_DEV void node_pos(const ProbeSet &S, int k, float *x, float *y) {
    const float sx = (k == 0 || k == 3) ? 1.f : -1.f, sy = k < 2 ? 1.f : -1.f;
    *x = fma_(sx, S.bh[0] + SKIN, S.bc[0]); *y = fma_(sy, S.bh[1] + SKIN, S.bc[1]);
}
/* g of node k by the direct segment: +inf when the node does not count or the segment is blocked.  Needs build_start. */
HRL_DEV float node_init(const ProbeSet &S, int k, float margin) {
    float x, y;
    node_pos(S, k, &x, &y);
    const bool ok = S.has_box && in_arena(S, x, y, margin) && !blocked(S, S.start[0], S.start[1], x, y);
    return ok ? dist_(S.start[0], S.start[1], x, y) : inf_();
}
/* one Jacobi round for node k from the values of the round before: through node j = 0, 1, 2, 3 in turn, a shorter route wins */
HRL_DEV void node_round(const ProbeSet &S, int k, float margin, const float *g_old, const int32_t *first_old, float *g, int32_t *first) {
    float x, y;
    node_pos(S, k, &x, &y);
    const bool counts = S.has_box && in_arena(S, x, y, margin);
    float best = g_old[k];
    int32_t f = first_old[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float u, v;
        node_pos(S, j, &u, &v);
        const float cand = g_old[j] + dist_(u, v, x, y);
        if (j != k && counts && cand < best && !blocked(S, u, v, x, y)) { best = cand; f = first_old[j]; }
    }
    *g = best; *first = f;
}

/* ------------------------------------------------------------------------------------------------ one point */
/* the point as given -> the table's frame */
HRL_DEV void to_robot(const ProbeSet &S, int frame, float px, float py, float *qx, float *qy) {
    if (frame == HRL_PROBE_WORLD) { *qx = px - S.org[0]; *qy = py - S.org[1]; }
    else if (frame == HRL_PROBE_HEADING) { *qx = fma_(S.fwd[0], px, -(S.fwd[1] * py)); *qy = fma_(S.fwd[1], px, S.fwd[0] * py); }
    else { *qx = px; *qy = py; }
}
HRL_DEV float sdist(const ProbeSet &S, int slot, float qx, float qy) {
    const int type = type_of(S, slot);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    float d = inf_();
    if (type == render::P_HALF) d = fma_(p0, qx, fma_(p1, qy, p2));
    else if (type == render::P_RECT) {
        const float ax = fabsf(qx - p0) - p2, ay = fabsf(qy - p1) - p3;
        const float ox = max_(ax, 0.f), oy = max_(ay, 0.f);
        d = sqrtf(fma_(ox, ox, oy * oy)) + min_(max_(ax, ay), 0.f);
    } else if (type == render::P_DISC) {
        const float dx = qx - p0, dy = qy - p1;
        d = sqrtf(fma_(dx, dx, dy * dy)) - sqrtf(p2);
    }
    return d;
}
struct Seg { float dx, dy, idx, idy, len; };
HRL_DEV float meet(const ProbeSet &S, int slot, const Seg &r) {
    const int type = type_of(S, slot);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    float t = inf_();
    if (type == render::P_HALF) t = scan::isect_half(p0, p1, p2, r.dx, r.dy);
    else if (type == render::P_RECT) t = scan::isect_rect(p0, p1, p2, p3, r.idx, r.idy);
    else if (type == render::P_DISC) t = scan::isect_disc(p0, p1, p2, r.dx, r.dy);
    return t;
}
/* length and unit direction of (0, 0) -> q; where the squared length leaves fp32's comfortable range, through a power of two */
HRL_DEV void segment(float qx, float qy, Seg &r) {
    const float l2 = fma_(qx, qx, qy * qy);
    float inv;
    if (l2 >= 1e-30f && l2 <= 3.0e38f) {
        r.len = sqrtf(l2); inv = 1.f / r.len;
    } else {
        const float up = l2 < 1.f ? 18446744073709551616.f : 5.42101086242752217e-20f, down = l2 < 1.f ? 5.42101086242752217e-20f : 18446744073709551616.f; /* 2^64, 2^-64 */
        qx *= up; qy *= up;
        const float ls = sqrtf(fma_(qx, qx, qy * qy));
        r.len = ls * down; inv = 1.f / ls;
    }
    r.dx = qx * inv; r.dy = qy * inv;
    r.idx = 1.f / r.dx; r.idy = 1.f / r.dy;
}

/* The point in the table's frame, and whether it gets answers at all (else those of `blank`). */
HRL_DEV bool locate(const ProbeSet &S, int frame, float px, float py, float *qx, float *qy) {
    to_robot(S, frame, px, py, qx, qy);
    return S.robot_ok && fin_(px) && fin_(py) && fin_(*qx) && fin_(*qy);
}
/* m0 / m1: bit i set = slot i / 64 + i is kept */
HRL_DEV void point_clearance(const ProbeSet &S, unsigned long long m0, unsigned long long m1, float qx, float qy, float *clearance, int32_t *nearest) {
    float best = inf_();
    int32_t who = 0;
    for (unsigned long long m = m0; m; m &= m - 1) {
        const int s = __builtin_ctzll(m);
        const float d = sdist(S, s, qx, qy);
        if (d < best) { best = d; who = S.code[s]; }
    }
    for (unsigned long long m = m1; m; m &= m - 1) {
        const int s = 64 + __builtin_ctzll(m);
        const float d = sdist(S, s, qx, qy);
        if (d < best) { best = d; who = S.code[s]; }
    }
    *clearance = best; *nearest = who;
}
HRL_DEV void point_sight(const ProbeSet &S, unsigned long long m0, unsigned long long m1, float qx, float qy, float *sight, int32_t *blocker) {
    Seg r;
    segment(qx, qy, r);
    float best = inf_();
    int32_t who = 0;
    if (r.len > 0.f) { /* (a point at the robot's own place: nothing lies before the segment's end) */
        for (unsigned long long m = m0; m; m &= m - 1) {
            const int s = __builtin_ctzll(m);
            const float t = meet(S, s, r);
            if (t < r.len && t < best) { best = t; who = S.code[s]; }
        }
        for (unsigned long long m = m1; m; m &= m - 1) {
            const int s = 64 + __builtin_ctzll(m);
            const float t = meet(S, s, r);
            if (t < r.len && t < best) { best = t; who = S.code[s]; }
        }
    }
    *sight = who != 0 ? best : (r.len > 0.f ? r.len : 0.f);
    *blocker = who;
}
HRL_DEV void point_path(const ProbeSet &S, float margin, float qx, float qy, float *path, int32_t *via_out) {
    float best = inf_();
    int32_t via = HRL_VIA_NONE;
    if (in_arena(S, qx, qy, margin) && !in_block(S, qx, qy)) {
        const float direct = dist_(S.start[0], S.start[1], qx, qy);
        if (direct <= 3.0e38f && !blocked(S, S.start[0], S.start[1], qx, qy)) { best = direct; via = HRL_VIA_STRAIGHT; } /* (a length fp32 cannot hold is no way) */
#pragma nounroll /* (unrolled, the compiler hoists each node's loop-invariant tests into scalar register pairs and runs out of them) */
        for (int k = 0; k < 4; ++k) {
            const float x = S.node[k][0], y = S.node[k][1];
            const float cand = S.g[k] + dist_(x, y, qx, qy);
            if (cand < best && !blocked(S, x, y, qx, qy)) { best = cand; via = HRL_VIA_CORNER0 + S.first[k]; }
        }
    }
    *path = via != HRL_VIA_NONE ? S.d0 + best : inf_();
    *via_out = via;
}
/* bit i set = output i (clearance, nearest, sight, blocker, path, via) is asked for: one integer instead of six pointer tests per point */
constexpr unsigned W_CLEARANCE = 1u, W_NEAREST = 2u, W_SIGHT = 4u, W_BLOCKER = 8u, W_PATH = 16u, W_VIA = 32u;
HRL_DEV unsigned wanted(const hrl_probe_out &o) {
    return (o.clearance ? W_CLEARANCE : 0u) | (o.nearest ? W_NEAREST : 0u) | (o.sight ? W_SIGHT : 0u) | (o.blocker ? W_BLOCKER : 0u) | (o.path ? W_PATH : 0u) | (o.via ? W_VIA : 0u);
}
/* The answers of the point (px, py) of the env, one 4-byte value per requested output, each pair stored as soon as it is known. */
HRL_DEV void probe_point(const ProbeSet &S, unsigned long long m0, unsigned long long m1, const hrl_probe_spec &sp, float px, float py, const hrl_probe_out &o, unsigned w, size_t at) {
    float qx, qy;
    const bool ok = locate(S, sp.frame, px, py, &qx, &qy);
    Answer a;
    blank(a);
    if (w & (W_CLEARANCE | W_NEAREST)) {
        if (ok) point_clearance(S, m0, m1, qx, qy, &a.clearance, &a.nearest);
        if (w & W_CLEARANCE) o.clearance[at] = a.clearance;
        if (w & W_NEAREST) o.nearest[at] = a.nearest;
    }
    if (w & (W_SIGHT | W_BLOCKER)) {
        if (ok) point_sight(S, m0, m1, qx, qy, &a.sight, &a.blocker);
        if (w & W_SIGHT) o.sight[at] = a.sight;
        if (w & W_BLOCKER) o.blocker[at] = a.blocker;
    }
    if (w & (W_PATH | W_VIA)) {
        if (ok) point_path(S, sp.margin, qx, qy, &a.path, &a.via);
        if (w & W_PATH) o.path[at] = a.path;
        if (w & W_VIA) o.via[at] = a.via;
    }
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_probe_spec *s) {
    if (!s) return "null probe spec";
    if (s->struct_size != sizeof(hrl_probe_spec)) return "hrl_probe_spec.struct_size is not sizeof(hrl_probe_spec): initialise the record with hrl_probe_default_spec()";
    if (s->n_points < 1 || s->n_points > MAX_POINTS) return "probe n_points must be within 1..512";
    if (s->frame != HRL_PROBE_WORLD && s->frame != HRL_PROBE_EGO && s->frame != HRL_PROBE_HEADING) return "unknown probe frame";
    if (s->classes == 0u || (s->classes & ~HRL_SCAN_ALL) != 0u) return "probe classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET";
    if (!(s->margin >= 0.f) || !(s->margin <= HRL_PROBE_MAX_MARGIN)) return "probe margin must be finite and within 0..2";
    return "";
}
inline std::string validate_out(const hrl_probe_out *o) {
    if (!o) return "null probe out";
    if (!o->clearance && !o->nearest && !o->sight && !o->blocker && !o->path && !o->via) return "probe out holds no pointer: at least one output must be given";
    return "";
}

/* 64 points, all classes, margin = the radius of the torso (the half side of the point bot's cube) */
inline int default_spec(const hrl_config *c, int32_t frame, hrl_probe_spec *s) {
    if (!c || !s || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN) return HRL_ERR_BAD_ARG;
    if (frame != HRL_PROBE_WORLD && frame != HRL_PROBE_EGO && frame != HRL_PROBE_HEADING) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    DevCfg dc;
    build_devcfg(*c, dc);
    s->struct_size = sizeof(*s); s->n_points = 64; s->frame = frame; s->classes = HRL_SCAN_ALL;
    s->margin = c->env_kind == HRL_POINT_GATHER ? render::POINT_HALF : dc.r_torso;
    return HRL_OK;
}

#ifdef HRL_EMU
/* The whole launch on the host, partitioned as the kernel partitions it: per env the table, its list, the start and the nodes (lane k
 * of a round reads the values of the round before), then runs of 64 points. */
inline void probe_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_probe_spec &sp, const float *points, const hrl_probe_out &out,
                           size_t at) {
    ProbeSet S;
    const Frame f = scan::table_frame(st);
    build_frame(S, st, sp);
    for (int slot = 0; slot < S_SLOTS; ++slot) build_slot(S, slot, c, st, items, aux, f, sp);
    unsigned long long m0 = 0, m1 = 0;
    for (int slot = 0; slot < 64; ++slot) if (kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (kept(S, slot)) m1 |= 1ull << (slot - 64);
    const unsigned w = wanted(out);
    build_start(S, sp.margin);
    float g[4];
    int32_t first[4];
    for (int k = 0; k < 4; ++k) { g[k] = node_init(S, k, sp.margin); first[k] = k; }
    for (int round = 0; round < 3; ++round) {
        float g2[4];
        int32_t first2[4];
        for (int k = 0; k < 4; ++k) node_round(S, k, sp.margin, g, first, &g2[k], &first2[k]);
        for (int k = 0; k < 4; ++k) { g[k] = g2[k]; first[k] = first2[k]; }
    }
    for (int k = 0; k < 4; ++k) { node_pos(S, k, &S.node[k][0], &S.node[k][1]); S.g[k] = g[k]; S.first[k] = first[k]; }
    for (int base = 0; base < sp.n_points; base += 64)
        for (int k = base; k < base + 64 && k < sp.n_points; ++k) probe_point(S, m0, m1, sp, points[2 * k], points[2 * k + 1], out, w, at + (size_t)k);
}
/* hrl_probe on host pointers; returns the status and leaves the reason in `why` */
inline int probe_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_probe_spec *sp, const float *points, const uint8_t *mask, const hrl_probe_out *out,
                            std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (why.empty() && !points) why = "null points";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        probe_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp,
                       points + (size_t)e * sp->n_points * 2, *out, (size_t)e * sp->n_points);
    }
    return HRL_OK;
}
#endif

}  // namespace probe
}  // namespace hrl
