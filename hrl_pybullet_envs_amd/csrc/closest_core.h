/*
 * closest_core.h -- specification of the batched closest points (include/hrl_closest.h), written once as plain C++: the device kernel
 * (closest_hip.hip) and the host build of the tests (tests/closest_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The cells of one env are a pure function of (DevCfg, the env's state / items record, hrl_closest_spec):
 *
 *   build_link   the ends p0, p1 of a link relative to O by links::link_world (the step's kinematics, bit for bit), and whether they and
 *                O are finite; the point bot: the cube's axes X, Y, Z by quat_axes as the step's point_substep keeps them
 *   build_surf   surface s of the env's table of S_SCENE = 70: the ground, planes 0..3, the maze box, item cubes 0..63 -- WHAT THE STEP
 *                COLLIDES WITH: DevCfg's plane_n / plane_d, box_lo / box_hi, and the cubes of ITEM_HALF at ITEM_Z about the items'
 *                positions (the scanner's item set: the gather kinds, i < n_food + n_poison); its class, its index and whether it is
 *                asked for and there
 *   pair         the candidate (link, surface s) or, s >= S_LINK0, (link, other link s - S_LINK0): distance, the two points and the
 *                normal.  The step's narrow phase, restated or called:
 *                  link_plane   sphere_vs_surface's plane arm at both ends (the deepest point of a capsule against a plane is an end)
 *                  link_box     sphere_vs_surface's box arm: step_core.h's seg_box_t and sphere_vs_box, CALLED (they need no WaveLds),
 *                               on pw = q + c0 and d = p1 - p0 as the step forms them
 *                  link_link    capsule_pair's closest points RESTATED EXPRESSION FOR EXPRESSION (that function reads the step's
 *                               WaveLds), in the step's order: the capsule of the lower leg is the first
 *                  cube_plane / cube_box   point_substep's corner tests (step_core.h: `corner` and the cubes' own corners against the
 *                               player's oriented box), restated
 *   key_of       (distance, index) as one 64-bit word whose unsigned order is the order of the distance, then of the index: the least key
 *                of a cell is its winner whatever the order of evaluation
 *   answer       the winner of a cell evaluated once more, now for its points and its normal
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items, except sincos_spec's guarded
 * quadrant (link_world).  `counts` is the one acceptance: -1e30 < d < 1e30, false for NaN.  A link that is not `ok` is a candidate for
 * nothing.
 */
#pragma once
#include "../../include/hrl_closest.h"
#include "links_core.h" /* link_world, pick (and host_cfg.h, step_core.h: seg_box_t, sphere_vs_box, ITEM_HALF, ITEM_Z, DevCfg) */

namespace hrl {
namespace closest {

using links::pick;

constexpr int LINKS = HRL_LINKS_ANT, LINK_PAD = 16, CLASSES = HRL_CLOSEST_CLASSES, CELLS = LINKS * CLASSES;
constexpr int S_GROUND = 0, S_PLANE0 = 1, S_BOX = 5, S_ITEM0 = 6, S_SCENE = S_ITEM0 + HRL_MAX_ITEMS, S_LINK0 = S_SCENE, S_ALL = S_LINK0 + LINKS, S_PAD = 72;
constexpr float CUBE_HALF = 0.35f; /* the half side of the point bot's cube: `he` of point_substep (assets/player_cube.xml:8) */
constexpr unsigned long long KEY_NONE = ~0ull;
static_assert(S_SCENE == 70 && S_SCENE <= S_PAD && S_ALL == 83, "the ground, four planes, the box, 64 items; then the links");

HRL_DEV float inf_() { return __builtin_inff(); }
HRL_DEV bool fin_(float v) { return fabsf(v) <= 3.0e38f; } /* (false for NaN) */
HRL_DEV bool counts(float d) { return d > -1e30f && d < 1e30f; } /* (false for NaN; 1e30: sphere_vs_box's word for a non-finite centre) */

/* ------------------------------------------------------------------------------------------------ the env's tables */
/* The links, structure of arrays.  Ants: rows 0..2 p0, 3..5 p1, relative to O.  The point bot (link 0): rows 0..2 X, 3..5 Y, 6..8 Z. */
struct alignas(16) LinkSet {
    float v[9][LINK_PAD];
    uint32_t ok[LINK_PAD];
};
HRL_DEV void build_link(LinkSet &L, int link, const DevCfg &c, const float *st) {
    bool fin = fin_(st[HRL_QPOS_OFF]) && fin_(st[HRL_QPOS_OFF + 1]) && fin_(st[HRL_QPOS_OFF + 2]);
    if (c.kind == HRL_POINT_GATHER) {
        float X[3], Y[3], Z[3];
        quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            L.v[k][link] = X[k]; L.v[3 + k][link] = Y[k]; L.v[6 + k][link] = Z[k];
            fin = fin && fin_(X[k]) && fin_(Y[k]) && fin_(Z[k]);
        }
    } else {
        links::Link K;
        links::link_world(c, st, link, K);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            L.v[k][link] = K.p0[k]; L.v[3 + k][link] = K.p1[k]; L.v[6 + k][link] = 0.f;
            fin = fin && fin_(K.p0[k]) && fin_(K.p1[k]);
        }
    }
    L.ok[link] = fin ? 1u : 0u;
}

/* The scene, structure of arrays.  A plane: rows 0..2 the normal, 3 the offset d.  A box: rows 0..2 lo, 3..5 hi.
 * meta: class | live << 8 | index << 16. */
struct alignas(16) SurfSet {
    float v[6][S_PAD];
    uint32_t meta[S_PAD];
};
HRL_DEV uint32_t class_bit(int cls) {
    return cls == HRL_CLOSEST_GROUND ? HRL_CAMERA_GROUND
         : cls == HRL_CLOSEST_WALL   ? HRL_SCAN_WALL
         : cls == HRL_CLOSEST_BOX    ? HRL_SCAN_BOX
         : cls == HRL_CLOSEST_FOOD   ? HRL_SCAN_FOOD
         : cls == HRL_CLOSEST_POISON ? HRL_SCAN_POISON
                                     : HRL_CHASE_ROBOT;
}
HRL_DEV void build_surf(SurfSet &S, int s, const DevCfg &c, const float *items, uint32_t classes) {
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int cls = HRL_CLOSEST_GROUND, idx = 0;
    bool there = false;
    if (s == S_GROUND) {
        v[2] = 1.f; v[3] = c.ground_z;
        there = true;
    } else if (s < S_BOX) {
        cls = HRL_CLOSEST_WALL; idx = s - S_PLANE0;
        there = idx < c.n_planes;
        v[0] = c.plane_n[idx][0]; v[1] = c.plane_n[idx][1]; v[2] = c.plane_n[idx][2]; v[3] = c.plane_d[idx];
    } else if (s == S_BOX) {
        cls = HRL_CLOSEST_BOX;
        there = c.n_boxes > 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { v[k] = c.box_lo[k]; v[3 + k] = c.box_hi[k]; }
    } else {
        const int i = s - S_ITEM0; /* 0..63 */
        const bool gather = c.kind == HRL_ANT_GATHER || c.kind == HRL_POINT_GATHER;
        cls = i < c.n_food ? HRL_CLOSEST_FOOD : HRL_CLOSEST_POISON; idx = i;
        there = gather && items != nullptr && i < c.n_food + c.n_poison && 2 * i + 1 < c.items_stride; /* the scanner's item set (render_core.h: make_prim) */
        if (there) { /* the step's cube: sphere_vs_surface */
            const float ix = items[2 * i], iy = items[2 * i + 1];
            there = fin_(ix) && fin_(iy); /* (clampf passes a NaN bound: such a cube would be a slab, not nothing) */
            v[0] = ix - ITEM_HALF; v[1] = iy - ITEM_HALF; v[2] = ITEM_Z - ITEM_HALF; v[3] = ix + ITEM_HALF; v[4] = iy + ITEM_HALF; v[5] = ITEM_Z + ITEM_HALF;
        }
    }
    const bool live = there && (classes & class_bit(cls)) != 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) S.v[k][s] = v[k];
    S.meta[s] = (uint32_t)cls | (live ? 256u : 0u) | ((uint32_t)idx << 16);
}

/* ------------------------------------------------------------------------------------------------ candidates */
struct Cand { float d, a[3], b[3], n[3]; }; /* distance, on_link, on_surface, normal */

/* leg and segment of a capsule link: segment 0 = the hip capsule 9 + l, 1 = aux 1 + 2 l, 2 = foot 2 + 2 l (the step's level) */
HRL_DEV void leg_seg(int link, int *leg, int *seg) {
    const bool hip = link >= 9;
    *leg = hip ? link - 9 : (link - 1) >> 1;
    *seg = hip ? 0 : 1 + ((link - 1) & 1);
}
/* whether the step holds a capsule pair of links a and b: different legs, not two hip capsules */
HRL_DEV bool self_pair(int a, int b) {
    if (a < 1 || a >= LINKS || b < 1 || b >= LINKS) return false;
    int la, sa, lb, sb;
    leg_seg(a, &la, &sa);
    leg_seg(b, &lb, &sb);
    return la != lb && (sa != 0 || sb != 0);
}

/* a plane against the segment w0 - w1 (world) of radius r: the lower end, a tie to w1 */
HRL_DEV void link_plane(const float *w0, const float *w1, float r, const float *n, float off, bool ground, Cand &o) {
    const float h0 = ground ? w0[2] - off : dot3(n, w0) - off, h1 = ground ? w1[2] - off : dot3(n, w1) - off;
    const bool first = h0 < h1;
    const float h = pick(first, h0, h1);
    o.d = h - r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = pick(first, w0[k], w1[k]);
        o.n[k] = n[k];
        o.a[k] = fma_(-r, n[k], p);
        o.b[k] = fma_(-h, n[k], p);
    }
}
/* a box against the capsule q + c0 .. q + c1 of radius r: sphere_vs_surface's box arm */
HRL_DEV void link_box(const float *q, const float *c0, const float *c1, float r, const float *lo, const float *hi, Cand &o) {
    float pw[3], d[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pw[k] = q[k] + c0[k]; d[k] = c1[k] - c0[k]; }
    const float t = seg_box_t(pw, d, lo, hi);
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = q[k] + fma_(d[k], t, c0[k]);
    o.d = sphere_vs_box(x, r, lo, hi, o.n);
    const float reach = o.d + r;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.a[k] = fma_(-r, o.n[k], x[k]); o.b[k] = fma_(-reach, o.n[k], x[k]); }
}
/* capsule `mine` against capsule `other` (ends relative to O in L), capsule_pair restated: the capsule of the lower leg is the step's first */
HRL_DEV void link_link(const DevCfg &c, const float *q, const LinkSet &L, int mine, int other, Cand &o) {
    int lm, sm, lo_, so;
    leg_seg(mine, &lm, &sm);
    leg_seg(other, &lo_, &so);
    const bool swap = lo_ < lm;
    const int A = swap ? other : mine, B = swap ? mine : other, a = swap ? so : sm, b = swap ? sm : so;
    float p1[3], q1[3], p2[3], q2[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) { p1[t] = L.v[t][A]; q1[t] = L.v[3 + t][A]; p2[t] = L.v[t][B]; q2[t] = L.v[3 + t][B]; }
    const float aa = a == 2 ? 0.32f : 0.08f, ia = a == 2 ? 3.125f : 12.5f, ee = b == 2 ? 0.32f : 0.08f, ie = b == 2 ? 3.125f : 12.5f;
    float d1[3], d2[3], r[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) { d1[t] = q1[t] - p1[t]; d2[t] = q2[t] - p2[t]; r[t] = p1[t] - p2[t]; }
    const float f = dot3(d2, r), cc = dot3(d1, r), bb = dot3(d1, d2);
    const float denom = fma_(aa, ee, -(bb * bb));
    float sp = 0.f, tp;
    if (denom > 1e-9f) sp = clampf(fma_(bb, f, -(cc * ee)) / denom, 0.f, 1.f);
    tp = fma_(bb, sp, f) * ie;
    if (tp < 0.f) { tp = 0.f; sp = clampf(-cc * ia, 0.f, 1.f); }
    else if (tp > 1.f) { tp = 1.f; sp = clampf((bb - cc) * ia, 0.f, 1.f); }
    float c1[3], c2[3], dv[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) { c1[t] = fma_(d1[t], sp, p1[t]); c2[t] = fma_(d2[t], tp, p2[t]); dv[t] = c1[t] - c2[t]; }
    const float d2n = dot3(dv, dv), len = sqrtf(d2n), rc = c.r_caps;
    o.d = len - (rc + rc);
    const float il = len > 0.f ? 1.f / len : 0.f, sg = swap ? -1.f : 1.f; /* (c - c' is c1 - c2 or its exact negative) */
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const float cm = pick(swap, c2[t], c1[t]), co = pick(swap, c1[t], c2[t]);
        o.n[t] = len > 0.f ? (sg * dv[t]) * il : (t == 2 ? 1.f : 0.f);
        o.a[t] = q[t] + fma_(-rc, o.n[t], cm);
        o.b[t] = q[t] + fma_(rc, o.n[t], co);
    }
}
/* a plane against the cube's 8 corners: the deepest, an equal one stays with the earlier corner */
HRL_DEV void cube_plane(const float *q, const float *X, const float *Y, const float *Z, const float *n, float off, bool ground, Cand &o) {
    float best = inf_(), p[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float sx = (i & 1) ? CUBE_HALF : -CUBE_HALF, sy = (i & 2) ? CUBE_HALF : -CUBE_HALF, sz = (i & 4) ? CUBE_HALF : -CUBE_HALF;
        float w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = q[k] + fma_(sz, Z[k], fma_(sy, Y[k], sx * X[k]));
        const float h = ground ? w[2] - off : dot3(n, w) - off;
        const bool won = h < best;
        best = pick(won, h, best);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = pick(won, w[k], p[k]);
    }
    o.d = best;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.n[k] = n[k]; o.a[k] = p[k]; o.b[k] = fma_(-best, n[k], p[k]); }
}
/* a box against the cube: the cube's corners against the box, then the box's corners against the cube in its own axes */
HRL_DEV void cube_box(const float *q, const float *X, const float *Y, const float *Z, const float *lo, const float *hi, Cand &o) {
    o.d = inf_();
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.a[k] = 0.f; o.b[k] = 0.f; o.n[k] = 0.f; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float sx = (i & 1) ? CUBE_HALF : -CUBE_HALF, sy = (i & 2) ? CUBE_HALF : -CUBE_HALF, sz = (i & 4) ? CUBE_HALF : -CUBE_HALF;
        float w[3], n[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = q[k] + fma_(sz, Z[k], fma_(sy, Y[k], sx * X[k]));
        const float d = sphere_vs_box(w, 0.f, lo, hi, n);
        const bool won = d < o.d;
        o.d = pick(won, d, o.d);
#pragma unroll
        for (int k = 0; k < 3; ++k) { o.a[k] = pick(won, w[k], o.a[k]); o.b[k] = pick(won, fma_(-d, n[k], w[k]), o.b[k]); o.n[k] = pick(won, n[k], o.n[k]); }
    }
    const float blo[3] = {-CUBE_HALF, -CUBE_HALF, -CUBE_HALF}, bhi[3] = {CUBE_HALF, CUBE_HALF, CUBE_HALF};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float pc[3] = {(i & 1) ? hi[0] : lo[0], (i & 2) ? hi[1] : lo[1], (i & 4) ? hi[2] : lo[2]};
        const float dv[3] = {pc[0] - q[0], pc[1] - q[1], pc[2] - q[2]};
        const float l[3] = {dot3(dv, X), dot3(dv, Y), dot3(dv, Z)};
        float nl[3];
        const float d = sphere_vs_box(l, 0.f, blo, bhi, nl);
        const bool won = d < o.d;
        o.d = pick(won, d, o.d);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float nw = fma_(nl[2], Z[k], fma_(nl[1], Y[k], nl[0] * X[k]));
            o.a[k] = pick(won, q[k] + fma_(-d, nw, dv[k]), o.a[k]); o.b[k] = pick(won, pc[k], o.b[k]); o.n[k] = pick(won, -nw, o.n[k]);
        }
    }
}

/* Candidate (link, s): s < S_SCENE a surface of the table, else the link s - S_LINK0.  Returns whether it is one at all (the surface is
 * live, the pair exists, the link is ok) -- then `o` is set and *cls, *idx name its cell and its index there.  Whether it COUNTS is
 * counts(o.d). */
HRL_DEV bool pair(const DevCfg &c, const float *st, const LinkSet &L, const SurfSet &S, uint32_t classes, int link, int s, int *cls, int *idx, Cand &o) {
    const bool point = c.kind == HRL_POINT_GATHER;
    const float q[3] = {st[HRL_QPOS_OFF], st[HRL_QPOS_OFF + 1], st[HRL_QPOS_OFF + 2]};
    o.d = inf_();
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.a[k] = 0.f; o.b[k] = 0.f; o.n[k] = 0.f; }
    *cls = HRL_CLOSEST_SELF; *idx = 0;
    if (link < 0 || link >= links::n_links(c.kind) || s < 0 || s >= S_ALL || L.ok[link] == 0u) return false;
    if (s >= S_LINK0) {
        const int other = s - S_LINK0;
        *idx = other;
        if (point || (classes & HRL_CHASE_ROBOT) == 0u || !self_pair(link, other) || L.ok[other] == 0u) return false;
        link_link(c, q, L, link, other, o);
        return true;
    }
    const uint32_t meta = S.meta[s];
    *cls = (int)(meta & 255u); *idx = (int)(meta >> 16);
    if ((meta & 256u) == 0u) return false;
    const float v[6] = {S.v[0][s], S.v[1][s], S.v[2][s], S.v[3][s], S.v[4][s], S.v[5][s]};
    const float e0[3] = {L.v[0][link], L.v[1][link], L.v[2][link]}, e1[3] = {L.v[3][link], L.v[4][link], L.v[5][link]}, e2[3] = {L.v[6][link], L.v[7][link], L.v[8][link]};
    const bool plane = s < S_BOX;
    if (point) {
        if (plane) cube_plane(q, e0, e1, e2, v, v[3], s == S_GROUND, o);
        else cube_box(q, e0, e1, e2, v, v + 3, o);
    } else {
        const float r = link == 0 ? c.r_torso : c.r_caps;
        if (plane) {
            const float w0[3] = {q[0] + e0[0], q[1] + e0[1], q[2] + e0[2]}, w1[3] = {q[0] + e1[0], q[1] + e1[1], q[2] + e1[2]};
            link_plane(w0, w1, r, v, v[3], s == S_GROUND, o);
        } else link_box(q, e0, e1, r, v, v + 3, o);
    }
    return true;
}

/* ------------------------------------------------------------------------------------------------ the winner of a cell */
/* (d, idx) -> a word whose unsigned order is d's order (d counts: neither NaN nor infinite; -0 is +0), then idx's */
HRL_DEV unsigned long long key_of(float d, int idx) {
    const float z = d + 0.f;
    uint32_t b;
    __builtin_memcpy(&b, &z, 4);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (unsigned long long)(uint32_t)idx;
}
/* the surface number of index idx of class cls: the inverse of build_surf's / pair's naming */
HRL_DEV int surf_of(int cls, int idx) {
    return cls == HRL_CLOSEST_GROUND ? S_GROUND : cls == HRL_CLOSEST_WALL ? S_PLANE0 + idx : cls == HRL_CLOSEST_BOX ? S_BOX : cls == HRL_CLOSEST_SELF ? S_LINK0 + idx : S_ITEM0 + idx;
}
HRL_DEV int32_t word_of(int cls, int idx) {
    const int32_t hit = cls == HRL_CLOSEST_GROUND ? HRL_HIT_GROUND
                      : cls == HRL_CLOSEST_WALL   ? HRL_HIT_WALL
                      : cls == HRL_CLOSEST_BOX    ? HRL_HIT_BOX
                      : cls == HRL_CLOSEST_FOOD   ? HRL_HIT_FOOD
                      : cls == HRL_CLOSEST_POISON ? HRL_HIT_POISON
                                                  : HRL_HIT_ROBOT;
    return hit | (int32_t)(idx << 8);
}
HRL_DEV float one_nan(float v) { return v != v ? __builtin_nanf("") : v; } /* 0x7FC00000: which NaN an operation yields differs between processors */

struct Answer { float distance; int32_t which; float on_link[3], on_surface[3], normal[3]; };

/* The answer of cell (link, cls) whose least key is `key` (KEY_NONE: no candidate counted). */
HRL_DEV void answer(const DevCfg &c, const float *st, const LinkSet &L, const SurfSet &S, uint32_t classes, int link, int cls, unsigned long long key, Answer &a) {
    const bool met = key != KEY_NONE;
    const int idx = met ? (int)(uint32_t)(key & 0xffffffffull) : 0;
    const int s = surf_of(cls, idx < 64 ? idx : 0); /* (an index is a plane, an item or a link: < 64) */
    Cand o;
    int cls2, idx2;
    const bool is = pair(c, st, L, S, classes, link, s, &cls2, &idx2, o);
    const bool ok = met && is && counts(o.d);
    a.distance = ok ? o.d + 0.f : inf_();
    a.which = ok ? word_of(cls, idx) : HRL_HIT_NONE;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.on_link[k] = ok ? one_nan(o.a[k]) : 0.f;
        a.on_surface[k] = ok ? one_nan(o.b[k]) : 0.f;
        a.normal[k] = ok ? one_nan(o.n[k]) : 0.f;
    }
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_closest_spec *s) {
    if (!s) return "null closest spec";
    if (s->struct_size != sizeof(hrl_closest_spec)) return "hrl_closest_spec.struct_size is not sizeof(hrl_closest_spec): initialise the record with hrl_closest_default_spec()";
    if (s->classes == 0u || (s->classes & ~HRL_CLOSEST_ALL) != 0u)
        return "closest classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND (the target post is no collision shape)";
    if (s->reserved != 0u) return "closest reserved must be 0";
    return "";
}
inline std::string validate_out(const hrl_closest_out *o) {
    if (!o) return "null closest out";
    if (!o->distance && !o->which && !o->on_link && !o->on_surface && !o->normal) return "closest out holds no pointer: at least one output must be given";
    return "";
}
inline int default_spec(const hrl_config *c, hrl_closest_spec *s) {
    if (!s || !c || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->classes = HRL_CLOSEST_ALL;
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: a link per lane and a surface per lane; a pair per lane, reduced to the
 * least key of its cell; a cell per lane. */
inline void closest_env_host(const DevCfg &c, const float *st, const float *items, const hrl_closest_spec &sp, const hrl_closest_out &out, size_t env) {
    LinkSet L;
    SurfSet S;
    unsigned long long key[CELLS];
    const int B = links::n_links(c.kind);
    memset(&L, 0, sizeof L);
    for (int link = 0; link < B; ++link) build_link(L, link, c, st);
    for (int s = 0; s < S_SCENE; ++s) build_surf(S, s, c, items, sp.classes);
    for (int cell = 0; cell < CELLS; ++cell) key[cell] = KEY_NONE;
    for (int p = 0; p < B * S_ALL; ++p) {
        const int link = p / S_ALL, s = p - link * S_ALL;
        Cand o;
        int cls, idx;
        if (pair(c, st, L, S, sp.classes, link, s, &cls, &idx, o) && counts(o.d)) {
            const unsigned long long k = key_of(o.d, idx);
            if (k < key[link * CLASSES + cls]) key[link * CLASSES + cls] = k;
        }
    }
    for (int cell = 0; cell < B * CLASSES; ++cell) {
        const int link = cell / CLASSES, cls = cell - link * CLASSES;
        Answer a;
        answer(c, st, L, S, sp.classes, link, cls, key[cell], a);
        const size_t at = env * (size_t)(B * CLASSES) + (size_t)cell;
        if (out.distance) out.distance[at] = a.distance;
        if (out.which) out.which[at] = a.which;
        for (int k = 0; k < 3; ++k) {
            if (out.on_link) out.on_link[3 * at + k] = a.on_link[k];
            if (out.on_surface) out.on_surface[3 * at + k] = a.on_surface[k];
            if (out.normal) out.normal[3 * at + k] = a.normal[k];
        }
    }
}
/* hrl_closest on host pointers; returns the status and leaves the reason in `why` */
inline int closest_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_closest_spec *sp, const uint8_t *mask, const hrl_closest_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        closest_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, *sp, *out, (size_t)e);
    }
    return HRL_OK;
}
#endif

}  // namespace closest
}  // namespace hrl
