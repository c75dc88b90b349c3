/*
 * scan_core.h -- specification of the batched range scanner (include/hrl_scan.h), written once as plain C++: the device kernel
 * (scan_hip.hip) and the host build of the tests (tests/scan_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The scan of one env is a pure function of (DevCfg, its state / items / aux record, hrl_scan_spec):
 *
 *   table_frame  the frame of the env's table: centred on the robot, WORLD axes (render_core.h: view_frame in HRL_VIEW_EGO), so every
 *                ray starts at (0, 0) of the table, rectangles stay axis-aligned and the heading enters the ray directions alone
 *   forward      the unit vector rays are counted from: world +x, or the ground projection of the torso's X axis (view_frame's rule)
 *   build_slot   slot s < S_SLOTS of the table: the renderer's primitive of that slot (render_core.h: make_prim, slots R_PLANE0 ..
 *                R_CAPS0 - 1: the four lateral planes, the maze box, the target, 64 items), a plane moved out to the wall's centre
 *                line (WALL_HALF), its hit code, and the cull: a slot is dropped when its class bit is off or its padded box lies
 *                farther than max_range from the origin
 *   ray_dir      direction of ray k: forward * cos(theta_k) + left * sin(theta_k), theta_k = fma(k, step_angle, first_angle), sincos_spec
 *   isect_*      one intersection function per primitive type: the ray parameter t >= 0 of the first point of the shape on the ray (0
 *                when the origin is in it; for the half plane: outside the arena), +inf when there is none
 *   scan_ray     walks the bit list of the surviving slots in slot order: a candidate counts if t <= max_range, the smallest t wins,
 *                equal t stays with the lower slot
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items.  Every acceptance test is a
 * float comparison that is false for NaN, so a shape with a non-finite parameter is not seen; aux[3] is range-checked as an integer.
 */
#pragma once
#include "../../include/hrl_scan.h"
#include "render_core.h" /* Frame, Prim, view_frame, make_prim (and through it step_core.h: fma_, sincos_spec, quat_axes, DevCfg) */

namespace hrl {
namespace scan {

using render::Frame;
using render::Prim;
using render::inf_;
using render::max_;
using render::min_;

constexpr int S_SLOTS = render::R_CAPS0; /* 70: planes 0..3, the box, the target, 64 items */
static_assert(S_SLOTS > 64 && S_SLOTS <= 128, "two 64-bit lists hold the table");
constexpr int MAX_RAYS = HRL_SCAN_MAX_RAYS;
/* Half the thickness of an arena wall (walls 0.1 thick centred on +-size / 2: host_cfg.h build_devcfg, wall.xml).  DevCfg's lateral
 * planes are the walls' INNER faces, what the robot collides with and the renderer paints; the reference's sense_walls meets the
 * bounding LINES through the walls' centres (sizeable_enclosed_scene.py:28-34, maze_scene.py), and so does the scanner: its wall k is
 * lateral plane k moved outwards by WALL_HALF. */
constexpr float WALL_HALF = 0.05f;

/* ------------------------------------------------------------------------------------------------ frame and directions */
HRL_DEV Frame table_frame(const float *st) {
    hrl_view v = {};
    v.mode = HRL_VIEW_EGO;
    return render::view_frame(v, st);
}
/* view_frame's heading rule (render_core.h), restated for the forward vector: when the projection vanishes, world +x */
HRL_DEV void forward(int frame, const float *st, float *fx, float *fy) {
    *fx = 1.f; *fy = 0.f;
    if (frame == HRL_SCAN_HEADING) {
        float X[3], Y[3], Z[3];
        quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
        const float n2 = fma_(X[0], X[0], X[1] * X[1]);
        if (n2 >= 1e-12f && n2 <= 3.0e38f) { /* (false for NaN; an overflowed norm is infinite) */
            const float inv = 1.f / sqrtf(n2);
            *fx = X[0] * inv; *fy = X[1] * inv;
        }
    }
}
HRL_DEV float ray_angle(const hrl_scan_spec &sp, int k) { return fma_((float)k, sp.step_angle, sp.first_angle); }
HRL_DEV void ray_dir(const hrl_scan_spec &sp, int k, float fx, float fy, float *dx, float *dy) {
    float s, c;
    sincos_spec(ray_angle(sp, k), &s, &c);
    *dx = fma_(fx, c, -(fy * s));
    *dy = fma_(fy, c, fx * s);
}

/* ------------------------------------------------------------------------------------------------ the table */
struct alignas(16) ScanSet { /* 1.7 KB; on the device in LDS.  Structure of arrays: built lane = slot, walked one slot wave-wide */
    float p[4][S_SLOTS];     /* P_HALF: nx, ny, offset (outside where nx x + ny y + offset < 0) | P_RECT: centre x, y, half sizes | P_DISC: centre, r^2 */
    uint32_t meta[S_SLOTS];  /* type | kept << 8 */
    int32_t code[S_SLOTS];   /* what `hit` reports for this slot */
    float fwd[2];
};

/* class bit and hit code of a slot */
HRL_DEV void slot_identity(int slot, const DevCfg &c, const int32_t *aux, uint32_t *cls, int32_t *code) {
    if (slot < render::R_BOX) { *cls = HRL_SCAN_WALL; *code = HRL_HIT_WALL | (slot << 8); }
    else if (slot == render::R_BOX) { *cls = HRL_SCAN_BOX; *code = HRL_HIT_BOX; }
    else if (slot == render::R_TARGET) {
        const bool maze = c.kind == HRL_ANT_MAZE || c.kind == HRL_ANT_MAZE_MJ;
        const int t = aux[3];
        *cls = HRL_SCAN_TARGET; *code = HRL_HIT_TARGET | ((maze && t >= 0 && t < HRL_MAX_TARGETS ? t : 0) << 8);
    } else {
        const int i = slot - render::R_ITEM0;
        *cls = i < c.n_food ? HRL_SCAN_FOOD : HRL_SCAN_POISON; *code = (i < c.n_food ? HRL_HIT_FOOD : HRL_HIT_POISON) | (i << 8);
    }
}
/* the cull: the squared distance from the origin to the primitive's padded box against max_range^2, widened by 2^-18 (the rounding of
 * either side is 2^-23 of it; the box itself is padded by a millimetre).  False for an empty box. */
HRL_DEV bool in_reach(const Prim &P, float max_range) {
    const float ex = max_(max_(P.bb[0], -P.bb[1]), 0.f), ey = max_(max_(P.bb[2], -P.bb[3]), 0.f);
    const float r2 = max_range * max_range;
    return P.type != render::P_NONE && fma_(ex, ex, ey * ey) <= fma_(r2, 3.814697265625e-6f, r2);
}
HRL_DEV void build_slot(ScanSet &S, int slot, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frame &f, const hrl_scan_spec &sp) {
    Prim P;
    render::make_prim(P, slot, c, st, items, aux, f);
    if (P.type == render::P_HALF) P.p[2] = fma_(P.p[0], f.cx, P.p[1] * f.cy) - (c.plane_d[slot] - WALL_HALF); /* (in the table's frame p[0], p[1] are the world normal) */
    uint32_t cls;
    int32_t code;
    slot_identity(slot, c, aux, &cls, &code);
    const bool kept = (sp.classes & cls) != 0u && in_reach(P, sp.max_range);
#pragma unroll
    for (int k = 0; k < 4; ++k) S.p[k][slot] = P.p[k];
    S.meta[slot] = (uint32_t)P.type | (kept ? 256u : 0u);
    S.code[slot] = code;
}
HRL_DEV bool kept(const ScanSet &S, int slot) { return (S.meta[slot] & 256u) != 0u; }

/* ------------------------------------------------------------------------------------------------ intersections: origin (0, 0), unit direction (dx, dy) */
/* inside where nx x + ny y + off >= 0; leaves through the boundary where the direction has a negative component along the normal */
HRL_DEV float isect_half(float nx, float ny, float off, float dx, float dy) {
    const float den = fma_(nx, dx, ny * dy);
    const float t = off / -den;
    return off < 0.f ? 0.f : (den < 0.f ? t : inf_());
}
/* one axis of the slab test: the interval of t in which the ray is within [c - h, c + h]; idir = 1 / d.  Empty (lo > hi) or NaN when it
 * never is.  A direction component whose reciprocal is not finite (zero, or a denormal) runs parallel to the slab: (c - h) * inf would be
 * NaN on the slab's edge. */
HRL_DEV void slab(float c, float h, float idir, float *lo, float *hi) {
    if (fabsf(idir) <= 3.0e38f) {
        const float a = (c - h) * idir, b = (c + h) * idir;
        *lo = min_(a, b); *hi = max_(a, b);
    } else {
        const bool in = fabsf(c) <= h;
        *lo = in ? -inf_() : inf_(); *hi = in ? inf_() : -inf_();
    }
}
HRL_DEV float isect_rect(float cx, float cy, float hx, float hy, float idx, float idy) {
    float lox, hix, loy, hiy;
    slab(cx, hx, idx, &lox, &hix);
    slab(cy, hy, idy, &loy, &hiy);
    const float tn = max_(lox, loy), tf = min_(hix, hiy);
    const bool ok = lox <= hix && loy <= hiy && tn <= tf && tf >= 0.f; /* (each false for NaN: min_ / max_ alone would drop one) */
    return ok ? max_(tn, 0.f) : inf_();
}
/* through the distance e of the centre from the ray's line (not b^2 - (|c|^2 - r^2), which cancels at 20 m) */
HRL_DEV float isect_disc(float cx, float cy, float r2, float dx, float dy) {
    const float cc = fma_(cx, cx, cy * cy), b = fma_(cx, dx, cy * dy), e = fma_(cx, dy, -(cy * dx));
    const float h = fma_(-e, e, r2);
    return cc <= r2 ? 0.f : ((h >= 0.f && b > 0.f) ? b - sqrtf(h) : inf_());
}

struct Ray { float dx, dy, idx, idy, best; int32_t hit; };

HRL_DEV void try_slot(const ScanSet &S, int slot, float max_range, Ray &r) {
    const int type = (int)(S.meta[slot] & 255u);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    float t = inf_();
    if (type == render::P_HALF) t = isect_half(p0, p1, p2, r.dx, r.dy);
    else if (type == render::P_RECT) t = isect_rect(p0, p1, p2, p3, r.idx, r.idy);
    else if (type == render::P_DISC) t = isect_disc(p0, p1, p2, r.dx, r.dy);
    if (t <= max_range && t < r.best) { r.best = t; r.hit = S.code[slot]; }
}

/* Ray k of the env.  m0 / m1: bit i set = slot i / 64 + i survived the cull. */
HRL_DEV void scan_ray(const ScanSet &S, unsigned long long m0, unsigned long long m1, const hrl_scan_spec &sp, int k, float *range, int32_t *hit) {
    Ray r;
    ray_dir(sp, k, S.fwd[0], S.fwd[1], &r.dx, &r.dy);
    r.idx = 1.f / r.dx; r.idy = 1.f / r.dy;
    r.best = inf_(); r.hit = HRL_HIT_NONE;
    for (unsigned long long m = m0; m; m &= m - 1) try_slot(S, __builtin_ctzll(m), sp.max_range, r);
    for (unsigned long long m = m1; m; m &= m - 1) try_slot(S, 64 + __builtin_ctzll(m), sp.max_range, r);
    *range = r.hit != HRL_HIT_NONE ? r.best : sp.max_range;
    *hit = r.hit;
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_scan_spec *s) {
    if (!s) return "null scan spec";
    if (s->struct_size != sizeof(hrl_scan_spec)) return "hrl_scan_spec.struct_size is not sizeof(hrl_scan_spec): initialise the record with hrl_scan_default_spec()";
    if (s->n_rays < 1 || s->n_rays > MAX_RAYS) return "scan n_rays must be within 1..512";
    if (s->frame != HRL_SCAN_WORLD && s->frame != HRL_SCAN_HEADING) return "unknown scan frame";
    /* theta_k is monotone in k: the two ends bound every ray (false for NaN) */
    const float a = s->first_angle, b = __builtin_fmaf((float)(s->n_rays - 1), s->step_angle, s->first_angle); /* (ray_angle, on the host) */
    if (!(fabsf(a) <= HRL_SCAN_MAX_ANGLE) || !(fabsf(s->step_angle) <= 2.f * HRL_SCAN_MAX_ANGLE) || !(fabsf(b) <= HRL_SCAN_MAX_ANGLE))
        return "scan angles must be finite and at most 64 rad in magnitude for every ray";
    if (!(s->max_range > 0.f) || !(s->max_range <= 3.0e38f)) return "scan max_range must be finite and positive";
    if (s->classes == 0u || (s->classes & ~HRL_SCAN_ALL) != 0u) return "scan classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET";
    return "";
}

/* 64 rays, a full circle centred on forward, all classes; max_range per kind: gather sqrt(wx^2 + wy^2) | maze sqrt(10^2 + 18^2)
 * (maze_scene.py:10) | flagrun (flag_size + 2) sqrt(2) (ant_flagrun_env.py:59-61) | flat 10 */
inline int default_spec(const hrl_config *c, int32_t frame, hrl_scan_spec *s) {
    if (!c || !s || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN) return HRL_ERR_BAD_ARG;
    if (frame != HRL_SCAN_WORLD && frame != HRL_SCAN_HEADING) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    const double pi = 3.14159265358979323846;
    s->struct_size = sizeof(*s); s->n_rays = 64; s->frame = frame; s->classes = HRL_SCAN_ALL;
    s->first_angle = (float)(-pi + pi / 64); s->step_angle = (float)(2 * pi / 64);
    double r = 10.0;
    switch (c->env_kind) {
        case HRL_ANT_GATHER: case HRL_POINT_GATHER: r = sqrt((double)c->world_size[0] * c->world_size[0] + (double)c->world_size[1] * c->world_size[1]); break;
        case HRL_ANT_MAZE: case HRL_ANT_MAZE_MJ: r = sqrt(10.0 * 10.0 + 18.0 * 18.0); break;
        case HRL_ANT_FLAGRUN: r = ((double)c->flag_size + 2.0) * sqrt(2.0); break;
        default: break;
    }
    s->max_range = (float)r;
    return HRL_OK;
}

#ifdef HRL_EMU
/* The whole launch on the host, partitioned as the kernel partitions it: per env the table and its list, then runs of 64 rays. */
inline void scan_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_scan_spec &sp, float *range, int32_t *hit) {
    ScanSet S;
    const Frame f = table_frame(st);
    forward(sp.frame, st, &S.fwd[0], &S.fwd[1]);
    for (int slot = 0; slot < S_SLOTS; ++slot) build_slot(S, slot, c, st, items, aux, f, sp);
    unsigned long long m0 = 0, m1 = 0;
    for (int slot = 0; slot < 64; ++slot) if (kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (kept(S, slot)) m1 |= 1ull << (slot - 64);
    for (int base = 0; base < sp.n_rays; base += 64)
        for (int k = base; k < base + 64 && k < sp.n_rays; ++k) scan_ray(S, m0, m1, sp, k, range + k, hit + k);
}
/* hrl_scan on host pointers; returns the status and leaves the reason in `why` */
inline int scan_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_scan_spec *sp, const uint8_t *mask, float *range, int32_t *hit, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty() && (!b || !b->state || !b->aux || !range || !hit)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        scan_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp,
                      range + (size_t)e * sp->n_rays, hit + (size_t)e * sp->n_rays);
    }
    return HRL_OK;
}
#endif

}  // namespace scan
}  // namespace hrl
