/*
 * chase_core.h -- specification of the batched chase camera (include/hrl_chase.h), written once as plain C++: the device kernel
 * (chase_hip.hip) and the host build of the tests (tests/chase_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The image of one env is a pure function of (DevCfg, its state / items / aux record, hrl_chase_spec):
 *
 *   view_of      the camera: F, L, U from the scanner's forward vector, the spec's yaw and pitch pairs; the eye E = T - distance F, kept
 *                as its offset from the robot in the ground plan (exact: the table is centred on the robot) and its world z
 *   build_slot   slot s of the scanner's table (scan_core.h: build_slot, culled about the ROBOT against cull_range = (max_range * the
 *                longest |D| + distance) * 1.01: t is a depth, so a point seen lies up to max_range |D| from the eye, and the eye lies
 *                `distance` |F| from the robot), RE-CENTRED on the eye's ground position, with the camera's z_extent; a slot whose solid
 *                contains the eye loses its `kept` bit
 *   build_prim   primitive k of the robot: 0 the torso's sphere, 2 l - 1 the open cylinder of link l, 2 l the ball at its far end (the
 *                point bot: 0 the cube), from links::link_world's p0 / p1, relative to the eye, with its ray-independent terms
 *   pixel_ray    D = F + u L + s U, NOT normalised: t is the depth along the optical axis
 *   try_slot     the span of the ray's ground-plan part through the slot's ground plan (camera::span_half / span_rect work for a
 *                direction of any length; span_disc is restated for one), then the camera's 3-D step on z(t) = fma(D_z, t, E_z)
 *   try_prim     ray against sphere, open cylinder or oriented cube.  The discriminants are formed from the ray's DISTANCE to the
 *                centre or to the axis (a cross product, a triple product), not as b^2 - |D|^2 (|oc|^2 - r^2), which cancels: at 7 m
 *                that form moves a silhouette by 1e-4 m, this one by 1e-6 m
 *   near_robot   the robot's cull, per pixel: the ray's line against a sphere about O that holds every drawn primitive (robot_bound)
 *   shade_pixel  scene slots in slot order, robot primitives in order, the ground: 0 < t <= max_range, strict < keeps the earlier one
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items, except sincos_spec's guarded
 * quadrant (link_world) and the guarded tile parity.  Every acceptance test is a comparison that is false for NaN.
 */
#pragma once
#include "../../include/hrl_chase.h"
#include "camera_core.h" /* z_extent, span_half, span_rect, col_u, row_s, shade_rgb, fin_, CHUNK (and scan_core.h, render_core.h, step_core.h) */
#include "links_core.h"  /* link_world */

namespace hrl {
namespace chase {

using camera::Span;
using camera::fin_;
using render::Frame;
using render::inf_;
using render::max_;
using render::min_;
using scan::ScanSet;

constexpr int S_SLOTS = scan::S_SLOTS; /* 70 */
constexpr int MAX_SIZE = HRL_CHASE_MAX_SIZE;
constexpr int CHUNK = camera::CHUNK;   /* pixels whose rgb bytes are staged at a time */
constexpr int PRIMS = 2 * HRL_LINKS_ANT - 1, PRIM_ROWS = 12, PRIM_PAD = 32; /* 25 primitives of 12 floats */
enum PrimType { Q_NONE = 0, Q_SPHERE, Q_CYLINDER, Q_BOX };
static_assert(PRIMS <= PRIM_PAD && PRIM_PAD <= 32, "one 32-bit list holds the robot");

/* ------------------------------------------------------------------------------------------------ the camera */
struct View {
    float F[3], L[2], U[3]; /* L_z = 0 */
    float ex, ey;           /* the eye's ground position relative to the robot's */
    float wx, wy, ez;       /* the eye in world coordinates */
    float oe[3];            /* O - E: the robot's origin relative to the eye */
    float gz;
    bool ok;                /* T and E are finite: the env sees */
};

HRL_DEV View view_of(const DevCfg &c, const float *st, const hrl_chase_spec &sp) {
    View v;
    float fx, fy;
    scan::forward(sp.frame, st, &fx, &fy);
    const float gx = fma_(fx, sp.yaw[0], -(fy * sp.yaw[1])), gy = fma_(fy, sp.yaw[0], fx * sp.yaw[1]);
    const float cp = sp.pitch[0], sn = sp.pitch[1];
    v.F[0] = cp * gx; v.F[1] = cp * gy; v.F[2] = sn;
    v.L[0] = -gy; v.L[1] = gx;
    v.U[0] = -(sn * gx); v.U[1] = -(sn * gy); v.U[2] = cp;
    const float tz = (sp.target_mode == HRL_EYE_TORSO ? st[HRL_QPOS_OFF + 2] : c.ground_z) + sp.target_height;
    v.ex = -(sp.distance * v.F[0]); v.ey = -(sp.distance * v.F[1]);
    v.wx = st[HRL_QPOS_OFF] + v.ex; v.wy = st[HRL_QPOS_OFF + 1] + v.ey;
    v.ez = fma_(-sp.distance, v.F[2], tz);
    v.oe[0] = -v.ex; v.oe[1] = -v.ey; v.oe[2] = st[HRL_QPOS_OFF + 2] - v.ez;
    v.gz = c.ground_z;
    v.ok = fin_(st[HRL_QPOS_OFF]) && fin_(st[HRL_QPOS_OFF + 1]) && fin_(tz) && fin_(v.wx) && fin_(v.wy) && fin_(v.ez);
    return v;
}

/* what scan::build_slot reads: the class bits and the range of its cull about the robot */
HRL_DEV hrl_scan_spec table_spec(const hrl_chase_spec &sp) {
    hrl_scan_spec s = {};
    const float dmax = sqrtf(fma_(sp.tan_half_h, sp.tan_half_h, fma_(sp.tan_half_v, sp.tan_half_v, 1.f)));
    s.struct_size = sizeof s; s.n_rays = 1; s.frame = sp.frame; s.classes = sp.classes & HRL_SCAN_ALL;
    s.max_range = fma_(sp.max_range, dmax, sp.distance) * 1.01f; /* (yaw's and pitch's norms are within 1e-3 of 1) */
    return s;
}

/* slot `slot` of the table about the eye, its z-interval, and whether it is walked */
HRL_DEV void build_slot(ScanSet &S, float *zl, float *zh, int slot, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frame &f, const hrl_scan_spec &ts,
                        const View &v) {
    scan::build_slot(S, slot, c, st, items, aux, f, ts);
    float lo, hi;
    camera::z_extent(slot, c, &lo, &hi);
    const int type = (int)(S.meta[slot] & 255u);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    bool over = false; /* the ground plan contains the eye's ground position */
    if (type == render::P_HALF) {
        const float off = fma_(p0, v.ex, fma_(p1, v.ey, p2));
        S.p[2][slot] = off;
        over = off < 0.f;
    } else if (type == render::P_RECT) {
        const float cx = p0 - v.ex, cy = p1 - v.ey;
        S.p[0][slot] = cx; S.p[1][slot] = cy;
        over = fabsf(cx) <= p2 && fabsf(cy) <= p3;
    } else if (type == render::P_DISC) {
        const float cx = p0 - v.ex, cy = p1 - v.ey;
        S.p[0][slot] = cx; S.p[1][slot] = cy;
        over = fma_(cx, cx, cy * cy) <= p2;
    }
    if (over && lo <= v.ez && v.ez <= hi) S.meta[slot] &= ~256u; /* the solid contains the eye: not drawn */
    zl[slot] = lo; zh[slot] = hi;
}

/* ------------------------------------------------------------------------------------------------ the robot's primitives */
struct alignas(16) PrimSet { /* 1.8 KB; on the device in LDS.  Structure of arrays: built lane = primitive, walked one primitive wave-wide */
    /* Q_SPHERE:   0..2 oc = centre - E | 11 r^2
     * Q_CYLINDER: 0..2 oc = p0 - E | 3..5 A = p1 - p0 | 6..8 n = oc x A | 9 |A|^2 | 10 oc . A | 11 r^2
     * Q_BOX:      0..2 oc . X, oc . Y, oc . Z | 3..5 X | 6..8 Y | 9..11 Z */
    float v[PRIM_ROWS][PRIM_PAD];
    float reach[PRIM_PAD];   /* how far from O the primitive reaches: |its far point - O| + r (the cube: half side * (|X| + |Y| + |Z|)) */
    uint32_t meta[PRIM_PAD]; /* type | drawn << 7 | link << 8 */
};
constexpr uint32_t DRAWN = 128u;

HRL_DEV int prim_link(int k) { return (k + 1) >> 1; }

HRL_DEV void build_prim(PrimSet &P, int k, const DevCfg &c, const float *st, const View &v, uint32_t classes) {
    const bool point = c.kind == HRL_POINT_GATHER;
    const int link = prim_link(k);
    links::Link K;
    links::link_world(c, st, link, K);
    const float *oe = v.oe;
    const bool cyl = (k & 1) != 0;
    float w[PRIM_ROWS];
    float X[3], Y[3], Z[3];
    quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
    float oc[3], A[3], n[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        oc[q] = links::pick(cyl, K.p0[q], K.p1[q]) + oe[q];
        A[q] = K.p1[q] - K.p0[q];
    }
    cross3(n, oc, A);
    const float r = k == 0 ? c.r_torso : c.r_caps;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        w[q] = links::pick(point, q == 0 ? dot3(oc, X) : (q == 1 ? dot3(oc, Y) : dot3(oc, Z)), oc[q]);
        w[3 + q] = links::pick(point, X[q], A[q]);
        w[6 + q] = links::pick(point, Y[q], n[q]);
    }
    w[9] = links::pick(point, Z[0], dot3(A, A));
    w[10] = links::pick(point, Z[1], dot3(oc, A));
    w[11] = links::pick(point, Z[2], r * r);
    bool fin = true;
#pragma unroll
    for (int q = 0; q < PRIM_ROWS; ++q) fin = fin && fin_(w[q]);
    const bool exists = point ? k == 0 : k < PRIMS;
    const uint32_t type = point ? Q_BOX : (cyl ? Q_CYLINDER : Q_SPHERE);
#pragma unroll
    for (int q = 0; q < PRIM_ROWS; ++q) P.v[q][k] = w[q];
    P.reach[k] = links::pick(point, render::POINT_HALF * ((sqrtf(dot3(X, X)) + sqrtf(dot3(Y, Y))) + sqrtf(dot3(Z, Z))), sqrtf(max_(dot3(K.p0, K.p0), dot3(K.p1, K.p1))) + r);
    P.meta[k] = type | ((exists && fin && (classes & HRL_CHASE_ROBOT) != 0u) ? DRAWN : 0u) | ((uint32_t)link << 8);
}
HRL_DEV bool drawn(const PrimSet &P, int k) { return (P.meta[k] & DRAWN) != 0u; }

/* The robot's cull: the squared radius of a sphere about O that holds every drawn primitive -- the largest reach, widened by 0.1 % and a
 * millimetre, four orders above the rounding of either side of near_robot's comparison at 50 m.  A ray whose line passes O farther
 * than that meets no primitive, so near_robot may skip the walk of the primitives; the result is the same either way. */
HRL_DEV float robot_bound(const PrimSet &P, uint32_t pm) {
    float r = 0.f;
    for (uint32_t m = pm; m; m &= m - 1) r = max_(r, P.reach[__builtin_ctz(m)]); /* (drawn primitives hold finite numbers only) */
    r = fma_(r, 1.001f, 1e-3f);
    return r * r;
}

/* ------------------------------------------------------------------------------------------------ rays */
struct Ray { float d[3], dd, inv_dd, idx, idy; };

HRL_DEV Ray pixel_ray(const hrl_chase_spec &sp, const View &v, int i, int j, float inv_w, float inv_h) {
    const float u = camera::col_u(j, sp.width, inv_w, sp.tan_half_h), s = camera::row_s(i, sp.height, inv_h, sp.tan_half_v);
    Ray r;
    r.d[0] = fma_(s, v.U[0], fma_(u, v.L[0], v.F[0]));
    r.d[1] = fma_(s, v.U[1], fma_(u, v.L[1], v.F[1]));
    r.d[2] = fma_(s, v.U[2], v.F[2]);
    r.dd = dot3(r.d, r.d);
    r.inv_dd = 1.f / r.dd;
    r.idx = 1.f / r.d[0]; r.idy = 1.f / r.d[1];
    return r;
}

/* whether the ray's line passes O within the robot's bound (rb2: robot_bound): false for NaN, as every primitive's acceptance is then */
HRL_DEV bool near_robot(const View &v, float rb2, const Ray &r) {
    float e[3];
    cross3(e, v.oe, r.d);
    return dot3(e, e) <= rb2 * r.dd;
}

/* camera::span_disc for a direction of any length, the null vector included: the roots of |t d - c|^2 = r^2 through the distance e / |d|
 * of the centre from the ray's line */
HRL_DEV Span span_disc(float cx, float cy, float r2, float dx, float dy) {
    const float cc = fma_(cx, cx, cy * cy), b = fma_(cx, dx, cy * dy), e = fma_(cx, dy, -(cy * dx)), dd = fma_(dx, dx, dy * dy);
    const float h = fma_(r2, dd, -(e * e));
    const float root = sqrtf(h);
    const bool in = cc <= r2;
    Span s;
    s.a = in ? 0.f : ((h >= 0.f && b > 0.f && dd > 0.f) ? (b - root) / dd : inf_());
    s.b = dd > 0.f ? (b + root) / dd : inf_(); /* (NaN when h < 0: no top or bottom is accepted then; a vertical ray never leaves) */
    s.face = in ? HRL_FACE_INSIDE : HRL_FACE_ROUND;
    return s;
}

struct Hit { float best; int32_t seg; };

HRL_DEV void offer(Hit &h, bool got, float t, float max_range, int32_t seg) {
    if (got && t > 0.f && t <= max_range && t < h.best) { h.best = t; h.seg = seg; }
}

/* the span of slot `slot` along the ray's ground-plan part, and from it the candidate (camera::try_slot's 3-D step with D_z for m) */
HRL_DEV void try_slot(const ScanSet &S, const float *zl, const float *zh, int slot, float max_range, float ez, const Ray &r, Hit &h) {
    const int type = (int)(S.meta[slot] & 255u);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    Span sp;
    sp.a = inf_(); sp.b = inf_(); sp.face = HRL_FACE_INSIDE;
    if (type == render::P_HALF) sp = camera::span_half(p0, p1, p2, r.d[0], r.d[1]);
    else if (type == render::P_RECT) sp = camera::span_rect(p0, p1, p2, p3, r.idx, r.idy);
    else if (type == render::P_DISC) sp = span_disc(p0, p1, p2, r.d[0], r.d[1]);
    const float lo = zl[slot], hi = zh[slot], dz = r.d[2];
    const float za = fma_(dz, sp.a, ez);
    float t = inf_();
    int32_t face = sp.face;
    bool got = false;
    if (lo <= za && za <= hi) { t = sp.a; got = true; }
    else if (za > hi && dz < 0.f) { t = (hi - ez) / dz; face = HRL_FACE_TOP; got = t <= sp.b; }
    else if (za < lo && dz > 0.f) { t = (lo - ez) / dz; face = HRL_FACE_BOTTOM; got = t <= sp.b; }
    offer(h, got, t, max_range, S.code[slot] | (face << 16));
}

HRL_DEV void try_prim(const PrimSet &P, int k, float max_range, const Ray &r, Hit &h) {
    const uint32_t meta = P.meta[k];
    const int type = (int)(meta & 127u);
    const int32_t code = HRL_HIT_ROBOT | (int32_t)((meta >> 8) << 8);
    const float oc[3] = {P.v[0][k], P.v[1][k], P.v[2][k]};
    if (type == Q_SPHERE) {
        float e[3];
        cross3(e, oc, r.d);
        const float b = dot3(r.d, oc), hh = fma_(P.v[11][k], r.dd, -dot3(e, e));
        const float t = (b - sqrtf(hh)) * r.inv_dd;
        offer(h, hh >= 0.f, t, max_range, code | (HRL_FACE_ROUND << 16));
    } else if (type == Q_CYLINDER) {
        const float A[3] = {P.v[3][k], P.v[4][k], P.v[5][k]}, n[3] = {P.v[6][k], P.v[7][k], P.v[8][k]};
        const float aa = P.v[9][k], ocA = P.v[10][k], r2 = P.v[11][k];
        float m[3];
        cross3(m, r.d, A);
        const float mm = dot3(m, m), w = dot3(oc, m), mn = dot3(m, n);
        const float hh = aa * fma_(r2, mm, -(w * w));
        const float t = (mn - sqrtf(hh)) / mm;
        const float s = fma_(t, dot3(r.d, A), -ocA); /* the hit's place along the axis, times |A| */
        offer(h, hh >= 0.f && s >= 0.f && s <= aa, t, max_range, code | (HRL_FACE_ROUND << 16));
    } else if (type == Q_BOX) {
        const float X[3] = {P.v[3][k], P.v[4][k], P.v[5][k]}, Y[3] = {P.v[6][k], P.v[7][k], P.v[8][k]}, Z[3] = {P.v[9][k], P.v[10][k], P.v[11][k]};
        const float dx = dot3(r.d, X), dy = dot3(r.d, Y), dz = dot3(r.d, Z);
        float lox, hix, loy, hiy, loz, hiz;
        scan::slab(oc[0], render::POINT_HALF, 1.f / dx, &lox, &hix);
        scan::slab(oc[1], render::POINT_HALF, 1.f / dy, &loy, &hiy);
        scan::slab(oc[2], render::POINT_HALF, 1.f / dz, &loz, &hiz);
        const float tn = max_(max_(lox, loy), loz), tf = min_(min_(hix, hiy), hiz);
        const bool ok = lox <= hix && loy <= hiy && loz <= hiz && tn <= tf;
        const int32_t face = (lox >= loy && lox >= loz) ? HRL_FACE_SIDE_X : (loy >= loz ? HRL_FACE_SIDE_Y : (dz < 0.f ? HRL_FACE_TOP : HRL_FACE_BOTTOM));
        offer(h, ok, tn, max_range, code | (face << 16));
    }
}

/* floor(a / tile) as an integer's lowest bit; 0 where the quotient is not a finite number of ordinary size */
HRL_DEV int tile_index(float a, float tile) {
    const float q = floorf(a / tile);
    return (int)(fabsf(q) < 1e9f ? q : 0.f);
}

/* The colour of a seg word, 0x00BBGGRR: integer arithmetic only, and no array is indexed at run time. */
HRL_DEV uint32_t shade_rgb(int32_t seg) {
    const int cls = seg & 255, index = (seg >> 8) & 255, face = (seg >> 16) & 7;
    if (cls == HRL_HIT_ROBOT) {
        const uint32_t base = index == 0 ? render::rgb_(HRL_RGB_TORSO) : index >= 9 ? render::rgb_(HRL_RGB_LEG0) : (index & 1) ? render::rgb_(HRL_RGB_LEG1) : render::rgb_(HRL_RGB_LEG2);
        constexpr unsigned long long SHADES = 128ull | (224ull << 9) | (176ull << 18) | (200ull << 27) | (256ull << 36) | (96ull << 45) | (256ull << 54); /* camera_core.h's */
        const uint32_t k = (uint32_t)((SHADES >> (9 * (face < 7 ? face : 0))) & 511ull);
        const uint32_t r = ((base & 255u) * k) >> 8, g = (((base >> 8) & 255u) * k) >> 8, b = (((base >> 16) & 255u) * k) >> 8;
        return r | (g << 8) | (b << 16);
    }
    const uint32_t w = camera::shade_rgb(seg);
    if (cls == HRL_HIT_GROUND && (index & 1) != 0) {
        const uint32_t k = HRL_CHASE_TILE_SHADE;
        return (((w & 255u) * k) >> 8) | (((((w >> 8) & 255u) * k) >> 8) << 8) | (((((w >> 16) & 255u) * k) >> 8) << 16);
    }
    return w;
}

/* The pixel of ray r.  m0 / m1: bit s set = slot s / 64 + s is walked; pm: bit k set = primitive k is drawn; `robot`: walk the
 * primitives -- true wherever near_robot(r) is (the kernel: wherever it is for some pixel of the wave). */
HRL_DEV void shade_pixel(const ScanSet &S, const float *zl, const float *zh, const PrimSet &P, unsigned long long m0, unsigned long long m1, uint32_t pm, bool robot,
                         const hrl_chase_spec &sp, const View &v, const Ray &r, float *depth, int32_t *seg, uint32_t *rgb) {
    Hit h;
    h.best = inf_(); h.seg = HRL_HIT_NONE;
    if (v.ok) {
        for (unsigned long long m = m0; m; m &= m - 1) try_slot(S, zl, zh, __builtin_ctzll(m), sp.max_range, v.ez, r, h);
        for (unsigned long long m = m1; m; m &= m - 1) try_slot(S, zl, zh, 64 + __builtin_ctzll(m), sp.max_range, v.ez, r, h);
        if (robot)
            for (uint32_t m = pm; m; m &= m - 1) try_prim(P, __builtin_ctz(m), sp.max_range, r, h);
        if ((sp.classes & HRL_CAMERA_GROUND) != 0u && v.ez > v.gz && r.d[2] < 0.f) { /* last: every shape wins a tie */
            const float t = (v.ez - v.gz) / -r.d[2];
            int parity = 0;
            if (sp.tile > 0.f) parity = (tile_index(fma_(t, r.d[0], v.wx), sp.tile) + tile_index(fma_(t, r.d[1], v.wy), sp.tile)) & 1;
            offer(h, true, t, sp.max_range, HRL_HIT_GROUND | (parity << 8) | (HRL_FACE_GROUND << 16));
        }
    }
    *depth = h.seg != HRL_HIT_NONE ? h.best : sp.max_range;
    *seg = h.seg;
    *rgb = shade_rgb(h.seg);
}

/* ------------------------------------------------------------------------------------------------ host side */
inline bool unit_(const float *p) {
    const float n2 = p[0] * p[0] + p[1] * p[1];
    return fabsf(n2 - 1.f) <= HRL_CHASE_UNIT_TOL; /* (false for NaN) */
}
inline std::string validate_spec(const hrl_chase_spec *s) {
    if (!s) return "null chase spec";
    if (s->struct_size != sizeof(hrl_chase_spec)) return "hrl_chase_spec.struct_size is not sizeof(hrl_chase_spec): initialise the record with hrl_chase_default_spec()";
    if (s->width < HRL_CHASE_MIN_WIDTH || s->width > HRL_CHASE_MAX_SIZE || s->width % 16 != 0) return "chase width must be a multiple of 16 within 16..256";
    if (s->height < HRL_CHASE_MIN_HEIGHT || s->height > HRL_CHASE_MAX_SIZE || s->height % 8 != 0) return "chase height must be a multiple of 8 within 8..256";
    if (s->frame != HRL_SCAN_WORLD && s->frame != HRL_SCAN_HEADING) return "unknown chase frame";
    if (s->target_mode != HRL_EYE_GROUND && s->target_mode != HRL_EYE_TORSO) return "unknown chase target_mode";
    if (!(s->target_height >= 0.f) || !(s->target_height <= HRL_CHASE_MAX_TARGET_HEIGHT)) return "chase target_height must be finite and within 0..10";
    if (!unit_(s->yaw)) return "chase yaw must be a (cos, sin) pair: cos^2 + sin^2 within 1e-3 of 1";
    if (!unit_(s->pitch) || !(s->pitch[0] >= 0.f)) return "chase pitch must be a (cos, sin) pair with cos >= 0: cos^2 + sin^2 within 1e-3 of 1, -90..+90 degrees";
    if (!(s->distance >= HRL_CHASE_MIN_DISTANCE) || !(s->distance <= HRL_CHASE_MAX_DISTANCE)) return "chase distance must be within 0.5..50";
    if (!(s->tan_half_h > HRL_CAMERA_MIN_TAN) || !(s->tan_half_h <= HRL_CAMERA_MAX_TAN)) return "chase tan_half_h must be finite and within (1e-3, 1e3]";
    if (!(s->tan_half_v > HRL_CAMERA_MIN_TAN) || !(s->tan_half_v <= HRL_CAMERA_MAX_TAN)) return "chase tan_half_v must be finite and within (1e-3, 1e3]";
    if (!(s->max_range > 0.f) || !(s->max_range <= 3.0e38f)) return "chase max_range must be finite and positive";
    if (s->classes == 0u || (s->classes & ~HRL_CHASE_ALL) != 0u)
        return "chase classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND";
    if (!(s->tile >= 0.f) || !(s->tile <= HRL_CHASE_MAX_TILE)) return "chase tile must be within 0..1e6";
    return "";
}
inline std::string validate_out(const hrl_chase_out *o) {
    if (!o) return "null chase out";
    if (!o->depth && !o->seg && !o->rgb) return "chase out holds no pointer: at least one output must be given";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t frame, hrl_chase_spec *s) {
    hrl_scan_spec r;
    if (!s || scan::default_spec(c, frame, &r) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->width = 64; s->height = 48; s->frame = frame;
    s->target_mode = HRL_EYE_TORSO; s->target_height = 0.f;
    s->yaw[0] = 1.f; s->yaw[1] = 0.f;
    s->pitch[0] = 0.86602540378443864676f; s->pitch[1] = -0.5f; /* -30 degrees */
    s->distance = 3.f;
    s->tan_half_h = 0.57735026918962576451f; s->tan_half_v = 0.43301270189221932338f; /* 60 degrees; * 48 / 64 */
    s->max_range = r.max_range + s->distance;
    s->classes = HRL_CHASE_ALL;
    s->tile = 1.f;
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: the table and the primitives with their lists, then chunks of CHUNK
 * pixels in runs of 64, the chunk's rgb bytes staged and copied out as words. */
inline void chase_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_chase_spec &sp, const hrl_chase_out &out, size_t env) {
    ScanSet S;
    PrimSet P;
    float zl[S_SLOTS], zh[S_SLOTS];
    static thread_local uint32_t stage[CHUNK * 3 / 4];
    uint8_t *bytes = reinterpret_cast<uint8_t *>(stage);
    const hrl_scan_spec ts = table_spec(sp);
    const Frame f = scan::table_frame(st);
    const View v = view_of(c, st, sp);
    for (int slot = 0; slot < S_SLOTS; ++slot) build_slot(S, zl, zh, slot, c, st, items, aux, f, ts, v);
    for (int k = 0; k < PRIMS; ++k) build_prim(P, k, c, st, v, sp.classes);
    unsigned long long m0 = 0, m1 = 0;
    uint32_t pm = 0;
    for (int slot = 0; slot < 64; ++slot) if (scan::kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (scan::kept(S, slot)) m1 |= 1ull << (slot - 64);
    for (int k = 0; k < PRIMS; ++k) if (drawn(P, k)) pm |= 1u << k;
    const float rb2 = robot_bound(P, pm);
    const int W = sp.width, pixels = sp.width * sp.height;
    const float inv_w = 1.f / (float)sp.width, inv_h = 1.f / (float)sp.height;
    const size_t base = env * (size_t)pixels;
    for (int k0 = 0; k0 < pixels; k0 += CHUNK) {
        const int k1 = k0 + CHUNK < pixels ? k0 + CHUNK : pixels;
        for (int k = k0; k < k1; ++k) {
            const int i = k / W, j = k - i * W;
            float d;
            int32_t s;
            uint32_t rgb;
            const Ray r = pixel_ray(sp, v, i, j, inv_w, inv_h);
            shade_pixel(S, zl, zh, P, m0, m1, pm, near_robot(v, rb2, r), sp, v, r, &d, &s, &rgb);
            if (out.depth) out.depth[base + k] = d;
            if (out.seg) out.seg[base + k] = s;
            bytes[3 * (k - k0)] = (uint8_t)rgb; bytes[3 * (k - k0) + 1] = (uint8_t)(rgb >> 8); bytes[3 * (k - k0) + 2] = (uint8_t)(rgb >> 16);
        }
        if (out.rgb) memcpy(out.rgb + 3 * (base + k0), stage, 3 * (size_t)(k1 - k0));
    }
}
/* hrl_chase on host pointers; returns the status and leaves the reason in `why` */
inline int chase_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_chase_spec *sp, const uint8_t *mask, const hrl_chase_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        chase_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp, *out, (size_t)e);
    }
    return HRL_OK;
}
#endif

}  // namespace chase
}  // namespace hrl
