/*
 * cast_core.h -- specification of the batched ray test (include/hrl_cast.h), written once as plain C++: the device kernel
 * (cast_hip.hip) and the host build of the tests (tests/cast_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The answer to one ray of one env is a pure function of (DevCfg, the env's state / items / aux record, hrl_cast_spec, the ray's six
 * numbers, its link):
 *
 *   base_of      O, the heading's forward vector, the ground's z, and whether O is finite: an env without a finite O meets nothing
 *   table        the scanner's 70 slots about the ROBOT, unchanged (scan::build_slot under table_spec: the asked classes and a range no
 *                finite shape lies beyond, so NOTHING IS CULLED), with the camera's z-intervals (camera::z_extent)
 *   primitives   chase::build_prim for a view whose eye is O itself: a PrimSet RELATIVE TO O.  Rows 0..2 (the sphere's centre, the
 *                cylinder's p0, zeros for the cube), 3..5 and 9 (the cylinder's axis A and |A|^2, the cube's X and Z), 11 (r^2) are read;
 *                the eye-relative rows 6..8 and 10 of a cylinder are formed per ray instead
 *   link_frame   the body frame of a link for HRL_CAST_LINK: origin (relative to O) and axes by quat_axes of links::link_world's
 *                quaternion, exactly links::site_out's; once per env and link
 *   make_ray     the ray's ends relative to O in world axes (e, g), D = g - e (HRL_CAST_WORLD: to - from itself), the ends in world
 *                coordinates, |D|^2 and the reciprocals the spans read; `live`: every one of these is finite, the env's O is, and
 *                the link is in range with a finite frame
 *   try_slot     re-centres the slot on the ray's own origin (a half plane: two fma_ on its offset; a rectangle or a disc: two
 *                subtractions), then camera::span_half / camera::span_rect / chase::span_disc and chase::try_slot's 3-D step
 *   try_prim     oc = the primitive's point - e, then chase::try_prim's distance-form discriminants (the cross and triple products)
 *                with oc x A and oc . A formed here
 *   near_robot   the robot's cull: the ray's LINE against chase::robot_bound's sphere about O, from the ray's own origin
 *   cast_ray     scene slots in slot order, robot primitives in order, the ground: 0 < t <= 1, strict < keeps the earlier one; then the
 *                point (a NaN component leaves as the one quiet NaN 0x7FC00000) and, ONCE FOR THE WINNER, the normal
 *
 * Outside only: a prism that holds `from` gives t = 0 (span a = 0 and the height within the z-interval), which `offer` refuses; the
 * sphere's, the cylinder's and the cube's candidates are their ENTRY roots, negative for a ray that starts inside.  No cull: the table's
 * range is 1e18 m, so in_reach keeps every slot with finite numbers and drops those without; near_robot changes no output (a line that
 * misses the bounding sphere misses every primitive in it).
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state, the items or the rays, except sincos_spec's
 * guarded quadrant (link_world).  ray_link is an integer of the caller's: compared with 0 and the number of links before it indexes.
 * Every acceptance test is a comparison that is false for NaN, and a ray that is not `live` is tried against nothing.
 */
#pragma once
#include "../../include/hrl_cast.h"
#include "chase_core.h" /* PrimSet, build_prim, robot_bound, span_disc (and camera_core.h: z_extent, span_half, span_rect; links_core.h: link_world, heading) */

namespace hrl {
namespace cast {

using camera::Span;
using camera::fin_;
using chase::PrimSet;
using render::Frame;
using render::inf_;
using render::max_;
using render::min_;
using scan::ScanSet;

constexpr int S_SLOTS = scan::S_SLOTS; /* 70 */
constexpr int MAX_RAYS = HRL_CAST_MAX_RAYS;
constexpr int PRIMS = chase::PRIMS;
constexpr int LINKS = HRL_LINKS_ANT, LINK_PAD = 16, FRAME_ROWS = 12;
constexpr int ID_GROUND = 255, ID_PRIM0 = 128, ID_NONE = -1; /* who won: a slot 0..69, 128 + a primitive, the ground */
static_assert(S_SLOTS <= ID_PRIM0 && ID_PRIM0 + PRIMS <= ID_GROUND, "the winners' names are distinct");

/* ------------------------------------------------------------------------------------------------ the env */
struct Base { float O[3], fx, fy, gz; bool ok; };

HRL_DEV Base base_of(const DevCfg &c, const float *st) {
    Base b;
    const links::Heading h = links::heading(st);
    b.O[0] = st[HRL_QPOS_OFF]; b.O[1] = st[HRL_QPOS_OFF + 1]; b.O[2] = st[HRL_QPOS_OFF + 2];
    b.fx = h.fx; b.fy = h.fy;
    b.gz = c.ground_z;
    b.ok = fin_(b.O[0]) && fin_(b.O[1]) && fin_(b.O[2]);
    return b;
}

/* what scan::build_slot reads: the class bits and a range beyond every finite shape (in_reach squares it: 1e36) */
HRL_DEV hrl_scan_spec table_spec(const hrl_cast_spec &sp) {
    hrl_scan_spec s = {};
    s.struct_size = sizeof s; s.n_rays = 1; s.frame = HRL_SCAN_WORLD; s.classes = sp.classes & HRL_SCAN_ALL;
    s.max_range = 1e18f;
    return s;
}
HRL_DEV void build_slot(ScanSet &S, float *zl, float *zh, int slot, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frame &f, const hrl_scan_spec &ts) {
    scan::build_slot(S, slot, c, st, items, aux, f, ts);
    camera::z_extent(slot, c, &zl[slot], &zh[slot]);
}
/* the robot relative to O: chase::build_prim from an eye at O */
HRL_DEV void build_prim(PrimSet &P, int k, const DevCfg &c, const float *st, uint32_t classes) {
    chase::View v = {};
    chase::build_prim(P, k, c, st, v, classes);
}

/* The links' body frames, structure of arrays: rows 0..2 the origin relative to O, 3..5 X, 6..8 Y, 9..11 Z; ok: all twelve are finite. */
struct alignas(16) LinkSet {
    float v[FRAME_ROWS][LINK_PAD];
    uint32_t ok[LINK_PAD];
};
HRL_DEV void build_link(LinkSet &L, int link, const DevCfg &c, const float *st) {
    links::Link K;
    links::link_world(c, st, link, K);
    float X[3], Y[3], Z[3];
    quat_axes(K.q[0], K.q[1], K.q[2], K.q[3], X, Y, Z);
    bool fin = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        L.v[q][link] = K.p0[q]; L.v[3 + q][link] = X[q]; L.v[6 + q][link] = Y[q]; L.v[9 + q][link] = Z[q];
        fin = fin && fin_(K.p0[q]) && fin_(X[q]) && fin_(Y[q]) && fin_(Z[q]);
    }
    L.ok[link] = fin ? 1u : 0u;
}

/* ------------------------------------------------------------------------------------------------ rays */
struct Ray {
    float e[3];      /* `from` relative to O, world axes */
    float d[3];      /* to - from, world axes */
    float fw[3], tw[3]; /* the ends in world coordinates */
    float dd, inv_dd, idx, idy;
    bool live;
};

/* in: the ray's six numbers.  link: ray_link's entry (0 where there is none), read under HRL_CAST_LINK only. */
HRL_DEV Ray make_ray(const DevCfg &c, const Base &b, const LinkSet &L, int frame, const float *in, int link) {
    Ray r;
    float e[3], g[3];
    bool ok = b.ok;
    if (frame == HRL_CAST_LINK) {
        const bool valid = link >= 0 && link < links::n_links(c.kind);
        const int l = valid ? link : 0;
        ok = ok && valid && L.ok[l] != 0u;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float o = L.v[q][l], X = L.v[3 + q][l], Y = L.v[6 + q][l], Z = L.v[9 + q][l];
            e[q] = o + fma_(in[2], Z, fma_(in[1], Y, in[0] * X)); /* links::site_out's sum */
            g[q] = o + fma_(in[5], Z, fma_(in[4], Y, in[3] * X));
        }
    } else if (frame == HRL_CAST_HEADING) {
        e[0] = fma_(b.fx, in[0], -(b.fy * in[1])); e[1] = fma_(b.fy, in[0], b.fx * in[1]); e[2] = in[2];
        g[0] = fma_(b.fx, in[3], -(b.fy * in[4])); g[1] = fma_(b.fy, in[3], b.fx * in[4]); g[2] = in[5];
    } else if (frame == HRL_CAST_EGO) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { e[q] = in[q]; g[q] = in[3 + q]; }
    } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) { e[q] = in[q] - b.O[q]; g[q] = in[3 + q] - b.O[q]; }
    }
    const bool world = frame == HRL_CAST_WORLD;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r.e[q] = e[q];
        r.d[q] = links::pick(world, in[3 + q] - in[q], g[q] - e[q]);
        r.fw[q] = links::pick(world, in[q], b.O[q] + e[q]);
        r.tw[q] = links::pick(world, in[3 + q], b.O[q] + g[q]);
        ok = ok && fin_(e[q]) && fin_(r.d[q]) && fin_(r.fw[q]) && fin_(r.tw[q]) && fin_(in[q]) && fin_(in[3 + q]);
    }
    r.dd = dot3(r.d, r.d);
    r.inv_dd = 1.f / r.dd;
    r.idx = 1.f / r.d[0]; r.idy = 1.f / r.d[1];
    r.live = ok && fin_(r.dd) && r.dd > 0.f;
    return r;
}

/* whether the ray's line passes O within the robot's bound (rb2: chase::robot_bound): false for NaN, as every primitive's acceptance is */
HRL_DEV bool near_robot(float rb2, const Ray &r) {
    float x[3];
    cross3(x, r.e, r.d);
    return r.live && dot3(x, x) <= rb2 * r.dd;
}

struct Hit { float best; int32_t seg; int id; };

HRL_DEV void offer(Hit &h, bool got, float t, int32_t seg, int id) {
    if (got && t > 0.f && t <= 1.f && t < h.best) { h.best = t; h.seg = seg; h.id = id; }
}

HRL_DEV void try_slot(const ScanSet &S, const float *zl, const float *zh, int slot, const Ray &r, Hit &h) {
    const int type = (int)(S.meta[slot] & 255u);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    Span sp;
    sp.a = inf_(); sp.b = inf_(); sp.face = HRL_FACE_INSIDE;
    if (type == render::P_HALF) sp = camera::span_half(p0, p1, fma_(p0, r.e[0], fma_(p1, r.e[1], p2)), r.d[0], r.d[1]);
    else if (type == render::P_RECT) sp = camera::span_rect(p0 - r.e[0], p1 - r.e[1], p2, p3, r.idx, r.idy);
    else if (type == render::P_DISC) sp = chase::span_disc(p0 - r.e[0], p1 - r.e[1], p2, r.d[0], r.d[1]);
    const float lo = zl[slot], hi = zh[slot], dz = r.d[2], ez = r.fw[2];
    const float za = fma_(dz, sp.a, ez);
    float t = inf_();
    int32_t face = sp.face;
    bool got = false;
    if (lo <= za && za <= hi) { t = sp.a; got = true; }
    else if (za > hi && dz < 0.f) { t = (hi - ez) / dz; face = HRL_FACE_TOP; got = t <= sp.b; }
    else if (za < lo && dz > 0.f) { t = (lo - ez) / dz; face = HRL_FACE_BOTTOM; got = t <= sp.b; }
    offer(h, got, t, S.code[slot] | (face << 16), slot);
}

HRL_DEV void try_prim(const PrimSet &P, int k, const Ray &r, Hit &h) {
    const uint32_t meta = P.meta[k];
    const int type = (int)(meta & 127u);
    const int32_t code = HRL_HIT_ROBOT | (int32_t)((meta >> 8) << 8);
    const float oc[3] = {P.v[0][k] - r.e[0], P.v[1][k] - r.e[1], P.v[2][k] - r.e[2]};
    if (type == chase::Q_SPHERE) {
        float x[3];
        cross3(x, oc, r.d);
        const float b = dot3(r.d, oc), hh = fma_(P.v[11][k], r.dd, -dot3(x, x));
        const float t = (b - sqrtf(hh)) * r.inv_dd;
        offer(h, hh >= 0.f, t, code | (HRL_FACE_ROUND << 16), ID_PRIM0 + k);
    } else if (type == chase::Q_CYLINDER) {
        const float A[3] = {P.v[3][k], P.v[4][k], P.v[5][k]};
        const float aa = P.v[9][k], r2 = P.v[11][k], ocA = dot3(oc, A);
        float m[3], n[3];
        cross3(n, oc, A);
        cross3(m, r.d, A);
        const float mm = dot3(m, m), w = dot3(oc, m), mn = dot3(m, n);
        const float hh = aa * fma_(r2, mm, -(w * w));
        const float t = (mn - sqrtf(hh)) / mm;
        const float s = fma_(t, dot3(r.d, A), -ocA); /* the hit's place along the axis, times |A| */
        offer(h, hh >= 0.f && s >= 0.f && s <= aa, t, code | (HRL_FACE_ROUND << 16), ID_PRIM0 + k);
    } else if (type == chase::Q_BOX) {
        const float X[3] = {P.v[3][k], P.v[4][k], P.v[5][k]}, Y[3] = {P.v[6][k], P.v[7][k], P.v[8][k]}, Z[3] = {P.v[9][k], P.v[10][k], P.v[11][k]};
        const float dx = dot3(r.d, X), dy = dot3(r.d, Y), dz = dot3(r.d, Z);
        float lox, hix, loy, hiy, loz, hiz;
        scan::slab(dot3(oc, X), render::POINT_HALF, 1.f / dx, &lox, &hix);
        scan::slab(dot3(oc, Y), render::POINT_HALF, 1.f / dy, &loy, &hiy);
        scan::slab(dot3(oc, Z), render::POINT_HALF, 1.f / dz, &loz, &hiz);
        const float tn = max_(max_(lox, loy), loz), tf = min_(min_(hix, hiy), hiz);
        const bool ok = lox <= hix && loy <= hiy && loz <= hiz && tn <= tf;
        const int32_t face = (lox >= loy && lox >= loz) ? HRL_FACE_SIDE_X : (loy >= loz ? HRL_FACE_SIDE_Y : (dz < 0.f ? HRL_FACE_TOP : HRL_FACE_BOTTOM));
        offer(h, ok, tn, code | (face << 16), ID_PRIM0 + k);
    }
}

/* v / |v|; zeros where the length is not a positive finite number */
HRL_DEV void unit3(const float *v, float *o) {
    const float n2 = dot3(v, v);
    const float inv = (n2 > 0.f && n2 <= 3.0e38f) ? 1.f / sqrtf(n2) : 0.f;
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
}

/* the outward normal of the winner (include/hrl_cast.h, by face); hp: the hit relative to O */
HRL_DEV void normal_of(const ScanSet &S, const PrimSet &P, const Ray &r, const Hit &h, float *n) {
    n[0] = 0.f; n[1] = 0.f; n[2] = 0.f;
    const int face = (h.seg >> 16) & 7;
    if (h.id == ID_NONE) return;
    float hp[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) hp[q] = fma_(h.best, r.d[q], r.e[q]);
    if (h.id < ID_PRIM0 || h.id == ID_GROUND) {
        if (face == HRL_FACE_TOP || face == HRL_FACE_GROUND) n[2] = 1.f;
        else if (face == HRL_FACE_BOTTOM) n[2] = -1.f;
        else {
            const int slot = h.id < S_SLOTS ? h.id : 0;
            const int type = (int)(S.meta[slot] & 255u);
            const float p0 = S.p[0][slot], p1 = S.p[1][slot];
            if (type == render::P_HALF) { n[0] = p0; n[1] = p1; }
            else if (type == render::P_DISC) {
                const float v[3] = {hp[0] - p0, hp[1] - p1, 0.f};
                unit3(v, n);
            } else if (face == HRL_FACE_SIDE_X) n[0] = r.d[0] > 0.f ? -1.f : 1.f;
            else n[1] = r.d[1] > 0.f ? -1.f : 1.f;
        }
        return;
    }
    const int k = h.id - ID_PRIM0 < chase::PRIM_PAD ? h.id - ID_PRIM0 : 0;
    const int type = (int)(P.meta[k] & 127u);
    const float q[3] = {hp[0] - P.v[0][k], hp[1] - P.v[1][k], hp[2] - P.v[2][k]};
    if (type == chase::Q_SPHERE) unit3(q, n);
    else if (type == chase::Q_CYLINDER) {
        const float A[3] = {P.v[3][k], P.v[4][k], P.v[5][k]};
        const float s = dot3(q, A) / P.v[9][k];
        const float v[3] = {fma_(-s, A[0], q[0]), fma_(-s, A[1], q[1]), fma_(-s, A[2], q[2])};
        unit3(v, n);
    } else {
        const int row = face == HRL_FACE_SIDE_X ? 3 : (face == HRL_FACE_SIDE_Y ? 6 : 9);
        const float B[3] = {P.v[row][k], P.v[row + 1][k], P.v[row + 2][k]};
        const float sg = dot3(r.d, B) > 0.f ? -1.f : 1.f;
        const float v[3] = {sg * B[0], sg * B[1], sg * B[2]};
        unit3(v, n);
    }
}

struct Answer { float fraction; int32_t seg; float point[3], normal[3]; };

/* The answer to ray r.  m0 / m1: bit s set = slot s / 64 + s is walked; pm: bit k set = primitive k is drawn; `robot`: walk the
 * primitives -- true wherever near_robot(r) is (the kernel: wherever it is for some ray of the wave). */
HRL_DEV void cast_ray(const ScanSet &S, const float *zl, const float *zh, const PrimSet &P, unsigned long long m0, unsigned long long m1, uint32_t pm, bool robot,
                      const hrl_cast_spec &sp, const Base &b, const Ray &r, Answer &a) {
    Hit h;
    h.best = inf_(); h.seg = HRL_HIT_NONE; h.id = ID_NONE;
    if (r.live) {
        for (unsigned long long m = m0; m; m &= m - 1) try_slot(S, zl, zh, __builtin_ctzll(m), r, h);
        for (unsigned long long m = m1; m; m &= m - 1) try_slot(S, zl, zh, 64 + __builtin_ctzll(m), r, h);
        if (robot)
            for (uint32_t m = pm; m; m &= m - 1) try_prim(P, __builtin_ctz(m), r, h);
        if ((sp.classes & HRL_CAMERA_GROUND) != 0u && r.fw[2] > b.gz && r.d[2] < 0.f) /* last: every shape wins a tie */
            offer(h, true, (r.fw[2] - b.gz) / -r.d[2], HRL_HIT_GROUND | (HRL_FACE_GROUND << 16), ID_GROUND);
    }
    const bool met = h.id != ID_NONE;
    a.fraction = met ? h.best : 1.f;
    a.seg = h.seg;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float v = links::pick(met, fma_(h.best, r.d[q], r.fw[q]), r.tw[q]);
        a.point[q] = v != v ? __builtin_nanf("") : v; /* one NaN, 0x7FC00000: which NaN an operation yields differs between processors */
    }
    normal_of(S, P, r, h, a.normal);
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_cast_spec *s) {
    if (!s) return "null cast spec";
    if (s->struct_size != sizeof(hrl_cast_spec)) return "hrl_cast_spec.struct_size is not sizeof(hrl_cast_spec): initialise the record with hrl_cast_default_spec()";
    if (s->n_rays < 1 || s->n_rays > HRL_CAST_MAX_RAYS) return "cast n_rays must be within 1..1024";
    if (s->frame < HRL_CAST_WORLD || s->frame > HRL_CAST_LINK) return "unknown cast frame";
    if (s->classes == 0u || (s->classes & ~HRL_CHASE_ALL) != 0u)
        return "cast classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND";
    if (s->reserved != 0u) return "cast reserved must be 0";
    return "";
}
inline std::string validate_out(const hrl_cast_out *o) {
    if (!o) return "null cast out";
    if (!o->fraction && !o->seg && !o->point && !o->normal) return "cast out holds no pointer: at least one output must be given";
    return "";
}
inline std::string validate_rays(const float *rays) {
    if (!rays) return "null rays";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t frame, hrl_cast_spec *s) {
    if (!s || !c || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN || frame < HRL_CAST_WORLD || frame > HRL_CAST_LINK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->n_rays = 64; s->frame = frame; s->classes = HRL_CHASE_ALL;
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: the table, the primitives and the links' frames with their lists, then
 * the rays in runs of 64 that share the vote on near_robot. */
inline void cast_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_cast_spec &sp, const float *rays, const int32_t *ray_link,
                          const hrl_cast_out &out, size_t env) {
    ScanSet S;
    PrimSet P;
    LinkSet L;
    float zl[S_SLOTS], zh[S_SLOTS];
    const hrl_scan_spec ts = table_spec(sp);
    const Frame f = scan::table_frame(st);
    const Base b = base_of(c, st);
    for (int slot = 0; slot < S_SLOTS; ++slot) build_slot(S, zl, zh, slot, c, st, items, aux, f, ts);
    for (int k = 0; k < PRIMS; ++k) build_prim(P, k, c, st, sp.classes);
    for (int l = 0; l < LINKS; ++l) build_link(L, l, c, st);
    unsigned long long m0 = 0, m1 = 0;
    uint32_t pm = 0;
    for (int slot = 0; slot < 64; ++slot) if (scan::kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (scan::kept(S, slot)) m1 |= 1ull << (slot - 64);
    for (int k = 0; k < PRIMS; ++k) if (chase::drawn(P, k)) pm |= 1u << k;
    const float rb2 = chase::robot_bound(P, pm);
    const int R = sp.n_rays;
    const size_t base = env * (size_t)R;
    for (int k0 = 0; k0 < R; k0 += 64) {
        const int k1 = k0 + 64 < R ? k0 + 64 : R;
        Ray run[64];
        bool robot = false;
        for (int k = k0; k < k1; ++k) {
            const int link = (sp.frame == HRL_CAST_LINK && ray_link) ? ray_link[k] : 0;
            run[k - k0] = make_ray(c, b, L, sp.frame, rays + 6 * (base + k), link);
            robot = robot || near_robot(rb2, run[k - k0]);
        }
        for (int k = k0; k < k1; ++k) {
            Answer a;
            cast_ray(S, zl, zh, P, m0, m1, pm, robot, sp, b, run[k - k0], a);
            if (out.fraction) out.fraction[base + k] = a.fraction;
            if (out.seg) out.seg[base + k] = a.seg;
            for (int q = 0; q < 3; ++q) {
                if (out.point) out.point[3 * (base + k) + q] = a.point[q];
                if (out.normal) out.normal[3 * (base + k) + q] = a.normal[q];
            }
        }
    }
}
/* hrl_cast on host pointers; returns the status and leaves the reason in `why` */
inline int cast_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_cast_spec *sp, const float *rays, const int32_t *ray_link, const uint8_t *mask,
                           const hrl_cast_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_rays(rays);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        cast_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp, rays, ray_link,
                      *out, (size_t)e);
    }
    return HRL_OK;
}
#endif

}  // namespace cast
}  // namespace hrl
