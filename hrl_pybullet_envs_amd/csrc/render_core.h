/*
 * render_core.h -- specification of the batched top-down renderer (include/hrl_render.h), written once as plain C++: the device
 * kernel (render_hip.hip) and the host build of the tests (tests/render_host, HRL_EMU) compile the same functions and produce
 * the same bytes.  fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The image of one env is a pure function of (DevCfg, its state / items / aux record, hrl_view):
 *
 *   view_frame   the camera of the env: centre, right and up (unit, orthogonal) in world coordinates
 *   make_prim    slot s of the env's FIXED table of R_SLOTS primitives, in VIEW coordinates (metres right / up of the centre) with a
 *                padded bounding box; the table's order is the painter's order:
 *                  0..3 outside of lateral plane k | 4 the maze box | 5 the target | 6..69 item i | 70..81 capsule 3 leg + level | 82 torso / cube
 *                a slot the env has no use for is P_NONE (its box is empty)
 *   hits         primitive box against the box of a run of strips: the cull test; a strip is 16 horizontally adjacent pixels, strip
 *                s = row * (W / 16) + column, and 64 consecutive strips are what one wave paints at a time
 *   shade_strip  the 16 pixels of a strip from the bit list of the primitives that survived the cull, walked in slot order: the
 *                last one that covers the pixel centre wins
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state, the items or the view centre.  Every
 * coverage and cull test is a float comparison that is false for NaN, so a shape with a non-finite parameter is not drawn; aux[3]
 * is range-checked as an integer.
 */
#pragma once
#include "../../include/hrl_render.h"
#include "host_cfg.h" /* (includes step_core.h: fma_, sincos_spec, quat_axes, DevCfg) */

namespace hrl {
namespace render {

constexpr int R_PLANE0 = 0, R_BOX = 4, R_TARGET = 5, R_ITEM0 = 6, R_CAPS0 = R_ITEM0 + HRL_MAX_ITEMS, R_BODY = R_CAPS0 + 12, R_SLOTS = 96;
static_assert(R_BODY < R_SLOTS && R_SLOTS <= 128, "two 64-bit lists hold the table");
enum PrimType { P_NONE = 0, P_HALF, P_RECT, P_DISC, P_STADIUM, P_QUAD };

constexpr float TARGET_R = 0.2f;
constexpr float POINT_HALF = 0.35f; /* the half side of the point bot's cube: `he` of point_substep (step_core.h:1570, assets/player_cube.xml:8) */
constexpr float BB_PAD = 1e-3f;     /* bounding boxes are padded by a millimetre: three orders above the rounding of the coverage tests on view coordinates */
constexpr int STRIP = 16;           /* pixels per strip */

HRL_DEV uint32_t rgb_(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
HRL_DEV float inf_() { return __builtin_inff(); }
HRL_DEV float min_(float a, float b) { return a < b ? a : b; }
HRL_DEV float max_(float a, float b) { return a > b ? a : b; }

/* ------------------------------------------------------------------------------------------------ camera */
struct Frame { float cx, cy, rx, ry, ux, uy; };

HRL_DEV Frame view_frame(const hrl_view &v, const float *st) {
    Frame f;
    f.cx = v.centre[0]; f.cy = v.centre[1]; f.rx = 1.f; f.ry = 0.f; f.ux = 0.f; f.uy = 1.f;
    if (v.mode != HRL_VIEW_WORLD) { f.cx = st[HRL_QPOS_OFF]; f.cy = st[HRL_QPOS_OFF + 1]; }
    if (v.mode == HRL_VIEW_EGO_HEADING) { /* up = the normalised ground projection of the torso's X axis; no inverse trigonometry */
        float X[3], Y[3], Z[3];
        quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
        const float n2 = fma_(X[0], X[0], X[1] * X[1]);
        if (n2 >= 1e-12f && n2 <= 3.0e38f) { /* (false for NaN; an overflowed norm is infinite) */
            const float inv = 1.f / sqrtf(n2);
            f.ux = X[0] * inv; f.uy = X[1] * inv; f.rx = f.uy; f.ry = -f.ux;
        }
    }
    return f;
}
HRL_DEV void to_view(const Frame &f, float x, float y, float *u, float *v) {
    const float dx = x - f.cx, dy = y - f.cy;
    *u = fma_(dx, f.rx, dy * f.ry);
    *v = fma_(dx, f.ux, dy * f.uy);
}
/* pixel centres: u of column j, v of row i (include/hrl_render.h); inv_w = 1.f / (float)W.  The numerators are integers: exact. */
HRL_DEV float pix_u(int j, int W, float inv_w, float he) { return ((float)(2 * j + 1 - W) * inv_w) * he; }
HRL_DEV float pix_v(int i, int H, float inv_w, float he) { return ((float)(H - (2 * i + 1)) * inv_w) * he; }

/* ------------------------------------------------------------------------------------------------ primitives */
struct Prim {
    int type;
    uint32_t rgb;
    float p[8];  /* P_HALF: nu, nv, offset (outside where nu u + nv v + offset < 0) | P_RECT: centre u, v, world half sizes x, y | P_DISC: centre, r^2
                    P_STADIUM: a, b, r^2, |b - a|^2 | P_QUAD: four corners */
    float bb[4]; /* u min, u max, v min, v max */
};

/* ph / pa / tip of leg l relative to the torso origin: the operations of phase_kin_ankle<POS_ONLY> (step_core.h:407-429), restated */
HRL_DEV void leg_points(const DevCfg &c, const float *q, int l, float *ph, float *pa, float *tip) {
    const float is2 = 0.70710678118654752440f;
    float X[3], Y[3], Z[3];
    quat_axes(q[3], q[4], q[5], q[6], X, Y, Z);
    float ch, sh, ca, sa;
    sincos_spec(q[7 + 2 * l], &sh, &ch);
    sincos_spec(q[8 + 2 * l], &sa, &ca);
    const float sx = (l == 0 || l == 3) ? 1.f : -1.f, sy = (l < 2) ? 1.f : -1.f, sg = (l == 1 || l == 2) ? 1.f : -1.f;
    const float e1x = fma_(sx, ch, -(sy * sh)) * is2, e1y = fma_(sx, sh, sy * ch) * is2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float e1 = fma_(e1y, Y[k], e1x * X[k]);
        const float e2 = fma_(sg * sa, Z[k], ca * e1);
        ph[k] = 0.2f * fma_(sy, Y[k], sx * X[k]);
        pa[k] = fma_(c.L1, e1, ph[k]);
        tip[k] = fma_(c.L2, e2, pa[k]);
    }
}

HRL_DEV void prim_none(Prim &P) {
    P.type = P_NONE; P.rgb = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) P.p[k] = 0.f;
    P.bb[0] = inf_(); P.bb[1] = -inf_(); P.bb[2] = inf_(); P.bb[3] = -inf_();
}
HRL_DEV void prim_disc(Prim &P, const Frame &f, float x, float y, float r, uint32_t rgb) {
    P.type = P_DISC; P.rgb = rgb;
    to_view(f, x, y, &P.p[0], &P.p[1]);
    P.p[2] = r * r;
    const float e = r + BB_PAD;
    P.bb[0] = P.p[0] - e; P.bb[1] = P.p[0] + e; P.bb[2] = P.p[1] - e; P.bb[3] = P.p[1] + e;
}
/* a rectangle with world-aligned sides, half sizes hx, hy */
HRL_DEV void prim_rect(Prim &P, const Frame &f, float x, float y, float hx, float hy, uint32_t rgb) {
    P.type = P_RECT; P.rgb = rgb;
    to_view(f, x, y, &P.p[0], &P.p[1]);
    P.p[2] = hx; P.p[3] = hy;
    const float eu = fma_(fabsf(f.rx), hx, fabsf(f.ry) * hy) + BB_PAD, ev = fma_(fabsf(f.ux), hx, fabsf(f.uy) * hy) + BB_PAD;
    P.bb[0] = P.p[0] - eu; P.bb[1] = P.p[0] + eu; P.bb[2] = P.p[1] - ev; P.bb[3] = P.p[1] + ev;
}
HRL_DEV void prim_stadium(Prim &P, const Frame &f, float ax, float ay, float bx, float by, float r, uint32_t rgb) {
    P.type = P_STADIUM; P.rgb = rgb;
    to_view(f, ax, ay, &P.p[0], &P.p[1]);
    to_view(f, bx, by, &P.p[2], &P.p[3]);
    const float du = P.p[2] - P.p[0], dv = P.p[3] - P.p[1];
    P.p[4] = r * r; P.p[5] = fma_(du, du, dv * dv);
    const float e = r + BB_PAD;
    P.bb[0] = min_(P.p[0], P.p[2]) - e; P.bb[1] = max_(P.p[0], P.p[2]) + e; P.bb[2] = min_(P.p[1], P.p[3]) - e; P.bb[3] = max_(P.p[1], P.p[3]) + e;
}

/* Slot `slot` of the env's table.  st: the packed state record; items: the env's items record or nullptr; aux: its four counters. */
HRL_DEV void make_prim(Prim &P, int slot, const DevCfg &c, const float *st, const float *items, const int32_t *aux, const Frame &f) {
    prim_none(P);
    const bool maze = c.kind == HRL_ANT_MAZE || c.kind == HRL_ANT_MAZE_MJ, gather = c.kind == HRL_ANT_GATHER || c.kind == HRL_POINT_GATHER;
    if (slot < R_BOX) { /* the outer side of lateral plane `slot`: n . world - d < 0, world = centre + u right + v up */
        if (slot < c.n_planes) {
            const float nx = c.plane_n[slot][0], ny = c.plane_n[slot][1];
            P.type = P_HALF; P.rgb = rgb_(HRL_RGB_WALL);
            P.p[0] = fma_(nx, f.rx, ny * f.ry); P.p[1] = fma_(nx, f.ux, ny * f.uy); P.p[2] = fma_(nx, f.cx, ny * f.cy) - c.plane_d[slot];
            P.bb[0] = -inf_(); P.bb[1] = inf_(); P.bb[2] = -inf_(); P.bb[3] = inf_();
        }
    } else if (slot == R_BOX) {
        if (maze && c.n_boxes > 0)
            prim_rect(P, f, 0.5f * (c.box_lo[0] + c.box_hi[0]), 0.5f * (c.box_lo[1] + c.box_hi[1]), 0.5f * (c.box_hi[0] - c.box_lo[0]), 0.5f * (c.box_hi[1] - c.box_lo[1]),
                      rgb_(HRL_RGB_BOX));
    } else if (slot == R_TARGET) {
        if (maze) {
            const int t = aux[3];
            if (t >= 0 && t < c.n_targets && t < HRL_MAX_TARGETS) prim_disc(P, f, c.targets[t][0], c.targets[t][1], TARGET_R, rgb_(HRL_RGB_TARGET));
        } else if (c.kind == HRL_ANT_FLAGRUN && items) {
            prim_disc(P, f, items[HRL_FLAG_GOAL_OFF], items[HRL_FLAG_GOAL_OFF + 1], TARGET_R, rgb_(HRL_RGB_TARGET));
        }
    } else if (slot < R_CAPS0) {
        const int i = slot - R_ITEM0;
        if (gather && items && i < c.n_food + c.n_poison && 2 * i + 1 < c.items_stride)
            prim_rect(P, f, items[2 * i], items[2 * i + 1], ITEM_HALF, ITEM_HALF, i < c.n_food ? rgb_(HRL_RGB_FOOD) : rgb_(HRL_RGB_POISON));
    } else if (slot < R_BODY) {
        if (c.kind != HRL_POINT_GATHER) {
            const int l = (slot - R_CAPS0) / 3, level = (slot - R_CAPS0) - 3 * l;
            float ph[3], pa[3], tip[3];
            leg_points(c, st, l, ph, pa, tip);
            const float ox = st[0], oy = st[1];
            if (level == 0) prim_stadium(P, f, ox, oy, ox + ph[0], oy + ph[1], c.r_caps, rgb_(HRL_RGB_LEG0));
            if (level == 1) prim_stadium(P, f, ox + ph[0], oy + ph[1], ox + pa[0], oy + pa[1], c.r_caps, rgb_(HRL_RGB_LEG1));
            if (level == 2) prim_stadium(P, f, ox + pa[0], oy + pa[1], ox + tip[0], oy + tip[1], c.r_caps, rgb_(HRL_RGB_LEG2));
        }
    } else if (slot == R_BODY) {
        if (c.kind != HRL_POINT_GATHER) {
            prim_disc(P, f, st[0], st[1], c.r_torso, rgb_(HRL_RGB_TORSO));
        } else { /* the ground projection of the corners (-,-) (+,-) (+,+) (-,+) of the cube's mid-plane square */
            float X[3], Y[3], Z[3];
            quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
            P.type = P_QUAD; P.rgb = rgb_(HRL_RGB_TORSO);
            float lo_u = inf_(), hi_u = -inf_(), lo_v = inf_(), hi_v = -inf_();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float sx = (k == 1 || k == 2) ? POINT_HALF : -POINT_HALF, sy = (k >= 2) ? POINT_HALF : -POINT_HALF;
                const float wx = st[0] + fma_(sy, Y[0], sx * X[0]), wy = st[1] + fma_(sy, Y[1], sx * X[1]);
                to_view(f, wx, wy, &P.p[2 * k], &P.p[2 * k + 1]);
                lo_u = min_(lo_u, P.p[2 * k]); hi_u = max_(hi_u, P.p[2 * k]); lo_v = min_(lo_v, P.p[2 * k + 1]); hi_v = max_(hi_v, P.p[2 * k + 1]);
            }
            /* (a NaN corner leaves a box of the others, or none: the cull only has to keep what the coverage test can accept, and that accepts nothing then) */
            P.bb[0] = lo_u - BB_PAD; P.bb[1] = hi_u + BB_PAD; P.bb[2] = lo_v - BB_PAD; P.bb[3] = hi_v + BB_PAD;
        }
    }
}

/* ------------------------------------------------------------------------------------------------ the table, as the painters read it */
struct alignas(16) PrimSet { /* 5.1 KB; on the device in LDS.  Structure of arrays: the cull reads it lane = slot, the painters read one slot wave-wide */
    float p[8][R_SLOTS];
    float bb[4][R_SLOTS];
    uint32_t meta[R_SLOTS]; /* type | rgb << 8 */
    float rot[4];           /* rx, ry, ux, uy */
};
HRL_DEV void store_prim(PrimSet &S, int slot, const Prim &P) {
#pragma unroll
    for (int k = 0; k < 8; ++k) S.p[k][slot] = P.p[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) S.bb[k][slot] = P.bb[k];
    S.meta[slot] = (uint32_t)P.type | (P.rgb << 8);
}
HRL_DEV void store_frame(PrimSet &S, const Frame &f) { S.rot[0] = f.rx; S.rot[1] = f.ry; S.rot[2] = f.ux; S.rot[3] = f.uy; }

/* the box of the pixel centres of strips s0..s1 (inclusive) */
struct TileBox { float u0, u1, v0, v1; };
HRL_DEV TileBox strips_box(int s0, int s1, int W, int H, float inv_w, float he) {
    const int spr = W / STRIP, r0 = s0 / spr, r1 = s1 / spr;
    const int c0 = r0 == r1 ? s0 - r0 * spr : 0, c1 = r0 == r1 ? s1 - r1 * spr : spr - 1;
    TileBox t;
    t.u0 = pix_u(STRIP * c0, W, inv_w, he); t.u1 = pix_u(STRIP * c1 + STRIP - 1, W, inv_w, he);
    t.v1 = pix_v(r0, H, inv_w, he); t.v0 = pix_v(r1, H, inv_w, he);
    return t;
}
HRL_DEV bool hits(const PrimSet &S, int slot, const TileBox &t) {
    return S.bb[0][slot] <= t.u1 && S.bb[1][slot] >= t.u0 && S.bb[2][slot] <= t.v1 && S.bb[3][slot] >= t.v0;
}

/* coverage of the point (u, v) */
HRL_DEV bool cov_half(const float *p, float u, float v) { return fma_(p[0], u, fma_(p[1], v, p[2])) < 0.f; }
HRL_DEV bool cov_rect(const float *p, const float *rot, float u, float v) {
    const float du = u - p[0], dv = v - p[1];
    const float lx = fma_(du, rot[0], dv * rot[2]), ly = fma_(du, rot[1], dv * rot[3]); /* the offset along world x, y */
    return fabsf(lx) <= p[2] && fabsf(ly) <= p[3];
}
HRL_DEV bool cov_disc(const float *p, float u, float v) {
    const float du = u - p[0], dv = v - p[1];
    return fma_(du, du, dv * dv) <= p[2];
}
/* within r of the segment a b, without a division: before a, the disc at a; past b, the disc at b; else the distance to the line */
HRL_DEV bool cov_stadium(const float *p, float u, float v) {
    const float dx = p[2] - p[0], dy = p[3] - p[1], ex = u - p[0], ey = v - p[1];
    const float t = fma_(ex, dx, ey * dy);
    const float fx = u - p[2], fy = v - p[3];
    const float cr = fma_(ex, dy, -(ey * dx));
    const bool at_a = fma_(ex, ex, ey * ey) <= p[4], at_b = fma_(fx, fx, fy * fy) <= p[4], mid = cr * cr <= p[4] * p[5];
    return t <= 0.f ? at_a : (t >= p[5] ? at_b : mid);
}
/* the four edge functions have one sign; either orientation counts */
HRL_DEV bool cov_quad(const float *p, float u, float v) {
    bool pos = true, neg = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = (k + 1) & 3;
        const float e = fma_(p[2 * n] - p[2 * k], v - p[2 * k + 1], -((p[2 * n + 1] - p[2 * k + 1]) * (u - p[2 * k])));
        pos = pos && e >= 0.f; neg = neg && e <= 0.f;
    }
    return pos || neg;
}

/* paints primitive `slot` over the strip's 16 colours */
HRL_DEV void shade_prim(const PrimSet &S, int slot, const float *u, float v, uint32_t *c) {
    const uint32_t meta = S.meta[slot], rgb = meta >> 8;
    const int type = (int)(meta & 255u);
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = S.p[k][slot];
    if (type == P_HALF) {
#pragma unroll
        for (int x = 0; x < STRIP; ++x) c[x] = cov_half(p, u[x], v) ? rgb : c[x];
    } else if (type == P_RECT) {
        const float rot[4] = {S.rot[0], S.rot[1], S.rot[2], S.rot[3]};
#pragma unroll
        for (int x = 0; x < STRIP; ++x) c[x] = cov_rect(p, rot, u[x], v) ? rgb : c[x];
    } else if (type == P_DISC) {
#pragma unroll
        for (int x = 0; x < STRIP; ++x) c[x] = cov_disc(p, u[x], v) ? rgb : c[x];
    } else if (type == P_STADIUM) {
#pragma unroll
        for (int x = 0; x < STRIP; ++x) c[x] = cov_stadium(p, u[x], v) ? rgb : c[x];
    } else if (type == P_QUAD) {
#pragma unroll
        for (int x = 0; x < STRIP; ++x) c[x] = cov_quad(p, u[x], v) ? rgb : c[x];
    }
}

/* Strip s of the image: its 48 bytes as twelve little-endian words (R0 G0 B0 R1 ...).  m0 / m1: bit i set = slot i / 64 + i is on the list. */
HRL_DEV void shade_strip(const PrimSet &S, unsigned long long m0, unsigned long long m1, int s, int W, int H, float inv_w, float he, uint32_t *out) {
    const int spr = W / STRIP, row = s / spr, col = s - row * spr;
    const float v = pix_v(row, H, inv_w, he);
    float u[STRIP];
    uint32_t c[STRIP];
#pragma unroll
    for (int x = 0; x < STRIP; ++x) { u[x] = pix_u(STRIP * col + x, W, inv_w, he); c[x] = rgb_(HRL_RGB_GROUND); }
    for (unsigned long long m = m0; m; m &= m - 1) shade_prim(S, __builtin_ctzll(m), u, v, c);
    for (unsigned long long m = m1; m; m &= m - 1) shade_prim(S, 64 + __builtin_ctzll(m), u, v, c);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t a = c[4 * g], b = c[4 * g + 1], d = c[4 * g + 2], e = c[4 * g + 3];
        out[3 * g] = a | (b << 24); out[3 * g + 1] = (b >> 8) | (d << 16); out[3 * g + 2] = (d >> 16) | (e << 8);
    }
}
/* byte offset of strip s of env `env` in rgb: a multiple of 48 */
HRL_DEV size_t strip_offset(int env, int s, int W, int H) { return ((size_t)env * (size_t)(W / STRIP * H) + (size_t)s) * (size_t)(3 * STRIP); }

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_view(const hrl_view *v) {
    if (!v) return "null view";
    if (v->struct_size != sizeof(hrl_view)) return "hrl_view.struct_size is not sizeof(hrl_view): initialise the record with hrl_render_default_view()";
    if (v->width < HRL_VIEW_MIN_SIZE || v->width > HRL_VIEW_MAX_SIZE || v->width % STRIP != 0) return "view width must be a multiple of 16 within 16..256";
    if (v->height < HRL_VIEW_MIN_SIZE || v->height > HRL_VIEW_MAX_SIZE || v->height % STRIP != 0) return "view height must be a multiple of 16 within 16..256";
    if (v->mode != HRL_VIEW_WORLD && v->mode != HRL_VIEW_EGO && v->mode != HRL_VIEW_EGO_HEADING) return "unknown view mode";
    if (!(v->half_extent > 0.f) || !(v->half_extent <= 3.0e38f)) return "view half_extent must be finite and positive";
    return "";
}

inline int default_view(const hrl_config *c, int32_t mode, hrl_view *v) {
    if (!c || !v || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN) return HRL_ERR_BAD_ARG;
    if (mode != HRL_VIEW_WORLD && mode != HRL_VIEW_EGO && mode != HRL_VIEW_EGO_HEADING) return HRL_ERR_BAD_ARG;
    memset(v, 0, sizeof(*v));
    v->struct_size = sizeof(*v); v->width = 64; v->height = 64; v->mode = mode;
    float he = 3.f;
    if (mode == HRL_VIEW_WORLD) {
        switch (c->env_kind) {
            case HRL_ANT_GATHER: case HRL_POINT_GATHER: he = 0.5f * (c->world_size[0] > c->world_size[1] ? c->world_size[0] : c->world_size[1]); break;
            case HRL_ANT_MAZE: case HRL_ANT_MAZE_MJ: he = 9.f; break; /* maze_scene.py:10: half extents 5 x 9 */
            case HRL_ANT_FLAGRUN: he = 0.5f * (c->flag_size + 2.f); break; /* ant_flagrun_env.py:59-61 */
            default: he = 6.f;
        }
    }
    v->half_extent = he;
    return HRL_OK;
}

#ifdef HRL_EMU
/* The whole launch on the host, partitioned as the kernel partitions it: per env the table, then runs of 64 strips with their own lists. */
inline void render_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_view &view, int env, uint8_t *rgb) {
    PrimSet S;
    const Frame f = view_frame(view, st);
    store_frame(S, f);
    for (int slot = 0; slot < R_SLOTS; ++slot) { Prim P; make_prim(P, slot, c, st, items, aux, f); store_prim(S, slot, P); }
    const int W = view.width, H = view.height, total = W / STRIP * H;
    const float inv_w = 1.f / (float)W, he = view.half_extent;
    for (int s0 = 0; s0 < total; s0 += 64) {
        const int s1 = s0 + 63 < total ? s0 + 63 : total - 1;
        const TileBox t = strips_box(s0, s1, W, H, inv_w, he);
        unsigned long long m0 = 0, m1 = 0;
        for (int slot = 0; slot < 64; ++slot) if (hits(S, slot, t)) m0 |= 1ull << slot;
        for (int slot = 64; slot < R_SLOTS; ++slot) if (hits(S, slot, t)) m1 |= 1ull << (slot - 64);
        for (int s = s0; s <= s1; ++s) {
            uint32_t w[12];
            shade_strip(S, m0, m1, s, W, H, inv_w, he, w);
            memcpy(rgb + strip_offset(env, s, W, H), w, sizeof w);
        }
    }
}
/* hrl_render on host pointers; returns the status and leaves the reason in `why` */
inline int render_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_view *view, const uint8_t *mask, uint8_t *rgb, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_view(view);
    if (why.empty() && (!b || !b->state || !b->aux || !rgb)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        render_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *view, e, rgb);
    }
    return HRL_OK;
}
#endif

}  // namespace render
}  // namespace hrl
