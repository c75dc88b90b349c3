/*
 * camera_core.h -- specification of the batched first-person camera (include/hrl_camera.h), written once as plain C++: the device kernel
 * (camera_hip.hip) and the host build of the tests (tests/camera_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The image of one env is a pure function of (DevCfg, its state / items / aux record, hrl_camera_spec):
 *
 *   table       the scanner's 70 slots, unchanged (scan_core.h: table_frame, forward, build_slot under table_spec: classes &
 *               HRL_SCAN_ALL and max_range -- the cull by max_range stays valid because a candidate is accepted on its HORIZONTAL range)
 *   z_extent    the z-interval [zl, zh] of a slot, a function of the slot and DevCfg alone: every shape is a vertical prism
 *   span_*      one function per primitive type: the interval [t_in, t_out] of the ray from the table's origin through the ground-plan
 *               shape and the face it is entered by.  t_in is computed BY THE SAME OPERATIONS as scan::isect_half / isect_rect /
 *               isect_disc and equals them bit for bit (+inf = no span)
 *   pixel_ray   column j and row i: the unit ground-plan direction d, cj = 1 / sqrt(1 + u^2) and m = s cj, the rise per metre of
 *               horizontal range.  The camera yaws with `forward` and neither pitches nor rolls, so a column shares one ground-plan ray
 *   candidate   the 3-D step: z(t_in) = fma(m, t_in, ez) against [zl, zh] picks the side face, the top or the bottom: one fma, one
 *               division at most and comparisons
 *   shade_pixel walks the bit list of the surviving slots in slot order, then the ground: a candidate counts if t <= max_range, the
 *               smallest t wins with a strict <, so an equal t stays with the lower slot and every shape wins a tie with the ground
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items.  Every acceptance test is a
 * float comparison that is false for NaN, so a shape with a non-finite parameter is not seen; an env whose x, y or eye z is not finite
 * sees nothing at all.
 */
#pragma once
#include "../../include/hrl_camera.h"
#include "scan_core.h" /* ScanSet, table_frame, forward, build_slot, kept, slab (and through it render_core.h, step_core.h: fma_, DevCfg, ITEM_Z) */

namespace hrl {
namespace camera {

using render::Frame;
using render::inf_;
using render::max_;
using render::min_;
using scan::ScanSet;

constexpr int S_SLOTS = scan::S_SLOTS; /* 70 */
constexpr int MAX_SIZE = HRL_CAMERA_MAX_SIZE, MAX_PIXELS = MAX_SIZE * MAX_SIZE;
constexpr int CHUNK = 1024; /* pixels whose rgb bytes are staged at a time (camera_hip.hip): 3 KB, a multiple of 4 bytes; images are multiples of 128 pixels */
constexpr float WALL_TOP = 2.5f, POST_TOP = 1.0f;

HRL_DEV bool fin_(float v) { return fabsf(v) <= 3.0e38f; }

/* what scan::build_slot reads: the class bits and the range of the cull.  It may carry no class bit at all (the ground alone): build_slot
 * only tests bits, and scan::validate_spec is not run on it. */
HRL_DEV hrl_scan_spec table_spec(const hrl_camera_spec &sp) {
    hrl_scan_spec s = {};
    s.struct_size = sizeof s; s.n_rays = 1; s.frame = sp.frame; s.max_range = sp.max_range; s.classes = sp.classes & HRL_SCAN_ALL;
    return s;
}

/* the z-interval of slot `slot`: walls | the box | the target post | item cubes */
HRL_DEV void z_extent(int slot, const DevCfg &c, float *zl, float *zh) {
    if (slot < render::R_BOX) { *zl = c.ground_z; *zh = c.ground_z + WALL_TOP; }
    else if (slot == render::R_BOX) { *zl = c.box_lo[2]; *zh = c.box_hi[2]; }
    else if (slot == render::R_TARGET) { *zl = c.ground_z; *zh = c.ground_z + POST_TOP; }
    else { *zl = ITEM_Z - ITEM_HALF; *zh = ITEM_Z + ITEM_HALF; }
}

/* ------------------------------------------------------------------------------------------------ spans: origin (0, 0), unit direction (dx, dy) */
struct Span { float a, b; int32_t face; }; /* [t_in, t_out]; a = +inf: none */

/* scan::isect_half, and the ray never leaves the half plane again */
HRL_DEV Span span_half(float nx, float ny, float off, float dx, float dy) {
    const float den = fma_(nx, dx, ny * dy);
    const float t = off / -den;
    Span s;
    s.a = off < 0.f ? 0.f : (den < 0.f ? t : inf_());
    s.b = inf_();
    s.face = s.a == 0.f ? HRL_FACE_INSIDE : (fabsf(nx) >= fabsf(ny) ? HRL_FACE_SIDE_X : HRL_FACE_SIDE_Y);
    return s;
}
/* scan::isect_rect; the exit is the slab test's far end, the face that of the slab entered last */
HRL_DEV Span span_rect(float cx, float cy, float hx, float hy, float idx, float idy) {
    float lox, hix, loy, hiy;
    scan::slab(cx, hx, idx, &lox, &hix);
    scan::slab(cy, hy, idy, &loy, &hiy);
    const float tn = max_(lox, loy), tf = min_(hix, hiy);
    const bool ok = lox <= hix && loy <= hiy && tn <= tf && tf >= 0.f;
    Span s;
    s.a = ok ? max_(tn, 0.f) : inf_();
    s.b = tf;
    s.face = s.a == 0.f ? HRL_FACE_INSIDE : (lox >= loy ? HRL_FACE_SIDE_X : HRL_FACE_SIDE_Y);
    return s;
}
/* scan::isect_disc; the exit is the far root */
HRL_DEV Span span_disc(float cx, float cy, float r2, float dx, float dy) {
    const float cc = fma_(cx, cx, cy * cy), b = fma_(cx, dx, cy * dy), e = fma_(cx, dy, -(cy * dx));
    const float h = fma_(-e, e, r2);
    const float root = sqrtf(h);
    Span s;
    s.a = cc <= r2 ? 0.f : ((h >= 0.f && b > 0.f) ? b - root : inf_());
    s.b = b + root; /* (NaN when h < 0: no top or bottom is accepted then) */
    s.face = s.a == 0.f ? HRL_FACE_INSIDE : HRL_FACE_ROUND;
    return s;
}

/* ------------------------------------------------------------------------------------------------ the eye and the rays */
struct Eye { float ez, gz; bool ok; }; /* eye z, the ground's z, and whether the env sees at all */

HRL_DEV Eye eye_of(const DevCfg &c, const float *st, const hrl_camera_spec &sp) {
    Eye e;
    e.gz = c.ground_z;
    e.ez = (sp.eye_mode == HRL_EYE_TORSO ? st[HRL_QPOS_OFF + 2] : c.ground_z) + sp.eye_height;
    e.ok = fin_(st[HRL_QPOS_OFF]) && fin_(st[HRL_QPOS_OFF + 1]) && fin_(e.ez);
    return e;
}

/* u of column j, s of row i (include/hrl_camera.h): the numerators are integers, exact */
HRL_DEV float col_u(int j, int W, float inv_w, float tan_h) { return ((float)(W - (2 * j + 1)) * inv_w) * tan_h; }
HRL_DEV float row_s(int i, int H, float inv_h, float tan_v) { return ((float)(H - (2 * i + 1)) * inv_h) * tan_v; }

struct Ray { float dx, dy, idx, idy, cj, m; };

HRL_DEV Ray pixel_ray(const hrl_camera_spec &sp, float fx, float fy, int i, int j, float inv_w, float inv_h) {
    const float u = col_u(j, sp.width, inv_w, sp.tan_half_h), s = row_s(i, sp.height, inv_h, sp.tan_half_v);
    const float lx = -fy, ly = fx;
    Ray r;
    r.cj = 1.f / sqrtf(fma_(u, u, 1.f));
    r.dx = fma_(u, lx, fx) * r.cj; r.dy = fma_(u, ly, fy) * r.cj;
    r.idx = 1.f / r.dx; r.idy = 1.f / r.dy;
    r.m = s * r.cj;
    return r;
}

struct Hit { float best; int32_t seg; };

/* the span of slot `slot` along the ray, and from it the candidate */
HRL_DEV void try_slot(const ScanSet &S, const float *zl, const float *zh, int slot, float max_range, float ez, const Ray &r, Hit &h) {
    const int type = (int)(S.meta[slot] & 255u);
    const float p0 = S.p[0][slot], p1 = S.p[1][slot], p2 = S.p[2][slot], p3 = S.p[3][slot];
    Span sp;
    sp.a = inf_(); sp.b = inf_(); sp.face = HRL_FACE_INSIDE;
    if (type == render::P_HALF) sp = span_half(p0, p1, p2, r.dx, r.dy);
    else if (type == render::P_RECT) sp = span_rect(p0, p1, p2, p3, r.idx, r.idy);
    else if (type == render::P_DISC) sp = span_disc(p0, p1, p2, r.dx, r.dy);
    const float lo = zl[slot], hi = zh[slot];
    const float za = fma_(r.m, sp.a, ez);
    float t = inf_();
    int32_t face = sp.face;
    bool got = false;
    if (lo <= za && za <= hi) { t = sp.a; got = true; }
    else if (za > hi && r.m < 0.f) { t = (hi - ez) / r.m; face = HRL_FACE_TOP; got = t <= sp.b; }
    else if (za < lo && r.m > 0.f) { t = (lo - ez) / r.m; face = HRL_FACE_BOTTOM; got = t <= sp.b; }
    if (got && t <= max_range && t < h.best) { h.best = t; h.seg = S.code[slot] | (face << 16); }
}

/* class colour * shade[face] >> 8 per channel, as 0x00BBGGRR.  The tables are packed into constants and picked by shifts and selects:
 * integer arithmetic only, and no array is indexed at run time. */
HRL_DEV uint32_t shade_rgb(int32_t seg) {
    const int cls = seg & 255, face = (seg >> 16) & 7;
    if (cls == HRL_HIT_NONE) return render::rgb_(HRL_RGB_SKY);
    const uint32_t base = cls == HRL_HIT_WALL ? render::rgb_(HRL_RGB_WALL)
                        : cls == HRL_HIT_BOX ? render::rgb_(HRL_RGB_BOX)
                        : cls == HRL_HIT_FOOD ? render::rgb_(HRL_RGB_FOOD)
                        : cls == HRL_HIT_POISON ? render::rgb_(HRL_RGB_POISON)
                        : cls == HRL_HIT_TARGET ? render::rgb_(HRL_RGB_TARGET)
                        : render::rgb_(HRL_RGB_GROUND);
    /* {128, 224, 176, 200, 256, 96, 256} by face, nine bits each */
    constexpr unsigned long long SHADES = 128ull | (224ull << 9) | (176ull << 18) | (200ull << 27) | (256ull << 36) | (96ull << 45) | (256ull << 54);
    const uint32_t k = (uint32_t)((SHADES >> (9 * (face < 7 ? face : 0))) & 511ull);
    const uint32_t r = ((base & 255u) * k) >> 8, g = (((base >> 8) & 255u) * k) >> 8, b = (((base >> 16) & 255u) * k) >> 8;
    return r | (g << 8) | (b << 16);
}

/* Pixel (i, j) of the env.  m0 / m1: bit s set = slot s / 64 + s survived the cull.  zl / zh: the slots' z-intervals. */
HRL_DEV void shade_pixel(const ScanSet &S, const float *zl, const float *zh, unsigned long long m0, unsigned long long m1, const hrl_camera_spec &sp, const Eye &eye, int i, int j,
                         float inv_w, float inv_h, float *depth, int32_t *seg, uint32_t *rgb) {
    const Ray r = pixel_ray(sp, S.fwd[0], S.fwd[1], i, j, inv_w, inv_h);
    Hit h;
    h.best = inf_(); h.seg = HRL_HIT_NONE;
    if (eye.ok) {
        for (unsigned long long m = m0; m; m &= m - 1) try_slot(S, zl, zh, __builtin_ctzll(m), sp.max_range, eye.ez, r, h);
        for (unsigned long long m = m1; m; m &= m - 1) try_slot(S, zl, zh, 64 + __builtin_ctzll(m), sp.max_range, eye.ez, r, h);
        if ((sp.classes & HRL_CAMERA_GROUND) != 0u) { /* last: every shape wins a tie */
            float t = inf_();
            bool got = false;
            if (eye.ez <= eye.gz) { t = 0.f; got = true; }
            else if (r.m < 0.f && eye.ez > eye.gz) { t = (eye.ez - eye.gz) / -r.m; got = true; }
            if (got && t <= sp.max_range && t < h.best) { h.best = t; h.seg = HRL_HIT_GROUND | (HRL_FACE_GROUND << 16); }
        }
    }
    *depth = h.seg != HRL_HIT_NONE ? h.best * r.cj : sp.max_range;
    *seg = h.seg;
    *rgb = shade_rgb(h.seg);
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_camera_spec *s) {
    if (!s) return "null camera spec";
    if (s->struct_size != sizeof(hrl_camera_spec)) return "hrl_camera_spec.struct_size is not sizeof(hrl_camera_spec): initialise the record with hrl_camera_default_spec()";
    if (s->width < HRL_CAMERA_MIN_WIDTH || s->width > HRL_CAMERA_MAX_SIZE || s->width % 16 != 0) return "camera width must be a multiple of 16 within 16..128";
    if (s->height < HRL_CAMERA_MIN_HEIGHT || s->height > HRL_CAMERA_MAX_SIZE || s->height % 8 != 0) return "camera height must be a multiple of 8 within 8..128";
    if (s->frame != HRL_SCAN_WORLD && s->frame != HRL_SCAN_HEADING) return "unknown camera frame";
    if (s->eye_mode != HRL_EYE_GROUND && s->eye_mode != HRL_EYE_TORSO) return "unknown camera eye_mode";
    if (!(s->eye_height >= 0.f) || !(s->eye_height <= HRL_CAMERA_MAX_EYE_HEIGHT)) return "camera eye_height must be finite and within 0..10";
    if (!(s->tan_half_h > HRL_CAMERA_MIN_TAN) || !(s->tan_half_h <= HRL_CAMERA_MAX_TAN)) return "camera tan_half_h must be finite and within (1e-3, 1e3]";
    if (!(s->tan_half_v > HRL_CAMERA_MIN_TAN) || !(s->tan_half_v <= HRL_CAMERA_MAX_TAN)) return "camera tan_half_v must be finite and within (1e-3, 1e3]";
    if (!(s->max_range > 0.f) || !(s->max_range <= 3.0e38f)) return "camera max_range must be finite and positive";
    if (s->classes == 0u || (s->classes & ~(HRL_SCAN_ALL | HRL_CAMERA_GROUND)) != 0u)
        return "camera classes must be a non-empty mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET | HRL_CAMERA_GROUND";
    return "";
}
inline std::string validate_out(const hrl_camera_out *o) {
    if (!o) return "null camera out";
    if (!o->depth && !o->seg && !o->rgb) return "camera out holds no pointer: at least one output must be given";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t frame, hrl_camera_spec *s) {
    hrl_scan_spec r;
    if (!s || scan::default_spec(c, frame, &r) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->width = 64; s->height = 48; s->frame = frame;
    s->eye_mode = HRL_EYE_TORSO; s->eye_height = c->env_kind == HRL_POINT_GATHER ? 0.4f : 0.3f;
    s->tan_half_h = 1.f; s->tan_half_v = 0.75f;
    s->max_range = r.max_range;
    s->classes = HRL_SCAN_ALL | HRL_CAMERA_GROUND;
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: the table, its z-intervals and its list, then chunks of CHUNK pixels in
 * runs of 64, the chunk's rgb bytes staged and copied out as words. */
inline void camera_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_camera_spec &sp, const hrl_camera_out &out, size_t env) {
    ScanSet S;
    float zl[S_SLOTS], zh[S_SLOTS];
    static thread_local uint32_t stage[CHUNK * 3 / 4];
    uint8_t *bytes = reinterpret_cast<uint8_t *>(stage);
    const hrl_scan_spec ts = table_spec(sp);
    const Frame f = scan::table_frame(st);
    scan::forward(sp.frame, st, &S.fwd[0], &S.fwd[1]);
    for (int slot = 0; slot < S_SLOTS; ++slot) { scan::build_slot(S, slot, c, st, items, aux, f, ts); z_extent(slot, c, &zl[slot], &zh[slot]); }
    unsigned long long m0 = 0, m1 = 0;
    for (int slot = 0; slot < 64; ++slot) if (scan::kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (scan::kept(S, slot)) m1 |= 1ull << (slot - 64);
    const Eye eye = eye_of(c, st, sp);
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
            shade_pixel(S, zl, zh, m0, m1, sp, eye, i, j, inv_w, inv_h, &d, &s, &rgb);
            if (out.depth) out.depth[base + k] = d;
            if (out.seg) out.seg[base + k] = s;
            bytes[3 * (k - k0)] = (uint8_t)rgb; bytes[3 * (k - k0) + 1] = (uint8_t)(rgb >> 8); bytes[3 * (k - k0) + 2] = (uint8_t)(rgb >> 16);
        }
        if (out.rgb) memcpy(out.rgb + 3 * (base + k0), stage, 3 * (size_t)(k1 - k0));
    }
}
/* hrl_camera on host pointers; returns the status and leaves the reason in `why` */
inline int camera_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_camera_spec *sp, const uint8_t *mask, const hrl_camera_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        camera_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp, *out, (size_t)e);
    }
    return HRL_OK;
}
#endif

}  // namespace camera
}  // namespace hrl
