/*
 * links_core.h -- specification of the batched link states (include/hrl_links.h), written once as plain C++: the device kernel
 * (links_hip.hip) and the host build of the tests (tests/links_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The state of one link of one env is a pure function of (DevCfg, the env's state record, the frame, the link's index):
 *
 *   link_world  the leg kinematics of the step, RESTATED EXPRESSION FOR EXPRESSION from phase_kin_ankle (step_core.h: that function
 *               needs the step's WaveLds and cannot be called from here): X, Y, Z by quat_axes, the joint angles through sincos_spec,
 *               e1 / axw / e2, ph / pa / tip relative to O, the joint screws Sh = (Z, ph x Z), Sa = (axw, pa x axw) and the spatial
 *               velocities v0, vx = v0 + Sh * rate, vf = vx + Sa * rate in the step's order (omega, v of O).  From them the link's
 *               ends p0, p1 relative to O, its body-frame quaternion (a product of the state's quaternion as stored and the joints'
 *               half-angle quaternions, no normalisation) and its twist
 *   link_out    the seven numbers a caller reads, in the spec's frame: world = O + relative, sum by sum as the CPU oracle's
 *               orc_ant_leg_points forms them, so origin equals the step's points bit for bit; heading = the relative vectors turned by
 *               minus the yaw of scan::forward (restated in `heading`)
 *   site_out    a point fixed to a link: origin + R(quat) * local with R by quat_axes, and the velocity of the point as carried
 *
 * A lane of the kernel evaluates one link or one site from the env's record alone, so the host build's loops are the kernel's
 * partition: no value crosses from one link's evaluation to another's.
 *
 * Totality: the link's index, the leg and the type are integers of the launch, never of the state; the only float-to-int conversion is
 * sincos_spec's guarded quadrant.  NaN and inf flow through the arithmetic to the env's own outputs.
 */
#pragma once
#include "../../include/hrl_links.h"
#include "host_cfg.h" /* (includes step_core.h: fma_, cross3, sincos_spec, quat_axes, DevCfg) */

namespace hrl {
namespace links {

constexpr int GROUP = 16;                     /* envs of a workgroup = lanes of an env (links_hip.hip) */
constexpr int MAX_B = HRL_LINKS_MAX, MAX_S = HRL_LINKS_MAX_SITES;
constexpr int ROW_MAX = 4 * MAX_B;            /* floats per env of the widest tensor: quat, 52 (sites: 48) */
static_assert(MAX_B <= GROUP && MAX_S <= GROUP && 3 * MAX_S <= ROW_MAX, "a lane per link, a lane per site, one staging row per env");

/* (constexpr: the host side's guards call it too) */
constexpr int n_links(int kind) { return kind == HRL_POINT_GATHER ? HRL_LINKS_POINT : HRL_LINKS_ANT; }

/* c ? a : b on VALUES: both operands are loaded before the choice.  (Written as a conditional expression on two array elements under a
 * uniform condition, the compiler chooses between the two ADDRESSES and loads once, which keeps both arrays in scratch memory.) */
HRL_DEV float pick(bool c, float a, float b) { return c ? a : b; }

/* Hamilton product a * b of quaternions stored (x, y, z, w): the rotation b, then a */
HRL_DEV void qmul(const float *a, const float *b, float *o) {
    const float x = fma_(a[3], b[0], fma_(a[0], b[3], fma_(a[1], b[2], -(a[2] * b[1]))));
    const float y = fma_(a[3], b[1], fma_(a[1], b[3], fma_(a[2], b[0], -(a[0] * b[2]))));
    const float z = fma_(a[3], b[2], fma_(a[2], b[3], fma_(a[0], b[1], -(a[1] * b[0]))));
    const float w = fma_(a[3], b[3], -fma_(a[0], b[0], fma_(a[1], b[1], a[2] * b[2])));
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

/* One link in world axes, relative to O.  centred: the torso or the cube -- origin = com = O and the twist is the state's as it is. */
struct Link {
    float p0[3], p1[3], mid[3]; /* the capsule's ends and 0.5 * (p0 + p1) */
    float q[4];                 /* body frame */
    float w[3], vO[3];          /* angular velocity, velocity of the body's point at O */
    bool centred, at_O;         /* at_O: p0 is O itself (torso, cube, hip capsules) */
};

/* (Straight-line code: every link evaluates a leg and picks by selects -- the torso and the cube pick nothing of it.  With an early
 * return for them the compiler merges the stores of the two paths into stores at run-time offsets, which keeps the record in scratch.) */
HRL_DEV void link_world(const DevCfg &c, const float *st, int link, Link &K) {
    const float *q = st + HRL_QPOS_OFF, *u = st + HRL_QVEL_OFF; /* u: v of O, omega, joint rates */
    const bool centred = c.kind == HRL_POINT_GATHER || link <= 0 || link >= HRL_LINKS_ANT;
    /* hip capsule 9 + l | aux 1 + 2 l | foot 2 + 2 l */
    const int type = centred || link >= 9 ? 0 : 1 + ((link - 1) & 1), l = centred ? 0 : (link >= 9 ? link - 9 : (link - 1) >> 1);
    K.centred = centred; K.at_O = type == 0;
    /* ---- phase_kin_ankle, restated (step_core.h:407-450) */
    const float is2 = 0.70710678118654752440f;
    float X[3], Y[3], Z[3];
    quat_axes(q[3], q[4], q[5], q[6], X, Y, Z);
    const float qh = q[7 + 2 * l], qa = q[8 + 2 * l], qdh = u[6 + 2 * l], qda = u[7 + 2 * l];
    float ch, sh, ca, sa;
    sincos_spec(qh, &sh, &ch);
    sincos_spec(qa, &sa, &ca);
    const float sx = (l == 0 || l == 3) ? 1.f : -1.f, sy = (l < 2) ? 1.f : -1.f;
    const float ax = (l & 1) ? 1.f : -1.f, ay = 1.f, sg = (l == 1 || l == 2) ? 1.f : -1.f;
    const float e1x = fma_(sx, ch, -(sy * sh)) * is2, e1y = fma_(sx, sh, sy * ch) * is2;
    const float axx = fma_(ax, ch, -(ay * sh)) * is2, axy = fma_(ax, sh, ay * ch) * is2;
    float e1[3], axw[3], e2[3], ph[3], pa[3], tip[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = fma_(e1y, Y[k], e1x * X[k]);
        axw[k] = fma_(axy, Y[k], axx * X[k]);
        e2[k] = fma_(sg * sa, Z[k], ca * e1[k]);
        ph[k] = 0.2f * fma_(sy, Y[k], sx * X[k]);
        pa[k] = fma_(c.L1, e1[k], ph[k]);
        tip[k] = fma_(c.L2, e2[k], pa[k]);
    }
    float Sh[6], Sa[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Sh[k] = Z[k]; Sa[k] = axw[k]; }
    cross3(Sh + 3, ph, Z);
    cross3(Sa + 3, pa, axw);
    float v0[6], vjh[6], vx[6], vja[6], vf[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { v0[k] = u[3 + k]; v0[3 + k] = u[k]; } /* qvel (v, omega) -> (omega, v): step_entry */
#pragma unroll
    for (int k = 0; k < 6; ++k) { vjh[k] = Sh[k] * qdh; vx[k] = v0[k] + vjh[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) { vja[k] = Sa[k] * qda; vf[k] = vx[k] + vja[k]; }
    /* ---- the body frames: q_torso * Rz(hip) * R(ankle axis, ankle); the ankle's axis in the aux frame is (ax, ay, 0) / sqrt 2 */
    float shh, chh, sha, cha;
    sincos_spec(0.5f * qh, &shh, &chh);
    sincos_spec(0.5f * qa, &sha, &cha);
    const float hz[4] = {0.f, 0.f, shh, chh}, ha[4] = {(ax * is2) * sha, (ay * is2) * sha, 0.f, cha};
    float qx[4], qf[4];
    qmul(q + 3, hz, qx);
    qmul(qx, ha, qf);
    /* ---- the lane's body */
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p0 = pick(type == 0, 0.f, pick(type == 1, ph[k], pa[k])), p1 = pick(type == 0, ph[k], pick(type == 1, pa[k], tip[k]));
        K.p0[k] = pick(centred, 0.f, p0);
        K.p1[k] = pick(centred, 0.f, p1);
        K.mid[k] = pick(centred, 0.f, 0.5f * (p0 + p1));
        K.w[k] = pick(type == 0, v0[k], pick(type == 1, vx[k], vf[k]));
        K.vO[k] = pick(type == 0, v0[3 + k], pick(type == 1, vx[3 + k], vf[3 + k]));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) K.q[k] = pick(type == 0, q[3 + k], pick(type == 1, qx[k], qf[k]));
}

/* The heading: scan::forward of HRL_SCAN_HEADING restated (scan_core.h:53-64: the normalised ground projection of the torso's X axis,
 * world +x when there is none), and the inverse yaw quaternion (0, 0, -sin(yaw / 2), cos(yaw / 2)) from it by the half-angle formulas,
 * taken on the side where they do not cancel: no inverse trigonometry. */
struct Heading { float fx, fy, qinv[4]; };

HRL_DEV Heading heading(const float *st) {
    Heading h;
    h.fx = 1.f; h.fy = 0.f;
    float X[3], Y[3], Z[3];
    quat_axes(st[3], st[4], st[5], st[6], X, Y, Z);
    const float n2 = fma_(X[0], X[0], X[1] * X[1]);
    if (n2 >= 1e-12f && n2 <= 3.0e38f) { /* (false for NaN; an overflowed norm is infinite) */
        const float inv = 1.f / sqrtf(n2);
        h.fx = X[0] * inv; h.fy = X[1] * inv;
    }
    float s, co;
    if (h.fx >= 0.f) { co = sqrtf(0.5f * (1.f + h.fx)); s = (0.5f * h.fy) / co; }
    else { s = sqrtf(0.5f * (1.f - h.fx)); s = h.fy < 0.f ? -s : s; co = (0.5f * h.fy) / s; }
    h.qinv[0] = 0.f; h.qinv[1] = 0.f; h.qinv[2] = -s; h.qinv[3] = co;
    return h;
}
/* v turned by minus the yaw */
HRL_DEV void turn(const Heading &h, const float *v, float *o) {
    const float x = fma_(h.fx, v[0], h.fy * v[1]), y = fma_(h.fx, v[1], -(h.fy * v[0]));
    o[0] = x; o[1] = y; o[2] = v[2];
}

struct LinkOut { float origin[3], com[3], quat[4], lin[3], ang[3]; };
struct SiteOut { float pos[3], vel[3]; };

/* the velocity of the point p (relative to O) carried by K */
HRL_DEV void point_velocity(const Link &K, const float *p, float *v) {
    float wxp[3];
    cross3(wxp, K.w, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = K.vO[k] + wxp[k];
}

/* (Both frames are evaluated and the spec's one is picked by selects: with a branch per frame the compiler merges the two arms' stores
 * into one store at a run-time offset, which keeps the record in scratch memory.) */
HRL_DEV void link_out(const DevCfg &c, const float *st, int frame, int link, LinkOut &o) {
    Link K;
    link_world(c, st, link, K);
    const bool hd = frame == HRL_LINKS_HEADING;
    float lin[3], t0[3], tm[3], tl[3], tw[3], tq[4];
    point_velocity(K, K.mid, lin);
#pragma unroll
    for (int k = 0; k < 3; ++k) lin[k] = pick(K.centred, K.vO[k], lin[k]); /* the state's bits (inf x 0 would be NaN) */
    const Heading h = heading(st);
    turn(h, K.p0, t0);
    turn(h, K.mid, tm);
    turn(h, lin, tl);
    turn(h, K.w, tw);
    qmul(h.qinv, K.q, tq);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float O = st[HRL_QPOS_OFF + k];
        const float a = pick(K.at_O, O, O + K.p0[k]), b = O + K.p1[k]; /* the oracle's sums: q[k] + ph[k], ... */
        const float m = pick(K.centred, O, 0.5f * (a + b));
        /* heading: O is the frame's origin whatever the state holds */
        o.origin[k] = pick(hd, pick(K.at_O, 0.f, t0[k]), a);
        o.com[k] = pick(hd, pick(K.centred, 0.f, tm[k]), m);
        o.lin[k] = pick(hd, tl[k], lin[k]);
        o.ang[k] = pick(hd, tw[k], K.w[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) o.quat[k] = pick(hd, tq[k], K.q[k]);
}

HRL_DEV void site_out(const DevCfg &c, const float *st, int frame, int link, float lx, float ly, float lz, SiteOut &o) {
    Link K;
    link_world(c, st, link, K);
    const bool hd = frame == HRL_LINKS_HEADING;
    float X[3], Y[3], Z[3], r[3], p[3], v[3], tp[3], tv[3];
    quat_axes(K.q[0], K.q[1], K.q[2], K.q[3], X, Y, Z);
#pragma unroll
    for (int k = 0; k < 3; ++k) { r[k] = fma_(lz, Z[k], fma_(ly, Y[k], lx * X[k])); p[k] = K.p0[k] + r[k]; }
    point_velocity(K, p, v);
    const Heading h = heading(st);
    turn(h, p, tp);
    turn(h, v, tv);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float O = st[HRL_QPOS_OFF + k];
        const float w = pick(K.at_O, O, O + K.p0[k]) + r[k]; /* origin[link] + R local */
        o.pos[k] = pick(hd, tp[k], w);
        o.vel[k] = pick(hd, tv[k], v[k]);
    }
}

/* ------------------------------------------------------------------------------------------------ host side */
inline const char *link_name(int32_t kind, int32_t i) {
    static const char *const ANT[HRL_LINKS_ANT] = {"torso", "aux_1", "front_left_foot", "aux_2", "front_right_foot", "aux_3", "left_back_foot", "aux_4", "right_back_foot",
                                                   "front_left_leg", "front_right_leg", "left_back_leg", "right_back_leg"};
    if (kind < HRL_ANT_FLAT || kind > HRL_ANT_FLAGRUN || i < 0 || i >= n_links(kind)) return nullptr;
    return kind == HRL_POINT_GATHER ? "cube" : ANT[i];
}

inline std::string validate_spec(const hrl_config *c, const hrl_links_spec *s) {
    if (!s) return "null links spec";
    if (s->struct_size != sizeof(hrl_links_spec)) return "hrl_links_spec.struct_size is not sizeof(hrl_links_spec): initialise the record with hrl_links_default_spec()";
    if (s->frame != HRL_LINKS_WORLD && s->frame != HRL_LINKS_HEADING) return "unknown links frame";
    if (s->n_sites < 0 || s->n_sites > HRL_LINKS_MAX_SITES) return "links n_sites must be within 0..16";
    const int B = n_links(c->env_kind);
    for (int i = 0; i < s->n_sites; ++i) {
        if (s->site_link[i] < 0 || s->site_link[i] >= B) return "links site_link must be within 0..B-1 (B = 13 links for the ants, 1 for the point bot)";
        for (int k = 0; k < 3; ++k)
            if (!(fabsf(s->site_local[i][k]) <= 3.0e38f)) return "links site_local must be finite";
    }
    return "";
}
inline std::string validate_out(const hrl_links_out *o, const hrl_links_spec *s) {
    if (!o) return "null links out";
    const bool sites = s->n_sites > 0 && (o->site_pos || o->site_vel);
    if (!o->origin && !o->com && !o->quat && !o->lin_vel && !o->ang_vel && !sites)
        return "links out holds no pointer: at least one output must be given (site_pos and site_vel count with n_sites > 0)";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t frame, hrl_links_spec *s) {
    if (!s || !c || c->env_kind < HRL_ANT_FLAT || c->env_kind > HRL_ANT_FLAGRUN || (frame != HRL_LINKS_WORLD && frame != HRL_LINKS_HEADING)) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->frame = frame;
    if (c->env_kind == HRL_POINT_GATHER) { s->n_sites = 1; return HRL_OK; } /* the cube's centre */
    s->n_sites = 4;
    for (int l = 0; l < 4; ++l) { /* the far end of the foot capsule's fromto: assets/ant.xml:22,33,44,55 */
        s->site_link[l] = HRL_LINK_FOOT(l);
        s->site_local[l][0] = (l == 0 || l == 3) ? 0.4f : -0.4f; s->site_local[l][1] = l < 2 ? 0.4f : -0.4f; s->site_local[l][2] = 0.f;
    }
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: a link per lane, then a site per lane. */
inline void links_env_host(const DevCfg &c, const float *st, const hrl_links_spec &sp, const hrl_links_out &out, size_t env) {
    const int B = n_links(c.kind);
    for (int link = 0; link < B; ++link) {
        LinkOut o;
        link_out(c, st, sp.frame, link, o);
        const size_t at = env * (size_t)B + (size_t)link;
        for (int k = 0; k < 3; ++k) {
            if (out.origin) out.origin[3 * at + k] = o.origin[k];
            if (out.com) out.com[3 * at + k] = o.com[k];
            if (out.lin_vel) out.lin_vel[3 * at + k] = o.lin[k];
            if (out.ang_vel) out.ang_vel[3 * at + k] = o.ang[k];
        }
        for (int k = 0; k < 4; ++k)
            if (out.quat) out.quat[4 * at + k] = o.quat[k];
    }
    for (int s = 0; s < sp.n_sites; ++s) {
        SiteOut o;
        site_out(c, st, sp.frame, sp.site_link[s], sp.site_local[s][0], sp.site_local[s][1], sp.site_local[s][2], o);
        const size_t at = env * (size_t)sp.n_sites + (size_t)s;
        for (int k = 0; k < 3; ++k) {
            if (out.site_pos) out.site_pos[3 * at + k] = o.pos[k];
            if (out.site_vel) out.site_vel[3 * at + k] = o.vel[k];
        }
    }
}
/* hrl_links on host pointers; returns the status and leaves the reason in `why` */
inline int links_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_links_spec *sp, const uint8_t *mask, const hrl_links_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(cfg, sp);
    if (why.empty()) why = validate_out(out, sp);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e0 = 0; e0 < cfg->num_envs; e0 += GROUP) /* a workgroup's envs */
        for (int e = e0; e < e0 + GROUP && e < cfg->num_envs; ++e) {
            if (mask && !mask[e]) continue;
            links_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, *sp, *out, (size_t)e);
        }
    return HRL_OK;
}
#endif

}  // namespace links
}  // namespace hrl
