/*
 * dyn_core.h -- specification of the batched dynamics terms (include/hrl_dyn.h), written once as plain C++: the device kernel
 * (dyn_hip.hip) and the host build of the tests (tests/dyn_host, HRL_EMU) compile the same functions and produce the same bits.  fp32
 * throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * Everything is in world axes and relative to O, the torso's origin, in the step's spatial notation (csrc/step_core.h): a motion vector is
 * (angular, linear at O), a force vector (moment about O, force), a spatial inertia the 21 floats of si().  The generalised velocity is the
 * state's qvel, (v of O, omega, joint rates): generalised index i < 6 is spatial index sp(i) = (i + 3) % 6.
 *
 * One env is evaluated in phases; between two phases values cross from one evaluation to another through the env's Work record (LDS on the
 * device), within a phase no value crosses:
 *
 *   body_terms   b = 0..8 (0 the torso, 1 + 2 l the upper body of leg l, 2 + 2 l its foot -- the link order of hrl_links.h).  The leg's
 *                kinematics of phase_kin_ankle, restated (leg_kin), then the step's own rigid-body quantities: spatial_inertia(m, alpha,
 *                beta, e, c), the velocity v_b, the momentum I v_b, and the body's bias wrench
 *                    f_b = I a_b + v_b x* (I v_b) - gravity + Bullet's damping wrench,
 *                a_b the spatial acceleration at udot = 0: the torso's (0, -(omega x v)) -- the generalised velocity holds the CLASSICAL
 *                velocity of O, whose derivative differs from the spatial one by omega x v -- plus v x (S rate) down the leg.  Also
 *                T_b = 0.5 v_b . I v_b and m_b c_b.  The foot's evaluation publishes the leg's two joint screws
 *   leg_terms    l = 0..3: the composite inertia and force of the leg (upper body + foot), F = I^c S of both joints (the base-joint
 *                block of M), the three joint-joint entries (+ armature), the joint rows of bias (+ joint_damping * rate).  With `accel`:
 *                the leg's part of the L D L^T factorisation of M along the tree -- pivot the ankle, then the hip -- and what it
 *                subtracts from the base block and the base's right-hand side
 *   base_terms   entry k = 0..26: torso + ((leg 0 + leg 1) + (leg 2 + leg 3)), the base block of M and the base rows of bias
 *   total_terms  entry k = 0..9: momentum about O, T and sum m c over the nine bodies, b0 + (((b1 + b2) + (b3 + b4)) + ((b5 + b6) + (b7 + b8)))
 *   base_solve   the 6 x 6 Schur complement by the step's ldl6_factor / ldl6_solve
 *   leg_back     l = 0..3: the back substitution of the leg's two joints
 *   then the outputs, entry by entry: mass_entry, bias_entry, jac_site, summary
 *
 * The point bot is one body (the cube: m = 10, isotropic inertia m (0.7)^2 / 6) and no leg: body_terms(0), base = that body.
 *
 * Totality: every index is an integer of the launch; the only float-to-int conversion is sincos_spec's guarded quadrant.  Divisions by a
 * pivot are carried out whatever its sign: a non-positive pivot or a NaN flows into the env's own outputs.
 */
#pragma once
#include "../../include/hrl_dyn.h"
#include "links_core.h" /* (includes host_cfg.h and step_core.h) */

namespace hrl {
namespace dyn {

constexpr int GROUP = 16;                      /* envs of a workgroup = lanes of an env (dyn_hip.hip) */
constexpr int NB = 9, MAX_S = HRL_DYN_MAX_SITES;
constexpr int NV_MAX = HRL_DYN_NV_ANT;
constexpr int ROW_MAX = NV_MAX * NV_MAX;       /* floats per env of the widest tensor: mass, 196 */
constexpr int JAC_CHUNK = 4;                   /* sites of jac that leave through the staging row at a time: 4 x 3 x 14 = 168 floats */
static_assert(MAX_S == HRL_LINKS_MAX_SITES && MAX_S <= GROUP && NB <= GROUP && JAC_CHUNK * 3 * NV_MAX <= ROW_MAX, "a lane per body, a lane per site, one staging row per env");

constexpr int nv_of(int kind) { return kind == HRL_POINT_GATHER ? HRL_DYN_NV_POINT : HRL_DYN_NV_ANT; }
using links::pick;

/* generalised index (v, omega) <-> spatial index (omega, v) of the base */
HRL_DEV constexpr int sp(int i) { return i < 3 ? i + 3 : i - 3; }

/* What crosses between the phases of one env. */
struct Work {
    float If[NB][27];    /* body_terms: spatial inertia [21], bias wrench [6] */
    float hT[NB][10];    /* body_terms: momentum I v [6], T, m c [3] */
    float S[8][6];       /* body_terms (feet): joint screws, S[2 l] the hip's, S[2 l + 1] the ankle's */
    float leg[4][27];    /* leg_terms: the leg's composite inertia and force */
    float F[8][6];       /* leg_terms: I^c S, the column of M between the base and joint j (spatial order) */
    float Mj[4][3];      /* leg_terms: M[hip][hip], M[hip][ankle], M[ankle][ankle] */
    float bj[8];         /* leg_terms: joint rows of bias */
    /* (leg_terms leaves what the leg's two pivots subtract from the base block [21] and from the base's right-hand side [6] in If[1 + 2 l],
     * the record of the leg's upper body, which nothing reads after leg_terms has summed it into `leg`: sch()) */
    float el[4][17];    /* leg_terms: ya, yh, 1/da, 1/dh, l_ha, La[6], Lh[6] */
    float base[27];      /* base_terms */
    float tot[10];       /* total_terms */
    float tau[NV_MAX];   /* the applied generalised force (zeros without one) */
    float x[NV_MAX];     /* base_solve, leg_back: udot, generalised order */
};

HRL_DEV float *sch(Work &W, int l) { return W.If[1 + 2 * l]; }
HRL_DEV const float *sch(const Work &W, int l) { return W.If[1 + 2 * l]; }

/* The kinematics of leg l: phase_kin_ankle restated expression for expression (step_core.h:407-452). */
struct Leg {
    float Z[3], axw[3], e1[3], e2[3], ph[3], pa[3], caux[3], cfoot[3];
    float Sh[6], Sa[6], v0[6], vx[6], vf[6], cbh[6], cba[6];
};

HRL_DEV void leg_kin(const DevCfg &c, const float *st, int l, Leg &G) {
    const float *q = st + HRL_QPOS_OFF, *u = st + HRL_QVEL_OFF; /* u: v of O, omega, joint rates */
    const float is2 = 0.70710678118654752440f;
    float X[3], Y[3];
    quat_axes(q[3], q[4], q[5], q[6], X, Y, G.Z);
    const float qh = q[7 + 2 * l], qa = q[8 + 2 * l], qdh = u[6 + 2 * l], qda = u[7 + 2 * l];
    float ch, sh, ca, sa;
    sincos_spec(qh, &sh, &ch);
    sincos_spec(qa, &sa, &ca);
    const float sx = (l == 0 || l == 3) ? 1.f : -1.f, sy = (l < 2) ? 1.f : -1.f;
    const float ax = (l & 1) ? 1.f : -1.f, ay = 1.f, sg = (l == 1 || l == 2) ? 1.f : -1.f;
    const float e1x = fma_(sx, ch, -(sy * sh)) * is2, e1y = fma_(sx, sh, sy * ch) * is2;
    const float axx = fma_(ax, ch, -(ay * sh)) * is2, axy = fma_(ax, sh, ay * ch) * is2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        G.e1[k] = fma_(e1y, Y[k], e1x * X[k]);
        G.axw[k] = fma_(axy, Y[k], axx * X[k]);
        G.e2[k] = fma_(sg * sa, G.Z[k], ca * G.e1[k]);
        G.ph[k] = 0.2f * fma_(sy, Y[k], sx * X[k]);
        G.pa[k] = fma_(c.L1, G.e1[k], G.ph[k]);
        G.caux[k] = fma_(c.L1 * 0.5f, G.e1[k], G.ph[k]);
        G.cfoot[k] = fma_(c.L2 * 0.5f, G.e2[k], G.pa[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { G.Sh[k] = G.Z[k]; G.Sa[k] = G.axw[k]; }
    cross3(G.Sh + 3, G.ph, G.Z);
    cross3(G.Sa + 3, G.pa, G.axw);
    float vjh[6], vja[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) { G.v0[k] = u[3 + k]; G.v0[3 + k] = u[k]; } /* qvel (v, omega) -> (omega, v): step_entry */
#pragma unroll
    for (int k = 0; k < 6; ++k) { vjh[k] = G.Sh[k] * qdh; G.vx[k] = G.v0[k] + vjh[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) { vja[k] = G.Sa[k] * qda; G.vf[k] = G.vx[k] + vja[k]; }
    crm(G.cbh, G.v0, vjh);
    crm(G.cba, G.vx, vja);
}

/* Body b of the env.  type: 0 foot, 1 upper body, 2 torso (the step's), 3 the point bot's cube. */
HRL_DEV void body_terms(const DevCfg &c, const float *st, int b, Work &W) {
    const bool cube = c.kind == HRL_POINT_GATHER;
    const int type = cube ? 3 : (b == 0 ? 2 : ((b - 1) & 1 ? 0 : 1)), l = (cube || b == 0) ? 0 : (b - 1) >> 1;
    Leg G;
    leg_kin(c, st, l, G);
    const float cm = 10.f, cI = cm * (0.7f * 0.7f) / 6.f; /* point_substep */
    const float bm = pick(type == 0, c.m2, pick(type == 1, c.m1, pick(type == 2, c.m0, cm)));
    const float bal = pick(type == 0, c.a2, pick(type == 1, c.a1, pick(type == 2, c.a0, cI)));
    const float bbe = pick(type == 0, c.b2, pick(type == 1, c.b1, pick(type == 2, c.b0, 0.f)));
    float be[3], bc[3], bv[6], ab[6], wxv[3];
    cross3(wxv, G.v0, G.v0 + 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        be[k] = pick(type == 0, G.e2[k], pick(type == 1, G.e1[k], pick(type == 2, G.Z[k], k == 2 ? 1.f : 0.f)));
        bc[k] = pick(type == 0, G.cfoot[k], pick(type == 1, G.caux[k], 0.f));
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        bv[k] = pick(type == 0, G.vf[k], pick(type == 1, G.vx[k], G.v0[k]));
        const float a0 = k < 3 ? 0.f : -wxv[k - 3], ax_ = a0 + G.cbh[k], af = ax_ + G.cba[k];
        ab[k] = pick(type == 0, af, pick(type == 1, ax_, a0));
    }
    float I[21], Iv[6], Ia[6], f[6], ng[3], p[6];
    spatial_inertia(I, bm, bal, bbe, be, bc);
    const float fg2[3] = {0.f, 0.f, -bm * c.g};
    sym6_matvec(Iv, I, bv);
    sym6_matvec(Ia, I, ab);
    crf(f, bv, Iv);
    cross3(ng, bc, fg2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = (Ia[k] + f[k]) - ng[k]; p[3 + k] = (Ia[3 + k] + f[3 + k]) - fg2[k]; }
    if (c.damping_on) { /* (uniform) Bullet's damping wrench, as phase_kin_ankle forms it (step_core.h:478-491) */
        float wc[3], vc[3], fd[3], nd[3], cf[3];
        cross3(wc, bv, bc);
#pragma unroll
        for (int k = 0; k < 3; ++k) vc[k] = bv[3 + k] + wc[k];
        const float kl = c.damp_lin * (1.f + sqrtf(dot3(vc, vc))), ka = c.damp_ang * (1.f + sqrtf(dot3(bv, bv)));
        const float ew = dot3(be, bv);
#pragma unroll
        for (int k = 0; k < 3; ++k) { fd[k] = (bm * vc[k]) * kl; nd[k] = fma_(bbe * ew, be[k], bal * bv[k]) * ka; }
        cross3(cf, bc, fd);
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = p[k] + (nd[k] + cf[k]); p[3 + k] = p[3 + k] + fd[k]; }
    }
#pragma unroll
    for (int k = 0; k < 21; ++k) W.If[b][k] = I[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) W.If[b][21 + k] = p[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) W.hT[b][k] = Iv[k];
    W.hT[b][6] = 0.5f * dot6(bv, Iv);
#pragma unroll
    for (int k = 0; k < 3; ++k) W.hT[b][7 + k] = bm * bc[k];
    if (type == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { W.S[2 * l][k] = G.Sh[k]; W.S[2 * l + 1][k] = G.Sa[k]; }
    }
}

/* Leg l of an ant, after body_terms of its two bodies. */
HRL_DEV void leg_terms(const DevCfg &c, const float *st, int l, bool solve, Work &W) {
    const int jh = 2 * l, ja = jh + 1, bx = 1 + 2 * l, bf = 2 + 2 * l;
    float Ifoot[21], Ic[21], ff[6], fc[6], Sh[6], Sa[6], Fa[6], Fh[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) { Ifoot[k] = W.If[bf][k]; Ic[k] = W.If[bx][k] + Ifoot[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) { ff[k] = W.If[bf][21 + k]; fc[k] = W.If[bx][21 + k] + ff[k]; Sh[k] = W.S[jh][k]; Sa[k] = W.S[ja][k]; }
    sym6_matvec(Fa, Ifoot, Sa);
    sym6_matvec(Fh, Ic, Sh);
    const float Maa = dot6(Sa, Fa) + c.armature, Mha = dot6(Sh, Fa), Mhh = dot6(Sh, Fh) + c.armature;
    const float bh = fma_(c.jdamp, st[HRL_QVEL_OFF + 6 + jh], dot6(Sh, fc)), ba = fma_(c.jdamp, st[HRL_QVEL_OFF + 6 + ja], dot6(Sa, ff));
#pragma unroll
    for (int k = 0; k < 21; ++k) W.leg[l][k] = Ic[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) { W.leg[l][21 + k] = fc[k]; W.F[jh][k] = Fh[k]; W.F[ja][k] = Fa[k]; }
    W.Mj[l][0] = Mhh; W.Mj[l][1] = Mha; W.Mj[l][2] = Maa;
    W.bj[jh] = bh; W.bj[ja] = ba;
    if (!solve) return; /* (uniform) */
    /* L D L^T along the tree: pivot the ankle, then the hip; the base block keeps what is left */
    const float ia = 1.f / Maa, lha = Mha * ia;
    const float ih = 1.f / fma_(-lha, Mha, Mhh);
    const float ya = W.tau[6 + ja] - ba, yh = fma_(-lha, ya, W.tau[6 + jh] - bh);
    float La[6], Fh2[6], Lh[6];
    float *out = sch(W, l); /* (its 27 floats were read above) */
#pragma unroll
    for (int k = 0; k < 6; ++k) { La[k] = Fa[k] * ia; Fh2[k] = fma_(-lha, Fa[k], Fh[k]); Lh[k] = Fh2[k] * ih; }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) out[si(a, b)] = fma_(Fh2[a], Lh[b], Fa[a] * La[b]);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[21 + k] = fma_(Lh[k], yh, La[k] * ya);
    W.el[l][0] = ya; W.el[l][1] = yh; W.el[l][2] = ia; W.el[l][3] = ih; W.el[l][4] = lha;
#pragma unroll
    for (int k = 0; k < 6; ++k) { W.el[l][5 + k] = La[k]; W.el[l][11 + k] = Lh[k]; }
}

/* Entry k = 0..26 of the base: the composite inertia of the whole robot about O [21] and the base rows of bias [6] (spatial order). */
HRL_DEV void base_terms(const DevCfg &c, int k, Work &W) {
    const float body = W.If[0][k];
    W.base[k] = c.kind == HRL_POINT_GATHER ? body : body + ((W.leg[0][k] + W.leg[1][k]) + (W.leg[2][k] + W.leg[3][k]));
}

/* Entry k = 0..9 of the totals: momentum about O [6] (angular, linear), T, sum m c [3]. */
HRL_DEV void total_terms(const DevCfg &c, int k, Work &W) {
    const float body = W.hT[0][k];
    W.tot[k] = c.kind == HRL_POINT_GATHER ? body : body + (((W.hT[1][k] + W.hT[2][k]) + (W.hT[3][k] + W.hT[4][k])) + ((W.hT[5][k] + W.hT[6][k]) + (W.hT[7][k] + W.hT[8][k])));
}

/* The base block's Schur complement, factorised and solved: udot of the base. */
HRL_DEV void base_solve(const DevCfg &c, Work &W) {
    const bool ant = c.kind != HRL_POINT_GATHER;
    float A[21], r[6], Lm[15], id[6], xb[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = ant ? W.base[k] - ((sch(W, 0)[k] + sch(W, 1)[k]) + (sch(W, 2)[k] + sch(W, 3)[k])) : W.base[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float r0 = W.tau[sp(k)] - W.base[21 + k];
        r[k] = ant ? r0 - ((sch(W, 0)[21 + k] + sch(W, 1)[21 + k]) + (sch(W, 2)[21 + k] + sch(W, 3)[21 + k])) : r0;
    }
    ldl6_factor(Lm, id, A);
    ldl6_solve(xb, Lm, id, r);
#pragma unroll
    for (int k = 0; k < 6; ++k) W.x[sp(k)] = xb[k];
}

/* The back substitution of leg l's two joints. */
HRL_DEV void leg_back(int l, Work &W) {
    float xb[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) xb[k] = W.x[sp(k)];
    const float *e = W.el[l];
    const float xh = e[1] * e[3] - dot6(e + 11, xb);
    const float xa = fma_(-e[4], xh, e[0] * e[2]) - dot6(e + 5, xb);
    W.x[6 + 2 * l] = xh; W.x[7 + 2 * l] = xa;
}

/* Entry i = r * nv + col of mass.  Both triangles read the one value computed for the pair. */
HRL_DEV float mass_entry(const DevCfg &c, const Work &W, int i) {
    const bool ant = c.kind != HRL_POINT_GATHER;
    const int r = ant ? i / HRL_DYN_NV_ANT : i / HRL_DYN_NV_POINT, col = ant ? i % HRL_DYN_NV_ANT : i % HRL_DYN_NV_POINT;
    const int lo = r < col ? r : col, hi = r < col ? col : r;
    if (hi < 6) return (ant || lo == hi) ? W.base[si(sp(lo), sp(hi))] : 0.f; /* the cube: diag(m, m, m, I, I, I) */
    if (lo < 6) return W.F[hi - 6][sp(lo)];
    const int jl = lo - 6, jh = hi - 6;
    if ((jl >> 1) != (jh >> 1)) return 0.f; /* joints of different legs do not couple */
    return W.Mj[jl >> 1][jl == jh ? ((jl & 1) ? 2 : 0) : 1];
}

HRL_DEV float bias_entry(const Work &W, int i) { return i < 6 ? W.base[21 + sp(i)] : W.bj[i - 6]; }

/* com [3], momentum [6], energy [2] */
struct Summary { float com[3], mom[6], en[2]; };

HRL_DEV void summary(const DevCfg &c, const float *st, const Work &W, Summary &o) {
    const float mt = c.kind == HRL_POINT_GATHER ? 10.f : fma_(4.f, c.m1 + c.m2, c.m0);
    float rG[3], P[3], rxP[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { rG[k] = W.tot[7 + k] / mt; P[k] = W.tot[3 + k]; o.com[k] = st[HRL_QPOS_OFF + k] + rG[k]; }
    cross3(rxP, rG, P);
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.mom[k] = P[k]; o.mom[3 + k] = W.tot[k] - rxP[k]; }
    o.en[0] = W.tot[6];
    o.en[1] = (mt * c.g) * o.com[2];
}

/* The linear Jacobian of a point fixed to `link` at (lx, ly, lz) in its frame: 3 x nv floats at J, row-major.  The point is links_core.h's
 * site: p = p0 + R(quat) local relative to O.  Columns: v -- the identity; omega -- e_m x p; the hip of the link's leg (upper body and
 * foot) -- Z x (p - ph); the ankle (foot) -- axw x (p - pa); the arms from the link's own anchor are R local itself, no difference of
 * sums.  Every other entry is +0.0. */
HRL_DEV void jac_site(const DevCfg &c, const float *st, int link, float lx, float ly, float lz, float *J) {
    const bool ant = c.kind != HRL_POINT_GATHER;
    const int nv = nv_of(c.kind);
    links::Link K;
    links::link_world(c, st, link, K);
    const bool centred = !ant || link <= 0 || link >= HRL_LINKS_ANT;
    const int type = centred || link >= 9 ? 0 : 1 + ((link - 1) & 1), l = centred || link >= 9 ? 0 : (link - 1) >> 1;
    Leg G;
    leg_kin(c, st, l, G);
    float X[3], Y[3], Z[3], r[3], p[3], dh[3], jh[3], ja[3];
    quat_axes(K.q[0], K.q[1], K.q[2], K.q[3], X, Y, Z);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = fma_(lz, Z[k], fma_(ly, Y[k], lx * X[k]));
        p[k] = K.p0[k] + r[k];
        dh[k] = pick(type == 2, (G.pa[k] - G.ph[k]) + r[k], r[k]);
    }
    cross3(jh, G.Z, dh);
    cross3(ja, G.axw, r);
    const float wp[3][3] = {{0.f, p[2], -p[1]}, {-p[2], 0.f, p[0]}, {p[1], -p[0], 0.f}}; /* wp[k][m] = (e_m x p)[k] */
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float *row = J + k * nv;
#pragma unroll
        for (int m = 0; m < 3; ++m) { row[m] = k == m ? 1.f : 0.f; row[3 + m] = wp[k][m]; }
        if (ant) {
#pragma unroll
            for (int ll = 0; ll < 4; ++ll) {
                row[6 + 2 * ll] = pick(type >= 1 && ll == l, jh[k], 0.f);
                row[7 + 2 * ll] = pick(type == 2 && ll == l, ja[k], 0.f);
            }
        }
    }
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_config *c, const hrl_dyn_spec *s) {
    if (!s) return "null dyn spec";
    if (s->struct_size != sizeof(hrl_dyn_spec)) return "hrl_dyn_spec.struct_size is not sizeof(hrl_dyn_spec): initialise the record with hrl_dyn_default_spec()";
    if (s->frame != HRL_DYN_WORLD) return "unknown dyn frame (world axes only)";
    if (s->n_sites < 0 || s->n_sites > HRL_DYN_MAX_SITES) return "dyn n_sites must be within 0..16";
    const int B = links::n_links(c->env_kind);
    for (int i = 0; i < s->n_sites; ++i) {
        if (s->site_link[i] < 0 || s->site_link[i] >= B) return "dyn site_link must be within 0..B-1 (B = 13 links for the ants, 1 for the point bot)";
        for (int k = 0; k < 3; ++k)
            if (!(fabsf(s->site_local[i][k]) <= 3.0e38f)) return "dyn site_local must be finite";
    }
    return "";
}
inline std::string validate_out(const hrl_dyn_out *o, const hrl_dyn_spec *s) {
    if (!o) return "null dyn out";
    if (o->jac && s->n_sites <= 0) return "dyn out.jac is given and the spec holds no site";
    if (!o->mass && !o->bias && !o->accel && !o->jac && !o->com && !o->momentum && !o->energy) return "dyn out holds no pointer: at least one output must be given";
    return "";
}

inline int default_spec(const hrl_config *c, hrl_dyn_spec *s) {
    static_assert(sizeof(hrl_dyn_spec) == sizeof(hrl_links_spec), "the site records are those of hrl_links_spec");
    if (!s || !c) return HRL_ERR_BAD_ARG;
    hrl_links_spec ls;
    const int rc = links::default_spec(c, HRL_LINKS_WORLD, &ls);
    if (rc != HRL_OK) return rc;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->frame = HRL_DYN_WORLD; s->n_sites = ls.n_sites;
    for (int i = 0; i < HRL_DYN_MAX_SITES; ++i) {
        s->site_link[i] = ls.site_link[i];
        for (int k = 0; k < 3; ++k) s->site_local[i][k] = ls.site_local[i][k];
    }
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, phase by phase as the kernel runs it. */
inline void dyn_env_host(const DevCfg &c, const float *st, const hrl_dyn_spec &sp_, const float *tau, const hrl_dyn_out &out, size_t env) {
    const bool ant = c.kind != HRL_POINT_GATHER;
    const int nv = nv_of(c.kind);
    Work W;
    memset(&W, 0, sizeof W);
    for (int i = 0; i < nv; ++i) W.tau[i] = tau ? tau[env * (size_t)nv + (size_t)i] : 0.f;
    const bool solve = out.accel != nullptr;
    for (int b = 0; b < (ant ? NB : 1); ++b) body_terms(c, st, b, W);
    if (ant)
        for (int l = 0; l < 4; ++l) leg_terms(c, st, l, solve, W);
    for (int k = 0; k < 27; ++k) base_terms(c, k, W);
    for (int k = 0; k < 10; ++k) total_terms(c, k, W);
    if (solve) {
        base_solve(c, W);
        if (ant)
            for (int l = 0; l < 4; ++l) leg_back(l, W);
    }
    if (out.mass)
        for (int i = 0; i < nv * nv; ++i) out.mass[env * (size_t)(nv * nv) + (size_t)i] = mass_entry(c, W, i);
    if (out.bias)
        for (int i = 0; i < nv; ++i) out.bias[env * (size_t)nv + (size_t)i] = bias_entry(W, i);
    if (out.accel)
        for (int i = 0; i < nv; ++i) out.accel[env * (size_t)nv + (size_t)i] = W.x[i];
    if (out.jac)
        for (int s = 0; s < sp_.n_sites; ++s)
            jac_site(c, st, sp_.site_link[s], sp_.site_local[s][0], sp_.site_local[s][1], sp_.site_local[s][2], out.jac + (env * (size_t)sp_.n_sites + (size_t)s) * (size_t)(3 * nv));
    Summary o;
    summary(c, st, W, o);
    for (int k = 0; k < 3; ++k)
        if (out.com) out.com[3 * env + k] = o.com[k];
    for (int k = 0; k < 6; ++k)
        if (out.momentum) out.momentum[6 * env + k] = o.mom[k];
    for (int k = 0; k < 2; ++k)
        if (out.energy) out.energy[2 * env + k] = o.en[k];
}
/* hrl_dyn on host pointers; returns the status and leaves the reason in `why` */
inline int dyn_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_dyn_spec *sp_, const float *tau, const uint8_t *mask, const hrl_dyn_out *out, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(cfg, sp_);
    if (why.empty()) why = validate_out(out, sp_);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    for (int e0 = 0; e0 < cfg->num_envs; e0 += GROUP) /* a workgroup's envs */
        for (int e = e0; e < e0 + GROUP && e < cfg->num_envs; ++e) {
            if (mask && !mask[e]) continue;
            dyn_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, *sp_, tau, *out, (size_t)e);
        }
    return HRL_OK;
}
#endif

}  // namespace dyn
}  // namespace hrl
