/*
 * hrl_dyn.h -- C-ABI of the batched dynamics terms: for every env of a shard the joint-space mass matrix, the bias force, the
 * contact-free acceleration, the linear Jacobians of points fixed to the robot's bodies, the centre of mass, the momenta and the energies,
 * from one launch.
 *
 * What a user of the reference asks the simulator one env at a time -- calculateMassMatrix, calculateInverseDynamics, calculateJacobian --
 * for a foot-placement controller (a Cartesian error through J^T), a computed-torque or gravity-compensated tracker (M and the bias
 * force), an energy or centroidal-momentum reward (T, V, P, L) and the mapping of contact forces to joint torques (J^T f).  The terms are
 * a pure function of (hrl_config, the env's state record, hrl_dyn_spec, tau), specified operation by operation in csrc/dyn_core.h and
 * computed for all N envs by one kernel (csrc/dyn_hip.hip -> libhrl_dyn_hip.so, a library of its own: the step library, the other
 * sensor libraries and their ABIs are untouched).  Every output stays in HBM.
 *
 * Coordinates.  The generalised velocity is the state's qvel in the state's own order: (v of O [3], omega in world axes [3], joint rates
 * [8]) -- O the torso's origin, the joints in the order hip 0, ankle 0, hip 1, ... of assets/ant.xml.  nv = HRL_DYN_NV_ANT = 14 for the
 * five ant kinds, nv = HRL_DYN_NV_POINT = 6 for the point bot.  The generalised force dual to it: (force [3], torque about O [3], joint
 * torques [8]).  World axes only.
 *
 * The model is the step's own (csrc/step_core.h: DevCfg::m0..b2, spatial_inertia, phase_kin_ankle): nine rigid bodies -- the torso (it
 * carries the four jointless hip capsules) and per leg the hinged upper body and the foot -- each a mass m and a central inertia
 * alpha 1 + beta e e^T about its capsule's axis e; the point bot's 10 kg cube of half extent 0.35 m.
 *
 * Outputs, float32:
 *   mass      [num_envs][nv][nv]  M(q) = sum over the bodies of J^T diag(m, I) J, plus model.joint_armature on the eight joint diagonals.
 *             One triangle is computed and mirrored: M[i][j] and M[j][i] hold the same bits.  Joints of different legs do not couple:
 *             those entries are +0.0.  The point bot: diag(m, m, m, I, I, I)
 *   bias      [num_envs][nv]      everything but the applied generalised force: Coriolis and centrifugal terms, gravity, Bullet's damping
 *             wrench of every body (force m v_c k_l (1 + |v_c|) at the centre of mass, torque (I_c omega) k_a (1 + |omega|); when
 *             model.linear_damping / angular_damping are not both zero) and model.joint_damping * rate on the joint rows.
 *             M udot + bias = tau describes the contact-free robot
 *   accel     [num_envs][nv]      udot = M^-1 (tau - bias): the classical derivative of qvel, what a finite difference of qvel over a
 *             contact-free step tends to.  By an L D L^T factorisation of M along the tree (ankle, hip, then the 6 x 6 base block)
 *   jac       [num_envs][n_sites][3][nv]  the linear Jacobian of the spec's sites: jac @ qvel is the site's velocity
 *   com       [num_envs][3]       the whole-body centre of mass G, world coordinates
 *   momentum  [num_envs][6]       linear momentum P [3], angular momentum about G [3]
 *   energy    [num_envs][2]       kinetic energy T of the nine bodies, potential energy V = M_total g z_G.  u^T M u / 2 is T plus
 *             joint_armature / 2 * |joint rates|^2: the armature is a term of M's diagonal, not a body
 *
 * tau: an optional input, [num_envs][nv] float32: the applied generalised force of `accel` (NULL = zeros).  The step applies
 * model.torque_scale * clip(action, -1, 1) on the joint rows and nothing on the base rows.
 *
 * Sites.  The records of hrl_links_spec: n_sites = 0..HRL_DYN_MAX_SITES points, the same for all envs; site s is site_local[s] in the
 * frame of link site_link[s] of include/hrl_links.h (13 links for the ants, the hip capsules among them; 1 for the point bot).
 *
 * Total: no address, loop bound or integer derives from a float of the state.  A NaN, an inf or a non-positive pivot of the
 * factorisation flows through the arithmetic into the outputs of its own env and nowhere else.  Except for `com` and V, every quantity is
 * computed relative to O and never adds the torso's position: moving a robot leaves their bits what they were.
 */
#ifndef HRL_DYN_H
#define HRL_DYN_H

#include "hrl_links.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_DYN_NV_ANT 14      /* generalised velocities of the five ant kinds */
#define HRL_DYN_NV_POINT 6     /* the point bot: a free cube */
#define HRL_DYN_MAX_SITES 16   /* == HRL_LINKS_MAX_SITES */

#define HRL_DYN_WORLD 0        /* the only frame: world axes */

/* INITIALISE IT with hrl_dyn_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_dyn_spec) is refused.  The layout is hrl_links_spec's. */
typedef struct hrl_dyn_spec {
    uint64_t struct_size;  /* sizeof(hrl_dyn_spec) of the header the caller was compiled against */
    int32_t frame;         /* HRL_DYN_WORLD */
    int32_t n_sites;       /* 0..HRL_DYN_MAX_SITES */
    int32_t site_link[HRL_DYN_MAX_SITES];     /* the first n_sites: a link of include/hrl_links.h, within 0..B-1 */
    float site_local[HRL_DYN_MAX_SITES][3];   /* the first n_sites: finite, in the link's frame */
} hrl_dyn_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given; jac with n_sites == 0 is refused. */
typedef struct hrl_dyn_out {
    float *mass;      /* [num_envs][nv][nv] */
    float *bias;      /* [num_envs][nv] */
    float *accel;     /* [num_envs][nv] */
    float *jac;       /* [num_envs][n_sites][3][nv] */
    float *com;       /* [num_envs][3] */
    float *momentum;  /* [num_envs][6] */
    float *energy;    /* [num_envs][2] */
} hrl_dyn_out;

/* nv of a kind (14 or 6); 0 for an unknown kind. */
int hrl_dyn_nv(int32_t env_kind);

/* The four foot tips as sites (hrl_links_default_spec's); the point bot: one site at the cube's centre. */
int hrl_dyn_default_spec(const hrl_config *cfg, hrl_dyn_spec *spec);

/* The dynamics terms of every env from bufs->state AS IT IS (a device pointer of the step's layout).  tau: device, [num_envs][nv],
 * 4-byte aligned, may be NULL (zeros); it is read only when out->accel is given.  Envs with mask[i] == 0 (device, may be NULL: all) keep
 * every byte.  Stateless: nothing but the tensors of `out` is written, no handle is needed, cfg is read at the call.  Asynchronous on
 * `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_dyn(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_dyn_spec *spec, const float *tau, const uint8_t *mask, const hrl_dyn_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_dyn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_DYN_H */
