/*
 * hrl_links.h -- C-ABI of the batched link states: for every env of a shard the pose and the velocity of every rigid body of the robot,
 * and of caller-defined points fixed to those bodies, from one launch.
 *
 * What the reference's users read one env at a time through the simulator's getLinkState -- `robot.parts[name]`, `robot.feet[i]`,
 * `parts['torso'].get_pose()` / `get_velocity()` -- for foot-placement and gait rewards, foot-height observations and skeleton overlays.
 * The states are a pure function of (hrl_config, the env's state record, hrl_links_spec), specified operation by operation in
 * csrc/links_core.h and computed for all N envs by one kernel (csrc/links_hip.hip -> libhrl_links_hip.so, a library of its own: the step
 * library, the other sensor libraries and their ABIs are untouched).  Every output stays in HBM.
 *
 * Links.  B = HRL_LINKS_ANT = 13 for the five ant kinds, B = HRL_LINKS_POINT = 1 for the point bot (the cube: its pose and velocity are
 * the state's as they are).  The ant's links, leg l = 0..3 in the order of assets/ant.xml:15-58:
 *     0        torso                                       `torso`
 *     1 + 2 l  the hinged upper body of leg l              `aux_1` .. `aux_4`
 *     2 + 2 l  the foot of leg l                           `front_left_foot`, `front_right_foot`, `left_back_foot`, `right_back_foot`
 *     9 + l    the jointless hip capsule, rigid to torso   `front_left_leg`, `front_right_leg`, `left_back_leg`, `right_back_leg`
 * Indices 0..8 are the body order of the contact report (contacts.body_of_link / link_force); the 13 are upstream's `parts`.
 * hrl_links_name(kind, i) gives the names.
 *
 * With O the torso's origin (qpos x, y, z), X, Y, Z the columns of the torso's rotation matrix, and ph / pa / tip the hip point, the ankle
 * point and the foot tip of leg l relative to O -- THE STEP'S OWN POINTS, by the step's own operations (csrc/step_core.h:
 * phase_kin_ankle) -- a link is the capsule from p0 to p1:
 *     hip capsule  p0 = 0,  p1 = ph        aux  p0 = ph, p1 = pa        foot  p0 = pa, p1 = tip
 *
 * Outputs, [num_envs][B][3] ([4] for quat):
 *   origin   the link frame's origin, the joint anchor: O for the torso and the hip capsules (the state's bits), O + p0 for aux and foot
 *   com      the centre of mass: O for the torso, else the capsule's midpoint 0.5 * (origin + (O + p1)).  The simulator's
 *            getLinkState()[0] is the centre of mass, so this is what upstream's `parts[name].get_position()` answers.  The capsule's far
 *            end is 2 com - origin (up to the rounding of the midpoint's sum)
 *   quat     (x, y, z, w): the MJCF BODY frame -- q_torso for the torso and the hip capsules, q_torso * Rz(hip angle) for aux, that *
 *            R(ankle axis, ankle angle) for the foot: a product of the state's quaternion AS STORED, with no normalisation.  The
 *            simulator reports the orientation of a link's INERTIAL frame, which its importer chooses (the capsule's principal axes);
 *            nothing here pins that frame and this is not it: rotate the capsule's local `fromto` direction by quat instead
 *   lin_vel  the velocity of the centre of mass
 *   ang_vel  the angular velocity, world axes
 *   site_pos, site_vel  [num_envs][n_sites][3], see Sites
 *
 * Velocities come from the state's qvel (v of O, omega, joint rates) with the spatial velocities of phase_kin_ankle, (angular, linear at
 * O): torso (omega, v); aux = torso + Sh * hip rate, Sh = (Z, ph x Z); foot = aux + Sa * ankle rate, Sa = (axw, pa x axw) with axw the
 * ankle's axis in world axes.  The velocity of a point p (relative to O) carried by a body is its linear part + its angular part x p.
 *
 * Sites.  n_sites = 0..HRL_LINKS_MAX_SITES points, the same for all envs: site s is site_local[s] in the frame of link site_link[s] -- the
 * `localPosition` of getLinkState: a foot pad, a sensor mount.  Its position is origin[link] + R(quat[link]) * local, R the rotation
 * matrix of quat by the step's quat_axes; its velocity that of the point as carried by the link.
 *
 * Frame.  HRL_LINKS_WORLD: world coordinates.  HRL_LINKS_HEADING: positions relative to O, and every vector turned by minus the heading
 * (the scanner's forward vector of HRL_SCAN_HEADING: the ground projection of the torso's X axis); quat is multiplied from the left by
 * the inverse yaw quaternion.  Velocities stay absolute -- they are not relative to the torso's -- and are only turned.
 *
 * Total: no address, loop bound or integer derives from a float of the state.  NaN and inf flow through to the outputs of their own env
 * and to nothing else.
 */
#ifndef HRL_LINKS_H
#define HRL_LINKS_H

#include "hrl_envs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_LINKS_ANT 13       /* links of the five ant kinds */
#define HRL_LINKS_POINT 1      /* the point bot: the cube */
#define HRL_LINKS_MAX 13
#define HRL_LINKS_MAX_SITES 16

#define HRL_LINKS_WORLD 0
#define HRL_LINKS_HEADING 1    /* == HRL_SCAN_HEADING */

#define HRL_LINK_TORSO 0
#define HRL_LINK_AUX(l) (1 + 2 * (l))
#define HRL_LINK_FOOT(l) (2 + 2 * (l))
#define HRL_LINK_HIP(l) (9 + (l))

/* INITIALISE IT with hrl_links_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_links_spec) is refused. */
typedef struct hrl_links_spec {
    uint64_t struct_size;  /* sizeof(hrl_links_spec) of the header the caller was compiled against */
    int32_t frame;         /* HRL_LINKS_WORLD or HRL_LINKS_HEADING */
    int32_t n_sites;       /* 0..HRL_LINKS_MAX_SITES */
    int32_t site_link[HRL_LINKS_MAX_SITES];     /* the first n_sites: within 0..B-1 */
    float site_local[HRL_LINKS_MAX_SITES][3];   /* the first n_sites: finite, in the link's frame */
} hrl_links_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given (site_pos / site_vel count only with n_sites > 0). */
typedef struct hrl_links_out {
    float *origin;   /* [num_envs][B][3] */
    float *com;      /* [num_envs][B][3] */
    float *quat;     /* [num_envs][B][4] */
    float *lin_vel;  /* [num_envs][B][3] */
    float *ang_vel;  /* [num_envs][B][3] */
    float *site_pos; /* [num_envs][n_sites][3] */
    float *site_vel; /* [num_envs][n_sites][3] */
} hrl_links_out;

/* The number of links of a kind (13 or 1); 0 for an unknown kind. */
int hrl_links_count(int32_t env_kind);

/* The name of link i of a kind as assets/ant.xml spells it ("cube" for the point bot); NULL outside 0..B-1. */
const char *hrl_links_name(int32_t env_kind, int32_t i);

/* `frame`, and the four foot tips as sites: link 2 + 2 l, local = the far end of the foot capsule's `fromto` (+-0.4, +-0.4, 0).  The
 * point bot: one site at the cube's centre. */
int hrl_links_default_spec(const hrl_config *cfg, int32_t frame, hrl_links_spec *spec);

/* The link states of every env from bufs->state AS IT IS (a device pointer of the step's layout).  Envs with mask[i] == 0 (device, may be
 * NULL: all) keep every byte.  Stateless: nothing but the tensors of `out` is written, no handle is needed, cfg is read at the call.
 * Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_links(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_links_spec *spec, const uint8_t *mask, const hrl_links_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_links_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_LINKS_H */
