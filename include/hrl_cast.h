/*
 * hrl_cast.h -- C-ABI of the batched ray test: for every env of a shard R rays of the CALLER'S, each a segment from `from` to `to` in
 * three dimensions, against the scene and the robot's own body -- what the reference's users get from the simulator's
 * rayTestBatch(from, to) one env at a time -- as the hit's fraction along the segment, the word that names what was met, the point and
 * the outward surface normal, from one launch.
 *
 * The scanner (hrl_scan.h) casts a flat ring of rays at shapes that are infinite in z and sees neither the robot nor the ground; the two
 * cameras (hrl_camera.h, hrl_chase.h) cast 3-D rays at exact solids, but from one eye per env through a pinhole, and report no normal.
 * This is the query for sensors of the caller's own: a range finder under each foot, a lidar that pitches and rolls with the torso, a
 * 3-D lidar pattern with elevation rings, depth and normal at a few chosen directions.  Every output is a pure function of (hrl_config,
 * the env's state / items / aux record, hrl_cast_spec, the env's rays, ray_link), specified operation by operation in csrc/cast_core.h
 * and computed for all N envs by one kernel (csrc/cast_hip.hip -> libhrl_cast_hip.so, a library of its own: the step library, the other
 * sensor libraries and their ABIs are untouched).  Every output stays in HBM.
 *
 * Rays.  `rays` is float [num_envs][n_rays][6]: from (3 floats) and to (3 floats) in the coordinates of `frame`.  With O the torso's
 * (the cube's) origin, the state's qpos x, y, z:
 *   HRL_CAST_WORLD    world positions
 *   HRL_CAST_EGO      offsets from O in world axes: the world position is O + v
 *   HRL_CAST_HEADING  offsets from O turned about world +z by the heading (hrl_links.h's: the normalised ground projection of the
 *                     torso's X axis, world +x where there is none): x forward, y left; the world position is
 *                     O + (f_x v_x - f_y v_y, f_y v_x + f_x v_y, v_z)
 *   HRL_CAST_LINK     coordinates in the body frame of a link: the world position is origin + v_x X + v_y Y + v_z Z with the link's
 *                     `origin` and the axes X, Y, Z of its `quat` as hrl_links() reports them in the world frame.  The link of ray r is
 *                     ray_link[r] (a device array of n_rays ints shared by all envs; NULL = link 0 for every ray); a value outside
 *                     0 .. B - 1 (B = 13 links for the ants, 1 for the point bot) means the ray meets nothing
 * The ray is X(t) = from + t D with D = to - from in world axes, NOT NORMALISED: t is the fraction, and a candidate counts if
 * 0 < t <= 1.
 *
 * Scene and robot are the chase camera's (hrl_chase.h), solid for solid: the scanner's shapes, slot for slot, as vertical prisms (walls
 * 2.5 m, the maze box, the item cubes, the target post of 1 m) -- the ray's ground-plan part crosses the ground-plan shape over
 * [t_in, t_out]; its height at t_in within the z-interval gives the side face (SIDE_X / SIDE_Y / ROUND) at t_in, above it a descending
 * ray meets the TOP at (zh - from_z) / D_z if that is <= t_out, below it a climbing ray the BOTTOM likewise; the ground z = ground_z,
 * met from above at (from_z - ground_z) / -D_z; the ant as the torso's sphere of radius 0.25 about O, and per capsule link (radius 0.08)
 * an OPEN CYLINDER from p0 to p1 and a BALL at its far end p1, so a joint ball names the proximal link; the point bot as one cube of half
 * side 0.35 about O turned by the state's quaternion, faces in BODY axes.  Class HRL_HIT_ROBOT, index = the link.
 *
 * Rules (the chase camera's, so the two agree where they overlap).  Candidates are tried in the order: scene slots in slot order
 * (planes 0..3, the box, the target, item 0, 1, ...), robot links in link order (per link the cylinder, then the ball), the ground.  A
 * candidate counts if 0 < t <= 1; the smallest t wins, an equal t stays with the earlier candidate.  ONLY SURFACES ENTERED FROM OUTSIDE
 * ARE MET: a ray that starts inside a solid does not see that solid (a prism whose ground plan and z-interval hold `from` yields t = 0,
 * which does not count; a sphere, a cylinder and the cube yield their entry root, which lies behind `from`).  A ray that starts at or
 * under the ground does not see the ground.  No shape is culled: every slot of the asked classes is tried for every ray.
 *
 * Outputs, each optional (NULL = not computed), at least one must be given:
 *   fraction  [num_envs][n_rays]     t of the hit, or 1.0 where nothing was met (the simulator's convention)
 *   seg       [num_envs][n_rays]     EXACTLY THE CHASE CAMERA'S WORD: class | index << 8 | face << 16 -- the scanner's hit code,
 *                                    HRL_HIT_GROUND, HRL_HIT_ROBOT (index = the link) or HRL_HIT_NONE.  The ground's tile parity is
 *                                    always 0: there is no checker here
 *   point     [num_envs][n_rays][3]  the hit in world coordinates, from + fraction D by one fused multiply-add per component; where
 *                                    nothing was met, `to` in world coordinates as the frame's formula above gives it
 *   normal    [num_envs][n_rays][3]  the outward surface normal at the hit in world axes, zeros where nothing was met.  By face:
 *                                    SIDE_X / SIDE_Y of a rectangle: -+ the axis, opposing the ray; a bounding wall's half plane: its
 *                                    inward normal; ROUND of a disc: the horizontal unit vector from the axis to the hit; TOP, the
 *                                    ground: (0, 0, 1); BOTTOM: (0, 0, -1); a sphere: (hit - centre) normalised; an open cylinder: the
 *                                    component of (hit - p0) orthogonal to the axis, normalised; the point bot's cube: -+ the body axis
 *                                    of the face (normalised), opposing the ray.  Computed once, for the winner
 *
 * Total: no address, loop bound or integer derives from a float of the state, the items or the rays, except the guarded quadrant of the
 * joint angles' sine and cosine (link_world); ray_link is compared with 0 and B before it picks a link.  Every acceptance test is a
 * comparison that is false for NaN: a shape or a link with a non-finite parameter is not met.  A ray meets NOTHING -- HRL_HIT_NONE,
 * fraction 1, a zero normal -- when it is null (to == from), when one of its six numbers or of their world forms is not finite, when
 * the env's O is not finite (IN EVERY FRAME: the scene's table is centred on the robot, so HRL_CAST_WORLD is no exception), when its
 * link is out of range, or when its link's frame is not finite (a non-finite joint angle takes the links beyond that joint, a non-finite
 * quaternion all of them).  The `point` of such a ray is `to` in world coordinates AS COMPUTED, WHICH MAY BE NON-FINITE
 * (+-inf, or NaN, always as the one quiet NaN 0x7FC00000); for a link out of range it is computed in link 0's frame.
 */
#ifndef HRL_CAST_H
#define HRL_CAST_H

#include "hrl_chase.h" /* HRL_CHASE_ALL, HRL_CHASE_ROBOT, HRL_HIT_ROBOT (and hrl_camera.h: HRL_CAMERA_GROUND, HRL_FACE_*; hrl_links.h: the links' order) */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_CAST_WORLD 0
#define HRL_CAST_EGO 1
#define HRL_CAST_HEADING 2
#define HRL_CAST_LINK 3
#define HRL_CAST_MAX_RAYS 1024

/* INITIALISE IT with hrl_cast_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_cast_spec) is refused.  (A from / to ray carries its own length: there is no max_range.) */
typedef struct hrl_cast_spec {
    uint64_t struct_size; /* sizeof(hrl_cast_spec) of the header the caller was compiled against */
    int32_t n_rays;       /* R: rays per env, 1..HRL_CAST_MAX_RAYS */
    int32_t frame;        /* HRL_CAST_WORLD, _EGO, _HEADING or _LINK: what the rays' coordinates mean */
    uint32_t classes;     /* a non-empty subset of HRL_CHASE_ALL: HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND */
    uint32_t reserved;    /* 0 */
} hrl_cast_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_cast_out {
    float *fraction; /* [num_envs][n_rays] */
    int32_t *seg;    /* [num_envs][n_rays] */
    float *point;    /* [num_envs][n_rays][3] */
    float *normal;   /* [num_envs][n_rays][3] */
} hrl_cast_out;

/* 64 rays in `frame`, every class. */
int hrl_cast_default_spec(const hrl_config *cfg, int32_t frame, hrl_cast_spec *spec);

/* The rays of every env against bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL: no items and no flagrun target, as everywhere).  `rays`: device, float [num_envs][n_rays][6], 8-byte aligned.  `ray_link`:
 * device, int32 [n_rays], 4-byte aligned, read under HRL_CAST_LINK only; may be NULL.  Envs with mask[i] == 0 (device, may be NULL: all)
 * keep every byte.  Stateless: nothing but the tensors of `out` is written, no handle is needed, cfg is read at the call.  Asynchronous
 * on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_cast(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_cast_spec *spec, const float *rays, const int32_t *ray_link, const uint8_t *mask, const hrl_cast_out *out,
             void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_cast_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_CAST_H */
