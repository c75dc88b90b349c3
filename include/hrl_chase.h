/*
 * hrl_chase.h -- C-ABI of the batched chase camera: for every env of a shard a pinhole image from a camera that orbits the robot at
 * `distance`, `yaw` and `pitch` and looks at it -- the third-person view with the robot's body in it -- as H x W pixels of depth (float,
 * metres along the optical axis), segmentation (int32: which shape or which link, and which face) and RGB (uint8), from one launch.
 *
 * The renderer (hrl_render.h) draws the legs as flat stadiums from straight above, the first-person camera (hrl_camera.h) sits on the
 * torso and shows no robot, the link states (hrl_links.h) are numbers.  This is the picture the reference's users get from
 * `env.render()` one env at a time: the simulator's camera behind and above the robot, the ant's legs moving on the ground.  The image
 * is a pure function of (hrl_config, the env's state / items / aux record, hrl_chase_spec), specified operation by operation in
 * csrc/chase_core.h and computed for all N envs by one kernel (csrc/chase_hip.hip -> libhrl_chase_hip.so, a library of its own: the
 * step library, the other sensor libraries and their ABIs are untouched).  Every output stays in HBM.
 *
 * Camera.  The point looked at is T = (x, y, z_T): the torso's (the cube's) x and y and z_T = the state's qpos z + target_height
 * (HRL_EYE_TORSO) or ground_z + target_height (HRL_EYE_GROUND).  With f the scanner's forward vector of `frame` (world +x, or the ground
 * projection of the torso's X axis), g = f turned by `yaw` about world +z, and p the pitch (negative looks down):
 *     F = (cos p g, sin p)      the optical axis
 *     L = (-g_y, g_x, 0)        left
 *     U = (-sin p g, cos p)     up
 *     E = T - distance F        the eye
 * `yaw` and `pitch` are handed over as (cos, sin) pairs: the kernel evaluates no trigonometric function of the spec.  Pixel (row i,
 * column j) looks along
 *     D = F + u_j L + s_i U,   u_j = (W - (2 j + 1)) / W * tan_half_h,   s_i = (H - (2 i + 1)) / H * tan_half_v
 * (hrl_camera.h's u_j and s_i: column 0 is the leftmost, row 0 the top).  D IS NOT NORMALISED: the ray is E + t D, so t is the depth
 * along the optical axis and `depth` = t.  The ground-plan part of D may vanish (pitch -90 degrees is a legal top-down perspective).
 *
 * Scene.  The scanner's shapes, slot for slot, as the vertical prisms of hrl_camera.h (walls 2.5 m, the maze box, the item cubes, the
 * target post of 1 m), met by general 3-D rays: the ray's ground-plan part crosses the ground-plan shape over [t_in, t_out]; the
 * height there, z(t_in) = E_z + D_z t_in, within the z-interval [zl, zh] gives the side face (SIDE_X / SIDE_Y / ROUND) at t_in; above
 * it a descending ray meets the TOP at (zh - E_z) / D_z if that is <= t_out; below it a climbing ray the BOTTOM likewise.  The ground
 * z = ground_z is met from above at (E_z - ground_z) / -D_z.  With tile > 0 the ground is a checkerboard: the index field of `seg` is
 * the parity of floor(x / tile) + floor(y / tile) at the hit point (0 where that is not finite), and parity 1 is drawn darker.
 *
 * Robot, class HRL_HIT_ROBOT, index = the link in hrl_links.h's order (hrl_links_name):
 *   ants       the torso is a sphere of radius 0.25 about the torso's origin O.  Each of the 12 capsule links (radius 0.08, from p0 to
 *              p1: hrl_links.h's capsule ends) is drawn as an OPEN CYLINDER from p0 to p1 and a BALL at its far end p1: 13 spheres and
 *              12 cylinders, whose union is exactly the union of the capsules.  A JOINT BALL THEREFORE NAMES THE PROXIMAL LINK: the
 *              ball between the hip capsule and `aux_1` is the hip capsule's, the one at the ankle is `aux_1`'s, the foot's own ball is
 *              its tip.  (Two-capped capsules would tie on every shared joint ball and rounding would pick the link.)  Face ROUND.
 *   point bot  one cube of half side 0.35 about O, turned by the state's quaternion; faces in BODY axes: SIDE_X, SIDE_Y, TOP (+z of
 *              the body), BOTTOM.
 * Only surfaces entered from outside are met: an eye inside a part of the robot does not see that part.
 *
 * Rules.  Candidates are tried in the order: scene slots in slot order (planes 0..3, the box, the target, item 0, 1, ...), robot links
 * in link order (per link the cylinder, then the ball), the ground.  A candidate counts if 0 < t <= max_range (the DEPTH, not the
 * distance); the smallest t wins, an equal t stays with the earlier candidate.  A solid that CONTAINS THE EYE is not drawn at all: its
 * ground plan contains the eye's ground position (for a wall: the eye is beyond the bounding line, outside the arena) and E_z lies in
 * its z-interval -- a camera that has swung through a wall or into the maze box looks out through it at the robot.  An eye at or under
 * the ground does not see the ground.
 *
 * Outputs, [num_envs][height][width] (rgb: [...][3]):
 *   depth  t; max_range where nothing was hit.  The point seen is E + depth * D
 *   seg    class | index << 8 | face << 16: the scanner's hit code, HRL_HIT_GROUND (index = the tile parity), HRL_HIT_ROBOT (index = the
 *          link), or HRL_HIT_NONE
 *   rgb    a pure integer function of seg: hrl_camera.h's colour of the scene classes; the ground of parity 1 times
 *          HRL_CHASE_TILE_SHADE >> 8 per channel; the robot in the renderer's HRL_RGB_TORSO (the torso, the cube), HRL_RGB_LEG0 (hip
 *          capsules), HRL_RGB_LEG1 (aux), HRL_RGB_LEG2 (feet), each times hrl_camera.h's shade[face] >> 8; HRL_RGB_SKY where nothing was hit
 *
 * Total: no address, loop bound or integer derives from a float of the state or the items, except the guarded quadrant of the joint
 * angles' sine and cosine and the guarded tile parity.  Every acceptance test is a comparison that is false for NaN: a shape or a link
 * with a non-finite parameter is not seen (a leg with a non-finite joint angle loses the links beyond that joint); an env whose T or E
 * is not finite sees nothing at all: HRL_HIT_NONE, max_range and the sky on every pixel.
 */
#ifndef HRL_CHASE_H
#define HRL_CHASE_H

#include "hrl_camera.h" /* HRL_CAMERA_GROUND, HRL_HIT_GROUND, HRL_FACE_*, HRL_EYE_*, HRL_RGB_SKY (and hrl_render.h, hrl_scan.h) */
#include "hrl_links.h"  /* the links' order */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_CHASE_ROBOT 32u /* the class bit of the robot's own body: hrl_field.h's HRL_FIELD_ROBOT, between HRL_SCAN_* and HRL_CAMERA_GROUND */
#define HRL_CHASE_ALL (HRL_SCAN_ALL | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND)
#define HRL_HIT_ROBOT 7     /* follows HRL_HIT_GROUND; index: the link */

#define HRL_CHASE_MIN_WIDTH 16  /* width: a multiple of 16 ... */
#define HRL_CHASE_MIN_HEIGHT 8  /* height: a multiple of 8 ... */
#define HRL_CHASE_MAX_SIZE 256  /* ... up to 256: an image is a multiple of 128 pixels */
#define HRL_CHASE_MIN_DISTANCE 0.5f
#define HRL_CHASE_MAX_DISTANCE 50.0f
#define HRL_CHASE_MAX_TARGET_HEIGHT 10.0f
#define HRL_CHASE_UNIT_TOL 1e-3f  /* |cos^2 + sin^2 - 1| of yaw and of pitch */
#define HRL_CHASE_MAX_TILE 1e6f
#define HRL_CHASE_TILE_SHADE 208  /* the ground of tile parity 1: every channel * 208 >> 8 */

/* INITIALISE IT with hrl_chase_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_chase_spec) is refused. */
typedef struct hrl_chase_spec {
    uint64_t struct_size; /* sizeof(hrl_chase_spec) of the header the caller was compiled against */
    int32_t width;        /* W: columns, a multiple of 16 within 16..256 */
    int32_t height;       /* H: rows, a multiple of 8 within 8..256 */
    int32_t frame;        /* HRL_SCAN_WORLD or HRL_SCAN_HEADING: the scanner's forward vector */
    int32_t target_mode;  /* HRL_EYE_TORSO: z_T = qpos z + target_height | HRL_EYE_GROUND: z_T = ground_z + target_height */
    float target_height;  /* metres, finite, within 0..10 */
    float yaw[2];         /* (cos, sin) of the camera's yaw about world +z, counted from `frame`'s forward; cos^2 + sin^2 within 1e-3 of 1 */
    float pitch[2];       /* (cos, sin) of the pitch, -90..+90 degrees, negative looks down: cos >= 0, cos^2 + sin^2 within 1e-3 of 1 */
    float distance;       /* metres from T to the eye, within 0.5..50 */
    float tan_half_h;     /* tangent of half the horizontal field of view; finite, within (1e-3, 1e3] */
    float tan_half_v;     /* tangent of half the vertical field of view; likewise (tan_half_h * H / W = square pixels) */
    float max_range;      /* metres of DEPTH along the optical axis; finite, > 0 */
    uint32_t classes;     /* a non-empty subset of HRL_CHASE_ALL */
    float tile;           /* metres, the side of the ground checker's squares, within 0..1e6; 0 = plain ground */
} hrl_chase_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_chase_out {
    float *depth; /* [num_envs][height][width] */
    int32_t *seg; /* [num_envs][height][width] */
    uint8_t *rgb; /* [num_envs][height][width][3] */
} hrl_chase_out;

/* 64 x 48 pixels in `frame`, yaw 0, pitch -30 degrees, distance 3 m, the torso as target (target_height 0), a horizontal field of view
 * of 60 degrees with square pixels, tile 1 m, every class, max_range = that of hrl_scan_default_spec (the arena's diagonal) + distance.
 * The angles, the distance and the field of view are those of upstream MJCFBaseBulletEnv.render (pybullet_envs) AS RECALLED, UNPINNED:
 * that package is not part of the reference tree and was not at hand to compare with. */
int hrl_chase_default_spec(const hrl_config *cfg, int32_t frame, hrl_chase_spec *spec);

/* The image of every env from bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL: no items and no flagrun target, as everywhere).  Envs with mask[i] == 0 (device, may be NULL: all) keep every byte.  Stateless:
 * nothing but the tensors of `out` is written, no handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t;
 * NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_chase(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_chase_spec *spec, const uint8_t *mask, const hrl_chase_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_chase_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_CHASE_H */
