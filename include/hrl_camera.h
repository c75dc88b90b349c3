/*
 * hrl_camera.h -- C-ABI of the batched first-person camera: for every env of a shard a pinhole image as the robot sees it, H x W pixels of
 * depth (float, metres along the optical axis), segmentation (int32: which shape and which of its faces) and RGB (uint8), from one launch.
 *
 * The renderer (hrl_render.h) looks at the arena from above, the scanner (hrl_scan.h) along the ground plane.  This is the robot's own
 * forward-looking image, what the reference's users get from the simulator's getCameraImage one env at a time: a wall ahead, food at two
 * o'clock, the box's edge on the left, as pixels.  The image is a pure function of (hrl_config, the env's state / items / aux record,
 * hrl_camera_spec), specified operation by operation in csrc/camera_core.h and computed for all N envs by one kernel
 * (csrc/camera_hip.hip -> libhrl_camera_hip.so, a library of its own: the step library, the other sensor libraries and their ABIs are
 * untouched).  Every output stays in HBM.
 *
 * Shapes.  Everything the sensors know is a vertical prism: a ground-plan shape and a z-interval.  The ground-plan shapes are the
 * scanner's, slot for slot (hrl_scan.h: a wall is met at the arena's bounding line, the centre of the 0.1 thick wall):
 *   wall    the half plane beyond bounding line k, z in [ground_z, ground_z + 2.5] (wall.xml is 5 m tall and is loaded with its centre at
 *           z = 0, sizeable_enclosed_scene.py:47-57).  A half plane is entered once and never left: for an eye beyond the line the span
 *           is the whole ray
 *   box     the maze box, z in [box_lo z, box_hi z] = [0, 2]
 *   food / poison   cubes of half side 0.125 about (x, y, 0.1): z in [-0.025, 0.225]
 *   target  the disc of radius 0.2 stood up as a marker post, z in [ground_z, ground_z + 1].  THE REFERENCE DRAWS NO BODY FOR THE TARGET;
 *           the post is this camera's way of showing what the renderer paints as a disc (leave HRL_SCAN_TARGET out of `classes` for an
 *           image without it)
 *   ground  the plane z = ground_z (HRL_CAMERA_GROUND), seen from above only
 * The robot's own body is not drawn: the eye sits in it.  `items == NULL` leaves out the items and the flagrun target, as everywhere.
 *
 * Camera.  The eye stands over the torso's (x, y) (the cube's for the point bot) at z = ground_z + eye_height (HRL_EYE_GROUND) or at the
 * torso's z + eye_height (HRL_EYE_TORSO).  It yaws with `frame` (the scanner's forward vector: world +x, or the ground projection of the
 * torso's X axis) and neither pitches nor rolls -- gimbal-stabilised, like HRL_SCAN_HEADING and HRL_VIEW_EGO_HEADING.  With left =
 * (-forward_y, forward_x) and up = world +z, pixel (row i, column j) looks along
 *     forward + u_j * left + s_i * up,   u_j = (W - (2 j + 1)) / W * tan_half_h,   s_i = (H - (2 i + 1)) / H * tan_half_v
 * so column 0 is the leftmost and row 0 the top; W and H are even, so no column points exactly along forward and no row lies on the
 * horizon.  The tangents of the half fields of view are taken by the caller: the kernel evaluates no trigonometric function.
 *
 * Per pixel, t is the HORIZONTAL range along the column's ground-plan ray (the scanner's ray parameter) and m = s_i / sqrt(1 + u_j^2)
 * the rise per metre of it.  A shape whose ground plan the ray crosses over [t_in, t_out] with z-interval [zl, zh] is met
 *   - at t_in on its side, when the ray's height there, z(t_in) = eye_z + m t_in, is within [zl, zh] (face INSIDE when t_in = 0: the eye
 *     is in the shape; else SIDE_X / SIDE_Y for the face of a rectangle or wall whose normal is along world x / y, ROUND for the post);
 *   - else on its TOP at t = (zh - eye_z) / m, when z(t_in) > zh, the ray descends and t <= t_out;
 *   - else on its BOTTOM at t = (zl - eye_z) / m, when z(t_in) < zl, the ray climbs and t <= t_out.
 * The ground is met at t = (eye_z - ground_z) / -m by a descending ray from above it, and at t = 0 by an eye at or below it.  A
 * candidate counts if t <= max_range (the horizontal range, as in the scanner); the smallest t wins; equal t goes to the lower slot of the
 * table (planes 0..3, the box, the target, item 0, 1, ...), and every shape wins a tie with the ground.
 *
 * Outputs, [num_envs][height][width] (rgb: [...][3]):
 *   depth  t / sqrt(1 + u_j^2): the distance along the optical axis, as a depth camera reports it (a wall faced squarely has one depth);
 *          max_range where nothing was hit.  The point seen is eye + depth * (forward + u_j left + s_i up)
 *   seg    code | face << 16: the scanner's hit code (class | index << 8), HRL_HIT_GROUND, or HRL_HIT_NONE (face 0)
 *   rgb    the renderer's colour of the class with every channel * shade[face] >> 8, shade = {128, 224, 176, 200, 256, 96, 256} by
 *          face; HRL_RGB_SKY where nothing was hit
 *
 * Total: no address, loop bound or integer derives from a float.  Every acceptance test is a comparison that is false for NaN, so a
 * shape with a non-finite parameter is not seen; an env whose x, y or eye z is not finite (fabsf(v) <= 3e38 is false) sees nothing at
 * all: HRL_HIT_NONE, max_range and the sky on every pixel.  aux[3] is range-checked as an integer.
 */
#ifndef HRL_CAMERA_H
#define HRL_CAMERA_H

#include "hrl_render.h" /* HRL_RGB_* */
#include "hrl_scan.h"   /* HRL_SCAN_*, HRL_HIT_* */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_CAMERA_GROUND 64u /* a class bit next to HRL_SCAN_* (1..16) and HRL_FIELD_ROBOT (32): the plane z = ground_z */
#define HRL_HIT_GROUND 6      /* follows the scanner's hit codes 0..5; index 0 */

/* seg >> 16 */
#define HRL_FACE_INSIDE 0 /* the eye is in the shape's ground plan and z-interval: depth 0 */
#define HRL_FACE_SIDE_X 1 /* a vertical face whose normal is along world x */
#define HRL_FACE_SIDE_Y 2 /* ... along world y */
#define HRL_FACE_ROUND 3  /* the target post's mantle */
#define HRL_FACE_TOP 4
#define HRL_FACE_BOTTOM 5
#define HRL_FACE_GROUND 6

#define HRL_EYE_GROUND 0 /* eye z = ground_z + eye_height */
#define HRL_EYE_TORSO 1  /* eye z = the state's qpos z + eye_height */

#define HRL_RGB_SKY 150, 200, 255

#define HRL_CAMERA_MIN_WIDTH 16   /* width: a multiple of 16 ... */
#define HRL_CAMERA_MIN_HEIGHT 8   /* height: a multiple of 8 ... */
#define HRL_CAMERA_MAX_SIZE 128   /* ... up to 128 */
#define HRL_CAMERA_MAX_EYE_HEIGHT 10.0f
#define HRL_CAMERA_MIN_TAN 1e-3f  /* tan_half_h, tan_half_v within (1e-3, 1e3] */
#define HRL_CAMERA_MAX_TAN 1e3f

/* INITIALISE IT with hrl_camera_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_camera_spec) is refused. */
typedef struct hrl_camera_spec {
    uint64_t struct_size; /* sizeof(hrl_camera_spec) of the header the caller was compiled against */
    int32_t width;        /* W: columns, a multiple of 16 within 16..128 */
    int32_t height;       /* H: rows, a multiple of 8 within 8..128 */
    int32_t frame;        /* HRL_SCAN_WORLD or HRL_SCAN_HEADING: the scanner's forward vector */
    int32_t eye_mode;     /* HRL_EYE_* */
    float eye_height;     /* metres, finite, within 0..10 */
    float tan_half_h;     /* tangent of half the horizontal field of view; finite, within (1e-3, 1e3] */
    float tan_half_v;     /* tangent of half the vertical field of view; likewise (tan_half_h * H / W = square pixels) */
    float max_range;      /* metres of HORIZONTAL range; finite, > 0 */
    uint32_t classes;     /* a non-empty subset of HRL_SCAN_ALL | HRL_CAMERA_GROUND */
} hrl_camera_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_camera_out {
    float *depth; /* [num_envs][height][width] */
    int32_t *seg; /* [num_envs][height][width] */
    uint8_t *rgb; /* [num_envs][height][width][3] */
} hrl_camera_out;

/* 64 x 48 pixels in `frame`, tan_half_h = 1 (90 degrees), tan_half_v = 0.75 (square pixels), HRL_EYE_TORSO with eye_height 0.3 (0.4 for
 * the point bot, whose cube reaches 0.35 above its centre), every class and the ground, max_range = that of hrl_scan_default_spec (the
 * arena's diagonal). */
int hrl_camera_default_spec(const hrl_config *cfg, int32_t frame, hrl_camera_spec *spec);

/* The image of every env from bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL).  Envs with mask[i] == 0 (device, may be NULL: all) keep every byte.  Stateless: nothing but the tensors of `out` is written, no
 * handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_camera(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_camera_spec *spec, const uint8_t *mask, const hrl_camera_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_camera_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_CAMERA_H */
