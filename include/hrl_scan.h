/*
 * hrl_scan.h -- C-ABI of the batched range scanner: a ring of rays per env of a shard in one launch.
 *
 * The reference's envs see the world through coarse range sensors (sizeable_enclosed_scene.py:63-97 sense_walls, the food / poison
 * bins of the gather kinds), packed into the observation by the step.  This is their general form as a sensor of its own: a lidar ring
 * of any resolution, world-fixed or turning with the robot, that sees the walls, the maze box, food, poison and the target as FINITE
 * shapes and reports WHICH one each ray met.  The scan is a pure function of (hrl_config, the env's state / items / aux record,
 * hrl_scan_spec), specified operation by operation in csrc/scan_core.h and computed for all N envs by one kernel
 * (csrc/scan_hip.hip -> libhrl_scan_hip.so, a library of its own: the step library, the renderer and their ABIs are untouched).
 * `range` and `hit` stay in HBM.
 *
 * Origin: the torso's (x, y) (the cube's for the point bot), as the renderer's ego modes.
 * Forward: HRL_SCAN_WORLD: world +x.  HRL_SCAN_HEADING: the normalised ground projection of the torso's body X axis, by the renderer's
 *   rule (HRL_VIEW_EGO_HEADING of hrl_render.h: squared norm of the projection within [1e-12, 3e38]); when the projection vanishes the
 *   frame falls back to world axes, i.e. forward = world +x as in HRL_SCAN_WORLD.
 * Ray k points at angle theta_k = first_angle + k * step_angle, counter-clockwise from forward seen from above:
 *   direction = forward * cos(theta_k) + left * sin(theta_k),  left = (-forward_y, forward_x).
 *
 * Shapes (the renderer's, hrl_render.h, EXCEPT that a wall is met 0.05 m beyond the plane the renderer paints: a robot touching a
 * wall reads 0.05 there, not 0):
 *   wall    lateral plane k of the arena is a half plane: hit at its boundary from inside; range 0 when the origin is outside it.
 *           The boundary is the arena's bounding LINE k, where the reference's sense_walls meets it: +-world_size / 2 for the gather
 *           kinds and an enclosed flagrun arena, +-5 and +-9 for the maze kinds -- the centre of the 0.1 thick wall, 0.05 beyond the
 *           face the robot collides with and the renderer paints
 *   box     the maze box, a world-aligned rectangle: hit by slab test; range 0 when the origin is inside
 *   food / poison   world-aligned squares of half side 0.125 around the item's position; range 0 when the origin is inside
 *   target  the disc of radius 0.2 around the current target (the maze kinds; flagrun when `items` is given); range 0 inside
 * The robot's own body is not seen.  `items == NULL` leaves out the items and the flagrun target, as in hrl_render.
 *
 * A candidate counts if t <= max_range; the smallest t wins; equal t goes to the lower slot of the table
 * (planes 0..3, the box, the target, item 0, 1, ...).
 */
#ifndef HRL_SCAN_H
#define HRL_SCAN_H

#include "hrl_envs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_SCAN_WORLD 0   /* forward = world +x */
#define HRL_SCAN_HEADING 1 /* forward = the ground projection of the torso's body X axis (world +x when it vanishes) */

#define HRL_SCAN_MAX_RAYS 512
#define HRL_SCAN_MAX_ANGLE 64.0f /* |theta_k| of every ray: sincos_spec (csrc/step_core.h) is specified for |x| < 100 */

/* hrl_scan_spec.classes: what the rays see */
#define HRL_SCAN_WALL 1u
#define HRL_SCAN_BOX 2u
#define HRL_SCAN_FOOD 4u
#define HRL_SCAN_POISON 8u
#define HRL_SCAN_TARGET 16u
#define HRL_SCAN_ALL 31u

/* hit[i][k] = class code | index << 8 */
#define HRL_HIT_NONE 0   /* nothing within max_range: range = max_range */
#define HRL_HIT_WALL 1   /* index: the plane, 0..3 (the wall on the +x, -x, +y, -y side of the arena) */
#define HRL_HIT_BOX 2    /* index 0 */
#define HRL_HIT_FOOD 3   /* index: the item's slot in `items` (food slots come first) */
#define HRL_HIT_POISON 4 /* index: the item's slot in `items` (n_food ...) */
#define HRL_HIT_TARGET 5 /* index: the target's index (aux[3]) for the maze kinds, 0 for flagrun */

/* INITIALISE IT with hrl_scan_default_spec() (or `hrl_scan_spec s = {sizeof s};` and every field): a record whose struct_size is not
 * sizeof(hrl_scan_spec) is refused. */
typedef struct hrl_scan_spec {
    uint64_t struct_size;          /* sizeof(hrl_scan_spec) of the header the caller was compiled against */
    int32_t n_rays;                /* 1..512, any integer */
    int32_t frame;                 /* HRL_SCAN_* */
    float first_angle, step_angle; /* radians; every theta_k finite and at most 64 in magnitude */
    float max_range;               /* metres; finite, > 0 */
    uint32_t classes;              /* HRL_SCAN_WALL | ...; 0 or an unknown bit is refused */
} hrl_scan_spec;

/* 64 rays, a full circle centred on forward (first_angle = -pi + pi/64, step_angle = 2 pi/64), all classes, in `frame`.  max_range =
 * the arena's diagonal: sqrt(world_size[0]^2 + world_size[1]^2) for the gather kinds (21.2 at the default 15 x 15), sqrt(10^2 + 18^2)
 * = 20.6 for the maze kinds (maze_scene.py:10), (flag_size + 2) * sqrt(2) for flagrun (17.0 at the default, ant_flagrun_env.py:59-61),
 * and 10 for the flat kind, which has nothing to see. */
int hrl_scan_default_spec(const hrl_config *cfg, int32_t frame, hrl_scan_spec *spec);

/* range[i][k] (float, metres) and hit[i][k] (int32), DEVICE memory, [cfg->num_envs][spec->n_rays]: the scan of env i from bufs->state,
 * bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be NULL).  Envs with mask[i] == 0 (device,
 * may be NULL: all) keep their bytes.  Stateless: nothing but `range` and `hit` is written, no handle is needed, cfg is read at the
 * call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Total: no address or loop bound derives from a float of the state; every acceptance test is a comparison that is false for NaN, so a
 * shape with a non-finite parameter is not seen and a robot at a NaN place sees nothing (range = max_range, hit = 0).
 * Errors: a config hrl_create() would refuse, a bad spec, null or misaligned pointers. */
int hrl_scan(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_scan_spec *spec, const uint8_t *mask, float *range, int32_t *hit, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_scan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_SCAN_H */
