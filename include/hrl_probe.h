/*
 * hrl_probe.h -- C-ABI of the batched point probes: P query points per env of a shard, three questions per point, one launch.
 *
 * The range scanner (hrl_scan.h) asks about DIRECTIONS from the robot; the probe asks about PLACES: for a candidate subgoal, a
 * relabelled goal or a sampled start it answers how much room there is, whether the robot can see it, and how far it is around the maze
 * box.  The reference asks the second question for its one current target on the host (ant_maze_bullet_env.py get_target_sensor_obs:
 * "the box occludes the goal", segment_intersection over scene.box_bounds) and pays its distance reward on the straight line through
 * the box.  The probe is a pure function of (hrl_config, the env's state / items / aux record, hrl_probe_spec, the env's points),
 * specified operation by operation in csrc/probe_core.h and computed for all N envs by one kernel (csrc/probe_hip.hip ->
 * libhrl_probe_hip.so, a library of its own: the step library, the renderer, the scanner and their ABIs are untouched).  Every output
 * stays in HBM.
 *
 * Shapes: the renderer's (hrl_render.h) -- lateral plane k of the arena, the maze box, the target disc of radius 0.2, the food and poison
 * squares of half side 0.125 -- under the scanner's class bits and codes (HRL_SCAN_* / HRL_HIT_* of hrl_scan.h).  A WALL IS THE PLANE THE
 * ROBOT COLLIDES WITH and the renderer paints (+-4.95 and +-8.95 in a maze, +-(world_size / 2 - 0.05) in a gather arena): the probe
 * answers what the robot can touch.  (The scanner makes the opposite choice: it meets the wall's centre line 0.05 m further out, where
 * the reference's sense_walls meets it.)  `items == NULL` leaves out the items and the flagrun target, as in hrl_render and hrl_scan.
 *
 * Frames (spec.frame) -- what a query point (px, py) means:
 *   HRL_PROBE_WORLD    a world position
 *   HRL_PROBE_EGO      an offset from the robot's (x, y) (the torso's; the cube's for the point bot) in world axes
 *   HRL_PROBE_HEADING  an offset with x forward and y left: position = robot + px * forward + py * left, left = (-forward_y,
 *                      forward_x); forward follows the scanner's rule (HRL_SCAN_HEADING of hrl_scan.h): the normalised ground projection
 *                      of the torso's body X axis, world +x when the projection vanishes
 * The arithmetic is done in robot-centred coordinates, so an ego point's answers do not depend on how far from the origin the robot is.
 *
 * Outputs, each [N][P]; a NULL pointer = that output is not computed:
 *
 * 1. clearance (float) and nearest (int32): the signed distance from the point to the nearest kept shape (spec.classes) and that
 *    shape's code, class | index << 8.
 *      half plane  n . p + off: positive inside the arena
 *      rectangle   the usual signed distance, negative inside: with a = |p - c| - half sizes, |max(a, 0)| + min(max(ax, ay), 0)
 *      disc        |p - c| - r
 *    The smallest distance wins; equal distances stay with the lower slot (planes 0..3, the box, the target, item 0, 1, ...).  With no
 *    kept shape: +inf and 0.
 *
 * 2. sight (float) and blocker (int32): the segment from the robot's (x, y) to the point, of length L = |p - o|.  blocker = the code
 *    of the first kept shape the segment meets strictly before its end (ray parameter t < L, the scanner's intersections: t = 0 for a
 *    robot standing inside a shape or outside a plane), 0 when nothing is in the way; sight = that t, or L when nothing is in the way.
 *    (A point at the robot's own place has L = 0: nothing is before its end.)
 *
 * 3. path (float) and via (int32): the length of the shortest way from the robot to the point for a disc of radius spec.margin among
 *    the walls and the box.  Items and the target never block it, and spec.classes does not bear on it.
 *      free space    a point is free when every lateral plane gives n . p + off >= margin and the point is not strictly inside the box
 *                    grown by margin on every side (the BLOCKING RECTANGLE)
 *      corner nodes  the four corners of the box grown by margin + HRL_PROBE_SKIN; corner k = (+x, +y), (-x, +y), (-x, -y), (+x, -y).
 *                    A node counts only if every plane gives n . node + off >= margin (in the maze the box runs into the -x wall: only
 *                    the two +x corners count)
 *      blocked       a segment is blocked when it overlaps the INTERIOR of the blocking rectangle over a stretch of positive length (a
 *                    segment along the rectangle's edge is not); the skin keeps a segment that rounds a corner a millimetre clear of
 *                    that test, three orders above fp32 rounding at 10 m.  The arena is convex, so the planes block no segment between
 *                    free points
 *      snapping      the robot's end is moved into free space first: for plane 0, 1, 2, 3 in turn, if n . s + off < margin, along the
 *                    plane's normal by the deficit; if it is then strictly inside the blocking rectangle, out through the nearest side
 *                    (ties: +x, -x, +y, -y) to margin + HRL_PROBE_SKIN from the box.  The lengths of these moves are added to `path`
 *                    (an ant leaning on the box would otherwise be unreachable from everywhere)
 *      the answer    a query point that is not free: path = +inf, via = 0.  Otherwise the minimum of the direct segment from the
 *                    snapped start, if it is not blocked, and g[k] + |p - node_k| over the nodes whose segment to the point is not
 *                    blocked, where g[k] is the shortest length from the snapped start to node k over unblocked segments between
 *                    counted nodes.  Equal lengths stay with the direct segment, then the lower k.
 *      via           1 = straight; 2 + k = the route first turns at corner k (the first corner after the start); 0 = unreachable
 *    Without a box (gather, flagrun, flat) path is the straight length, or +inf outside the shrunk arena.
 *    (A point so far away that the square of its distance overflows fp32, beyond 1.8e19 m, is unreachable as well.)
 *
 * Total: no address or loop bound derives from a float.  A robot position or a query point with a non-finite coordinate (tested as
 * fabsf(x) <= 3e38 on the robot's x, y, on the point as given and on the point in robot-centred coordinates) gives clearance +inf,
 * nearest 0, sight 0, blocker 0, path +inf, via 0.  A shape with a non-finite parameter is not seen; every acceptance test is a
 * comparison that is false for NaN; aux[3] is range-checked as an integer.
 */
#ifndef HRL_PROBE_H
#define HRL_PROBE_H

#include "hrl_scan.h" /* the class bits HRL_SCAN_* and the codes HRL_HIT_* (and through it hrl_envs.h) */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_PROBE_WORLD 0   /* points are world positions */
#define HRL_PROBE_EGO 1     /* points are offsets from the robot in world axes */
#define HRL_PROBE_HEADING 2 /* points are offsets with x forward, y left */

#define HRL_PROBE_MAX_POINTS 512
#define HRL_PROBE_MAX_MARGIN 2.0f
#define HRL_PROBE_SKIN 1e-3f /* metres: how far beyond the blocking rectangle the corner nodes lie */

/* hrl_probe_out.via */
#define HRL_VIA_NONE 0     /* unreachable: path = +inf */
#define HRL_VIA_STRAIGHT 1 /* the direct segment */
#define HRL_VIA_CORNER0 2  /* 2 + k: the route first turns at corner k of the box */

/* INITIALISE IT with hrl_probe_default_spec() (or `hrl_probe_spec s = {sizeof s};` and every field): a record whose struct_size is not
 * sizeof(hrl_probe_spec) is refused. */
typedef struct hrl_probe_spec {
    uint64_t struct_size; /* sizeof(hrl_probe_spec) of the header the caller was compiled against */
    int32_t n_points;     /* P: 1..512, any integer */
    int32_t frame;        /* HRL_PROBE_* */
    uint32_t classes;     /* HRL_SCAN_WALL | ...: what clearance and sight see; 0 or an unknown bit is refused */
    float margin;         /* metres: the radius of the disc `path` moves; finite, within 0..2 */
} hrl_probe_spec;

/* DEVICE pointers, each [num_envs][n_points], 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_probe_out {
    float *clearance;
    int32_t *nearest;
    float *sight;
    int32_t *blocker;
    float *path;
    int32_t *via;
} hrl_probe_out;

/* 64 points in `frame`, all classes, margin = the torso's radius (0.25; the cube's half side 0.35 for the point bot). */
int hrl_probe_default_spec(const hrl_config *cfg, int32_t frame, hrl_probe_spec *spec);

/* The probes of env i at points[i][0 .. n_points - 1] (float [num_envs][n_points][2], DEVICE memory, 8-byte aligned) from bufs->state,
 * bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be NULL).  Envs with mask[i] == 0 (device,
 * may be NULL: all) keep their bytes.  Stateless: nothing but the tensors of `out` is written, no handle is needed, cfg is read at the
 * call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors: those of hrl_scan (a config hrl_create() would refuse, null or misaligned pointers, no device), a bad spec, a null `points`,
 * an `out` without a single pointer. */
int hrl_probe(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_probe_spec *spec, const float *points, const uint8_t *mask, const hrl_probe_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_probe_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_PROBE_H */
