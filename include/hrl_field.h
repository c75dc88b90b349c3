/*
 * hrl_field.h -- C-ABI of the batched navigation field: for every env of a shard a top-down grid of H x W cells that holds, per cell,
 * the length of the shortest 8-connected way to the nearest source cell and the neighbour that way leaves through.  One launch.
 *
 * The point probes (hrl_probe.h) answer "how far is it round the maze box to THIS point"; the field answers "how far is it from
 * EVERYWHERE to where I want to go, and which way do I move": a reward potential, a scripted teacher (descend the field), a
 * path-length-normalised evaluation, or one more CNN channel that lines up pixel for pixel with hrl_render's image.  Unlike the probe's
 * `path` it avoids whatever `blocking` names (poison too), works in every arena and covers the whole grid.  The reference's dense reward
 * is walk_target_dist, the straight line through the box.  The field is a pure function of (hrl_config, the env's state / items / aux
 * record, hrl_field_spec), specified operation by operation in csrc/field_core.h and computed for all N envs by one kernel
 * (csrc/field_hip.hip -> libhrl_field_hip.so, a library of its own: the step library, the renderer, the scanner, the probes and their ABIs
 * are untouched).  Both outputs stay in HBM.
 *
 * Grid.  `width` x `height` cells, each a multiple of 8 within 8..64.  `mode`, `centre` and `half_extent` mean what they mean in hrl_view
 * (hrl_render.h), and the centre of cell (row i, column j) is the centre of the renderer's pixel (i, j), by the same formula:
 *     u_j = ((2 j + 1 - W) / W) * half_extent to the right of the view's centre, v_i = ((H - (2 i + 1)) / W) * half_extent up
 * so a field and an image of the same mode, size and extent cover the same ground.  A cell is cell = (2 / W) * half_extent metres wide.
 *
 * Blocking.  The shapes are the probe's (hrl_probe.h): lateral plane k of the arena WHERE THE ROBOT COLLIDES WITH IT, the maze box, the
 * target disc, the food and poison squares, under the scanner's class bits HRL_SCAN_*; `blocking` keeps the classes that are in the
 * way.  A cell is FREE when for every kept shape the probe's signed clearance of the cell's centre is >= margin: the field is that of a
 * disc of radius `margin`.  The clearances are computed in the probe's robot-centred frame (in HRL_VIEW_WORLD with a robot whose place is
 * not finite: centred on the world's origin).  `items == NULL` leaves out the items and the flagrun target, as everywhere.
 *
 * Sources.  `sources` names what the ways lead to: HRL_FIELD_ROBOT (the robot's x, y) and / or the centres of the kept shapes of the
 * classes HRL_SCAN_FOOD, HRL_SCAN_POISON, HRL_SCAN_TARGET.  The source cells of a source point are those whose centre lies within
 * cell / 2 of it on both axes of the grid (<=): one cell, two or four on an exact tie, none when the point lies outside the grid.  A
 * source cell is free whatever the blocking says (an ant leaning on the box must not be cut off from everything: the probe's reason for
 * snapping its start).
 *
 * Graph.  Direction codes 0..7 = E, NE, N, NW, W, SW, S, SE; N is row - 1 (up in the image), E is column + 1.  A step costs w1 = cell
 * (orthogonal) or w2 = cell * 1.41421354f (diagonal) and needs both of its cells free; a diagonal step also needs the two cells
 * orthogonally adjacent to both free, so no way cuts a corner.  Nothing lies beyond the grid's edge.
 *
 * Outputs, each [N][H][W]; a NULL pointer = that output is not computed:
 *   dist (float)    0 on source cells, +inf on blocked cells and on free cells no source is reachable from; elsewhere the fixed point of
 *                   d(c) = min over the admissible steps k of fl(d(neighbour_k) + w_k), fl = rounding to fp32.  The fixed point is unique
 *                   and independent of the order of relaxation (csrc/field_core.h says why), so it is the length, accumulated in fp32
 *                   from the source outwards, of the shortest way.
 *   parent (uint8)  0..7: the lowest direction code k with fl(d(neighbour_k) + w_k) == d(c), the step to take towards the source;
 *                   HRL_FIELD_SOURCE on a source cell, HRL_FIELD_UNREACHED on a free cell with dist = +inf, HRL_FIELD_BLOCKED on a
 *                   blocked one.
 *
 * Total: no address or loop bound derives from a float, and no integer is converted from one.  Every test is a comparison that is
 * false for NaN: a shape with a non-finite parameter is not seen (neither as an obstacle nor as a source), a cell whose centre is not
 * finite is blocked.  In the ego modes a robot with a non-finite x or y (tested as fabsf(x) <= 3e38) blocks every cell; in
 * HRL_VIEW_WORLD such a robot is not a source and the grid is otherwise what it is.  aux[3] is range-checked as an integer.
 */
#ifndef HRL_FIELD_H
#define HRL_FIELD_H

#include "hrl_probe.h" /* HRL_PROBE_MAX_MARGIN; through it hrl_scan.h (HRL_SCAN_*) and hrl_envs.h */
#include "hrl_render.h" /* HRL_VIEW_WORLD / EGO / EGO_HEADING */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_FIELD_ROBOT 32u /* a source bit next to HRL_SCAN_FOOD | POISON | TARGET: the robot's (x, y) */

#define HRL_FIELD_MIN_SIZE 8  /* width and height: multiples of 8 ... */
#define HRL_FIELD_MAX_SIZE 64 /* ... from 8 to 64 */
#define HRL_FIELD_MIN_HALF_EXTENT 1e-3f /* exclusive */
#define HRL_FIELD_MAX_HALF_EXTENT 1e4f  /* inclusive */

/* hrl_field_out.parent: 0..7 = E, NE, N, NW, W, SW, S, SE, and */
#define HRL_FIELD_SOURCE 8    /* a source cell: dist = 0 */
#define HRL_FIELD_UNREACHED 9 /* free, but no source is reachable: dist = +inf */
#define HRL_FIELD_BLOCKED 10  /* blocked: dist = +inf */

/* INITIALISE IT with hrl_field_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_field_spec) is refused. */
typedef struct hrl_field_spec {
    uint64_t struct_size; /* sizeof(hrl_field_spec) of the header the caller was compiled against */
    int32_t width;        /* W: columns, a multiple of 8 within 8..64 */
    int32_t height;       /* H: rows, likewise */
    int32_t mode;         /* HRL_VIEW_* */
    float centre[2];      /* world x, y of the grid's centre (HRL_VIEW_WORLD only) */
    float half_extent;    /* metres from the centre to the left and right edges; finite, within (1e-3, 1e4] */
    uint32_t blocking;    /* HRL_SCAN_WALL | ...: what is in the way; 0 or an unknown bit is refused */
    uint32_t sources;     /* HRL_FIELD_ROBOT | HRL_SCAN_FOOD | HRL_SCAN_POISON | HRL_SCAN_TARGET; 0, WALL, BOX or an unknown bit is refused */
    float margin;         /* metres: the radius of the disc that moves; finite, within 0..HRL_PROBE_MAX_MARGIN */
} hrl_field_spec;

/* DEVICE pointers, each [num_envs][height][width], 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_field_out {
    float *dist;
    uint8_t *parent;
} hrl_field_out;

/* The size and extent of hrl_render_default_view(cfg, mode) (64 x 64), blocking = WALL | BOX | POISON, margin = the torso's radius
 * (0.25; the cube's half side 0.35 for the point bot), sources = TARGET for the maze kinds and flagrun, FOOD for the gather kinds, ROBOT
 * for the flat kind. */
int hrl_field_default_spec(const hrl_config *cfg, int32_t mode, hrl_field_spec *spec);

/* The field of every env from bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL).  Envs with mask[i] == 0 (device, may be NULL: all) keep their bytes.  Stateless: nothing but the tensors of `out` is written, no
 * handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors: those of hrl_probe (a config hrl_create() would refuse, null or misaligned pointers, no device), a bad spec, an `out` without a
 * single pointer. */
int hrl_field(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_field_spec *spec, const uint8_t *mask, const hrl_field_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_field_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_FIELD_H */
