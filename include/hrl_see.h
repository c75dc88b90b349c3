/*
 * hrl_see.h -- C-ABI of the batched visibility map: for every env of a shard a top-down grid of H x W cells that says, per cell, whether
 * the robot can see the cell's centre right now (`visible`), whether it has seen it so far in this episode (`seen`, a memory the CALLER
 * holds), and how many cells it saw for the first time in this call (`fresh`).  One launch.
 *
 * The renderer (hrl_render.h) and the field (hrl_field.h) describe the arena as an omniscient observer sees it: the image shows the target
 * behind the maze box, the field knows every poison cube.  The reference's own maze observation does not (get_target_sensor_obs blanks the
 * goal when the box occludes it).  This map is the missing mask, on the same grid: fog of war as rgb * visible[..., None], a count-based
 * exploration reward from `fresh`, a "known space" mask over the field, a partially observable maze.  The point probes (hrl_probe.h)
 * answer the same question for one point (`sight`, `blocker`); here it is asked of every cell centre of the field's grid, with the
 * episode's memory kept and counted in the same launch.  The map is a pure function of (hrl_config, the env's state / items / aux record,
 * hrl_see_spec, the bytes of `seen` and `clear`), specified operation by operation in csrc/see_core.h and computed for all N envs by one
 * kernel (csrc/see_hip.hip -> libhrl_see_hip.so, a library of its own: the step library, the other sensor libraries and their ABIs are
 * untouched).  Every output stays in HBM.
 *
 * Grid.  `width`, `height`, `mode`, `centre` and `half_extent` are exactly hrl_field_spec's (hrl_field.h): multiples of 8 within 8..64,
 * HRL_VIEW_*, half_extent within (1e-3, 1e4], and the centre of cell (row i, column j) is the centre of the renderer's pixel (i, j).  A
 * map, a field and an image of the same mode, size and extent line up cell for cell for pixel.
 *
 * Occluders.  The shapes are the probe's (hrl_probe.h): lateral plane k of the arena WHERE THE ROBOT COLLIDES WITH IT, the maze box, the
 * target disc, the food and poison squares, in the probe's robot-centred frame with world axes.  A shape occludes when the probe would
 * keep it under classes = `occluders` (its class bit is on and its parameters are finite).  `items == NULL` leaves out the items and the
 * flagrun target, as everywhere.  occluders = 0 is allowed: nothing occludes, and range and field of view alone decide.
 *
 * visible[i][j] = 1 when all of these hold, else 0.  q = the cell's centre relative to the robot, L = |q| and d = q / L as the probe
 * computes them (probe_core.h: segment), fwd = the scanner's forward vector in HRL_SCAN_HEADING (the ground projection of the torso's X
 * axis; world +x when it vanishes):
 *   - the robot's x and y are finite (tested as fabsf(x) <= 3e38) and q is finite: a robot without a finite place sees nothing, in
 *     every mode;
 *   - L <= max_range;
 *   - fov_cos <= -1, or not L > 0, or fma(fwd_x, d_x, fwd_y * d_y) >= fov_cos;
 *   - no occluding shape meets the ray from the robot along d at a parameter t < L - slack, t being the probe's (the scanner's
 *     isect_* functions: 0 when the origin is in the shape or outside a plane, +inf when the ray misses).
 * With slack = 0 this is exactly "the probe's `blocker` of the point is 0".  A slack of one cell lights the first layer of cells of a
 * wall or of the box, so a fogged image still shows the surface the robot is looking at.  THE SCANNER'S CONVENTION CARRIES OVER: a robot
 * standing inside an occluding shape, or outside a plane, meets it at t = 0 and sees nothing beyond `slack`.  An ant walks over food and
 * poison and stands on its target, which is why the default occluders are WALL | BOX.
 *
 * seen (read AND written; HRL_VIEW_WORLD only -- an ego grid moves under the memory).  With old = (clear && clear[env]) ? 0 :
 * (seen[k] != 0), seen[k] is written as old | visible[k], as 0 or 1: any non-zero byte found counts as seen.  `clear` is the episode's
 * reset flag, for instance the step's `done`.
 *
 * fresh[env] = the number of cells with visible == 1 and old == 0.  It needs `seen`.
 *
 * Total: no address, loop bound or integer derives from a float.  Every acceptance test is a comparison that is false for NaN; a shape
 * with a non-finite parameter does not occlude.  aux[3] is range-checked as an integer.
 */
#ifndef HRL_SEE_H
#define HRL_SEE_H

#include "hrl_field.h" /* HRL_FIELD_MIN_SIZE ...; through it hrl_probe.h (HRL_PROBE_MAX_MARGIN), hrl_scan.h (HRL_SCAN_*), hrl_render.h (HRL_VIEW_*) and hrl_envs.h */

#ifdef __cplusplus
extern "C" {
#endif

/* INITIALISE IT with hrl_see_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size is
 * not sizeof(hrl_see_spec) is refused. */
typedef struct hrl_see_spec {
    uint64_t struct_size; /* sizeof(hrl_see_spec) of the header the caller was compiled against */
    int32_t width;        /* W: columns, a multiple of 8 within 8..64 */
    int32_t height;       /* H: rows, likewise */
    int32_t mode;         /* HRL_VIEW_* */
    float centre[2];      /* world x, y of the grid's centre (HRL_VIEW_WORLD only) */
    float half_extent;    /* metres from the centre to the left and right edges; finite, within (1e-3, 1e4] */
    uint32_t occluders;   /* HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET; 0 = nothing occludes; an unknown bit is refused */
    float max_range;      /* metres; finite, > 0 */
    float fov_cos;        /* cosine of HALF the field of view about the robot's heading, within [-1, 1]; <= -1 = all round */
    float slack;          /* metres, within 0..HRL_PROBE_MAX_MARGIN: how far behind a surface a cell still counts as seen */
} hrl_see_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given; `visible` and `seen` must not be the same pointer. */
typedef struct hrl_see_out {
    uint8_t *visible; /* [num_envs][height][width], 0 or 1 */
    uint8_t *seen;    /* [num_envs][height][width], READ AND WRITTEN; HRL_VIEW_WORLD only */
    int32_t *fresh;   /* [num_envs]; needs `seen` */
} hrl_see_out;

/* The grid of hrl_field_default_spec(cfg, mode) (64 x 64, the renderer's default view), occluders = WALL | BOX, max_range = that of
 * hrl_scan_default_spec (the arena's diagonal), fov_cos = -1 (all round), slack = one cell, (2 / width) * half_extent. */
int hrl_see_default_spec(const hrl_config *cfg, int32_t mode, hrl_see_spec *spec);

/* The map of every env from bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL).  `clear` (device, [num_envs], may be NULL: none): envs whose memory starts from nothing in this call.  Envs with mask[i] == 0
 * (device, may be NULL: all) keep every byte, `seen` and `fresh` included.  Stateless: nothing but the tensors of `out` is written, no
 * handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): those of hrl_field (a config hrl_create() would refuse, null or misaligned pointers, no
 * device, everything hrl_field refuses about the grid); a bad occluders, max_range, fov_cos or slack; `seen` outside HRL_VIEW_WORLD;
 * `fresh` without `seen`; `visible` and `seen` the same pointer; an `out` without a single pointer. */
int hrl_see(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_see_spec *spec, const uint8_t *clear, const uint8_t *mask, const hrl_see_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_see_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_SEE_H */
