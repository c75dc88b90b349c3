/*
 * hrl_route.h -- C-ABI of the batched routes: for P start points per env of a shard the way to the nearest source of the env's navigation
 * field (hrl_field.h), pulled tight into a handful of waypoints, and its length.  One launch.
 *
 * The field answers "which cell next"; a high-level policy, a subgoal relabeller or an evaluation wants the way itself: a short polyline
 * to steer along and one number for the progress made.  The 8-connected chain of the field zig-zags, so its length over-estimates the
 * way (13.28 m from the maze's start to its evaluation target, where the exact way is 12.84 m); the pulled route does not.  The route is
 * a pure function of (hrl_config, the env's state / items / aux record, hrl_route_spec, the start point), specified operation by
 * operation in csrc/route_core.h and computed for all N envs by one kernel (csrc/route_hip.hip -> libhrl_route_hip.so, a library of its
 * own: the step library, the other sensors and their ABIs are untouched).  Every output stays in HBM.
 *
 * 1. Field.  width .. margin of the spec mean what they mean in hrl_field_spec, and the grid, its blocked cells, its source cells,
 *    `dist` and `parent` are those of hrl_field for these values.
 *
 * 2. Start cell.  A start (px, py) is given in one of the probe's frames (hrl_probe.h: HRL_PROBE_WORLD a world position, HRL_PROBE_EGO an
 *    offset from the robot in world axes, HRL_PROBE_HEADING an offset with x forward and y left).  With u, v its coordinates to the right
 *    of and up from the grid's centre (hrl_field.h), its column is the lowest j with |u - u_j| <= cell / 2 and its row the lowest i with
 *    |v - v_i| <= cell / 2: the test that makes a source cell of a source point, so a start on a source's point lies on a source cell.
 *    `starts == NULL`: every start is the robot's own place.
 *    THERE IS NO ROUTE when the start has no column or no row (outside the grid), when a coordinate of it is not finite (as given or in
 *    robot-centred coordinates, tested as fabsf(x) <= 3e38), when the robot's x or y is not finite, or when parent of the start cell is
 *    HRL_FIELD_BLOCKED or HRL_FIELD_UNREACHED.  Then count = 0, length = +inf, every entry of cells is -1 and every entry of waypoints NaN.
 *
 * 3. Chain.  c_0 = the start cell; c_{t+1} = c_t moved by the direction parent[c_t] (hrl_field.h); the chain ends at the first cell c_L
 *    whose parent is HRL_FIELD_SOURCE.  L < width * height.
 *
 * 4. Clear.  For cells a = (row i0, column j0) and b = (i1, j1) let di = i1 - i0, dj = j1 - j0.  clear(a, b) is true when no BLOCKED cell
 *    (i, j) with min(i0, i1) <= i <= max(i0, i1) and min(j0, j1) <= j <= max(j0, j1) satisfies
 *        2 |dj (i - i0) - di (j - j0)| <= |di| + |dj|
 *    -- the cells whose CLOSED square the segment between the two cell centres meets; a segment through a cell's corner meets that cell.
 *    Integers only.  This is the field's own rule against cutting corners: a step of the chain is always clear.
 *
 * 5. Pull (greedy, forwards).  The first waypoint is c_0, which is also the first anchor.  For t = 1 .. L: if clear(anchor, c_t) does not
 *    hold, c_{t-1} is the next waypoint and the new anchor.  c_L is the last waypoint.  A start on a source cell has the one waypoint c_0.
 *    Consecutive waypoints are clear of each other, so the polyline through the cell centres stays off every blocked cell.
 *
 * 6. Outputs; a NULL pointer = that output is not computed.  K = max_waypoints.
 *      count     (int32) [N][P]        the number of waypoints of the whole route, which may exceed K; 0 = no route
 *      cells     (int32) [N][P][K]     row * width + column of waypoint k for k < min(count, K); the entries from there up to K repeat the
 *                                      last one written
 *      waypoints (float) [N][P][K][2]  the world x, y of that cell's centre (padded likewise)
 *      length    (float) [N][P]        the sum over consecutive waypoints OF THE WHOLE ROUTE of fl(cell * sqrtf((float)(di di + dj dj))),
 *                                      accumulated in fp32 from the start onwards; 0 for a start on a source cell
 *
 * Total: no address, loop bound or integer derives from a float, and every test on a float is a comparison that is false for NaN.
 */
#ifndef HRL_ROUTE_H
#define HRL_ROUTE_H

#include "hrl_field.h" /* the field's constants; through it hrl_probe.h (HRL_PROBE_WORLD / EGO / HEADING), hrl_render.h and hrl_envs.h */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_ROUTE_MAX_STARTS 64
#define HRL_ROUTE_MIN_WAYPOINTS 2
#define HRL_ROUTE_MAX_WAYPOINTS 32

/* INITIALISE IT with hrl_route_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose struct_size
 * is not sizeof(hrl_route_spec) is refused. */
typedef struct hrl_route_spec {
    uint64_t struct_size; /* sizeof(hrl_route_spec) of the header the caller was compiled against */
    int32_t width;        /* these nine: hrl_field_spec's, with its bounds */
    int32_t height;
    int32_t mode;
    float centre[2];
    float half_extent;
    uint32_t blocking;
    uint32_t sources;
    float margin;
    int32_t n_starts;      /* P: 1..HRL_ROUTE_MAX_STARTS */
    int32_t frame;         /* HRL_PROBE_*: what a start point means */
    int32_t max_waypoints; /* K: HRL_ROUTE_MIN_WAYPOINTS..HRL_ROUTE_MAX_WAYPOINTS */
} hrl_route_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_route_out {
    float *waypoints; /* [num_envs][n_starts][max_waypoints][2] */
    int32_t *count;   /* [num_envs][n_starts] */
    float *length;    /* [num_envs][n_starts] */
    int32_t *cells;   /* [num_envs][n_starts][max_waypoints] */
} hrl_route_out;

/* hrl_field_default_spec(cfg, mode)'s field, one start in HRL_PROBE_EGO (an offset from the robot) and 16 waypoints. */
int hrl_route_default_spec(const hrl_config *cfg, int32_t mode, hrl_route_spec *spec);

/* The routes of env i from starts[i][0 .. n_starts - 1] (float [num_envs][n_starts][2], DEVICE memory, 4-byte aligned; NULL = the robot's
 * place n_starts times) on the field of bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items`
 * may be NULL).  Envs with mask[i] == 0 (device, may be NULL: all) keep their bytes.  Stateless: nothing but the tensors of `out` is
 * written, no handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors: those of hrl_field (a config hrl_create() would refuse, null or misaligned pointers, no device), a bad spec, an `out` without a
 * single pointer. */
int hrl_route(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_route_spec *spec, const float *starts, const uint8_t *mask, const hrl_route_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_route_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_ROUTE_H */
