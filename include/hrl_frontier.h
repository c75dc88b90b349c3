/*
 * hrl_frontier.h -- C-ABI of the batched frontier map: for every env of a shard, on the world grid of the visibility map's memory
 * (hrl_see.h: `seen`), where the space the robot has seen ends, how far the nearest such place is through what it has seen, and which way
 * the route there starts.  One launch.
 *
 * The field (hrl_field.h) plans with an omniscient observer's geometry; the visibility map (hrl_see.h) keeps what the robot has seen so
 * far.  This map joins the two: cells are classified by knowledge as well as by geometry, the field's relaxation runs over the result, and
 * the answer is reduced to a few numbers per env -- frontier-based exploration as a subgoal generator, an exploration teacher, an
 * "episode fully explored" signal (count == 0), and optimistic replanning (the way to the target through what is known, unknown cells
 * counted free).  It is a pure function of (hrl_config, the env's state / items / aux record, hrl_frontier_spec, the env's bytes of
 * `seen`), specified operation by operation in csrc/frontier_core.h and computed for all N envs by one kernel (csrc/frontier_hip.hip ->
 * libhrl_frontier_hip.so, a library of its own: the step library, the other sensor libraries and their ABIs are untouched).  Every output
 * stays in HBM; `seen` is only read.
 *
 * Grid.  `width`, `height`, `centre` and `half_extent` are hrl_field_spec's in HRL_VIEW_WORLD (hrl_field.h): multiples of 8 within 8..64,
 * half_extent within (1e-3, 1e4], and the centre of cell (row i, column j) is the centre of the renderer's pixel (i, j).  There is no
 * ego mode: the memory exists on world grids only.  Give the map the grid the memory was written on.
 *
 * Per env:
 *   geometry   g(c) = the field's first value of the cell under `blocking`, `margin` and the class part of `sources` (HRL_FIELD_ROBOT |
 *              HRL_SCAN_FOOD | POISON | TARGET; it may be empty here): 0 on a class-source cell, +inf on a free cell, blocked otherwise
 *   robot      r = the cell the robot stands in: the lowest row and the lowest column whose centre lies within cell / 2 of the robot's
 *              place (<=, the field's test for a source cell).  r exists only when the robot's x, y are finite and lie inside the grid
 *   known      known(c) = seen[c] != 0 or c == r: the robot knows where it stands, also with a narrow field of view
 *   edge       edge(c) = known(c), g(c) is not blocked, and some orthogonal neighbour INSIDE the grid is not known.  The grid's rim is
 *              no edge
 *   value      an unknown cell is blocked under HRL_FRONTIER_KNOWN_ONLY; under HRL_FRONTIER_OPTIMISTIC it is 0 if it is a class source
 *              and free otherwise, whatever the geometry says.  A known cell is g(c).  Then 0 wherever edge(c) and `sources` holds
 *              HRL_FRONTIER_EDGE
 *   field      the field's graph, relaxation and codes (hrl_field.h: Graph, Outputs), unchanged, over these values
 *
 * Outputs; a NULL pointer = that output is not computed:
 *   edge   (uint8)  [N][H][W]  1 on an edge cell, else 0
 *   dist   (float)  [N][H][W]  as hrl_field_out.dist: 0 on source cells, +inf on blocked and unreached ones
 *   parent (uint8)  [N][H][W]  as hrl_field_out.parent: 0..7, HRL_FIELD_SOURCE, HRL_FIELD_UNREACHED, HRL_FIELD_BLOCKED
 *   count  (int32)  [N]        the number of edge cells; 0 = nothing is left to explore from what has been seen
 *   length (float)  [N]        dist at r; +inf without r, or with r blocked or unreached
 *   goal   (float)  [N][2]     the world x, y of the centre of the source cell the walk from r along `parent` ends on (at most W H steps);
 *                              NaN without r, or with r blocked or unreached
 *   cell   (int32)  [N]        row * width + column of that cell; -1 likewise
 *
 * Total: no address, loop bound or integer derives from a float of the state, and every test on a float is a comparison that is false
 * for NaN.  The bytes of `seen` are read as they are found: any non-zero byte counts as seen.
 */
#ifndef HRL_FRONTIER_H
#define HRL_FRONTIER_H

#include "hrl_route.h" /* through it hrl_field.h (HRL_FIELD_*), hrl_probe.h, hrl_scan.h (HRL_SCAN_*), hrl_render.h and hrl_envs.h */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_FRONTIER_EDGE 64u /* a source bit next to HRL_FIELD_ROBOT | HRL_SCAN_FOOD | POISON | TARGET: the edge cells */

#define HRL_FRONTIER_KNOWN_ONLY 0 /* hrl_frontier_spec.unknown: an unknown cell is blocked */
#define HRL_FRONTIER_OPTIMISTIC 1 /* ... is free (a source if a class source lies on it) */

/* INITIALISE IT with hrl_frontier_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose
 * struct_size is not sizeof(hrl_frontier_spec) is refused. */
typedef struct hrl_frontier_spec {
    uint64_t struct_size; /* sizeof(hrl_frontier_spec) of the header the caller was compiled against */
    int32_t width;        /* W: columns, a multiple of 8 within 8..64 */
    int32_t height;       /* H: rows, likewise */
    float centre[2];      /* world x, y of the grid's centre */
    float half_extent;    /* metres from the centre to the left and right edges; finite, within (1e-3, 1e4] */
    uint32_t blocking;    /* HRL_SCAN_WALL | ...: what is in the way; 0 or an unknown bit is refused */
    uint32_t sources;     /* HRL_FRONTIER_EDGE | HRL_FIELD_ROBOT | HRL_SCAN_FOOD | HRL_SCAN_POISON | HRL_SCAN_TARGET; 0 or another bit is refused */
    float margin;         /* metres: the radius of the disc that moves; finite, within 0..HRL_PROBE_MAX_MARGIN */
    int32_t unknown;      /* HRL_FRONTIER_KNOWN_ONLY or HRL_FRONTIER_OPTIMISTIC */
} hrl_frontier_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_frontier_out {
    uint8_t *edge;   /* [num_envs][height][width] */
    float *dist;     /* [num_envs][height][width] */
    uint8_t *parent; /* [num_envs][height][width] */
    int32_t *count;  /* [num_envs] */
    float *length;   /* [num_envs] */
    float *goal;     /* [num_envs][2] */
    int32_t *cell;   /* [num_envs] */
} hrl_frontier_out;

/* The grid, blocking and margin of hrl_field_default_spec(cfg, HRL_VIEW_WORLD) -- so the grid of hrl_see_default_spec(cfg,
 * HRL_VIEW_WORLD) --, sources = HRL_FRONTIER_EDGE, unknown = HRL_FRONTIER_KNOWN_ONLY. */
int hrl_frontier_default_spec(const hrl_config *cfg, hrl_frontier_spec *spec);

/* The map of every env from bufs->state, bufs->aux and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be
 * NULL) and from `seen` (device, [num_envs][height][width], 4-byte aligned, required, ONLY READ; it must not be the memory of `edge` or
 * `parent`).  Envs with mask[i] == 0 (device, may be NULL: all) keep their bytes.  Stateless: nothing but the tensors of `out` is
 * written, no handle is needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): those of hrl_field (a config hrl_create() would refuse, null or misaligned pointers, no
 * device, everything hrl_field refuses about the grid, the blocking and the margin); a bad sources or unknown; a null `seen`; `seen` the
 * same pointer as `edge` or `parent`; an `out` without a single pointer. */
int hrl_frontier(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_frontier_spec *spec, const uint8_t *seen, const uint8_t *mask, const hrl_frontier_out *out,
                 void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_frontier_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_FRONTIER_H */
