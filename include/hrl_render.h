/*
 * hrl_render.h -- C-ABI of the batched top-down renderer: an RGB image of every env of a shard in one launch.
 *
 * The reference's envs answer `render('rgb_array')` through the simulator's camera (upstream MJCFBaseBulletEnv.render), one env at a
 * time.  Here the picture is a pure function of (hrl_config, the env's state / items / aux record, hrl_view), specified operation by
 * operation in csrc/render_core.h and computed for all N envs by one kernel (csrc/render_hip.hip -> libhrl_render_hip.so, a library of
 * its own: the step library and its ABI are untouched).  `rgb` stays in HBM: a policy's CNN or a video writer reads it there.
 *
 * The camera looks straight down (orthographic).  Pixel (row i, col j) of a W x H image has its centre at
 *     u = ((j + 0.5) * 2 / W - 1) * half_extent          (to the right)
 *     v = (H / W - (i + 0.5) * 2 / W) * half_extent      (up; row 0 is the top of the image)
 * and shows the world point  centre + u * right + v * up.  Pixels are square; half_extent is the distance from the centre to the
 * left / right edge of the image, so the top / bottom edges lie half_extent * H / W away.
 *
 * Layers, back to front (the last one that covers the pixel CENTRE wins; coverage is binary, nothing is blended):
 *   1 ground  2 outside of the arena (beyond any lateral wall plane)  3 the maze box  4 the current target, a disc of radius 0.2
 *   5 items: squares of half side 0.125, food slots first, then poison  6 the robot: ant = the twelve leg capsules as stadiums
 *   (per leg: torso -> hip point, hip -> ankle, ankle -> foot tip), then the torso disc; point bot = the quadrilateral of its cube's
 *   mid-plane square.
 */
#ifndef HRL_RENDER_H
#define HRL_RENDER_H

#include "hrl_envs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_VIEW_WORLD 0       /* a fixed camera at centre[2], world axes (x right, y up) */
#define HRL_VIEW_EGO 1         /* centred on the robot's x, y; world axes */
#define HRL_VIEW_EGO_HEADING 2 /* centred on the robot; up = the ground projection of the torso's body X axis (world axes when that projection vanishes) */

#define HRL_VIEW_MIN_SIZE 16   /* width and height: multiples of 16 (a lane writes 16 pixels = 48 bytes as three 16-byte stores) ... */
#define HRL_VIEW_MAX_SIZE 256  /* ... from 16 to 256 */

/* The palette, R, G, B (a documented part of the interface: consumers segment the image by colour). */
#define HRL_RGB_GROUND 240, 240, 240
#define HRL_RGB_WALL 60, 60, 60      /* outside of the arena */
#define HRL_RGB_BOX 170, 170, 170    /* the maze box */
#define HRL_RGB_TARGET 255, 200, 0
#define HRL_RGB_FOOD 0, 170, 0
#define HRL_RGB_POISON 210, 0, 0
#define HRL_RGB_LEG0 120, 80, 20     /* torso -> hip point */
#define HRL_RGB_LEG1 150, 100, 30    /* hip -> ankle */
#define HRL_RGB_LEG2 200, 140, 40    /* ankle -> foot tip */
#define HRL_RGB_TORSO 0, 50, 200     /* the ant's torso disc and the point bot's cube */

/* INITIALISE IT with hrl_render_default_view() (or `hrl_view v = {sizeof v};` and every field): a record whose struct_size is not
 * sizeof(hrl_view) is refused. */
typedef struct hrl_view {
    uint64_t struct_size; /* sizeof(hrl_view) of the header the caller was compiled against */
    int32_t width, height; /* pixels; multiples of 16 within 16..256 */
    int32_t mode;          /* HRL_VIEW_* */
    float centre[2];       /* HRL_VIEW_WORLD: the world point at the image centre (the ego modes ignore it) */
    float half_extent;     /* metres from the centre to the left / right image edge; finite, > 0 */
} hrl_view;

/* A 64 x 64 view of `cfg`'s kind.  HRL_VIEW_WORLD: the whole arena, centred on the origin -- half the larger world_size for the gather
 * kinds, 9 for the maze kinds (the 5 x 9 half extents of maze_scene.py:10), 6 for the flat kind, (flag_size + 2) / 2 for flagrun
 * (ant_flagrun_env.py:59-61).  The ego modes: 3 m around the robot. */
int hrl_render_default_view(const hrl_config *cfg, int32_t mode, hrl_view *view);

/* rgb[i][row][col][0..2] (uint8, DEVICE memory, 16-byte aligned) = the picture of env i < cfg->num_envs from bufs->state, bufs->aux and
 * bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be NULL: the flagrun target and the items are then left
 * out).  Envs with mask[i] == 0 (device, may be NULL: all) keep their bytes.  Stateless: nothing but `rgb` is written, no handle is
 * needed, cfg is read at the call.  Asynchronous on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 * Errors: a config hrl_create() would refuse, a bad view (sizes, mode, half_extent, struct_size), null or misaligned pointers. */
int hrl_render(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_view *view, const uint8_t *mask, uint8_t *rgb, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_render_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_RENDER_H */
