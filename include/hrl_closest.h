/*
 * hrl_closest.h -- C-ABI of the batched closest points: for every env of a shard, how far every body of the robot is from everything it
 * could collide with, which two points are closest and along which normal, BEFORE anything touches -- what the reference's users get
 * from the simulator's getClosestPoints(bodyA, bodyB, distance) one pair at a time -- from one launch.
 *
 * The contact report (hrl_envs.h: record_contacts) names a pair only once it is inside the contact distance; the point probes
 * (hrl_probe.h) give a 2-D clearance of points, not bodies; the ray test (hrl_cast.h) needs a ray that points the right way.  This is
 * the continuous quantity behind the step's contact test: a foot's height, a leg's clearance from a wall, a cube or another leg.  Every
 * output is a pure function of (hrl_config, the env's state / items record, hrl_closest_spec), specified operation by operation in
 * csrc/closest_core.h and computed for all N envs by one kernel (csrc/closest_hip.hip -> libhrl_closest_hip.so, a library of its own:
 * the step library, the other sensor libraries and their ABIs are untouched).  Every output stays in HBM.
 *
 * Cells.  Per env, every link of hrl_links.h's order (B = 13 for the ants, 1 for the point bot) is asked for its nearest surface in each
 * of six classes, in this fixed order:
 *   0 HRL_CLOSEST_GROUND   the plane z = ground_z
 *   1 HRL_CLOSEST_WALL     the n_planes lateral planes the STEP collides with: the walls' INNER FACES, so a wall is 0.05 m nearer here
 *                          than the centre line the scanner (hrl_scan.h) and the ray test meet
 *   2 HRL_CLOSEST_BOX      the maze box [box_lo, box_hi], when the config holds one
 *   3 HRL_CLOSEST_FOOD     the item cubes i < n_food: half side 0.125 m, centred at (items[2 i], items[2 i + 1], 0.1)
 *   4 HRL_CLOSEST_POISON   the item cubes n_food <= i < n_food + n_poison.  The item set is the scanner's (the gather kinds, items
 *                          given, up to 64 of them), so the indices agree with hrl_scan.h and hrl_cast.h
 *   5 HRL_CLOSEST_SELF     exactly the step's 48 capsule pairs: the nine capsules of the three OTHER legs, never hip capsule against
 *                          hip capsule.  The torso and the point bot have no self class
 * The surfaces are what the step collides with, not the scanner's table.  The target post is no collision shape and is left out.  The
 * config's self_collision and item_collision do not matter: the query is geometric.
 *
 * Definitions.  O is the state's qpos x, y, z.  A link is its axis segment p0 - p1 (hrl_links.h's ends: the torso a segment of length
 * zero at O, a hip capsule O - hip, an aux body hip - ankle, a foot ankle - tip) with radius r = r_caps (the torso: r_torso).
 *   Box and items   t = the parameter of the axis point closest to the box (the step's seg_box_t on the axis in world coordinates, formed
 *                   as the step forms it); x = that point.  Outside the solid the distance is |x - clamp(x, lo, hi)| - r and n is that
 *                   vector normalised; where the axis runs through the solid, t is the middle of the stretch, the distance is -(depth
 *                   to the nearest face) - r and n is that face's normal.  on_link = x - r n, on_surface = x - (distance + r) n.
 *   Ground, walls   the signed height of each end is h = n . p - d (the ground: p_z - ground_z, n = (0, 0, 1)).  The end with the
 *                   smaller h wins, a tie goes to p1.  distance = h - r, on_link = p - r n, on_surface = p - h n.
 *   Self            the closest points c1, c2 of the two axes by the step's capsule_pair (Ericson 5.1.9 with the fixed squared lengths
 *                   0.08 / 0.32), evaluated IN THE STEP'S ORDER -- the capsule of the lower leg first -- so both links of a pair report
 *                   the same distance, bit for bit the step's.  With c the link's own point and c' the other's:
 *                   distance = |c - c'| - 2 r_caps, n = (c - c') / |c - c'|, (0, 0, 1) for a zero vector; on_link = c - r n,
 *                   on_surface = c' + r n.
 *   Point bot       the cube of half side 0.35 turned by the state's quaternion.  Ground and walls: the deepest of its 8 corners,
 *                   which is exact (distance = h, on_link = the corner, on_surface = corner - h n).  Boxes and item cubes: the least
 *                   of two corner sets, as the step tests them -- the player's 8 corners against the cube's box (on_link = the corner),
 *                   then the cube's 8 corners against the player's oriented box (on_surface = the corner).  THIS IS EXACT UNLESS THE
 *                   NEAREST FEATURES ARE TWO EDGES; THEN IT IS AN UPPER BOUND.
 *   Winner          the candidate with the least distance wins the cell; an exact fp32 tie goes to the lowest surface index (plane,
 *                   item) or link index; among the point bot's corners to the earlier corner, the player's before the cube's.
 *
 * Outputs, each optional (NULL = not computed), at least one must be given:
 *   distance    [num_envs][B][6]     the signed gap between the two surfaces, negative = penetration; +inf where the class has no
 *                                    surface, was not asked for, or nothing finite was found
 *   which       [num_envs][B][6]     the scanner's word, class in the low byte, index << 8: HRL_HIT_GROUND, HRL_HIT_WALL | plane << 8,
 *                                    HRL_HIT_BOX, HRL_HIT_FOOD / HRL_HIT_POISON | item << 8, HRL_HIT_ROBOT | other link << 8;
 *                                    HRL_HIT_NONE wherever distance is +inf
 *   on_link     [num_envs][B][6][3]  world coordinates of the closest point on the link's surface (the simulator's positionOnA)
 *   on_surface  [num_envs][B][6][3]  ... and on the other shape's (positionOnB)
 *   normal      [num_envs][B][6][3]  the unit normal from the surface towards the link
 * Where `which` is HRL_HIT_NONE the three vectors are zeros.
 *
 * Total: no address, loop bound or integer conversion derives from a float of the state or the items, except the guarded quadrant of
 * the joint angles' sine and cosine.  Every acceptance is a comparison that is false for NaN: a candidate counts if its distance d has
 * -1e30 < d < 1e30 (1e30 is the step's word for a sphere with a non-finite centre), so a candidate with a NaN or infinite distance is no
 * candidate.  An item cube with a non-finite coordinate is not there.  A link with a non-finite end (the point bot: a non-finite O or
 * axis) reports +inf / HRL_HIT_NONE in every class; the torso is a sphere about O, whatever the quaternion holds.  A NaN component of a
 * vector leaves as the one quiet NaN 0x7FC00000.  Nothing is culled.
 */
#ifndef HRL_CLOSEST_H
#define HRL_CLOSEST_H

#include "hrl_chase.h" /* HRL_CHASE_ROBOT, HRL_HIT_ROBOT (and hrl_camera.h: HRL_CAMERA_GROUND, HRL_HIT_GROUND; hrl_scan.h: HRL_SCAN_*, HRL_HIT_*; hrl_links.h: the links' order) */

#ifdef __cplusplus
extern "C" {
#endif

#define HRL_CLOSEST_GROUND 0
#define HRL_CLOSEST_WALL 1
#define HRL_CLOSEST_BOX 2
#define HRL_CLOSEST_FOOD 3
#define HRL_CLOSEST_POISON 4
#define HRL_CLOSEST_SELF 5
#define HRL_CLOSEST_CLASSES 6
#define HRL_CLOSEST_ALL (HRL_SCAN_WALL | HRL_SCAN_BOX | HRL_SCAN_FOOD | HRL_SCAN_POISON | HRL_CHASE_ROBOT | HRL_CAMERA_GROUND)

/* INITIALISE IT with hrl_closest_default_spec() (or zero the record, set struct_size = sizeof and every field): a record whose
 * struct_size is not sizeof(hrl_closest_spec) is refused. */
typedef struct hrl_closest_spec {
    uint64_t struct_size; /* sizeof(hrl_closest_spec) of the header the caller was compiled against */
    uint32_t classes;     /* a non-empty subset of HRL_CLOSEST_ALL: HRL_SCAN_WALL | BOX | FOOD | POISON | HRL_CHASE_ROBOT (self) | HRL_CAMERA_GROUND; HRL_SCAN_TARGET is refused */
    uint32_t reserved;    /* 0 */
} hrl_closest_spec;

/* DEVICE pointers, 4-byte aligned; NULL = not computed.  At least one must be given. */
typedef struct hrl_closest_out {
    float *distance;   /* [num_envs][B][6] */
    int32_t *which;    /* [num_envs][B][6] */
    float *on_link;    /* [num_envs][B][6][3] */
    float *on_surface; /* [num_envs][B][6][3] */
    float *normal;     /* [num_envs][B][6][3] */
} hrl_closest_out;

/* Every class. */
int hrl_closest_default_spec(const hrl_config *cfg, hrl_closest_spec *spec);

/* The cells of every env from bufs->state and bufs->items AS THEY ARE (device pointers of the step's layout; `items` may be NULL: no
 * items, as everywhere; bufs->aux must be given, as for every sensor).  Envs with mask[i] == 0 (device, may be NULL: all) keep every
 * byte.  Stateless: nothing but the tensors of `out` is written, no handle is needed, cfg is read at the call.  Asynchronous on `stream`
 * (a hipStream_t; NULL = the default stream).
 *
 * The device the pointers live on must be the current one (HRL_ERR_BAD_ARG otherwise, as in hrl_step).  The kernel constants derived
 * from a config are uploaded once per distinct (device, config) and kept for the life of the process, so a later launch with the same
 * config allocates and copies nothing and may be captured into a graph: THE FIRST CALL WITH A CONFIG MUST HAPPEN OUTSIDE CAPTURE.
 *
 * Errors (HRL_ERR_BAD_ARG and a message): a config hrl_create() would refuse, a bad spec, null or misaligned pointers, an `out` without
 * a single pointer, no device. */
int hrl_closest(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_closest_spec *spec, const uint8_t *mask, const hrl_closest_out *out, void *stream);

/* Last error text of the calling thread ("" if none). */
const char *hrl_closest_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HRL_CLOSEST_H */
