/*
 * cast_hip.hip -- gfx950 (MI355X) implementation of include/hrl_cast.h: libhrl_cast_hip.so.
 *
 * One workgroup of 256 threads answers the rays of one env, in the chase camera's layout (chase_hip.hip).  Its threads stage the env's
 * state, aux and items records in LDS.  Then lane = slot builds the scanner's table of 70 slots about the robot with the slots'
 * z-intervals (cast_core.h: build_slot), and, in the workgroup's last wave, lane = primitive evaluates links::link_world once per
 * primitive of the robot (25 at most) and writes its terms relative to O, and after it lane = link writes the 13 links' body frames for
 * HRL_CAST_LINK -- once per env, not per ray.  Two ballots give the list of walked slots and one more the list of drawn primitives --
 * wave-uniform, so they live in scalar registers and the walk's table reads are LDS broadcasts.  Then lane = ray: a wave takes 64
 * consecutive rays (the lanes past n_rays carry a ray that is not live and store nothing) and walks both lists in uniform control flow;
 * the primitives' list is skipped by a wave none of whose rays' lines passes the robot's bounding sphere (cast_core.h: near_robot, voted
 * with __any).
 *
 * A ray's six numbers arrive as three 8-byte loads (`rays` is 8-byte aligned and a ray is 24 bytes).  `fraction` and `seg` leave
 * lane = ray, 256 consecutive bytes per wave; `point` and `normal` as three 4-byte stores per lane at a stride of 12 bytes.  No barrier
 * follows the two of the prologue; n_rays and the pointers of `out` are kernel arguments, so both sit in uniform control flow; a masked
 * env returns as a whole workgroup before the first one.
 *
 * LDS: the table 1 688 B, its z-intervals 560 B, the primitives with their reach 1 792 B, the links' frames 832 B, the staged records
 * 656 B: about 5.5 KB a workgroup, so occupancy is bounded by waves, not by LDS.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "cast_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::cast;

namespace {

constexpr char LIB[] = "hrl_cast";
constexpr int BLOCK = 256;
static_assert(S_SLOTS <= BLOCK - 64 && PRIMS <= 64 && LINKS <= 64, "the slots' lanes and the primitives' wave are different threads");

__global__ __launch_bounds__(BLOCK) void cast_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const float *rays, const int32_t *ray_link,
                                                     const uint8_t *mask, hrl_cast_out out, hrl_cast_spec sp) {
    __shared__ ScanSet S;
    __shared__ PrimSet P;
    __shared__ LinkSet L;
    __shared__ float s_zl[S_SLOTS], s_zh[S_SLOTS];
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    __shared__ int32_t s_aux[HRL_AUX_STRIDE];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) s_aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) s_items[i] = items[(size_t)env * c.items_stride + i];
    const hrl_scan_spec ts = table_spec(sp);
    const int R = sp.n_rays; /* 1..MAX_RAYS: validate_spec */
    __syncthreads();
    const Base b = base_of(c, s_st);
    const Frame f = scan::table_frame(s_st);
    if (tid < S_SLOTS) build_slot(S, s_zl, s_zh, tid, c, s_st, items ? s_items : nullptr, s_aux, f, ts);
    if (tid >= BLOCK - 64) { /* (the last wave: no slot's lane) */
        if (lane < PRIMS) build_prim(P, lane, c, s_st, sp.classes);
        if (lane < LINKS) build_link(L, lane, c, s_st);
    }
    __syncthreads();
    const unsigned long long m0 = __ballot(scan::kept(S, lane)), m1 = __ballot(lane < S_SLOTS - 64 && scan::kept(S, lane < S_SLOTS - 64 ? 64 + lane : 0));
    const uint32_t pm = (uint32_t)__ballot(lane < PRIMS && chase::drawn(P, lane < PRIMS ? lane : 0));
    const float rb2 = chase::robot_bound(P, pm);
    const size_t base = (size_t)env * (size_t)R;
    const float2 *rays2 = reinterpret_cast<const float2 *>(rays); /* 8-byte aligned: hrl_cast's guard */
    for (int k0 = tid - lane; k0 < R; k0 += BLOCK) { /* whole waves: k0 is the wave's first ray, uniform over the wave */
        const int k = k0 + lane;
        const bool mine = k < R;
        float in[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; /* (a null ray: not live) */
        int link = 0;
        if (mine) {
            const size_t at = 3 * (base + (size_t)k); /* in float2 */
            const float2 a0 = rays2[at], a1 = rays2[at + 1], a2 = rays2[at + 2];
            in[0] = a0.x; in[1] = a0.y; in[2] = a1.x; in[3] = a1.y; in[4] = a2.x; in[5] = a2.y;
            if (sp.frame == HRL_CAST_LINK && ray_link) link = ray_link[k];
        }
        const Ray r = make_ray(c, b, L, sp.frame, in, link);
        const bool robot = __any(near_robot(rb2, r)); /* (a wave none of whose rays passes the robot skips its primitives) */
        Answer a;
        cast_ray(S, s_zl, s_zh, P, m0, m1, pm, robot, sp, b, r, a);
        if (mine) {
            const size_t at = base + (size_t)k;
            if (out.fraction) out.fraction[at] = a.fraction;
            if (out.seg) out.seg[at] = a.seg;
            if (out.point) { out.point[3 * at] = a.point[0]; out.point[3 * at + 1] = a.point[1]; out.point[3 * at + 2] = a.point[2]; }
            if (out.normal) { out.normal[3 * at] = a.normal[0]; out.normal[3 * at + 1] = a.normal[1]; out.normal[3 * at + 2] = a.normal[2]; }
        }
    }
}

}  // namespace

extern "C" {

int hrl_cast_default_spec(const hrl_config *cfg, int32_t frame, hrl_cast_spec *spec) {
    const int rc = default_spec(cfg, frame, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_cast_default_spec: null argument, bad env_kind or unknown frame");
}

int hrl_cast(const hrl_config *cfg, const hrl_buffers *b, const hrl_cast_spec *spec, const float *rays, const int32_t *ray_link, const uint8_t *mask, const hrl_cast_out *out,
             void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_rays(rays);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_cast: " + why);
    if (const int rc = check_record(LIB, b, "hrl_cast: null state or aux")) return rc;
    const Pointer ptrs[] = {{rays, "rays", 8}, {ray_link, "ray_link", 4}, {out->fraction, "fraction", 4}, {out->seg, "seg", 4}, {out->point, "point", 4}, {out->normal, "normal", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 6, &d_dc)) return rc;
    hipLaunchKernelGGL(cast_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, rays, ray_link, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_cast_last_error(void) { return g_err.c_str(); }

}  // extern "C"
