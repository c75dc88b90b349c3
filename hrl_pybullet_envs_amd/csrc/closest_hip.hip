/*
 * closest_hip.hip -- gfx950 (MI355X) implementation of include/hrl_closest.h: libhrl_closest_hip.so.
 *
 * One workgroup of 256 threads answers one env, in the ray test's layout (cast_hip.hip), in three stages.
 *   1  Its threads stage the env's state and items records in LDS and set the 78 cells' keys to "none".  Then lane = surface builds the
 *      table of 70 scene surfaces (closest_core.h: build_surf), and, in the workgroup's last wave, lane = link evaluates
 *      links::link_world once per link (13 lanes; the point bot: one) and writes its ends relative to O -- once per env, not per pair.
 *   2  lane = pair: the B x 83 (link, surface or other link) pairs are walked 256 at a time (five passes for an ant, one for the point
 *      bot); a pair that counts offers its key (distance, index) to its cell with ONE 64-BIT LDS MINIMUM (ds_min_u64, no return).  The
 *      key's unsigned order is a total order, so the cell's least key does not depend on the order in which the lanes arrive.
 *   3  lane = cell: the 78 (6) winners are evaluated once more for their points and normals, and stored: `distance` and `which`
 *      lane = cell, consecutive 4-byte stores; the three vectors as three 4-byte stores per lane at a stride of 12 bytes.
 *
 * Three barriers; the pointers of `out` are kernel arguments, so a NULL member costs nothing; a masked env returns as a whole workgroup
 * before the first barrier.  Every value leaves through ordinary vector stores.
 *
 * Measured (tools/kernel_resources.sh, -O2): 123 VGPRs, 0 bytes of scratch, 3 920 B of LDS a workgroup (the surfaces 2 016 B, the
 * links 640 B, the keys 624 B, the staged records 640 B): four waves per SIMD by registers, one workgroup of four waves per env.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "closest_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::closest;

namespace {

constexpr char LIB[] = "hrl_closest";
constexpr int BLOCK = 256;
static_assert(S_SCENE <= BLOCK - 64 && LINK_PAD <= 64 && CELLS <= BLOCK, "the surfaces' lanes and the links' wave are different threads; a cell per lane");

__global__ __launch_bounds__(BLOCK) void closest_kernel(const DevCfg *cfg, const float *state, const float *items, const uint8_t *mask, hrl_closest_out out, hrl_closest_spec sp) {
    __shared__ SurfSet S;
    __shared__ LinkSet L;
    __shared__ unsigned long long s_key[CELLS];
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    const int B = links::n_links(c.kind);
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 64 && tid < 64 + CELLS) s_key[tid - 64] = KEY_NONE;
    if (items)
        for (int i = tid; i < stride; i += BLOCK) s_items[i] = items[(size_t)env * c.items_stride + i];
    __syncthreads();
    if (tid < S_SCENE) build_surf(S, tid, c, items ? s_items : nullptr, sp.classes);
    if (tid >= BLOCK - 64 && lane < LINK_PAD) { /* (the last wave: no surface's lane) */
        if (lane < B) build_link(L, lane, c, s_st);
        else L.ok[lane] = 0u;
    }
    __syncthreads();
    for (int p = tid; p < B * S_ALL; p += BLOCK) {
        const int link = p / S_ALL, s = p - link * S_ALL;
        Cand o;
        int cls, idx;
        if (pair(c, s_st, L, S, sp.classes, link, s, &cls, &idx, o) && counts(o.d)) atomicMin(&s_key[link * CLASSES + cls], key_of(o.d, idx));
    }
    __syncthreads();
    if (tid < B * CLASSES) {
        const int link = tid / CLASSES, cls = tid - link * CLASSES;
        Answer a;
        answer(c, s_st, L, S, sp.classes, link, cls, s_key[tid], a);
        const size_t at = (size_t)env * (size_t)(B * CLASSES) + (size_t)tid;
        if (out.distance) out.distance[at] = a.distance;
        if (out.which) out.which[at] = a.which;
        if (out.on_link) { out.on_link[3 * at] = a.on_link[0]; out.on_link[3 * at + 1] = a.on_link[1]; out.on_link[3 * at + 2] = a.on_link[2]; }
        if (out.on_surface) { out.on_surface[3 * at] = a.on_surface[0]; out.on_surface[3 * at + 1] = a.on_surface[1]; out.on_surface[3 * at + 2] = a.on_surface[2]; }
        if (out.normal) { out.normal[3 * at] = a.normal[0]; out.normal[3 * at + 1] = a.normal[1]; out.normal[3 * at + 2] = a.normal[2]; }
    }
}

}  // namespace

extern "C" {

int hrl_closest_default_spec(const hrl_config *cfg, hrl_closest_spec *spec) {
    const int rc = default_spec(cfg, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_closest_default_spec: null argument or bad env_kind");
}

int hrl_closest(const hrl_config *cfg, const hrl_buffers *b, const hrl_closest_spec *spec, const uint8_t *mask, const hrl_closest_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_closest: " + why);
    if (const int rc = check_record(LIB, b, "hrl_closest: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->distance, "distance", 4}, {out->which, "which", 4}, {out->on_link, "on_link", 4}, {out->on_surface, "on_surface", 4}, {out->normal, "normal", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 5, &d_dc)) return rc;
    hipLaunchKernelGGL(closest_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_closest_last_error(void) { return g_err.c_str(); }

}  // extern "C"
