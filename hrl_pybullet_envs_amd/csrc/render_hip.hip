/*
 * render_hip.hip -- gfx950 (MI355X) implementation of include/hrl_render.h: libhrl_render_hip.so.
 *
 * One 256-thread workgroup paints one env.  Its first 96 threads build the env's table of primitives (render_core.h: lane = slot, in
 * view coordinates, each with its bounding box) in 5 KB of LDS.  Each of the four waves then takes runs of 64 strips (a strip = 16
 * horizontally adjacent pixels; at 64 x 64 a run is a band of 16 rows, and the four waves cover the image in one pass): lane = slot
 * tests the slot's box against the run's box, two ballots give the run's list, and every lane walks only the set bits, in slot order
 * = painter's order, for the 16 pixels of its strip -- all ~80 primitives at every pixel would be ~1.3e12 coverage tests per
 * 4096 x 64 x 64 frame.  The list is wave-uniform (it lives in scalar registers, the table reads are LDS broadcasts), the 16 colours of
 * a strip live in registers under fully unrolled loops (no scratch), and a lane stores its 48 bytes as three 16-byte vectors; the
 * lanes of a wave write 3 KB of consecutive addresses.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "render_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::render;

namespace {

constexpr char LIB[] = "hrl_render";
constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void render_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *mask,
                                                       uint8_t *rgb, hrl_view view) {
    __shared__ PrimSet S;
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    __shared__ int32_t s_aux[HRL_AUX_STRIDE];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 64 && tid < 64 + HRL_AUX_STRIDE) s_aux[tid - 64] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 64)];
    if (items && tid >= 128 && tid - 128 < stride) s_items[tid - 128] = items[(size_t)env * c.items_stride + (tid - 128)];
    __syncthreads();
    if (tid < R_SLOTS) {
        const Frame f = view_frame(view, s_st);
        if (tid == 0) store_frame(S, f);
        Prim P;
        make_prim(P, tid, c, s_st, items ? s_items : nullptr, s_aux, f);
        store_prim(S, tid, P);
    }
    __syncthreads();
    const int W = view.width, H = view.height, total = W / STRIP * H;
    const float inv_w = 1.f / (float)W, he = view.half_extent;
    for (int base = wave * 64; base < total; base += BLOCK) { /* wave-uniform */
        const int last = base + 63 < total ? base + 63 : total - 1;
        const TileBox t = strips_box(base, last, W, H, inv_w, he);
        const bool h0 = hits(S, lane, t), h1 = lane < R_SLOTS - 64 && hits(S, 64 + lane, t);
        const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1);
        const int s = base + lane;
        if (s < total) {
            uint32_t w[12];
            shade_strip(S, m0, m1, s, W, H, inv_w, he, w);
            uint4 *dst = reinterpret_cast<uint4 *>(rgb + strip_offset(env, s, W, H));
            dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
            dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
            dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
        }
    }
}

}  // namespace

extern "C" {

int hrl_render_default_view(const hrl_config *cfg, int32_t mode, hrl_view *view) {
    const int rc = default_view(cfg, mode, view);
    return rc == HRL_OK ? rc : fail(rc, "hrl_render_default_view: null argument, bad env_kind or unknown mode");
}

int hrl_render(const hrl_config *cfg, const hrl_buffers *b, const hrl_view *view, const uint8_t *mask, uint8_t *rgb, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_view(view);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_render: " + why);
    constexpr char NULLS[] = "hrl_render: null state, aux or rgb";
    if (const int rc = check_record(LIB, b, NULLS)) return rc;
    if (!rgb) return fail(HRL_ERR_BAD_ARG, NULLS);
    if (reinterpret_cast<uintptr_t>(rgb) % 16 != 0) return fail(HRL_ERR_BAD_ARG, "hrl_render: rgb must be 16-byte aligned (a strip of 16 pixels is stored as three 16-byte vectors)");
    const Pointer ptrs[] = {{rgb, "rgb", 0}}; /* its alignment has the wording above */
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 1, &d_dc)) return rc;
    hipLaunchKernelGGL(render_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, mask, rgb, *view);
    return launched(LIB);
}

const char *hrl_render_last_error(void) { return g_err.c_str(); }

}  // extern "C"
