/*
 * chase_hip.hip -- gfx950 (MI355X) implementation of include/hrl_chase.h: libhrl_chase_hip.so.
 *
 * One workgroup of 256 threads computes the image of one env, in the camera's layout (camera_hip.hip).  Its threads stage the env's
 * state, aux and items records in LDS.  Then lane = slot builds the scanner's table of 70 slots about the eye with the slots'
 * z-intervals (chase_core.h: build_slot), and, in the workgroup's last wave, lane = primitive evaluates links::link_world once per
 * primitive of the robot (25 at most) and writes its ray-independent terms.  Two ballots give the list of walked slots and one more
 * the list of drawn primitives -- wave-uniform, so they live in scalar registers and the walk's table reads are LDS broadcasts.  Then
 * lane = pixel, row-major: a wave takes 64 consecutive pixels and walks both lists in uniform control flow; the primitives' list is
 * skipped by a wave none of whose 64 rays passes the robot's bounding sphere (chase_core.h: near_robot, voted with __any).
 *
 * `depth` and `seg` leave lane = pixel, 256 consecutive bytes per wave.  The bytes of `rgb` go to LDS and leave as 4-byte words, a chunk
 * of CHUNK = 1024 pixels (3 KB, four passes of the workgroup) at a time: an image is a multiple of 128 pixels, so every chunk, the last
 * one included, is a whole number of words at a 4-byte aligned offset.  The chunk size is a compile-time constant and the pointers of
 * `out` are kernel arguments, so the barriers sit in uniform control flow; a masked env returns as a whole workgroup before the first one.
 *
 * LDS: the table 1 688 B, its z-intervals 560 B, the primitives with their reach 1 792 B, the staged records 656 B, 3 072 B of rgb
 * bytes: 7 792 B a workgroup with the alignment, so occupancy is bounded by waves (the 80 VGPRs allow 6 waves a SIMD, 6 workgroups a
 * compute unit: 47 KB of its 160 KB), not by LDS.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "chase_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::chase;

namespace {

constexpr char LIB[] = "hrl_chase";
constexpr int BLOCK = 256;
static_assert(CHUNK % BLOCK == 0 && (3 * CHUNK) % 4 == 0, "a chunk is whole passes of the workgroup and whole words");
static_assert(S_SLOTS <= BLOCK - 64 && PRIMS <= 64, "the slots' lanes and the primitives' wave are different threads");

__global__ __launch_bounds__(BLOCK) void chase_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *mask, hrl_chase_out out,
                                                      hrl_chase_spec sp) {
    __shared__ ScanSet S;
    __shared__ PrimSet P;
    __shared__ float s_zl[S_SLOTS], s_zh[S_SLOTS];
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    __shared__ int32_t s_aux[HRL_AUX_STRIDE];
    __shared__ uint32_t s_rgb4[CHUNK * 3 / 4];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    uint8_t *bytes = reinterpret_cast<uint8_t *>(s_rgb4);
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) s_aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) s_items[i] = items[(size_t)env * c.items_stride + i];
    const hrl_scan_spec ts = table_spec(sp);
    const int W = sp.width, pixels = sp.width * sp.height; /* <= MAX_SIZE^2 and a multiple of 128: validate_spec */
    const float inv_w = 1.f / (float)sp.width, inv_h = 1.f / (float)sp.height;
    __syncthreads();
    const View v = view_of(c, s_st, sp);
    const Frame f = scan::table_frame(s_st);
    if (tid < S_SLOTS) build_slot(S, s_zl, s_zh, tid, c, s_st, items ? s_items : nullptr, s_aux, f, ts, v);
    if (tid >= BLOCK - 64 && lane < PRIMS) build_prim(P, lane, c, s_st, v, sp.classes); /* (the last wave: no slot's lane) */
    __syncthreads();
    const unsigned long long m0 = __ballot(scan::kept(S, lane)), m1 = __ballot(lane < S_SLOTS - 64 && scan::kept(S, lane < S_SLOTS - 64 ? 64 + lane : 0));
    const uint32_t pm = (uint32_t)__ballot(lane < PRIMS && drawn(P, lane < PRIMS ? lane : 0));
    const float rb2 = robot_bound(P, pm);
    const size_t base = (size_t)env * (size_t)pixels;
    for (int k0 = 0; k0 < pixels; k0 += CHUNK) { /* (uniform: k0 and pixels are the same in every thread) */
        const int k1 = k0 + CHUNK < pixels ? k0 + CHUNK : pixels;
        for (int k = k0 + tid; k < k1; k += BLOCK) { /* lane = pixel; whole waves */
            const int i = k / W, j = k - i * W;
            float d;
            int32_t s;
            uint32_t rgb;
            const Ray r = pixel_ray(sp, v, i, j, inv_w, inv_h);
            const bool robot = __any(near_robot(v, rb2, r)); /* (whole waves: a wave whose 64 rays all pass the robot by skips its primitives) */
            shade_pixel(S, s_zl, s_zh, P, m0, m1, pm, robot, sp, v, r, &d, &s, &rgb);
            if (out.depth) out.depth[base + k] = d;
            if (out.seg) out.seg[base + k] = s;
            if (out.rgb) {
                const int at = 3 * (k - k0); /* < 3 * CHUNK */
                bytes[at] = (uint8_t)rgb; bytes[at + 1] = (uint8_t)(rgb >> 8); bytes[at + 2] = (uint8_t)(rgb >> 16);
            }
        }
        if (out.rgb) { /* (uniform over the grid: a kernel argument) */
            __syncthreads();
            uint32_t *dst = reinterpret_cast<uint32_t *>(out.rgb + 3 * (base + (size_t)k0)); /* 3 * pixels and 3 * CHUNK are multiples of 4, the tensor 4-byte aligned */
            const int words = 3 * (k1 - k0) / 4; /* <= 3 * CHUNK / 4 */
            for (int q = tid; q < words; q += BLOCK) dst[q] = s_rgb4[q];
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" {

int hrl_chase_default_spec(const hrl_config *cfg, int32_t frame, hrl_chase_spec *spec) {
    const int rc = default_spec(cfg, frame, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_chase_default_spec: null argument, bad env_kind or unknown frame");
}

int hrl_chase(const hrl_config *cfg, const hrl_buffers *b, const hrl_chase_spec *spec, const uint8_t *mask, const hrl_chase_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_chase: " + why);
    if (const int rc = check_record(LIB, b, "hrl_chase: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->depth, "depth", 4}, {out->seg, "seg", 4}, {out->rgb, "rgb", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 3, &d_dc)) return rc;
    hipLaunchKernelGGL(chase_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_chase_last_error(void) { return g_err.c_str(); }

}  // extern "C"
