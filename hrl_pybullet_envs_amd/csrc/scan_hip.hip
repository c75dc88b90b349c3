/*
 * scan_hip.hip -- gfx950 (MI355X) implementation of include/hrl_scan.h: libhrl_scan_hip.so.
 *
 * One workgroup of 64 x min(4, ceil(n_rays / 64)) threads scans one env.  Its threads build the env's table of 70 slots
 * (scan_core.h: lane = slot; the renderer's primitives of the planes, the box, the target and the items in a robot-centred frame,
 * each with its hit code and the verdict of the cull) in 1.7 KB of LDS.  Each wave then takes runs of 64 rays: lane = slot reads the
 * verdicts, two ballots give the list of surviving slots -- wave-uniform, so it lives in scalar registers and the walk's table reads are
 * LDS broadcasts -- and lane = ray walks only the set bits in slot order.  A lane stores one float and one int32; the lanes of a wave
 * write 256 consecutive bytes of each output.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "scan_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::scan;

namespace {

constexpr char LIB[] = "hrl_scan";
constexpr int MAX_BLOCK = 256;

__global__ __launch_bounds__(MAX_BLOCK) void scan_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *mask, float *range,
                                                         int32_t *hit, hrl_scan_spec sp) {
    __shared__ ScanSet S;
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    __shared__ int32_t s_aux[HRL_AUX_STRIDE];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63, block = blockDim.x; /* block: 64, 128, 192 or 256 */
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) s_aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += block) s_items[i] = items[(size_t)env * c.items_stride + i];
    __syncthreads();
    if (tid == 0) forward(sp.frame, s_st, &S.fwd[0], &S.fwd[1]);
    const Frame f = table_frame(s_st);
    for (int slot = tid; slot < S_SLOTS; slot += block) build_slot(S, slot, c, s_st, items ? s_items : nullptr, s_aux, f, sp);
    __syncthreads();
    const bool k0 = kept(S, lane), k1 = lane < S_SLOTS - 64 && kept(S, 64 + lane);
    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
    const int n = sp.n_rays;
    for (int base = wave * 64; base < n; base += block) { /* wave-uniform */
        const int k = base + lane;
        if (k < n) {
            float r;
            int32_t h;
            scan_ray(S, m0, m1, sp, k, &r, &h);
            const size_t o = (size_t)env * (size_t)n + (size_t)k;
            range[o] = r;
            hit[o] = h;
        }
    }
}

}  // namespace

extern "C" {

int hrl_scan_default_spec(const hrl_config *cfg, int32_t frame, hrl_scan_spec *spec) {
    const int rc = default_spec(cfg, frame, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_scan_default_spec: null argument, bad env_kind or unknown frame");
}

int hrl_scan(const hrl_config *cfg, const hrl_buffers *b, const hrl_scan_spec *spec, const uint8_t *mask, float *range, int32_t *hit, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_scan: " + why);
    constexpr char NULLS[] = "hrl_scan: null state, aux, range or hit";
    if (const int rc = check_record(LIB, b, NULLS)) return rc;
    if (!range || !hit) return fail(HRL_ERR_BAD_ARG, NULLS);
    if (reinterpret_cast<uintptr_t>(range) % 4 != 0 || reinterpret_cast<uintptr_t>(hit) % 4 != 0) return fail(HRL_ERR_BAD_ARG, "hrl_scan: range and hit must be 4-byte aligned");
    const Pointer ptrs[] = {{range, "range", 0}, {hit, "hit", 0}}; /* their alignment has the wording above */
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 2, &d_dc)) return rc;
    const int waves = (spec->n_rays + 63) / 64; /* a 64-ray scan does not carry three idle waves */
    const int block = 64 * (waves < 4 ? waves : 4);
    hipLaunchKernelGGL(scan_kernel, dim3(cfg->num_envs), dim3(block), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, mask, range, hit, *spec);
    return launched(LIB);
}

const char *hrl_scan_last_error(void) { return g_err.c_str(); }

}  // extern "C"
