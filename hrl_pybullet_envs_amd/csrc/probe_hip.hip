/*
 * probe_hip.hip -- gfx950 (MI355X) implementation of include/hrl_probe.h: libhrl_probe_hip.so.
 *
 * One workgroup of 64 x min(4, ceil(n_points / 64)) threads probes one env.  Its threads stage the env's state, aux and items records
 * in LDS and build the env's table of 70 slots (probe_core.h: lane = slot; the renderer's primitives of the planes, the box, the target
 * and the items in a robot-centred frame, each with its code and the verdict `kept`).  Two ballots give the list of kept slots --
 * wave-uniform, so it lives in scalar registers and the walks' table reads are LDS broadcasts.  Thread 0 snaps the start; the lanes of
 * wave 0 then hold corner node lane & 3 each and run the three Jacobi rounds through lane shuffles, and lanes 0..3 leave the nodes and
 * g[] in LDS.  Each wave then takes runs of 64 points, lane = point: a lane reads one float2 and stores one 4-byte value per requested
 * output, so the lanes of a wave write 256 consecutive bytes of each tensor.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "probe_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::probe;

namespace {

constexpr char LIB[] = "hrl_probe";
constexpr int MAX_BLOCK = 256;

__global__ __launch_bounds__(MAX_BLOCK) void probe_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *mask,
                                                          const float2 *points, hrl_probe_out out, hrl_probe_spec sp) {
    __shared__ ProbeSet S;
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
    if (tid == 0) build_frame(S, s_st, sp);
    const render::Frame f = scan::table_frame(s_st);
    for (int slot = tid; slot < S_SLOTS; slot += block) build_slot(S, slot, c, s_st, items ? s_items : nullptr, s_aux, f, sp);
    __syncthreads();
    const bool k0 = kept(S, lane), k1 = lane < S_SLOTS - 64 && kept(S, 64 + lane);
    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
    const unsigned w = wanted(out);
    if (w & (W_PATH | W_VIA)) { /* (uniform over the workgroup: a kernel argument) */
        if (tid == 0) build_start(S, sp.margin);
        __syncthreads();
        if (wave == 0) { /* every lane works: lane l holds node l & 3, lanes 0..3 are the ones that are read */
            const int k = lane & 3;
            float g = node_init(S, k, sp.margin);
            int32_t first = k;
            for (int round = 0; round < 3; ++round) {
                float g_old[4];
                int32_t first_old[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { g_old[j] = __shfl(g, j); first_old[j] = __shfl(first, j); }
                node_round(S, k, sp.margin, g_old, first_old, &g, &first);
            }
            if (lane < 4) {
                node_pos(S, lane, &S.node[lane][0], &S.node[lane][1]);
                S.g[lane] = g; S.first[lane] = first;
            }
        }
        __syncthreads();
    }
    const int n = sp.n_points;
    for (int base = wave * 64; base < n; base += block) { /* wave-uniform */
        const int k = base + lane;
        if (k < n) {
            const size_t at = (size_t)env * (size_t)n + (size_t)k;
            const float2 p = points[at];
            probe_point(S, m0, m1, sp, p.x, p.y, out, w, at);
        }
    }
}

}  // namespace

extern "C" {

int hrl_probe_default_spec(const hrl_config *cfg, int32_t frame, hrl_probe_spec *spec) {
    const int rc = default_spec(cfg, frame, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_probe_default_spec: null argument, bad env_kind or unknown frame");
}

int hrl_probe(const hrl_config *cfg, const hrl_buffers *b, const hrl_probe_spec *spec, const float *points, const uint8_t *mask, const hrl_probe_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_probe: " + why);
    if (const int rc = check_record(LIB, b, "hrl_probe: null state or aux")) return rc;
    if (!points) return fail(HRL_ERR_BAD_ARG, "hrl_probe: null points");
    if (reinterpret_cast<uintptr_t>(points) % 8 != 0) return fail(HRL_ERR_BAD_ARG, "hrl_probe: points must be 8-byte aligned");
    const Pointer ptrs[] = {{points, "points", 0},       {out->clearance, "clearance", 4}, {out->nearest, "nearest", 4}, {out->sight, "sight", 4},
                            {out->blocker, "blocker", 4}, {out->path, "path", 4},           {out->via, "via", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 7, &d_dc)) return rc;
    const int waves = (spec->n_points + 63) / 64; /* 64 points do not carry three idle waves */
    const int block = 64 * (waves < 4 ? waves : 4);
    hipLaunchKernelGGL(probe_kernel, dim3(cfg->num_envs), dim3(block), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, mask, (const float2 *)points, *out, *spec);
    return launched(LIB);
}

const char *hrl_probe_last_error(void) { return g_err.c_str(); }

}  // extern "C"
