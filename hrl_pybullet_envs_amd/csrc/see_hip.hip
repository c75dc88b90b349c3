/*
 * see_hip.hip -- gfx950 (MI355X) implementation of include/hrl_see.h: libhrl_see_hip.so.
 *
 * One workgroup of 256 threads computes the map of one env.  Its threads stage the env's state, aux and items records in LDS and build
 * the probe's table of 70 slots (see_core.h: lane = slot, in the robot-centred frame, each with the verdict `kept` = it occludes); one
 * thread adds the heading's forward vector and whether the robot's place is finite.  Two ballots give the list of occluders --
 * wave-uniform, so it lives in scalar registers and the walk's table reads are LDS broadcasts.  Then lane = cell: a wave takes 64
 * consecutive cells of the row-major grid and walks the list until none of its cells is still visible (the verdict is a boolean "any").
 *
 * The bytes of `visible` go to LDS and leave as 4-byte words of four cells, 256 consecutive bytes per wave, like the field's `parent`.
 * The memory is read and written the same way, lane = word: `seen` of four cells is one load, see_core.h's merge4 and one store, and the
 * lane's count of fresh cells is summed over the wave by five shuffles, over the four waves through LDS, and stored by one thread.
 * `clear` and the pointers of `out` are the same for the whole workgroup, so the barriers sit in uniform control flow; a masked env
 * returns as a whole workgroup before the first one.
 *
 * LDS: the table 1.8 KB, the staged records under 1 KB, 4 KB of cell bytes and four words: 6.6 KB, so occupancy is bounded by waves, not
 * by LDS.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "see_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::see;

namespace {

constexpr char LIB[] = "hrl_see";
constexpr int BLOCK = 256, WAVES = BLOCK / 64;

__global__ __launch_bounds__(BLOCK) void see_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *clear, const uint8_t *mask,
                                                    hrl_see_out out, hrl_see_spec sp) {
    __shared__ ProbeSet S;
    __shared__ float s_st[HRL_STATE_STRIDE];
    __shared__ float s_items[2 * HRL_MAX_ITEMS];
    __shared__ int32_t s_aux[HRL_AUX_STRIDE];
    __shared__ uint32_t s_vis4[MAX_CELLS / 4];
    __shared__ int32_t s_fresh[WAVES];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    uint8_t *vis = reinterpret_cast<uint8_t *>(s_vis4);
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) s_st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) s_aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) s_items[i] = items[(size_t)env * c.items_stride + i];
    const hrl_field_spec fs = grid_part(sp);
    const hrl_probe_spec ps = table_spec(sp);
    const Grid g = field::grid_of(fs);
    const int cells = g.W * g.H; /* <= MAX_CELLS and a multiple of 64: validate_spec */
    __syncthreads();
    const Frames f = field::frames_of(s_st, fs);
    for (int e = tid; e < S_SLOTS; e += BLOCK) probe::build_slot(S, e, c, s_st, items ? s_items : nullptr, s_aux, f.T, ps);
    if (tid == BLOCK - 1) probe::build_frame(S, s_st, ps); /* forward and whether the robot's place is finite */
    __syncthreads();
    const unsigned long long m0 = __ballot(probe::kept(S, lane)), m1 = __ballot(lane < S_SLOTS - 64 && probe::kept(S, lane < S_SLOTS - 64 ? 64 + lane : 0));
    for (int k = tid; k < cells; k += BLOCK) { /* lane = cell; whole waves */
        const int i = k / g.W, j = k - i * g.W;
        vis[k] = (uint8_t)cell_visible(S, m0, m1, g, f, sp, i, j);
    }
    __syncthreads();
    const size_t base = (size_t)env * (size_t)cells; /* a multiple of 64 and the tensors 4-byte aligned */
    if (out.visible) { /* (uniform over the grid: a kernel argument) */
        uint32_t *dst = reinterpret_cast<uint32_t *>(out.visible + base);
        for (int q = tid; q < cells / 4; q += BLOCK) dst[q] = s_vis4[q];
    }
    if (out.seen) {
        const bool fresh_start = clear && clear[env]; /* (the same in every thread) */
        uint32_t *mem = reinterpret_cast<uint32_t *>(out.seen + base);
        int32_t count = 0;
        for (int q = tid; q < cells / 4; q += BLOCK) mem[q] = merge4(s_vis4[q], fresh_start ? 0u : mem[q], &count);
        if (out.fresh) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
            if (lane == 0) s_fresh[wave] = count;
            __syncthreads();
            if (tid == 0) out.fresh[env] = s_fresh[0] + s_fresh[1] + s_fresh[2] + s_fresh[3];
        }
    }
}

}  // namespace

extern "C" {

int hrl_see_default_spec(const hrl_config *cfg, int32_t mode, hrl_see_spec *spec) {
    const int rc = default_spec(cfg, mode, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_see_default_spec: null argument, bad env_kind or unknown mode");
}

int hrl_see(const hrl_config *cfg, const hrl_buffers *b, const hrl_see_spec *spec, const uint8_t *clear, const uint8_t *mask, const hrl_see_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out, spec);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_see: " + why);
    if (const int rc = check_record(LIB, b, "hrl_see: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->visible, "visible", 4}, {out->seen, "seen", 4}, {out->fresh, "fresh", 4}, {clear, "clear", 0}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 4, &d_dc)) return rc;
    hipLaunchKernelGGL(see_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, clear, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_see_last_error(void) { return g_err.c_str(); }

}  // extern "C"
