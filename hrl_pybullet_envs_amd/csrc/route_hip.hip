/*
 * route_hip.hip -- gfx950 (MI355X) implementation of include/hrl_route.h: libhrl_route_hip.so.
 *
 * One workgroup of 256 threads computes the routes of one env.  Its first three phases are field_hip.hip's, on the same core functions
 * (field_core.h): the env's records are staged in LDS, the table of 71 entries is built lane = entry, the cells are classified lane = cell
 * into the padded image, and the image is relaxed in place until no lane writes, with __syncthreads_or as the loop's only barrier.  The
 * field itself is not written out.  After convergence the parent bytes go to LDS (4 KB), and with them one 64-bit mask of blocked cells
 * per row: a wave's ballot over 64 consecutive cells is cut into bytes of eight cells -- W is a multiple of 8, so a byte never spans two
 * rows -- and every eighth lane stores its byte where the row's mask has it.
 *
 * Then the four waves take the starts wave, wave + 4, ... and each start is wave-level work only, with no barrier:
 *   start cell   lane = column and lane = row ask col_holds / row_holds; two ballots, the lowest bit of each
 *   chain, pull  route_core.h's trace, the same in every lane: the parent byte of the current cell is an LDS broadcast made scalar, so
 *                the walk branches uniformly.  It is a serial chain of dependent LDS reads, one per cell of the way
 *   clear        lane = row: row_touch's interval of columns ANDed with the row's mask of blocked cells, one ballot
 *   outputs      the cells of the waypoints are staged in LDS (every lane writes the same value); then lane = entry: K consecutive
 *                cells and 2 K consecutive floats leave per start
 * A masked env returns as a whole workgroup before the first barrier.
 *
 * LDS: the image 17424 B, the bytes of admissible steps 4368 B, the table and the staged records 3.4 KB, the parent bytes 4 KB, the row
 * masks and the staged waypoints 512 B each: 30.3 KB, five workgroups per CU.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "route_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::route;

namespace {

constexpr char LIB[] = "hrl_route";
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int MAX_PADDED = field::MAX_PADDED, ADM_WORDS = (MAX_PADDED + 3) / 4;

struct Tables { /* what the classification and the starts read */
    field::FieldSet F;
    float st[HRL_STATE_STRIDE];
    float items[2 * HRL_MAX_ITEMS];
    int32_t aux[HRL_AUX_STRIDE];
};

__global__ __launch_bounds__(BLOCK) void route_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const float *starts, const uint8_t *mask,
                                                      hrl_route_out out, hrl_route_spec sp) {
    __shared__ alignas(16) float img[MAX_PADDED];
    __shared__ uint32_t s_adm4[ADM_WORDS];
    __shared__ Tables T;
    __shared__ uint32_t s_par4[MAX_CELLS / 4];
    __shared__ unsigned long long s_rows[MAX_SIZE];
    __shared__ int32_t s_stage[WAVES][MAX_WAYPOINTS];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    uint8_t *adm = reinterpret_cast<uint8_t *>(s_adm4);
    uint8_t *par = reinterpret_cast<uint8_t *>(s_par4);
    uint8_t *row_bytes = reinterpret_cast<uint8_t *>(s_rows); /* byte 8 i + b = columns 8 b .. 8 b + 7 of row i (little endian) */
    const DevCfg &c = *cfg;
    const hrl_field_spec fs = field_part(sp);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) T.st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) T.aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) T.items[i] = items[(size_t)env * c.items_stride + i];
    if (tid >= 64 && tid < 64 + MAX_SIZE) s_rows[tid - 64] = 0ull;
    const Grid g = field::grid_of(fs);
    const int cells = g.W * g.H, n_padded = g.PW * (g.H + 2); /* <= MAX_CELLS, <= MAX_PADDED: validate_spec */
    for (int p = tid; p < n_padded; p += BLOCK) { img[p] = field::BLOCKED_; adm[p] = 0; }
    __syncthreads();
    const Frames f = field::frames_of(T.st, fs);
    for (int e = tid; e < field::N_ENTRIES; e += BLOCK) field::build_entry(T.F, e, c, T.st, items ? T.items : nullptr, T.aux, f, fs);
    if (tid == BLOCK - 1) probe::build_frame(T.F.S, T.st, frame_spec(sp.frame)); /* forward, the robot's place and whether it is finite: what locate reads */
    __syncthreads();
    {
        const uint32_t fl0 = T.F.flags[lane], fl1 = lane < field::N_ENTRIES - 64 ? T.F.flags[64 + lane] : 0u;
        const unsigned long long b0 = __ballot((fl0 & field::F_BLOCKS) != 0u), b1 = __ballot((fl1 & field::F_BLOCKS) != 0u);
        const unsigned long long s0 = __ballot((fl0 & field::F_SOURCE) != 0u), s1 = __ballot((fl1 & field::F_SOURCE) != 0u);
        for (int k = tid; k < cells; k += BLOCK) { /* lane = cell */
            const int i = k / g.W, j = k - i * g.W;
            img[field::padded(g, i, j)] = field::cell_init(T.F, b0, b1, s0, s1, g, f, fs.margin, i, j);
        }
    }
    __syncthreads();
    for (int k = tid; k < cells; k += BLOCK) {
        const int i = k / g.W, j = k - i * g.W, p = field::padded(g, i, j);
        adm[p] = (uint8_t)field::cell_adm(img, p, g.PW);
    }
    __syncthreads();
    for (int r = 0; r < cells; ++r) { /* Bellman-Ford's bound: a way has fewer than W H cells */
        int changed = 0;
        for (int p = tid; p < n_padded; p += BLOCK) { /* lane = padded index */
            const uint32_t a = adm[p];
            if (a != 0u) {
                const float old = img[p], d = field::cell_relax(img, p, g.PW, a, g.w1, g.w2);
                if (d != old) { img[p] = d; changed = 1; }
            }
        }
        if (!__syncthreads_or(changed)) break; /* the same value in every thread; the barrier between two rounds */
    }
    for (int k = tid; k < cells; k += BLOCK) { /* cells is a multiple of 64: whole waves */
        const int i = k / g.W, j = k - i * g.W, p = field::padded(g, i, j);
        const uint32_t code = field::cell_parent(img, p, g.PW, adm[p], g.w1, g.w2);
        par[k] = (uint8_t)code;
        const unsigned long long blocked = __ballot(code == (uint32_t)HRL_FIELD_BLOCKED);
        if ((lane & 7) == 0) row_bytes[8 * i + (j >> 3)] = (uint8_t)(blocked >> lane);
    }
    __syncthreads(); /* the last barrier: from here a wave works alone */

    const int P = sp.n_starts, K = sp.max_waypoints; /* <= MAX_STARTS, <= MAX_WAYPOINTS: validate_spec */
    const unsigned long long my_row = lane < g.H ? s_rows[lane] : 0ull;
    int32_t *stage = s_stage[wave];
    for (int p = wave; p < P; p += WAVES) {
        const size_t at = (size_t)env * (size_t)P + (size_t)p;
        float px = 0.f, py = 0.f; /* (no starts: the robot, an offset of nothing from itself) */
        int frame = HRL_PROBE_EGO;
        if (starts) { px = starts[2 * at]; py = starts[2 * at + 1]; frame = sp.frame; }
        float u, v;
        const bool ok = start_uv(T.F.S, f, frame, px, py, &u, &v);
        const unsigned long long cm = __ballot(lane < g.W && col_holds(g, u, lane)), rm = __ballot(lane < g.H && row_holds(g, v, lane));
        const int j = cm != 0ull ? __builtin_ctzll(cm) : 0, i = rm != 0ull ? __builtin_ctzll(rm) : 0;
        const bool go = __ballot(ok && cm != 0ull && rm != 0ull && par[i * g.W + j] <= HRL_FIELD_SOURCE) != 0ull; /* (the same in every lane; the ballot makes it scalar) */
        int n = 0;
        float len = inf_();
        if (go) {
            auto clear = [&](int ai, int aj, int bi, int bj) { return __ballot((row_touch(ai, aj, bi, bj, lane) & my_row) != 0ull) == 0ull; };
            trace(par, g, i, j, K, stage, clear, &n, &len);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier(); /* (this wave's staged cells, written above, are read below by other lanes) */
        const int written = n < K ? n : K;
        const int k = lane >> 1;
        int32_t cell_k = -1, cell_l = -1; /* of waypoint lane >> 1 and of waypoint lane */
        if (n > 0 && k < K) cell_k = stage[k < written ? k : written - 1];
        if (n > 0 && lane < K) cell_l = stage[lane < written ? lane : written - 1];
        if (lane == 0) {
            if (out.count) out.count[at] = n;
            if (out.length) out.length[at] = len;
        }
        if (out.cells && lane < K) out.cells[at * (size_t)K + (size_t)lane] = cell_l;
        if (out.waypoints && lane < 2 * K) {
            float x = __builtin_nanf(""), y = __builtin_nanf("");
            if (n > 0) waypoint_of(g, f, cell_k, &x, &y);
            out.waypoints[at * (size_t)(2 * K) + (size_t)lane] = (lane & 1) ? y : x;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier(); /* (before the next start overwrites the stage) */
    }
}

}  // namespace

extern "C" {

int hrl_route_default_spec(const hrl_config *cfg, int32_t mode, hrl_route_spec *spec) {
    const int rc = default_spec(cfg, mode, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_route_default_spec: null argument, bad env_kind or unknown mode");
}

int hrl_route(const hrl_config *cfg, const hrl_buffers *b, const hrl_route_spec *spec, const float *starts, const uint8_t *mask, const hrl_route_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_route: " + why);
    if (const int rc = check_record(LIB, b, "hrl_route: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->waypoints, "waypoints", 4}, {out->count, "count", 4}, {out->length, "length", 4}, {out->cells, "cells", 4}, {starts, "starts", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 5, &d_dc)) return rc;
    hipLaunchKernelGGL(route_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, starts, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_route_last_error(void) { return g_err.c_str(); }

}  // extern "C"
