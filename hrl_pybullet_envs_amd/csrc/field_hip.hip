/*
 * field_hip.hip -- gfx950 (MI355X) implementation of include/hrl_field.h: libhrl_field_hip.so.
 *
 * One workgroup of 256 threads computes the field of one env.  Its threads stage the env's state, aux and items records in LDS and
 * build the table of 71 entries (field_core.h: lane = entry; the probe's 70 slots in the robot-centred frame, each with the verdicts
 * `blocks` and `source`, and the robot).  Four ballots give the lists of blocking and source entries -- wave-uniform, so they live in
 * scalar registers and the walks' table reads are LDS broadcasts.  Then lane = cell: a wave takes 64 consecutive cells of a row-major
 * grid, classifies each (source 0, free +inf, blocked -1) into a padded (H + 2) x (W + 2) float image whose ring is blocked, and
 * derives each cell's byte of admissible steps from its neighbours.
 *
 * Relaxation: chaotic relaxation IN PLACE on the one padded image, lane = padded index, so the inner loop has no edge test, no division
 * and reads consecutive LDS words (the eight neighbours of 64 consecutive cells are 64 consecutive words each: no bank conflict).  A cell
 * whose byte is 0 (blocked, source, ring) is skipped.  Plain 32-bit LDS reads and writes only: a lane may read a neighbour's old or new
 * value -- both are lengths of real ways, values only decrease, and the fixed point is unique (field_core.h), so the bits do not depend on
 * who wins; a round in which no lane wrote has read only final values.  Every thread takes the exit decision from __syncthreads_or over
 * `some cell of mine changed`, which is also the round's only barrier; the loop is capped at W * H rounds, an integer of the spec.  No
 * barrier sits inside divergent control flow.  (Jacobi rounds over two images, the schedule this kernel started with, give the same bits
 * and take a third longer: profiles/EXPERIMENTS.md section 14.)
 *
 * LDS: the image of 17424 B, the bytes of admissible steps (4368 B), 4 KB for the table and the staged records (3.4 KB, dead once the
 * cells are classified; the parent bytes take their place at the end) and a few words: 25.5 KB, so six workgroups fit the 160 KB of a CU.
 *
 * Stores: `dist` lane = cell, 256 consecutive bytes per wave; `parent` goes through LDS as bytes and leaves as 4-byte words of four
 * cells, 256 consecutive bytes per wave.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "field_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::field;

namespace {

constexpr char LIB[] = "hrl_field";
constexpr int BLOCK = 256;
constexpr int ADM_WORDS = (MAX_PADDED + 3) / 4;

struct Tables { /* what the classification reads; the parent bytes take its place at the end */
    FieldSet F;
    float st[HRL_STATE_STRIDE];
    float items[2 * HRL_MAX_ITEMS];
    int32_t aux[HRL_AUX_STRIDE];
};
constexpr int SECOND_WORDS = MAX_CELLS / 4; /* room for the tables and, later, the parent bytes */
static_assert(sizeof(Tables) <= sizeof(float) * SECOND_WORDS, "the tables fit the second area");
static_assert((sizeof(float) * MAX_PADDED) % 16 == 0, "the second area starts 16-byte aligned");

__global__ __launch_bounds__(BLOCK) void field_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *mask, hrl_field_out out,
                                                      hrl_field_spec sp) {
    __shared__ alignas(16) float s_mem[MAX_PADDED + SECOND_WORDS];
    float *const img = s_mem;
    __shared__ uint32_t s_adm4[ADM_WORDS];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    Tables &T = *reinterpret_cast<Tables *>(s_mem + MAX_PADDED);
    uint8_t *adm = reinterpret_cast<uint8_t *>(s_adm4);
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) T.st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) T.aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) T.items[i] = items[(size_t)env * c.items_stride + i];
    const Grid g = grid_of(sp);
    const int cells = g.W * g.H, n_padded = g.PW * (g.H + 2); /* <= MAX_CELLS, <= MAX_PADDED: validate_spec */
    for (int p = tid; p < n_padded; p += BLOCK) { img[p] = BLOCKED_; adm[p] = 0; }
    __syncthreads();
    const Frames f = frames_of(T.st, sp);
    for (int e = tid; e < N_ENTRIES; e += BLOCK) build_entry(T.F, e, c, T.st, items ? T.items : nullptr, T.aux, f, sp);
    __syncthreads();
    const uint32_t fl0 = T.F.flags[lane], fl1 = lane < N_ENTRIES - 64 ? T.F.flags[64 + lane] : 0u;
    const unsigned long long b0 = __ballot((fl0 & F_BLOCKS) != 0u), b1 = __ballot((fl1 & F_BLOCKS) != 0u);
    const unsigned long long s0 = __ballot((fl0 & F_SOURCE) != 0u), s1 = __ballot((fl1 & F_SOURCE) != 0u);
    for (int k = tid; k < cells; k += BLOCK) { /* lane = cell */
        const int i = k / g.W, j = k - i * g.W;
        img[padded(g, i, j)] = cell_init(T.F, b0, b1, s0, s1, g, f, sp.margin, i, j);
    }
    __syncthreads(); /* the tables are dead from here */
    const int cap = cells; /* Bellman-Ford's bound: a way has fewer than W H cells */
    for (int k = tid; k < cells; k += BLOCK) {
        const int i = k / g.W, j = k - i * g.W, p = padded(g, i, j);
        adm[p] = (uint8_t)cell_adm(img, p, g.PW);
    }
    __syncthreads();
    for (int r = 0; r < cap; ++r) {
        int changed = 0;
        for (int p = tid; p < n_padded; p += BLOCK) { /* lane = padded index */
            const uint32_t a = adm[p];
            if (a != 0u) {
                const float old = img[p], d = cell_relax(img, p, g.PW, a, g.w1, g.w2);
                if (d != old) { img[p] = d; changed = 1; }
            }
        }
        if (!__syncthreads_or(changed)) break; /* the same value in every thread; the barrier between two rounds */
    }
    uint8_t *par = reinterpret_cast<uint8_t *>(s_mem + MAX_PADDED); /* (the tables' place) */
    const size_t base = (size_t)env * (size_t)cells;
    for (int k = tid; k < cells; k += BLOCK) {
        const int i = k / g.W, j = k - i * g.W, p = padded(g, i, j);
        if (out.dist) out.dist[base + (size_t)k] = cell_dist(img, p);
        if (out.parent) par[k] = (uint8_t)cell_parent(img, p, g.PW, adm[p], g.w1, g.w2);
    }
    if (out.parent) { /* (uniform over the grid: a kernel argument) */
        __syncthreads();
        const uint32_t *par4 = reinterpret_cast<const uint32_t *>(par);
        uint32_t *dst = reinterpret_cast<uint32_t *>(out.parent + base); /* base is a multiple of 64 and the tensor 4-byte aligned */
        for (int q = tid; q < cells / 4; q += BLOCK) dst[q] = par4[q];
    }
}

}  // namespace

extern "C" {

int hrl_field_default_spec(const hrl_config *cfg, int32_t mode, hrl_field_spec *spec) {
    const int rc = default_spec(cfg, mode, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_field_default_spec: null argument, bad env_kind or unknown mode");
}

int hrl_field(const hrl_config *cfg, const hrl_buffers *b, const hrl_field_spec *spec, const uint8_t *mask, const hrl_field_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_field: " + why);
    if (const int rc = check_record(LIB, b, "hrl_field: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->dist, "dist", 4}, {out->parent, "parent", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 2, &d_dc)) return rc;
    hipLaunchKernelGGL(field_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_field_last_error(void) { return g_err.c_str(); }

}  // extern "C"
