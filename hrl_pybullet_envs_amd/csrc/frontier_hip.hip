/*
 * frontier_hip.hip -- gfx950 (MI355X) implementation of include/hrl_frontier.h: libhrl_frontier_hip.so.
 *
 * One workgroup of 256 threads computes the map of one env, on field_hip.hip's plan and on the same core functions (field_core.h): the
 * env's state, aux and items records are staged in LDS, the table of 71 entries is built lane = entry, four ballots give the wave-uniform
 * lists of blocking and source entries, the cells are classified lane = cell into the padded image, and the image is relaxed in place until
 * no lane writes, with __syncthreads_or as the only barrier of a round.
 *
 * What is new here (frontier_core.h):
 *   memory      the env's bytes of `seen` come in as 4-byte words of four cells, lane = word; known4 makes four bits of a word, a shuffle
 *               joins two lanes' bits into a byte of eight cells, and 512 B of LDS hold the grid; one thread sets the bit of the robot's
 *               cell, which every wave has found by two ballots over col_holds / row_holds (lane = column, lane = row)
 *   two passes  g first (cell_init, the only pass that reads the table), a barrier, then value and edge: a lane reads its own g and the
 *               knowledge of its four neighbours from LDS and writes its own cell of the image and its own byte of `edge`
 *   edge        the bytes go to the 4 KB that held the table and the staged records (dead after the first pass) and leave as words of
 *               four cells; the parent bytes take the same place once the relaxation is over, as in the field's kernel
 *   count       the lane's edge cells are summed over the wave by six shuffles, over the four waves through LDS, and stored by one thread
 *   summary     wave 0 alone, no barrier: the walk along the parent bytes is the same in every lane (an LDS broadcast made scalar), and
 *               lane 0 stores length, goal and cell
 * `out`, `sp` and the mask byte are the same for the whole workgroup, so every barrier sits in uniform control flow; a masked env returns
 * as a whole workgroup before the first one.
 *
 * LDS: the image 17424 B, the bytes of admissible steps 4368 B, 4 KB for the table / edge / parent, 512 B of memory and four words:
 * 26.0 KB, so six workgroups fit the 160 KB of a CU, as with the field's kernel.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "frontier_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::frontier;

namespace {

constexpr char LIB[] = "hrl_frontier";
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int ADM_WORDS = (MAX_PADDED + 3) / 4;

struct Tables { /* what the first pass reads; the edge bytes and then the parent bytes take its place */
    FieldSet F;
    float st[HRL_STATE_STRIDE];
    float items[2 * HRL_MAX_ITEMS];
    int32_t aux[HRL_AUX_STRIDE];
};
constexpr int SECOND_WORDS = MAX_CELLS / 4;
static_assert(sizeof(Tables) <= sizeof(float) * SECOND_WORDS, "the tables fit the second area");
static_assert((sizeof(float) * MAX_PADDED) % 16 == 0, "the second area starts 16-byte aligned");

__global__ __launch_bounds__(BLOCK) void frontier_kernel(const DevCfg *cfg, const float *state, const float *items, const int32_t *aux, const uint8_t *seen, const uint8_t *mask,
                                                         hrl_frontier_out out, hrl_frontier_spec sp) {
    __shared__ alignas(16) float s_mem[MAX_PADDED + SECOND_WORDS];
    float *const img = s_mem;
    __shared__ uint32_t s_adm4[ADM_WORDS];
    __shared__ uint32_t s_bits4[MAX_CELLS / 32];
    __shared__ int32_t s_count[WAVES];
    const int env = blockIdx.x;
    if (mask && !mask[env]) return; /* (the whole workgroup: no barrier is left waiting) */
    Tables &T = *reinterpret_cast<Tables *>(s_mem + MAX_PADDED);
    uint32_t *const second4 = reinterpret_cast<uint32_t *>(s_mem + MAX_PADDED);
    uint8_t *const second = reinterpret_cast<uint8_t *>(second4); /* the edge bytes, later the parent bytes */
    uint8_t *adm = reinterpret_cast<uint8_t *>(s_adm4);
    uint8_t *bits = reinterpret_cast<uint8_t *>(s_bits4); /* the memory, a bit per cell */
    const DevCfg &c = *cfg;
    const hrl_field_spec fs = field_part(sp);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = c.items_stride < 2 * HRL_MAX_ITEMS ? c.items_stride : 2 * HRL_MAX_ITEMS;
    if (tid < HRL_STATE_STRIDE) T.st[tid] = state[(size_t)env * HRL_STATE_STRIDE + tid];
    if (tid >= 32 && tid < 32 + HRL_AUX_STRIDE) T.aux[tid - 32] = aux[(size_t)env * HRL_AUX_STRIDE + (tid - 32)];
    if (items)
        for (int i = tid; i < stride; i += BLOCK) T.items[i] = items[(size_t)env * c.items_stride + i];
    const Grid g = field::grid_of(fs);
    const int cells = g.W * g.H, n_padded = g.PW * (g.H + 2); /* <= MAX_CELLS, <= MAX_PADDED: validate_spec */
    const size_t base = (size_t)env * (size_t)cells;          /* a multiple of 64 and the tensors 4-byte aligned */
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(seen + base);
        for (int q0 = 0; q0 < cells / 4; q0 += BLOCK) { /* lane = word; every lane takes part in the shuffle */
            const int q = q0 + tid;
            const uint32_t mine = q < cells / 4 ? known4(src[q]) : 0u, next = (uint32_t)__shfl_xor((int)mine, 1);
            if (q < cells / 4 && (tid & 1) == 0) bits[q >> 1] = (uint8_t)(mine | (next << 4));
        }
    }
    for (int p = tid; p < n_padded; p += BLOCK) { img[p] = BLOCKED_; adm[p] = 0; }
    __syncthreads();
    const Frames f = field::frames_of(T.st, fs);
    for (int e = tid; e < field::N_ENTRIES; e += BLOCK) field::build_entry(T.F, e, c, T.st, items ? T.items : nullptr, T.aux, f, fs);
    __syncthreads();
    int ri, rj;
    bool has_r;
    { /* the robot's cell: the lowest column and row that hold its entry's centre; the same in every thread */
        const float su = T.F.su[field::E_ROBOT], sv = T.F.sv[field::E_ROBOT];
        const unsigned long long cm = __ballot(lane < g.W && route::col_holds(g, su, lane)), rm = __ballot(lane < g.H && route::row_holds(g, sv, lane));
        rj = cm != 0ull ? __builtin_ctzll(cm) : 0;
        ri = rm != 0ull ? __builtin_ctzll(rm) : 0;
        has_r = f.robot_ok && cm != 0ull && rm != 0ull;
    }
    if (tid == 0 && has_r) bits[(ri * g.W + rj) >> 3] |= (uint8_t)(1u << ((ri * g.W + rj) & 7));
    {
        const uint32_t fl0 = T.F.flags[lane], fl1 = lane < field::N_ENTRIES - 64 ? T.F.flags[64 + lane] : 0u;
        const unsigned long long b0 = __ballot((fl0 & field::F_BLOCKS) != 0u), b1 = __ballot((fl1 & field::F_BLOCKS) != 0u);
        const unsigned long long s0 = __ballot((fl0 & field::F_SOURCE) != 0u), s1 = __ballot((fl1 & field::F_SOURCE) != 0u);
        for (int k = tid; k < cells; k += BLOCK) { /* lane = cell: g */
            const int i = k / g.W, j = k - i * g.W;
            img[field::padded(g, i, j)] = field::cell_init(T.F, b0, b1, s0, s1, g, f, fs.margin, i, j);
        }
    }
    __syncthreads(); /* the tables are dead from here; the memory holds the robot's cell */
    int32_t count = 0;
    for (int k = tid; k < cells; k += BLOCK) { /* lane = cell: value and edge, from the lane's own g and its neighbours' knowledge */
        const int i = k / g.W, j = k - i * g.W, p = field::padded(g, i, j);
        const float gv = img[p];
        const bool ed = cell_edge(bits, g, i, j, gv);
        img[p] = cell_value(gv, known_at(bits, k), ed, sp.sources, sp.unknown);
        second[k] = ed ? 1 : 0;
        count += ed ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (lane == 0) s_count[wave] = count;
    __syncthreads();
    if (out.edge) { /* (uniform over the grid: a kernel argument) */
        uint32_t *dst = reinterpret_cast<uint32_t *>(out.edge + base);
        for (int q = tid; q < cells / 4; q += BLOCK) dst[q] = second4[q];
    }
    if (out.count && tid == 0) out.count[env] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
    for (int k = tid; k < cells; k += BLOCK) {
        const int i = k / g.W, j = k - i * g.W, p = field::padded(g, i, j);
        adm[p] = (uint8_t)field::cell_adm(img, p, g.PW);
    }
    __syncthreads(); /* (the edge bytes have left: their place is free) */
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
    uint8_t *par = second;
    for (int k = tid; k < cells; k += BLOCK) {
        const int i = k / g.W, j = k - i * g.W, p = field::padded(g, i, j);
        if (out.dist) out.dist[base + (size_t)k] = field::cell_dist(img, p);
        par[k] = (uint8_t)field::cell_parent(img, p, g.PW, adm[p], g.w1, g.w2);
    }
    __syncthreads(); /* the last barrier */
    if (out.parent) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(out.parent + base);
        for (int q = tid; q < cells / 4; q += BLOCK) dst[q] = second4[q];
    }
    if (wave == 0 && (out.length || out.goal || out.cell)) { /* the summary: wave-uniform throughout */
        const bool go = has_r && par[ri * g.W + rj] <= HRL_FIELD_SOURCE; /* (ri, rj are 0 without r: inside the grid) */
        const int cell = go ? walk(par, g, ri, rj) : -1;
        float x = __builtin_nanf(""), y = __builtin_nanf("");
        if (cell >= 0) route::waypoint_of(g, f, cell, &x, &y);
        if (lane == 0) {
            if (out.length) out.length[env] = go ? field::cell_dist(img, field::padded(g, ri, rj)) : inf_();
            if (out.goal) { out.goal[2 * (size_t)env] = x; out.goal[2 * (size_t)env + 1] = y; }
            if (out.cell) out.cell[env] = cell;
        }
    }
}

}  // namespace

extern "C" {

int hrl_frontier_default_spec(const hrl_config *cfg, hrl_frontier_spec *spec) {
    const int rc = default_spec(cfg, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_frontier_default_spec: null argument or bad env_kind");
}

int hrl_frontier(const hrl_config *cfg, const hrl_buffers *b, const hrl_frontier_spec *spec, const uint8_t *seen, const uint8_t *mask, const hrl_frontier_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(spec);
    if (why.empty()) why = validate_out(out, seen);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_frontier: " + why);
    if (const int rc = check_record(LIB, b, "hrl_frontier: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->edge, "edge", 4}, {out->dist, "dist", 4}, {out->parent, "parent", 4}, {out->count, "count", 4}, {out->length, "length", 4},
                            {out->goal, "goal", 4}, {out->cell, "cell", 4}, {seen, "seen", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 8, &d_dc)) return rc;
    hipLaunchKernelGGL(frontier_kernel, dim3(cfg->num_envs), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, (const float *)b->items,
                       (const int32_t *)b->aux, seen, mask, *out, *spec);
    return launched(LIB);
}

const char *hrl_frontier_last_error(void) { return g_err.c_str(); }

}  // extern "C"
