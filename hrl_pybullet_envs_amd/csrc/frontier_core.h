/*
 * frontier_core.h -- specification of the batched frontier map (include/hrl_frontier.h), written once as plain C++: the device kernel
 * (frontier_hip.hip) and the host build of the tests (tests/frontier_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The map of one env is a pure function of (DevCfg, its state / items / aux record, hrl_frontier_spec, its bytes of `seen`):
 *
 *   geometry     field_core.h's, for field_part(spec) -- the world mode, the class part of `sources` -- : frames_of, build_entry and
 *                g(c) = field::cell_init.  Nothing of it is restated here
 *   robot_cell   r: the lowest row with route::row_holds and the lowest column with route::col_holds, asked of the robot's entry (su, sv
 *                of field::E_ROBOT, which build_entry fills whatever `sources` says); it exists when the robot's place is finite and both
 *                are found.  No float becomes an integer
 *   known        a bit per cell (known4, known_at): whether the byte of `seen` is not 0, and 1 at r
 *   cell_edge    known(c), g(c) is not BLOCKED_, and an orthogonal neighbour inside the grid is not known
 *   cell_value   what the relaxation starts from: known ? g : (OPTIMISTIC ? (g == 0 ? 0 : +inf) : BLOCKED_), then 0 where edge(c) and
 *                `sources` holds HRL_FRONTIER_EDGE
 *   field        field::cell_adm, cell_relax to the fixed point (cap W H rounds), cell_parent and cell_dist on the padded image, unchanged:
 *                the values are again 0, +inf or BLOCKED_ before the first round, so field_core.h's argument that the fixed point is unique
 *                and independent of the order of relaxation carries over word for word
 *   walk         c_0 = r, c_{t+1} = c_t moved by parent[c_t], at most W H steps; the cell it stands on if that is a SOURCE, else -1
 *   summary      count = the number of edge cells; length = cell_dist at r; cell = walk from r; goal = route::waypoint_of(cell).  Without
 *                r, or with r blocked or unreached (parent > SOURCE): length +inf, cell -1, goal NaN
 *
 * Totality: the field's.  The walk's addresses derive from the parent bytes and from r, found by comparisons; the bytes of `seen` are
 * only compared with 0.
 */
#pragma once
#include "../../include/hrl_frontier.h"
#include "route_core.h" /* col_holds, row_holds, waypoint_of, uniform_ (and through it field_core.h: Grid, Frames, FieldSet, build_entry, cell_init, cell_adm, cell_relax, cell_parent, cell_dist) */

namespace hrl {
namespace frontier {

using field::BLOCKED_;
using field::FieldSet;
using field::Frames;
using field::Grid;
using render::inf_;

constexpr int MAX_SIZE = field::MAX_SIZE, MAX_CELLS = field::MAX_CELLS, MAX_PADDED = field::MAX_PADDED;
constexpr uint32_t CLASS_SOURCES = HRL_FIELD_ROBOT | HRL_SCAN_FOOD | HRL_SCAN_POISON | HRL_SCAN_TARGET;

/* the spec's geometry as the field's own record: the world mode, the class part of the sources (it may be empty) */
HRL_BOTH hrl_field_spec field_part(const hrl_frontier_spec &sp) {
    hrl_field_spec f = {};
    f.struct_size = sizeof f; f.width = sp.width; f.height = sp.height; f.mode = HRL_VIEW_WORLD;
    f.centre[0] = sp.centre[0]; f.centre[1] = sp.centre[1]; f.half_extent = sp.half_extent;
    f.blocking = sp.blocking; f.sources = sp.sources & CLASS_SOURCES; f.margin = sp.margin;
    return f;
}

/* The memory as the kernel keeps it: a bit per cell, bit k & 7 of byte k >> 3 for the row-major cell k = i W + j.
 * known4: four cells of `seen` as the bytes of one word -> their four bits, bit b = byte b is not 0 (the sum carries into bit 7 of a byte
 * and no further). */
HRL_DEV uint32_t known4(uint32_t found4) {
    const uint32_t old4 = ((found4 | ((found4 & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
    return (old4 & 1u) | ((old4 >> 7) & 2u) | ((old4 >> 14) & 4u) | ((old4 >> 21) & 8u);
}
HRL_DEV bool known_at(const uint8_t *bits, int k) { return ((bits[k >> 3] >> (k & 7)) & 1u) != 0u; }
/* gv = g(c) */
HRL_DEV bool cell_edge(const uint8_t *bits, const Grid &g, int i, int j, float gv) {
    const int k = i * g.W + j;
    const bool hidden = (j + 1 < g.W && !known_at(bits, k + 1)) || (j > 0 && !known_at(bits, k - 1)) || (i > 0 && !known_at(bits, k - g.W)) || (i + 1 < g.H && !known_at(bits, k + g.W));
    return known_at(bits, k) && gv != BLOCKED_ && hidden;
}
HRL_DEV float cell_value(float gv, bool known, bool edge, uint32_t sources, int32_t unknown) {
    const float hidden = unknown == HRL_FRONTIER_OPTIMISTIC ? (gv == 0.f ? 0.f : inf_()) : BLOCKED_;
    const float v = known ? gv : hidden;
    return edge && (sources & HRL_FRONTIER_EDGE) != 0u ? 0.f : v;
}
/* From the cell (i, j), which has a way (parent <= HRL_FIELD_SOURCE).  par: the parent bytes [H][W].  The same in every lane of a wave. */
HRL_DEV int walk(const uint8_t *par, const Grid &g, int i, int j) {
    const int cap = g.W * g.H;
    for (int t = 0; t < cap; ++t) {
        const int k = route::uniform_((int)par[i * g.W + j]);
        if (k > 7) break;
        i += field::drow(k); j += field::dcol(k);
    }
    return par[i * g.W + j] == HRL_FIELD_SOURCE ? i * g.W + j : -1;
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_frontier_spec *s) {
    if (!s) return "null frontier spec";
    if (s->struct_size != sizeof(hrl_frontier_spec)) return "hrl_frontier_spec.struct_size is not sizeof(hrl_frontier_spec): initialise the record with hrl_frontier_default_spec()";
    hrl_field_spec f = field_part(*s);
    f.sources = HRL_FIELD_ROBOT; /* (the field refuses an empty set; here the class part may be empty) */
    const std::string why = field::validate_spec(&f);
    if (!why.empty()) return "frontier " + why;
    if (s->sources == 0u || (s->sources & ~(HRL_FRONTIER_EDGE | CLASS_SOURCES)) != 0u)
        return "frontier sources must be a non-empty mask of HRL_FRONTIER_EDGE | HRL_FIELD_ROBOT | HRL_SCAN_FOOD | POISON | TARGET (a wall or the box is no source)";
    if (s->unknown != HRL_FRONTIER_KNOWN_ONLY && s->unknown != HRL_FRONTIER_OPTIMISTIC) return "frontier unknown must be HRL_FRONTIER_KNOWN_ONLY or HRL_FRONTIER_OPTIMISTIC";
    return "";
}
inline std::string validate_out(const hrl_frontier_out *o, const uint8_t *seen) {
    if (!o) return "null frontier out";
    if (!o->edge && !o->dist && !o->parent && !o->count && !o->length && !o->goal && !o->cell) return "frontier out holds no pointer: at least one output must be given";
    if (!seen) return "frontier seen is null: the memory of hrl_see is required";
    if (seen == o->edge || seen == o->parent) return "frontier seen must not be the memory of edge or parent: it is only read";
    return "";
}
inline int default_spec(const hrl_config *c, hrl_frontier_spec *s) {
    hrl_field_spec f;
    if (!s || field::default_spec(c, HRL_VIEW_WORLD, &f) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->width = f.width; s->height = f.height;
    s->centre[0] = f.centre[0]; s->centre[1] = f.centre[1]; s->half_extent = f.half_extent;
    s->blocking = f.blocking; s->sources = HRL_FRONTIER_EDGE; s->margin = f.margin; s->unknown = HRL_FRONTIER_KNOWN_ONLY;
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, in the kernel's order: the table, g, the memory with the robot's cell, value and edge, the relaxation under
 * `schedule` (field_core.h: SCHED_*), the outputs, the summary.  seen: the env's bytes [H][W].  Returns the rounds it ran. */
inline int frontier_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_frontier_spec &sp, const uint8_t *seen, int schedule,
                             const hrl_frontier_out &out, size_t env) {
    static thread_local FieldSet F;
    static thread_local float img[2][MAX_PADDED];
    static thread_local uint8_t adm[MAX_PADDED], bits[MAX_CELLS / 8], edge[MAX_CELLS], par[MAX_CELLS];
    const hrl_field_spec fs = field_part(sp);
    const Grid g = field::grid_of(fs);
    const Frames f = field::frames_of(st, fs);
    for (int e = 0; e < field::N_ENTRIES; ++e) field::build_entry(F, e, c, st, items, aux, f, fs);
    unsigned long long b0 = 0, b1 = 0, s0 = 0, s1 = 0;
    for (int e = 0; e < field::N_ENTRIES; ++e) {
        if (F.flags[e] & field::F_BLOCKS) (e < 64 ? b0 : b1) |= 1ull << (e & 63);
        if (F.flags[e] & field::F_SOURCE) (e < 64 ? s0 : s1) |= 1ull << (e & 63);
    }
    int ri = -1, rj = -1;
    for (int k = g.W - 1; k >= 0; --k) rj = route::col_holds(g, F.su[field::E_ROBOT], k) ? k : rj;
    for (int k = g.H - 1; k >= 0; --k) ri = route::row_holds(g, F.sv[field::E_ROBOT], k) ? k : ri;
    const bool has_r = f.robot_ok && ri >= 0 && rj >= 0;
    const int cells = g.W * g.H, n_padded = g.PW * (g.H + 2);
    for (int q = 0; q < cells / 4; q += 2) { /* two words of four cells make a byte */
        uint32_t lo, hi;
        memcpy(&lo, seen + 4 * (size_t)q, 4); memcpy(&hi, seen + 4 * (size_t)q + 4, 4);
        bits[q >> 1] = (uint8_t)(known4(lo) | (known4(hi) << 4));
    }
    if (has_r) bits[(ri * g.W + rj) >> 3] |= (uint8_t)(1u << ((ri * g.W + rj) & 7));
    for (int p = 0; p < n_padded; ++p) { img[0][p] = BLOCKED_; adm[p] = 0; }
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) img[0][field::padded(g, i, j)] = field::cell_init(F, b0, b1, s0, s1, g, f, fs.margin, i, j);
    int32_t count = 0;
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) {
            const int p = field::padded(g, i, j), k = i * g.W + j;
            const bool ed = cell_edge(bits, g, i, j, img[0][p]);
            img[0][p] = cell_value(img[0][p], known_at(bits, k), ed, sp.sources, sp.unknown);
            edge[k] = ed ? 1 : 0;
            count += ed ? 1 : 0;
        }
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) adm[field::padded(g, i, j)] = (uint8_t)field::cell_adm(img[0], field::padded(g, i, j), g.PW);
    memcpy(img[1], img[0], sizeof(float) * (size_t)n_padded);
    int cur = 0, rounds = 0;
    for (int r = 0; r < cells; ++r) {
        bool changed = false;
        ++rounds;
        if (schedule == field::SCHED_JACOBI) {
            for (int p = 0; p < n_padded; ++p)
                if (adm[p]) {
                    const float old = img[cur][p], d = field::cell_relax(img[cur], p, g.PW, adm[p], g.w1, g.w2);
                    img[cur ^ 1][p] = d; changed = changed || d != old;
                }
            cur ^= 1;
        } else {
            for (int q = 0; q < n_padded; ++q) {
                const int p = schedule == field::SCHED_FORWARD ? q : n_padded - 1 - q;
                if (adm[p]) {
                    const float old = img[cur][p], d = field::cell_relax(img[cur], p, g.PW, adm[p], g.w1, g.w2);
                    img[cur][p] = d; changed = changed || d != old;
                }
            }
        }
        if (!changed) break;
    }
    const size_t base = env * (size_t)cells;
    for (int i = 0; i < g.H; ++i)
        for (int j = 0; j < g.W; ++j) {
            const int p = field::padded(g, i, j), k = i * g.W + j;
            par[k] = (uint8_t)field::cell_parent(img[cur], p, g.PW, adm[p], g.w1, g.w2);
            if (out.dist) out.dist[base + (size_t)k] = field::cell_dist(img[cur], p);
        }
    if (out.edge) memcpy(out.edge + base, edge, (size_t)cells);
    if (out.parent) memcpy(out.parent + base, par, (size_t)cells);
    if (out.count) out.count[env] = count;
    const bool go = has_r && par[(has_r ? ri : 0) * g.W + (has_r ? rj : 0)] <= HRL_FIELD_SOURCE;
    const int cell = go ? walk(par, g, ri, rj) : -1;
    float x = __builtin_nanf(""), y = __builtin_nanf("");
    if (cell >= 0) route::waypoint_of(g, f, cell, &x, &y);
    if (out.length) out.length[env] = go ? field::cell_dist(img[cur], field::padded(g, ri, rj)) : inf_();
    if (out.goal) { out.goal[2 * env] = x; out.goal[2 * env + 1] = y; }
    if (out.cell) out.cell[env] = cell;
    return rounds;
}
/* hrl_frontier on host pointers; returns the status and leaves the reason in `why`; rounds (may be null): [num_envs] */
inline int frontier_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_frontier_spec *sp, const uint8_t *seen, const uint8_t *mask, const hrl_frontier_out *out,
                               int schedule, int32_t *rounds, std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out, seen);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (why.empty() && (schedule < field::SCHED_JACOBI || schedule > field::SCHED_REVERSE)) why = "unknown schedule";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    const size_t cells = (size_t)sp->width * (size_t)sp->height;
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        const int r = frontier_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE,
                                        *sp, seen + (size_t)e * cells, schedule, *out, (size_t)e);
        if (rounds) rounds[e] = r;
    }
    return HRL_OK;
}
#endif

}  // namespace frontier
}  // namespace hrl
