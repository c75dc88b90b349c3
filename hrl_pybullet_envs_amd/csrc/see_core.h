/*
 * see_core.h -- specification of the batched visibility map (include/hrl_see.h), written once as plain C++: the device kernel
 * (see_hip.hip) and the host build of the tests (tests/see_host, HRL_EMU) compile the same functions and produce the same bits.
 * fp32 throughout, fused operations written out as fma_ (the sources are compiled with -ffp-contract=off).
 *
 * The map of one env is a pure function of (DevCfg, its state / items / aux record, hrl_see_spec, its bytes of `seen`, its `clear`):
 *
 *   frames        field_core.h's frames_of on the grid part of the spec: V = the renderer's camera, T = the probe's table frame, centred
 *                 on the robot with WORLD axes
 *   table         the probe's 70 slots in T (probe_core.h: build_slot under classes = occluders; a plane is the face the robot collides
 *                 with); a slot OCCLUDES when the probe keeps it.  probe::build_frame leaves the heading's forward vector and whether
 *                 the robot's place is finite in the same record
 *   cell_visible  cell (i, j): q = field::cell_centre in T, probe::segment(q) = length L and unit direction d; the verdict of
 *                 include/hrl_see.h -- finite, in range, in the field of view, and no occluding slot with probe::meet < L - slack.  The
 *                 verdict is a boolean "any", so the walk over the list of slots stops once no cell of the run of 64 is still visible
 *                 (any_lane: one lane on the host, the wave on the device): the same bits whenever it stops
 *   merge4        four cells of the memory at once, as the bytes of one word: old = the byte found is not 0 (0 after a clear),
 *                 seen = old | visible as 0 or 1, and the number of cells with visible and not old
 *
 * Totality: no address, loop bound or integer conversion derives from a float of the state or the items.  Every acceptance test is a
 * float comparison that is false for NaN; a slot with a non-finite parameter is not kept and does not occlude.
 */
#pragma once
#include "../../include/hrl_see.h"
#include "field_core.h" /* Grid, Frames, grid_of, frames_of, cell_centre (and through it probe_core.h: ProbeSet, build_slot, build_frame, segment, meet; scan_core.h: forward, default_spec) */

namespace hrl {
namespace see {

using field::Frames;
using field::Grid;
using probe::ProbeSet;
using probe::Seg;
using probe::fin_;

constexpr int S_SLOTS = probe::S_SLOTS; /* 70 */
constexpr int MAX_SIZE = field::MAX_SIZE, MAX_CELLS = field::MAX_CELLS;

#ifdef HRL_EMU
HRL_DEV bool any_lane(bool x) { return x; }
#else
HRL_DEV bool any_lane(bool x) { return __any(x) != 0; } /* (every lane of the wave gets here together: cells come in whole runs of 64) */
#endif

/* the grid of the spec as the field's functions read it (grid_of, frames_of: width, height, mode, centre, half_extent) */
HRL_DEV hrl_field_spec grid_part(const hrl_see_spec &sp) {
    hrl_field_spec f = {};
    f.struct_size = sizeof f; f.width = sp.width; f.height = sp.height; f.mode = sp.mode;
    f.centre[0] = sp.centre[0]; f.centre[1] = sp.centre[1]; f.half_extent = sp.half_extent;
    return f;
}
/* what probe::build_slot keeps and probe::build_frame reads: the occluding classes, the heading frame */
HRL_DEV hrl_probe_spec table_spec(const hrl_see_spec &sp) {
    hrl_probe_spec p = {};
    p.struct_size = sizeof p; p.n_points = 1; p.frame = HRL_PROBE_HEADING; p.classes = sp.occluders & HRL_SCAN_ALL; p.margin = 0.f;
    return p;
}

/* m0 / m1: bit s set = slot s / 64 + s occludes.  S.fwd and S.robot_ok: probe::build_frame under table_spec. */
HRL_DEV uint32_t cell_visible(const ProbeSet &S, unsigned long long m0, unsigned long long m1, const Grid &g, const Frames &f, const hrl_see_spec &sp, int i, int j) {
    float u, v, qx, qy;
    field::cell_centre(g, f, i, j, &u, &v, &qx, &qy);
    Seg r;
    probe::segment(qx, qy, r);
    bool vis = S.robot_ok && fin_(qx) && fin_(qy) && r.len <= sp.max_range;
    vis = vis && (sp.fov_cos <= -1.f || !(r.len > 0.f) || fma_(S.fwd[0], r.dx, S.fwd[1] * r.dy) >= sp.fov_cos);
    const float reach = r.len - sp.slack;
    for (unsigned long long m = m0; m && any_lane(vis); m &= m - 1) vis = vis && !(probe::meet(S, __builtin_ctzll(m), r) < reach);
    for (unsigned long long m = m1; m && any_lane(vis); m &= m - 1) vis = vis && !(probe::meet(S, 64 + __builtin_ctzll(m), r) < reach);
    return vis ? 1u : 0u;
}

/* four cells: vis4 = their bytes of `visible` (0 or 1 each), found4 = their bytes of `seen` as found (anything; 0 after a clear).  Returns
 * their bytes of `seen` as written and adds to *fresh how many of them are visible and were not seen. */
HRL_DEV uint32_t merge4(uint32_t vis4, uint32_t found4, int32_t *fresh) {
    const uint32_t old4 = ((found4 | ((found4 & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; /* byte != 0, per byte: the sum carries into bit 7 and no further */
    *fresh += __builtin_popcount(vis4 & ~old4);
    return old4 | vis4;
}

/* ------------------------------------------------------------------------------------------------ host side */
inline std::string validate_spec(const hrl_see_spec *s) {
    if (!s) return "null see spec";
    if (s->struct_size != sizeof(hrl_see_spec)) return "hrl_see_spec.struct_size is not sizeof(hrl_see_spec): initialise the record with hrl_see_default_spec()";
    if (s->width < HRL_FIELD_MIN_SIZE || s->width > HRL_FIELD_MAX_SIZE || s->width % 8 != 0) return "see width must be a multiple of 8 within 8..64";
    if (s->height < HRL_FIELD_MIN_SIZE || s->height > HRL_FIELD_MAX_SIZE || s->height % 8 != 0) return "see height must be a multiple of 8 within 8..64";
    if (s->mode != HRL_VIEW_WORLD && s->mode != HRL_VIEW_EGO && s->mode != HRL_VIEW_EGO_HEADING) return "unknown see mode";
    if (!(s->half_extent > HRL_FIELD_MIN_HALF_EXTENT) || !(s->half_extent <= HRL_FIELD_MAX_HALF_EXTENT)) return "see half_extent must be finite and within (1e-3, 1e4]";
    if ((s->occluders & ~HRL_SCAN_ALL) != 0u) return "see occluders must be a mask of HRL_SCAN_WALL | BOX | FOOD | POISON | TARGET (0 = nothing occludes)";
    if (!(s->max_range > 0.f) || !(s->max_range <= 3.0e38f)) return "see max_range must be finite and positive";
    if (!(s->fov_cos >= -1.f) || !(s->fov_cos <= 1.f)) return "see fov_cos must be within -1..1 (-1 = all round)";
    if (!(s->slack >= 0.f) || !(s->slack <= HRL_PROBE_MAX_MARGIN)) return "see slack must be finite and within 0..2";
    return "";
}
/* (after validate_spec) */
inline std::string validate_out(const hrl_see_out *o, const hrl_see_spec *s) {
    if (!o) return "null see out";
    if (!o->visible && !o->seen && !o->fresh) return "see out holds no pointer: at least one output must be given";
    if (o->seen && s->mode != HRL_VIEW_WORLD) return "see seen needs HRL_VIEW_WORLD: an ego grid moves under the memory";
    if (o->fresh && !o->seen) return "see fresh needs seen: it counts the cells the memory did not hold";
    if (o->visible && o->visible == o->seen) return "see visible and seen must not be the same pointer";
    return "";
}

inline int default_spec(const hrl_config *c, int32_t mode, hrl_see_spec *s) {
    hrl_field_spec f;
    hrl_scan_spec r;
    if (!s || field::default_spec(c, mode, &f) != HRL_OK || scan::default_spec(c, HRL_SCAN_HEADING, &r) != HRL_OK) return HRL_ERR_BAD_ARG;
    memset(s, 0, sizeof(*s));
    s->struct_size = sizeof(*s); s->width = f.width; s->height = f.height; s->mode = mode;
    s->centre[0] = f.centre[0]; s->centre[1] = f.centre[1]; s->half_extent = f.half_extent;
    s->occluders = HRL_SCAN_WALL | HRL_SCAN_BOX;
    s->max_range = r.max_range;
    s->fov_cos = -1.f;
    s->slack = (2.0f / (float)f.width) * f.half_extent; /* one cell: field::grid_of's expression */
    return HRL_OK;
}

#ifdef HRL_EMU
/* One env on the host, partitioned as the kernel partitions it: the table and its list, runs of 64 cells, then the memory a word at a
 * time.  centres (may be null): [H][W][2], the cell centres in T. */
inline void see_env_host(const DevCfg &c, const float *st, const float *items, const int32_t *aux, const hrl_see_spec &sp, bool clear, const hrl_see_out &out, size_t env, float *centres) {
    static thread_local ProbeSet S;
    static thread_local uint32_t vis4[MAX_CELLS / 4];
    uint8_t *vis = reinterpret_cast<uint8_t *>(vis4);
    const hrl_field_spec fs = grid_part(sp);
    const hrl_probe_spec ps = table_spec(sp);
    const Grid g = field::grid_of(fs);
    const Frames f = field::frames_of(st, fs);
    probe::build_frame(S, st, ps);
    for (int slot = 0; slot < S_SLOTS; ++slot) probe::build_slot(S, slot, c, st, items, aux, f.T, ps);
    unsigned long long m0 = 0, m1 = 0;
    for (int slot = 0; slot < 64; ++slot) if (probe::kept(S, slot)) m0 |= 1ull << slot;
    for (int slot = 64; slot < S_SLOTS; ++slot) if (probe::kept(S, slot)) m1 |= 1ull << (slot - 64);
    const int cells = g.W * g.H;
    const size_t base = env * (size_t)cells;
    for (int k = 0; k < cells; ++k) {
        const int i = k / g.W, j = k - i * g.W;
        vis[k] = (uint8_t)cell_visible(S, m0, m1, g, f, sp, i, j);
        if (centres) {
            float u, v;
            field::cell_centre(g, f, i, j, &u, &v, &centres[2 * k], &centres[2 * k + 1]);
        }
    }
    if (out.visible) memcpy(out.visible + base, vis, (size_t)cells);
    if (out.seen) {
        int32_t fresh = 0;
        for (int q = 0; q < cells / 4; ++q) {
            uint32_t found = 0u;
            if (!clear) memcpy(&found, out.seen + base + 4 * (size_t)q, 4);
            const uint32_t now = merge4(vis4[q], found, &fresh);
            memcpy(out.seen + base + 4 * (size_t)q, &now, 4);
        }
        if (out.fresh) out.fresh[env] = fresh;
    }
}
/* hrl_see on host pointers; returns the status and leaves the reason in `why`; centres (may be null): [num_envs][H][W][2] */
inline int see_host_batch(const hrl_config *cfg, const hrl_buffers *b, const hrl_see_spec *sp, const uint8_t *clear, const uint8_t *mask, const hrl_see_out *out, float *centres,
                          std::string &why) {
    why = validate(cfg);
    if (why.empty()) why = validate_spec(sp);
    if (why.empty()) why = validate_out(out, sp);
    if (why.empty() && (!b || !b->state || !b->aux)) why = "null buffer";
    if (!why.empty()) return HRL_ERR_BAD_ARG;
    DevCfg dc;
    build_devcfg(*cfg, dc);
    const size_t cells = (size_t)sp->width * (size_t)sp->height;
    for (int e = 0; e < cfg->num_envs; ++e) {
        if (mask && !mask[e]) continue;
        see_env_host(dc, b->state + (size_t)e * HRL_STATE_STRIDE, b->items ? b->items + (size_t)e * dc.items_stride : nullptr, b->aux + (size_t)e * HRL_AUX_STRIDE, *sp,
                     clear && clear[e], *out, (size_t)e, centres ? centres + (size_t)e * cells * 2 : nullptr);
    }
    return HRL_OK;
}
#endif

}  // namespace see
}  // namespace hrl
