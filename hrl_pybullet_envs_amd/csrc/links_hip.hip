/*
 * links_hip.hip -- gfx950 (MI355X) implementation of include/hrl_links.h: libhrl_links_hip.so.
 *
 * Sixteen lanes per env: a workgroup of 256 threads takes GROUP = 16 consecutive envs, four to a wave.  Its threads stage the 16 state
 * records (2 KB, consecutive in HBM) in LDS with coalesced loads.  Then lane = link: each of the 13 link lanes of an env evaluates
 * links_core.h's link_out for its link from the staged record -- the leg's kinematics once per lane, the lanes differing only in the
 * selects of their leg and type -- and lane = site: each of the first n_sites lanes evaluates site_out.  The results stay in the lane's
 * registers.
 *
 * They leave one output tensor at a time through one staging row per env: the lanes write their floats to LDS, and the workgroup copies
 * the rows out as ONE CONTIGUOUS RUN OF DWORDS per tensor (16 envs x 39 floats of `origin` are 624 consecutive floats).  The pointers of
 * `out` are kernel arguments and the row width is uniform, so every barrier sits in uniform control flow; the copying threads skip the
 * range of a masked env (its flag is in LDS), and the last workgroup stages and copies N % 16 envs.
 *
 * LDS: 2 KB of state, 3.3 KB of staging rows (16 x 52 floats, the width of `quat`), 16 flags: 5.4 KB.  No scratch.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "links_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::links;

namespace {

constexpr char LIB[] = "hrl_links";
constexpr int BLOCK = 256;
static_assert(BLOCK == GROUP * 16, "sixteen lanes per env");

/* The rows of one tensor, `width` floats per env, from the staging rows to dst.  Called by the whole workgroup. */
__device__ __forceinline__ void flush(float *dst, const float *s_row, const int *s_on, int e0, int n_here, int width, int tid) {
    __syncthreads();
    const size_t base = (size_t)e0 * (size_t)width;
    const int n = n_here * width; /* <= GROUP * ROW_MAX */
    for (int i = tid; i < n; i += BLOCK)
        if (s_on[i / width]) dst[base + (size_t)i] = s_row[i];
    __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void links_kernel(const DevCfg *cfg, const float *state, const uint8_t *mask, hrl_links_out out, hrl_links_spec sp, int n_envs) {
    __shared__ float s_st[GROUP * HRL_STATE_STRIDE];
    __shared__ float s_row[GROUP * ROW_MAX];
    __shared__ int s_on[GROUP];
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, g = tid >> 4, lane = tid & 15;
    const int e0 = blockIdx.x * GROUP;
    const int left = n_envs - e0, n_here = left < GROUP ? left : GROUP; /* >= 1: the grid is ceil(n_envs / GROUP) */
    for (int i = tid; i < n_here * HRL_STATE_STRIDE; i += BLOCK) s_st[i] = state[(size_t)e0 * HRL_STATE_STRIDE + i];
    if (tid < GROUP) s_on[tid] = (tid < n_here && (!mask || mask[e0 + tid])) ? 1 : 0;
    __syncthreads();
    const int B = n_links(c.kind), S = sp.n_sites; /* S <= MAX_S: validate_spec */
    const float *st = s_st + g * HRL_STATE_STRIDE;
    const bool on = s_on[g] != 0, is_link = on && lane < B, is_site = on && lane < S;
    LinkOut L = {};
    SiteOut P = {};
    if (is_link) link_out(c, st, sp.frame, lane, L);
    if (is_site) site_out(c, st, sp.frame, sp.site_link[lane], sp.site_local[lane][0], sp.site_local[lane][1], sp.site_local[lane][2], P);
    const int w3 = 3 * B, w4 = 4 * B, ws = 3 * S;
    if (out.origin) {
        if (is_link) { float *r = s_row + g * w3 + 3 * lane; r[0] = L.origin[0]; r[1] = L.origin[1]; r[2] = L.origin[2]; }
        flush(out.origin, s_row, s_on, e0, n_here, w3, tid);
    }
    if (out.com) {
        if (is_link) { float *r = s_row + g * w3 + 3 * lane; r[0] = L.com[0]; r[1] = L.com[1]; r[2] = L.com[2]; }
        flush(out.com, s_row, s_on, e0, n_here, w3, tid);
    }
    if (out.quat) {
        if (is_link) { float *r = s_row + g * w4 + 4 * lane; r[0] = L.quat[0]; r[1] = L.quat[1]; r[2] = L.quat[2]; r[3] = L.quat[3]; }
        flush(out.quat, s_row, s_on, e0, n_here, w4, tid);
    }
    if (out.lin_vel) {
        if (is_link) { float *r = s_row + g * w3 + 3 * lane; r[0] = L.lin[0]; r[1] = L.lin[1]; r[2] = L.lin[2]; }
        flush(out.lin_vel, s_row, s_on, e0, n_here, w3, tid);
    }
    if (out.ang_vel) {
        if (is_link) { float *r = s_row + g * w3 + 3 * lane; r[0] = L.ang[0]; r[1] = L.ang[1]; r[2] = L.ang[2]; }
        flush(out.ang_vel, s_row, s_on, e0, n_here, w3, tid);
    }
    if (out.site_pos && S > 0) {
        if (is_site) { float *r = s_row + g * ws + 3 * lane; r[0] = P.pos[0]; r[1] = P.pos[1]; r[2] = P.pos[2]; }
        flush(out.site_pos, s_row, s_on, e0, n_here, ws, tid);
    }
    if (out.site_vel && S > 0) {
        if (is_site) { float *r = s_row + g * ws + 3 * lane; r[0] = P.vel[0]; r[1] = P.vel[1]; r[2] = P.vel[2]; }
        flush(out.site_vel, s_row, s_on, e0, n_here, ws, tid);
    }
}

}  // namespace

extern "C" {

int hrl_links_count(int32_t env_kind) { return env_kind < HRL_ANT_FLAT || env_kind > HRL_ANT_FLAGRUN ? 0 : n_links(env_kind); }

const char *hrl_links_name(int32_t env_kind, int32_t i) { return link_name(env_kind, i); }

int hrl_links_default_spec(const hrl_config *cfg, int32_t frame, hrl_links_spec *spec) {
    const int rc = default_spec(cfg, frame, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_links_default_spec: null argument, bad env_kind or unknown frame");
}

int hrl_links(const hrl_config *cfg, const hrl_buffers *b, const hrl_links_spec *spec, const uint8_t *mask, const hrl_links_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(cfg, spec);
    if (why.empty()) why = validate_out(out, spec);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_links: " + why);
    if (const int rc = check_record(LIB, b, "hrl_links: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->origin, "origin", 4},   {out->com, "com", 4},           {out->quat, "quat", 4},         {out->lin_vel, "lin_vel", 4},
                            {out->ang_vel, "ang_vel", 4}, {out->site_pos, "site_pos", 4}, {out->site_vel, "site_vel", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 7, &d_dc)) return rc;
    const int groups = (cfg->num_envs + GROUP - 1) / GROUP;
    hipLaunchKernelGGL(links_kernel, dim3(groups), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, mask, *out, *spec, (int)cfg->num_envs);
    return launched(LIB);
}

const char *hrl_links_last_error(void) { return g_err.c_str(); }

}  // extern "C"
