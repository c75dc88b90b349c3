/*
 * dyn_hip.hip -- gfx950 (MI355X) implementation of include/hrl_dyn.h: libhrl_dyn_hip.so.
 *
 * Sixteen lanes per env, as in links_hip.hip: a workgroup of 256 threads takes GROUP = 16 consecutive envs, four to a wave, and stages
 * their state records (2 KB, consecutive in HBM) in LDS with coalesced loads.  The phases of dyn_core.h then run on the env's 16-lane
 * row, each env's values crossing between them through its Work record in LDS:
 *
 *   lane = body      body_terms: the nine rigid bodies' world inertias, velocities and bias wrenches (one lane for the cube)
 *   lane = leg       leg_terms: the composite inertias passed up the depth-two legs, the joint blocks of M, the legs' pivots
 *   lane = entry     base_terms (27 entries over the 16 lanes), total_terms (10)
 *   one lane         base_solve: the 6 x 6 factorisation; then lane = leg again for leg_back
 *   lane = entry     the 196 entries of mass, lane, lane + 16, ...; the 14 of bias and accel
 *   lane = site      jac_site, JAC_CHUNK sites at a time
 *
 * Each output leaves through one staging row per env: the lanes write their floats to LDS, and the workgroup copies the rows out as ONE
 * CONTIGUOUS RUN OF DWORDS per tensor (16 envs x 196 floats of `mass` are 3136 consecutive floats).  The pointers of `out`, the kind and
 * the spec are kernel arguments or constants of the launch, so every barrier sits in uniform control flow; the copying threads skip the
 * range of a masked env (its flag is in LDS), and the last workgroup stages and copies N % 16 envs.
 *
 * LDS: 2 KB of state, 43.1 KB of Work records (16 x 690 floats), 12.3 KB of staging rows (16 x 196 floats), 16 flags: 57.4 KB (two workgroups per CU).  No scratch.
 *
 * The host side of the entry point -- the guards, the cache of kernel constants, the launch epilogue -- is sensor_launch.h, shared with
 * the other sensor libraries.
 */
#include <hip/hip_runtime.h>

#include "dyn_core.h"
#include "sensor_launch.h"

using namespace hrl;
using namespace hrl::dyn;

namespace {

constexpr char LIB[] = "hrl_dyn";
constexpr int BLOCK = 256;
static_assert(BLOCK == GROUP * 16, "sixteen lanes per env");

/* `width` floats per env from the staging rows to dst, where an env owns `stride` floats and the run starts `offset` floats into them
 * (offset + width <= stride).  Called by the whole workgroup. */
__device__ __forceinline__ void flush(float *dst, const float *s_row, const int *s_on, int e0, int n_here, int width, int stride, int offset, int tid) {
    __syncthreads();
    const int n = n_here * width; /* <= GROUP * ROW_MAX */
    for (int i = tid; i < n; i += BLOCK) {
        const int e = i / width, j = i - e * width;
        if (s_on[e]) dst[(size_t)(e0 + e) * (size_t)stride + (size_t)(offset + j)] = s_row[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void dyn_kernel(const DevCfg *cfg, const float *state, const float *tau, const uint8_t *mask, hrl_dyn_out out, hrl_dyn_spec sp_, int n_envs) {
    __shared__ float s_st[GROUP * HRL_STATE_STRIDE];
    __shared__ Work s_w[GROUP];
    __shared__ float s_row[GROUP * ROW_MAX];
    __shared__ int s_on[GROUP];
    const DevCfg &c = *cfg;
    const int tid = threadIdx.x, g = tid >> 4, lane = tid & 15;
    const int e0 = blockIdx.x * GROUP;
    const int left = n_envs - e0, n_here = left < GROUP ? left : GROUP; /* >= 1: the grid is ceil(n_envs / GROUP) */
    const bool ant = c.kind != HRL_POINT_GATHER, solve = out.accel != nullptr;
    const int nv = nv_of(c.kind), S = sp_.n_sites; /* S <= MAX_S: validate_spec */
    for (int i = tid; i < n_here * HRL_STATE_STRIDE; i += BLOCK) s_st[i] = state[(size_t)e0 * HRL_STATE_STRIDE + i];
    if (tid < GROUP) s_on[tid] = (tid < n_here && (!mask || mask[e0 + tid])) ? 1 : 0;
    Work &W = s_w[g];
    if (g < n_here && lane < nv) W.tau[lane] = (solve && tau) ? tau[(size_t)(e0 + g) * (size_t)nv + (size_t)lane] : 0.f;
    __syncthreads();
    const float *st = s_st + g * HRL_STATE_STRIDE;
    const bool on = s_on[g] != 0;
    if (on && lane < (ant ? NB : 1)) body_terms(c, st, lane, W);
    __syncthreads();
    if (on && ant && lane < 4) leg_terms(c, st, lane, solve, W);
    __syncthreads();
    if (on) {
        base_terms(c, lane, W);
        if (lane + 16 < 27) base_terms(c, lane + 16, W);
        if (lane < 10) total_terms(c, lane, W);
    }
    __syncthreads();
    if (solve) {
        if (on && lane == 0) base_solve(c, W);
        __syncthreads();
        if (on && ant && lane < 4) leg_back(lane, W);
        __syncthreads();
    }
    const int nn = nv * nv;
    if (out.mass) {
        if (on)
            for (int i = lane; i < nn; i += 16) s_row[g * nn + i] = mass_entry(c, W, i);
        flush(out.mass, s_row, s_on, e0, n_here, nn, nn, 0, tid);
    }
    if (out.bias) {
        if (on && lane < nv) s_row[g * nv + lane] = bias_entry(W, lane);
        flush(out.bias, s_row, s_on, e0, n_here, nv, nv, 0, tid);
    }
    if (out.accel) {
        if (on && lane < nv) s_row[g * nv + lane] = W.x[lane];
        flush(out.accel, s_row, s_on, e0, n_here, nv, nv, 0, tid);
    }
    if (out.jac) {
        const int w1 = 3 * nv;
        for (int s0 = 0; s0 < S; s0 += JAC_CHUNK) { /* S is the launch's: uniform */
            const int cnt = S - s0 < JAC_CHUNK ? S - s0 : JAC_CHUNK, wc = cnt * w1;
            if (on && lane >= s0 && lane < s0 + cnt)
                jac_site(c, st, sp_.site_link[lane], sp_.site_local[lane][0], sp_.site_local[lane][1], sp_.site_local[lane][2], s_row + g * wc + (lane - s0) * w1);
            flush(out.jac, s_row, s_on, e0, n_here, wc, S * w1, s0 * w1, tid);
        }
    }
    if (out.com || out.momentum || out.energy) {
        Summary o = {};
        if (on && lane == 0) summary(c, st, W, o);
        if (out.com) {
            if (on && lane == 0) { float *r = s_row + g * 3; r[0] = o.com[0]; r[1] = o.com[1]; r[2] = o.com[2]; }
            flush(out.com, s_row, s_on, e0, n_here, 3, 3, 0, tid);
        }
        if (out.momentum) {
            if (on && lane == 0) {
                float *r = s_row + g * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) r[k] = o.mom[k];
            }
            flush(out.momentum, s_row, s_on, e0, n_here, 6, 6, 0, tid);
        }
        if (out.energy) {
            if (on && lane == 0) { float *r = s_row + g * 2; r[0] = o.en[0]; r[1] = o.en[1]; }
            flush(out.energy, s_row, s_on, e0, n_here, 2, 2, 0, tid);
        }
    }
}

}  // namespace

extern "C" {

int hrl_dyn_nv(int32_t env_kind) { return env_kind < HRL_ANT_FLAT || env_kind > HRL_ANT_FLAGRUN ? 0 : nv_of(env_kind); }

int hrl_dyn_default_spec(const hrl_config *cfg, hrl_dyn_spec *spec) {
    const int rc = default_spec(cfg, spec);
    return rc == HRL_OK ? rc : fail(rc, "hrl_dyn_default_spec: null argument or bad env_kind");
}

int hrl_dyn(const hrl_config *cfg, const hrl_buffers *b, const hrl_dyn_spec *spec, const float *tau, const uint8_t *mask, const hrl_dyn_out *out, void *stream) {
    std::string why = validate(cfg);
    if (why.empty()) why = validate_spec(cfg, spec);
    if (why.empty()) why = validate_out(out, spec);
    if (!why.empty()) return fail(HRL_ERR_BAD_ARG, "hrl_dyn: " + why);
    if (const int rc = check_record(LIB, b, "hrl_dyn: null state or aux")) return rc;
    const Pointer ptrs[] = {{out->mass, "mass", 4}, {out->bias, "bias", 4}, {out->accel, "accel", 4},       {out->jac, "jac", 4},
                            {out->com, "com", 4},   {out->momentum, "momentum", 4}, {out->energy, "energy", 4}, {tau, "tau", 4}};
    DevCfg *d_dc = nullptr;
    if (const int rc = prepare(LIB, cfg, b, stream, ptrs, 8, &d_dc)) return rc;
    const int groups = (cfg->num_envs + GROUP - 1) / GROUP;
    hipLaunchKernelGGL(dyn_kernel, dim3(groups), dim3(BLOCK), 0, (hipStream_t)stream, (const DevCfg *)d_dc, (const float *)b->state, tau, mask, *out, *spec, (int)cfg->num_envs);
    return launched(LIB);
}

const char *hrl_dyn_last_error(void) { return g_err.c_str(); }

}  // extern "C"
