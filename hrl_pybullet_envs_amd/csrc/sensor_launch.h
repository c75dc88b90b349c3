/*
 * sensor_launch.h -- the host side that the nine sensor libraries share (render_hip.hip, scan_hip.hip, probe_hip.hip, field_hip.hip,
 * route_hip.hip, see_hip.hip, frontier_hip.hip, camera_hip.hip, links_hip.hip): the error string, the guards of the buffer record and of the
 * pointers' alignment and devices, the cache of kernel constants, the prologue of a launch (prepare) and its epilogue (launched).  Host
 * only; `lib` is the library's name as its messages carry it ("hrl_scan").
 *
 * Everything here has INTERNAL linkage (one unnamed namespace, no inline or template statics): the libraries are loaded into one
 * process, and the dynamic loader may unify a symbol of vague linkage across them -- hrl_scan_last_error() would answer with the
 * renderer's message.  Each library therefore holds its own copy of the state below.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "host_cfg.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const std::string &what) { return fail(HRL_ERR_HIP, what + ": " + hipGetErrorString(e)); }

/* The kernel constants of every (device, config) this process has used, uploaded once and kept: a launch with a known config allocates
 * and copies nothing (graph capture).  Entries are never freed -- a captured graph may hold their address. */
struct CacheEntry { int device; hrl_config cfg; hrl::DevCfg *d_dc; };
std::mutex g_mutex;
std::vector<CacheEntry> g_cache;
constexpr size_t CACHE_MAX = 1024; /* 0.7 MB of constants */

int devcfg_for(const char *lib, const hrl_config *cfg, int device, hrl::DevCfg **out) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (const CacheEntry &e : g_cache)
        if (e.device == device && memcmp(&e.cfg, cfg, sizeof(hrl_config)) == 0) { *out = e.d_dc; return HRL_OK; }
    if (g_cache.size() >= CACHE_MAX)
        return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": more than 1024 distinct configs used by this process (their constants are kept for captured graphs)");
    hrl::DevCfg dc, *d = nullptr;
    hrl::build_devcfg(*cfg, dc);
    hipError_t e = hipMalloc((void **)&d, sizeof(hrl::DevCfg));
    if (e == hipSuccess) e = hipMemcpy(d, &dc, sizeof(hrl::DevCfg), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return hip_fail(e, std::string(lib) + ": device constants (the first call with a config must happen outside stream capture)");
    }
    g_cache.push_back(CacheEntry{device, *cfg, d});
    *out = d;
    return HRL_OK;
}

/* the buffer record: present, of a known size, with the two records every sensor reads; `nulls` is the library's whole message for a null
 * pointer (it names the library's own outputs too where the library refuses them in the same words) */
int check_record(const char *lib, const hrl_buffers *b, const char *nulls) {
    if (!b) return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": null buffer record");
    if (b->struct_size < HRL_BUFFERS_SIZE_V7_BASE || b->struct_size > 4096 || b->struct_size % sizeof(void *) != 0)
        return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": hrl_buffers.struct_size is not the size of a known layout: initialise the record with hrl_buffers_init() (include/hrl_envs.h)");
    if (!b->state || !b->aux) return fail(HRL_ERR_BAD_ARG, nulls);
    return HRL_OK;
}

/* where a launch goes: the current device, and whether pointers may be looked at -- not while the stream is being captured (the pointers
 * were looked at by the call that came before the capture) */
struct Context { int device; bool inspect; };

int device_context(const char *lib, void *stream, Context *ctx) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(HRL_ERR_NO_DEVICE, std::string(lib) + ": no HIP device (this library has no CPU path)");
    }
    if (hipGetDevice(&ctx->device) != hipSuccess) return fail(HRL_ERR_HIP, std::string(lib) + ": hipGetDevice");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
    ctx->inspect = cap == hipStreamCaptureStatusNone;
    return HRL_OK;
}

/* the device guard of the step library (hrl_hip.hip: check_call): a launch goes to the CURRENT device, so the buffers must live there.
 * A null pointer is an output that is not asked for. */
int check_device(const char *lib, const Context &ctx, const void *p, const char *name) {
    if (!ctx.inspect || !p) return HRL_OK;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": " + name + " is not memory the HIP runtime knows (device pointers are required)");
    }
    if (a.type == hipMemoryTypeDevice && a.device != ctx.device)
        return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": " + name + " lives on HIP device " + std::to_string(a.device) + ", the current device is " + std::to_string(ctx.device) +
                                         ": hipSetDevice(" + std::to_string(a.device) + ") before calling");
    return HRL_OK;
}

/* A pointer a launch is handed, as the messages name it; `align`: the bytes its address must be a multiple of, 0 = not checked here. */
struct Pointer { const void *p; const char *name; unsigned align; };

/* What the entry points of the record-style sensors do between check_record and the launch, in this order: the alignment of `ptrs` in
 * list order (a null pointer is aligned), the context, the device of `state` and of `ptrs` in list order, the kernel constants. */
int prepare(const char *lib, const hrl_config *cfg, const hrl_buffers *b, void *stream, const Pointer *ptrs, int n, hrl::DevCfg **d_dc) {
    for (int i = 0; i < n; ++i)
        if (ptrs[i].align && reinterpret_cast<uintptr_t>(ptrs[i].p) % ptrs[i].align != 0)
            return fail(HRL_ERR_BAD_ARG, std::string(lib) + ": " + ptrs[i].name + " must be " + std::to_string(ptrs[i].align) + "-byte aligned");
    Context ctx;
    if (const int rc = device_context(lib, stream, &ctx)) return rc;
    if (const int rc = check_device(lib, ctx, b->state, "state")) return rc;
    for (int i = 0; i < n; ++i)
        if (const int rc = check_device(lib, ctx, ptrs[i].p, ptrs[i].name)) return rc;
    return devcfg_for(lib, cfg, ctx.device, d_dc);
}

/* after hipLaunchKernelGGL */
int launched(const char *lib) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HRL_OK : hip_fail(e, std::string(lib) + " launch");
}

}  // namespace
