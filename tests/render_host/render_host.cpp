/* csrc/render_core.h compiled for the host (HRL_EMU): what the device kernel must reproduce byte for byte.  Loaded with ctypes
 * (tests/render_cases.py). */
#include "../../hrl_pybullet_envs_amd/csrc/render_core.h"

static thread_local std::string g_why;

extern "C" {
/* hrl_render on host pointers */
int render_host(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_view *view, const uint8_t *mask, uint8_t *rgb) {
    return hrl::render::render_host_batch(cfg, bufs, view, mask, rgb, g_why);
}
const char *render_host_last_error(void) { return g_why.c_str(); }
int render_host_default_view(const hrl_config *cfg, int32_t mode, hrl_view *view) { return hrl::render::default_view(cfg, mode, view); }
}

#include "check_cases.h"
extern "C" {
int render_check_n_cases(void) { return render_check::n_cases(); }
/* the checksum of case k of render_check_main, from this (unsanitised) build; name: at least 64 bytes */
int render_check_case(int k, char *name, unsigned long long *checksum) {
    uint64_t s = 0;
    const int rc = render_check::run_case(k, name, 64, &s);
    *checksum = s;
    return rc;
}
}
