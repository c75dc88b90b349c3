/* csrc/cast_core.h compiled for the host (HRL_EMU): what the device kernel must reproduce bit for bit.  Loaded with ctypes
 * (tests/cast_cases.py). */
#include "../../hrl_pybullet_envs_amd/csrc/cast_core.h"

static thread_local std::string g_why;

extern "C" {
/* hrl_cast on host pointers */
int cast_host(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_cast_spec *spec, const float *rays, const int32_t *ray_link, const uint8_t *mask, const hrl_cast_out *out) {
    return hrl::cast::cast_host_batch(cfg, bufs, spec, rays, ray_link, mask, out, g_why);
}
const char *cast_host_last_error(void) { return g_why.c_str(); }
int cast_host_default_spec(const hrl_config *cfg, int32_t frame, hrl_cast_spec *spec) { return hrl::cast::default_spec(cfg, frame, spec); }
}

#include "check_cases.h"
extern "C" {
int cast_check_n_cases(void) { return cast_check::n_cases(); }
/* the checksum of case k of cast_check_main, from this (unsanitised) build; name: at least 64 bytes */
int cast_check_case(int k, char *name, unsigned long long *checksum) {
    uint64_t s = 0;
    const int rc = cast_check::run_case(k, name, 64, &s);
    *checksum = s;
    return rc;
}
}
