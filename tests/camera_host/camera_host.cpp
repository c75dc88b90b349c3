/* csrc/camera_core.h compiled for the host (HRL_EMU): what the device kernel must reproduce bit for bit.  Loaded with ctypes
 * (tests/camera_cases.py). */
#include "../../hrl_pybullet_envs_amd/csrc/camera_core.h"

static thread_local std::string g_why;

extern "C" {
/* hrl_camera on host pointers */
int camera_host(const hrl_config *cfg, const hrl_buffers *bufs, const hrl_camera_spec *spec, const uint8_t *mask, const hrl_camera_out *out) {
    return hrl::camera::camera_host_batch(cfg, bufs, spec, mask, out, g_why);
}
const char *camera_host_last_error(void) { return g_why.c_str(); }
int camera_host_default_spec(const hrl_config *cfg, int32_t frame, hrl_camera_spec *spec) { return hrl::camera::default_spec(cfg, frame, spec); }
/* camera_core.h's shade_rgb on one seg word: 0x00BBGGRR */
unsigned camera_shade_rgb(int seg) { return hrl::camera::shade_rgb(seg); }
}

#include "check_cases.h"
extern "C" {
int camera_check_n_cases(void) { return camera_check::n_cases(); }
/* the checksum of case k of camera_check_main, from this (unsanitised) build; name: at least 64 bytes */
int camera_check_case(int k, char *name, unsigned long long *checksum) {
    uint64_t s = 0;
    const int rc = camera_check::run_case(k, name, 64, &s);
    *checksum = s;
    return rc;
}
}
