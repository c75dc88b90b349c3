/* A second translation unit that includes the specification: step_core.h, host_cfg.h, render_core.h, scan_core.h and camera_core.h are
 * headers of inline functions, so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/camera_core.h"

extern "C" unsigned long long camera_sizeof_spec(void) { return sizeof(hrl_camera_spec); }
extern "C" unsigned long long camera_sizeof_out(void) { return sizeof(hrl_camera_out); }
extern "C" const char *camera_validate_spec(const hrl_camera_spec *s) {
    static thread_local std::string why;
    why = hrl::camera::validate_spec(s);
    return why.c_str();
}
