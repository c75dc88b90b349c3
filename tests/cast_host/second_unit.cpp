/* A second translation unit that includes the specification: step_core.h, host_cfg.h, render_core.h, scan_core.h, camera_core.h,
 * links_core.h, chase_core.h and cast_core.h are headers of inline functions, so two units that include them must link into one library /
 * program. */
#include "../../hrl_pybullet_envs_amd/csrc/cast_core.h"

extern "C" unsigned long long cast_sizeof_spec(void) { return sizeof(hrl_cast_spec); }
extern "C" unsigned long long cast_sizeof_out(void) { return sizeof(hrl_cast_out); }
extern "C" const char *cast_validate_spec(const hrl_cast_spec *s) {
    static thread_local std::string why;
    why = hrl::cast::validate_spec(s);
    return why.c_str();
}
