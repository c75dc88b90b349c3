/* A second translation unit that includes the specification: step_core.h, host_cfg.h, render_core.h, scan_core.h, camera_core.h,
 * links_core.h and chase_core.h are headers of inline functions, so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/chase_core.h"

extern "C" unsigned long long chase_sizeof_spec(void) { return sizeof(hrl_chase_spec); }
extern "C" unsigned long long chase_sizeof_out(void) { return sizeof(hrl_chase_out); }
extern "C" const char *chase_validate_spec(const hrl_chase_spec *s) {
    static thread_local std::string why;
    why = hrl::chase::validate_spec(s);
    return why.c_str();
}
