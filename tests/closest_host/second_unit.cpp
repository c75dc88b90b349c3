/* A second translation unit that includes the specification: step_core.h, host_cfg.h, links_core.h and closest_core.h are headers of
 * inline functions, so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/closest_core.h"

extern "C" unsigned long long closest_sizeof_spec(void) { return sizeof(hrl_closest_spec); }
extern "C" unsigned long long closest_sizeof_out(void) { return sizeof(hrl_closest_out); }
extern "C" const char *closest_validate_spec(const hrl_closest_spec *s) {
    static thread_local std::string why;
    why = hrl::closest::validate_spec(s);
    return why.c_str();
}
