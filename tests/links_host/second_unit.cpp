/* A second translation unit that includes the specification: step_core.h, host_cfg.h and links_core.h are headers of inline functions,
 * so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/links_core.h"

extern "C" unsigned long long links_sizeof_spec(void) { return sizeof(hrl_links_spec); }
extern "C" unsigned long long links_sizeof_out(void) { return sizeof(hrl_links_out); }
extern "C" const char *links_validate_spec(const hrl_config *c, const hrl_links_spec *s) {
    static thread_local std::string why;
    why = hrl::links::validate_spec(c, s);
    return why.c_str();
}
