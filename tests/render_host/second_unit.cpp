/* A second translation unit that includes the specification: step_core.h, host_cfg.h and render_core.h are headers of inline
 * functions, so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/render_core.h"

extern "C" unsigned long long render_sizeof_view(void) { return sizeof(hrl_view); }
extern "C" const char *render_validate_view(const hrl_view *v) {
    static thread_local std::string why;
    why = hrl::render::validate_view(v);
    return why.c_str();
}
