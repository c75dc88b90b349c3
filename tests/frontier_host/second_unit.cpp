/* A second translation unit that includes the specification: step_core.h, host_cfg.h, render_core.h, scan_core.h, probe_core.h,
 * field_core.h, route_core.h and frontier_core.h are headers of inline functions, so two units that include them must link into one
 * library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/frontier_core.h"

extern "C" unsigned long long frontier_sizeof_spec(void) { return sizeof(hrl_frontier_spec); }
extern "C" unsigned long long frontier_sizeof_out(void) { return sizeof(hrl_frontier_out); }
extern "C" const char *frontier_validate_spec(const hrl_frontier_spec *s) {
    static thread_local std::string why;
    why = hrl::frontier::validate_spec(s);
    return why.c_str();
}
