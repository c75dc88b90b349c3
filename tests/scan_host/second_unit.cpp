/* A second translation unit that includes the specification: step_core.h, host_cfg.h, render_core.h and scan_core.h are headers of
 * inline functions, so two units that include them must link into one library / program. */
#include "../../hrl_pybullet_envs_amd/csrc/scan_core.h"

extern "C" unsigned long long scan_sizeof_spec(void) { return sizeof(hrl_scan_spec); }
extern "C" const char *scan_validate_spec(const hrl_scan_spec *s) {
    static thread_local std::string why;
    why = hrl::scan::validate_spec(s);
    return why.c_str();
}
