/* Stand-alone program, built with -fsanitize=address,undefined: probes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long probe_sizeof_spec(void);

int main() { return check_main("hrl_probe_spec", probe_sizeof_spec(), probe_check::n_cases(), probe_check::run_case); }
