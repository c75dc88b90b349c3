/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long dyn_sizeof_spec(void);

int main() { return check_main("hrl_dyn_spec", dyn_sizeof_spec(), dyn_check::n_cases(), dyn_check::run_case); }
