/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long route_sizeof_spec(void);

int main() { return check_main("hrl_route_spec", route_sizeof_spec(), route_check::n_cases(), route_check::run_case); }
