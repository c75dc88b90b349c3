/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long frontier_sizeof_spec(void);

int main() { return check_main("hrl_frontier_spec", frontier_sizeof_spec(), frontier_check::n_cases(), frontier_check::run_case); }
