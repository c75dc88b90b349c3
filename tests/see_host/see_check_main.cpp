/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long see_sizeof_spec(void);

int main() { return check_main("hrl_see_spec", see_sizeof_spec(), see_check::n_cases(), see_check::run_case); }
