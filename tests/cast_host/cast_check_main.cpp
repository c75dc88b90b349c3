/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long cast_sizeof_spec(void);

int main() { return check_main("hrl_cast_spec", cast_sizeof_spec(), cast_check::n_cases(), cast_check::run_case); }
