/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long chase_sizeof_spec(void);

int main() { return check_main("hrl_chase_spec", chase_sizeof_spec(), chase_check::n_cases(), chase_check::run_case); }
