/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long closest_sizeof_spec(void);

int main() { return check_main("hrl_closest_spec", closest_sizeof_spec(), closest_check::n_cases(), closest_check::run_case); }
