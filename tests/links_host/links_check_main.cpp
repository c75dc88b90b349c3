/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long links_sizeof_spec(void);

int main() { return check_main("hrl_links_spec", links_sizeof_spec(), links_check::n_cases(), links_check::run_case); }
