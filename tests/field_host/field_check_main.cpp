/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long field_sizeof_spec(void);

int main() { return check_main("hrl_field_spec", field_sizeof_spec(), field_check::n_cases(), field_check::run_case); }
