/* Stand-alone program, built with -fsanitize=address,undefined: scans every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long scan_sizeof_spec(void);

int main() { return check_main("hrl_scan_spec", scan_sizeof_spec(), scan_check::n_cases(), scan_check::run_case); }
