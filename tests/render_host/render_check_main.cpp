/* Stand-alone program, built with -fsanitize=address,undefined: renders every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long render_sizeof_view(void);

int main() { return check_main("hrl_view", render_sizeof_view(), render_check::n_cases(), render_check::run_case); }
