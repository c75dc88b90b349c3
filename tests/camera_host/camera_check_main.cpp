/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h (../check_main.h). */
#include "check_cases.h"
#include "../check_main.h"

extern "C" unsigned long long camera_sizeof_spec(void);

int main() { return check_main("hrl_camera_spec", camera_sizeof_spec(), camera_check::n_cases(), camera_check::run_case); }
