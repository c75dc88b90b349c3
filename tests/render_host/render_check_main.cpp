/* Stand-alone program, built with -fsanitize=address,undefined: renders every case of check_cases.h and prints sizeof(hrl_view) and a
 * checksum per case.  Exit status 0 = every render succeeded and the sanitisers saw nothing. */
#include "check_cases.h"

extern "C" unsigned long long render_sizeof_view(void);

int main() {
    printf("sizeof_hrl_view %llu\n", render_sizeof_view());
    for (int k = 0; k < render_check::n_cases(); ++k) {
        char name[64];
        uint64_t sum = 0;
        if (render_check::run_case(k, name, sizeof name, &sum) != HRL_OK) return 1;
        printf("case %s %016llx\n", name, (unsigned long long)sum);
    }
    return 0;
}
