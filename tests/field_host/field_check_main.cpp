/* Stand-alone program, built with -fsanitize=address,undefined: computes every case of check_cases.h and prints sizeof(hrl_field_spec)
 * and a checksum per case.  Exit status 0 = every launch succeeded and the sanitisers saw nothing. */
#include "check_cases.h"

extern "C" unsigned long long field_sizeof_spec(void);

int main() {
    printf("sizeof_hrl_field_spec %llu\n", field_sizeof_spec());
    for (int k = 0; k < field_check::n_cases(); ++k) {
        char name[64];
        uint64_t sum = 0;
        if (field_check::run_case(k, name, sizeof name, &sum) != HRL_OK) return 1;
        printf("case %s %016llx\n", name, (unsigned long long)sum);
    }
    return 0;
}
