/* Stand-alone program, built with -fsanitize=address,undefined: probes every case of check_cases.h and prints sizeof(hrl_probe_spec)
 * and a checksum per case.  Exit status 0 = every launch succeeded and the sanitisers saw nothing. */
#include "check_cases.h"

extern "C" unsigned long long probe_sizeof_spec(void);

int main() {
    printf("sizeof_hrl_probe_spec %llu\n", probe_sizeof_spec());
    for (int k = 0; k < probe_check::n_cases(); ++k) {
        char name[64];
        uint64_t sum = 0;
        if (probe_check::run_case(k, name, sizeof name, &sum) != HRL_OK) return 1;
        printf("case %s %016llx\n", name, (unsigned long long)sum);
    }
    return 0;
}
