/* The body of the stand-alone programs tests/<name>_host/<name>_check_main.cpp, built with -fsanitize=address,undefined: runs every case
 * of the sensor's check_cases.h and prints the size of its spec record and a checksum per case.  Exit status 0 = every launch succeeded
 * and the sanitisers saw nothing. */
#pragma once
#include <stdint.h>
#include <stdio.h>

inline int check_main(const char *record, unsigned long long size, int n_cases, int (*run_case)(int, char *, size_t, uint64_t *)) {
    printf("sizeof_%s %llu\n", record, size);
    for (int k = 0; k < n_cases; ++k) {
        char name[64];
        uint64_t sum = 0;
        if (run_case(k, name, sizeof name, &sum) != HRL_OK) return 1;
        printf("case %s %016llx\n", name, (unsigned long long)sum);
    }
    return 0;
}
