/* The cases of frontier_check_main, shared with libfrontier_host.so so that the sanitised program's checksums can be compared with the
 * plain host build's: every kind, from a reset-like state and from hostile ones (in the state and the items), at grid sizes that are no
 * multiple of 256 cells and at the maximum, with both meanings of `unknown`, every source set, blocking set and schedule in turn, and
 * memories that are empty, full, or hold arbitrary bytes in some cells. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/frontier_core.h"

namespace frontier_check {

constexpr int N_ENVS = 4, N_VARIANTS = 7, N_MEMORIES = 3; /* reset-like, NaN, +inf, -inf, 1e20, denormal, aux[3] out of range */
inline int n_cases() { return 6 * N_MEMORIES * N_VARIANTS; }

inline float hostile_value(int variant) {
    switch (variant) {
        case 1: return __builtin_nanf("");
        case 2: return __builtin_inff();
        case 3: return -__builtin_inff();
        case 4: return 1e20f;
        case 5: return 1e-41f;
        default: return 0.f;
    }
}

/* FNV-1a over the bytes of the seven outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (N_MEMORIES * N_VARIANTS), memory = (k / N_VARIANTS) % N_MEMORIES, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_memory%d_variant%d", kind, memory, variant);
    hrl_config cfg;
    if (hrl::default_config(kind, &cfg) != HRL_OK) return HRL_ERR_BAD_ARG;
    cfg.num_envs = N_ENVS;
    const int stride = hrl::items_stride(&cfg);
    std::vector<float> state((size_t)N_ENVS * HRL_STATE_STRIDE, 0.f), items((size_t)N_ENVS * stride, 0.f);
    std::vector<int32_t> aux((size_t)N_ENVS * HRL_AUX_STRIDE, 0);
    uint32_t lcg = 13579u + (uint32_t)k;
    auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f) * 2.f - 1.f; }; /* [-1, 1) */
    for (int e = 0; e < N_ENVS; ++e) {
        float *st = &state[(size_t)e * HRL_STATE_STRIDE];
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.55f;
        const float yaw = 3.f * rnd();
        st[5] = sinf(0.5f * yaw); st[6] = cosf(0.5f * yaw);
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        aux[(size_t)e * HRL_AUX_STRIDE + 3] = e % 4;
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[0] = h;
            if (e == 1) st[6] = h;
            if (e == 2) items[(size_t)e * stride + 1] = h;
            if (e == 3) { items[(size_t)e * stride] = h; st[1] = h; }
        }
        if (variant == 6) aux[(size_t)e * HRL_AUX_STRIDE + 3] = e == 0 ? 1000 : (e == 1 ? -5 : (e == 2 ? 0x7fffffff : (int32_t)0x80000000));
    }
    hrl_frontier_spec spec;
    if (hrl::frontier::default_spec(&cfg, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{64, 64}, {8, 8}, {24, 40}, {64, 8}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.blocking = 1u + (uint32_t)(k % 31);
    spec.sources = (1u + (uint32_t)(k % 31)) << 2; /* every non-empty set of FOOD (4) .. EDGE (64) */
    spec.unknown = k % 2;
    spec.margin = 0.2f * (float)(k % 3);
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = items.data(); b.aux = aux.data();
    const size_t cells = (size_t)spec.width * spec.height;
    std::vector<uint8_t> seen(N_ENVS * cells), edge(N_ENVS * cells, 0x7B), parent(N_ENVS * cells, 0x7B);
    std::vector<float> dist(N_ENVS * cells, -7.f), length(N_ENVS, -7.f), goal(2 * N_ENVS, -7.f);
    std::vector<int32_t> count(N_ENVS, -7), cell(N_ENVS, -7);
    for (size_t i = 0; i < seen.size(); ++i) {
        const size_t in_env = i % cells, row = in_env / spec.width, col = in_env % spec.width;
        seen[i] = memory == 0 ? (uint8_t)((i * 7u + (uint32_t)k) % 3u == 0u ? 0u : 1u + (i & 0xfeu))       /* arbitrary bytes in two thirds of the cells */
                              : (memory == 1 ? (uint8_t)(row + col + (size_t)k < (size_t)(spec.width + spec.height) / 2 ? 1 : 0) /* a corner */
                                             : (uint8_t)(k % 4 == 0 ? 0 : 1));                            /* empty or full */
    }
    hrl_frontier_out out = {k % 5 == 4 ? nullptr : edge.data(), dist.data(), k % 7 == 6 ? nullptr : parent.data(), count.data(), length.data(), goal.data(), cell.data()};
    std::string why;
    const int rc = hrl::frontier::frontier_host_batch(&cfg, &b, &spec, seen.data(), nullptr, &out, k % 3, nullptr, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    uint64_t h = 1469598103934665603ull;
    auto eat = [&h](const void *p, size_t bytes) {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (size_t j = 0; j < bytes; ++j) { h ^= q[j]; h *= 1099511628211ull; }
    };
    eat(edge.data(), edge.size()); eat(dist.data(), dist.size() * 4); eat(parent.data(), parent.size()); eat(count.data(), count.size() * 4);
    eat(length.data(), length.size() * 4); eat(goal.data(), goal.size() * 4); eat(cell.data(), cell.size() * 4);
    *checksum = h;
    return HRL_OK;
}

}  // namespace frontier_check
