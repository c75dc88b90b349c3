/* The cases of closest_check_main, shared with libclosest_host.so so that the sanitised program's checksums can be compared with the
 * plain host build's: every kind from a reset-like state with tilted torsos and bent legs, robots low enough to touch the ground and
 * near the walls, the box and the items, and from hostile ones (in the position, the height, the quaternion, a joint angle and the
 * items), with every set of classes in turn, masks, a missing items record, and each subset of the outputs. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/closest_core.h"

namespace closest_check {

constexpr int N_ENVS = 5, N_VARIANTS = 6, N_ROUNDS = 4; /* reset-like, NaN, +inf, -inf, 1e20, denormal */
constexpr int N_CASES = 6 * N_ROUNDS * N_VARIANTS;
inline int n_cases() { return N_CASES; }

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

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void eat(const void *p, size_t bytes) {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        for (size_t j = 0; j < bytes; ++j) { h ^= q[j]; h *= 1099511628211ull; }
    }
    /* (a NaN as one word: which NaN an operation yields is not part of the specification) */
    void eat_floats(const float *p, size_t n) {
        for (size_t j = 0; j < n; ++j) {
            uint32_t w = 0x7fc00000u;
            if (p[j] == p[j]) memcpy(&w, &p[j], 4);
            eat(&w, 4);
        }
    }
};

/* FNV-1a over the bytes of the five outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (N_ROUNDS * N_VARIANTS), round = (k / N_VARIANTS) % N_ROUNDS, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_round%d_variant%d", kind, round, variant);
    hrl_config cfg;
    if (hrl::default_config(kind, &cfg) != HRL_OK) return HRL_ERR_BAD_ARG;
    cfg.num_envs = N_ENVS;
    const int stride = hrl::items_stride(&cfg);
    const int B = hrl::links::n_links(kind);
    std::vector<float> state((size_t)N_ENVS * HRL_STATE_STRIDE, 0.f), items((size_t)N_ENVS * stride, 0.f);
    std::vector<int32_t> aux((size_t)N_ENVS * HRL_AUX_STRIDE, 0);
    uint32_t lcg = 24680u + (uint32_t)k;
    auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f) * 2.f - 1.f; }; /* [-1, 1) */
    for (int e = 0; e < N_ENVS; ++e) {
        float *st = &state[(size_t)e * HRL_STATE_STRIDE];
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.45f + 0.4f * rnd();
        const float yaw = 3.f * rnd(), tilt = (round == 3 ? 1.5f : 0.3f) * rnd();
        st[3] = sinf(0.5f * tilt) * cosf(0.5f * yaw); st[4] = sinf(0.5f * tilt) * sinf(0.5f * yaw);
        st[5] = cosf(0.5f * tilt) * sinf(0.5f * yaw); st[6] = cosf(0.5f * tilt) * cosf(0.5f * yaw);
        for (int j = 0; j < 8; ++j) st[7 + j] = 1.2f * rnd();
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        if (round >= 1) { /* an item at the robot, one under a foot's reach, and the robot at the box of the maze kinds */
            items[(size_t)e * stride] = st[0] + 0.3f * rnd(); items[(size_t)e * stride + 1] = st[1] + 0.3f * rnd();
            items[(size_t)e * stride + 2] = st[0] + 0.8f * rnd(); items[(size_t)e * stride + 3] = st[1] + 0.8f * rnd();
        }
        if (round == 2) { st[0] = -2.f + 2.5f * rnd(); st[1] = 2.5f * rnd(); }
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[k % 3] = h;
            if (e == 1) st[2] = h;
            if (e == 2) { items[(size_t)e * stride + 1] = h; st[7 + k % 8] = h; }
            if (e == 3) { items[(size_t)e * stride] = h; st[3 + k % 4] = h; }
        }
    }
    hrl_closest_spec spec;
    if (hrl::closest::default_spec(&cfg, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const uint32_t bits[6] = {HRL_CAMERA_GROUND, HRL_SCAN_WALL, HRL_SCAN_BOX, HRL_SCAN_FOOD, HRL_SCAN_POISON, HRL_CHASE_ROBOT};
    if (k % 3 == 2) { /* a subset: every class bit in turn, and pairs of them */
        spec.classes = bits[k % 6] | bits[(k / 6) % 6];
    }
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = k % 11 == 10 ? nullptr : items.data(); b.aux = aux.data();
    const size_t n = (size_t)N_ENVS * B * HRL_CLOSEST_CLASSES;
    std::vector<float> distance(n, -3.f), on_link(3 * n, -5.f), on_surface(3 * n, -6.f), normal(3 * n, -9.f);
    std::vector<int32_t> which(n, -7);
    std::vector<uint8_t> mask(N_ENVS, 1);
    mask[k % N_ENVS] = (uint8_t)(k % 3 == 0 ? 0 : 2);
    hrl_closest_out out = {k % 5 == 4 ? nullptr : distance.data(), k % 7 == 6 ? nullptr : which.data(), k % 5 == 3 ? nullptr : on_link.data(), k % 5 == 2 ? nullptr : on_surface.data(),
                           k % 5 == 1 ? nullptr : normal.data()};
    std::string why;
    const int rc = hrl::closest::closest_host_batch(&cfg, &b, &spec, k % 2 ? mask.data() : nullptr, &out, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    Fnv f;
    f.eat_floats(distance.data(), n); f.eat(which.data(), n * 4); f.eat_floats(on_link.data(), 3 * n); f.eat_floats(on_surface.data(), 3 * n); f.eat_floats(normal.data(), 3 * n);
    *checksum = f.h;
    return HRL_OK;
}

}  // namespace closest_check
