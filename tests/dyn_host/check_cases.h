/* The cases of dyn_check_main, shared with libdyn_host.so so that the sanitised program's checksums can be compared with the plain host
 * build's: every kind, from a reset-like state with random joint angles and rates and from hostile ones (NaN, +-inf, 1e20, a denormal and
 * a zero quaternion, in another place of the record per env), under two models (the defaults; no body damping, joint damping 1 and
 * armature 0.01), at batch sizes that leave a group's tail empty, fill it and cross it (5, 16, 17, 37), with 0, 1, 4 and 16 sites on every
 * link in turn, with and without tau and a mask, and each subset of the outputs. */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/dyn_core.h"

namespace dyn_check {

constexpr int N_VARIANTS = 7; /* reset-like, NaN, +inf, -inf, 1e20, denormal, a zero quaternion */
constexpr int N_CASES = 6 * 2 * N_VARIANTS;
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
};

/* FNV-1a over the bytes of the seven outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    const int kind = k / (2 * N_VARIANTS), model = (k / N_VARIANTS) % 2, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_model%d_variant%d", kind, model, variant);
    const int sizes[4] = {5, 16, 17, 37};
    const int n = sizes[k % 4];
    hrl_config cfg;
    if (hrl::default_config(kind, &cfg) != HRL_OK) return HRL_ERR_BAD_ARG;
    cfg.num_envs = n;
    if (model) { cfg.model.linear_damping = 0.f; cfg.model.angular_damping = 0.f; cfg.model.joint_damping = 1.f; cfg.model.joint_armature = 0.01f; }
    std::vector<float> state((size_t)n * HRL_STATE_STRIDE, 0.f);
    std::vector<int32_t> aux((size_t)n * HRL_AUX_STRIDE, 0);
    uint32_t lcg = 13579u + (uint32_t)k;
    auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f) * 2.f - 1.f; }; /* [-1, 1) */
    for (int e = 0; e < n; ++e) {
        float *st = &state[(size_t)e * HRL_STATE_STRIDE];
        st[0] = 7.f * rnd(); st[1] = 7.f * rnd(); st[2] = 0.55f + 0.3f * rnd();
        float qn = 0.f;
        for (int i = 3; i < 7; ++i) { st[i] = rnd(); qn += st[i] * st[i]; }
        qn = 1.f / sqrtf(qn > 1e-6f ? qn : 1.f);
        for (int i = 3; i < 7; ++i) st[i] *= qn;
        for (int i = 7; i < 15; ++i) st[i] = 1.8f * rnd();
        for (int i = 15; i < 29; ++i) st[i] = 5.f * rnd();
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const int places[6] = {0, 2, 4, 9, 16, 24}; /* x, z, a quaternion component, a joint angle, a velocity, a joint rate */
            st[places[e % 6]] = hostile_value(variant);
        }
        if (variant == 6 && e % 2 == 0) st[3] = st[4] = st[5] = st[6] = 0.f;
    }
    hrl_dyn_spec spec;
    if (hrl::dyn::default_spec(&cfg, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int B = hrl::links::n_links(kind), nv = hrl::dyn::nv_of(kind);
    const int counts[4] = {0, 1, 4, HRL_DYN_MAX_SITES};
    spec.n_sites = counts[(k / 4) % 4];
    for (int s = 0; s < spec.n_sites; ++s) {
        spec.site_link[s] = (s + k) % B;
        for (int i = 0; i < 3; ++i) spec.site_local[s][i] = 0.5f * rnd();
    }
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.aux = aux.data();
    const size_t S = (size_t)(spec.n_sites > 0 ? spec.n_sites : 1);
    std::vector<float> mass((size_t)n * nv * nv, -3.f), bias((size_t)n * nv, -3.f), accel((size_t)n * nv, -3.f), jac((size_t)n * S * 3 * nv, -3.f), com((size_t)n * 3, -3.f),
        mom((size_t)n * 6, -3.f), en((size_t)n * 2, -3.f), tau((size_t)n * nv, 0.f);
    for (auto &t : tau) t = 250.f * rnd();
    std::vector<uint8_t> mask(n, 1);
    for (int e = 0; e < n; ++e) mask[e] = (uint8_t)((e + k) % 3 == 0 ? 0 : 1 + e % 2);
    hrl_dyn_out out = {k % 5 == 4 ? nullptr : mass.data(), k % 7 == 6 ? nullptr : bias.data(), k % 5 == 3 ? nullptr : accel.data(), spec.n_sites > 0 && k % 3 != 2 ? jac.data() : nullptr,
                       com.data(), k % 4 == 1 ? nullptr : mom.data(), k % 4 == 2 ? nullptr : en.data()};
    std::string why;
    const int rc = hrl::dyn::dyn_host_batch(&cfg, &b, &spec, k % 3 ? tau.data() : nullptr, k % 2 ? mask.data() : nullptr, &out, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    Fnv f;
    for (std::vector<float> *v : {&mass, &bias, &accel, &jac, &com, &mom, &en}) {
        for (float &x : *v)
            if (x != x) x = __builtin_nanf(""); /* one NaN: which operand's sign and payload a sum of two NaNs keeps is the compiler's choice of operand order */
        f.eat(v->data(), v->size() * 4);
    }
    *checksum = f.h;
    return HRL_OK;
}

}  // namespace dyn_check
