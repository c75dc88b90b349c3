/* The cases of camera_check_main, shared with libcamera_host.so so that the sanitised program's checksums can be compared with the plain
 * host build's: every kind in both frames, from a reset-like state and from hostile ones (in the state and the items), at image sizes
 * that leave waves idle, that end on a half-full pass and at the maximum, with every set of classes, both eye modes, ranges and fields of
 * view in turn, and each subset of the outputs.  Two more cases hold the spans to the scanner: over a few thousand random rays and
 * shapes the t_in of span_half / span_rect / span_disc equals scan::isect_* bit for bit, and t_in <= t_out wherever a span exists.  (One
 * family of the degenerate draws puts the origin ON a disc's rim to the last bit: t_in = 0 there and t_out = b + sqrtf(h) is a rounding
 * of 0 for a ray that leaves at once, with h = r^2 - e^2 the difference of two equal numbers: its sign is rounding.  Those draws check
 * the equality of t_in alone.) */
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../hrl_pybullet_envs_amd/csrc/camera_core.h"

namespace camera_check {

constexpr int N_ENVS = 4, N_VARIANTS = 7; /* reset-like, NaN, +inf, -inf, 1e20, denormal, aux[3] out of range */
constexpr int N_IMAGES = 6 * 2 * N_VARIANTS, N_SPANS = 2, SPAN_RAYS = 4096;
inline int n_cases() { return N_IMAGES + N_SPANS; }

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

inline bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

/* which = 0: shapes about the origin at ordinary distances; which = 1: degenerate ones (axis-parallel rays, origins on edges and inside) */
inline int run_spans(int which, uint64_t *checksum) {
    using namespace hrl;
    uint32_t lcg = 97531u + (uint32_t)which;
    auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 16777216.f) * 2.f - 1.f; }; /* [-1, 1) */
    Fnv f;
    for (int k = 0; k < SPAN_RAYS; ++k) {
        float ang = 3.2f * rnd();
        if (which == 1 && k % 4 == 0) ang = 1.57079632679f * (float)(k / 4 % 4);
        float dx = cosf(ang), dy = sinf(ang);
        if (which == 1 && k % 8 == 0) { dx = (k / 8) % 2 ? 0.f : 1.f; dy = (k / 8) % 2 ? 1.f : 0.f; }
        const float idx = 1.f / dx, idy = 1.f / dy;
        const float cx = 12.f * rnd(), cy = 12.f * rnd();
        float hx = 0.05f + 3.f * fabsf(rnd()), hy = 0.05f + 3.f * fabsf(rnd());
        if (which == 1 && k % 3 == 0) { hx = fabsf(cx); }              /* the origin on an edge */
        if (which == 1 && k % 5 == 0) { hx = fabsf(cx) + 1.f; hy = fabsf(cy) + 1.f; } /* inside */
        const float r2 = which == 1 && k % 7 == 0 ? fmaf(cx, cx, cy * cy) : hx * hx;
        const float nang = 3.2f * rnd(), nx = which == 1 && k % 2 ? (k % 4 == 1 ? 1.f : 0.f) : cosf(nang), ny = which == 1 && k % 2 ? (k % 4 == 1 ? 0.f : -1.f) : sinf(nang);
        const float off = 9.f * rnd() + 4.f;
        const camera::Span a = camera::span_half(nx, ny, off, dx, dy), b = camera::span_rect(cx, cy, hx, hy, idx, idy), c = camera::span_disc(cx, cy, r2, dx, dy);
        const float ta = scan::isect_half(nx, ny, off, dx, dy), tb = scan::isect_rect(cx, cy, hx, hy, idx, idy), tc = scan::isect_disc(cx, cy, r2, dx, dy);
        if (!same_bits(a.a, ta) || !same_bits(b.a, tb) || !same_bits(c.a, tc)) { fprintf(stderr, "spans%d: ray %d: t_in differs from the scanner's\n", which, k); return HRL_ERR_BAD_ARG; }
        const camera::Span *all[3] = {&a, &b, &c};
        for (int s = 0; s < 3; ++s) {
            const camera::Span &sp = *all[s];
            const bool exists = sp.a < __builtin_inff();
            const bool on_rim = s == 2 && which == 1 && k % 7 == 0;
            if (exists && !on_rim && !(sp.a <= sp.b)) { fprintf(stderr, "spans%d: ray %d shape %d: t_in %g > t_out %g\n", which, k, s, sp.a, sp.b); return HRL_ERR_BAD_ARG; }
            if (exists && (sp.a == 0.f) != (sp.face == HRL_FACE_INSIDE)) return HRL_ERR_BAD_ARG;
            f.eat(&sp.a, 4); f.eat(&sp.b, 4); f.eat(&sp.face, 4);
        }
    }
    *checksum = f.h;
    return HRL_OK;
}

/* FNV-1a over the bytes of the three outputs; returns HRL_OK or the status of the launch */
inline int run_case(int k, char *name, size_t name_len, uint64_t *checksum) {
    if (k >= N_IMAGES) {
        snprintf(name, name_len, "spans%d", k - N_IMAGES);
        return run_spans(k - N_IMAGES, checksum);
    }
    const int kind = k / (2 * N_VARIANTS), frame = (k / N_VARIANTS) % 2, variant = k % N_VARIANTS;
    snprintf(name, name_len, "kind%d_frame%d_variant%d", kind, frame, variant);
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
        st[0] = 4.f * rnd(); st[1] = 6.f * rnd(); st[2] = 0.55f + 0.3f * rnd();
        const float yaw = 3.f * rnd();
        st[5] = sinf(0.5f * yaw); st[6] = cosf(0.5f * yaw);
        for (int i = 0; i < stride; ++i) items[(size_t)e * stride + i] = 6.f * rnd();
        aux[(size_t)e * HRL_AUX_STRIDE + 3] = e % 4;
        if (variant >= 1 && variant <= 5) { /* hostile floats, in another place per env */
            const float h = hostile_value(variant);
            if (e == 0) st[0] = h;
            if (e == 1) st[2] = h;
            if (e == 2) items[(size_t)e * stride + 1] = h;
            if (e == 3) { items[(size_t)e * stride] = h; st[6] = h; }
        }
        if (variant == 6) aux[(size_t)e * HRL_AUX_STRIDE + 3] = e == 0 ? 1000 : (e == 1 ? -5 : (e == 2 ? 0x7fffffff : (int32_t)0x80000000));
    }
    hrl_camera_spec spec;
    if (hrl::camera::default_spec(&cfg, frame, &spec) != HRL_OK) return HRL_ERR_BAD_ARG;
    const int sizes[4][2] = {{128, 128}, {16, 8}, {48, 24}, {64, 40}};
    spec.width = sizes[variant % 4][0]; spec.height = sizes[variant % 4][1];
    spec.classes = (uint32_t)(k % 127) + 1u; /* 1..127: every bit of HRL_SCAN_ALL | HRL_CAMERA_GROUND in turn */
    spec.classes = (spec.classes & 31u) | ((spec.classes & 32u) << 1) | (spec.classes & 64u);
    spec.eye_mode = k % 2;
    spec.eye_height = 0.1f + 0.7f * (float)(k % 4);
    if (k % 3 == 1) spec.max_range = 4.f;
    if (k % 4 >= 2) { spec.tan_half_h = k % 4 == 2 ? 0.4f : 2.5f; spec.tan_half_v = 0.6f; }
    hrl_buffers b;
    memset(&b, 0, sizeof b);
    b.struct_size = sizeof b; b.state = state.data(); b.items = k % 11 == 10 ? nullptr : items.data(); b.aux = aux.data();
    const size_t pixels = (size_t)spec.width * spec.height;
    std::vector<float> depth(N_ENVS * pixels, -3.f);
    std::vector<int32_t> seg(N_ENVS * pixels, -7);
    std::vector<uint8_t> rgb(N_ENVS * pixels * 3, 0x7B), mask(N_ENVS, 1);
    mask[k % N_ENVS] = (uint8_t)(k % 3 == 0 ? 0 : 2);
    hrl_camera_out out = {k % 5 == 4 ? nullptr : depth.data(), k % 7 == 6 ? nullptr : seg.data(), k % 5 == 3 ? nullptr : rgb.data()};
    std::string why;
    const int rc = hrl::camera::camera_host_batch(&cfg, &b, &spec, k % 2 ? mask.data() : nullptr, &out, why);
    if (rc != HRL_OK) { fprintf(stderr, "%s: %s\n", name, why.c_str()); return rc; }
    Fnv f;
    f.eat(depth.data(), depth.size() * 4); f.eat(seg.data(), seg.size() * 4); f.eat(rgb.data(), rgb.size());
    *checksum = f.h;
    return HRL_OK;
}

}  // namespace camera_check
