/*
 * emu_contacts.cpp -- TEST INFRASTRUCTURE: the lock-step host executor (emu_lib.cpp) with the step's optional contact report switched on.
 *
 * emu_step() hands the phases a DevBufs without the `contacts` pointer (the report is off, as for every caller that does not ask for it);
 * emu_step_contacts() is the same launch with the pointer set, so that the report phase of csrc/step_core.h (write_contacts) runs lane by lane
 * on the CPU and its records can be compared with the oracle's last substep -- and, on an MI355X, with the kernel's bytes.
 * Built by tests/contacts_cases.py into libhrl_emu_contacts.so with the flags of the Makefile next to it.
 */
#include "emu_lib.cpp"

extern "C" int emu_step_contacts(const hrl_config *cfg, const hrl_buffers *b, int reverse) {
    if (!validate(cfg).empty()) return HRL_ERR_BAD_ARG;
    DevCfg c; build_devcfg(*cfg, c);
    DevBufs d = to_dev(b, nullptr);
    d.contacts = b->struct_size >= sizeof(hrl_buffers_ext) ? reinterpret_cast<const hrl_buffers_ext *>(b)->contacts : nullptr;
    if (cfg->env_kind == HRL_POINT_GATHER) {
        for (int e = 0; e < cfg->num_envs; ++e) { CpuGroup g(1); CpuExec x(g, 0); x.reverse = reverse != 0; step_dispatch(x, d, c, e); }
        return HRL_OK;
    }
    const int n_groups = (cfg->num_envs + 3) / 4;
    std::vector<CpuGroup *> groups;
    for (int k = 0; k < n_groups; ++k) groups.push_back(new CpuGroup(4));
    std::vector<std::thread> team;
    for (int w = 0; w < 4; ++w)
        team.emplace_back([&, w]() {
            for (int k = 0; k < n_groups; ++k) { CpuExec x(*groups[k], w); x.reverse = reverse != 0; step_dispatch(x, d, c, 4 * k + w); }
        });
    for (auto &t : team) t.join();
    for (auto *g : groups) delete g;
    return HRL_OK;
}
