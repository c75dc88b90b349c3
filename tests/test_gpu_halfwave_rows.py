"""The row build on both half-waves (csrc/step_core.h: phase_build_A_halves; GpuExec::half_swap = v_permlane32_swap_b32) on the MI355X: the cases of
tests/test_emu_halfwave_rows.py at 64 envs, device == fp32 oracle byte for byte -- all nine buffers and the solver-row counter after each of 8
steps; the poses go in through hrl_set_state -- and the device's own contact records must show the classes each case is about.  Cases, classes
and the comparison: tests/halfwave_cases.py."""
import pytest

import halfwave_cases as hc
from backends import Device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_device_equals_the_oracle_and_shows_the_classes(name):
    n = 64
    d = Device(Device.config(hc.CASES[name][0], num_envs=n, seed=5, auto_reset=1, **hc.CASES[name][1]), count_rows=True)
    assert bytes(d.cfg) == bytes(hc.make_cfg(name, n))
    d.reset()
    d.env.record_contacts().fill_(float('nan'))   # every float must be written by the step
    seen = hc.run_side(name, n, d, lambda s: s.env.contacts.cpu().numpy(), lambda s, k: getattr(s, k))
    d.close()
    print(name, sorted(seen))
    assert hc.CASES[name][4] <= seen, (name, 'classes missing', sorted(hc.CASES[name][4] - seen))
