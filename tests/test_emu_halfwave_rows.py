"""The row build on both half-waves (csrc/step_core.h: mirror rows in phase_build_row, phase_build_A_halves, half_swap) on the lock-step host
executor: emulator == fp32 oracle byte for byte -- all nine buffers and the solver-row counter after each of 8 steps -- on poses that show every
class of substep in front of that build: no rows, one to four limit rows alone, bounded and friction blocks just under / on / just over a
multiple of four columns, the standing ant's 20 rows, exactly 32, more than 32 (the fallback) and a self contact (the fallback).  Cases, classes
and the comparison: tests/halfwave_cases.py.  Both lane orders: the exchange between the half-waves must not depend on the order of the lanes."""
import pytest

import contacts_cases as cc
import halfwave_cases as hc


class EmuSide(cc.EmuContactsEnv):
    def set(self, qpos, qvel):   # what hrl_set_state does to the record
        self.state[:, 0:15] = qpos; self.state[:, 15:29] = qvel


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_emulator_equals_the_oracle_and_shows_the_classes(name, reverse):
    n = hc.CPU_ENVS[name]
    assert n <= 16 and hc.STEPS >= 8
    e = EmuSide(hc.make_cfg(name, n), reverse=reverse)
    e.reset()
    seen = hc.run_side(name, n, e, lambda s: s.contacts.copy(), lambda s, k: getattr(s, k).copy())
    print(name, sorted(seen))
    assert hc.CASES[name][4] <= seen, (name, 'classes missing', sorted(hc.CASES[name][4] - seen))


def test_the_classes_are_what_the_counts_say():
    """classes_of on hand-made counts: which build a substep takes and which class it is counted in"""
    assert hc.classes_of(0, 0, False) == {'rows0'} and hc.classes_of(3, 0, False) == {'bounded_1_4_alone'} and hc.classes_of(5, 0, False) == set()
    assert hc.classes_of(8, 4, False) == {'nB_on', 'nF_on', 'standing20'}
    assert hc.classes_of(2, 1, False) == {'nB_under', 'nF_under'} and hc.classes_of(2, 3, False) == {'nB_over', 'nF_under', 'nF_over'}
    assert hc.classes_of(8, 8, False) == {'nB_on', 'nF_on', 'rows32'} and hc.classes_of(5, 9, False) == {'nF_under', 'nF_over', 'rows32'}
    assert hc.classes_of(8, 9, False) == {'rows33plus'} and hc.classes_of(8, 4, True) == {'self'}
