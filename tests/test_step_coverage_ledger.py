"""tests/STEP_COVERAGE.md, the ledger of the branches of csrc/step_core.h that tests/tools/step_coverage.py reports, stays true to the code: every
source text it quotes still stands on the line it names, every scenario it names exists in tests/parity_cases.py (a test it names, in tests/test_emu_parity.py), and every row carries exactly one
verdict.  (Whether the rows are still the lines the tool prints is the tool's own --ledger check: a run takes minutes.)"""
import importlib.util
import os
import re

import parity_cases

HERE = os.path.dirname(os.path.abspath(__file__))
VERDICTS = ('taken by ', 'unreachable from a valid config and any records, because ', 'instrumentation artefact: ')


def tool():
    spec = importlib.util.spec_from_file_location('step_coverage', os.path.join(HERE, 'tools', 'step_coverage.py'))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_ledger_quotes_the_code_as_it_is_and_names_scenarios_that_exist():
    t = tool()
    rows = t.ledger_rows()
    with open(t.CORE) as f:
        src = f.read().split('\n')
    with open(os.path.join(HERE, 'test_emu_parity.py')) as f:
        emu_tests = f.read()
    assert len(rows) >= 20 and len({no for no, _, _ in rows}) == len(rows)   # one row per line
    for no, text, verdict in rows:
        assert text and text in src[no - 1], (no, text)
        assert sum(verdict.startswith(v) for v in VERDICTS) == 1, (no, verdict)
        names = re.findall(r'`(\w+)`', verdict.split(';')[0]) if verdict.startswith('taken by ') else []   # (what follows a `;` is a remark)
        assert names or not verdict.startswith('taken by '), (no, verdict)
        for name in names:   # a scenario of tests/parity_cases.py, or a test of the host executor alone
            assert callable(getattr(parity_cases, name, None)) or (name.startswith('test_') and 'def %s(' % name in emu_tests), (no, name)
