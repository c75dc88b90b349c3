#!/usr/bin/env python3
"""Which branches of csrc/step_core.h does no CPU test take?  A tool, not a test: a run takes minutes.

Builds the --coverage targets of tests/emu/Makefile (libhrl_emu_cov.so, libhrl_emu_contacts_cov.so: -O1 -g --coverage, otherwise the flags of
libhrl_emu.so) into a temporary directory, runs every CPU test file that drives the host executor with HRL_EMU_COVERAGE pointing there
(tests/emu_env.py and tests/contacts_cases.py then load those builds), runs `gcov -b -c` on both, sums every branch over all template instances
and over both libraries, and prints the source lines of step_core.h that still have a branch no test took, with their text.  tests/STEP_COVERAGE.md
holds one row per printed line.

    python tests/tools/step_coverage.py [--jobs J] [--only FILE ...] [--keep DIR [--report-only]] [--ledger]

The test files are those under tests/ that reach `emu_env` or `backends` through their imports, without the GPU files (every test of theirs
needs the device) and without test_emu_asan.py (it runs only with the whole suite) and the ledger's own test (it runs no step).  --only restricts the run to the named files (the figures of
a subset are comparable only with figures of the same subset).  --ledger also checks the printed lines against tests/STEP_COVERAGE.md.

What the figures are not: they measure the HOST build at -O1, where gcc folds and splits conditions (a line can be reported for a branch the source
does not have, or hide one it has), and they say nothing of what the device does in a branch -- only that no test could have compared it."""
import argparse
import collections
import concurrent.futures
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = os.path.join(ROOT, 'tests')
CORE = os.path.join(ROOT, 'hrl_pybullet_envs_amd', 'csrc', 'step_core.h')
LEDGER = os.path.join(TESTS, 'STEP_COVERAGE.md')
SEEDS = ('emu_env', 'backends')
LEFT_OUT = ('test_emu_asan.py', 'test_step_coverage_ledger.py')   # the second reaches `backends` through parity_cases and runs no step


def emulator_test_files():
    """test_*.py under tests/ whose imports (through the shared *_cases / replay / tool modules) reach emu_env or backends"""
    mods = {}
    for p in glob.glob(os.path.join(TESTS, '*.py')) + glob.glob(os.path.join(TESTS, 'tools', '*.py')):
        with open(p) as f:
            text = f.read()
        mods[os.path.splitext(os.path.basename(p))[0]] = (p, set(re.findall(r'^\s*(?:import|from)\s+([A-Za-z_]\w*)', text, re.M)) |
                                                           set(re.findall(r"'(fuzz_\w+)'", text)))
    reach = set(SEEDS)
    while True:
        more = {m for m, (_, imp) in mods.items() if m not in reach and imp & reach}
        if not more:
            break
        reach |= more
    files = sorted(os.path.basename(mods[m][0]) for m in reach if m.startswith('test_') and os.path.dirname(mods[m][0]) == TESTS)
    return [f for f in files if not f.startswith('test_gpu_') and f not in LEFT_OUT]


def run_file(name, env):
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'not gpu', '-p', 'no:cacheprovider', os.path.join(TESTS, name)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = [ln for ln in r.stdout.strip().splitlines() if ln.strip()][-1:] or ['']
    return name, r.returncode, tail[0], r.stdout


def gcov_json(cov, stem):
    """`gcov -b -c` of one object file, as JSON: the records of step_core.h"""
    if not os.path.exists(os.path.join(cov, stem + '.gcda')):
        return None
    out = subprocess.run(['gcov', '-b', '-c', '--json-format', '--stdout', '-o', cov, os.path.join(cov, stem + '.gcno')],
                         cwd=cov, stdout=subprocess.PIPE, check=True).stdout
    for doc in out.decode().splitlines():
        if not doc.strip():
            continue
        for f in json.loads(doc)['files']:
            if os.path.basename(f['file']) == 'step_core.h':
                return f
    return None


def instances(funcs, line):
    """how many functions hold `line` as instances of one piece of source: the functions of the smallest line range around it (the six KINDs of a
    template, of a lambda inside it) -- gcov lists their branches on the line one instance after the other"""
    cover = [(f['end_line'] - f['start_line'], f['start_line']) for f in funcs if f['start_line'] <= line <= f['end_line']]
    return cover.count(min(cover)) if cover else 1


def summed(records):
    """line -> {number of branches: [executions, [branch counts]]} summed over template instances and libraries.  gcov gives one record per
    line with the branches of all instances in a row: where their number divides by the number of instances the record is folded, branch by
    branch; where it does not (gcc gave the instances different layouts) it stays as it is.  Records of the two libraries are summed where they
    have the same layout, else kept side by side, and the line counts as having a never-taken branch if some layout that was executed has one.
    Exception edges (`throw`) are not branches of the source."""
    by_line = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, None]))
    for rec in records:
        funcs = rec.get('functions', [])
        for ln in rec['lines']:
            br = [b['count'] for b in ln.get('branches', []) if not b.get('throw')]
            n = instances(funcs, ln['line_number']) if br else 1
            if n > 1 and len(br) % n == 0:
                k = len(br) // n
                br = [sum(br[i * k + j] for i in range(n)) for j in range(k)]
            slot = by_line[ln['line_number']][len(br)]
            slot[0] += ln['count']
            slot[1] = br if slot[1] is None else [a + b for a, b in zip(slot[1], br)]
    return by_line


def figures(by_line):
    n_lines = n_exec = n_br = n_taken = 0
    never = []
    for no in sorted(by_line):
        layouts = by_line[no]
        n_lines += 1
        n_exec += int(any(c for c, _ in layouts.values()))
        hit = False
        for k, (count, br) in layouts.items():
            n_br += k; n_taken += sum(1 for b in br if b)
            if k and count and not all(br):
                hit = True
        if hit:
            never.append(no)
    return n_lines, n_exec, n_br, n_taken, never


def ledger_rows():
    """tests/STEP_COVERAGE.md: the table rows `| line | `source text` | verdict |` -> [(line, text, verdict)]"""
    rows = []
    with open(LEDGER) as f:
        for ln in f:
            m = re.match(r'^\|\s*(\d+)\s*\|\s*`(.*?)`\s*\|\s*(.*?)\s*\|\s*$', ln)
            if m:
                rows.append((int(m.group(1)), m.group(2).replace('\\|', '|'), m.group(3)))   # (a `|` of the code is written \| inside the table)
    return rows


def run_tests(cov, files, jobs):
    """the coverage builds into `cov`, then the test files against them, `jobs` at once (the counts of processes that end together are merged under
    a file lock); -> the number of files with a failure"""
    emu = os.path.join(TESTS, 'emu')
    subprocess.check_call(['make', '-s', '-C', emu, 'COVDIR=' + cov, os.path.join(cov, 'libhrl_emu_cov.so'), os.path.join(cov, 'libhrl_emu_contacts_cov.so')])
    # what the tests build on first use, once, before several of them start at the same time
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle'), 'liborc.so', 'libtextbook.so'])
    subprocess.check_call(['make', '-s', '-C', emu, 'libhrl_emu.so'])
    env = dict(os.environ, HRL_EMU_COVERAGE=cov)
    print('%d test files, %d at once' % (len(files), jobs), flush=True)
    failed = 0
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for name, rc, tail, out in pool.map(lambda f: run_file(f, env), files):
            print('  %-40s %s' % (name, tail), flush=True)
            if rc not in (0, 5):   # 5: nothing but GPU tests in the file
                failed += 1
                print(out)
    return failed


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1), help='test files run at once')
    ap.add_argument('--only', nargs='+', help='run these test files only')
    ap.add_argument('--keep', help='build and count in this directory and keep it (default: a temporary one)')
    ap.add_argument('--report-only', action='store_true', help='with --keep DIR: no build, no tests, the report of the counts DIR already holds')
    ap.add_argument('--ledger', action='store_true', help='compare the printed lines with tests/STEP_COVERAGE.md')
    a = ap.parse_args()
    files = a.only or emulator_test_files()
    tmp = None
    if a.keep:
        os.makedirs(a.keep, exist_ok=True); cov = os.path.abspath(a.keep)
    else:
        tmp = tempfile.TemporaryDirectory(prefix='step_cov_'); cov = tmp.name
    failed = 0
    if not (a.report_only and a.keep):
        failed = run_tests(cov, files, a.jobs)
    records = [r for r in (gcov_json(cov, 'emu_lib_cov'), gcov_json(cov, 'emu_contacts_cov')) if r]
    assert records, 'no counts were written'
    n_lines, n_exec, n_br, n_taken, never = figures(summed(records))
    with open(CORE) as f:
        src = f.read().split('\n')
    print('step_core.h: lines executed %.2f %% of %d, branches taken at least once %.2f %% of %d, lines with a never-taken branch: %d'
          % (100.0 * n_exec / n_lines, n_lines, 100.0 * n_taken / max(n_br, 1), n_br, len(never)))
    for no in never:
        print('%5d: %s' % (no, src[no - 1].strip()))
    rc = 1 if failed else 0
    if a.ledger:
        rows = {no: text for no, text, _ in ledger_rows()}
        missing = [no for no in never if no not in rows]
        stale = [no for no in never if no in rows and rows[no] not in src[no - 1]]
        print('without a ledger row: %s; rows whose text is not on that line any more: %s' % (missing, stale))
        rc = rc or (1 if missing or stale else 0)
    if tmp:
        tmp.cleanup()
    return rc


if __name__ == '__main__':
    sys.exit(main())
