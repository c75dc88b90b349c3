"""Build the gfx950 HIP libraries in-tree: hrl_pybullet_envs_amd/libhrl_envs_hip.so (the step, include/hrl_envs.h),
hrl_pybullet_envs_amd/libhrl_render_hip.so (the batched renderer, include/hrl_render.h), hrl_pybullet_envs_amd/libhrl_scan_hip.so
(the batched range scanner, include/hrl_scan.h), hrl_pybullet_envs_amd/libhrl_probe_hip.so (the batched point probes,
include/hrl_probe.h) and hrl_pybullet_envs_amd/libhrl_field_hip.so (the batched navigation field, include/hrl_field.h).

hipcc cross-compiles for gfx950 without a GPU.  Usage: python -m hrl_pybullet_envs_amd.build [--force]
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, 'csrc')
LIB = os.path.join(PKG, 'libhrl_envs_hip.so')
SOURCES = ['hrl_hip.hip', 'step_core.h', 'host_cfg.h']
RENDER_LIB = os.path.join(PKG, 'libhrl_render_hip.so')
RENDER_SOURCES = ['render_hip.hip', 'render_core.h', 'step_core.h', 'host_cfg.h']   # a library of its own: the step library's code object stays what it was
SCAN_LIB = os.path.join(PKG, 'libhrl_scan_hip.so')
SCAN_SOURCES = ['scan_hip.hip', 'scan_core.h', 'render_core.h', 'step_core.h', 'host_cfg.h']   # likewise: it reads the renderer's table, not its library
PROBE_LIB = os.path.join(PKG, 'libhrl_probe_hip.so')
PROBE_SOURCES = ['probe_hip.hip', 'probe_core.h', 'scan_core.h', 'render_core.h', 'step_core.h', 'host_cfg.h']   # likewise: the scanner's intersections through an include
FIELD_LIB = os.path.join(PKG, 'libhrl_field_hip.so')
FIELD_SOURCES = ['field_hip.hip', 'field_core.h'] + PROBE_SOURCES[1:]   # likewise: the probe's table and clearances through an include
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O2', '-std=c++17', '-ffp-contract=off', '-fno-slp-vectorize', '-fPIC', '-shared']


def kernel_source_hash():
    """sha256 over the kernel sources (csrc/step_core.h + csrc/hrl_hip.hip) and the compiler flags: ties a committed counter summary
    (profiles/pmc_summary.json, tools/summarize_profile.py) to the code it was collected from (bench.py: roofline.pmc_stale)."""
    import hashlib
    h = hashlib.sha256()
    for name in ('step_core.h', 'hrl_hip.hip'):
        with open(os.path.join(CSRC, name), 'rb') as f:
            h.update(f.read())
    h.update(' '.join(HIPCC_FLAGS).encode())
    return h.hexdigest()


def _stale(lib=LIB, sources=SOURCES, headers=('hrl_envs.h',)):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, s) for s in sources] + [os.path.join(PKG, '..', 'include', h) for h in headers] + [os.path.abspath(__file__)]  # this file holds the flags
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(lib, source, verbose):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + HIPCC_FLAGS + ['-o', lib, os.path.join(CSRC, source)]
    if verbose:
        cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
        print(' '.join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return lib


def build_render(force=False, verbose=False):
    if not force and not _stale(RENDER_LIB, RENDER_SOURCES, ('hrl_envs.h', 'hrl_render.h')):
        return RENDER_LIB
    return _compile(RENDER_LIB, 'render_hip.hip', verbose)


def build_scan(force=False, verbose=False):
    if not force and not _stale(SCAN_LIB, SCAN_SOURCES, ('hrl_envs.h', 'hrl_render.h', 'hrl_scan.h')):
        return SCAN_LIB
    return _compile(SCAN_LIB, 'scan_hip.hip', verbose)


def build_probe(force=False, verbose=False):
    if not force and not _stale(PROBE_LIB, PROBE_SOURCES, ('hrl_envs.h', 'hrl_render.h', 'hrl_scan.h', 'hrl_probe.h')):
        return PROBE_LIB
    return _compile(PROBE_LIB, 'probe_hip.hip', verbose)


def build_field(force=False, verbose=False):
    if not force and not _stale(FIELD_LIB, FIELD_SOURCES, ('hrl_envs.h', 'hrl_render.h', 'hrl_scan.h', 'hrl_probe.h', 'hrl_field.h')):
        return FIELD_LIB
    return _compile(FIELD_LIB, 'field_hip.hip', verbose)


def build(force=False, verbose=False):
    """The five libraries; returns the step library's path."""
    if force or _stale():
        _compile(LIB, 'hrl_hip.hip', verbose)
    build_render(force, verbose)
    build_scan(force, verbose)
    build_probe(force, verbose)
    build_field(force, verbose)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
    print(RENDER_LIB)
    print(SCAN_LIB)
    print(PROBE_LIB)
    print(FIELD_LIB)
