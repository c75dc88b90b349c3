"""Build the gfx950 HIP libraries in-tree: hrl_pybullet_envs_amd/libhrl_envs_hip.so (the step, include/hrl_envs.h),
hrl_pybullet_envs_amd/libhrl_render_hip.so (the batched renderer, include/hrl_render.h), hrl_pybullet_envs_amd/libhrl_scan_hip.so
(the batched range scanner, include/hrl_scan.h), hrl_pybullet_envs_amd/libhrl_probe_hip.so (the batched point probes,
include/hrl_probe.h), hrl_pybullet_envs_amd/libhrl_field_hip.so (the batched navigation field, include/hrl_field.h),
hrl_pybullet_envs_amd/libhrl_route_hip.so (the batched routes, include/hrl_route.h), hrl_pybullet_envs_amd/libhrl_see_hip.so (the
batched visibility map, include/hrl_see.h), hrl_pybullet_envs_amd/libhrl_frontier_hip.so (the batched frontier map, include/hrl_frontier.h),
hrl_pybullet_envs_amd/libhrl_camera_hip.so (the batched first-person camera, include/hrl_camera.h),
hrl_pybullet_envs_amd/libhrl_links_hip.so (the batched link states, include/hrl_links.h), hrl_pybullet_envs_amd/libhrl_chase_hip.so
(the batched chase camera, include/hrl_chase.h), hrl_pybullet_envs_amd/libhrl_dyn_hip.so (the batched dynamics terms,
include/hrl_dyn.h), hrl_pybullet_envs_amd/libhrl_cast_hip.so (the batched ray test, include/hrl_cast.h) and
hrl_pybullet_envs_amd/libhrl_closest_hip.so (the batched closest points, include/hrl_closest.h): fourteen libraries.

hipcc cross-compiles for gfx950 without a GPU.  Usage: python -m hrl_pybullet_envs_amd.build [--force]
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, 'csrc')
LIB = os.path.join(PKG, 'libhrl_envs_hip.so')
SOURCES = ['hrl_hip.hip', 'step_core.h', 'host_cfg.h']
# The sensor libraries in build order: (name, library, source, specification, public header).  Each is a library of its own -- the step
# library's code object stays what it was -- and reads its predecessor's table through an include, not its library: what a sensor depends
# on is its own three files plus everything its predecessor depends on.  csrc/sensor_launch.h is the host side of all four.
SENSORS = [('render', 'libhrl_render_hip.so', 'render_hip.hip', 'render_core.h', 'hrl_render.h'),
           ('scan', 'libhrl_scan_hip.so', 'scan_hip.hip', 'scan_core.h', 'hrl_scan.h'),
           ('probe', 'libhrl_probe_hip.so', 'probe_hip.hip', 'probe_core.h', 'hrl_probe.h'),
           ('field', 'libhrl_field_hip.so', 'field_hip.hip', 'field_core.h', 'hrl_field.h')]
# The routes stand on the field's whole chain and are an entry of their own, in the table's form: SENSORS stays the four sensors.
ROUTE = ('route', 'libhrl_route_hip.so', 'route_hip.hip', 'route_core.h', 'hrl_route.h')
# The visibility map stands on the field's whole chain too (not on the routes), likewise as an entry of its own.
SEE = ('see', 'libhrl_see_hip.so', 'see_hip.hip', 'see_core.h', 'hrl_see.h')
# The frontier map stands on the field's chain and on the routes' specification (the test that names a point's cell, the cell-to-world function).
FRONTIER = ('frontier', 'libhrl_frontier_hip.so', 'frontier_hip.hip', 'frontier_core.h', 'hrl_frontier.h')
# The first-person camera stands on the scanner's chain alone (render, scan): the scanner's table plus a z-interval per slot.
CAMERA = ('camera', 'libhrl_camera_hip.so', 'camera_hip.hip', 'camera_core.h', 'hrl_camera.h')
# The link states stand on no other sensor: the step's own kinematics (step_core.h, included) restated in a specification of their own.
LINKS = ('links', 'libhrl_links_hip.so', 'links_hip.hip', 'links_core.h', 'hrl_links.h')
# The chase camera stands on the first-person camera's chain (render, scan, camera) and on the link states' specification.
CHASE = ('chase', 'libhrl_chase_hip.so', 'chase_hip.hip', 'chase_core.h', 'hrl_chase.h')
# The dynamics terms stand on the link states' specification (the sites) and, like it, on the step's own model (step_core.h, included).
DYN = ('dyn', 'libhrl_dyn_hip.so', 'dyn_hip.hip', 'dyn_core.h', 'hrl_dyn.h')
# The ray test stands on the chase camera's whole chain (render, scan, camera, links, chase): its solids and their intersections.
CAST = ('cast', 'libhrl_cast_hip.so', 'cast_hip.hip', 'cast_core.h', 'hrl_cast.h')
# The closest points stand on the link states' specification and on the step's own narrow phase (step_core.h, included); of the chase
# camera's chain they read the headers alone (the class bits and the hit codes).
CLOSEST = ('closest', 'libhrl_closest_hip.so', 'closest_hip.hip', 'closest_core.h', 'hrl_closest.h')
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


def build_sensor(name, force=False, verbose=False):
    """Sensor library `name` of SENSORS; returns its path."""
    upto = [n for n, *_ in SENSORS].index(name) + 1
    lib, source = os.path.join(PKG, SENSORS[upto - 1][1]), SENSORS[upto - 1][2]
    sources = [source, 'sensor_launch.h'] + [core for *_, core, _ in SENSORS[:upto]] + SOURCES[1:]
    if force or _stale(lib, sources, ['hrl_envs.h'] + [header for *_, header in SENSORS[:upto]]):
        _compile(lib, source, verbose)
    return lib


def build_render(force=False, verbose=False):
    return build_sensor('render', force, verbose)


def build_scan(force=False, verbose=False):
    return build_sensor('scan', force, verbose)


def build_probe(force=False, verbose=False):
    return build_sensor('probe', force, verbose)


def build_field(force=False, verbose=False):
    return build_sensor('field', force, verbose)


def _build_on_the_field(entry, force, verbose, more_sources=(), more_headers=()):
    _, lib, source, core, header = entry
    lib = os.path.join(PKG, lib)
    sources = [source, core, 'sensor_launch.h'] + list(more_sources) + [c for *_, c, _ in SENSORS] + SOURCES[1:]
    if force or _stale(lib, sources, ['hrl_envs.h', header] + list(more_headers) + [h for *_, h in SENSORS]):
        _compile(lib, source, verbose)
    return lib


def build_route(force=False, verbose=False):
    """The route library; returns its path.  It depends on everything the field depends on plus its own three files."""
    return _build_on_the_field(ROUTE, force, verbose)


def build_see(force=False, verbose=False):
    """The visibility map's library; returns its path.  It depends on everything the field depends on plus its own three files."""
    return _build_on_the_field(SEE, force, verbose)


def build_frontier(force=False, verbose=False):
    """The frontier map's library; returns its path.  It depends on everything the field depends on, on the routes' specification and
    header, and on its own three files."""
    return _build_on_the_field(FRONTIER, force, verbose, (ROUTE[3],), (ROUTE[4],))


def build_camera(force=False, verbose=False):
    """The first-person camera's library; returns its path.  It depends on everything the scanner depends on plus its own three files."""
    _, lib, source, core, header = CAMERA
    lib = os.path.join(PKG, lib)
    sources = [source, core, 'sensor_launch.h'] + [c for *_, c, _ in SENSORS[:2]] + SOURCES[1:]
    if force or _stale(lib, sources, ['hrl_envs.h', header] + [h for *_, h in SENSORS[:2]]):
        _compile(lib, source, verbose)
    return lib


def build_links(force=False, verbose=False):
    """The link states' library; returns its path.  It depends on its own three files, the shared launcher and the step's headers."""
    _, lib, source, core, header = LINKS
    lib = os.path.join(PKG, lib)
    if force or _stale(lib, [source, core, 'sensor_launch.h'] + SOURCES[1:], ['hrl_envs.h', header]):
        _compile(lib, source, verbose)
    return lib


def build_chase(force=False, verbose=False):
    """The chase camera's library; returns its path.  It depends on everything the first-person camera and the link states depend on
    plus its own three files."""
    _, lib, source, core, header = CHASE
    lib = os.path.join(PKG, lib)
    sources = [source, core, CAMERA[3], LINKS[3], 'sensor_launch.h'] + [c for *_, c, _ in SENSORS[:2]] + SOURCES[1:]
    if force or _stale(lib, sources, ['hrl_envs.h', header, CAMERA[4], LINKS[4]] + [h for *_, h in SENSORS[:2]]):
        _compile(lib, source, verbose)
    return lib


def build_dyn(force=False, verbose=False):
    """The dynamics terms' library; returns its path.  It depends on everything the link states depend on, on their specification and
    header, and on its own three files."""
    _, lib, source, core, header = DYN
    lib = os.path.join(PKG, lib)
    if force or _stale(lib, [source, core, LINKS[3], 'sensor_launch.h'] + SOURCES[1:], ['hrl_envs.h', header, LINKS[4]]):
        _compile(lib, source, verbose)
    return lib


def build_cast(force=False, verbose=False):
    """The ray test's library; returns its path.  It depends on everything the chase camera depends on, on its specification and
    header, and on its own three files."""
    _, lib, source, core, header = CAST
    lib = os.path.join(PKG, lib)
    sources = [source, core, CHASE[3], CAMERA[3], LINKS[3], 'sensor_launch.h'] + [c for *_, c, _ in SENSORS[:2]] + SOURCES[1:]
    if force or _stale(lib, sources, ['hrl_envs.h', header, CHASE[4], CAMERA[4], LINKS[4]] + [h for *_, h in SENSORS[:2]]):
        _compile(lib, source, verbose)
    return lib


def build_closest(force=False, verbose=False):
    """The closest points' library; returns its path.  It depends on everything the link states depend on, on their specification, on
    the headers its own header includes, and on its own three files."""
    _, lib, source, core, header = CLOSEST
    lib = os.path.join(PKG, lib)
    headers = ['hrl_envs.h', header, CHASE[4], CAMERA[4], LINKS[4]] + [h for *_, h in SENSORS[:2]]
    if force or _stale(lib, [source, core, LINKS[3], 'sensor_launch.h'] + SOURCES[1:], headers):
        _compile(lib, source, verbose)
    return lib


def build(force=False, verbose=False):
    """The fourteen libraries; returns the step library's path."""
    if force or _stale():
        _compile(LIB, 'hrl_hip.hip', verbose)
    for name, *_ in SENSORS:
        build_sensor(name, force, verbose)
    build_route(force, verbose)
    build_see(force, verbose)
    build_frontier(force, verbose)
    build_camera(force, verbose)
    build_links(force, verbose)
    build_chase(force, verbose)
    build_dyn(force, verbose)
    build_cast(force, verbose)
    build_closest(force, verbose)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
    for _, lib, *_ in SENSORS + [ROUTE, SEE, FRONTIER, CAMERA, LINKS, CHASE, DYN, CAST, CLOSEST]:
        print(os.path.join(PKG, lib))
