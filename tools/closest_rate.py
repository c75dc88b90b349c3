#!/usr/bin/env python3
"""Time of one launch of the batched closest points (BatchedEnv.closest, include/hrl_closest.h).  GPU box:

    python tools/closest_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the query under every class is timed with HIP events, once
asking all five outputs and once `distance` alone.  Two yardsticks are timed IN THE SAME PROCESS AND INTERLEAVED, window by window (20
warm-up launches each, then 5 rounds; a round gives every candidate one window of 1000 launches between two events; the median window
and the spread are printed, one JSON line per row):

  links  `env.links()`, all seven outputs at the default sites: the same forward kinematics once per link, and nothing else.
  cast   `env.cast()` of a 64-ray lidar (16 x 4, the heading frame, every class), all four outputs: the other query that walks every
         shape of the scene and every link of the robot.

`ns_per_cell` = the launch's time over envs x links x 6 classes.  `near` is the share of the finite cells within 0.1 m, `none` the
share of cells without a surface.  The kernel's VGPR / LDS / scratch figures come from the compiler
(`SRC=closest_hip.hip tools/kernel_resources.sh`)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import cast_device as Ca  # noqa: E402
from hrl_pybullet_envs_amd import closest_device as Cl  # noqa: E402
from hrl_pybullet_envs_amd import links_device as Lk  # noqa: E402
from tools.chase_rate import interleaved  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402

LAUNCHES = 1000   # per window
RAYS = 64


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    common = {'kind': kind, 'envs': n, 'windows': 5, 'launches': LAUNCHES, 'device': torch.cuda.get_device_name(0)}
    spec = Cl.default_spec(be.cfg)
    full = Cl.Closest(*(torch.empty(shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(Cl.shapes(be.cfg, spec, (n,)), Cl.FIELDS)))
    alone = Cl.Closest(distance=torch.empty_like(full.distance))
    lspec = Lk.default_spec(be.cfg)
    lout = be.links(lspec)
    rays = Ca.expand(Ca.lidar_rays(16, tuple(np.linspace(-60.0, 20.0, 4)), 8.0, 0.3), n, 'cuda')   # materialised once
    cspec = Ca.default_spec(be.cfg, 'heading', RAYS)
    cout = be.cast(rays, cspec)
    t = interleaved({'all': (lambda: be.closest(spec, out=full), LAUNCHES), 'distance': (lambda: be.closest(spec, out=alone), LAUNCHES),
                     'links': (lambda: be.links(lspec, out=lout), LAUNCHES), 'cast': (lambda: be.cast(rays, cspec, out=cout), LAUNCHES)})
    cells = full.distance.numel()
    met = full.which != Cl.HIT_NONE
    near, none = round(float((full.distance[met] <= 0.1).float().mean()), 4), round(float((~met).float().mean()), 4)
    rows = [dict(common, what='links', us_per_call=t['links'][0], us_min=t['links'][1], us_max=t['links'][2]),
            dict(common, what='cast', rays=RAYS, us_per_call=t['cast'][0], us_min=t['cast'][1], us_max=t['cast'][2])]
    for what, outs in (('all', 'distance + which + on_link + on_surface + normal'), ('distance', 'distance')):
        rows.append(dict(common, what='closest', outputs=outs, cells_per_env=cells // n, us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                         ns_per_cell=round(t[what][0] * 1e3 / cells, 4), over_links=round(t[what][0] / t['links'][0], 2), over_cast=round(t[what][0] / t['cast'][0], 2), near=near, none=none))
    env.close()
    return rows


def main():
    argv, json_file, n = sys.argv[1:], None, 4096
    for flag in ('--json', '--envs'):
        if flag in argv:
            i = argv.index(flag)
            value = argv[i + 1]
            del argv[i:i + 2]
            if flag == '--json':
                json_file = value
            else:
                n = int(value)
    kinds = argv or ['gather', 'maze']
    if not torch.cuda.is_available():
        sys.exit('closest_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'closest':
                what = (f"closest ({r['outputs']}): {r['ns_per_cell']} ns per cell, {r['over_links']} x the link states, {r['over_cast']} x the ray test at {RAYS} rays, "
                        f"{100 * r['near']:.1f} % of the finite cells within 0.1 m, {100 * r['none']:.1f} % without a surface")
            else:
                what = 'link states (seven outputs)' if r['what'] == 'links' else f'ray test of {RAYS} rays (four outputs)'
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
