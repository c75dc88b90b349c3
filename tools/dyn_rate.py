#!/usr/bin/env python3
"""Time of one launch of the batched dynamics terms (BatchedEnv.dynamics, include/hrl_dyn.h).  GPU box:

    python tools/dyn_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default spec (the four foot tips as sites) is timed
with HIP events under the torques of a random action, asking all seven outputs, `mass` alone and `accel` alone.  A yardstick is timed IN
THE SAME PROCESS AND INTERLEAVED, window by window (20 warm-up launches each, then 5 rounds; a round gives every candidate one window of
2000 launches between two events; the median window and the spread are printed, one JSON line per row):

  links   `env.links()` with the default spec, all seven outputs: the neighbour kernel of the same lane mapping.  `over_links` = the
          dynamics' time / this.

`bytes_per_env` = what the launch reads and writes per env (the 128-byte state record, tau where accel is asked, and the outputs asked
for), and `gb_per_s` = that over the launch's time.  The kernel's VGPR / LDS / scratch figures come from the compiler
(`SRC=dyn_hip.hip tools/kernel_resources.sh`)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import dyn_device as Dy  # noqa: E402
from hrl_pybullet_envs_amd import links_device as Lk  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402
from tools.see_rate import interleaved  # noqa: E402

LAUNCHES = 2000   # per window


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    spec = Dy.default_spec(be.cfg)
    shapes = Dy.shapes(be.cfg, spec)
    tau = Dy.torques(be.cfg, torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    full = Dy.Dynamics(*(torch.empty((n,) + shape, device='cuda') for shape in shapes))
    mass = Dy.Dynamics(mass=torch.empty((n,) + shapes[0], device='cuda'))
    accel = Dy.Dynamics(accel=torch.empty((n,) + shapes[2], device='cuda'))
    lspec = Lk.default_spec(be.cfg, 'world')
    lout = Lk.Links(*(torch.empty((n,) + shape, device='cuda') for shape in Lk.shapes(be.cfg, lspec)))
    t = interleaved({'all': lambda: be.dynamics(spec, tau=tau, out=full), 'mass': lambda: be.dynamics(spec, out=mass), 'accel': lambda: be.dynamics(spec, tau=tau, out=accel),
                     'links': lambda: be.links(lspec, out=lout)}, LAUNCHES)
    common = {'kind': kind, 'envs': n, 'windows': 5, 'launches': LAUNCHES, 'device': torch.cuda.get_device_name(0)}
    rows = [dict(common, what='links', outputs='all seven', us_per_call=t['links'][0], us_min=t['links'][1], us_max=t['links'][2])]
    for what, outs, tensors in (('all', 'all seven', full), ('mass', 'mass', mass), ('accel', 'accel', accel)):
        per_env = 128 + (tau[0].numel() * 4 if tensors.accel is not None else 0) + sum(x[0].numel() * 4 for x in tensors if x is not None)
        rows.append(dict(common, what='dynamics', outputs=outs, nv=Dy.nv(be.cfg), sites=spec.n_sites, us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                         bytes_per_env=per_env, gb_per_s=round(per_env * n / t[what][0] / 1e3, 1), ns_per_env=round(t[what][0] * 1e3 / n, 3), over_links=round(t[what][0] / t['links'][0], 2)))
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
        sys.exit('dyn_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            what = f"dynamics ({r['outputs']}): {r['bytes_per_env']} B per env, {r['gb_per_s']} GB/s, {r['over_links']} x the links" if r['what'] == 'dynamics' else 'links (all seven)'
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
