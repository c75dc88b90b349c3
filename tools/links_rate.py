#!/usr/bin/env python3
"""Time of one launch of the batched link states (BatchedEnv.links, include/hrl_links.h).  GPU box:

    python tools/links_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default spec (world frame, the four foot tips as
sites) is timed with HIP events, once asking all seven outputs and once `com` alone.  A yardstick is timed IN THE SAME PROCESS AND
INTERLEAVED, window by window (20 warm-up launches each, then 5 rounds; a round gives every candidate one window of 2000 launches between
two events; the median window and the spread are printed, one JSON line per row):

  scan    `env.scan()` with 64 rays, the default ring.  `over_scan` = the links' time / this.

`bytes_per_env` = what the launch reads and writes per env (the 128-byte state record and the outputs asked for), and `gb_per_s` = that
over the launch's time: the launch moves about 1 KB per env, so against an HBM of several TB/s its time is the time of a dispatch, not
of its traffic.  The kernel's VGPR / LDS / scratch figures come from the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints
its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import links_device as Lk  # noqa: E402
from hrl_pybullet_envs_amd import scan_device as S  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402
from tools.see_rate import interleaved  # noqa: E402

LAUNCHES = 2000   # per window


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    spec = Lk.default_spec(be.cfg, 'world')
    full = Lk.Links(*(torch.empty((n,) + shape, device='cuda') for shape in Lk.shapes(be.cfg, spec)))
    alone = Lk.Links(com=torch.empty((n,) + Lk.shapes(be.cfg, spec)[1], device='cuda'))
    sspec = S.default_spec(be.cfg, 'heading', 64)
    sout = (torch.empty(n, 64, device='cuda'), torch.empty(n, 64, dtype=torch.int32, device='cuda'))
    t = interleaved({'all': lambda: be.links(spec, out=full), 'com': lambda: be.links(spec, out=alone), 'scan': lambda: be.scan(sspec, out=sout)}, LAUNCHES)
    common = {'kind': kind, 'envs': n, 'windows': 5, 'launches': LAUNCHES, 'device': torch.cuda.get_device_name(0)}
    rows = [dict(common, what='scan', rays=64, us_per_call=t['scan'][0], us_min=t['scan'][1], us_max=t['scan'][2])]
    for what, outs, tensors in (('all', 'all seven', full), ('com', 'com', alone)):
        per_env = 128 + sum(x[0].numel() * 4 for x in tensors if x is not None)
        rows.append(dict(common, what='links', outputs=outs, links=Lk.n_links(be.cfg), sites=spec.n_sites, us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                         bytes_per_env=per_env, gb_per_s=round(per_env * n / t[what][0] / 1e3, 1), ns_per_env=round(t[what][0] * 1e3 / n, 3), over_scan=round(t[what][0] / t['scan'][0], 2)))
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
        sys.exit('links_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            what = f"links ({r['outputs']}): {r['bytes_per_env']} B per env, {r['gb_per_s']} GB/s, {r['over_scan']} x the scan" if r['what'] == 'links' else f"scan of {r['rays']} rays"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
