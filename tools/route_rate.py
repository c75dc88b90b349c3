#!/usr/bin/env python3
"""Time of one launch of the batched routes (BatchedEnv.route, include/hrl_route.h).  GPU box:

    python tools/route_rate.py [kind ...] [--envs N] [--mode world|ego|ego_heading] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096; mode: default world.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default route (route_device.default_spec: the default
field, 16 waypoints) is timed at 16 x 16, 32 x 32 and 64 x 64 cells with HIP events (tools/field_rate.py's windows: 20 warm-up launches,
500 launches between two events, 5 times; the median and the spread are printed, one JSON line per row), once with P = 1 (starts = None,
the robot) and once with P = 64 starts drawn uniformly over the arena in the world frame.  The route launch computes the field first, so
the yardstick is `env.field()` on the field part of the same spec, timed in the same run: `over_field` = the route's time / the
field's.  `routes` is the share of starts that have a route, `waypoints` their mean count and `steps` the mean number of cells of
their chains (length / cell is a lower bound for it): what the per-start phase costs grows with the last.  The kernel's VGPR / LDS /
scratch figures come from the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import field_device as F  # noqa: E402
from hrl_pybullet_envs_amd import route_device as R  # noqa: E402
from tools.field_rate import LAUNCHES, SIZES, windows  # noqa: E402
from tools.probe_rate import half_extent  # noqa: E402
from tools.scan_rate import IDS, WINDOWS  # noqa: E402

STARTS = (1, 64)


def measure(kind='gather', n=4096, mode='world'):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': WINDOWS, 'launches': LAUNCHES, 'mode': mode, 'device': torch.cuda.get_device_name(0)}
    g = torch.Generator(device='cuda').manual_seed(1)
    hx, hy = half_extent(be.cfg)
    for size in SIZES:
        fspec = F.default_spec(be.cfg, mode, size, size)
        fout = F.Field(*(torch.empty(n, size, size, dtype=dt, device='cuda') for _, dt in F.FIELDS))
        field_us, lo, hi = windows(lambda: be.field(fspec, out=fout))
        rows.append(dict(common, what='field', cells=f'{size}x{size}', us_per_launch=field_us, us_min=lo, us_max=hi))
        for p in STARTS:
            spec = R.from_field_spec(fspec, 'ego' if p == 1 else 'world', p, 16)
            starts = None if p == 1 else ((torch.rand(n, p, 2, device='cuda', generator=g) * 2 - 1) * torch.tensor([hx, hy], device='cuda')).contiguous()
            out = R.Route(*(torch.empty(n, *shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(R.shapes(spec), R.FIELDS)))
            us, lo, hi = windows(lambda: be.route(starts, spec, out=out))
            has = out.count > 0
            steps = (out.length[has] / R.cell_size(fspec)).mean() if bool(has.any()) else torch.tensor(0.0)
            rows.append(dict(common, what='route', cells=f'{size}x{size}', starts=p, max_waypoints=16, us_per_launch=us, us_min=lo, us_max=hi, over_field=round(us / field_us, 2),
                             routes=round(float(has.float().mean()), 4), waypoints=round(float(out.count[has].float().mean()) if bool(has.any()) else 0.0, 2),
                             steps=round(float(steps), 1), truncated=round(float((out.count > 16).float().mean()), 4)))
    env.close()
    return rows


def main():
    argv, json_file, n, mode = sys.argv[1:], None, 4096, 'world'
    for flag in ('--json', '--envs', '--mode'):
        if flag in argv:
            i = argv.index(flag)
            value = argv[i + 1]
            del argv[i:i + 2]
            if flag == '--json':
                json_file = value
            elif flag == '--envs':
                n = int(value)
            else:
                mode = value
    kinds = argv or ['gather', 'maze']
    if not torch.cuda.is_available():
        sys.exit('route_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n, mode):
            what = f"{r['cells']} cells, field" if r['what'] == 'field' else f"{r['cells']} cells, route from {r['starts']} start(s): {r['over_field']} x the field"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_launch']} us per launch (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
