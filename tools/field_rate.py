#!/usr/bin/env python3
"""Time of one launch of the batched navigation field (BatchedEnv.field, include/hrl_field.h).  GPU box:

    python tools/field_rate.py [kind ...] [--envs N] [--mode world|ego|ego_heading] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096; mode: default world.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default field (field_device.default_spec: WALL | BOX |
POISON in the way, margin = the torso's radius, towards the food / the target) is timed at 16 x 16, 32 x 32 and 64 x 64 cells with HIP
events, once with both outputs and once with `dist` alone: 20 warm-up launches, then 500 launches between two events, repeated 5 times
-- the median and the spread of the five windows are printed, one JSON line per row.  `longest_way` is the largest number of steps
`parent` takes from any cell to its source: the kernel's Jacobi rounds are at most that plus one (a round per step of the way that
needs the fewest, and the round that changes nothing).  For scale the same run times `env.probe()` at 512 points (all six outputs) the
same way (tools/probe_rate.py).  The kernel's VGPR / LDS / scratch figures come from the compiler
(`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import field_device as F  # noqa: E402
from hrl_pybullet_envs_amd import probe_device as P  # noqa: E402
from tools.probe_rate import half_extent  # noqa: E402
from tools.scan_rate import IDS, WARMUP, WINDOWS  # noqa: E402

SIZES = (16, 32, 64)
LAUNCHES = 500   # a window of 500 launches lasts 10 to 300 ms


def windows(launch, launches=LAUNCHES):
    """Median, min and max over WINDOWS windows of the time per launch in microseconds; warm-up excluded."""
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            launch()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / launches)
    times.sort()
    return round(times[WINDOWS // 2], 2), round(times[0], 2), round(times[-1], 2)


def longest_way(parent):
    """The largest number of steps `parent` [N, H, W] takes from a cell to its source, by relaxing the step count in torch."""
    n, h, w = parent.shape
    d = torch.tensor(F.DIRECTIONS, device=parent.device)
    moving = parent < 8
    k = torch.where(moving, parent, torch.zeros_like(parent)).long()
    rows = (torch.arange(h, device=parent.device)[None, :, None] + d[k][..., 1]).clamp(0, h - 1)
    cols = (torch.arange(w, device=parent.device)[None, None, :] + d[k][..., 0]).clamp(0, w - 1)
    nxt = (rows * w + cols).reshape(n, -1)
    steps = torch.zeros(n, h * w, dtype=torch.int32, device=parent.device)
    mv = moving.reshape(n, -1)
    for _ in range(h * w):
        new = torch.where(mv, torch.gather(steps, 1, nxt) + 1, steps)
        if torch.equal(new, steps):
            break
        steps = new
    return int(steps.max())


def measure(kind='gather', n=4096, mode='world'):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)}
    for size in SIZES:
        spec = F.default_spec(be.cfg, mode, size, size)
        full = F.Field(*(torch.empty(n, size, size, dtype=dt, device='cuda') for _, dt in F.FIELDS))
        for what, out in (('field', full), ('field_dist', F.Field(dist=full.dist))):
            us, lo, hi = windows(lambda: be.field(spec, out=out))
            rows.append(dict(common, what=what, cells=f'{size}x{size}', mode=mode, margin=round(spec.margin, 3), blocking=spec.blocking, sources=spec.sources, launches=LAUNCHES,
                             us_per_launch=us, us_min=lo, us_max=hi, mcells_per_s=round(n * size * size / us, 1), reached=round(float(torch.isfinite(full.dist).float().mean()), 4),
                             blocked=round(float((full.parent == F.BLOCKED).float().mean()), 4), longest_way=longest_way(full.parent)))
    g = torch.Generator(device='cuda').manual_seed(1)
    hx, hy = half_extent(be.cfg)
    pts = ((torch.rand(n, 512, 2, device='cuda', generator=g) * 2 - 1) * torch.tensor([hx, hy], device='cuda')).contiguous()
    pspec = P.default_spec(be.cfg, 'world', 512)
    pout = P.Probe(*(torch.empty(n, 512, dtype=dt, device='cuda') for _, dt in P.FIELDS))
    us, lo, hi = windows(lambda: be.probe(pts, pspec, out=pout), 2000)
    rows.append(dict(common, what='probe', points=512, frame='world', launches=2000, us_per_launch=us, us_min=lo, us_max=hi))
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
        sys.exit('field_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n, mode):
            what = {'field': f"{r.get('cells')} cells, dist and parent", 'field_dist': f"{r.get('cells')} cells, dist alone", 'probe': 'probe, 512 points, all six outputs'}[r['what']]
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_launch']} us per launch (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
