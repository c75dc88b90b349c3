#!/usr/bin/env python3
"""Time of one launch of the batched point probes (BatchedEnv.probe, include/hrl_probe.h).  GPU box:

    python tools/probe_rate.py [kind ...] [--envs N] [--frame world|ego|heading] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096; frame: default world.

The envs are settled first (300 random-action steps, as bench.py), then each of 64, 256 and 512 points per env (uniform over the arena
grown by 1 m, seeded; the library's default spec of the kind: all classes, margin = the torso's radius) is timed with HIP events, once
with all six outputs and once with `path` alone: 20 warm-up launches, then 2000 launches between two events, repeated 5 times -- the
median and the spread of the five windows are printed, one JSON line per row.  As the yardstick the same run times `env.scan()` at the
same counts of rays the same way (tools/scan_rate.py).  The kernel's VGPR / LDS / scratch figures come from the compiler
(`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import _capi as K  # noqa: E402
from hrl_pybullet_envs_amd import probe_device as P  # noqa: E402
from hrl_pybullet_envs_amd import scan_device as S  # noqa: E402
from tools.scan_rate import IDS, LAUNCHES, WINDOWS, windows  # noqa: E402

COUNTS = (64, 256, 512)


def half_extent(cfg):
    """Half sizes of the box the points are drawn from: the arena's, grown by 1 m (7 x 7 where there is none)."""
    if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ):
        return 6.0, 10.0
    if cfg.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER):
        return cfg.world_size[0] / 2 + 1.0, cfg.world_size[1] / 2 + 1.0
    return 7.0, 7.0


def measure(kind='gather', n=4096, frame='world'):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    g = torch.Generator(device='cuda').manual_seed(1)
    hx, hy = half_extent(be.cfg)
    rows = []
    common = {'kind': kind, 'envs': n, 'launches': LAUNCHES, 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)}
    for count in COUNTS:
        world = (torch.rand(n, count, 2, device='cuda', generator=g) * 2 - 1) * torch.tensor([hx, hy], device='cuda')
        pts = (world if frame == 'world' else world - be.state[:, None, 0:2]).contiguous()   # (heading: the same offsets, read along the heading)
        spec = P.default_spec(be.cfg, frame, count)
        full = P.Probe(*(torch.empty(n, count, dtype=dt, device='cuda') for _, dt in P.FIELDS))
        for what, out in (('probe', full), ('probe_path', P.Probe(path=full.path))):
            us, lo, hi = windows(lambda: be.probe(pts, spec, out=out))
            rows.append(dict(common, what=what, points=count, frame=frame, margin=round(spec.margin, 3), us_per_launch=us, us_min=lo, us_max=hi,
                             mpoints_per_s=round(n * count / us, 1), reachable=round(float((full.path < float('inf')).float().mean()), 4),
                             round_the_box=round(float((full.via >= P.VIA_CORNER0).float().mean()), 4), visible=round(float((full.blocker == 0).float().mean()), 4)))
        sspec = S.default_spec(be.cfg, 'heading', count)
        sout = torch.empty(n, count, device='cuda'), torch.empty(n, count, dtype=torch.int32, device='cuda')
        us, lo, hi = windows(lambda: be.scan(sspec, out=sout))
        rows.append(dict(common, what='scan', rays=count, frame='heading', us_per_launch=us, us_min=lo, us_max=hi, mrays_per_s=round(n * count / us, 1)))
    env.close()
    return rows


def main():
    argv, json_file, n, frame = sys.argv[1:], None, 4096, 'world'
    for flag in ('--json', '--envs', '--frame'):
        if flag in argv:
            i = argv.index(flag)
            value = argv[i + 1]
            del argv[i:i + 2]
            if flag == '--json':
                json_file = value
            elif flag == '--envs':
                n = int(value)
            else:
                frame = value
    kinds = argv or ['gather', 'maze']
    if not torch.cuda.is_available():
        sys.exit('probe_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n, frame):
            what = {'probe': f"{r.get('points')} points, all six outputs", 'probe_path': f"{r.get('points')} points, path alone", 'scan': f"scan, {r.get('rays')} rays"}[r['what']]
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_launch']} us per launch (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
