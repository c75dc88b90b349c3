#!/usr/bin/env python3
"""Time of one launch of the batched range scanner (BatchedEnv.scan, include/hrl_scan.h).  GPU box:

    python tools/scan_rate.py [kind] [envs] [frame] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default gather); envs: default 4096; frame: heading | world (default heading).

The envs are settled first (300 random-action steps, as bench.py), then each of 64, 256 and 512 rays (the library's default spec of the
kind: all classes, out to the arena's diagonal) is timed with HIP events: 20 warm-up launches, then 2000 launches between two events,
repeated 5 times -- the median and the spread of the five windows are printed, one JSON line per ray count.  For context the same run
times `env.render()` at 64 x 64 (the renderer's default world view) the same way.  The kernel's VGPR / LDS / scratch figures come from
the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import render_device as R  # noqa: E402
from hrl_pybullet_envs_amd import scan_device as S  # noqa: E402

IDS = {'gather': 'AntGatherBulletEnv-v0', 'point': 'PointGatherBulletEnv-v0', 'maze': 'AntMazeBulletEnv-v0', 'flat': 'AntMjEnv-v0',
       'maze_mj': 'AntMazeMjEnv-v0', 'flagrun': 'AntFlagrunBulletEnv-v0'}
RAYS = (64, 256, 512)
WARMUP, LAUNCHES, WINDOWS = 20, 2000, 5   # a window of 2000 launches lasts 20 to 150 ms


def windows(launch):
    """Median, min and max over WINDOWS windows of the time per launch in microseconds; warm-up excluded."""
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(LAUNCHES):
            launch()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / LAUNCHES)
    times.sort()
    return round(times[WINDOWS // 2], 2), round(times[0], 2), round(times[-1], 2)


def measure(kind='gather', n=4096, frame='heading'):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    for rays in RAYS:
        spec = S.default_spec(be.cfg, frame, rays)
        out = torch.empty(n, rays, device='cuda'), torch.empty(n, rays, dtype=torch.int32, device='cuda')
        us, lo, hi = windows(lambda: be.scan(spec, out=out))
        cls = S.decode(out[1])[0]
        rows.append({'what': 'scan', 'kind': kind, 'envs': n, 'rays': rays, 'frame': frame, 'us_per_launch': us, 'us_min': lo, 'us_max': hi,
                     'mrays_per_s': round(n * rays / us, 1), 'rays_that_hit': round(float((cls != 0).float().mean()), 4), 'mean_range': round(float(out[0].mean()), 3),
                     'launches': LAUNCHES, 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)})
    view = R.default_view(be.cfg, 'world', 64, 64)
    img = torch.empty(n, 64, 64, 3, dtype=torch.uint8, device='cuda')
    us, lo, hi = windows(lambda: be.render(view, out=img))
    rows.append({'what': 'render', 'kind': kind, 'envs': n, 'size': 64, 'mode': 'world', 'us_per_launch': us, 'us_min': lo, 'us_max': hi,
                 'launches': LAUNCHES, 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)})
    env.close()
    return rows


def main():
    argv, json_file = sys.argv[1:], None
    if '--json' in argv:
        i = argv.index('--json')
        json_file = argv[i + 1]
        del argv[i:i + 2]
    kind = argv[0] if len(argv) > 0 else 'gather'
    n = int(argv[1]) if len(argv) > 1 else 4096
    frame = argv[2] if len(argv) > 2 else 'heading'
    if not torch.cuda.is_available():
        sys.exit('scan_rate.py needs the GPU: a time taken elsewhere says nothing')
    for r in measure(kind, n, frame):
        what = f"{r['rays']} rays, {frame}" if r['what'] == 'scan' else 'render 64 x 64, world'
        print(f"{IDS[kind]} x {n}, {what}: {r['us_per_launch']} us per launch (windows {r['us_min']} .. {r['us_max']})")
        print(json.dumps(r))
        if json_file:
            with open(json_file, 'a') as f:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
