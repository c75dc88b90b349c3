#!/usr/bin/env python3
"""Time of one launch of the batched renderer (BatchedEnv.render, include/hrl_render.h).  GPU box:

    python tools/render_rate.py [kind] [envs] [size] [mode] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default gather); envs: default 4096; size: the image's width = height, a multiple
of 16 (default 64); mode: world | ego | ego_heading (default world).

The envs are settled first (300 random-action steps, as bench.py), then the launch is timed with HIP events: 20 warm-up launches, then
200 launches between two events, repeated 5 times -- the median and the spread of the five windows are printed, with the bytes of the
frame and the write bandwidth they imply.  The kernel's VGPR / LDS / scratch figures come from the compiler
(`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import render_device as R  # noqa: E402

IDS = {'gather': 'AntGatherBulletEnv-v0', 'point': 'PointGatherBulletEnv-v0', 'maze': 'AntMazeBulletEnv-v0', 'flat': 'AntMjEnv-v0',
       'maze_mj': 'AntMazeMjEnv-v0', 'flagrun': 'AntFlagrunBulletEnv-v0'}
WARMUP, LAUNCHES, WINDOWS = 20, 200, 5


def measure(kind='gather', n=4096, size=64, mode='world'):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    view = R.default_view(be.cfg, mode, size, size)
    out = torch.empty(n, size, size, 3, dtype=torch.uint8, device='cuda')
    for _ in range(WARMUP):
        be.render(view, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(LAUNCHES):
            be.render(view, out=out)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / LAUNCHES)
    times.sort()
    us, nbytes = times[WINDOWS // 2], out.numel()
    colours = int(torch.unique(out.view(-1, 3)[:: max(1, out.numel() // 3 // 200000)], dim=0).shape[0])
    env.close()
    return {'kind': kind, 'envs': n, 'size': size, 'mode': mode, 'us_per_launch': round(us, 2), 'us_min': round(times[0], 2), 'us_max': round(times[-1], 2),
            'frame_bytes': nbytes, 'write_GBps': round(nbytes / us * 1e-3, 1), 'mpixels_per_s': round(n * size * size / us, 1), 'colours_seen': colours,
            'launches': LAUNCHES, 'windows': WINDOWS, 'device': torch.cuda.get_device_name(0)}


def main():
    argv, json_file = sys.argv[1:], None
    if '--json' in argv:
        i = argv.index('--json')
        json_file = argv[i + 1]
        del argv[i:i + 2]
    args = argv
    kind = args[0] if len(args) > 0 else 'gather'
    n = int(args[1]) if len(args) > 1 else 4096
    size = int(args[2]) if len(args) > 2 else 64
    mode = args[3] if len(args) > 3 else 'world'
    if not torch.cuda.is_available():
        sys.exit('render_rate.py needs the GPU: a time taken elsewhere says nothing')
    r = measure(kind, n, size, mode)
    print(f"{IDS[kind]} x {n}, {size} x {size}, {mode}: {r['us_per_launch']} us per launch (windows {r['us_min']} .. {r['us_max']}), "
          f"{r['frame_bytes'] / 1e6:.1f} MB -> {r['write_GBps']} GB/s written, {r['mpixels_per_s']} Mpixel/s")
    print(json.dumps(r))
    if json_file:
        with open(json_file, 'a') as f:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
