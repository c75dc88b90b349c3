#!/usr/bin/env python3
"""Time of one launch of the batched ray test (BatchedEnv.cast, include/hrl_cast.h).  GPU box:

    python tools/cast_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then a 3-D lidar of 64, 256 and 1024 rays per env (16 x 4, 32 x 8 and
64 x 16 azimuths x elevation rings from -60 to +20 degrees, 0.3 to 8 m, the heading frame, every class) is timed with HIP events, once
asking all four outputs and once `fraction` alone.  Two yardsticks are timed IN THE SAME PROCESS AND INTERLEAVED, window by window (20
warm-up launches each, then 5 rounds; a round gives every candidate one window of 1000 launches between two events -- 300 at 1024 rays;
the median window and the spread are printed, one JSON line per row):

  scan   `env.scan()` at the same ray count (512 at most: its maximum): a flat ring against the same table of scene slots, no z, no
         robot, no ground, no point and no normal.  `over_scan` = the ray test's time per ray / the scanner's.
  chase  `env.chase()`, all three outputs, at a pixel count near the ray count (16 x 8 -- its smallest image --, 16 x 16, 32 x 32): the
         same solids and the same intersections from one eye per env.  `over_chase` = the ray test's time per ray / its time per pixel.

`ns_per_ray` = the launch's time over envs x rays.  `hit` is the share of rays that met anything, `robot` the share that met the robot.
The kernel's VGPR / LDS / scratch figures come from the compiler (`SRC=cast_hip.hip tools/kernel_resources.sh`)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import cast_device as Ca  # noqa: E402
from hrl_pybullet_envs_amd import chase_device as Ch  # noqa: E402
from hrl_pybullet_envs_amd import scan_device as S  # noqa: E402
from tools.chase_rate import interleaved  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402

PATTERNS = {64: (16, 4), 256: (32, 8), 1024: (64, 16)}      # rays: azimuths, rings
CHASE_SIZES = {64: (16, 8), 256: (16, 16), 1024: (32, 32)}  # width, height
LAUNCHES = {64: 1000, 256: 1000, 1024: 300}                 # per window
SCAN_MAX = 512


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': 5, 'device': torch.cuda.get_device_name(0)}
    for R, (az, rings) in PATTERNS.items():
        rays = Ca.expand(Ca.lidar_rays(az, tuple(np.linspace(-60.0, 20.0, rings)), 8.0, 0.3), n, 'cuda')   # materialised once
        spec = Ca.default_spec(be.cfg, 'heading', R)
        full = Ca.Cast(torch.empty(n, R, device='cuda'), torch.empty(n, R, dtype=torch.int32, device='cuda'), torch.empty(n, R, 3, device='cuda'), torch.empty(n, R, 3, device='cuda'))
        alone = Ca.Cast(fraction=torch.empty(n, R, device='cuda'))
        sr = min(R, SCAN_MAX)
        sspec = S.default_spec(be.cfg, 'heading', sr)
        sout = (torch.empty(n, sr, device='cuda'), torch.empty(n, sr, dtype=torch.int32, device='cuda'))
        w, h = CHASE_SIZES[R]
        cspec = Ch.default_spec(be.cfg, 'heading', w, h)
        cout = Ch.Chase(torch.empty(n, h, w, device='cuda'), torch.empty(n, h, w, dtype=torch.int32, device='cuda'), torch.empty(n, h, w, 3, dtype=torch.uint8, device='cuda'))
        k = LAUNCHES[R]
        t = interleaved({'all': (lambda: be.cast(rays, spec, out=full), k), 'fraction': (lambda: be.cast(rays, spec, out=alone), k),
                         'scan': (lambda: be.scan(sspec, out=sout), k), 'chase': (lambda: be.chase(cspec, out=cout), k)})
        common['launches'] = k
        kinds = full.seg & 255
        hit, robot = round(float((kinds != 0).float().mean()), 4), round(float((kinds == Ca.HIT_ROBOT).float().mean()), 4)
        scan_pr, chase_pp = t['scan'][0] * 1e3 / (n * sr), t['chase'][0] * 1e3 / (n * w * h)
        rows.append(dict(common, what='scan', rays=sr, us_per_call=t['scan'][0], us_min=t['scan'][1], us_max=t['scan'][2], ns_per_ray=round(scan_pr, 4)))
        rows.append(dict(common, what='chase', pixels=f'{w}x{h}', us_per_call=t['chase'][0], us_min=t['chase'][1], us_max=t['chase'][2], ns_per_pixel=round(chase_pp, 4)))
        for what, outs in (('all', 'fraction + seg + point + normal'), ('fraction', 'fraction')):
            pr = t[what][0] * 1e3 / (n * R)
            rows.append(dict(common, what='cast', outputs=outs, rays=R, us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2], ns_per_ray=round(pr, 4),
                             over_scan=round(pr / scan_pr, 2), over_chase=round(pr / chase_pp, 2), hit=hit, robot=robot))
        del rays, full, alone, sout, cout
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
        sys.exit('cast_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'cast':
                what = (f"{r['rays']} rays, cast ({r['outputs']}): {r['ns_per_ray']} ns per ray, {r['over_scan']} x the scanner per ray, {r['over_chase']} x the chase camera per pixel, "
                        f"{100 * r['hit']:.1f} % hit, {100 * r['robot']:.1f} % robot")
            else:
                what = f"scan of {r['rays']} rays ({r['ns_per_ray']} ns per ray)" if r['what'] == 'scan' else f"chase of {r['pixels']} pixels ({r['ns_per_pixel']} ns per pixel)"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
