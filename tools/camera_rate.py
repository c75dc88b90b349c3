#!/usr/bin/env python3
"""Time of one launch of the batched first-person camera (BatchedEnv.camera, include/hrl_camera.h).  GPU box:

    python tools/camera_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default camera (camera_device.default_spec: turning
with the heading, 90 degrees, from the torso, every class and the ground) is timed at 32 x 24, 64 x 48 and 128 x 96 pixels with HIP
events, once asking all three outputs and once `depth` alone.  Two yardsticks are timed IN THE SAME PROCESS AND INTERLEAVED, window by
window (20 warm-up launches each, then 5 rounds; a round gives every candidate one window of 2000, 1000 or 400 launches between two
events, the fewer the larger the image -- the camera's windows last 0.08 to 0.65 s, the scanner's 20 ms as in tools/scan_rate.py; the median
window and the spread are printed, one JSON line per row):

  scan    `env.scan()` with as many rays as the image has columns, over the same 90 degrees: per RAY the camera does the scanner's work
          (a column's ground-plan ray against the same table), and then once more for every row.  `over_scan` = the camera's time / this.
  render  `env.render()` at the same pixel count (32 x 24 as 48 x 16: the renderer's sides are multiples of 16), the ego-heading view:
          per PIXEL the camera does a fraction of the renderer's work.  `over_render`.

`ns_per_pixel` = the launch's time over envs x pixels.  `hit` is the share of pixels that saw anything.  The kernel's VGPR / LDS / scratch
figures come from the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import camera_device as Cm  # noqa: E402
from hrl_pybullet_envs_amd import render_device as R  # noqa: E402
from hrl_pybullet_envs_amd import scan_device as S  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402
from tools.see_rate import interleaved  # noqa: E402

SIZES = ((32, 24), (64, 48), (128, 96))           # width, height
RENDER_SIZES = {(32, 24): (48, 16)}               # the same pixel count in multiples of 16
LAUNCHES = {(32, 24): 2000, (64, 48): 1000, (128, 96): 400}   # per window


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': 5, 'device': torch.cuda.get_device_name(0)}
    for w, h in SIZES:
        spec = Cm.default_spec(be.cfg, 'heading', w, h)
        full = Cm.Camera(torch.empty(n, h, w, device='cuda'), torch.empty(n, h, w, dtype=torch.int32, device='cuda'), torch.empty(n, h, w, 3, dtype=torch.uint8, device='cuda'))
        alone = Cm.Camera(depth=torch.empty(n, h, w, device='cuda'))
        sspec = S.default_spec(be.cfg, 'heading', w)
        sspec.first_angle, sspec.step_angle, sspec.max_range = -math.pi / 4 + math.pi / 4 / w, math.pi / 2 / w, spec.max_range
        sout = (torch.empty(n, w, device='cuda'), torch.empty(n, w, dtype=torch.int32, device='cuda'))
        rw, rh = RENDER_SIZES.get((w, h), (w, h))
        view = R.default_view(be.cfg, 'ego_heading', rw, rh)
        rout = torch.empty(n, rh, rw, 3, dtype=torch.uint8, device='cuda')
        t = interleaved({'all': lambda: be.camera(spec, out=full), 'depth': lambda: be.camera(spec, out=alone), 'scan': lambda: be.scan(sspec, out=sout),
                         'render': lambda: be.render(view, out=rout)}, LAUNCHES[(w, h)])
        common['launches'] = LAUNCHES[(w, h)]
        hit = round(float((full.seg != 0).float().mean()), 4)
        rows.append(dict(common, what='scan', rays=w, us_per_call=t['scan'][0], us_min=t['scan'][1], us_max=t['scan'][2]))
        rows.append(dict(common, what='render', pixels=f'{rw}x{rh}', us_per_call=t['render'][0], us_min=t['render'][1], us_max=t['render'][2]))
        for what, outs in (('all', 'depth + seg + rgb'), ('depth', 'depth')):
            rows.append(dict(common, what='camera', outputs=outs, pixels=f'{w}x{h}', us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                             ns_per_pixel=round(t[what][0] * 1e3 / (n * w * h), 4), over_scan=round(t[what][0] / t['scan'][0], 2), over_render=round(t[what][0] / t['render'][0], 2),
                             hit=hit))
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
        sys.exit('camera_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'camera':
                what = f"{r['pixels']} pixels, camera ({r['outputs']}): {r['ns_per_pixel']} ns per pixel, {r['over_scan']} x the scan, {r['over_render']} x the render, {100 * r['hit']:.1f} % hit"
            else:
                what = f"scan of {r['rays']} rays" if r['what'] == 'scan' else f"render of {r['pixels']} pixels"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
