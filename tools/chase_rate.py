#!/usr/bin/env python3
"""Time of one launch of the batched chase camera (BatchedEnv.chase, include/hrl_chase.h).  GPU box:

    python tools/chase_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default chase camera (chase_device.default_spec: 3 m
behind the torso and 30 degrees above it, turning with the heading, 60 degrees wide, every class, tiles of 1 m) is timed at 64 x 48,
128 x 96 and 256 x 192 pixels with HIP events, once asking all three outputs and once `rgb` alone.  Two yardsticks are timed IN THE SAME
PROCESS AND INTERLEAVED, window by window (20 warm-up launches each, then 5 rounds; a round gives every candidate one window between
two events: 200, 50 or 15 launches of the chase camera, the fewer the larger the image, 800, 200 or 150 of the first-person camera and
2000 of the link states; the median window and the spread are printed, one JSON line per row):

  camera  `env.camera()`, all three outputs, at the same pixel count -- 256 x 192 is beyond its 128 x 128, so there it runs at 128 x 128
          and the ratio is taken PER PIXEL.  Per pixel the chase camera walks the same table of scene slots with 3-D rays and then the
          robot's 25 primitives.  `over_camera` = the chase camera's time per pixel / this one's.
  links   `env.links()`: the kinematics the chase camera's prologue evaluates once per primitive.  `over_links`.

`ns_per_pixel` = the launch's time over envs x pixels.  `robot` is the share of pixels that show the robot, `hit` the share that saw
anything.  The kernel's VGPR / LDS / scratch figures come from the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints its
resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import camera_device as Cm  # noqa: E402
from hrl_pybullet_envs_amd import chase_device as Ch  # noqa: E402
from tools.scan_rate import IDS  # noqa: E402
from tools.see_rate import WARMUP, WINDOWS  # noqa: E402

SIZES = ((64, 48), (128, 96), (256, 192))          # width, height
CAMERA_SIZES = {(256, 192): (128, 128)}            # the first-person camera's largest image
LAUNCHES = {(64, 48): 200, (128, 96): 50, (256, 192): 15}   # of the chase camera per window
CAMERA_LAUNCHES = {(64, 48): 800, (128, 96): 200, (128, 128): 150}
LINKS_LAUNCHES = 2000


def interleaved(launchers):
    """{name: (median, min, max)} of the time per call in microseconds over WINDOWS rounds; in a round every launcher (name: (call,
    launches per window)) gets one window (tools/see_rate.py's, with a window length per candidate)."""
    for launch, _ in launchers.values():
        for _ in range(WARMUP):
            launch()
    torch.cuda.synchronize()
    times = {name: [] for name in launchers}
    for _ in range(WINDOWS):
        for name, (launch, launches) in launchers.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                launch()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / launches)
    return {name: (round(sorted(t)[WINDOWS // 2], 2), round(min(t), 2), round(max(t), 2)) for name, t in times.items()}


def images(kind, n, w, h):
    return kind(torch.empty(n, h, w, device='cuda'), torch.empty(n, h, w, dtype=torch.int32, device='cuda'), torch.empty(n, h, w, 3, dtype=torch.uint8, device='cuda'))


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': 5, 'device': torch.cuda.get_device_name(0)}
    lout = be.links()
    for w, h in SIZES:
        spec = Ch.default_spec(be.cfg, 'heading', w, h)
        full = images(Ch.Chase, n, w, h)
        alone = Ch.Chase(rgb=torch.empty(n, h, w, 3, dtype=torch.uint8, device='cuda'))
        cw, ch = CAMERA_SIZES.get((w, h), (w, h))
        cspec = Cm.default_spec(be.cfg, 'heading', cw, ch)
        cout = images(Cm.Camera, n, cw, ch)
        k = LAUNCHES[(w, h)]
        t = interleaved({'all': (lambda: be.chase(spec, out=full), k), 'rgb': (lambda: be.chase(spec, out=alone), k),
                         'camera': (lambda: be.camera(cspec, out=cout), CAMERA_LAUNCHES[(cw, ch)]), 'links': (lambda: be.links(out=lout), LINKS_LAUNCHES)})
        common['launches'] = k
        kinds = full.seg & 255
        hit, robot = round(float((kinds != 0).float().mean()), 4), round(float((kinds == Ch.HIT_ROBOT).float().mean()), 4)
        camera_pp = t['camera'][0] * 1e3 / (n * cw * ch)
        rows.append(dict(common, what='camera', pixels=f'{cw}x{ch}', us_per_call=t['camera'][0], us_min=t['camera'][1], us_max=t['camera'][2], ns_per_pixel=round(camera_pp, 4)))
        rows.append(dict(common, what='links', us_per_call=t['links'][0], us_min=t['links'][1], us_max=t['links'][2]))
        for what, outs in (('all', 'depth + seg + rgb'), ('rgb', 'rgb')):
            pp = t[what][0] * 1e3 / (n * w * h)
            rows.append(dict(common, what='chase', outputs=outs, pixels=f'{w}x{h}', us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2], ns_per_pixel=round(pp, 4),
                             over_camera=round(pp / camera_pp, 2), over_links=round(t[what][0] / t['links'][0], 2), hit=hit, robot=robot))
        del full, alone, cout
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
        sys.exit('chase_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'chase':
                what = (f"{r['pixels']} pixels, chase ({r['outputs']}): {r['ns_per_pixel']} ns per pixel, {r['over_camera']} x the camera per pixel, {r['over_links']} x links(), "
                        f"{100 * r['hit']:.1f} % hit, {100 * r['robot']:.1f} % robot")
            else:
                what = f"camera of {r['pixels']} pixels ({r['ns_per_pixel']} ns per pixel)" if r['what'] == 'camera' else 'links()'
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
