#!/usr/bin/env python3
"""Time of one launch of the batched visibility map (BatchedEnv.see, include/hrl_see.h).  GPU box:

    python tools/see_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default map (see_device.default_spec: the world grid,
WALL | BOX occlude, all round, a slack of one cell) is timed at 16 x 16, 32 x 32 and 64 x 64 cells with HIP events, once asking `visible`
alone and once `visible + seen + fresh`.  Two yardsticks are timed IN THE SAME PROCESS AND INTERLEAVED, window by window (20 warm-up
launches each, then 5 rounds; a round gives every candidate one window of 500 launches between two events; the median window and the
spread are printed, one JSON line per row):

  probe   the same number of segment tests through the existing point probes: the cell centres as world points, in launches of at most 512
          points (eight at 64 x 64), asking only `sight` and `blocker`, with classes = the map's occluders.  `over_probe` = the map's time /
          this.
  field   `env.field()` on the same grid (field_device.default_spec): `over_field`.

`lit` is the share of visible cells.  The kernel's VGPR / LDS / scratch figures come from the compiler (`python -m
hrl_pybullet_envs_amd.build --force` prints its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import field_device as F  # noqa: E402
from hrl_pybullet_envs_amd import probe_device as P  # noqa: E402
from hrl_pybullet_envs_amd import see_device as V  # noqa: E402
from tools.field_rate import LAUNCHES, SIZES  # noqa: E402
from tools.scan_rate import IDS, WARMUP, WINDOWS  # noqa: E402


def interleaved(launchers, launches=LAUNCHES):
    """{name: (median, min, max)} of the time per call in microseconds over WINDOWS rounds; in a round every launcher gets one window."""
    for launch in launchers.values():
        for _ in range(WARMUP):
            launch()
    torch.cuda.synchronize()
    times = {name: [] for name in launchers}
    for _ in range(WINDOWS):
        for name, launch in launchers.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                launch()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / launches)
    return {name: (round(sorted(t)[WINDOWS // 2], 2), round(min(t), 2), round(max(t), 2)) for name, t in times.items()}


def cell_points(spec, state):
    """The cell centres of a world grid as world points: float32 [N, H * W, 2]."""
    n = state.shape[0]
    centre, right, up = F.axes(spec, state)
    w, h, he = spec.width, spec.height, spec.half_extent
    u = ((torch.arange(w, device=state.device) + 0.5) * 2 / w - 1) * he
    v = (h / w - (torch.arange(h, device=state.device) + 0.5) * 2 / w) * he
    vv, uu = torch.meshgrid(v, u, indexing='ij')
    pts = centre[:, None, :] + uu.reshape(1, -1, 1) * right[:, None, :] + vv.reshape(1, -1, 1) * up[:, None, :]
    return pts.reshape(n, h * w, 2).float().contiguous()


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': WINDOWS, 'launches': LAUNCHES, 'device': torch.cuda.get_device_name(0)}
    for size in SIZES:
        spec = V.default_spec(be.cfg, 'world', size, size)
        alone = V.See(torch.empty(n, size, size, dtype=torch.uint8, device='cuda'))
        full = V.See(torch.empty(n, size, size, dtype=torch.uint8, device='cuda'), V.memory(n, spec, 'cuda'), torch.empty(n, dtype=torch.int32, device='cuda'))
        fspec = F.default_spec(be.cfg, 'world', size, size)
        fout = F.Field(*(torch.empty(n, size, size, dtype=dt, device='cuda') for _, dt in F.FIELDS))
        pts = cell_points(spec, be.state)
        per = min(size * size, P.MAX_POINTS)
        chunks = [pts[:, lo:lo + per].contiguous() for lo in range(0, size * size, per)]
        pspec = P.default_spec(be.cfg, 'world', per)
        pspec.classes = spec.occluders
        pouts = [P.Probe(sight=torch.empty(n, per, device='cuda'), blocker=torch.empty(n, per, dtype=torch.int32, device='cuda')) for _ in chunks]

        def probes():
            for c, o in zip(chunks, pouts):
                be.probe(c, pspec, out=o)

        t = interleaved({'visible': lambda: be.see(spec, out=alone), 'memory': lambda: be.see(spec, out=full), 'probe': probes, 'field': lambda: be.field(fspec, out=fout)})
        lit = round(float(alone.visible.float().mean()), 4)
        for what in ('probe', 'field'):
            rows.append(dict(common, what=what, cells=f'{size}x{size}', launches_per_call=len(chunks) if what == 'probe' else 1, us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2]))
        for what, outs in (('visible', 'visible'), ('memory', 'visible + seen + fresh')):
            rows.append(dict(common, what='see', outputs=outs, cells=f'{size}x{size}', us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                             over_probe=round(t[what][0] / t['probe'][0], 2), over_field=round(t[what][0] / t['field'][0], 2), lit=lit))
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
        sys.exit('see_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'see':
                what = f"{r['cells']} cells, see ({r['outputs']}): {r['over_probe']} x the probes, {r['over_field']} x the field, {100 * r['lit']:.1f} % lit"
            else:
                what = f"{r['cells']} cells, {r['what']} ({r['launches_per_call']} launch(es))"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
