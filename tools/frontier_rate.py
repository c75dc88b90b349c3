#!/usr/bin/env python3
"""Time of one launch of the batched frontier map (BatchedEnv.frontier, include/hrl_frontier.h).  GPU box:

    python tools/frontier_rate.py [kind ...] [--envs N] [--json FILE]

kind: gather | point | maze | flat | maze_mj | flagrun (default: gather and maze); envs: default 4096.

The envs are settled first (300 random-action steps, as bench.py), then the kind's default map (frontier_device.default_spec: the world
grid of the visibility map, towards the edge, unknown cells blocked, all seven outputs) is timed at 16 x 16, 32 x 32 and 64 x 64 cells
with HIP events on three memories:

  full   every cell seen.  Towards the kind's field sources instead of the edge, so the relaxation's work is that of `env.field()` and the
         difference is the cost of reading the memory, the second classification pass and the summary: `over_field`.
  look   one call of `env.see()` (the default map with 4 m of range: WALL | BOX occlude, all round) on an empty memory.
  half   that look and the left half of the grid.

Two yardsticks are timed IN THE SAME PROCESS AND INTERLEAVED, window by window (tools/see_rate.py: interleaved): `env.field()` and
`env.see()` with the memory, on the same grids.  `edges` is the mean number of edge cells per env, `reached` the share of envs with a
finite `length`.  The kernel's VGPR / LDS / scratch figures come from the compiler (`python -m hrl_pybullet_envs_amd.build --force` prints
its resource remarks)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hrl_pybullet_envs_amd as envs  # noqa: E402
from hrl_pybullet_envs_amd import field_device as F  # noqa: E402
from hrl_pybullet_envs_amd import frontier_device as X  # noqa: E402
from hrl_pybullet_envs_amd import see_device as V  # noqa: E402
from tools.field_rate import LAUNCHES, SIZES  # noqa: E402
from tools.scan_rate import IDS, WINDOWS  # noqa: E402
from tools.see_rate import interleaved  # noqa: E402


def measure(kind='gather', n=4096):
    env = envs.make(IDS[kind], num_envs=n, seed=0)
    env.reset()
    be = env._backend()
    for _ in range(300):
        env.step(torch.rand(n, be.act_dim, device='cuda') * 2 - 1)
    rows = []
    common = {'kind': kind, 'envs': n, 'windows': WINDOWS, 'launches': LAUNCHES, 'device': torch.cuda.get_device_name(0)}
    for size in SIZES:
        sspec = V.default_spec(be.cfg, 'world', size, size)
        fspec = F.default_spec(be.cfg, 'world', size, size)
        spec = X.spec_like(be.cfg, sspec)
        as_field = X.spec_like(be.cfg, sspec, sources=fspec.sources)
        look = V.memory(n, sspec, 'cuda')
        be.see(V.default_spec(be.cfg, 'world', size, size, max_range=4.0), out=V.See(None, look, None))
        half = look.clone()
        half[:, :, :size // 2] = 1
        full = torch.ones_like(look)
        out = X.Frontier(*(torch.empty((n,) + shape, dtype=dt, device='cuda') for shape, (_, dt) in zip(X.shapes(spec), X.FIELDS)))
        fout = F.Field(*(torch.empty(n, size, size, dtype=dt, device='cuda') for _, dt in F.FIELDS))
        sout = V.See(torch.empty(n, size, size, dtype=torch.uint8, device='cuda'), V.memory(n, sspec, 'cuda'), torch.empty(n, dtype=torch.int32, device='cuda'))
        stats = {}
        for name, mem, sp in (('full', full, as_field), ('look', look, spec), ('half', half, spec)):
            be.frontier(mem, sp, out=out)
            stats[name] = (round(float(out.count.float().mean()), 1), round(float(torch.isfinite(out.length).float().mean()), 4))
        t = interleaved({'full': lambda: be.frontier(full, as_field, out=out), 'look': lambda: be.frontier(look, spec, out=out), 'half': lambda: be.frontier(half, spec, out=out),
                         'field': lambda: be.field(fspec, out=fout), 'see': lambda: be.see(sspec, out=sout)})
        for what in ('field', 'see'):
            rows.append(dict(common, what=what, cells=f'{size}x{size}', us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2]))
        for what in ('full', 'look', 'half'):
            rows.append(dict(common, what='frontier', memory=what, cells=f'{size}x{size}', us_per_call=t[what][0], us_min=t[what][1], us_max=t[what][2],
                             over_field=round(t[what][0] / t['field'][0], 2), over_see=round(t[what][0] / t['see'][0], 2), edges=stats[what][0], reached=stats[what][1]))
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
        sys.exit('frontier_rate.py needs the GPU: a time taken elsewhere says nothing')
    for kind in kinds:
        for r in measure(kind, n):
            if r['what'] == 'frontier':
                what = f"{r['cells']} cells, frontier (memory: {r['memory']}): {r['over_field']} x the field, {r['over_see']} x see, {r['edges']} edge cells, {100 * r['reached']:.1f} % reached"
            else:
                what = f"{r['cells']} cells, {r['what']}"
            print(f"{IDS[kind]} x {n}, {what}: {r['us_per_call']} us (windows {r['us_min']} .. {r['us_max']})")
            print(json.dumps(r))
            if json_file:
                with open(json_file, 'a') as f:
                    f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
