"""The batched visibility map's specification (csrc/see_core.h) on the CPU: its host build (tests/see_host) against an independent fp64
reference written from include/hrl_see.h alone (tests/see_cases.py), the tie to the host probe's `blocker`, known answers in the maze,
the memory, exact monotonicity, totality on hostile states, spec validation, the sanitised stand-alone program and the gfx950
cross-compile.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_cases as fc
import orc
import probe_cases as pc
import see_cases as vc
import sensor_configs as scfg
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import probe_device as P
from hrl_pybullet_envs_amd import scan_device as S
from hrl_pybullet_envs_amd import see_device as V
from test_field_host import maze_env
from test_render_host import shard   # the oracle's shards of 5 envs after reset + 30 random steps: computed once, read-only

N = 5
EXEMPT_CAP = 0.01   # of the cells of a (kind, spec): asserted on the reference alone


def states_of(cfg, state):
    return (('shard', state), ('hand-made', vc.hand_made(cfg, state)), ('spread', vc.spread(cfg, state)))


@pytest.mark.parametrize('kind', vc.KINDS)
def test_host_build_equals_the_fp64_reference(kind):
    """Six kinds x three modes x 8 x 8, 24 x 40, 64 x 8 and 64 x 64 cells x the three specs of see_cases.sweep_specs (everything occludes /
    all round / any range / a slack of one cell, or of the 2 m the header allows where a cell is wider: the maze's 8 x 8 world grid; WALL | BOX / fov_cos 0.5 / 6 m / no slack; nothing occludes / fov_cos 0 / 3 m) on the
    shard's states, the hand-made poses and the robots spread about the arena.  A cell is exempt where the reference's verdict changes
    when its centre moves by +-1e-4 m along x or y; at most 1 % of the cells of a (kind, spec) may be, asserted on the reference alone
    before the build is looked at.  Every other cell equals the reference exactly.

    Measured share of exempt cells over this sweep (253 440 cells per (kind, spec)): at most 0.005 % (13 cells: the maze kind under the
    first spec; 12 and 9 in the gather kinds under it), at most 5 cells under the second spec, at most 1 under the third."""
    cfg, state, items, aux = shard(kind)
    for k in range(3):
        specs = [vc.sweep_specs(size, mode, kind)[k] for mode in vc.MODES for size in vc.SIZES]
        seen_cells, cells = compare_with_the_reference(cfg, state, items, aux, specs, f'kind {kind} spec {k}')
        assert 0 < seen_cells and (seen_cells < cells or k == 0), (kind, k)   # both verdicts occur (an arena with nothing in it hides nothing all round)


def compare_with_the_reference(cfg, state, items, aux, specs, tag):
    """The comparison of test_host_build_equals_the_fp64_reference of one group of specs (the cap of exempt cells is the group's) on the
    given states, their hand-made poses and with the robots spread about the arena; returns (the cells the reference sees, all cells)."""
    runs = []
    exempt_cells = cells = seen_cells = 0
    for spec in specs:
        for label, st in states_of(cfg, state):
            refs = [vc.stable_reference(cfg, st[e], None if items is None else items[e], aux[e], spec) for e in range(N)]
            exempt_cells += sum(int(x.sum()) for _, x in refs)
            cells += N * spec.width * spec.height
            runs.append((label, spec, st, refs))
    share = exempt_cells / cells
    print(f'{tag}: {exempt_cells} of {cells} cells exempt ({100 * share:.3f} %)')
    assert share <= EXEMPT_CAP, (tag, share)   # on the reference alone
    for label, spec, st, refs in runs:
        got = vc.see_host(cfg, st, items, aux, spec).visible
        assert got.dtype == np.uint8 and got.max() <= 1
        for e, (ref, exempt) in enumerate(refs):
            wrong = (got[e].astype(bool) != ref) & ~exempt
            assert not wrong.any(), (tag, spec.mode, (spec.width, spec.height), label, e, np.argwhere(wrong)[:5].tolist())
            seen_cells += int(ref.sum())
    return seen_cells, cells


@pytest.mark.parametrize('name', scfg.NAMES)
def test_host_build_equals_the_fp64_reference_on_the_sensor_config_matrix(name):
    """The comparison above, with its cap of 1 % exempt cells per spec, on every entry of sensor_configs.MATRIX: everything occludes on a
    24 x 40 grid in the heading mode with a slack of one cell, walls and the box occlude a field of view of 120 degrees out to 6 m on a
    24 x 40 world grid about the entry's own arena, and the library's default spec, whose extent is derived from the config (flagrun's
    open field has no walls: nothing is hidden there).  On the entry's hostile states the map equals that of the clean twin and a
    robot without a finite place sees nothing."""
    cfg, state, items, aux = scfg.shard(name)
    specs = [vc.sweep_specs((24, 40), V.HRL_VIEW_EGO_HEADING, cfg)[0], vc.sweep_specs((24, 40), V.HRL_VIEW_WORLD, cfg)[1], V.default_spec(cfg)]
    for k, spec in enumerate(specs):
        seen_cells, cells = compare_with_the_reference(cfg, state, items, aux, [spec], f'{name} spec {k}')
        assert 0 < seen_cells and (seen_cells < cells or k != 1), (name, k)   # a field of view hides something in every arena
    for spec in specs[:2]:
        spec = spec.copy()
        spec.occluders, spec.slack = V.ALL, 0.1
        for s, it, a, cs, cit, ca, far, blind in scfg.hostile(name, fc.hostile):
            got = vc.see_host(cfg, s, it, a, spec).visible
            want = vc.see_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec).visible
            rows = [e for e in range(N) if e not in blind]
            assert np.array_equal(got[rows], want[rows]), (name, spec.mode)
            assert (got[list(blind)] == 0).all() and want.any()


@pytest.mark.parametrize('kind', vc.KINDS)
def test_visible_is_the_probes_blocker_bit_for_bit(kind):
    """Slack 0, all round, max_range 3e38: at the cell centres the host library exports (in the table's frame), visible == (the host
    probe's blocker == 0) with frame = HRL_PROBE_EGO and classes = occluders, on every cell of 24 x 40 grids in the three modes."""
    cfg, state, items, aux = shard(kind)
    cells = 24 * 40
    for mode in vc.MODES:
        for occluders in (V.ALL, V.WALL | V.BOX):
            for label, st in states_of(cfg, state):
                spec = vc.spec_of((24, 40), mode, occluders, kind=kind, centre=fc.WORLD_CENTRE)
                centres = np.full((N, 40, 24, 2), np.nan, np.float32)
                vis = vc.see_host(cfg, st, items, aux, spec, centres=centres).visible
                assert np.isfinite(centres).all()
                blocker = np.zeros((N, cells), np.int32)
                for lo in range(0, cells, 480):   # the probe takes at most 512 points
                    pts = np.ascontiguousarray(centres.reshape(N, cells, 2)[:, lo:lo + 480])
                    blocker[:, lo:lo + 480] = pc.probe_host(cfg, st, items, aux, pc.spec_of(480, P.HRL_PROBE_EGO, 0.0, occluders), pts, want=('blocker',)).blocker
                assert np.array_equal(vis.reshape(N, cells), (blocker == 0).astype(np.uint8)), (kind, mode, occluders, label)
                if mode != V.HRL_VIEW_WORLD:   # ... and the exported centres are where the renderer's pixels are, seen from the robot
                    pos = fc.centres(st[0], spec)[0] - np.array(st[0, 0:2], float)
                    assert np.abs(centres[0] - pos).max() <= 1e-5


def maze_start():
    cfg, st, aux = maze_env(((-2.0, -5.0),))
    return cfg, st, aux


def test_known_answers_in_the_maze():
    """The box spans x in [-5, 1] and y in [-2, 2]; the robot stands at the start (-2, -5) with identity heading (forward = +x);
    WALL | BOX occlude; a 64 x 64 world grid of half extent 9 (cells of 0.28125 m, no centre on the line x = -2).  At slack 0 the cells
    holding the evaluation target (-2, 4) and (3, 3) are hidden behind the box, those holding (4, 0) and (-2, -3) are visible, a cell
    inside the box and one beyond the +x wall are hidden.  With a slack of one cell the box's first row of cells behind its y = -2 face
    is visible (and was not at slack 0).  With fov_cos = 0 the cells with x < -3 are hidden."""
    cfg, st, aux = maze_start()
    spec = vc.spec_of((64, 64), V.HRL_VIEW_WORLD, V.WALL | V.BOX, half=9.0)
    vis = vc.see_host(cfg, st, None, aux, spec).visible[0]
    at = lambda x, y: vis[vc.cell_of(spec, x, y)]
    assert at(-2.0, 4.0) == 0 and at(3.0, 3.0) == 0
    assert at(4.0, 0.0) == 1 and at(-2.0, -3.0) == 1
    assert at(-2.0, 0.0) == 0 and at(-4.0, 1.0) == 0   # inside the box
    assert at(6.0, -5.0) == 0 and at(4.0, -5.0) == 1   # beyond the +x wall (its plane is at 4.95) and before it
    pos = fc.centres(st[0], spec)[0]
    row = vc.cell_of(spec, 0.0, -1.9)[0]
    assert -2.0 < pos[row, 0, 1] < -2.0 + 0.28125 and pos[row + 1, 0, 1] < -2.0   # the first row of cell centres inside the box
    cols = (pos[row, :, 0] > -4.9) & (pos[row, :, 0] < 1.0)
    assert cols.sum() == 21 and (vis[row][cols] == 0).all()
    lit = vc.see_host(cfg, st, None, aux, vc.spec_of((64, 64), V.HRL_VIEW_WORLD, V.WALL | V.BOX, slack=None, half=9.0)).visible[0]
    assert (lit[row][cols] == 1).all() and (lit[row - 2][cols] == 0).all()   # the face is lit, the box's inside is not
    assert (lit >= vis).all()
    ahead = vc.see_host(cfg, st, None, aux, vc.spec_of((64, 64), V.HRL_VIEW_WORLD, V.WALL | V.BOX, fov_cos=0.0, half=9.0)).visible[0]
    assert (ahead[pos[..., 0] < -3.0] == 0).all() and (vis[pos[..., 0] < -3.0] == 1).any()
    assert ahead[vc.cell_of(spec, 4.0, 0.0)] == 1 and (ahead <= vis).all()


def test_memory():
    """Two robot places A then B: seen == vis_A | vis_B and fresh_B == count(vis_B & ~vis_A).  clear: seen == vis_B and fresh ==
    count(vis_B).  Bytes of 0x7B found in `seen` count as seen and come back as 1.  A masked env keeps its bytes and its fresh.  visible
    may be NULL.  merge4 equals the rule byte by byte on arbitrary words."""
    cfg, st, aux = maze_env(((-2.0, -5.0), (3.0, 6.0), (4.0, -8.0)))
    a, b = st, st.copy()
    b[:, 0:2] = ((3.0, -3.0), (-4.0, 6.0), (4.0, 8.0))
    spec = vc.spec_of((64, 64), V.HRL_VIEW_WORLD, V.WALL | V.BOX, slack=None, half=9.0)
    va, vb = (vc.see_host(cfg, s, None, aux, spec).visible for s in (a, b))
    assert (va != vb).any() and va.any() and vb.any()
    out = vc.See(np.zeros((3, 64, 64), np.uint8), np.zeros((3, 64, 64), np.uint8), np.full(3, -7, np.int32))
    vc.see_host(cfg, a, None, aux, spec, out=out)
    assert np.array_equal(out.visible, va) and np.array_equal(out.seen, va) and out.fresh.tolist() == va.reshape(3, -1).sum(1).tolist()
    vc.see_host(cfg, b, None, aux, spec, out=out)
    assert np.array_equal(out.visible, vb) and np.array_equal(out.seen, va | vb)
    assert out.fresh.tolist() == (vb & ~va & 1).reshape(3, -1).sum(1).tolist() and (out.fresh > 0).all()
    vc.see_host(cfg, b, None, aux, spec, out=out)
    assert np.array_equal(out.seen, va | vb) and (out.fresh == 0).all()   # nothing new the second time
    vc.see_host(cfg, b, None, aux, spec, clear=np.array([1, 0, 9], np.uint8), out=out)
    assert np.array_equal(out.seen[[0, 2]], vb[[0, 2]]) and np.array_equal(out.seen[1], (va | vb)[1])
    assert out.fresh.tolist() == [int(vb[0].sum()), 0, int(vb[2].sum())]
    # bytes of 0x7B found in the memory count as seen and come back as 1; only the memory is asked for
    dirty = np.zeros((3, 64, 64), np.uint8)
    dirty[:, ::3, 1::2] = 0x7B
    mem = vc.See(None, dirty.copy(), np.zeros(3, np.int32))
    vc.see_host(cfg, a, None, aux, spec, out=mem)
    assert np.array_equal(mem.seen, ((dirty != 0) | (va != 0)).astype(np.uint8))
    assert mem.fresh.tolist() == ((va != 0) & (dirty == 0)).reshape(3, -1).sum(1).tolist()
    # a masked env keeps every byte
    kept = vc.See(np.full((3, 64, 64), 0x55, np.uint8), dirty.copy(), np.full(3, -7, np.int32))
    vc.see_host(cfg, a, None, aux, spec, clear=np.ones(3, np.uint8), mask=np.array([1, 0, 1], np.uint8), out=kept)
    assert (kept.visible[1] == 0x55).all() and np.array_equal(kept.seen[1], dirty[1]) and kept.fresh[1] == -7
    assert np.array_equal(kept.visible[[0, 2]], va[[0, 2]]) and np.array_equal(kept.seen[[0, 2]], va[[0, 2]]) and kept.fresh[0] == va[0].sum()
    rng = np.random.RandomState(4)
    for found in list(rng.randint(0, 2 ** 32, 300, np.uint64)) + [0, 0xffffffff, 0x80808080, 0x7f7f7f7f, 0x01000100, 0x00800001]:
        v4 = int(rng.randint(0, 16))
        v4 = sum(((v4 >> i) & 1) << (8 * i) for i in range(4))
        n = C.c_int(-1)
        now = vc.lib().see_merge4(v4, int(found), C.byref(n))
        fb, vb4 = [(int(found) >> (8 * i)) & 255 for i in range(4)], [(v4 >> (8 * i)) & 1 for i in range(4)]
        assert now == sum((1 if f or v else 0) << (8 * i) for i, (f, v) in enumerate(zip(fb, vb4))) and n.value == sum(1 for f, v in zip(fb, vb4) if v and not f)


@pytest.mark.parametrize('kind', vc.KINDS)
def test_exact_monotonicity_in_fp32(kind):
    """Fewer occluder classes, a larger slack, a larger range and a smaller fov_cos each never hide a cell: exactly, cell by cell, in the
    host build's fp32."""
    cfg, state, items, aux = shard(kind)
    for mode in vc.MODES:
        for label, st in states_of(cfg, state)[::2]:
            base = dict(kind=kind, centre=fc.WORLD_CENTRE)
            see = lambda **kw: vc.see_host(cfg, st, items, aux, vc.spec_of((24, 40), mode, **dict(base, **kw))).visible
            chains = ([see(occluders=o, slack=0.1) for o in (V.ALL, V.WALL | V.BOX | V.POISON, V.WALL | V.BOX, V.BOX, 0)],
                      [see(occluders=V.ALL, slack=s) for s in (0.0, 0.05, 0.3, 1.0, 2.0)],
                      [see(occluders=V.ALL, max_range=r) for r in (0.5, 2.0, 2.5, 6.0, 30.0, vc.HUGE)],
                      [see(occluders=V.ALL, fov_cos=c) for c in (1.0, 0.9, 0.5, 0.0, -0.5, -0.999, -1.0)])
            for chain in chains:
                for lo, hi in zip(chain, chain[1:]):
                    assert (hi >= lo).all(), (kind, mode, label)
            assert all((chain[-1] > chain[0]).any() for chain in chains[2:]), (kind, mode, label)   # (range and field of view matter in every arena)


@pytest.mark.parametrize('kind', vc.KINDS)
def test_hostile_states_get_the_contract(kind):
    """NaN and +-inf in the robot's position, an item or the flagrun goal, and target indices out of range (field_cases.hostile): a robot
    without a finite place sees nothing, in every mode, and adds nothing to the memory; a shape with a non-finite parameter does not
    occlude -- the map equals, bit for bit, that of the clean twin without the shape."""
    cfg, state, items, aux = shard(kind)
    for mode in vc.MODES:
        for size in ((24, 40), (64, 64)):
            spec = vc.spec_of(size, mode, V.ALL, slack=0.1, kind=kind)
            for s, it, a, cs, cit, ca, far, blind in fc.hostile(cfg, state, items, aux):
                got = vc.see_host(cfg, s, it, a, spec).visible
                want = vc.see_host(fc.far_targets(cfg) if far else cfg, cs, cit, ca, spec).visible
                rows = [e for e in range(N) if e not in blind]
                assert np.array_equal(got[rows], want[rows]), (kind, mode, size)
                assert (got[list(blind)] == 0).all() and want.any()
                if mode == V.HRL_VIEW_WORLD and blind:
                    mem = vc.See(None, np.zeros((N,) + size[::-1], np.uint8), np.full(N, -7, np.int32))
                    vc.see_host(cfg, s, it, a, spec, out=mem)
                    assert (mem.seen[list(blind)] == 0).all() and (mem.fresh[list(blind)] == 0).all() and np.array_equal(mem.seen[rows], want[rows])


BAD = [('width', 0), ('width', 12), ('width', 72), ('height', 4), ('height', 72), ('mode', 3), ('mode', -1), ('half_extent', 0.0), ('half_extent', float('inf')),
       ('half_extent', float('nan')), ('occluders', 32), ('occluders', 64 | 1), ('max_range', 0.0), ('max_range', -1.0), ('max_range', float('inf')), ('max_range', float('nan')),
       ('fov_cos', 1.5), ('fov_cos', -1.5), ('fov_cos', float('nan')), ('slack', -0.1), ('slack', 2.5), ('slack', float('nan')), ('struct_size', 16), ('struct_size', 0),
       ('out', 'empty'), ('out', 'seen in ego'), ('out', 'fresh alone'), ('out', 'aliased')]
REASONS = {'width': 'width must be a multiple of 8', 'height': 'height must be a multiple of 8', 'mode': 'unknown see mode', 'half_extent': 'half_extent must be finite',
           'occluders': 'occluders must be a mask of', 'max_range': 'max_range must be finite and positive', 'fov_cos': 'fov_cos must be within -1..1',
           'slack': 'slack must be finite and within 0..2', 'struct_size': 'struct_size is not sizeof', 'empty': 'holds no pointer', 'seen in ego': 'seen needs HRL_VIEW_WORLD',
           'fresh alone': 'fresh needs seen', 'aliased': 'must not be the same pointer'}


@pytest.mark.parametrize('field,value', BAD)
def test_bad_specs_are_refused_with_a_reason(field, value):
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = vc.spec_of((24, 40), V.HRL_VIEW_EGO if value == 'seen in ego' else V.HRL_VIEW_WORLD, kind=K.HRL_ANT_FLAT)
    out = vc.See(np.full((N, 64, 64), 0x7B, np.uint8), np.full((N, 64, 64), 0x7B, np.uint8), np.full(N, -7, np.int32))
    handed = out
    if field == 'out':
        handed = {'empty': vc.See(None, None, None), 'seen in ego': out, 'fresh alone': out._replace(seen=None), 'aliased': out._replace(seen=out.visible)}[value]
    else:
        setattr(spec, field, value)
    b = K.make_buffers(vc.ptr(state), vc.ptr(items), vc.ptr(aux), None, None, None, None, None)
    o = V.hrl_see_out(**{name: vc.ptr(a) for name, a in zip(vc.NAMES, handed)})
    code = vc.lib().see_host(C.byref(cfg), C.byref(b), C.byref(spec), None, None, C.byref(o), None)
    why = vc.lib().see_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and REASONS[value if field == 'out' else field] in why, why
    assert (out.visible == 0x7B).all() and (out.seen == 0x7B).all() and (out.fresh == -7).all()
    # the device library runs the same checks before it looks for a device
    L = V.lib()
    assert L.hrl_see(C.byref(cfg), C.byref(b), C.byref(spec), None, None, C.byref(o), None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_see_last_error() == b'hrl_see: ' + why.encode()
    assert (out.visible == 0x7B).all() and (out.seen == 0x7B).all() and (out.fresh == -7).all()


def test_default_spec_and_the_mirrors():
    for kind in vc.KINDS:
        cfg = orc.default_config(kind, num_envs=1)
        for name, mode in V.MODES.items():
            s, h, f, r = V.default_spec(cfg, name), V.hrl_see_spec(), F.default_spec(cfg, name), S.default_spec(cfg)
            assert vc.lib().see_host_default_spec(C.byref(cfg), mode, C.byref(h)) == 0 and bytes(s) == bytes(h)
            assert (s.width, s.height, s.mode, s.centre[0], s.centre[1], s.half_extent) == (f.width, f.height, f.mode, f.centre[0], f.centre[1], f.half_extent)
            assert (s.struct_size, s.occluders, s.max_range, s.fov_cos) == (C.sizeof(V.hrl_see_spec), V.WALL | V.BOX, r.max_range, -1.0)
            assert s.slack == np.float32(2.0 / 64) * np.float32(s.half_extent) == np.float32(F.cell_size(f))
            assert vc.lib().see_validate_spec(C.byref(s)) == b''
    s = V.default_spec(cfg, 'ego', 24, 40, fov_degrees=120, max_range=6.0)
    assert (s.width, s.height, s.mode, s.max_range) == (24, 40, 1, 6.0) and abs(s.fov_cos - 0.5) < 1e-6
    assert s.slack == np.float32(np.float32(2.0) / np.float32(24)) * np.float32(s.half_extent)   # one cell of the resized grid, as the library computes it
    assert V.default_spec(cfg, 'world', 64, 32).half_extent == 2 * V.default_spec(cfg).half_extent
    assert V.default_spec(cfg, slack=0.0).slack == 0.0 and V.default_spec(cfg, fov_degrees=360).fov_cos == -1.0
    with pytest.raises(ValueError):
        V.default_spec(cfg, 'sideways')
    assert vc.lib().see_sizeof_spec() == C.sizeof(V.hrl_see_spec) == 48 and vc.lib().see_sizeof_out() == C.sizeof(V.hrl_see_out) == 24
    assert V.See() == (None,) * 3 and V.See._fields == vc.NAMES
    m = V.memory(3, s, 'cpu')
    assert m.shape == (3, 40, 24) and m.dtype.is_floating_point is False and int(m.sum()) == 0


def test_sanitised_program_runs_clean_and_agrees_with_the_plain_build():
    """see_check_main (address + undefined-behaviour sanitisers, a program of its own) computes the maps of every kind in the three modes
    from reset-like and hostile states, with the memory in the world mode: exit status 0, sizeof(hrl_see_spec) == the ctypes mirror's,
    checksums == the unsanitised host build's."""
    p = subprocess.run([vc.check_program()], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split('\n')
    assert lines[0] == f'sizeof_hrl_see_spec {C.sizeof(V.hrl_see_spec)}'
    sums = dict(l.split()[1:3] for l in lines if l.startswith('case '))
    n = vc.lib().see_check_n_cases()
    assert n == len(sums) == 6 * 3 * 7
    for k in range(n):
        name, s = C.create_string_buffer(64), C.c_ulonglong()
        assert vc.lib().see_check_case(k, name, C.byref(s)) == 0
        assert sums[name.value.decode()] == '%016x' % s.value, name.value
    assert len(set(sums.values())) > n // 2   # the cases are different maps


def test_see_library_cross_compiles_for_gfx950_without_scratch():
    """build.py makes libhrl_see_hip.so with hipcc --offload-arch=gfx950; the compiler's resource remarks report no scratch and no spills
    for the kernel and an LDS footprint of at most 16 KB; the header's symbols are SYMBOLS; the map is an entry of build.py of its own,
    built by build() after the routes."""
    code = 'from hrl_pybullet_envs_amd.build import build_see, HIPCC_FLAGS; assert "--offload-arch=gfx950" in HIPCC_FLAGS; print(build_see(force=True, verbose=True))'
    p = subprocess.run([sys.executable, '-c', code], cwd=vc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert os.path.exists(os.path.join(vc.ROOT, 'hrl_pybullet_envs_amd', 'libhrl_see_hip.so'))
    text = p.stdout
    kernels = re.findall(r'Function Name: (\S*see_kernel\S*)', text)
    assert len(kernels) == 1
    block = text[text.index(kernels[0]):]
    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1)) == 0
    assert int(re.search(r'VGPRs Spill: (\d+)', block).group(1)) == 0 and int(re.search(r'SGPRs Spill: (\d+)', block).group(1)) == 0
    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', block).group(1)) <= 16384
    hdr = open(os.path.join(vc.ROOT, 'include', 'hrl_see.h')).read()
    assert set(re.findall(r'\b(hrl_see(?:_[a-z_]+)?)\s*\(', hdr)) - {'hrl_see_out', 'hrl_see_spec'} == set(V.SYMBOLS)
    for s in V.SYMBOLS:
        assert hasattr(V.lib(), s)
    from hrl_pybullet_envs_amd import build
    assert build.SEE == ('see', 'libhrl_see_hip.so', 'see_hip.hip', 'see_core.h', 'hrl_see.h') and 'see' not in [name for name, *_ in build.SENSORS]
    src = open(build.__file__).read()
    assert src.index('build_route(force, verbose)\n    build_see(force, verbose)') > 0
