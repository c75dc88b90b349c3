"""The step's optional contact report (hrl_buffers_ext.contacts) on the CPU: the report phase of csrc/step_core.h (write_contacts) run by the
lock-step host executor, against the oracle's own account of the step's last substep -- bit for bit where the oracle speaks (counts, surfaces,
every impulse), against the fp64 textbook reference where only it speaks (distances, the point bot's impulses) -- and the invariants a
record must satisfy.  Scenarios, the emulator build and the oracle replay: tests/contacts_cases.py."""
import ctypes as C

import numpy as np
import pytest

import contacts_cases as cc
import textbook as tb
from hrl_pybullet_envs_amd import _capi as K

ANT = ('random', 'items', 'walls', 'box', 'self')


def surf_class(s, link2=-1):
    if link2 >= 0:
        return 'self'
    return 'ground' if s == 0 else ('wall' if s < K.HRL_SURF_BOX else ('box' if s < K.HRL_SURF_ITEM else 'item'))


def oracle_classes(tr):
    """Env-steps of the ORACLE's replay per class (the coverage floors are conditions on the reference alone)."""
    n = dict(item=0, cap=0, wall=0, box=0, self_pushing=0, done=0, limits=0)
    for s in tr.steps:
        for i, rp in enumerate(s['replay']):
            sf, nL = rp['surf'], rp['n_limits']
            n['item'] += bool(((sf >= 16) & (sf < 64)).any()); n['cap'] += rp['n_contacts'] == cc.MAXC
            n['wall'] += bool(((sf >= 1) & (sf < 8)).any()); n['box'] += bool(((sf >= 8) & (sf < 16)).any())
            n['self_pushing'] += any(sf[k] >= 64 and rp['lam'][nL + k] > 0 for k in range(rp['n_contacts']))
            n['done'] += int(s['done'][i]); n['limits'] += nL > 0
    return n


@pytest.mark.parametrize('name', ANT)
def test_ant_records_equal_the_oracle_bit_for_bit(name):
    """Counts, every surface code, lambda_n / lambda_t1 / lambda_t2 of every contact and the limit impulses (rebuilt from the masks, ascending
    joint order) of every env-step == `orc_ant_substeps_items_f32` on the step's inputs, bitwise; envs whose episode ended in the step are
    compared like the others (the record is the terminal step's, written before the reset).  Forward and reverse lane order give the same
    records.  The replay itself is checked first: it reproduces the stepped state of every env that was not reset."""
    tr, rec, rev = cc.trace(name), cc.emu_records(name), cc.emu_records(name, reverse=True)
    assert not np.isnan(rec).any()  # the buffer started as NaN: every float of every record is written in every step
    assert np.array_equal(cc.bits(rec), cc.bits(rev)), 'lane-order dependence'
    for t, s in enumerate(tr.steps):
        for i, rp in enumerate(s['replay']):
            if not s['done'][i]:
                after = s['after'][i]
                assert np.array_equal(cc.bits(rp['q']), cc.bits(after[:15])), (t, i, 'the replay is not the step')
            cc.check_against_oracle(rec[t, i], rp, (name, t, i))
    n = oracle_classes(tr)
    print(name, n)
    floors = {'random': n['limits'] >= 1, 'items': n['item'] >= 1 and n['cap'] >= 1, 'walls': n['wall'] >= 1, 'box': n['box'] >= 1 and n['done'] >= 1,
              'self': n['self_pushing'] >= 1}
    assert floors[name], (name, n)


def item_box(items, k):
    return np.r_[items[2 * k] - 0.125, items[2 * k + 1] - 0.125, -0.025], np.r_[items[2 * k] + 0.125, items[2 * k + 1] + 0.125, 0.225]


def check_invariants(cfg, rec, items, where):
    f = np.float32
    nC, nL = int(rec[0]), int(rec[1])
    assert rec[0] == nC and rec[1] == nL and 0 <= nC <= cc.MAXC and 0 <= nL <= 8, where
    assert rec[2] == nL + 3 * nC and cc.bits(rec[3:4])[0] == cc.bits(np.array([cfg.model.timestep], f))[0], where
    assert not cc.bits(rec[14:16]).any() and not cc.bits(rec[cc.HEAD + cc.WIDTH * nC:]).any(), (where, 'stale tail')  # +0.0 bitwise
    held, neg = int(rec[12]), int(rec[13])
    assert bin(held).count('1') == nL and neg & ~held == 0, where
    for j in range(8):
        if not (held >> j) & 1:
            assert cc.bits(rec[4 + j:5 + j])[0] == 0, where
        else:  # a limit row pushes the joint back into its range: lambda >= 0, signed by the side
            assert rec[4 + j] * (-1 if (neg >> j) & 1 else 1) >= 0, where
    for i in range(nC):
        c = cc.contact(rec, i).astype(np.float64)
        n, t1, t2 = c[4:7], c[8:11], c[12:15]
        for v in (n, t1, t2):
            assert abs(np.linalg.norm(v) - 1) <= 1e-6, (where, i, v)
        assert abs(n @ t1) <= 1e-6 and abs(n @ t2) <= 1e-6 and abs(t1 @ t2) <= 1e-6, (where, i)
        lam_n, mu = c[7], c[19]
        bound = cc.contact(rec, i)[19] * cc.contact(rec, i)[7]  # the solver's own clamp: the fp32 product mu * lambda_n
        assert lam_n >= 0 and abs(c[11]) <= bound and abs(c[15]) <= bound and mu > 0, (where, i, c)
        kind = surf_class(int(c[16]), int(c[18]))
        if kind == 'ground':
            assert np.array_equal(c[4:7], [0, 0, 1]) and abs(c[2] - f(cfg.model.ground_z) - c[3]) <= 1e-5, (where, i, c)
        if kind == 'item' and c[3] > 0:
            k = int(c[16]) - K.HRL_SURF_ITEM
            lo, hi = item_box(items, k)
            gap = np.linalg.norm(c[0:3] - np.clip(c[0:3], lo, hi))
            assert gap <= c[3] + 1e-5, (where, i, k, gap, c[3])
        if cfg.env_kind == K.HRL_POINT_GATHER:
            assert c[17] == 0 and c[18] == -1, where
        else:
            assert 0 <= int(c[17]) < 16 and (int(c[17]) & 3) < 3 and (c[18] == -1 or kind == 'self'), where


@pytest.mark.parametrize('name', cc.NAMES)
def test_record_invariants(name):
    """What a record must satisfy whatever the step was: no stale tail (+0.0 bitwise beyond the contacts and in the spare header floats), h,
    n_rows = n_limit_rows + 3 n_contacts, an orthonormal frame per contact (1e-6: a few fp32 roundings on unit vectors), ground contacts with
    the normal (0, 0, 1) exactly and position consistent with the distance (1e-5: roundings of numbers below 2 m), lambda_n >= 0 and
    |lambda_t| <= mu lambda_n with the contact's own mu, item contacts within `dist` of the item's box."""
    tr, rec = cc.trace(name), cc.emu_records(name)
    seen = 0
    for t, s in enumerate(tr.steps):
        for i in range(tr.cfg.num_envs):
            check_invariants(tr.cfg, rec[t, i], s['items'][i], (name, t, i))
            seen += int(rec[t, i, 0])
    assert seen > 0, name


def tb_code(s, cfg):
    """textbook_ref.c's surface code (0 ground, 1.. planes, 100 + k box k, 200 + pair) as the record's."""
    if s < 100:
        return s
    if s >= 200:
        return K.HRL_SURF_SELF + (s - 200)
    return K.HRL_SURF_BOX + (s - 100) if cfg.env_kind in (K.HRL_ANT_MAZE, K.HRL_ANT_MAZE_MJ) else K.HRL_SURF_ITEM + (s - 100)


def textbook_step(tr, s, i):
    cfg = tr.cfg
    q, u, tau = cc.pre_step(cfg, s['state'][i], s['act'][i])
    ni = cc.n_items(cfg)
    p = tb.params(cfg, items=s['items'][i, :2 * ni].astype(np.float64) if ni else None)
    f = tb.point_substep if cfg.env_kind == K.HRL_POINT_GATHER else tb.ant_substep
    return f(p, q.astype(np.float64), u.astype(np.float64), tau.astype(np.float64))[2]


DIST_MEASURED = 4.6e-7   # largest |fp32 emulator - fp64 textbook| distance over the scenarios below, metres
DIST_TOL = 4 * DIST_MEASURED


def test_distances_against_the_fp64_textbook_reference():
    """Scenarios (a)-(d) at one substep per step (the textbook reference steps one substep): where the record's surface list equals
    `textbook.ant_substep`'s -- it must on >= 90 % of the env-steps; measured: 480 of 480 in each of the four -- every contact's distance is
    the fp64 one within 4 x the largest difference measured over these scenarios: 4.6e-7 m measured (items 7.8e-8, walls 4.5e-7, box 1.9e-7;
    the free-falling random run meets no surface in its 30 substeps), so 1.84e-6 m, far under the ceiling of 1e-4 m; a mixed-up contact is
    off by the scale of contact_dist = 0.02 m."""
    assert DIST_TOL <= 1e-4
    worst, compared = 0.0, 0
    for name in ('random', 'items', 'walls', 'box'):
        tr, rec = cc.trace(name, frame_skip=1), cc.emu_records(name, frame_skip=1)
        agree = total = 0
        for t, s in enumerate(tr.steps):
            for i in range(tr.cfg.num_envs):
                out, r = textbook_step(tr, s, i), rec[t, i]
                n = int(r[0])
                total += 1
                if [int(cc.contact(r, k)[16]) for k in range(n)] != [tb_code(out.contact_surface[k], tr.cfg) for k in range(out.n_contacts)]:
                    continue
                agree += 1
                for k in range(n):
                    err = abs(float(cc.contact(r, k)[3]) - out.contact_dist[k])
                    worst = max(worst, err); compared += 1
                    assert err <= DIST_TOL, (name, t, i, k, err)
        assert agree >= 0.9 * total, (name, agree, total)
    print(f'contact distances vs fp64: worst {worst:.2e} m over {compared} contacts')
    assert compared > 500


def test_point_bot_counts_equal_the_oracle():
    """PointGather among cubes placed around it: n_contacts, n_rows and the number of item-surface contacts of every env-step equal
    `orc_point_substeps_items_f32`'s (the force a / |a| * point_force formed in fp32 as the kernel does); lane order does not matter."""
    tr, rec, rev = cc.trace('point'), cc.emu_records('point'), cc.emu_records('point', reverse=True)
    assert not np.isnan(rec).any() and np.array_equal(cc.bits(rec), cc.bits(rev))
    with_item = 0
    for t, s in enumerate(tr.steps):
        for i, rp in enumerate(s['replay']):
            r = rec[t, i]
            if not s['done'][i]:
                assert np.array_equal(cc.bits(rp['q']), cc.bits(s['after'][i, :7])), (t, i, 'the replay is not the step')
            n_item = sum(int(cc.contact(r, k)[16]) >= K.HRL_SURF_ITEM for k in range(int(r[0])))
            assert (int(r[0]), int(r[1]), int(r[2]), n_item) == (rp['n_contacts'], 0, rp['n_rows'], rp['n_item_contacts']), (t, i, r[:3], rp)
            assert not cc.bits(r[4:16]).any()  # no joints: impulses and masks +0.0
            with_item += rp['n_item_contacts'] > 0
    assert with_item >= 1, with_item


POINT_LAM_MEASURED = 1.71e-5   # largest |fp32 emulator - fp64 textbook| impulse over the cases below, N s (largest impulse there: 0.75 N s)
POINT_LAM_TOL = 4 * POINT_LAM_MEASURED


def test_point_bot_impulses_against_the_fp64_textbook_reference():
    """lambda of the point bot against `textbook.point_substep` at one substep per step, where the surface lists agree.

    The scenario the records are specified on (cubes placed within +-0.9 m of the player's centre) yields NO env-step to compare at one
    substep per step: the player is still falling from its reset height when the cubes arrive (30 substeps), so its only contacts are with
    cubes inside its own box, where the kernel's second pass (the cubes' corners against the player's box) finds contacts the textbook
    reference does not model -- 0 of 24 env-steps with a contact agree.  So the comparison runs on that scenario (whatever agrees) AND on
    the same scenario with the player set down on the floor at step 0 (z = 0.355 + ground_z: four ground corners per step, every one of the
    480 env-steps agrees).  Tolerance: 4 x the largest |difference| measured there: 1.71e-5 N s measured (impulses up to 0.75 N s; what one fp32
    ulp of a corner height, 3e-8 m, is worth through the bias dist / h on a 10 kg body: 3e-8 x 242 x 2.5 = 1.8e-5), asserted 6.84e-5 N s; a
    wrong row order or a friction row read for a normal is off by the impulses themselves, 0.02 .. 0.75 N s."""
    worst, compared = 0.0, 0
    for rest in (False, True):
        tr, rec = point_one_substep(rest)
        for t, s in enumerate(tr.steps):
            for i in range(tr.cfg.num_envs):
                a = s['act'][i]
                if not np.isfinite(cc.pre_step(tr.cfg, s['state'][i], a)[2]).all():
                    continue
                out, r = textbook_step(tr, s, i), rec[t, i]
                n = int(r[0])
                if n == 0 or [int(cc.contact(r, k)[16]) for k in range(n)] != [tb_code(out.contact_surface[k], tr.cfg) for k in range(out.n_contacts)]:
                    continue
                got = np.r_[[cc.contact(r, k)[7] for k in range(n)], np.array([[cc.contact(r, k)[11], cc.contact(r, k)[15]] for k in range(n)]).reshape(-1)]
                ref = np.array([out.lambda_[k] for k in range(out.n_rows)])
                assert out.n_rows == 3 * n
                err = np.abs(got - ref).max()
                worst = max(worst, err); compared += 1
                assert err <= POINT_LAM_TOL, (rest, t, i, err, got, ref)
    print(f'point impulses vs fp64: worst |difference| {worst:.2e} N s over {compared} env-steps')
    assert compared >= 100, compared


def point_one_substep(rest):
    """The point scenario at one substep per step; rest: the player starts on the floor (the driver's state is edited before step 0)."""
    if not rest:
        return cc.trace('point', frame_skip=1), cc.emu_records('point', frame_skip=1)
    import orc
    cfg = cc.make_cfg('point', frame_skip=1)
    o = orc.OracleEnv(cfg, np.float32)
    o.reset()
    o.state[:, 2] = np.float32(0.355) + np.float32(cfg.model.ground_z)
    rng = np.random.RandomState(cc.SEED)
    tr = cc.Trace()
    tr.name, tr.cfg, tr.steps = 'point', cfg, []
    for t in range(30):
        a = rng.uniform(-1, 1, (o.N, o.ad)).astype(np.float32)
        tr.steps.append(dict(state=o.state.copy(), items=o.items.copy(), aux=o.aux.copy(), act=a))
        o.step(a)
    e = cc.EmuContactsEnv(cfg)
    e.reset()
    return tr, cc.run(tr, e, lambda env, a: env.step(a))


def test_capi_mirror_and_older_layout():
    """make_buffers(..., contacts=p) round-trips as the longer record hrl_buffers_ext = hrl_buffers + the pointer, of the header's size; the v7
    record keeps its size (without the pointer make_buffers hands out exactly it), and its size -- the offset of `contacts` -- is a known layout:
    a multiple of the pointer size between the v7 base and the longer record, which is what the library's range check admits."""
    import os
    import re
    import subprocess
    import tempfile
    b = K.make_buffers(1, 2, 3, 4, 5, 6, 7, 8, contacts=0x1000)
    assert isinstance(b, K.hrl_buffers_ext) and b.contacts == 0x1000 and b.solver_rows is None and b.info == 8 and b.struct_size == C.sizeof(K.hrl_buffers_ext)
    plain = K.make_buffers(1, 2, 3, 4, 5, 6, 7, 8)
    assert type(plain) is K.hrl_buffers and plain.struct_size == C.sizeof(K.hrl_buffers)
    e = K.hrl_buffers_ext.of(plain)
    assert e.contacts is None and e.struct_size == C.sizeof(K.hrl_buffers_ext) and [getattr(e, f) for f, _ in K.hrl_buffers._fields_[1:]] == [getattr(plain, f) for f, _ in K.hrl_buffers._fields_[1:]]
    off = K.hrl_buffers_ext.contacts.offset
    assert off == C.sizeof(K.hrl_buffers) and off + C.sizeof(C.c_void_p) == C.sizeof(K.hrl_buffers_ext)
    base = C.sizeof(C.c_uint64) + 8 * C.sizeof(C.c_void_p)
    assert base <= off <= C.sizeof(K.hrl_buffers_ext) and off % C.sizeof(C.c_void_p) == 0
    src = '#include "include/hrl_envs.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu", sizeof(hrl_buffers), sizeof(hrl_buffers_ext), offsetof(hrl_buffers_ext, contacts));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', cc.ROOT, '-o', os.path.join(d, 't'), os.path.join(d, 't.c')], cwd=cc.ROOT)
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).decode().split()]
    assert out == [C.sizeof(K.hrl_buffers), C.sizeof(K.hrl_buffers_ext), off]
    assert (K.HRL_CONTACTS_STRIDE, K.HRL_CONTACTS_HEADER + K.HRL_CONTACT_MAX * K.HRL_CONTACT_WIDTH) == (256, 256)
    hdr = open(os.path.join(cc.ROOT, 'include', 'hrl_envs.h')).read()
    for name in ('HRL_CONTACT_MAX', 'HRL_CONTACT_WIDTH', 'HRL_CONTACTS_HEADER', 'HRL_CONTACTS_STRIDE', 'HRL_SURF_BOX', 'HRL_SURF_ITEM', 'HRL_SURF_SELF'):
        assert int(re.search(rf'#define {name} (\d+)', hdr).group(1)) == getattr(K, name), name


def hand_made_record():
    import torch
    raw = torch.zeros(2, 256)
    h = 0.004125
    raw[0, 0:4] = torch.tensor([3, 1, 10, h]); raw[0, 4 + 2] = -0.5; raw[0, 12] = 4; raw[0, 13] = 4

    def put(e, i, pos, dist, n, ln, t1, l1, t2, l2, surf, link, link2, mu):
        raw[e, 16 + 20 * i: 36 + 20 * i] = torch.tensor([*pos, dist, *n, ln, *t1, l1, *t2, l2, surf, link, link2, mu], dtype=torch.float32)
    put(0, 0, (1, 2, 0.005), -0.001, (0, 0, 1), 0.2, (1, 0, 0), 0.05, (0, 1, 0), -0.02, 0, 2 | (1 << 2), -1, 1.2)        # foot of leg 1 on the ground
    put(0, 1, (1, 2, 0.1), 0.01, (1, 0, 0), 0.1, (0, 1, 0), 0.0, (0, 0, 1), 0.01, K.HRL_SURF_ITEM + 5, 0, -1, 1.2)        # torso against cube 5
    put(0, 2, (1, 2, 0.3), 0.0, (0, 1, 0), 0.3, (0, 0, 1), 0.1, (1, 0, 0), 0.0, K.HRL_SURF_SELF + 7, 1 | (0 << 2), 2 | (3 << 2), 2.25)  # aux of leg 0 against foot of leg 3
    raw[1, 0:4] = torch.tensor([2, 0, 6, h])
    put(1, 0, (0, 0, 0.005), 0.0, (-1, 0, 0), 0.4, (0, 1, 0), 0.0, (0, 0, 1), 0.0, 2, 1 | (2 << 2), -1, 1.2)             # a wall plane
    put(1, 1, (0, 0, 0.005), 0.0, (0, -1, 0), 0.4, (0, 0, 1), 0.0, (1, 0, 0), 0.0, K.HRL_SURF_BOX, 0, -1, 1.2)           # the maze box
    return raw, h


def test_decode_and_link_force_on_a_hand_made_record():
    import torch
    from hrl_pybullet_envs_amd import contacts
    raw, h = hand_made_record()
    d = contacts.decode(raw)
    assert d['n'].tolist() == [3, 2] and d['valid'].sum(1).tolist() == [3, 2]
    assert d['kind'][0, :4].tolist() == [contacts.GROUND, contacts.ITEM, contacts.SELF, -1] and d['kind'][1, :3].tolist() == [contacts.WALL, contacts.BOX, -1]
    assert d['item'][0, :3].tolist() == [-1, 5, -1] and d['link2'][0, :4].tolist() == [-1, -1, 14, -1]
    assert d['position'].shape == (2, 12, 3) and d['friction_force'].shape == (2, 12, 3) and d['limit_impulse'].shape == (2, 8)
    assert d['position'].data_ptr() == raw[:, 16:].data_ptr()  # views of the record, not copies
    assert torch.allclose(d['normal_force'][0, :3], torch.tensor([0.2, 0.1, 0.3]) / h)
    assert torch.allclose(d['friction_force'][0, 0], torch.tensor([0.05, -0.02, 0.0]) / h)
    assert d['limit_impulse'][0].tolist() == [0, 0, -0.5, 0, 0, 0, 0, 0] and int(d['n_limit_rows'][0]) == 1 and int(d['n_rows'][0]) == 10
    lf = contacts.link_force(d)
    assert lf.shape == (2, 9, 3)
    f = d['normal_force'][..., None] * d['normal'] + d['friction_force']
    # the sum over bodies == the sum of the per-contact forces of the contacts with the world (a self contact cancels itself)
    world = (d['valid'] & (d['link2'] < 0))[..., None]
    assert torch.allclose(lf.sum(1), (f * world).sum(1), atol=1e-4)
    # the self contact alone: equal and opposite on aux of leg 0 (body 1) and foot of leg 3 (body 8)
    assert torch.allclose(lf[0, 1], f[0, 2], atol=1e-4) and torch.allclose(lf[0, 8], -f[0, 2], atol=1e-4)
    assert torch.allclose(lf[0, 4], f[0, 0], atol=1e-4) and torch.allclose(lf[0, 0], f[0, 1], atol=1e-4)   # foot of leg 1; the torso
    assert torch.allclose(lf[1, 5], f[1, 0], atol=1e-4) and torch.allclose(lf[1, 0], f[1, 1], atol=1e-4)
    # a cube beyond the 48th sits behind the capsule-pair codes; link2 = -1 tells it from a self contact
    raw[1, 16 + 20 + 16] = K.HRL_SURF_SELF + 50
    assert int(contacts.decode(raw)['item'][1, 1]) == 50 and int(contacts.decode(raw)['kind'][1, 1]) == contacts.ITEM
    pts = contacts.as_list(raw, 0)
    assert [p['kind'] for p in pts] == ['ground', 'item', 'self'] and pts[1]['item'] == 5 and pts[0]['normal_force'] == pytest.approx(0.2 / h, rel=1e-6)
    assert contacts.as_list(torch.zeros(1, 256)) == []  # a record no step has written
    with pytest.raises(ValueError):
        contacts.decode(torch.zeros(2, 255))
