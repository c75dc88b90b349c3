"""The step's optional contact report (hrl_buffers_ext.contacts, BatchedEnv.record_contacts) on the MI355X: the kernel's records against the
lock-step host executor (whole records, bit for bit) and against the oracle directly, that switching it on changes nothing else, what a
finished env reports, the host / hipGraph paths and the one-env classes.  Scenarios and references: tests/contacts_cases.py."""
import numpy as np
import pytest
import torch

import contacts_cases as cc
from backends import Device

pytestmark = pytest.mark.gpu


def device_env(cfg, record=True):
    d = Device(cfg)
    d.reset()
    if record:
        d.env.record_contacts().fill_(float('nan'))  # every float must be written by the step
    return d


def device_records(tr, step=lambda d, a: d.env.step(torch.tensor(a).cuda())):
    d = device_env(tr.cfg)
    rec = cc.run(tr, d, step, fetch=lambda d: d.env.contacts.cpu().numpy(), push=Device.push)
    d.close()
    return rec


@pytest.mark.parametrize('name,n', [(name, None) for name in cc.NAMES] + [('items', 5), ('items', 1), ('point', 5), ('self', 5)])
def test_device_records_equal_the_emulator_bit_for_bit(name, n):
    """Identical inputs each step (state, items, aux, actions of the scenario's trace): the [N, 256] record array of the kernel == the host
    executor's as uint32.  N = 5 and N = 1: a ragged last group of four whose spare records are parked, and a single record."""
    tr = cc.trace(name, n)
    dev, emu = device_records(tr), cc.emu_records(name, n)
    assert not np.isnan(dev).any()
    assert dev[:, :, 0].sum() > 0 or name == 'self'   # (five envs of the self scenario need not touch; the full one does)
    for t in range(len(tr.steps)):
        assert np.array_equal(cc.bits(dev[t]), cc.bits(emu[t])), (name, t, np.argwhere(cc.bits(dev[t]) != cc.bits(emu[t]))[:4])


def test_device_records_equal_the_oracle_directly():
    """Scenario (b) -- cubes, ground, limit rows, the contact cap -- without the emulator in between: counts, surface codes and every impulse
    of the kernel's record == the oracle's replay of the step, bitwise."""
    tr = cc.trace('items')
    dev = device_records(tr)
    for t, s in enumerate(tr.steps):
        for i, rp in enumerate(s['replay']):
            cc.check_against_oracle(dev[t, i], rp, (t, i))
    assert any(rp['n_contacts'] == cc.MAXC for s in tr.steps for rp in s['replay'])


@pytest.mark.parametrize('name', ['items', 'point'])
def test_off_means_off(name):
    """The same free-running rollout with and without record_contacts(): state, items, aux and every output identical bitwise."""
    tr = cc.trace(name)
    a_env, b_env = device_env(tr.cfg).env, device_env(tr.cfg, record=False).env
    for s in tr.steps:
        a = torch.tensor(s['act']).cuda()
        ra, rb = a_env.step(a), b_env.step(a)
        for x, y in list(zip(ra[:3], rb[:3])) + [(a_env.state, b_env.state), (a_env.items, b_env.items), (a_env.info, b_env.info), (a_env.final_obs, b_env.final_obs)]:
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
        assert torch.equal(a_env.aux, b_env.aux) and torch.equal(a_env.truncated, b_env.truncated)
    assert getattr(b_env, 'contacts', None) is None and 'contacts' not in a_env.state_dict()
    # switching it off again: the tensor is left alone from then on
    last = a_env.contacts.clone()
    a_env.record_contacts(False)
    a_env.step(a)
    torch.cuda.synchronize()
    assert a_env.contacts is None and not torch.isnan(last).any()
    a_env.close(); b_env.close()


def test_a_finished_env_reports_its_terminal_step():
    """max_episode_steps = 5 with auto-reset: in the step that sets `done` the record is the oracle's replay of THAT step (from the state
    before it), not of the reset state the env holds afterwards."""
    tr = cc.trace('random', max_episode_steps=5)
    dev = device_records(tr)
    ended = tells = 0
    for t, s in enumerate(tr.steps):
        for i, rp in enumerate(s['replay']):
            cc.check_against_oracle(dev[t, i], rp, (t, i))
            if s['done'][i]:
                ended += 1
                # what a record written AFTER the reset would hold: the same action applied to the state the env was reset to
                late = cc.oracle_replay(tr.cfg, s['after'][i], s['items'][i], s['act'][i])
                tells += (late['n_rows'], late['lam'].tobytes()) != (rp['n_rows'], rp['lam'].tobytes())
    # the ants are still falling when the limit cuts in (they land around step 10): the records that tell the two apart are limit rows
    assert ended >= tr.cfg.num_envs and tells >= ended // 2, (ended, tells)


def test_step_host_and_a_graph_replay_write_the_same_record():
    tr = cc.trace('items')
    eager = device_records(tr)
    # step_host(): actions from and outputs to pinned host memory, the report stays in HBM
    host = device_records(tr, lambda d, a: d.env.step_host(a))
    assert np.array_equal(cc.bits(host), cc.bits(eager))
    # switched on AFTER the host record exists: step_host()'s record follows
    d = device_env(tr.cfg, record=False)
    g = d.env
    g.step_host(tr.steps[0]['act'])
    g.record_contacts()
    d.push(tr.steps[12]); g.step_host(tr.steps[12]['act'])
    assert np.array_equal(cc.bits(g.contacts.cpu().numpy()), cc.bits(eager[12]))
    g.close()
    # one captured step, replayed: the pointer is fixed, the replay writes the same tensor
    d = device_env(tr.cfg)
    g = d.env
    static_a = torch.tensor(tr.steps[0]['act']).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the warm-up launch torch asks for before a capture
        g.step(static_a)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(static_a)
    for t in (10, 11):
        d.push(tr.steps[t]); static_a.copy_(torch.tensor(tr.steps[t]['act']))
        g.contacts.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cc.bits(g.contacts.cpu().numpy()), cc.bits(eager[t])), t
    del graph
    g.close()


def test_single_env_get_contact_points():
    """`AntGatherBulletEnv().get_contact_points()`: the first call switches the recording on (nothing recorded yet: an empty list); after 20
    steps it names the ground contacts of the standing / tumbling ant, which carry its weight."""
    import hrl_pybullet_envs_amd as H
    from hrl_pybullet_envs_amd import contacts
    env = H.AntGatherBulletEnv(seed=3)
    env.reset()
    assert env.get_contact_points() == []
    rng = np.random.RandomState(0)
    for _ in range(20):
        env.step(rng.uniform(-1, 1, 8))
    pts = env.get_contact_points()
    ground = [p for p in pts if p['kind'] == 'ground']
    assert ground and all(p['normal'] == (0.0, 0.0, 1.0) and p['link2'] == -1 and abs(p['position'][2] - 0.005 - p['distance']) < 1e-5 for p in ground)
    assert sum(p['normal_force'] for p in ground) > 0
    d = contacts.decode(env._backend().contacts, env._cfg)
    assert int(d['n'][0]) == len(pts) and d['normal_force'].device.type == 'cuda'
    lf = contacts.link_force(d)
    up = sum(p['normal_force'] * p['normal'][2] + p['lateral_friction1'] * p['lateral_friction_dir1'][2] + p['lateral_friction2'] * p['lateral_friction_dir2'][2] for p in pts)
    assert lf.shape == (1, 9, 3) and float(lf[0, :, 2].sum()) == pytest.approx(up, rel=1e-4)
    env.close()
    # the batched class: record_contacts() hands out the tensor every step rewrites
    env = H.AntGatherBulletEnv(num_envs=8, seed=3)
    env.reset()
    raw = env.record_contacts()
    for _ in range(14):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (8, 8)).astype(np.float32)).cuda())
    d = contacts.decode(raw, env._cfg)
    assert raw.shape == (8, 256) and int(d['n'].min()) > 0 and bool((d['kind'][d['valid']] == contacts.GROUND).all())
    up = contacts.link_force(d)[:, :, 2].sum(1)   # ground contacts push up or, still closing within the contact distance, not at all
    assert bool((up >= 0).all()) and int((up > 0).sum()) >= 4
    env.close()


# ------------------------------------------------------------------------------------------------ the device's records against fp64 physics
# The checks of tests/test_contacts_physics.py (helpers: tests/contacts_cases.py) on the kernel's own records and the kernel's own states
# after the step, at one substep per step (the balance is stated for frame_skip = 1 only: with four substeps the pose at the start of the
# last one is no output).  Envs that ended in a step are left out here: their state was reset.
def device_run(name, n=None):
    """(trace, records [steps, N, 256], states after each step [steps, N, stride]) of the scenario at one substep per step on the device"""
    tr = cc.trace(name, n, 1)
    d = device_env(tr.cfg)
    after = []
    rec = cc.run(tr, d, lambda d, a: d.env.step(torch.tensor(a).cuda()), fetch=lambda d: d.env.contacts.cpu().numpy(), push=Device.push, after=after)
    d.close()
    assert not np.isnan(rec).any()
    return tr, rec, np.stack(after)


@pytest.mark.parametrize('name,n', [(name, None) for name in cc.NAMES] + [('items', 5), ('self', 5)])
def test_device_records_against_fp64_physics(name, n):
    """The kernel's records and after-states: the momentum balance (tolerances, clamp criterion and coverage floors of
    tests/test_contacts_physics.py; the floors hold for the full scenario shapes), the geometry of every contact against fp64 kinematics,
    and contacts.link_force on CUDA tensors against the numpy regrouping of the records.  n = 5: a ragged last group."""
    tr, rec, after = device_run(name, n)
    b = cc.balance(tr, rec, after, skip_done=True)
    cc.check_balance(name, b, floors=n is None)   # (the floors are the full shapes')
    if name != 'point':
        g = cc.geometry(tr, rec, skip_done=True)
        print(name, n, g)
        assert n is not None or cc.geometry_floor(name, g), (name, g)
    worst, n_self = cc.check_link_force(rec.reshape(-1, cc.STRIDE), cc.P_TOL, device='cuda')
    print(f'{name} {n}: link_force on the device vs numpy, worst {worst:.2e} N s; {n_self} self contacts')


def test_device_capsule_records_against_fp64_physics():
    """The same on the states of tests/capsule_cases.py: mid-section and second-support contacts among the compared env-steps."""
    mid = second = 0
    for name in cc.CAPSULE:
        tr, rec, after = device_run(name)
        b = cc.balance(tr, rec, after, skip_done=True)
        cc.check_balance(name, b, clamp_share=1.0)
        m, s = cc.capsule_coverage(tr, lambda t: [i for tt, i in b['rows'] if tt == t])
        mid += m; second += s
        print(name, cc.geometry(tr, rec, skip_done=True))
    assert mid >= 1 and second >= 1, (mid, second)
