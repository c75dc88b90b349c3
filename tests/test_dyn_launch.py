"""The guards of the dynamics terms' library (libhrl_dyn_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_links_launch.py.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/dyn_hip.hip and csrc/dyn_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import dyn_device as Dy
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in Dy.FIELDS)


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output and of tau, to be moved or nulled by a test."""

    def __init__(self):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = Dy.default_spec(self.cfg)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 16 * 3 * 14 * 4) for o in OUTPUTS}
        self.tau = self.room(N * 14 * 4)

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True, out=True):
        o = Dy.hrl_dyn_out(**self.addr)
        return Dy.lib().hrl_dyn(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), self.tau, None, C.byref(o) if out else None, None)

    def last_error(self):
        return Dy.lib().hrl_dyn_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_dyn: ') and phrase in why, why
        assert all((a == 0x7B).all() for a in self.keep[2:])   # nothing was written


def test_buffer_record_guards():
    c = Call()
    c.refused('null buffer record', record=False)
    for size in (0, BASE - 8, 4104, BASE + 4):
        c.bufs.struct_size = size
        c.refused(STRUCT_SIZE)
    for member in ('state', 'aux'):
        c = Call()
        setattr(c.bufs, member, None)
        c.refused('null state or aux')


def test_output_and_tau_guards():
    for output in OUTPUTS:
        c = Call()
        for _ in range(3):   # 1, 2 and 3 bytes past a multiple of 4
            c.addr[output] += 1
            c.refused(f'{output} must be 4-byte aligned')
    for first, second in (('mass', 'bias'), ('accel', 'energy'), ('jac', 'momentum')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_dyn: {first} must be 4-byte aligned'
    c = Call()
    for _ in range(3):
        c.tau += 1
        c.refused('tau must be 4-byte aligned')
    c = Call()
    c.tau += 2
    c.addr['energy'] += 1   # the outputs come before tau
    c.refused('energy must be 4-byte aligned')
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('dyn out holds no pointer: at least one output must be given')
    c = Call()
    c.spec.n_sites = 0   # a Jacobian, and no site to write
    c.refused('dyn out.jac is given and the spec holds no site')
    Call().refused('null dyn out', out=False)


def test_config_and_spec_guards_come_first():
    """A config hrl_create() would refuse and a bad spec are named before the buffer record is looked at."""
    c = Call()
    c.cfg.num_envs = 0
    assert c(record=False) == K.HRL_ERR_BAD_ARG and c.last_error().startswith('hrl_dyn: ') and 'null buffer record' not in c.last_error()
    for field, value, phrase in (('frame', 1, 'unknown dyn frame'), ('n_sites', 17, 'dyn n_sites must be within 0..16'), ('n_sites', -1, 'dyn n_sites must be within 0..16'),
                                 ('struct_size', 264, 'hrl_dyn_spec.struct_size is not sizeof(hrl_dyn_spec)')):
        c = Call()
        setattr(c.spec, field, value)
        c.refused(phrase, record=False)
    c = Call()
    c.spec.site_link[3] = 13
    c.refused('dyn site_link must be within 0..B-1', record=False)
    c = Call()
    c.spec.site_local[0][2] = float('nan')
    c.refused('dyn site_local must be finite', record=False)
    c = Call()
    c.spec.site_link[4], c.spec.site_local[9][0] = 99, float('inf')   # beyond n_sites = 4: not looked at
    c.refused('null buffer record', record=False)
    s = Dy.hrl_dyn_spec()
    assert Dy.lib().hrl_dyn_default_spec(None, C.byref(s)) == K.HRL_ERR_BAD_ARG and Dy.lib().hrl_dyn_last_error().startswith(b'hrl_dyn_default_spec: ')
    assert Dy.lib().hrl_dyn_nv(K.HRL_ANT_FLAT) == 14 and Dy.lib().hrl_dyn_nv(K.HRL_POINT_GATHER) == 6 and Dy.lib().hrl_dyn_nv(99) == 0


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, scan = Call(), Other('scan')
    scan.refused('null buffer record', record=False)
    before = scan.last_error()
    mine.spec.frame = 7
    mine.refused('unknown dyn frame')
    assert scan.last_error() == before and before.startswith('hrl_scan: ')
    why = mine.last_error()
    scan.bufs.struct_size = 0
    scan.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_and_check_tau_on_host_tensors():
    """What BatchedEnv.dynamics hands to the binding's checks, with host tensors against an env on cuda:0: the exception types that the
    GPU test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = Dy.default_spec(cfg)
    out = Dy.Dynamics(*(torch.zeros(N, *shape) for shape in Dy.shapes(cfg, spec)))
    assert tuple(out.mass.shape) == (N, 14, 14) and tuple(out.jac.shape) == (N, 4, 3, 14) and tuple(out.momentum.shape) == (N, 6)
    assert Dy.check_out(out, N, cfg, spec, cpu) is out
    assert Dy.check_out(Dy.Dynamics(bias=out.bias), N, cfg, spec, cpu).bias is out.bias   # None members are skipped
    with pytest.raises(TypeError, match='out must be a dyn_device.Dynamics'):
        Dy.check_out(tuple(out), N, cfg, spec, dev)
    with pytest.raises(TypeError, match='out.mass must be a torch.float32 tensor'):
        Dy.check_out(out._replace(mass=out.mass.double()), N, cfg, spec, dev)
    with pytest.raises(ValueError, match=r'out.accel must be contiguous \(2, 14\)'):
        Dy.check_out(out._replace(accel=torch.zeros(N, 8)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match=r'out.jac must be contiguous \(2, 4, 3, 14\)'):
        Dy.check_out(out._replace(jac=torch.zeros(N, 16, 3, 14)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.mass must be contiguous'):
        Dy.check_out(out._replace(mass=torch.zeros(N, 14, 28)[..., ::2]), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.mass lives on cpu, the env on cuda:0'):
        Dy.check_out(out, N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        Dy.check_out(Dy.Dynamics(), N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out.com must be 4-byte aligned'):
        Dy.check_out(out._replace(com=unaligned((N, 3), torch.float32, 2)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.bias and out.accel must not be the same memory'):
        Dy.check_out(out._replace(accel=out.bias), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.com must be 4-byte aligned'):   # every member's own check comes before the same-memory rule
        Dy.check_out(out._replace(accel=out.bias, com=unaligned((N, 3), torch.float32, 2)), N, cfg, spec, cpu)
    tau = torch.zeros(N, 14)
    assert Dy.check_tau(tau, N, cfg, cpu) is tau and Dy.check_out(out, N, cfg, spec, cpu, tau) is out
    with pytest.raises(ValueError, match='out.accel and tau must not be the same memory'):
        Dy.check_out(out._replace(accel=tau), N, cfg, spec, cpu, tau)
    with pytest.raises(TypeError, match='tau must be a torch.float32 tensor'):
        Dy.check_tau(tau.double(), N, cfg, cpu)
    with pytest.raises(ValueError, match=r'tau must be contiguous \(2, 14\)'):
        Dy.check_tau(torch.zeros(N, 8), N, cfg, cpu)
    with pytest.raises(ValueError, match='tau lives on cpu, the env on cuda:0'):
        Dy.check_tau(tau, N, cfg, dev)
    with pytest.raises(ValueError, match='tau must be 4-byte aligned'):
        Dy.check_tau(unaligned((N, 14), torch.float32, 1), N, cfg, cpu)
    none = Dy.default_spec(cfg, ())
    with pytest.raises(ValueError, match='out.jac is given and the spec holds no site'):
        Dy.check_out(Dy.Dynamics(mass=out.mass, jac=torch.zeros(N, 0, 3, 14)), N, cfg, none, cpu)
    point = _lib.default_config(K.HRL_POINT_GATHER, num_envs=N)
    assert Dy.shapes(point, Dy.default_spec(point)) == ((6, 6), (6,), (6,), (1, 3, 6), (3,), (6,), (2,))
    assert Dy.sized(spec) and not Dy.sized(Dy.hrl_dyn_spec(n_sites=17)) and not Dy.sized(Dy.hrl_dyn_spec(n_sites=-1))
