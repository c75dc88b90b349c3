"""The guards of the link states' library (libhrl_links_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_sensor_launch.py.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/links_hip.hip and csrc/links_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import links_device as Lk
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in Lk.FIELDS)


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output, to be moved or nulled by a test."""

    def __init__(self, frame='heading'):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = Lk.default_spec(self.cfg, frame)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 13 * 4 * 4) for o in OUTPUTS}

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True, out=True):
        o = Lk.hrl_links_out(**self.addr)
        return Lk.lib().hrl_links(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), None, C.byref(o) if out else None, None)

    def last_error(self):
        return Lk.lib().hrl_links_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_links: ') and phrase in why, why
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


def test_output_guards():
    for output in OUTPUTS:
        c = Call()
        for _ in range(3):   # 1, 2 and 3 bytes past a multiple of 4
            c.addr[output] += 1
            c.refused(f'{output} must be 4-byte aligned')
    for first, second in (('origin', 'com'), ('quat', 'site_vel'), ('ang_vel', 'site_pos')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_links: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('links out holds no pointer: at least one output must be given')
    c = Call()
    for output in OUTPUTS[:5]:
        c.addr[output] = None
    c.spec.n_sites = 0   # the site tensors alone, and no site to write
    c.refused('links out holds no pointer: at least one output must be given')
    Call().refused('null links out', out=False)


def test_config_and_spec_guards_come_first():
    """A config hrl_create() would refuse and a bad spec are named before the buffer record is looked at."""
    c = Call()
    c.cfg.num_envs = 0
    assert c(record=False) == K.HRL_ERR_BAD_ARG and c.last_error().startswith('hrl_links: ') and 'null buffer record' not in c.last_error()
    for field, value, phrase in (('frame', 2, 'unknown links frame'), ('n_sites', 17, 'links n_sites must be within 0..16'), ('n_sites', -1, 'links n_sites must be within 0..16'),
                                 ('struct_size', 264, 'hrl_links_spec.struct_size is not sizeof(hrl_links_spec)')):
        c = Call()
        setattr(c.spec, field, value)
        c.refused(phrase, record=False)
    c = Call()
    c.spec.site_link[3] = 13
    c.refused('links site_link must be within 0..B-1', record=False)
    c = Call()
    c.spec.site_local[0][2] = float('nan')
    c.refused('links site_local must be finite', record=False)
    c = Call()
    c.spec.site_link[4], c.spec.site_local[9][0] = 99, float('inf')   # beyond n_sites = 4: not looked at
    c.refused('null buffer record', record=False)
    s = Lk.hrl_links_spec()
    assert Lk.lib().hrl_links_default_spec(None, 0, C.byref(s)) == K.HRL_ERR_BAD_ARG and Lk.lib().hrl_links_last_error().startswith(b'hrl_links_default_spec: ')
    assert Lk.lib().hrl_links_default_spec(C.byref(Call().cfg), 2, C.byref(s)) == K.HRL_ERR_BAD_ARG
    assert Lk.lib().hrl_links_count(K.HRL_ANT_FLAT) == 13 and Lk.lib().hrl_links_count(K.HRL_POINT_GATHER) == 1 and Lk.lib().hrl_links_count(99) == 0
    assert Lk.NAMES(K.HRL_ANT_FLAT)[2] == 'front_left_foot' and Lk.lib().hrl_links_name(K.HRL_ANT_FLAT, 13) is None and Lk.lib().hrl_links_name(99, 0) is None


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, scan = Call(), Other('scan')
    scan.refused('null buffer record', record=False)
    before = scan.last_error()
    mine.spec.frame = 7
    mine.refused('unknown links frame')
    assert scan.last_error() == before and before.startswith('hrl_scan: ')
    why = mine.last_error()
    scan.bufs.struct_size = 0
    scan.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_on_host_tensors():
    """What BatchedEnv.links hands to the binding's check, with host tensors against an env on cuda:0: the exception types that the GPU
    test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = Lk.default_spec(cfg, 'world')
    out = Lk.Links(*(torch.zeros(N, *shape) for shape in Lk.shapes(cfg, spec)))
    assert tuple(out.quat.shape) == (N, 13, 4) and tuple(out.site_vel.shape) == (N, 4, 3)
    assert Lk.check_out(out, N, cfg, spec, cpu) is out
    assert Lk.check_out(Lk.Links(com=out.com), N, cfg, spec, cpu).com is out.com   # None members are skipped
    with pytest.raises(TypeError, match='out must be a links_device.Links'):
        Lk.check_out(tuple(out), N, cfg, spec, dev)
    with pytest.raises(TypeError, match='out.origin must be a torch.float32 tensor'):
        Lk.check_out(out._replace(origin=out.origin.double()), N, cfg, spec, dev)
    with pytest.raises(TypeError, match='out.com must be a torch.float32 tensor'):
        Lk.check_out(out._replace(com=out.com.double()), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match=r'out.quat must be contiguous \(2, 13, 4\)'):
        Lk.check_out(out._replace(quat=torch.zeros(N, 13, 3)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match=r'out.site_pos must be contiguous \(2, 4, 3\)'):
        Lk.check_out(out._replace(site_pos=torch.zeros(N, 16, 3)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.origin must be contiguous'):
        Lk.check_out(out._replace(origin=torch.zeros(N, 13, 6)[..., ::2]), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.origin lives on cpu, the env on cuda:0'):
        Lk.check_out(out, N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        Lk.check_out(Lk.Links(), N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out.lin_vel must be 4-byte aligned'):
        Lk.check_out(out._replace(lin_vel=unaligned((N, 13, 3), torch.float32, 2)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.origin and out.com must not be the same memory'):
        Lk.check_out(out._replace(com=out.origin), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.lin_vel must be 4-byte aligned'):   # every member's own check comes before the same-memory rule
        Lk.check_out(out._replace(com=out.origin, lin_vel=unaligned((N, 13, 3), torch.float32, 2)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.origin and out.com must not be the same memory'):   # the first pair in the record's order
        Lk.check_out(out._replace(com=out.origin, ang_vel=out.origin, site_vel=out.site_pos), N, cfg, spec, cpu)
    none = Lk.default_spec(cfg, 'world', ())
    empty = torch.zeros(N, 0, 3)
    assert Lk.check_out(Lk.Links(origin=out.origin, site_pos=empty, site_vel=empty), N, cfg, none, cpu).site_vel is empty   # empty tensors share their (null) address
    point = _lib.default_config(K.HRL_POINT_GATHER, num_envs=N)
    assert Lk.shapes(point, Lk.default_spec(point)) == ((1, 3), (1, 3), (1, 4), (1, 3), (1, 3), (1, 3), (1, 3))
    assert Lk.sized(spec) and not Lk.sized(Lk.hrl_links_spec(n_sites=17)) and not Lk.sized(Lk.hrl_links_spec(n_sites=-1))
    t = Lk.Links(origin=torch.tensor([[[1.0, 2.0, 3.0]]]), com=torch.tensor([[[2.0, 2.5, 3.0]]]))
    assert Lk.tip(t).tolist() == [[[3.0, 3.0, 3.0]]]
    assert Lk.FEET == (2, 4, 6, 8) and tuple(Lk.NAMES(cfg)[i] for i in Lk.FEET) == Lk.FOOT_LIST
