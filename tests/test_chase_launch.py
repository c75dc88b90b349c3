"""The guards of the chase camera's library (libhrl_chase_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_sensor_launch.py.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/chase_hip.hip and csrc/chase_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import chase_device as Ch
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in Ch.FIELDS)


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output, to be moved or nulled by a test."""

    def __init__(self, frame='heading'):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = Ch.default_spec(self.cfg, frame)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 48 * 64 * 4) for o in OUTPUTS}

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True, out=True):
        o = Ch.hrl_chase_out(**self.addr)
        return Ch.lib().hrl_chase(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), None, C.byref(o) if out else None, None)

    def last_error(self):
        return Ch.lib().hrl_chase_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_chase: ') and phrase in why, why
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
    for first, second in (('depth', 'rgb'), ('seg', 'rgb'), ('depth', 'seg')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_chase: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('chase out holds no pointer: at least one output must be given')
    Call().refused('null chase out', out=False)


def test_config_and_spec_guards_come_first():
    """A config hrl_create() would refuse and a bad spec are named before the buffer record is looked at."""
    c = Call()
    c.cfg.num_envs = 0
    assert c(record=False) == K.HRL_ERR_BAD_ARG and c.last_error().startswith('hrl_chase: ') and 'null buffer record' not in c.last_error()
    for field, value, phrase in (('width', 24, 'chase width must be a multiple of 16 within 16..256'), ('height', 260, 'chase height must be a multiple of 8 within 8..256'),
                                 ('frame', 2, 'unknown chase frame'), ('target_mode', 2, 'unknown chase target_mode'),
                                 ('target_height', 11.0, 'chase target_height must be finite and within 0..10'), ('yaw', (0.5, 0.5), 'chase yaw must be a (cos, sin) pair'),
                                 ('pitch', (-1.0, 0.0), 'chase pitch must be a (cos, sin) pair with cos >= 0'), ('distance', 0.25, 'chase distance must be within 0.5..50'),
                                 ('tan_half_h', 0.0, 'chase tan_half_h must be finite'), ('tan_half_v', float('nan'), 'chase tan_half_v must be finite'),
                                 ('max_range', float('inf'), 'chase max_range must be finite and positive'), ('classes', 0, 'chase classes must be a non-empty mask'),
                                 ('classes', 128, 'chase classes must be a non-empty mask'), ('tile', -0.5, 'chase tile must be within 0..1e6'),
                                 ('struct_size', 64, 'hrl_chase_spec.struct_size is not sizeof(hrl_chase_spec)')):
        c = Call()
        if field in ('yaw', 'pitch'):
            getattr(c.spec, field)[0], getattr(c.spec, field)[1] = value
        else:
            setattr(c.spec, field, value)
        c.refused(phrase, record=False)
    s = Ch.hrl_chase_spec()
    assert Ch.lib().hrl_chase_default_spec(None, 0, C.byref(s)) == K.HRL_ERR_BAD_ARG and Ch.lib().hrl_chase_last_error().startswith(b'hrl_chase_default_spec: ')
    assert Ch.lib().hrl_chase_default_spec(C.byref(Call().cfg), 2, C.byref(s)) == K.HRL_ERR_BAD_ARG


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, scan = Call(), Other('scan')
    scan.refused('null buffer record', record=False)
    before = scan.last_error()
    mine.spec.classes = 0
    mine.refused('chase classes must be a non-empty mask')
    assert scan.last_error() == before and before.startswith('hrl_scan: ')
    why = mine.last_error()
    scan.bufs.struct_size = 0
    scan.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_on_host_tensors():
    """What BatchedEnv.chase hands to the binding's check, with host tensors against an env on cuda:0: the exception types that the GPU
    test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = Ch.default_spec(cfg, 'world', 48, 24)
    out = Ch.Chase(torch.zeros(N, 24, 48), torch.zeros(N, 24, 48, dtype=torch.int32), torch.zeros(N, 24, 48, 3, dtype=torch.uint8))
    assert Ch.check_out(out, N, spec, cpu) is out
    assert Ch.check_out(Ch.Chase(seg=out.seg), N, spec, cpu).seg is out.seg   # None members are skipped
    with pytest.raises(TypeError, match='out must be a chase_device.Chase'):
        Ch.check_out(tuple(out), N, spec, dev)
    with pytest.raises(TypeError, match='out.depth must be a torch.float32 tensor'):
        Ch.check_out(out._replace(depth=out.depth.double()), N, spec, dev)
    with pytest.raises(TypeError, match='out.seg must be a torch.int32 tensor'):
        Ch.check_out(out._replace(seg=out.seg.long()), N, spec, cpu)
    with pytest.raises(TypeError, match='out.rgb must be a torch.uint8 tensor'):
        Ch.check_out(out._replace(rgb=out.rgb.float()), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.depth must be contiguous \(2, 24, 48\)'):
        Ch.check_out(out._replace(depth=torch.zeros(N, 48, 24)), N, spec, dev)
    with pytest.raises(ValueError, match=r'out.rgb must be contiguous \(2, 24, 48, 3\)'):
        Ch.check_out(out._replace(rgb=torch.zeros(N, 24, 48, 4, dtype=torch.uint8)[..., :3]), N, spec, cpu)
    with pytest.raises(ValueError, match='out.seg must be contiguous'):
        Ch.check_out(out._replace(seg=torch.zeros(N, 24, 96, dtype=torch.int32)[..., ::2]), N, spec, cpu)
    with pytest.raises(ValueError, match='out.depth lives on cpu, the env on cuda:0'):
        Ch.check_out(out, N, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        Ch.check_out(Ch.Chase(), N, spec, dev)
    with pytest.raises(ValueError, match='out.rgb must be 4-byte aligned'):
        Ch.check_out(out._replace(rgb=unaligned((N, 24, 48, 3), torch.uint8, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.depth and out.seg must not be the same memory'):
        Ch.check_out(out._replace(seg=out.depth.view(torch.int32)), N, spec, cpu)
    # every member's own check comes before the same-memory rule, in the record's order
    with pytest.raises(ValueError, match='out.rgb must be 4-byte aligned'):
        Ch.check_out(Ch.Chase(out.depth, out.depth.view(torch.int32), unaligned((N, 24, 48, 3), torch.uint8, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.depth must be 4-byte aligned'):
        Ch.check_out(Ch.Chase(unaligned((N, 24, 48), torch.float32, 2), out.seg, unaligned((N, 24, 48, 3), torch.uint8, 1)), N, spec, cpu)
    assert Ch.sized(spec) and not Ch.sized(Ch.hrl_chase_spec(width=272, height=24)) and not Ch.sized(Ch.hrl_chase_spec(width=48, height=0))
    assert 'spec.width must be within 16..256' in Ch.size_error(Ch.hrl_chase_spec(width=512, height=8))
