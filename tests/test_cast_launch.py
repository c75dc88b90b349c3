"""The guards of the ray test's library (libhrl_cast_hip.so) that return before a device is looked for, and what its Python binding refuses
before it calls, in the form of test_chase_launch.py.  CPU only: every call below returns before the HIP runtime is asked anything, so the
results are the same with and without a GPU.  The phrases are copied from csrc/cast_hip.hip and csrc/cast_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import cast_device as Ca
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in Ca.FIELDS)
R = 64


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output, `rays` and `ray_link` those of the inputs, to be moved or nulled by a test."""

    def __init__(self, frame='heading'):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = Ca.default_spec(self.cfg, frame, R)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * R * 3 * 4) for o in OUTPUTS}
        self.rays, self.ray_link = self.room(N * R * 6 * 4), self.room(R * 4)

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True, out=True):
        o = Ca.hrl_cast_out(**self.addr)
        return Ca.lib().hrl_cast(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), self.rays, self.ray_link, None, C.byref(o) if out else None, None)

    def last_error(self):
        return Ca.lib().hrl_cast_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_cast: ') and phrase in why, why
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


def test_ray_guards():
    """`rays` must be there and 8-byte aligned (a ray is read as three 8-byte loads); `ray_link` may be NULL and is 4-byte aligned."""
    c = Call()
    c.rays = None
    c.refused('null rays', record=False)   # named before the buffer record is looked at
    for off in (1, 2, 4, 6):
        c = Call()
        c.rays += off
        c.refused('rays must be 8-byte aligned')
        assert c.last_error() == 'hrl_cast: rays must be 8-byte aligned'
    for off in (1, 2, 3):
        c = Call('link')
        c.ray_link += off
        c.refused('ray_link must be 4-byte aligned')
    c = Call()
    c.rays += 4
    c.ray_link += 2
    c.addr['fraction'] += 1
    c.refused('rays must be 8-byte aligned')   # of several, the first in the entry point's order is named
    c = Call()
    c.ray_link += 2
    c.addr['fraction'] += 1
    c.refused('ray_link must be 4-byte aligned')


def test_output_guards():
    for output in OUTPUTS:
        c = Call()
        for _ in range(3):   # 1, 2 and 3 bytes past a multiple of 4
            c.addr[output] += 1
            c.refused(f'{output} must be 4-byte aligned')
    for first, second in (('fraction', 'normal'), ('seg', 'point'), ('point', 'normal'), ('fraction', 'seg')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_cast: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('cast out holds no pointer: at least one output must be given')
    Call().refused('null cast out', out=False)


def test_config_and_spec_guards_come_first():
    """A config hrl_create() would refuse and a bad spec are named before the buffer record is looked at."""
    c = Call()
    c.cfg.num_envs = 0
    assert c(record=False) == K.HRL_ERR_BAD_ARG and c.last_error().startswith('hrl_cast: ') and 'null buffer record' not in c.last_error()
    for field, value, phrase in (('n_rays', 0, 'cast n_rays must be within 1..1024'), ('n_rays', 1025, 'cast n_rays must be within 1..1024'), ('n_rays', -3, 'cast n_rays must be within 1..1024'),
                                 ('frame', 4, 'unknown cast frame'), ('frame', -1, 'unknown cast frame'), ('classes', 0, 'cast classes must be a non-empty mask'),
                                 ('classes', 128, 'cast classes must be a non-empty mask'), ('classes', 256 | 1, 'cast classes must be a non-empty mask'),
                                 ('reserved', 1, 'cast reserved must be 0'), ('struct_size', 16, 'hrl_cast_spec.struct_size is not sizeof(hrl_cast_spec)'),
                                 ('struct_size', 0, 'hrl_cast_spec.struct_size is not sizeof(hrl_cast_spec)')):
        c = Call()
        setattr(c.spec, field, value)
        c.refused(phrase, record=False)
    for n_rays in (1, 1024):
        c = Call()
        c.spec.n_rays = n_rays
        c.refused('null buffer record', record=False)   # the spec itself passes
    s = Ca.hrl_cast_spec()
    assert Ca.lib().hrl_cast_default_spec(None, 0, C.byref(s)) == K.HRL_ERR_BAD_ARG and Ca.lib().hrl_cast_last_error().startswith(b'hrl_cast_default_spec: ')
    assert Ca.lib().hrl_cast_default_spec(C.byref(Call().cfg), 4, C.byref(s)) == K.HRL_ERR_BAD_ARG
    for frame in range(4):
        assert Ca.lib().hrl_cast_default_spec(C.byref(Call().cfg), frame, C.byref(s)) == K.HRL_OK
        assert (s.struct_size, s.n_rays, s.frame, s.classes, s.reserved) == (C.sizeof(Ca.hrl_cast_spec), 64, frame, Ca.EVERYTHING, 0)


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, scan = Call(), Other('scan')
    scan.refused('null buffer record', record=False)
    before = scan.last_error()
    mine.spec.classes = 0
    mine.refused('cast classes must be a non-empty mask')
    assert scan.last_error() == before and before.startswith('hrl_scan: ')
    why = mine.last_error()
    scan.bufs.struct_size = 0
    scan.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_and_the_input_checks_on_host_tensors():
    """What BatchedEnv.cast hands to the binding's checks, with host tensors against an env on cuda:0: the exception types that the GPU
    test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = Ca.default_spec(cfg, 'world', 24)
    out = Ca.Cast(torch.zeros(N, 24), torch.zeros(N, 24, dtype=torch.int32), torch.zeros(N, 24, 3), torch.zeros(N, 24, 3))
    assert Ca.check_out(out, N, spec, cpu) is out
    assert Ca.check_out(Ca.Cast(seg=out.seg), N, spec, cpu).seg is out.seg   # None members are skipped
    with pytest.raises(TypeError, match='out must be a cast_device.Cast'):
        Ca.check_out(tuple(out), N, spec, dev)
    with pytest.raises(TypeError, match='out.fraction must be a torch.float32 tensor'):
        Ca.check_out(out._replace(fraction=out.fraction.double()), N, spec, dev)
    with pytest.raises(TypeError, match='out.seg must be a torch.int32 tensor'):
        Ca.check_out(out._replace(seg=out.seg.long()), N, spec, cpu)
    with pytest.raises(TypeError, match='out.normal must be a torch.float32 tensor'):
        Ca.check_out(out._replace(normal=out.normal.half()), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.fraction must be contiguous \(2, 24\)'):
        Ca.check_out(out._replace(fraction=torch.zeros(N, 25)), N, spec, dev)
    with pytest.raises(ValueError, match=r'out.point must be contiguous \(2, 24, 3\)'):
        Ca.check_out(out._replace(point=torch.zeros(N, 24, 4)[..., :3]), N, spec, cpu)
    with pytest.raises(ValueError, match='out.fraction lives on cpu, the env on cuda:0'):
        Ca.check_out(out, N, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        Ca.check_out(Ca.Cast(), N, spec, dev)
    with pytest.raises(ValueError, match='out.normal must be 4-byte aligned'):
        Ca.check_out(out._replace(normal=unaligned((N, 24, 3), torch.float32, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.fraction and out.seg must not be the same memory'):
        Ca.check_out(out._replace(seg=out.fraction.view(torch.int32)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.point and out.normal must not be the same memory'):
        Ca.check_out(out._replace(normal=out.point), N, spec, cpu)
    rays = torch.zeros(N, 24, 6)
    assert Ca.check_rays(rays, N, spec, cpu) is rays
    with pytest.raises(ValueError, match='out.point and rays must not be the same memory'):
        Ca.check_out(out._replace(point=rays.view(-1)[:N * 24 * 3].view(N, 24, 3)), N, spec, cpu, rays)
    with pytest.raises(TypeError, match='rays must be a torch.float32 tensor'):
        Ca.check_rays(rays.double(), N, spec, cpu)
    with pytest.raises(ValueError, match=r'rays must be contiguous \(2, 24, 6\)'):
        Ca.check_rays(torch.zeros(N, 25, 6), N, spec, cpu)
    with pytest.raises(ValueError, match='rays must be contiguous'):
        Ca.check_rays(torch.zeros(24, 6).expand(N, 24, 6), N, spec, cpu)   # a broadcast view: materialise it (cast_device.expand)
    with pytest.raises(ValueError, match='rays lives on cpu, the env on cuda:0'):
        Ca.check_rays(rays, N, spec, dev)
    with pytest.raises(ValueError, match='rays must be 8-byte aligned'):
        Ca.check_rays(unaligned((N, 24, 6), torch.float32, 4), N, spec, cpu)
    links = torch.zeros(24, dtype=torch.int32)
    assert Ca.check_ray_link(links, spec, cpu) is links
    with pytest.raises(TypeError, match='ray_link must be a torch.int32 tensor'):
        Ca.check_ray_link(links.long(), spec, cpu)
    with pytest.raises(ValueError, match=r'ray_link must be contiguous \(24,\)'):
        Ca.check_ray_link(torch.zeros(23, dtype=torch.int32), spec, cpu)
    assert Ca.sized(spec) and not Ca.sized(Ca.hrl_cast_spec(n_rays=0)) and not Ca.sized(Ca.hrl_cast_spec(n_rays=1025))
    assert 'spec.n_rays must be within 1..1024' in Ca.size_error(Ca.hrl_cast_spec(n_rays=2000))
    e = Ca.expand(torch.zeros(24, 6), N)
    assert tuple(e.shape) == (N, 24, 6) and e.is_contiguous() and Ca.check_rays(e, N, spec, cpu) is e
    with pytest.raises(ValueError, match=r'a ray pattern must be \[R, 6\]'):
        Ca.expand(torch.zeros(24, 5), N)
