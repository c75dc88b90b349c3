"""The guards of the closest points' library (libhrl_closest_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_cast_launch.py.  CPU only: every call below returns before the HIP runtime is asked anything,
so the results are the same with and without a GPU.  The phrases are copied from csrc/closest_hip.hip and csrc/closest_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

import closest_cases as hc
from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import closest_device as Cl
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in Cl.FIELDS)
B = 13
BAD_SPECS = (('classes', 0, 'closest classes must be a non-empty mask'), ('classes', Cl.TARGET, 'closest classes must be a non-empty mask'),
             ('classes', Cl.EVERYTHING | Cl.TARGET, 'closest classes must be a non-empty mask'), ('classes', 128, 'closest classes must be a non-empty mask'),
             ('classes', 256 | 1, 'closest classes must be a non-empty mask'), ('reserved', 1, 'closest reserved must be 0'),
             ('struct_size', 24, 'hrl_closest_spec.struct_size is not sizeof(hrl_closest_spec)'), ('struct_size', 0, 'hrl_closest_spec.struct_size is not sizeof(hrl_closest_spec)'))


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output, to be moved or nulled by a test."""

    def __init__(self):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = Cl.default_spec(self.cfg)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * B * 6 * 3 * 4) for o in OUTPUTS}

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True, out=True):
        o = Cl.hrl_closest_out(**self.addr)
        return Cl.lib().hrl_closest(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), None, C.byref(o) if out else None, None)

    def last_error(self):
        return Cl.lib().hrl_closest_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_closest: ') and phrase in why, why
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
    for first, second in (('distance', 'normal'), ('which', 'on_link'), ('on_link', 'on_surface'), ('on_surface', 'normal'), ('distance', 'which')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_closest: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('closest out holds no pointer: at least one output must be given')
    Call().refused('null closest out', out=False)


def test_config_and_spec_guards_come_first():
    """A config hrl_create() would refuse and a bad spec are named before the buffer record is looked at: classes 0, the TARGET bit
    alone and among the others, bits beyond the classes, reserved != 0, a wrong struct_size.  The host build refuses the same specs in
    the same words."""
    c = Call()
    c.cfg.num_envs = 0
    assert c(record=False) == K.HRL_ERR_BAD_ARG and c.last_error().startswith('hrl_closest: ') and 'null buffer record' not in c.last_error()
    for field, value, phrase in BAD_SPECS:
        c = Call()
        setattr(c.spec, field, value)
        c.refused(phrase, record=False)
        assert hc.lib().closest_validate_spec(C.byref(c.spec)).decode() == c.last_error()[len('hrl_closest: '):]
    for classes in (Cl.GROUND, Cl.ROBOT, Cl.EVERYTHING, Cl.WALL | Cl.POISON):
        c = Call()
        c.spec.classes = classes
        c.refused('null buffer record', record=False)   # the spec itself passes
    s = Cl.hrl_closest_spec()
    assert Cl.lib().hrl_closest_default_spec(None, C.byref(s)) == K.HRL_ERR_BAD_ARG and Cl.lib().hrl_closest_last_error().startswith(b'hrl_closest_default_spec: ')
    assert Cl.lib().hrl_closest_default_spec(C.byref(Call().cfg), None) == K.HRL_ERR_BAD_ARG
    assert Cl.lib().hrl_closest_default_spec(C.byref(Call().cfg), C.byref(s)) == K.HRL_OK
    assert (s.struct_size, s.classes, s.reserved) == (C.sizeof(Cl.hrl_closest_spec), Cl.EVERYTHING, 0)


@pytest.mark.parametrize('field,value,phrase', BAD_SPECS + (('out', 'empty', 'closest out holds no pointer: at least one output must be given'), ('out', 'null', 'null closest out')))
def test_the_host_build_refuses_bad_specs_with_the_librarys_reason(field, value, phrase):
    from test_render_host import shard
    cfg, state, items, aux = shard(K.HRL_ANT_FLAT)
    spec = hc.spec_of()
    fills = (-3, -7, -5, -6, -9)
    out = hc.Closest(*(np.full(shape, fill, dt) for shape, fill, dt in zip(hc.shapes_of(cfg.num_envs, cfg), fills, hc.DTYPES)))
    if field != 'out':
        setattr(spec, field, value)
    b = K.make_buffers(hc.ptr(state), hc.ptr(items), hc.ptr(aux), None, None, None, None, None)
    o = Cl.hrl_closest_out(**({} if value == 'empty' else {name: hc.ptr(a) for name, a in zip(hc.NAMES, out)}))
    ref = None if (field, value) == ('out', 'null') else C.byref(o)
    code = hc.lib().closest_host(C.byref(cfg), C.byref(b), C.byref(spec), None, ref)
    why = hc.lib().closest_host_last_error().decode()
    assert code == K.HRL_ERR_BAD_ARG and phrase in why, why
    untouched = lambda: all((x == fill).all() for x, fill in zip(out, fills))
    assert untouched()
    # the device library runs the same checks before it looks for a device
    L = Cl.lib()
    assert L.hrl_closest(C.byref(cfg), C.byref(b), C.byref(spec), None, ref, None) == K.HRL_ERR_BAD_ARG
    assert L.hrl_closest_last_error() == b'hrl_closest: ' + why.encode()
    assert untouched()


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, scan = Call(), Other('scan')
    scan.refused('null buffer record', record=False)
    before = scan.last_error()
    mine.spec.classes = 0
    mine.refused('closest classes must be a non-empty mask')
    assert scan.last_error() == before and before.startswith('hrl_scan: ')
    why = mine.last_error()
    scan.bufs.struct_size = 0
    scan.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_on_host_tensors():
    """What BatchedEnv.closest hands to the binding's check, with host tensors against an env on cuda:0: the exception types that the GPU
    test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = Cl.default_spec(cfg)
    out = Cl.Closest(torch.zeros(N, B, 6), torch.zeros(N, B, 6, dtype=torch.int32), torch.zeros(N, B, 6, 3), torch.zeros(N, B, 6, 3), torch.zeros(N, B, 6, 3))
    assert Cl.check_out(out, N, cfg, spec, cpu) is out
    assert Cl.check_out(Cl.Closest(which=out.which), N, cfg, spec, cpu).which is out.which   # None members are skipped
    with pytest.raises(TypeError, match='out must be a closest_device.Closest'):
        Cl.check_out(tuple(out), N, cfg, spec, dev)
    with pytest.raises(TypeError, match='out.distance must be a torch.float32 tensor'):
        Cl.check_out(out._replace(distance=out.distance.double()), N, cfg, spec, dev)
    with pytest.raises(TypeError, match='out.which must be a torch.int32 tensor'):
        Cl.check_out(out._replace(which=out.which.long()), N, cfg, spec, cpu)
    with pytest.raises(TypeError, match='out.normal must be a torch.float32 tensor'):
        Cl.check_out(out._replace(normal=out.normal.half()), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match=r'out.distance must be contiguous \(2, 13, 6\)'):
        Cl.check_out(out._replace(distance=torch.zeros(N, B, 5)), N, cfg, spec, dev)
    with pytest.raises(ValueError, match=r'out.on_link must be contiguous \(2, 13, 6, 3\)'):
        Cl.check_out(out._replace(on_link=torch.zeros(N, B, 6, 4)[..., :3]), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.distance lives on cpu, the env on cuda:0'):
        Cl.check_out(out, N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        Cl.check_out(Cl.Closest(), N, cfg, spec, dev)
    with pytest.raises(ValueError, match='out.normal must be 4-byte aligned'):
        Cl.check_out(out._replace(normal=unaligned((N, B, 6, 3), torch.float32, 2)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.distance and out.which must not be the same memory'):
        Cl.check_out(out._replace(which=out.distance.view(torch.int32)), N, cfg, spec, cpu)
    with pytest.raises(ValueError, match='out.on_link and out.normal must not be the same memory'):
        Cl.check_out(out._replace(normal=out.on_link), N, cfg, spec, cpu)
    point = _lib.default_config(K.HRL_POINT_GATHER, num_envs=N)   # the point bot: B = 1
    with pytest.raises(ValueError, match=r'out.distance must be contiguous \(2, 1, 6\)'):
        Cl.check_out(out, N, point, spec, cpu)
    assert Cl.sized(spec) and Cl.size_error(spec) is None
