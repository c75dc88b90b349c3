"""The guards of the visibility map's library (libhrl_see_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_sensor_launch.py.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/see_hip.hip and csrc/see_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import see_device as V
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in V.FIELDS)


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output, to be moved or nulled by a test."""

    def __init__(self, mode='world'):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = V.default_spec(self.cfg, mode)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 64 * 64) for o in OUTPUTS}

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True):
        o = V.hrl_see_out(**self.addr)
        return V.lib().hrl_see(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), None, None, C.byref(o), None)

    def last_error(self):
        return V.lib().hrl_see_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_see: ') and phrase in why, why
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
        c.addr[output] += 1
        c.refused(f'{output} must be 4-byte aligned')
        c.addr[output] += 1
        c.refused(f'{output} must be 4-byte aligned')
    for first, second in (('visible', 'seen'), ('seen', 'fresh')):   # of two, the first in the record's order is named
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_see: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('see out holds no pointer: at least one output must be given')
    for mode in ('ego', 'ego_heading'):
        c = Call(mode)
        c.refused('see seen needs HRL_VIEW_WORLD: an ego grid moves under the memory')
        c.addr['fresh'] = None
        c.refused('see seen needs HRL_VIEW_WORLD: an ego grid moves under the memory')
    c = Call()
    c.addr['seen'] = None
    c.refused('see fresh needs seen: it counts the cells the memory did not hold')
    c = Call()
    c.addr['seen'] = c.addr['visible']
    c.refused('see visible and seen must not be the same pointer')


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, field = Call(), Other('field')
    field.refused('null buffer record', record=False)
    before = field.last_error()
    mine.addr['seen'] = None
    mine.refused('see fresh needs seen')
    assert field.last_error() == before and before.startswith('hrl_field: ')
    why = mine.last_error()
    field.bufs.struct_size = 0
    field.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_out_on_host_tensors():
    """What BatchedEnv.see hands to the binding's check, with host tensors against an env on cuda:0: the exception types that the GPU test
    `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = V.default_spec(cfg, 'world', 24, 40)
    out = V.See(torch.zeros(N, 40, 24, dtype=torch.uint8), V.memory(N, spec, cpu), torch.zeros(N, dtype=torch.int32))
    assert V.check_out(out, N, spec, cpu) is out
    assert V.check_out(V.See(seen=out.seen), N, spec, cpu).seen is out.seen   # None members are skipped
    assert V.check_out(V.See(out.visible), N, V.default_spec(cfg, 'ego', 24, 40), cpu).visible is out.visible
    with pytest.raises(TypeError, match='out must be a see_device.See'):
        V.check_out(tuple(out), N, spec, dev)
    with pytest.raises(TypeError, match='out.visible must be a torch.uint8 tensor'):
        V.check_out(out._replace(visible=out.visible.float()), N, spec, dev)
    with pytest.raises(TypeError, match='out.fresh must be a torch.int32 tensor'):
        V.check_out(out._replace(fresh=out.fresh.long()), N, spec, cpu)   # (the members before it are checked first: they have to pass)
    with pytest.raises(ValueError, match=r'out.visible must be contiguous \(2, 40, 24\)'):
        V.check_out(out._replace(visible=torch.zeros(N, 24, 40, dtype=torch.uint8)), N, spec, dev)
    with pytest.raises(ValueError, match='out.seen must be contiguous'):
        V.check_out(out._replace(seen=torch.zeros(N, 40, 48, dtype=torch.uint8)[..., ::2]), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.fresh must be contiguous \(2,\)'):
        V.check_out(out._replace(fresh=torch.zeros(N, 1, dtype=torch.int32)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.visible lives on cpu, the env on cuda:0'):
        V.check_out(out, N, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        V.check_out(V.See(), N, spec, dev)
    with pytest.raises(ValueError, match='out.seen must be 4-byte aligned'):
        V.check_out(out._replace(seen=unaligned((N, 40, 24), torch.uint8, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match="out.seen needs a spec in the 'world' mode"):
        V.check_out(out, N, V.default_spec(cfg, 'ego', 24, 40), cpu)
    with pytest.raises(ValueError, match='out.fresh needs out.seen'):
        V.check_out(out._replace(seen=None), N, spec, cpu)
    with pytest.raises(ValueError, match='out.visible and out.seen must not be the same memory'):
        V.check_out(out._replace(seen=out.visible), N, spec, cpu)
    # the members' own checks come before the three rules, in the record's order
    with pytest.raises(TypeError, match='out.visible must be a torch.uint8 tensor'):
        V.check_out(V.See(out.visible.float(), None, out.fresh), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.visible must be contiguous \(2, 40, 24\)'):
        V.check_out(V.See(torch.zeros(N, 24, 40, dtype=torch.uint8), None, out.fresh), N, spec, cpu)
    with pytest.raises(ValueError, match='out.fresh must be 4-byte aligned'):
        V.check_out(V.See(out.visible, None, unaligned((N,), torch.int32, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.visible must be 4-byte aligned'):
        V.check_out(V.See(unaligned((N, 40, 24), torch.uint8, 1), unaligned((N, 40, 24), torch.uint8, 2), out.fresh), N, spec, cpu)
    with pytest.raises(ValueError, match='out holds no tensor'):
        V.check_out(V.See(), N, V.default_spec(cfg, 'ego', 24, 40), cpu)
    assert F.MIN_SIZE == V.MIN_SIZE and F.MAX_SIZE == V.MAX_SIZE
