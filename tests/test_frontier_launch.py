"""The guards of the frontier map's library (libhrl_frontier_hip.so) that return before a device is looked for, and what its Python binding
refuses before it calls, in the form of test_see_launch.py.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/frontier_hip.hip and
csrc/frontier_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import frontier_device as X
from hrl_pybullet_envs_amd import see_device as V
from test_sensor_launch import BASE, N, STRUCT_SIZE, unaligned
from test_sensor_launch import Call as Other

OUTPUTS = tuple(n for n, _ in X.FIELDS)


class Call:
    """One launch on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are refused first).  `addr`:
    the address of each output and of `seen`, to be moved or nulled by a test."""

    def __init__(self):
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = X.default_spec(self.cfg)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 64 * 64 * 4) for o in OUTPUTS + ('seen',)}

    def room(self, nbytes):
        a = np.full(nbytes + 128, 0x7B, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True):
        o = X.hrl_frontier_out(**{k: v for k, v in self.addr.items() if k != 'seen'})
        return X.lib().hrl_frontier(C.byref(self.cfg), C.byref(self.bufs) if record else None, C.byref(self.spec), self.addr['seen'], None, C.byref(o), None)

    def last_error(self):
        return X.lib().hrl_frontier_last_error().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith('hrl_frontier: ') and phrase in why, why
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


def test_output_and_memory_guards():
    for name in OUTPUTS + ('seen',):
        c = Call()
        c.addr[name] += 1
        c.refused(f'{name} must be 4-byte aligned')
        c.addr[name] += 1
        c.refused(f'{name} must be 4-byte aligned')
    for first, second in (('edge', 'seen'), ('cell', 'seen'), ('dist', 'goal')):   # of two, the first in the record's order is named; `seen` comes last
        c = Call()
        c.addr[first] += 2
        c.addr[second] += 1
        c.refused(f'{first} must be 4-byte aligned')
        assert c.last_error() == f'hrl_frontier: {first} must be 4-byte aligned'
    c = Call()
    for output in OUTPUTS:
        c.addr[output] = None
    c.refused('frontier out holds no pointer: at least one output must be given')
    c = Call()
    c.addr['seen'] = None
    c.refused('frontier seen is null: the memory of hrl_see is required')
    for output in ('edge', 'parent'):
        c = Call()
        c.addr['seen'] = c.addr[output]
        c.refused('frontier seen must not be the memory of edge or parent: it is only read')
    c = Call()
    c.spec.unknown = 2
    c.refused('frontier unknown must be HRL_FRONTIER_KNOWN_ONLY or HRL_FRONTIER_OPTIMISTIC')
    c = Call()
    c.spec.sources = 128
    c.refused('frontier sources must be a non-empty mask of HRL_FRONTIER_EDGE | HRL_FIELD_ROBOT | HRL_SCAN_FOOD | POISON | TARGET')
    c = Call()
    c.spec.width = 12
    c.refused('frontier field width must be a multiple of 8 within 8..64')


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string."""
    mine, field = Call(), Other('field')
    field.refused('null buffer record', record=False)
    before = field.last_error()
    mine.addr['seen'] = None
    mine.refused('frontier seen is null')
    assert field.last_error() == before and before.startswith('hrl_field: ')
    why = mine.last_error()
    field.bufs.struct_size = 0
    field.refused(STRUCT_SIZE)
    assert mine.last_error() == why


def test_check_seen_and_check_out_on_host_tensors():
    """What BatchedEnv.frontier hands to the binding's checks, with host tensors against an env on cuda:0: the exception types that the GPU
    test `test_out_is_reused_and_checked` expects, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
    spec = X.default_spec(cfg, 24, 40)
    seen = V.memory(N, V.default_spec(cfg, 'world', 24, 40), cpu)
    grid = lambda dt: torch.zeros(N, 40, 24, dtype=dt)
    out = X.Frontier(grid(torch.uint8), grid(torch.float32), grid(torch.uint8), torch.zeros(N, dtype=torch.int32), torch.zeros(N), torch.zeros(N, 2), torch.zeros(N, dtype=torch.int32))
    assert X.check_seen(seen, N, spec, cpu) is seen
    assert X.check_out(out, N, spec, cpu, seen) is out
    assert X.check_out(X.Frontier(goal=out.goal), N, spec, cpu, seen).goal is out.goal   # None members are skipped
    with pytest.raises(TypeError, match='seen must be a torch.uint8 tensor'):
        X.check_seen(seen.float(), N, spec, cpu)
    with pytest.raises(TypeError, match='seen must be a torch.uint8 tensor'):
        X.check_seen(None, N, spec, cpu)
    with pytest.raises(ValueError, match=r'seen must be contiguous \(2, 40, 24\)'):
        X.check_seen(torch.zeros(N, 24, 40, dtype=torch.uint8), N, spec, cpu)
    with pytest.raises(ValueError, match='seen lives on cpu, the env on cuda:0'):
        X.check_seen(seen, N, spec, dev)
    with pytest.raises(ValueError, match='seen must be 4-byte aligned'):
        X.check_seen(unaligned((N, 40, 24), torch.uint8, 2), N, spec, cpu)
    with pytest.raises(TypeError, match='out must be a frontier_device.Frontier'):
        X.check_out(tuple(out), N, spec, dev)
    with pytest.raises(TypeError, match='out.edge must be a torch.uint8 tensor'):
        X.check_out(out._replace(edge=out.edge.float()), N, spec, dev)
    with pytest.raises(TypeError, match='out.cell must be a torch.int32 tensor'):
        X.check_out(out._replace(cell=out.cell.long()), N, spec, cpu)   # (the members before it are checked first: they have to pass)
    with pytest.raises(ValueError, match=r'out.dist must be contiguous \(2, 40, 24\)'):
        X.check_out(out._replace(dist=torch.zeros(N, 24, 40)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.parent must be contiguous'):
        X.check_out(out._replace(parent=torch.zeros(N, 40, 48, dtype=torch.uint8)[..., ::2]), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.goal must be contiguous \(2, 2\)'):
        X.check_out(out._replace(goal=torch.zeros(N, 3)), N, spec, cpu)
    with pytest.raises(ValueError, match=r'out.count must be contiguous \(2,\)'):
        X.check_out(out._replace(count=torch.zeros(N, 1, dtype=torch.int32)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.edge lives on cpu, the env on cuda:0'):
        X.check_out(out, N, spec, dev)
    with pytest.raises(ValueError, match='out holds no tensor'):
        X.check_out(X.Frontier(), N, spec, dev)
    with pytest.raises(ValueError, match='out.parent must be 4-byte aligned'):
        X.check_out(out._replace(parent=unaligned((N, 40, 24), torch.uint8, 2)), N, spec, cpu)
    with pytest.raises(ValueError, match='out.edge and seen must not be the same memory'):
        X.check_out(out._replace(edge=seen), N, spec, cpu, seen)
    with pytest.raises(ValueError, match='out.parent and seen must not be the same memory'):
        X.check_out(out._replace(parent=seen), N, spec, cpu, seen)
    with pytest.raises(ValueError, match='out.cell must be 4-byte aligned'):   # every member's own check comes before the rule about `seen`
        X.check_out(out._replace(edge=seen, cell=unaligned((N,), torch.int32, 2)), N, spec, cpu, seen)
    assert F.MIN_SIZE == X.MIN_SIZE and F.MAX_SIZE == X.MAX_SIZE
