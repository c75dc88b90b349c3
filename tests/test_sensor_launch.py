"""The guards that the nine sensor libraries share (csrc/sensor_launch.h, _sensor.py), on the first four of them
(libhrl_{render,scan,probe,field}_hip.so; the others have test_route_host.py and test_{see,frontier,camera,links}_launch.py in this form):
what their launchers refuse before they look for a device, and what the Python bindings refuse before they call.  CPU only: every call below returns before the HIP runtime is asked
anything, so the results are the same with and without a GPU.  The phrases are copied from csrc/*_hip.hip and csrc/*_core.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from hrl_pybullet_envs_amd import _capi as K
from hrl_pybullet_envs_amd import _lib
from hrl_pybullet_envs_amd import field_device as F
from hrl_pybullet_envs_amd import probe_device as P
from hrl_pybullet_envs_amd import render_device as R
from hrl_pybullet_envs_amd import scan_device as S

N = 2
BASE = 8 + 8 * 8   # HRL_BUFFERS_SIZE_V7_BASE: struct_size and the eight pointers through `info`
NAMES = ('render', 'scan', 'probe', 'field')
MODULES = {'render': R, 'scan': S, 'probe': P, 'field': F}
OUTPUTS = {'render': ('rgb',), 'scan': ('range', 'hit'), 'probe': tuple(n for n, _ in P.FIELDS), 'field': tuple(n for n, _ in F.FIELDS)}
NULL_RECORD = {'render': 'null state, aux or rgb', 'scan': 'null state, aux, range or hit', 'probe': 'null state or aux', 'field': 'null state or aux'}
EMPTY_OUT = {'probe': 'probe out holds no pointer: at least one output must be given', 'field': 'field out holds no pointer: at least one output must be given'}
STRUCT_SIZE = 'hrl_buffers.struct_size is not the size of a known layout: initialise the record with hrl_buffers_init() (include/hrl_envs.h)'


def misaligned(name, output):
    if name == 'render':
        return 8, 'rgb must be 16-byte aligned (a strip of 16 pixels is stored as three 16-byte vectors)'
    return 1, 'range and hit must be 4-byte aligned' if name == 'scan' else f'{output} must be 4-byte aligned'


class Call:
    """One launch of library `name` on 2 envs of the flat kind with host memory behind every pointer (none is read: the calls are
    refused first).  `addr`: the address of each output and of `points`, to be moved or nulled by a test."""

    def __init__(self, name):
        self.name, self.mod = name, MODULES[name]
        self.cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)
        self.spec = R.default_view(self.cfg) if name == 'render' else self.mod.default_spec(self.cfg)
        self.keep = [np.zeros(N * K.HRL_STATE_STRIDE, np.float32), np.zeros(N * K.HRL_AUX_STRIDE, np.int32)]
        self.bufs = K.make_buffers(self.keep[0].ctypes.data, None, self.keep[1].ctypes.data, None, None, None, None, None)
        self.addr = {o: self.room(N * 64 * 64 * 4) for o in OUTPUTS[name] + ('points',)}

    def room(self, nbytes):
        a = np.zeros(nbytes + 128, np.uint8)
        self.keep.append(a)
        return (a.ctypes.data + 63) // 64 * 64

    def __call__(self, record=True):
        L, a, b = self.mod.lib(), self.addr, C.byref(self.bufs) if record else None
        if self.name == 'render':
            return L.hrl_render(C.byref(self.cfg), b, C.byref(self.spec), None, a['rgb'], None)
        if self.name == 'scan':
            return L.hrl_scan(C.byref(self.cfg), b, C.byref(self.spec), None, a['range'], a['hit'], None)
        if self.name == 'probe':
            o = P.hrl_probe_out(**{n: a[n] for n in OUTPUTS['probe']})
            return L.hrl_probe(C.byref(self.cfg), b, C.byref(self.spec), a['points'], None, C.byref(o), None)
        o = F.hrl_field_out(**{n: a[n] for n in OUTPUTS['field']})
        return L.hrl_field(C.byref(self.cfg), b, C.byref(self.spec), None, C.byref(o), None)

    def last_error(self):
        return getattr(self.mod.lib(), f'hrl_{self.name}_last_error')().decode()

    def refused(self, phrase, **kw):
        assert self(**kw) == K.HRL_ERR_BAD_ARG
        why = self.last_error()
        assert why.startswith(f'hrl_{self.name}: ') and phrase in why, why


@pytest.mark.parametrize('name', NAMES)
def test_buffer_record_guards(name):
    c = Call(name)
    c.refused('null buffer record', record=False)
    for size in (0, BASE - 8, 4104, BASE + 4):
        c.bufs.struct_size = size
        c.refused(STRUCT_SIZE)
    for member in ('state', 'aux'):
        c = Call(name)
        setattr(c.bufs, member, None)
        c.refused(NULL_RECORD[name])


@pytest.mark.parametrize('name', NAMES)
def test_output_guards(name):
    for output in OUTPUTS[name]:
        c = Call(name)
        by, phrase = misaligned(name, output)
        c.addr[output] += by
        c.refused(phrase)
        if name in ('render', 'scan'):
            c.addr[output] = None
            c.refused(NULL_RECORD[name])
    if name in EMPTY_OUT:
        c = Call(name)
        for output in OUTPUTS[name]:
            c.addr[output] = None
        c.refused(EMPTY_OUT[name])


def test_probe_points_guards():
    c = Call('probe')
    c.addr['points'] += 4
    c.refused('points must be 8-byte aligned')
    c.addr['points'] = None
    c.refused('null points')
    for output in OUTPUTS['probe']:   # `points` is looked at before the outputs
        c = Call('probe')
        c.addr['points'] += 4
        c.addr[output] += 1
        c.refused('points must be 8-byte aligned')
        assert c.last_error() == 'hrl_probe: points must be 8-byte aligned'
        c.addr['points'] = None
        c.refused('null points')
    c = Call('probe')   # and of two outputs the first in the record's order is named
    c.addr['clearance'] += 2
    c.addr['via'] += 1
    c.refused('clearance must be 4-byte aligned')
    assert c.last_error() == 'hrl_probe: clearance must be 4-byte aligned'
    c = Call('field')
    c.addr['dist'] += 2
    c.addr['parent'] += 1
    c.refused('dist must be 4-byte aligned')
    assert c.last_error() == 'hrl_field: dist must be 4-byte aligned'


def test_a_refusal_stays_in_its_own_library():
    """The libraries live in one process; each keeps its own error string (four of the nine here)."""
    calls = {name: Call(name) for name in NAMES}
    for c in calls.values():
        c.refused('null buffer record', record=False)
    before = {name: c.last_error() for name, c in calls.items()}
    calls['scan'].bufs.struct_size = 0
    calls['scan'].refused(STRUCT_SIZE)
    for name in ('render', 'probe', 'field'):
        assert calls[name].last_error() == before[name] and before[name].startswith(f'hrl_{name}: ')


def unaligned(shape, dtype, by=1):
    """A contiguous CPU tensor whose address is `by` bytes past a multiple of 64."""
    count = int(np.prod(shape))
    raw = bytearray(count * torch.empty(0, dtype=dtype).element_size() + 128)
    at = -C.addressof(C.c_char.from_buffer(raw)) % 64 + by
    t = torch.frombuffer(raw, dtype=dtype, count=count, offset=at).reshape(shape)
    assert t.data_ptr() % 64 == by and t.is_contiguous()
    return t


def test_check_out_and_check_points():
    """What BatchedEnv hands to the bindings' checks, with host tensors against an env on cuda:0: the exception types that the GPU tests
    `test_out_is_reused_and_checked` expect, and their texts."""
    dev, cpu = torch.device('cuda:0'), torch.device('cpu')
    cfg = _lib.default_config(K.HRL_ANT_FLAT, num_envs=N)

    view = R.hrl_view(width=32, height=48, mode=R.HRL_VIEW_WORLD, half_extent=5.0)
    good = torch.zeros(N, 48, 32, 3, dtype=torch.uint8)
    assert R.check_out(good, N, view, cpu) is good
    with pytest.raises(TypeError, match='out must be a torch.uint8 tensor'):
        R.check_out(good.float(), N, view, dev)
    with pytest.raises(TypeError, match='out must be a torch.uint8 tensor'):
        R.check_out(None, N, view, dev)
    with pytest.raises(ValueError, match=r'out must be contiguous \(2, 48, 32, 3\)'):
        R.check_out(torch.zeros(N, 32, 48, 3, dtype=torch.uint8), N, view, dev)
    with pytest.raises(ValueError, match='out must be contiguous'):
        R.check_out(torch.zeros(N, 48, 32, 6, dtype=torch.uint8)[..., ::2], N, view, dev)
    with pytest.raises(ValueError, match='out lives on cpu, the env on cuda:0'):
        R.check_out(good, N, view, dev)
    with pytest.raises(ValueError, match='out must be 16-byte aligned'):
        R.check_out(unaligned((N, 48, 32, 3), torch.uint8, 8), N, view, cpu)

    spec = S.default_spec(cfg, 'world', 37)
    rng, hit = torch.zeros(N, 37), torch.zeros(N, 37, dtype=torch.int32)
    assert S.check_out((rng, hit), N, spec, cpu) == (rng, hit)
    with pytest.raises(TypeError, match='out must be a pair'):
        S.check_out(rng, N, spec, dev)
    with pytest.raises(TypeError, match='out hit must be a torch.int32 tensor'):
        S.check_out((rng, hit.float()), N, spec, cpu)   # (range is checked first: it has to pass)
    with pytest.raises(TypeError, match='out range must be a torch.float32 tensor'):
        S.check_out((rng.int(), hit), N, spec, dev)
    with pytest.raises(ValueError, match=r'out range must be contiguous \(2, 37\)'):
        S.check_out((torch.zeros(N, 64), hit), N, spec, dev)
    with pytest.raises(ValueError, match='out hit must be contiguous'):
        S.check_out((rng, torch.zeros(N, 74, dtype=torch.int32)[:, ::2]), N, spec, cpu)
    with pytest.raises(ValueError, match='out range lives on cpu, the env on cuda:0'):
        S.check_out((rng, hit), N, spec, dev)
    with pytest.raises(ValueError, match='out hit must be 4-byte aligned'):   # (the library refuses it too, later)
        S.check_out((rng, unaligned((N, 37), torch.int32)), N, spec, cpu)

    pts = torch.zeros(N, 5, 2)
    assert P.check_points(pts, N, cpu) is pts
    with pytest.raises(TypeError, match='points must be a torch.float32 tensor'):
        P.check_points(pts.double(), N, dev)
    for bad in (torch.zeros(N, 5, 3), torch.zeros(N + 1, 5, 2), torch.zeros(N, 0, 2), torch.zeros(N, P.MAX_POINTS + 1, 2), torch.zeros(N, 5, 4)[:, :, ::2]):
        with pytest.raises(ValueError, match=r'points must be contiguous \[2, P, 2\]'):
            P.check_points(bad, N, dev)
    with pytest.raises(ValueError, match='points live on cpu, the env on cuda:0'):
        P.check_points(pts, N, dev)

    for M, kind, spec, shape in ((P, P.Probe, P.default_spec(cfg, 'world', 5), (N, 5)), (F, F.Field, F.default_spec(cfg, 'world', 24, 40), (N, 40, 24))):
        out = kind(*(torch.zeros(shape, dtype=dt) for _, dt in M.FIELDS))
        assert M.check_out(out, N, spec, cpu) is out
        first, fdt = M.FIELDS[0]
        last, ldt = M.FIELDS[-1]
        assert M.check_out(kind(**{last: out[-1]}), N, spec, cpu)[-1] is out[-1]   # None members are skipped
        with pytest.raises(TypeError, match='out must be a'):
            M.check_out(tuple(out), N, spec, dev)
        with pytest.raises(TypeError, match=f'out.{first} must be a torch.float32 tensor'):
            M.check_out(out._replace(**{first: out[0].double()}), N, spec, dev)
        with pytest.raises(TypeError, match=f'out.{last} must be a {ldt} tensor'):
            M.check_out(out._replace(**{last: out[-1].long()}), N, spec, cpu)   # (the members before it are checked first: they have to pass)
        with pytest.raises(ValueError, match=f'out.{first} must be contiguous'):
            M.check_out(out._replace(**{first: torch.zeros(shape[::-1])}), N, spec, dev)
        with pytest.raises(ValueError, match=f'out.{first} must be contiguous'):
            M.check_out(out._replace(**{first: torch.zeros(shape[:-1] + (2 * shape[-1],))[..., ::2]}), N, spec, dev)
        with pytest.raises(ValueError, match=f'out.{first} lives on cpu, the env on cuda:0'):
            M.check_out(out, N, spec, dev)
        with pytest.raises(ValueError, match='out holds no tensor'):
            M.check_out(kind(), N, spec, dev)
        with pytest.raises(ValueError, match=f'out.{first} must be 4-byte aligned'):   # (probe: the library refuses it too, later)
            M.check_out(out._replace(**{first: unaligned(shape, fdt)}), N, spec, cpu)
