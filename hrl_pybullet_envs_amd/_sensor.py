"""What the bindings of the thirteen sensor libraries share (render_device.py, scan_device.py, probe_device.py, field_device.py, route_device.py,
see_device.py, frontier_device.py, camera_device.py, links_device.py, chase_device.py, dyn_device.py, cast_device.py, closest_device.py): the base of their spec records, the loader of a library, the checks of
the tensors handed in (`out=`, points), and -- for the eleven whose outputs are a record of optional members (all but render and scan) -- the
namedtuple and the ctypes record made from FIELDS, the one check of `out=` and the launch."""
import collections
import ctypes as C
import os

import torch

from . import _capi as K
from ._lib import HrlError


class Spec(C.Structure):
    """A record that starts with `struct_size`: filled in unless given; copy() is a new record with the same bytes."""

    def __init__(self, **kw):
        super().__init__(**kw)
        if 'struct_size' not in kw:
            self.struct_size = C.sizeof(type(self))

    def copy(self):
        s = type(self)()
        C.memmove(C.byref(s), C.byref(self), C.sizeof(type(self)))
        return s


def loader(path, symbols, name, what, argtypes):
    """(lib, check) of library `name` ('hrl_scan'): lib() loads the file path() names on first use, insists on every one of `symbols`, and
    sets `argtypes` (symbol -> list); check(rc) raises HrlError with the library's `<name>_last_error()`.  `what` names the sensor in the
    message about a missing file.  There is no CPU fallback: a missing library is an error."""
    loaded = []

    def lib():
        if not loaded:
            p = path()
            if not os.path.exists(p):
                raise HrlError(f'{p} is missing: build it with `python -m hrl_pybullet_envs_amd.build` '
                               f'(hipcc --offload-arch=gfx950); {what} no CPU fallback')
            L = C.CDLL(p)
            for s in symbols:
                getattr(L, s)
            getattr(L, name + '_last_error').restype = C.c_char_p
            for s, a in argtypes.items():
                getattr(L, s).argtypes = a
            loaded.append(L)
        return loaded[0]

    def check(rc):
        if rc != K.HRL_OK:
            raise HrlError(f'{name} error {rc}: {getattr(lib(), name + "_last_error")().decode()}')

    return lib, check


def check_tensors(tensors, label, fields, shapes, device, align, optional=False):
    """Every one of `tensors` is a contiguous tensor on `device`, of the dtype of its entry in `fields` ((name, dtype), ...) and the shape of
    its entry in `shapes`, its address a multiple of `align` bytes.  The messages call it label + name.  optional: a None is skipped, but at
    least one must be given.  (One loop for all of them: this runs before every launch that is handed `out=`.)"""
    none = optional
    for (name, dtype), shape, t in zip(fields, shapes, tensors):
        if t is None and optional:
            continue
        none = False
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f'{label}{name} must be a {dtype} tensor, got {getattr(t, "dtype", type(t))}')
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'{label}{name} must be contiguous {shape}, got {tuple(t.shape)}')
        if t.device != device:
            raise ValueError(f'{label}{name} lives on {t.device}, the env on {device}')
        if t.data_ptr() % align:
            raise ValueError(f'{label}{name} must be {align}-byte aligned')
    if none:
        raise ValueError('out holds no tensor: at least one output must be given')
    return tensors


def check_points(points, name, most, n, device):
    """An input of points (`points` of probe(), `starts` of route()): float32, contiguous [n, P, 2] with 1 <= P <= most, on `device`."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise TypeError(f'{name} must be a torch.float32 tensor, got {getattr(points, "dtype", type(points))}')
    if points.dim() != 3 or points.shape[0] != n or points.shape[2] != 2 or not 1 <= points.shape[1] <= most or not points.is_contiguous():
        raise ValueError(f'{name} must be contiguous [{n}, P, 2] with 1 <= P <= {most}, got {tuple(points.shape)}')
    if points.device != device:
        raise ValueError(f'{name} live on {points.device}, the env on {device}')
    return points


def out_types(name, record, fields, module):
    """(namedtuple `name` whose members default to None, ctypes Structure `record` of one c_void_p per member) of `fields`
    ((name, dtype), ...) for the binding `module` (its __name__)."""
    names = [f for f, _ in fields]
    kind = collections.namedtuple(name, names, defaults=(None,) * len(names), module=module)
    return kind, type(record, (C.Structure,), {'_fields_': [(f, C.c_void_p) for f in names], '__module__': module})


def check_out(kind, module, fields, shapes, out, device, distinct=False, note='a None member is skipped'):
    """`out=` of a record-style sensor: a `kind` (a namedtuple of binding `module`, 'links_device') whose members are None (skipped) or
    contiguous, 4-byte aligned tensors of the member's dtype (`fields`) and shape (its entry in `shapes`, N included) on `device`.  In this
    order: the type; the members in the order of `fields`, so the first offending one is named; at least one must be given; then, if
    `distinct`, no two of them (that hold anything) may be the same memory."""
    if not isinstance(out, kind):
        raise TypeError(f'out must be a {module}.{kind.__name__} ({note})')
    check_tensors(out, 'out.', fields, shapes, device, 4, optional=True)
    if distinct:
        given = [(name, t) for (name, _), t in zip(fields, out) if t is not None]
        for k, (a, x) in enumerate(given):
            for b, y in given[k + 1:]:
                if x.data_ptr() == y.data_ptr() and x.numel() and y.numel():
                    raise ValueError(f'out.{a} and out.{b} must not be the same memory')
    return out


def out_record(record, fields, out):
    """The ctypes record of output pointers (`record`: a Structure of one c_void_p per field) of the namedtuple `out`; None stays NULL."""
    return record(**{name: (None if t is None else t.data_ptr()) for (name, _), t in zip(fields, out)})


def launch(check, entry, record, fields, cfg, bufs_ref, spec, inputs, out, stream):
    """One launch of a record-style sensor: entry(cfg, buffers, spec, *inputs, the record of `out`'s pointers, stream), the library's
    hrl_<x>; `inputs` are the pointers between the spec and the outputs (the mask, and before it points, starts, clear or seen)."""
    o = out_record(record, fields, out)
    check(entry(C.byref(cfg), bufs_ref, C.byref(spec), *inputs, C.byref(o), stream))
    return out
