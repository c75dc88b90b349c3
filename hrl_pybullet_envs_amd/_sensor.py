"""What the bindings of the sensor libraries share (render_device.py, scan_device.py, probe_device.py, field_device.py, route_device.py, see_device.py, frontier_device.py, camera_device.py): the base of their
spec records, the loader of a library, the check of the tensors handed in as `out=`, and the record of output pointers."""
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


def check_tensors(tensors, label, fields, shape, device, align, optional=False):
    """Every one of `tensors` is a contiguous tensor of `shape` on `device`, of the dtype of its entry in `fields` ((name, dtype), ...), its
    address a multiple of `align` bytes.  The messages call it label + name.  optional: a None is skipped, but at least one must be given.
    (One loop for all of them: this runs before every launch that is handed `out=`.)"""
    none = optional
    for (name, dtype), t in zip(fields, tensors):
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


def out_record(record, fields, out):
    """The ctypes record of output pointers (`record`: a Structure of one c_void_p per field) of the namedtuple `out`; None stays NULL."""
    return record(**{name: (None if t is None else t.data_ptr()) for (name, _), t in zip(fields, out)})
