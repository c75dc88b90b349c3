"""The batched dynamics terms (include/hrl_dyn.h): loader of libhrl_dyn_hip.so, the ctypes mirrors of `hrl_dyn_spec` and `hrl_dyn_out`,
and the launch behind `BatchedEnv.dynamics()` -- for every env of a shard the joint-space mass matrix `mass` float32 [N, nv, nv], the
bias force `bias` [N, nv] (Coriolis, centrifugal, gravity, damping), the contact-free acceleration `accel` [N, nv] = M^-1 (tau - bias),
the linear Jacobians `jac` [N, S, 3, nv] of points fixed to the robot's bodies, the centre of mass `com` [N, 3], `momentum` [N, 6]
(linear, angular about the centre of mass) and `energy` [N, 2] (kinetic, potential), in HBM, from one kernel launch.  nv = 14 for the
ants, 6 for the point bot, in the order of the state's qvel: (v of the torso's origin, omega, joint rates).  What the reference's users
ask the simulator one env at a time through calculateMassMatrix, calculateInverseDynamics and calculateJacobian.

Like the other sensors', the library is the step library's neighbour, not a part of it.  There is no CPU fallback: a missing library is
an error."""
import ctypes as C
import os

import torch

from . import _capi as K
from . import _sensor

HRL_DYN_WORLD = 0
NV_ANT, NV_POINT, MAX_SITES = 14, 6, 16   # HRL_DYN_NV_ANT, HRL_DYN_NV_POINT, HRL_DYN_MAX_SITES

FIELDS = tuple((name, torch.float32) for name in ('mass', 'bias', 'accel', 'jac', 'com', 'momentum', 'energy'))
Dynamics, hrl_dyn_out = _sensor.out_types('Dynamics', 'hrl_dyn_out', FIELDS, __name__)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('HRL_DYN_LIB') or os.path.join(_PKG, 'libhrl_dyn_hip.so')
SYMBOLS = ['hrl_dyn_nv', 'hrl_dyn_default_spec', 'hrl_dyn', 'hrl_dyn_last_error']   # every symbol include/hrl_dyn.h declares


class hrl_dyn_spec(_sensor.Spec):
    _fields_ = [('struct_size', C.c_uint64), ('frame', C.c_int32), ('n_sites', C.c_int32), ('site_link', C.c_int32 * MAX_SITES), ('site_local', (C.c_float * 3) * MAX_SITES)]


lib, check = _sensor.loader(lambda: LIB_PATH, SYMBOLS, 'hrl_dyn', 'the batched dynamics terms have', {
    'hrl_dyn_nv': [C.c_int32],
    'hrl_dyn_default_spec': [C.POINTER(K.hrl_config), C.POINTER(hrl_dyn_spec)],
    'hrl_dyn': [C.POINTER(K.hrl_config), C.c_void_p, C.POINTER(hrl_dyn_spec), C.c_void_p, C.c_void_p, C.POINTER(hrl_dyn_out), C.c_void_p]})


def nv(kind):
    """nv: 14 for the ant kinds, 6 for the point bot (`kind`: an HRL_* env kind or an hrl_config)."""
    return NV_POINT if getattr(kind, 'env_kind', kind) == K.HRL_POINT_GATHER else NV_ANT


def default_spec(cfg, sites=None):
    """The library's default spec of `cfg`'s kind: the four foot tips as sites (the cube's centre for the point bot).  `sites`: a sequence
    of up to 16 (link, (x, y, z)) pairs -- a point fixed to a link of links_device.NAMES, in the link's frame -- instead; () for none."""
    s = hrl_dyn_spec()
    check(lib().hrl_dyn_default_spec(C.byref(cfg), C.byref(s)))
    if sites is not None:
        sites = list(sites)
        if len(sites) > MAX_SITES:
            raise ValueError(f'at most {MAX_SITES} sites, got {len(sites)}')
        s.n_sites = len(sites)
        for i in range(MAX_SITES):
            link, local = sites[i] if i < len(sites) else (0, (0.0, 0.0, 0.0))
            s.site_link[i] = int(link)
            s.site_local[i][0], s.site_local[i][1], s.site_local[i][2] = (float(v) for v in local)
    return s


def torques(cfg, actions):
    """The applied generalised force of an action, as the step applies it: float32 [N, nv] -- for the ants zeros on the six base rows and
    model.torque_scale * clip(a, -1, 1) on the joint rows (actions [N, 8]); for the point bot model.point_force * a / |a| on the force
    rows x, y (actions [N, 2])."""
    a = actions.to(torch.float32)
    tau = torch.zeros(a.shape[0], nv(cfg), dtype=torch.float32, device=a.device)
    if cfg.env_kind == K.HRL_POINT_GATHER:
        tau[:, 0:2] = a / torch.linalg.vector_norm(a, dim=1, keepdim=True) * cfg.model.point_force
    else:
        tau[:, 6:] = cfg.model.torque_scale * a.clamp(-1.0, 1.0)
    return tau


def shapes(cfg, spec, lead=()):
    """The shape after N of each member of Dynamics (with `lead` = (N,): the whole shape)."""
    n = nv(cfg)
    return (lead + (n, n), lead + (n,), lead + (n,), lead + (spec.n_sites, 3, n), lead + (3,), lead + (6,), lead + (2,))


def size_error(spec):
    """Why no tensors can be shaped after the spec (the library refuses it too), or None."""
    return None if 0 <= spec.n_sites <= MAX_SITES else f'spec.n_sites must be within 0..{MAX_SITES}, got {spec.n_sites}'


def sized(spec):
    """Whether tensors can be shaped after the spec."""
    return size_error(spec) is None


def check_tau(tau, n, cfg, device):
    """`tau=` of BatchedEnv.dynamics(): a contiguous, 4-byte aligned float32 tensor [N, nv] on the env's device."""
    return _sensor.check_tensors((tau,), '', (('tau', torch.float32),), ((n, nv(cfg)),), device, 4)[0]


def dynamics(cfg, bufs_ref, spec, tau_ptr, mask_ptr, out, stream):
    """One launch: the tensors of `out` (a Dynamics; a None one is not computed) on the current device, from the buffer record behind
    `bufs_ref`."""
    return _sensor.launch(check, lib().hrl_dyn, hrl_dyn_out, FIELDS, cfg, bufs_ref, spec, (tau_ptr, mask_ptr), out, stream)


def check_out(out, n, cfg, spec, device, tau=None):
    """`out=` of BatchedEnv.dynamics(): a Dynamics whose members are None (skipped) or contiguous, 4-byte aligned float32 tensors -- mass
    [N, nv, nv], bias, accel [N, nv], jac [N, n_sites, 3, nv], com [N, 3], momentum [N, 6], energy [N, 2] -- on the env's device, no two
    of them the same memory, none of them `tau`'s; at least one must be given."""
    _sensor.check_out(Dynamics, 'dyn_device', FIELDS, shapes(cfg, spec, (n,)), out, device, distinct=True)
    if out.jac is not None and spec.n_sites == 0:
        raise ValueError('out.jac is given and the spec holds no site')
    if tau is not None:
        for (name, _), t in zip(FIELDS, out):
            if t is not None and t.numel() and t.data_ptr() == tau.data_ptr():
                raise ValueError(f'out.{name} and tau must not be the same memory')
    return out
