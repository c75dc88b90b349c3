"""The two implementations under test behind the buffer names and call shapes of tests/orc.py::OracleEnv, so that one scenario (tests/parity_cases.py,
the fuzz tools, the fixture replay, the fingerprint) drives the oracle and any of them alike:

    Emu     the wave phases on the lock-step host executor (tests/emu_env.py) -- runs anywhere
    Device  the HIP kernels through BatchedEnv(cfg, 'cuda:0'), the public path -- needs an MI355X

    state items aux obs rew done info final_obs truncated [goal, solver_rows]   numpy arrays;   N od ad cfg
    reset(mask=None)  step(a)  observe(mask=None)  set_goals(goals, mask=None)  next_target(mask=None) -> ok  push(o)  fill(name, v)  close()
    give_items(given)                                                           an items record or NULL in the buffer record
    set(qpos, qvel, items=None, aux3=None, initial_z=None)                      the teleport of tests/golden_replay.py

Importing this module needs no GPU: torch and the HIP library are loaded by Device() only.  Test infrastructure only."""
import ctypes as C

import numpy as np

import emu_env
import orc
from hrl_pybullet_envs_amd import _capi as K

ALL = ('state', 'items', 'aux', 'obs', 'rew', 'done', 'info', 'final_obs', 'truncated')


def same(o, b, tag='', names=ALL):
    """every named buffer of `b` equals `o`'s bit for bit (NaNs as equal)"""
    for name in names:
        x, y = getattr(o, name), getattr(b, name)
        assert np.array_equal(x, y, equal_nan=True), (tag, name, np.argwhere(~((x == y) | ((x != x) & (y != y))))[:4].tolist())


def _rec(o, name):   # the oracle itself, or one recorded step of tests/contacts_cases.py (a dict of read-only arrays)
    return o[name] if isinstance(o, dict) else getattr(o, name)


class Emu(emu_env.EmuEnv):
    def __init__(self, cfg, reverse=False, asan=False):
        msg = emu_env.lib(asan).emu_validate(C.byref(cfg))
        if msg:
            raise ValueError(msg.decode())
        super().__init__(cfg, reverse=reverse, asan=asan)

    @staticmethod
    def config(kind, **over):
        a = K.hrl_config(); emu_env.lib().emu_default_config(kind, C.byref(a))
        assert bytes(a) == bytes(orc.default_config(kind))   # product defaults (the headers' host build) == oracle defaults
        return orc.default_config(kind, **over)

    def push(self, o):
        self.state[...] = _rec(o, 'state'); self.items[...] = _rec(o, 'items'); self.aux[...] = _rec(o, 'aux')

    def fill(self, name, v):
        getattr(self, name)[...] = v

    def set(self, qpos, qvel, items=None, aux3=None, initial_z=None):
        self.state[:, 0:15] = qpos; self.state[:, 15:29] = qvel
        if initial_z is not None:
            self.state[:, K.HRL_INITZ_OFF] = initial_z
        if items is not None:
            self.items[:, :items.shape[1]] = items
        if aux3 is not None:
            self.aux[:, 3] = aux3

    def set_goals(self, goals, mask=None):
        goals = np.ascontiguousarray(goals, np.float32)
        if emu_env.lib(self.asan).emu_set_goals(C.byref(self.cfg), C.byref(self._bufs()), orc.ptr(goals), goals.shape[1], orc.ptr(mask), self.reverse) != 0:
            raise ValueError('emu_set_goals refused')

    def next_target(self, mask=None):
        ok = np.ones(self.N, np.uint8)
        assert emu_env.lib(self.asan).emu_next_target(C.byref(self.cfg), C.byref(self._bufs()), orc.ptr(mask), orc.ptr(ok), self.reverse) == 0
        return ok

    def give_items(self, given):
        """hand the step an items record (True) or NULL (False): only the kinds that keep nothing there may go without"""
        self.null_items = not given

    def close(self):
        pass


class Device:
    def __init__(self, cfg, count_rows=False):
        import torch
        from hrl_pybullet_envs_amd.vec_env import BatchedEnv
        self.t, self.env, self.cfg = torch, BatchedEnv(cfg, 'cuda:0'), cfg
        self.N, self.od, self.ad = cfg.num_envs, self.env.obs_dim, self.env.act_dim
        if count_rows:
            self.env.count_solver_rows()

    @staticmethod
    def config(kind, **over):
        # torch before the library, as hrl_pybullet_envs_amd.vec_env has it: the library then binds to the HIP runtime torch brought.  Loaded on its
        # own first, in a process that imports torch afterwards, its hipGetDeviceCount has come back empty (`hrl_create: no HIP device`)
        import torch  # noqa: F401
        from hrl_pybullet_envs_amd import _lib
        cfg = _lib.default_config(kind, **over)
        assert bytes(cfg) == bytes(orc.default_config(kind, **over))   # product defaults == oracle defaults
        return cfg

    def _dev(self, a):
        return None if a is None else self.t.tensor(a).cuda()   # (a copy first: recorded traces are read-only arrays)

    def __getattr__(self, name):
        if name not in ALL + ('goal', 'solver_rows'):
            raise AttributeError(name)
        a = getattr(self.env, 'reward' if name == 'rew' else name).cpu().numpy()
        # the kinds that keep nothing in the items record hand the library NULL for it (BatchedEnv._uses_items): whatever push() left in the tensor
        # is never read or written by a launch, and the oracle's record of such a kind stays zero
        return np.zeros_like(a) if name == 'items' and self.env._bufs.items is None else a

    def reset(self, mask=None):
        self.env.reset(self._dev(mask))

    def step(self, a):
        self.env.step(self._dev(a))

    def observe(self, mask=None):
        return self.env.observe(self._dev(mask)).cpu().numpy()

    def push(self, o):
        e = self.env
        e.state.copy_(self._dev(_rec(o, 'state'))); e.items.copy_(self._dev(_rec(o, 'items'))); e.aux.copy_(self._dev(_rec(o, 'aux')))

    def fill(self, name, v):
        getattr(self.env, 'reward' if name == 'rew' else name).fill_(v)

    def set(self, qpos, qvel, items=None, aux3=None, initial_z=None):
        e = self.env
        if initial_z is not None:
            e.state[:, K.HRL_INITZ_OFF] = initial_z
        if items is not None:
            e.items[:, :items.shape[1]] = self._dev(items)
        if aux3 is not None:
            e.aux[:, 3] = self._dev(aux3)
        e.set_state(self._dev(qpos), self._dev(qvel), observe=False)   # hrl_set_state

    def set_goals(self, goals, mask=None):
        self.env.set_goals(self._dev(goals), self._dev(mask))

    def next_target(self, mask=None):
        return self.env.next_target(self._dev(mask))[1].cpu().numpy()

    def give_items(self, given):
        """hand the library an items record (True) or NULL (False) through the C ABI's buffer record"""
        e = self.env
        assert given or not e._uses_items
        e._bufs.items = e.items.data_ptr() if given else None

    def close(self):
        self.env.close()
