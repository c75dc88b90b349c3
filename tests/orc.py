"""ctypes binding of the CPU oracle (oracle/liborc.so).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from hrl_pybullet_envs_amd import _capi as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        asan = bool(os.environ.get('HRL_ORC_ASAN'))   # the AddressSanitizer + UBSan build (tests/test_emu_asan.py preloads libasan; no OpenMP in it)
        path = os.path.join(ROOT, 'oracle', 'liborc_asan.so' if asan else 'liborc.so')
        if asan or not os.path.exists(path):
            subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle'), os.path.basename(path)])
        _LIB = C.CDLL(path)
        if asan:
            _LIB.omp_set_num_threads(1)
        elif 'OMP_NUM_THREADS' not in os.environ:
            # OpenMP's default team is one thread per VISIBLE cpu; a GPU box shows all of the host's and grants a 16-core share, and a team
            # several times the share spends its time spinning at the barrier of every batch call (88 s instead of 1 s for 700 small steps)
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            _LIB.omp_set_num_threads(max(1, min(ncpu, 16)))
        _LIB.orc_sq_dist_f64.restype = C.c_double
        _LIB.orc_sq_dist_f32.restype = C.c_float
    return _LIB


def suffix(dtype):
    return '_f64' if np.dtype(dtype) == np.float64 else '_f32'


def fn(name, dtype=np.float64):
    return getattr(lib(), name + suffix(dtype))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def creal(dtype):
    return C.c_double if np.dtype(dtype) == np.float64 else C.c_float


def default_config(kind, **over):
    cfg = K.hrl_config()
    lib().orc_default_config(C.c_int32(kind), C.byref(cfg))
    for k, v in over.items():
        if k.startswith('model_'):
            setattr(cfg.model, k[6:], v)
        elif k == 'world_size':
            cfg.world_size[0], cfg.world_size[1] = v
        elif k == 'targets':
            cfg.n_targets = len(v)
            for i, t in enumerate(v):
                cfg.targets[i][0], cfg.targets[i][1] = float(t[0]), float(t[1])
        else:
            setattr(cfg, k, v)
    return cfg


def obs_dim(cfg):
    return lib().orc_obs_dim(C.byref(cfg))


def act_dim(cfg):
    return lib().orc_act_dim(C.byref(cfg))


def items_stride(cfg):
    return lib().orc_items_stride(C.byref(cfg))


class OracleEnv:
    """Batched env on host numpy buffers with the device buffer layout (include/hrl_envs.h)."""

    def __init__(self, cfg, dtype=np.float32):
        self.cfg, self.dtype = cfg, np.dtype(dtype)
        n = cfg.num_envs
        self.N, self.od, self.ad = n, obs_dim(cfg), act_dim(cfg)
        self.state = np.zeros((n, K.HRL_STATE_STRIDE), self.dtype)
        self.items = np.zeros((n, items_stride(cfg)), self.dtype)
        self.aux = np.zeros((n, K.HRL_AUX_STRIDE), np.int32)
        self.obs = np.zeros((n, self.od), self.dtype)
        self.rew = np.zeros(n, self.dtype)
        self.done = np.zeros(n, np.uint8)
        self.info = np.zeros((n, K.HRL_INFO_STRIDE), self.dtype)
        self.final_obs = np.zeros((n, self.od), self.dtype)
        self.truncated = np.zeros(n, np.uint8)
        self.goal = np.zeros((n, K.HRL_GOAL_STRIDE), self.dtype)
        self.solver_rows = np.zeros(n, np.int32)

    def reset(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        fn('orc_reset_batch', self.dtype)(C.byref(self.cfg), ptr(self.state), ptr(self.items), ptr(self.aux), ptr(m),
                                          ptr(self.obs))
        return self.obs

    def step(self, actions):
        a = np.ascontiguousarray(actions, self.dtype).reshape(self.N, self.ad)
        fn('orc_step_batch_v7', self.dtype)(C.byref(self.cfg), ptr(self.state), ptr(self.items), ptr(self.aux), ptr(a),
                                            ptr(self.obs), ptr(self.rew), ptr(self.done), ptr(self.info), ptr(self.final_obs),
                                            ptr(self.truncated), ptr(self.goal), ptr(self.solver_rows))
        return self.obs, self.rew, self.done, self.info

    def observe(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        fn('orc_observe_batch', self.dtype)(C.byref(self.cfg), ptr(self.state), ptr(self.items), ptr(self.aux), ptr(m), ptr(self.obs))
        return self.obs

    def set_goals(self, goals, mask=None):
        """AntFlagrun with flag_manual_goals: `env.goals = [...]; env.next_target()`, goals [N, n_goals, 2]"""
        g = np.ascontiguousarray(goals, self.dtype)
        fn('orc_set_goals_batch', self.dtype)(C.byref(self.cfg), ptr(self.state), ptr(self.items), ptr(self.aux), ptr(g), g.shape[1], ptr(mask), ptr(self.obs))

    def next_target(self, mask=None):
        """`env.next_target()` of every (masked) env; ok[i] == 0 where the reference raises IndexError, 1 where mask[i] == 0"""
        ok = np.ones(self.N, np.uint8)
        fn('orc_next_target_batch', self.dtype)(C.byref(self.cfg), ptr(self.state), ptr(self.items), ptr(self.aux), ptr(mask), ptr(self.obs), ptr(ok))
        return ok

    @property
    def qpos(self):
        return self.state[:, :15]

    @property
    def qvel(self):
        return self.state[:, 15:29]
