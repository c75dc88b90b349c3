"""Batched environment on one GPU: torch-ROCm tensors for storage and streams, the HIP C-ABI for the step.

Mirrors the reference's Env API batched over N envs (README.md:24-34):
    obs = env.reset(); obs, rew, done, info = env.step(actions)
All tensors stay resident in HBM.  Layout: include/hrl_envs.h.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi as K
from . import _lib


class BatchedEnv:
    def __init__(self, cfg, device='cuda:0'):
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise _lib.HrlError('BatchedEnv needs an MI355X (torch.cuda.is_available() is False or a CPU device was '
                                'requested): the env step has no CPU path')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        L = _lib.lib()
        self.num_envs = cfg.num_envs
        self.obs_dim, self.act_dim = L.hrl_obs_dim(C.byref(cfg)), L.hrl_act_dim(C.byref(cfg))
        self.items_stride = L.hrl_items_stride(C.byref(cfg))  # 32 unless the config holds more than 16 items / 15 manual goals
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            _lib.check(L.hrl_create(C.byref(cfg), C.byref(h)))
        self._h = h
        n, dev, f32 = self.num_envs, self.device, torch.float32
        self.state = torch.zeros(n, K.HRL_STATE_STRIDE, dtype=f32, device=dev)
        self.items = torch.zeros(n, self.items_stride, dtype=f32, device=dev)
        self.aux = torch.zeros(n, K.HRL_AUX_STRIDE, dtype=torch.int32, device=dev)
        # the step's outputs; `final_obs` = the observation of the step that ended an episode (rows of envs that did not finish keep their
        # last terminal observation) and `truncated` = the step limit alone ended it: what a trainer bootstraps a truncated episode from
        # (include/hrl_envs.h).  Read them through the properties below: after step_host() they are refreshed from the host buffers first.
        self._out = {'obs': torch.zeros(n, self.obs_dim, dtype=f32, device=dev), 'reward': torch.zeros(n, dtype=f32, device=dev),
                     'done': torch.zeros(n, dtype=torch.uint8, device=dev), 'info': torch.zeros(n, K.HRL_INFO_STRIDE, dtype=f32, device=dev),
                     'final_obs': torch.zeros(n, self.obs_dim, dtype=f32, device=dev), 'truncated': torch.zeros(n, dtype=torch.uint8, device=dev)}
        if cfg.env_kind == K.HRL_ANT_FLAGRUN:  # the goal being chased and whether this step switched to it: info['target'] (ant_flagrun_env.py:191,199)
            self._out['goal'] = torch.zeros(n, K.HRL_GOAL_STRIDE, dtype=f32, device=dev)
        self._host = None         # pinned host buffers of step_host(), made on first use
        self._host_fresh = False  # the last step wrote its outputs to the host buffers: the device tensors are stale until read
        self._bind()

    def _bind(self):
        """The buffer record handed to the library and what step() hands out as `info`, from the tensors as they are now.  Both are made once:
        the tensors never move, a view costs a microsecond or two of host time, and an eager rollout loop is host-bound long before the GPU is."""
        o = self._out
        self._info_views = {'food_rew': o['info'][:, 0], 'dead_rew': o['info'][:, 1], 'episode_return': o['info'][:, 2], 'episode_length': o['info'][:, 3],
                            # valid where done: the terminal observation (the returned obs of such an env is already the next episode's first
                            # when auto_reset is on) and gym's TimeLimit flag
                            'final_observation': o['final_obs'], 'TimeLimit.truncated': o['truncated']}
        # the items record is state of the gather kinds (item positions) and of every flagrun env (the bookkeeping of set_target(); the goal itself in the
        # manual and near-the-robot modes); the other kinds keep nothing in it, and the library takes NULL for it (include/hrl_envs.h): 128 B per
        # env and step less to read and to write back
        c = self.cfg
        self._uses_items = c.env_kind in (K.HRL_ANT_GATHER, K.HRL_POINT_GATHER, K.HRL_ANT_FLAGRUN)
        goal = o['goal'].data_ptr() if 'goal' in o else None
        if 'goal' in o:  # `target`: the goal after the step; `retargeted`: the rows whose step switched to it (the reference sets info['target'] on those steps only)
            self._info_views['target'] = o['goal'][:, 0:2]
            self._info_views['retargeted'] = o['goal'][:, 2]
        self._bufs = K.make_buffers(self.state.data_ptr(), self.items.data_ptr() if self._uses_items else None, self.aux.data_ptr(), None,
                                    o['obs'].data_ptr(), o['reward'].data_ptr(), o['done'].data_ptr(),
                                    o['info'].data_ptr(), o['final_obs'].data_ptr(), o['truncated'].data_ptr(), goal)
        self._bufs_ref = C.byref(self._bufs)
        # set_goals always hands the items record over: an env that has no use for it is refused by the library with the reason (not a manual env)
        self._bufs_with_items = K.make_buffers(self.state.data_ptr(), self.items.data_ptr(), self.aux.data_ptr(), None,
                                               o['obs'].data_ptr(), o['reward'].data_ptr(), o['done'].data_ptr(),
                                               o['info'].data_ptr(), o['final_obs'].data_ptr(), o['truncated'].data_ptr(), goal)

    def _device_out(self, name):
        """Output tensor `name` on the device.  step_host() leaves the step's outputs in pinned host memory only (that is its point: one
        launch, one synchronisation); whoever then reads a device tensor -- ReturnGatherer's snapshot of info[:, 2], code that mixes step()
        and step_host() -- gets the host values copied over first, once, instead of silently stale ones."""
        if self._host_fresh:
            self._host_fresh = False
            h = self._host
            for k, hk in (('obs', 'obs'), ('reward', 'rew'), ('done', 'done'), ('info', 'info')):
                self._out[k].copy_(h[hk], non_blocking=True)
            # final_obs: the kernel writes rows only where an episode ended; the rows that ended in any host step since the last refresh
            if self._host_ended.any():
                d = torch.from_numpy(self._host_ended)
                self._out['final_obs'][d.to(self.device)] = h['final_obs'][d].to(self.device)
                self._host_ended[:] = False
            self._out['truncated'].copy_(h['trunc'], non_blocking=True)
            if 'goal' in h:
                self._out['goal'].copy_(h['goal'], non_blocking=True)
        return self._out[name]

    def _before_device_launch(self):
        """A launch that writes the device output tensors comes after a step_host(): bring the host outputs over first (they would
        otherwise be copied over the NEW device values at the next read)."""
        if self._host_fresh:
            self._device_out('obs')

    obs = property(lambda self: self._device_out('obs'))
    reward = property(lambda self: self._device_out('reward'))
    done = property(lambda self: self._device_out('done'))
    info = property(lambda self: self._device_out('info'))
    final_obs = property(lambda self: self._device_out('final_obs'))
    truncated = property(lambda self: self._device_out('truncated'))
    goal = property(lambda self: self._device_out('goal'))  # AntFlagrun only: [N, 4] = goal x, y | switched to it in the last step | steps since the goal changed

    def update_config(self, cfg):
        """A changed copy of this env's config takes effect for the launches that follow on the current stream (hrl_update_config): the step limit,
        reward weights, tolerances, engine parameters ... of a LIVE env -- the simulation, every tensor and the pinned host buffers stay as they
        are.  What the tensors' shapes depend on cannot change (the library refuses and nothing happens)."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_update_config(self._h, C.byref(cfg), self._stream()))
        self.cfg = cfg
        self.__dict__.pop('_default_specs', None)   # the sensors' default specs are derived from the config (the arena's extent): asked again

    def count_solver_rows(self, on=True):
        """Diagnostic: from now on every step ADDS to `self.solver_rows` [N] (int32, zeroed here) the constraint rows each env's solver held
        -- joint limits + 3 per contact over the step's substeps (hrl_buffers.solver_rows).  What a launch costs depends on it."""
        self.solver_rows = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device) if on else None
        p = self.solver_rows.data_ptr() if on else None
        self._bufs.solver_rows = p
        self._bufs_with_items.solver_rows = p
        if self._host is not None:   # step_host()'s record too
            self._hbufs.solver_rows = p
        return self.solver_rows

    def record_contacts(self, on=True):
        """From now on every step writes `self.contacts` [N, HRL_CONTACTS_STRIDE] (float32): per env the contacts of the step's last collision
        pass -- point, normal, distance, link, surface -- and their solved impulses, what `p.getContactPoints()` answers in the reference
        (hrl_buffers_ext.contacts; contacts.decode() names the fields).  Written by the step's own launch, before an auto-reset; the tensor never
        moves, so a captured graph keeps writing it.  step_host() leaves it on the device.  Not part of state_dict(): it is an output."""
        self.contacts = torch.zeros(self.num_envs, K.HRL_CONTACTS_STRIDE, dtype=torch.float32, device=self.device) if on else None
        p = self.contacts.data_ptr() if on else None
        if on:   # the pointer lives in the longer record (hrl_buffers_ext); until it is asked for, the library is handed the plain v7 record
            self._bufs, self._bufs_with_items = K.hrl_buffers_ext.of(self._bufs), K.hrl_buffers_ext.of(self._bufs_with_items)
            self._bufs_ref = C.byref(self._bufs)
            if self._host is not None:   # step_host()'s record too
                self._hbufs = K.hrl_buffers_ext.of(self._hbufs)
        for b in (self._bufs, self._bufs_with_items, self._hbufs if self._host is not None else None):
            if isinstance(b, K.hrl_buffers_ext):
                b.contacts = p
        return self.contacts

    # the sensors (render, scan, probe, field, route, see, frontier, camera, links): each is one launch of a library of its own on the state / items / aux tensors as they are
    def _default_spec(self, key, make):
        """The spec a sensor uses when none is given: asked of its library once per `key`."""
        specs = self.__dict__.setdefault('_default_specs', {})
        if key not in specs:
            specs[key] = make()
        return specs[key]

    def _fresh(self, mask, shape, dtype):
        """A new output tensor [N, *shape]: zeros where a mask may leave envs unwritten."""
        return (torch.empty if mask is None else torch.zeros)(self.num_envs, *shape, dtype=dtype, device=self.device)

    def _fresh_out(self, M, kind, shapes, spec, mask, only=None):
        """The new outputs of a record-style sensor (binding M, namedtuple `kind`): a _fresh tensor per entry of `shapes` (M.shapes), of the
        first `only` when given; None where there is nothing to write (a first entry of 0).  M.size_error(spec) is raised: no tensor can
        be shaped after such a spec."""
        why = M.size_error(spec)
        if why is not None:
            raise ValueError(why)
        return kind(*(self._fresh(mask, shape, dtype) if shape[:1] != (0,) else None for shape, (_, dtype) in zip(shapes[:only], M.FIELDS)))

    def _sensor_launch(self, keep, mask, launch):
        """launch(mask pointer or None, stream) on this env's device and the current stream; the converted mask stays alive as attribute `keep`."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        if torch.cuda.current_device() == self.device.index:   # as in step(): the context manager costs more host time than this helper does
            launch(None if m is None else m.data_ptr(), self._stream())
        else:
            with torch.cuda.device(self.device):
                launch(None if m is None else m.data_ptr(), self._stream())
        setattr(self, keep, m)  # until the stream has consumed it

    def render(self, view=None, mask=None, out=None):
        """A top-down RGB image of every env: torch.uint8 [N, H, W, 3] on this device, from ONE launch on the current stream (render_device.py,
        include/hrl_render.h) -- what a high-level policy's CNN or a video writer reads without leaving HBM.  `view`: an hrl_view
        (render_device.default_view(cfg, mode, width, height)); None = the 64 x 64 world view of the whole arena.  Envs with mask[i] == 0 keep
        the bytes `out` holds (zeros in a fresh tensor).  `out` is reused when given (uint8, [N, H, W, 3], contiguous).  The picture is of
        the state / items / aux tensors as they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import render_device as R
        if view is None:
            view = self._default_spec('render', lambda: R.default_view(self.cfg))
        if out is None:
            out = self._fresh(mask, (view.height, view.width, 3), torch.uint8)
        else:
            R.check_out(out, self.num_envs, view, self.device)
        self._sensor_launch('_last_render_mask', mask, lambda m, stream: R.render(self.cfg, self._bufs_ref, view, m, out, stream))
        return out

    def scan(self, spec=None, mask=None, out=None):
        """A ring of range rays per env: (range float32 [N, n_rays] in metres, hit int32 [N, n_rays]) on this device, from ONE launch on the
        current stream (scan_device.py, include/hrl_scan.h).  The rays see the walls, the maze box, food, poison and the target as finite
        shapes; `hit` = class code | index << 8 (scan_device.decode).  `spec`: an hrl_scan_spec (scan_device.default_spec(cfg, frame,
        n_rays), scan_device.sensor_spec(...)); None = 64 rays around the robot's heading out to the arena's diagonal.  Envs with
        mask[i] == 0 keep what `out` holds (zeros in fresh tensors).  `out=(range, hit)` is reused when given.  The scan is of the state /
        items / aux tensors as they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import scan_device as S
        if spec is None:
            spec = self._default_spec('scan', lambda: S.default_spec(self.cfg))
        if out is None:
            why = S.size_error(spec)
            if why is not None:
                raise ValueError(why)
            rng, hit = self._fresh(mask, (spec.n_rays,), torch.float32), self._fresh(mask, (spec.n_rays,), torch.int32)
        else:
            rng, hit = S.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_scan_mask', mask, lambda m, stream: S.scan(self.cfg, self._bufs_ref, spec, m, rng, hit, stream))
        return rng, hit

    def probe(self, points, spec=None, mask=None, out=None):
        """Point probes: for P query points per env (`points` float32 [N, P, 2] on this device, 1 <= P <= 512) a namedtuple
        Probe(clearance, nearest, sight, blocker, path, via), each [N, P] on this device, from ONE launch on the current stream
        (probe_device.py, include/hrl_probe.h).  clearance / nearest: the signed distance to the nearest shape and its code (class |
        index << 8, probe_device.decode); sight / blocker: how far the segment from the robot to the point runs free and what stops it (0 =
        the point is visible); path / via: the length of the shortest way round the maze box for a disc of radius spec.margin and the
        corner it first turns at (probe_device.corner_table).  `spec`: an hrl_probe_spec (probe_device.default_spec(cfg, frame, n_points));
        None = world-frame points, all classes, margin = the torso's radius.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh
        tensors).  `out`: a Probe of tensors to reuse; a None field is not computed.  The probes are of the state / items / aux tensors as
        they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import probe_device as P
        points = P.check_points(points, self.num_envs, self.device)
        if spec is None:
            spec = self._default_spec(('probe', points.shape[1]), lambda: P.default_spec(self.cfg, 'world', points.shape[1]))
        elif spec.n_points != points.shape[1]:
            raise ValueError(f'spec.n_points is {spec.n_points}, points hold {points.shape[1]} per env')
        out = self._fresh_out(P, P.Probe, P.shapes(spec), spec, mask) if out is None else P.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_probe_mask', mask, lambda m, stream: P.probe(self.cfg, self._bufs_ref, spec, points, m, out, stream))
        return out

    def field(self, spec=None, mask=None, out=None):
        """The navigation field of every env: a namedtuple Field(dist float32 [N, H, W], parent uint8 [N, H, W]) on this device, from ONE
        launch on the current stream (field_device.py, include/hrl_field.h).  On the renderer's pixel grid, for a disc of radius
        spec.margin among the shapes of spec.blocking: dist = the length of the shortest 8-connected way from the cell to the nearest
        source cell (spec.sources: the robot, the target, food, poison), 0 on a source, +inf where there is no way; parent = the direction
        code 0..7 of that way's first step (field_device.DIRECTIONS, direction_vectors), or SOURCE / UNREACHED / BLOCKED.  `spec`: an
        hrl_field_spec (field_device.default_spec(cfg, mode, width, height)); None = the 64 x 64 world grid of the whole arena towards the
        kind's goal.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh tensors).  `out`: a Field of tensors to reuse; a None
        member is not computed.  The field is of the state / items / aux tensors as they are; nothing else is read or written.
        Capturable: call it once before the capture."""
        from . import field_device as F
        if spec is None:
            spec = self._default_spec('field', lambda: F.default_spec(self.cfg))
        out = self._fresh_out(F, F.Field, F.shapes(spec), spec, mask) if out is None else F.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_field_mask', mask, lambda m, stream: F.field(self.cfg, self._bufs_ref, spec, m, out, stream))
        return out

    def route(self, starts=None, spec=None, mask=None, out=None):
        """Routes down the navigation field: for P start points per env (`starts` float32 [N, P, 2] on this device, 1 <= P <= 64; None =
        the robot's own place) a namedtuple Route(waypoints float32 [N, P, K, 2], count int32 [N, P], length float32 [N, P], cells int32
        [N, P, K]) on this device, from ONE launch on the current stream (route_device.py, include/hrl_route.h).  The route follows the
        field of the spec's field part from the start's cell to the nearest source and is pulled tight: a waypoint is kept only where the
        straight line from the last one would touch a blocked cell.  waypoints = the world x, y of the kept cells' centres, cells = row *
        width + column of them, both padded with the last one up to K = spec.max_waypoints; count = how many the whole route has (it may
        exceed K; 0 = there is no route: the start is outside the grid, not finite, or on a blocked or cut-off cell, and then length is
        +inf, cells -1 and waypoints NaN); length = the polyline's length in metres.  `spec`: an hrl_route_spec
        (route_device.default_spec(cfg, mode, width, height, frame, n_starts, max_waypoints)); None = the default field, starts as
        offsets from the robot, 16 waypoints.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh tensors).  `out`: a Route of
        tensors to reuse; a None member is not computed.  The routes are of the state / items / aux tensors as they are; nothing else is
        read or written.  Capturable: call it once before the capture."""
        from . import route_device as R
        p = 1 if starts is None else R.check_starts(starts, self.num_envs, self.device).shape[1]
        if spec is None:
            spec = self._default_spec(('route', p), lambda: R.default_spec(self.cfg, n_starts=p))
        elif spec.n_starts != p:
            raise ValueError(f'spec.n_starts is {spec.n_starts}, starts hold {p} per env' if starts is not None else f'spec.n_starts is {spec.n_starts}: without starts there is one per env, the robot')
        out = self._fresh_out(R, R.Route, R.shapes(spec), spec, mask) if out is None else R.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_route_mask', mask, lambda m, stream: R.route(self.cfg, self._bufs_ref, spec, starts, m, out, stream))
        return out

    def see(self, spec=None, clear=None, mask=None, out=None):
        """The visibility map of every env: a namedtuple See(visible uint8 [N, H, W], seen uint8 [N, H, W], fresh int32 [N]) on this device,
        from ONE launch on the current stream (see_device.py, include/hrl_see.h).  On the field's and the renderer's grid: visible = 1 where
        the robot sees the cell's centre -- within spec.max_range, within the field of view spec.fov_cos about its heading, and with no
        shape of spec.occluders before it (the probe's `blocker` test; spec.slack metres behind a surface still count, so the face of a
        wall is lit).  `seen` is the episode's memory, HELD BY THE CALLER (see_device.memory): it is read and written as seen | visible,
        in the world mode only, and `fresh` counts the cells seen for the first time.  `clear`: [N], envs whose memory starts from nothing
        in this call (the step's `done`).  `spec`: an hrl_see_spec (see_device.default_spec(cfg, mode, width, height, fov_degrees,
        max_range, slack)); None = the 64 x 64 world grid, WALL | BOX occlude, all round, a slack of one cell.  Envs with mask[i] == 0 keep
        every byte.  `out`: a See of tensors to use; a None member is not computed; None = See(visible, None, None) in a fresh tensor.
        The map is of the state / items / aux tensors as they are; nothing else is read or written.  Capturable: call it once before the
        capture."""
        from . import see_device as V
        if spec is None:
            spec = self._default_spec('see', lambda: V.default_spec(self.cfg))
        out = self._fresh_out(V, V.See, V.shapes(spec), spec, mask, only=1) if out is None else V.check_out(out, self.num_envs, spec, self.device)
        c =None if clear is None else clear.to(device=self.device, dtype=torch.uint8).contiguous()
        if c is not None and tuple(c.shape) != (self.num_envs,):
            raise ValueError(f'clear must be [{self.num_envs}], got {tuple(c.shape)}')
        self._sensor_launch('_last_see_mask', mask, lambda m, stream: V.see(self.cfg, self._bufs_ref, spec, None if c is None else c.data_ptr(), m, out, stream))
        self._last_see_clear = c  # until the stream has consumed it
        return out

    def frontier(self, seen, spec=None, mask=None, out=None):
        """The frontier map of every env: a namedtuple Frontier(edge uint8 [N, H, W], dist float32 [N, H, W], parent uint8 [N, H, W], count
        int32 [N], length float32 [N], goal float32 [N, 2], cell int32 [N]) on this device, from ONE launch on the current stream
        (frontier_device.py, include/hrl_frontier.h).  `seen`: the memory of see() on the same world grid (uint8 [N, H, W], only read; any
        non-zero byte counts as seen, and the robot always knows the cell it stands in).  edge = 1 on a known cell that is not blocked and
        has an unknown orthogonal neighbour inside the grid; dist / parent = the navigation field (field()'s codes) over the known space --
        an unknown cell is blocked, or free with spec.unknown = OPTIMISTIC -- towards spec.sources: the edge cells (EDGE) and / or the
        robot, food, poison, the target; count = the number of edge cells (0 = nothing left to explore); length = dist at the robot's
        cell; goal / cell = the world x, y and row * width + column of the source cell the way from the robot ends on (NaN, -1 and +inf
        when the robot stands outside the grid, on a blocked cell or cut off).  `spec`: an hrl_frontier_spec
        (frontier_device.default_spec(cfg, width, height, sources, unknown, margin) or spec_like(cfg, see_spec, ...)); None = the 64 x 64
        world grid of see(), towards the edge, unknown cells blocked.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh
        tensors).  `out`: a Frontier of tensors to reuse; a None member is not computed.  The map is of the state / items / aux tensors
        and of `seen` as they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import frontier_device as X
        if spec is None:
            spec = self._default_spec('frontier', lambda: X.default_spec(self.cfg))
        why = X.size_error(spec)   # before `seen` is measured against the spec, so with `out` given too
        if why is not None:
            raise ValueError(why)
        X.check_seen(seen, self.num_envs, spec, self.device)
        out = self._fresh_out(X, X.Frontier, X.shapes(spec), spec, mask) if out is None else X.check_out(out, self.num_envs, spec, self.device, seen)
        self._sensor_launch('_last_frontier_mask', mask, lambda m, stream: X.frontier(self.cfg, self._bufs_ref, spec, seen.data_ptr(), m, out, stream))
        return out

    def camera(self, spec=None, mask=None, out=None):
        """The first-person image of every env: a namedtuple Camera(depth float32 [N, H, W], seg int32 [N, H, W], rgb uint8 [N, H, W, 3]) on
        this device, from ONE launch on the current stream (camera_device.py, include/hrl_camera.h).  A pinhole camera over the robot that
        yaws with spec.frame and neither pitches nor rolls sees the walls, the maze box, the item cubes, the target post and the ground as
        solids: depth = metres along the optical axis (spec.max_range where nothing was hit), seg = the scanner's hit code | face << 16
        (camera_device.decode), rgb = the class colour shaded by face, the sky where nothing was hit.  `spec`: an hrl_camera_spec
        (camera_device.default_spec(cfg, frame, width, height, hfov_degrees, vfov_degrees, eye, eye_height, max_range, classes)); None =
        64 x 48 pixels, 90 degrees, from the torso, turning with the heading.  Envs with mask[i] == 0 keep what `out` holds (zeros in
        fresh tensors).  `out`: a Camera of tensors to reuse; a None member is not computed.  The image is of the state / items / aux
        tensors as they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import camera_device as Cm
        if spec is None:
            spec = self._default_spec('camera', lambda: Cm.default_spec(self.cfg))
        out = self._fresh_out(Cm, Cm.Camera, Cm.shapes(spec), spec, mask) if out is None else Cm.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_camera_mask', mask, lambda m, stream: Cm.camera(self.cfg, self._bufs_ref, spec, m, out, stream))
        return out

    def links(self, spec=None, mask=None, out=None):
        """The state of every rigid body of every env's robot: a namedtuple Links(origin, com, quat, lin_vel, ang_vel, site_pos, site_vel) on
        this device, from ONE launch on the current stream (links_device.py, include/hrl_links.h).  B = 13 links for the ants (the torso,
        per leg the hinged upper body and the foot, then the four jointless hip capsules: links_device.NAMES), 1 for the point bot.  origin
        [N, B, 3] = the link frame's origin, the joint anchor; com [N, B, 3] = the centre of mass, what the reference's
        `parts[name].get_position()` answers (links_device.tip: the capsule's far end); quat [N, B, 4] = the body frame (x, y, z, w);
        lin_vel / ang_vel [N, B, 3] = the velocity of the centre of mass and the angular velocity; site_pos / site_vel [N, S, 3] = the
        spec's sites, points fixed to links (by default the four foot tips).  `spec`: an hrl_links_spec
        (links_device.default_spec(cfg, frame, sites)); None = world frame, the default sites.  In the 'heading' frame positions are
        relative to the torso and every vector is turned by minus the heading.  Envs with mask[i] == 0 keep what `out` holds (zeros in
        fresh tensors).  `out`: a Links of tensors to reuse; a None member is not computed.  The states are of the state tensor as it is;
        nothing else is read or written.  Capturable: call it once before the capture."""
        from . import links_device as Lk
        if spec is None:
            spec = self._default_spec('links', lambda: Lk.default_spec(self.cfg))
        out = self._fresh_out(Lk, Lk.Links, Lk.shapes(self.cfg, spec), spec, mask) if out is None else Lk.check_out(out, self.num_envs, self.cfg, spec, self.device)
        self._sensor_launch('_last_links_mask', mask, lambda m, stream: Lk.links(self.cfg, self._bufs_ref, spec, m, out, stream))
        return out

    def dynamics(self, spec=None, tau=None, mask=None, out=None):
        """The dynamics terms of every env's robot: a namedtuple Dynamics(mass, bias, accel, jac, com, momentum, energy) on this device,
        from ONE launch on the current stream (dyn_device.py, include/hrl_dyn.h) -- what the simulator's calculateMassMatrix,
        calculateInverseDynamics and calculateJacobian answer one env at a time.  Generalised velocities are the state's qvel in its own
        order, (v of the torso's origin, omega, joint rates): nv = 14 for the ants, 6 for the point bot.  mass [N, nv, nv] = the
        joint-space mass matrix M(q) (bitwise symmetric); bias [N, nv] = Coriolis and centrifugal terms, gravity and the model's damping,
        so that M udot + bias = tau describes the contact-free robot; accel [N, nv] = M^-1 (tau - bias); jac [N, S, 3, nv] = the linear
        Jacobian of the spec's sites, points fixed to links (by default the four foot tips): jac @ qvel is the site's velocity; com
        [N, 3] = the whole-body centre of mass; momentum [N, 6] = linear momentum and angular momentum about the centre of mass; energy
        [N, 2] = kinetic and potential energy.  `spec`: an hrl_dyn_spec (dyn_device.default_spec(cfg, sites)); None = the default sites.
        `tau`: float32 [N, nv] on this device, the applied generalised force of `accel` (dyn_device.torques(cfg, actions)); None =
        zeros.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh tensors).  `out`: a Dynamics of tensors to reuse; a None
        member is not computed.  The terms are of the state tensor as it is; nothing else is read or written.  Capturable: call it once
        before the capture."""
        from . import dyn_device as Dy
        if spec is None:
            spec = self._default_spec('dynamics', lambda: Dy.default_spec(self.cfg))
        if tau is not None:
            Dy.check_tau(tau, self.num_envs, self.cfg, self.device)
        out = self._fresh_out(Dy, Dy.Dynamics, Dy.shapes(self.cfg, spec), spec, mask) if out is None else Dy.check_out(out, self.num_envs, self.cfg, spec, self.device, tau)
        self._sensor_launch('_last_dynamics_mask', mask, lambda m, stream: Dy.dynamics(self.cfg, self._bufs_ref, spec, None if tau is None else tau.data_ptr(), m, out, stream))
        self._last_dynamics_tau = tau  # until the stream has consumed it
        return out

    def chase(self, spec=None, mask=None, out=None):
        """The third-person image of every env, the robot's body in it: a namedtuple Chase(depth float32 [N, H, W], seg int32 [N, H, W], rgb
        uint8 [N, H, W, 3]) on this device, from ONE launch on the current stream (chase_device.py, include/hrl_chase.h).  A pinhole
        camera orbits each robot at spec.distance, yaw and pitch and looks at it: it sees the walls, the maze box, the item cubes, the
        target post and a checkered ground as solids, the ant as its torso sphere and twelve capsules (the point bot as its cube): depth =
        metres along the optical axis (spec.max_range where nothing was hit), seg = class | index << 8 | face << 16 with class
        chase_device.HIT_ROBOT and index = the link for the body (chase_device.decode), rgb = the class or link colour shaded by face,
        the sky where nothing was hit.  `spec`: an hrl_chase_spec (chase_device.default_spec(cfg, frame, width, height, yaw_degrees,
        pitch_degrees, distance, hfov_degrees, vfov_degrees, target, target_height, max_range, classes, tile)); None = 64 x 48 pixels from
        3 m behind the torso and 30 degrees above it, turning with the heading.  Envs with mask[i] == 0 keep what `out` holds (zeros in
        fresh tensors).  `out`: a Chase of tensors to reuse; a None member is not computed.  The image is of the state / items / aux
        tensors as they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import chase_device as Ch
        if spec is None:
            spec = self._default_spec('chase', lambda: Ch.default_spec(self.cfg))
        out = self._fresh_out(Ch, Ch.Chase, Ch.shapes(spec), spec, mask) if out is None else Ch.check_out(out, self.num_envs, spec, self.device)
        self._sensor_launch('_last_chase_mask', mask, lambda m, stream: Ch.chase(self.cfg, self._bufs_ref, spec, m, out, stream))
        return out

    def cast(self, rays, spec=None, mask=None, out=None, ray_link=None):
        """The caller's 3-D rays against every env's scene and robot: a namedtuple Cast(fraction float32 [N, R], seg int32 [N, R], point
        float32 [N, R, 3], normal float32 [N, R, 3]) on this device, from ONE launch on the current stream (cast_device.py,
        include/hrl_cast.h) -- what the simulator's rayTestBatch(from, to) answers one env at a time.  `rays`: float32 [N, R, 6] on this
        device, contiguous and 8-byte aligned, 1 <= R <= 1024: per ray `from` and `to` in the coordinates of spec.frame -- world
        positions, offsets from the torso in world axes ('ego'), offsets turned by the heading ('heading': x forward, y left) or
        coordinates in the body frame of a link ('link'; the link of ray r is ray_link[r], an int32 tensor [R] on this device shared by
        all envs, None = the torso for every ray; a link out of range meets nothing).  A pattern [R, 6] is expanded to [N, R, 6] here,
        which COPIES IT AT EVERY CALL: in a loop hand in cast_device.expand(pattern, N, device), materialised once.  The rays meet the
        chase camera's solids under its rules: walls, the maze box, item cubes and the target post as prisms, the ground, the ant as its
        torso sphere and twelve capsules (the point bot as its cube), entered from outside only; the nearest hit with 0 < t <= 1 wins.
        fraction = t (1.0 where nothing was met), seg = class | index << 8 | face << 16 (cast_device.decode; class cast_device.HIT_ROBOT
        with index = the link), point = the hit in world coordinates (`to` where nothing was met), normal = the outward unit normal in
        world axes (zeros where nothing was met).  `spec`: an hrl_cast_spec (cast_device.default_spec(cfg, frame, n_rays, classes));
        None = the 'heading' frame, every class, R rays.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh tensors).  `out`:
        a Cast of tensors to reuse; a None member is not computed.  The answer is of the state / items / aux tensors as they are;
        nothing else is read or written.  Capturable: call it once before the capture."""
        from . import cast_device as Ca
        if isinstance(rays, torch.Tensor) and rays.dim() == 2:
            rays = Ca.expand(rays, self.num_envs, self.device)
        if spec is None:
            r = int(rays.shape[1]) if isinstance(rays, torch.Tensor) and rays.dim() == 3 else 0
            spec = self._default_spec(('cast', r), lambda: Ca.default_spec(self.cfg, n_rays=r))
        why = Ca.size_error(spec)
        if why is not None:
            raise ValueError(why)
        Ca.check_rays(rays, self.num_envs, spec, self.device)
        if ray_link is not None:
            Ca.check_ray_link(ray_link, spec, self.device)
        out = self._fresh_out(Ca, Ca.Cast, Ca.shapes(spec), spec, mask) if out is None else Ca.check_out(out, self.num_envs, spec, self.device, rays)
        self._sensor_launch('_last_cast_mask', mask,
                            lambda m, stream: Ca.cast(self.cfg, self._bufs_ref, spec, rays.data_ptr(), None if ray_link is None else ray_link.data_ptr(), m, out, stream))
        self._last_cast_rays = (rays, ray_link)  # until the stream has consumed them
        return out

    def closest(self, spec=None, mask=None, out=None):
        """How far every body of every env's robot is from everything it could collide with: a namedtuple Closest(distance float32
        [N, B, 6], which int32 [N, B, 6], on_link, on_surface, normal float32 [N, B, 6, 3]) on this device, from ONE launch on the current
        stream (closest_device.py, include/hrl_closest.h) -- what the simulator's getClosestPoints answers one pair at a time.  B = 13
        links for the ants, 1 for the point bot (links_device.NAMES); the class axis is closest_device.CLASS_NAMES: ground, wall, box,
        food, poison, self.  The surfaces are what the STEP collides with: the ground plane, the walls' inner faces (0.05 m nearer than
        the line scan() and cast() meet), the maze box, the item cubes (indices as in scan() and cast()) and, for `self`, the capsules
        of the other legs in the step's 48 pairs.  distance = the signed gap between the two surfaces (negative = penetration, +inf
        where the class has no surface, was not asked for or nothing finite was found), which = class | index << 8
        (closest_device.decode; closest_device.HIT_NONE wherever distance is +inf), on_link / on_surface = the closest points in world
        coordinates, normal = the unit normal from the surface towards the link (zeros where nothing was found).  The point bot's cube
        against an item cube is exact unless the nearest features are two edges, then an upper bound.  `spec`: an hrl_closest_spec
        (closest_device.default_spec(cfg, classes)); None = every class.  Envs with mask[i] == 0 keep what `out` holds (zeros in fresh
        tensors).  `out`: a Closest of tensors to reuse; a None member is not computed.  The answer is of the state / items tensors as
        they are; nothing else is read or written.  Capturable: call it once before the capture."""
        from . import closest_device as Cl
        if spec is None:
            spec = self._default_spec('closest', lambda: Cl.default_spec(self.cfg))
        out = self._fresh_out(Cl, Cl.Closest, Cl.shapes(self.cfg, spec), spec, mask) if out is None else Cl.check_out(out, self.num_envs, self.cfg, spec, self.device)
        self._sensor_launch('_last_closest_mask', mask, lambda m, stream: Cl.closest(self.cfg, self._bufs_ref, spec, m, out, stream))
        return out

    def close(self):
        if getattr(self, '_h', None):
            _lib.lib().hrl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._before_device_launch()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_reset(self._h, C.byref(self._bufs), None if m is None else m.data_ptr(),
                                            self._stream()))
        return self.obs

    def step(self, actions):
        """actions: float32 [N, act_dim] on this device.  Returns (obs, reward, done, info) -- views of the env's
        own output tensors, overwritten by the next step."""
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous() \
                or tuple(actions.shape) != (self.num_envs, self.act_dim):
            actions = actions.to(device=self.device, dtype=torch.float32).reshape(self.num_envs, self.act_dim).contiguous()
        self._bufs.actions = actions.data_ptr()
        if self._host_fresh:
            self._before_device_launch()
        if torch.cuda.current_device() == self.device.index:   # the usual case; the context manager costs more host time than the launch
            rc = _lib.lib().hrl_step(self._h, self._bufs_ref, self._stream())
        else:
            with torch.cuda.device(self.device):
                rc = _lib.lib().hrl_step(self._h, self._bufs_ref, self._stream())
        if rc != K.HRL_OK:
            _lib.check(rc)
        self._last_actions = actions  # keep alive until the stream has consumed it
        o = self._out                 # (current: a pending host refresh was brought over before the launch)
        return o['obs'], o['reward'], o['done'], dict(self._info_views)

    def step_host(self, actions):
        """One step with HOST input and outputs -- what the reference's numpy-in / numpy-out `env.step(a)` hands over
        (README.md:24-34), for the one-env classes: the action is written into pinned host memory that the kernel reads
        directly, and observations / reward / done / info land in pinned host memory the kernel writes directly, so a step is
        one launch and one stream synchronisation -- no staging copies, no packing kernel.  The simulation state stays in HBM.
        Returns numpy views (obs [N, obs_dim], reward [N], done [N] uint8, info [N, 4]) that the next call overwrites (the terminal
        observation / truncation flag of this path: `host_final_obs()`); the device tensors `obs` / `reward` / `done` / `info` are
        refreshed from these host buffers when they are next read (`_device_out`), not by this call."""
        if self._host is None:
            f32 = torch.float32
            t = {'act': torch.zeros(self.num_envs, self.act_dim, dtype=f32).pin_memory(),
                 'obs': torch.zeros(self.num_envs, self.obs_dim, dtype=f32).pin_memory(),
                 'rew': torch.zeros(self.num_envs, dtype=f32).pin_memory(),
                 'done': torch.zeros(self.num_envs, dtype=torch.uint8).pin_memory(),
                 'info': torch.zeros(self.num_envs, K.HRL_INFO_STRIDE, dtype=f32).pin_memory(),
                 'final_obs': torch.zeros(self.num_envs, self.obs_dim, dtype=f32).pin_memory(),
                 'trunc': torch.zeros(self.num_envs, dtype=torch.uint8).pin_memory()}
            if 'goal' in self._out:
                t['goal'] = torch.zeros(self.num_envs, K.HRL_GOAL_STRIDE, dtype=f32).pin_memory()
            self._host = t
            self._host_np = {k: v.numpy() for k, v in t.items()}
            self._host_ended = np.zeros(self.num_envs, bool)  # envs whose episode ended in a host step since the device tensors were refreshed
            self._hbufs = K.make_buffers(self.state.data_ptr(), self.items.data_ptr() if self._uses_items else None, self.aux.data_ptr(), t['act'].data_ptr(),
                                         t['obs'].data_ptr(), t['rew'].data_ptr(), t['done'].data_ptr(), t['info'].data_ptr(),
                                         t['final_obs'].data_ptr(), t['trunc'].data_ptr(), t['goal'].data_ptr() if 'goal' in t else None)
            self._hbufs.solver_rows = self._bufs.solver_rows   # the diagnostic counter, when count_solver_rows() switched it on
            if isinstance(self._bufs, K.hrl_buffers_ext):      # the contact report, when record_contacts() switched it on
                self._hbufs = K.hrl_buffers_ext.of(self._hbufs)
                self._hbufs.contacts = self._bufs.contacts
        h = self._host_np
        h['act'][...] = actions
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_step(self._h, C.byref(self._hbufs), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()
        self._host_fresh = True
        self._host_ended |= h['done'] != 0
        return h['obs'], h['rew'], h['done'], h['info']

    def host_goal(self):
        """AntFlagrun: [N, 4] numpy view of the last step_host(): goal x, y | 1 if that step switched to it | steps since the goal changed."""
        return self._host_np['goal']

    def host_final_obs(self):
        """(final_obs [N, obs_dim], truncated [N] uint8) numpy views of the last step_host(): valid where its `done` was set."""
        return self._host_np['final_obs'], self._host_np['trunc']

    def set_goals(self, goals, mask=None):
        """AntFlagrun with flag_manual_goals: goals float32 [N, n_goals, 2] on this device (include/hrl_envs.h: hrl_set_goals)."""
        goals = goals.to(device=self.device, dtype=torch.float32).contiguous()
        if goals.dim() != 3 or goals.shape[0] != self.num_envs or goals.shape[2] != 2:
            raise ValueError(f'goals must be [num_envs={self.num_envs}, n_goals, 2], got {tuple(goals.shape)}')
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._before_device_launch()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_set_goals(self._h, C.byref(self._bufs_with_items), goals.data_ptr(), int(goals.shape[1]),
                                                None if m is None else m.data_ptr(), self._stream()))
        self._last_goals = goals  # keep alive until the stream has consumed it
        return self.obs

    def next_target(self, mask=None):
        """AntFlagrun with flag_manual_goals: `env.next_target()` for every (masked) env (include/hrl_envs.h: hrl_next_target).
        Returns (obs, ok): ok[i] == 0 where the reference raises IndexError (empty list; that env is unchanged)."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        ok = torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)
        self._before_device_launch()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_next_target(self._h, C.byref(self._bufs), None if m is None else m.data_ptr(), ok.data_ptr(), self._stream()))
        return self.obs, ok

    # checkpoint / resume: everything an env carries from one step to the next is three tensors -- `state` (pose, velocities, episode
    # return, potential), `items` (item positions / pending goals) and `aux` (step, pickup, episode and goal counters: the keys of the counter-based
    # random streams) -- plus the config (seed, env_id_offset, constructor arguments).  torch.save()-able; resuming continues bit for bit.
    def state_dict(self):
        self._before_device_launch()
        out = {k: getattr(self, k).detach().cpu().clone() for k in ('state', 'items', 'aux', 'obs', 'reward', 'done', 'info', 'final_obs', 'truncated') + (('goal',) if 'goal' in self._out else ())}
        out['config'] = bytes(self.cfg)
        out['abi_version'] = K.HRL_ABI_VERSION
        return out

    def load_state_dict(self, sd, strict=True):
        """Restores a state_dict() of an env with the same config.  strict: the whole config (seed and env_id_offset included: they key the
        random streams) must be equal; strict=False only insists on what the buffers' shapes depend on."""
        if sd.get('abi_version') != K.HRL_ABI_VERSION:
            raise _lib.HrlError(f"checkpoint of ABI v{sd.get('abi_version')}, this library is v{K.HRL_ABI_VERSION}")
        if strict and sd['config'] != bytes(self.cfg):
            raise _lib.HrlError('checkpoint was taken from an env with another config (strict=False skips this check)')
        for k in ('state', 'items', 'aux'):
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise _lib.HrlError(f'checkpoint {k} is {tuple(sd[k].shape)}, this env holds {tuple(getattr(self, k).shape)}')
        self._before_device_launch()
        for k in ('state', 'items', 'aux'):
            getattr(self, k).copy_(sd[k])
        for k in ('obs', 'reward', 'done', 'info', 'final_obs', 'truncated', 'goal'):
            if k in sd and k in self._out and tuple(sd[k].shape) == tuple(self._out[k].shape):
                self._out[k].copy_(sd[k])
        return self.obs

    # state access (identical-state parity tests)
    @property
    def qpos(self):
        return self.state[:, K.HRL_QPOS_OFF:K.HRL_QPOS_OFF + 15]

    @property
    def qvel(self):
        return self.state[:, K.HRL_QVEL_OFF:K.HRL_QVEL_OFF + 14]

    def get_state(self):
        qpos = torch.empty(self.num_envs, 15, dtype=torch.float32, device=self.device)
        qvel = torch.empty(self.num_envs, 14, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_get_state(self._h, C.byref(self._bufs), qpos.data_ptr(), qvel.data_ptr(), self._stream()))
        return qpos, qvel

    def set_state(self, qpos, qvel, observe=True):
        """Teleport: writes qpos [N, 15] / qvel [N, 14] into the state records and -- as the reference does after
        `resetBasePositionAndOrientation` (ant_maze_bullet_env.py:117-121: calc_state(), _get_obs()) -- recomputes the observations of the new
        state (hrl_observe).  Returns them."""
        qpos = qpos.to(device=self.device, dtype=torch.float32).contiguous()
        qvel = qvel.to(device=self.device, dtype=torch.float32).contiguous()
        self._before_device_launch()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_set_state(self._h, C.byref(self._bufs), qpos.data_ptr(), qvel.data_ptr(), self._stream()))
            if observe:
                _lib.check(_lib.lib().hrl_observe(self._h, C.byref(self._bufs), None, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        return self.obs

    def observe(self, mask=None):
        """The observations of the state / items / aux tensors AS THEY ARE (after writing into them: a teleport, moved items, another target):
        hrl_observe.  Nothing else changes.  Rows with mask == 0 keep their observation."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._before_device_launch()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hrl_observe(self._h, C.byref(self._bufs), None if m is None else m.data_ptr(), self._stream()))
        return self.obs
