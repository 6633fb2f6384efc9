"""Monte-Carlo driver: what main.py of the reference does, as one HIP grid per sweep instead of sequential trials.

Keeps the reference's ``config.json`` schema (main.py:16-98), sweep cells (``linspace(0, .2, 12)`` of rho, or
``linspace(1, 2, 12)`` of alpha for ALPHA_STABLE, main.py:104-106), global trial numbering, per-trial noise seed
``seed + trial`` (main.py:137-139), the q_start jitter stream ``NoiseProfiler(2, UNIFORM, seed=experiment_seed)`` with
the ``2 (r - 1)`` formula (main.py:118, 132-134) and the 41-column results.csv (main.py:152-196; SURVEY.md says 43, the DataFrame has 4 + 6 + 6 + 8 + 8 + 8 + 1 = 41).
"""
import functools
import json
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib, dist, engine, noise_device
from .experiment import ExperimentStatus, Method, bandwidth_log
from .noise import NoiseProfiler, NoiseType, noise_batch
from .plant import SyntheticPlant

REQUIRED = {'experiments': ('dt', 't_max', 'epoch', 'ibvs_gain', 'q_start', 'desired_f', 'visualization', 'change_q_start', 'seed'),
            'estimator': ('method', 'estimator_params'),
            'noise': ('type', 'noise_params', 'hold', 'hold_time', 'seed')}


def load_config(path_or_dict):
    """Parse and validate a reference-format config (main.py:16-98); unknown method / noise names and missing keys raise."""
    cfg = path_or_dict if isinstance(path_or_dict, dict) else json.load(open(path_or_dict, 'r', encoding='utf-8'))
    if 'log_level' not in cfg:
        raise KeyError('log_level')
    for section, keys in REQUIRED.items():
        for key in keys:
            if key not in cfg[section]:
                raise KeyError(f'{section}.{key}')
    if cfg['estimator']['method'] not in Method.__members__:
        raise ValueError('Estimation method ' + cfg['estimator']['method'] + ' unknown.')
    if cfg['noise']['type'] not in NoiseType.__members__:
        raise ValueError('Noise type ' + cfg['noise']['type'] + ' unknown.')
    return cfg


def sweep_cells(noise_type):
    return np.linspace(1, 2, 12) if noise_type == NoiseType.ALPHA_STABLE else np.linspace(0, 0.2, 12)   # main.py:104-106


@dataclass
class TrialPlan:
    """Global enumeration of a sweep: trial t belongs to cell ``cell[t]`` with swept value ``value[t]``."""
    cell: np.ndarray
    value: np.ndarray
    seed: np.ndarray
    q_start: np.ndarray
    cells: np.ndarray = field(default=None)

    def __len__(self):
        return len(self.cell)


def plan_trials(cfg, cells=None, epoch=None):
    """Enumerate trials like main.py:121-139.  ``cells`` overrides the 12-point sweep (e.g. [1.5]); ``epoch`` the trials per cell."""
    ex, nz = cfg['experiments'], cfg['noise']
    noise_type = NoiseType[nz['type']]
    cells = sweep_cells(noise_type) if cells is None else np.asarray(cells, float)
    epoch = int(ex['epoch'] if epoch is None else epoch)
    T = len(cells) * epoch
    q0 = np.tile(np.asarray(ex['q_start'], float), (T, 1))
    if ex['change_q_start']:
        # two UNIFORM generators seeded seed and seed + 10 (noise.py:70); trial t consumes the t-th draw of each
        g0, g1 = (NoiseProfiler(2, NoiseType.UNIFORM, seed=ex['seed']).generators[i] for i in range(2))
        q0[:, 0] += 2 * (g0.random(T) - 1) * (np.pi / 18)           # main.py:133
        q0[:, 1] += 2 * (g1.random(T) - 1) * (np.pi / 9)            # main.py:134
    seed0 = nz['seed']
    if seed0 is not None:
        seeds = seed0 + np.arange(T)                                # main.py:137-139: seed, seed + 1, ... over the whole sweep
    else:
        # seed: null is legal in the reference: main.py:138 skips the increment and NoiseProfiler(seed=None) falls back to
        # default_rng() per generator (noise.py:61-70), i.e. every trial gets independent OS-entropy streams.  Draw one fresh
        # 62-bit seed per trial (so that seed + 10 j and 2 seed + i stay below 2^64) and keep them in the plan / npz sink:
        # the run is then reproducible after the fact, and no two trials share a noise realisation.
        seeds = (np.random.SeedSequence().generate_state(T, np.uint64) >> np.uint64(2)).astype(np.int64)
    return TrialPlan(cell=np.repeat(np.arange(len(cells)), epoch), value=np.repeat(cells, epoch), seed=seeds, q_start=q0, cells=cells)


class NoiseSpec:
    """What a config says about the measurement noise, but for the swept value of a cell."""

    def __init__(self, cfg):
        ex, nz = cfg['experiments'], cfg['noise']
        self.type, self.params, self.hold, self.m = NoiseType[nz['type']], nz['noise_params'], nz['hold'], len(ex['desired_f'])
        self.key = 'alpha' if self.type == NoiseType.ALPHA_STABLE else 'rho'    # the swept parameter (main.py:104-106)
        self.hold_cnt = int(nz['hold_time'] / ex['dt'])             # main.py:137

    def cell_params(self, value):
        return {**self.params, self.key: float(value)}              # main.py:123-126


def trial_noise(cfg, plan, lo, hi, steps, out):
    """Fill ``out`` (logical [trial][step][m] array-like covering trials lo..hi) with the reference's noise streams."""
    nd = NoiseSpec(cfg)
    for c in np.unique(plan.cell[lo:hi]):
        idx = np.nonzero(plan.cell[lo:hi] == c)[0]
        out[idx] = noise_batch(nd.type, nd.cell_params(plan.cells[c]), plan.seed[lo:hi][idx], nd.m, steps, nd.hold, nd.hold_cnt)
    return out


@dataclass
class BatchResult:
    plan: TrialPlan
    lo: int
    hi: int
    t: np.ndarray
    stats: object            # (T_local, 3) cuda tensor
    status: object           # (T_local,) int32 cuda tensor
    k_done: object
    streams: dict            # optional per-step tensors, trial-fastest [K][comp][T_local]
    noise: object
    seconds: float = 0.0


def _upload_seeds(seeds, device):
    """int64 device tensor of the uint64 bit patterns of ``seeds``: one upload for a shard, sliced per piece."""
    return engine._torch().as_tensor(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64), device=device)


def _cell_noise(nd, value, seeds, seeds_dev, steps, device, share=True, out=None):
    """Noise streams, [step][feature][trial], of the trials of ONE cell (swept value ``value``) whose seeds are ``seeds`` (host) / ``seeds_dev`` (their
    _upload_seeds slice, or None: uploaded here), generated on the GPU (noise_device.py).  ``share``: where the trials' streams alias
    (noise_device.shares_streams: consecutive seeds, no hold) generate the T + 70 distinct streams once and return an overlapping view (main.py:137-139 +
    noise.py:70) -- bit-identical to the per-trial generation.  ``out``: None (a fresh tensor), a flat fp64 buffer of at least steps x max(T + 70, m T)
    that either form is laid into, or -- with ``share`` off -- the [step][feature][trial] destination."""
    T, m = len(seeds), nd.m
    params = nd.cell_params(value)
    flat = out is not None and out.dim() == 1
    if share and (out is None or flat) and noise_device.shares_streams(nd.type, nd.hold, seeds):
        S = T + noise_device.SEED_STEP * (m - 1)
        return noise_device.generate_shared(nd.type, params, int(seeds[0]), T, m, steps, out=out[:steps * S].view(steps, S) if flat else None, device=device)[1]
    if out is None:
        out = engine.alloc_stream(T, steps, m, 'kct', device)
    elif flat:
        out = out[:steps * m * T].view(steps, m, T)
    return noise_device.generate(nd.type, params, seeds if seeds_dev is None else seeds_dev, m, steps, nd.hold, nd.hold_cnt, 'kct', out=out, device=device)


def device_noise(cfg, plan, lo, hi, steps, device='cuda', share=True):
    """Noise streams of trials lo..hi generated on the GPU, [step][feature][trial] (_cell_noise).  ``share``: where the shard is one cell whose trials'
    streams alias, generate each distinct stream once and return an overlapping view."""
    nd = NoiseSpec(cfg)
    runs = sweep_pieces(plan, lo, hi)                               # cells are contiguous runs of trials (main.py:121-127)
    if len(runs) == 1:
        return _cell_noise(nd, plan.cells[runs[0][2]], plan.seed[lo:hi], None, steps, device, share)
    out = engine.alloc_stream(hi - lo, steps, nd.m, 'kct', device)
    seeds_dev = _upload_seeds(plan.seed[lo:hi], device)
    for a, b, c in runs:
        _cell_noise(nd, plan.cells[c], plan.seed[a:b], seeds_dev[a - lo:b - lo], steps, device, False, out[:, :, a - lo:b - lo])
    return out


@dataclass
class LaunchSetup:
    """What a reference config means to a launch (launch_setup)."""
    cfg: dict                # validated (load_config)
    method: Method
    analytical: bool
    plant: object
    fp: object               # uvs_filter_params, option bits in ``reserved``
    t_log: np.ndarray        # engine.loop_clock: the K logged times
    K: int
    m: int
    n: int
    x0: np.ndarray           # (1, m n) row of estimator_params['x0'] when initial_guess is false, else None
    noise: NoiseSpec

    @functools.cached_property
    def plant_struct(self):
        """uvs_plant, made on first use: a LinearPlant uploads its arrays to the device that is current then."""
        return self.plant.to_struct()

    def x0_rows(self, T, device):
        """(T, m n) device tensor of the x0 row, or None."""
        return None if self.x0 is None else engine._torch().as_tensor(self.x0.repeat(T, 0), device=device)

    def closed_loop(self, q_start, noise, x0, want, reuse=None, trial_params=None):
        """The engine launch of this method; ``x0``: x0_rows(...) of at least as many trials, or None."""
        if self.analytical:
            return engine.analytical_closed_loop(self.fp, self.plant_struct, q_start, noise, want=want, reuse=reuse)
        return engine.closed_loop(self.fp, self.plant_struct, q_start, noise, x0, want=want, reuse=reuse, trial_params=trial_params)


def launch_setup(cfg, plant=None, lanes=0, strict_pinv=False, latency=False):
    """Everything run_batch, run_sweep and run_grid derive from a reference config before they touch the device -- THE place where an estimator
    parameter, its default, an option bit or a noise rule is read.  Host only.  Raises what load_config raises, ValueError for ANALYTICAL with lane
    options and KeyError when an estimator's ``initial_guess`` is missing (ANALYTICAL, which estimates nothing, defaults it).  ``strict_pinv`` /
    ``latency``: the library's launch options UVS_OPT_STRICT_PINV and UVS_OPT_LATENCY -- not part of config.json, whose schema stays the reference's."""
    cfg = load_config(cfg)
    ex, est = cfg['experiments'], cfg['estimator']
    method = Method[est['method']]
    # the calibrated baseline (engine.analytical_closed_loop) runs one lane per trial, so the estimators' lane options do not apply; the reference's
    # Experiment.run() crashes there (R unbound, experiment.py:121) in two lines only the estimators use
    analytical = method == Method.ANALYTICAL
    if analytical and (lanes or latency):
        raise ValueError('lanes / latency select estimator kernels; the ANALYTICAL closed loop has one mapping (strict_pinv applies)')
    plant = SyntheticPlant.ur10(ex['desired_f']) if plant is None else plant
    p = est.get('estimator_params') or {}
    m, n = len(ex['desired_f']), plant.n_joints
    initial_guess = p.get('initial_guess', True) if analytical else p['initial_guess']
    t_log = engine.loop_clock(ex['dt'], ex['t_max'])
    fp = engine.make_params(m, n, method.name, p.get('kernel_bw', 1.0), p.get('annealing', False), ex['dt'], ex['t_max'], ex['ibvs_gain'],
                            ex['desired_f'], initial_guess, lanes, len(t_log), p.get('fpi_threshold', 0.1), p.get('fpi_epoch_max', 1000))
    fp.reserved = (_lib.UVS_OPT_STRICT_PINV if strict_pinv else 0) | (_lib.UVS_OPT_LATENCY if latency else 0)
    x0 = None if analytical or initial_guess else np.asarray(p['x0'], float).reshape(1, m * n)
    return LaunchSetup(cfg, method, analytical, plant, fp, t_log, len(t_log), m, n, x0, NoiseSpec(cfg))


def run_batch(cfg, plant=None, cells=None, epoch=None, rank=0, world=1, want=('err',), lanes=0, noise_tensor=None,
              device='cuda', noise_on_device=True, strict_pinv=False, latency=False):
    """Run this rank's shard of the sweep on its GPU.  Returns a BatchResult whose tensors stay on the device.
    ``noise_on_device``: generate the measurement noise with the HIP generator (default) or with numpy on the host.
    ``strict_pinv`` / ``latency``: the library's launch options UVS_OPT_STRICT_PINV (numpy's pinv on every control-law solve, slower) and
    UVS_OPT_LATENCY (four lanes per filter for shards that do not fill the chip: last-bit differences), see launch_setup."""
    import torch
    s = launch_setup(cfg, plant, lanes, strict_pinv, latency)
    plan = plan_trials(s.cfg, cells, epoch)
    lo, hi = dist.shard_range(len(plan), rank, world)
    dev = engine.current_device(device)
    with torch.cuda.device(dev):                                    # the engine launches on the CURRENT device's current stream
        if noise_tensor is None and noise_on_device:
            noise_tensor = device_noise(s.cfg, plan, lo, hi, s.K, dev)
        if noise_tensor is None:
            host = np.empty((s.K, s.m, hi - lo))
            trial_noise(s.cfg, plan, lo, hi, s.K, host.transpose(2, 0, 1))  # logical [trial][step][m] view of the trial-fastest buffer
            noise_tensor = torch.as_tensor(host, device=dev)
        q0 = torch.as_tensor(plan.q_start[lo:hi].copy(), device=dev)
        out = s.closed_loop(q0, noise_tensor, s.x0_rows(hi - lo, dev), want)
    start, stop = out['events']                                     # HIP events around the kernel launch (output allocation excluded)
    stop.synchronize()
    return BatchResult(plan, lo, hi, s.t_log, out['stats'], out['status'], out['k_done'],
                       {k: out[k] for k in ('x', 'j', 'err', 'q', 'f', 'dq') if out.get(k) is not None}, noise_tensor,
                       start.elapsed_time(stop) * 1e-3)


_COPY_STREAMS = {}


def sweep_pieces(plan, lo, hi, max_trials=None):
    """[(a, b, cell)]: this shard's trials [lo, hi) cut at the cell boundaries (main.py:121-127: a cell is a contiguous run of trials) and,
    when ``max_trials`` is given, into pieces of at most that many trials -- the launches of run_sweep, in trial order."""
    out, a = [], lo
    while a < hi:
        c = int(plan.cell[a])
        b = a + int(np.searchsorted(plan.cell[a:hi], c, side='right'))
        if max_trials:
            b = min(b, a + int(max_trials))
        out.append((a, b, c))
        a = b
    return out


@dataclass
class SweepResult:
    """Per-trial rows of a shard of the sweep on the HOST (pinned memory): what main.py keeps of a trial once its CSV rows are written."""
    plan: TrialPlan
    lo: int
    hi: int
    stats: np.ndarray        # (T_local, 3)  ||ISE||_2, ||IAE||_2, ||ITAE||_2
    status: np.ndarray       # (T_local,) int32
    k_done: np.ndarray       # (T_local,) int32
    pieces: list
    seconds: float = 0.0     # wall clock of the whole sweep, synchronised on both sides

    def rows(self):
        """(T_local, 5) fp64 [ISE, IAE, ITAE, status, k_done]."""
        return np.concatenate([self.stats, self.status[:, None].astype(float), self.k_done[:, None].astype(float)], axis=1)

    def cell_summary(self):
        from . import stats as _stats
        return _stats.cell_summary(self.stats, self.status, self.plan.cell[self.lo:self.hi])

    def gather(self, group=None, device=None):
        """The rows of ALL ranks in global trial order, (len(plan), 5), on every rank: the sweep's one collective, an all-gather
        of 40 B per trial.  ``device``: where the exchanged tensors live -- a cuda device for the nccl (RCCL) backend, None (host) for gloo."""
        import torch
        rows = torch.from_numpy(np.ascontiguousarray(self.rows()))
        if device is not None:
            rows = rows.to(device)
        return dist.gather_trial_rows(rows, len(self.plan), group).cpu().numpy()


def _check_plan(plan, cfg, cells, epoch):
    """A plan made earlier must be THIS sweep's: a stale one would silently run other seeds / cells."""
    ex, nz = cfg['experiments'], cfg['noise']
    n_cells = len(sweep_cells(NoiseType[nz['type']])) if cells is None else len(cells)
    per_cell = int(ex['epoch'] if epoch is None else epoch)
    first_seed = nz['seed']
    if len(plan) != n_cells * per_cell or len(plan.cells) != n_cells or (cells is not None and not np.array_equal(plan.cells, np.asarray(cells, float))) or \
            (first_seed is not None and len(plan) and int(plan.seed[0]) != int(first_seed)) or \
            (len(plan) and not ex['change_q_start'] and not np.array_equal(plan.q_start[0], np.asarray(ex['q_start'], float))):
        raise ValueError('run_sweep(plan=...): the plan does not belong to this config / cells / epoch')


def run_sweep(cfg, plant=None, cells=None, epoch=None, rank=0, world=1, want=(), lanes=0, device='cuda', max_trials=None,
              share_noise=True, on_piece=None, strict_pinv=False, latency=False, plan=None):
    """The whole sweep of main.py:104-148 on this rank's GPU, cell after cell through ONE set of device buffers: for each piece (a cell, or
    ``max_trials`` trials of it) device seeding + noise generation (the T + 70 distinct streams where they alias), the closed-loop launch,
    and the per-trial [ISE, IAE, ITAE], status, k_done copied to pinned host memory on a second stream while the next piece computes.
    Device memory is that of the largest piece, whatever the sweep's size; results are bit-identical to ``run_batch`` over the same trials
    (same global seeds and jitter draws; a rank of ``world`` owns the contiguous global trials of dist.shard_range).

    ``want``: per-step streams to log on the device; they live until the next piece overwrites them, so ``on_piece(a, b, cell, out)`` --
    called after the piece has finished, with engine.closed_loop's dict -- is where a sink consumes them (it serialises the pipeline).
    ``plan``: a TrialPlan of this config made earlier (plan_trials takes 0.3 s for 786 432 trials; the GPU idles and clocks down meanwhile).
    The engine launches on the CURRENT device's current stream: the sweep runs with ``device`` made current, so that the events that order the
    row copies against the kernels are recorded on the stream the kernels are launched on."""
    import time
    import torch
    s = launch_setup(cfg, plant, lanes, strict_pinv, latency)       # (refusals before any device work)
    if plan is None:
        plan = plan_trials(s.cfg, cells, epoch)
    else:
        _check_plan(plan, s.cfg, cells, epoch)
    lo, hi = dist.shard_range(len(plan), rank, world)
    pieces = sweep_pieces(plan, lo, hi, max_trials)
    K, m, n, Tl = s.K, s.m, s.n, hi - lo
    dev = engine.current_device(device)
    with torch.cuda.device(dev):
        host = dict(stats=torch.empty((Tl, 3), dtype=torch.float64).pin_memory(), status=torch.empty(Tl, dtype=torch.int32).pin_memory(),
                    k_done=torch.empty(Tl, dtype=torch.int32).pin_memory())
        if not pieces:
            return SweepResult(plan, lo, hi, host['stats'].numpy(), host['status'].numpy(), host['k_done'].numpy(), pieces)
        Tmax = max(b - a for a, b, _ in pieces)
        q0 = torch.as_tensor(plan.q_start[lo:hi].copy(), device=dev)
        x0 = s.x0_rows(Tmax, dev)
        seeds_dev = _upload_seeds(plan.seed[lo:hi], dev)
        # two sets of per-trial outputs (a set is copied out while the next piece writes the other), one set of streams, one noise buffer
        S = Tmax + noise_device.SEED_STEP * (m - 1)
        noise_buf = torch.empty(K * max(S, m * Tmax), dtype=torch.float64, device=dev)
        streams = {k_: engine.alloc_stream(Tmax, K, c, 'kct', dev) for k_, c in (('x', m * n), ('j', m * n), ('err', m), ('q', n), ('f', m), ('dq', n))
                   if k_ in want}
        # the streams are allocated ONCE and shared by both sets (7.5 GB of X per 65 536 trials)
        sets = [dict(streams, stats=torch.zeros((Tmax, 3), dtype=torch.float64, device=dev), status=torch.zeros(Tmax, dtype=torch.int32, device=dev),
                     k_done=torch.zeros(Tmax, dtype=torch.int32, device=dev)) for _ in range(2)]
        main = torch.cuda.current_stream(dev)
        copier = _COPY_STREAMS.get(str(dev))                       # one per device, kept: the first use of a new stream costs ~4 ms on the host
        if copier is None:                                         # (queue creation), during which the GPU runs dry
            copier = _COPY_STREAMS[str(dev)] = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(copier):
                torch.zeros(1, device=dev)
        copied = []
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i, (a, b, c) in enumerate(pieces):
            noise = _cell_noise(s.noise, plan.cells[c], plan.seed[a:b], seeds_dev[a - lo:b - lo], K, dev, share_noise, noise_buf)
            if i >= 2:
                main.wait_event(copied[i - 2])                      # this set's previous rows have left the device
            out = s.closed_loop(q0[a - lo:b - lo], noise, None if x0 is None else x0[:b - a], want, reuse=sets[i % 2])
            done = torch.cuda.Event()
            done.record(main)
            copier.wait_event(done)
            with torch.cuda.stream(copier):
                for k_ in ('stats', 'status', 'k_done'):
                    host[k_][a - lo:b - lo].copy_(out[k_], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copier)
            copied.append(ev)
            if on_piece is not None:
                done.synchronize()
                on_piece(a, b, c, out)
        torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
    return SweepResult(plan, lo, hi, host['stats'].numpy(), host['status'].numpy(), host['k_done'].numpy(), pieces, seconds)


GRID_KEYS = ('kernel_bw', 'ibvs_gain', 'fpi_threshold')          # config names of what a grid may vary -> trial_params 'kernel_bw', 'gain', 'fpi_threshold'


@dataclass
class GridPlan:
    """A hyperparameter grid over the trials of one noise cell: grid cell h has the values ``values[h]`` (one column per axis of ``axes``, the
    product of the axes in the order given, last axis fastest), launch ``pieces[i] = (h_lo, h_hi)`` runs grid cells [h_lo, h_hi) as
    (h_hi - h_lo) x epoch trials, trial t of a launch reading the inputs of trial ``t % epoch`` of the noise cell (``source``)."""
    axes: dict               # name -> list of values, as given
    values: np.ndarray       # (H, len(axes))
    epoch: int
    pieces: list

    def __len__(self):
        return len(self.values)

    def source(self, h_lo, h_hi):
        return np.tile(np.arange(self.epoch, dtype=np.int32), h_hi - h_lo)

    def column(self, name, h_lo, h_hi):
        """Per-trial values of axis ``name`` for the launch of grid cells [h_lo, h_hi)."""
        return np.repeat(self.values[h_lo:h_hi, list(self.axes).index(name)], self.epoch)

    def substituted(self, cfg, h):
        """The config whose uniform sweep grid cell ``h`` reproduces bit for bit."""
        cfg = json.loads(json.dumps(load_config(cfg)))
        for name, v in zip(self.axes, self.values[h]):
            if name == 'ibvs_gain':
                cfg['experiments']['ibvs_gain'] = float(v)
            else:
                cfg['estimator']['estimator_params'][name] = float(v)
        return cfg


def plan_grid(grid, epoch, max_trials=None):
    """GridPlan of ``grid`` (a dict mapping any of GRID_KEYS to a list of values) over ``epoch`` trials per cell; launches of at most
    ``max_trials`` trials, cut at grid-cell boundaries (at least one grid cell per launch)."""
    unknown = [k for k in grid if k not in GRID_KEYS]
    if unknown or not grid:
        raise ValueError(f'run_grid: grid maps any of {GRID_KEYS} to a list of values, got {list(grid)}')
    axes = {k: [float(v) for v in vs] for k, vs in grid.items()}
    if any(len(vs) == 0 for vs in axes.values()):
        raise ValueError('run_grid: an axis of the grid is empty')
    mesh = np.meshgrid(*axes.values(), indexing='ij')
    values = np.stack([g.reshape(-1) for g in mesh], axis=1)
    H = len(values)
    per = H if not max_trials else max(1, int(max_trials) // int(epoch))
    return GridPlan(axes, values, int(epoch), [(h, min(H, h + per)) for h in range(0, H, per)])


@dataclass
class GridResult:
    """Per-trial rows of run_grid on the host, indexed (noise cell, grid cell, trial of the cell)."""
    plan: TrialPlan
    grid: GridPlan
    stats: np.ndarray        # (C, H, epoch, 3)
    status: np.ndarray       # (C, H, epoch) int32
    k_done: np.ndarray       # (C, H, epoch) int32
    seconds: float = 0.0

    def rows(self):
        """(C, H, epoch, 5) fp64 [ISE, IAE, ITAE, status, k_done]."""
        return np.concatenate([self.stats, self.status[..., None].astype(float), self.k_done[..., None].astype(float)], axis=-1)

    def cell_summary(self):
        """{(noise cell, grid cell): stats.cell_summary's entry}."""
        from . import stats as _stats
        out = {}
        for c in range(self.stats.shape[0]):
            H, E = self.status.shape[1:]
            summ = _stats.cell_summary(self.stats[c].reshape(H * E, 3), self.status[c].reshape(-1), np.repeat(np.arange(H), E))
            out.update({(c, h): v for h, v in summ.items()})
        return out


def run_grid(cfg, grid, cells=None, epoch=None, want=(), lanes=0, device='cuda', plant=None, max_trials=None, on_piece=None):
    """A hyperparameter study in one launch per noise cell: every grid cell of ``grid`` (plan_grid: kernel_bw x ibvs_gain x fpi_threshold, any subset)
    over the SAME trials -- plan_trials' seeds and start-pose jitter, unchanged -- instead of one sweep per grid cell.  For every noise cell the noise
    of its ``epoch`` trials is generated once (the shared T + 70 streams where they alias, as run_sweep does), then ONE launch of H x epoch trials
    with per-trial parameters reads them through ``source = t % epoch`` (engine.closed_loop(trial_params=...); pieces of at most ``max_trials``
    trials, cut at grid-cell boundaries).  Contract: grid cell h equals run_sweep on ``GridPlan.substituted(cfg, h)``, bit for bit.
    ``on_piece(c, h_lo, h_hi, out)`` is called after each launch has finished (c: noise cell) with engine.closed_loop's dict, where a sink reads the
    ``want`` streams.  Method.ANALYTICAL has no per-trial kernel: ValueError (as have strict_pinv and latency, which this function does not offer)."""
    import time
    import torch
    cfg = load_config(cfg)
    if Method[cfg['estimator']['method']] == Method.ANALYTICAL:
        raise ValueError('run_grid: Method.ANALYTICAL has no per-trial parameters (no bandwidth, and no per-trial kernel for its gain)')
    if lanes not in (0, 2):
        raise ValueError('run_grid: lanes must be 0 or 2 (the per-trial kernels run two lanes per filter)')
    plan = plan_trials(cfg, cells, epoch)
    E = int(cfg['experiments']['epoch'] if epoch is None else epoch)
    gp = plan_grid(grid, E, max_trials)
    s = launch_setup(cfg, plant, lanes)
    C_, H = len(plan.cells), len(gp)
    stats = np.empty((C_, H, E, 3))
    status = np.empty((C_, H, E), np.int32)
    k_done = np.empty((C_, H, E), np.int32)
    dev = engine.current_device(device)
    with torch.cuda.device(dev):
        q0 = torch.as_tensor(plan.q_start.copy(), device=dev)
        x0 = s.x0_rows(E, dev)
        seeds_dev = _upload_seeds(plan.seed, dev)
        names = {'kernel_bw': 'kernel_bw', 'ibvs_gain': 'gain', 'fpi_threshold': 'fpi_threshold'}
        launches = []                                              # per piece: trial_params on the device, made once
        for h_lo, h_hi in gp.pieces:
            tp = {names[k_]: torch.as_tensor(gp.column(k_, h_lo, h_hi), device=dev) for k_ in gp.axes}
            tp['source'] = torch.as_tensor(gp.source(h_lo, h_hi), device=dev)
            launches.append(tp)
        reuse = None
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for c in range(C_):
            a, b = c * E, (c + 1) * E
            noise = _cell_noise(s.noise, plan.cells[c], plan.seed[a:b], seeds_dev[a:b], s.K, dev)      # a fresh tensor per noise cell
            for (h_lo, h_hi), tp in zip(gp.pieces, launches):
                out = s.closed_loop(q0[a:b], noise, x0, want, reuse=reuse, trial_params=tp)
                if reuse is None:
                    reuse = out                                    # the first piece is the largest: later ones write into its tensors
                hc = h_hi - h_lo
                stats[c, h_lo:h_hi] = out['stats'].cpu().numpy().reshape(hc, E, 3)
                status[c, h_lo:h_hi] = out['status'].cpu().numpy().reshape(hc, E)
                k_done[c, h_lo:h_hi] = out['k_done'].cpu().numpy().reshape(hc, E)
                if on_piece is not None:
                    on_piece(c, h_lo, h_hi, out)
        torch.cuda.synchronize(dev)
    return GridResult(plan, gp, stats, status, k_done, time.perf_counter() - t0)


CSV_COLUMNS = (['experiment_id', 'status', 'rho', 't'] + [f'q_{i}' for i in range(1, 7)] +
               ['camera_x', 'camera_y', 'camera_z', 'camera_roll', 'camera_pitch', 'camera_yaw'] +
               [f'f_{i}' for i in range(1, 9)] + [f'desired_f_{i}' for i in range(1, 9)] + [f'noise_{i}' for i in range(1, 9)] + ['kernel_bw'])


def write_results_csv(result, cfg, plant, path):
    """results.csv in the reference's long format (main.py:152-196): one row per logged step, 41 columns.  Needs the
    'q' and 'f' streams; meant for sweeps of the reference's size (~10^3 trials) -- larger runs keep tensors/npz."""
    import pandas as pd
    q = result.streams['q'].cpu().numpy()
    f = result.streams['f'].cpu().numpy()
    noise = result.noise.cpu().numpy()
    status, k_done = result.status.cpu().numpy(), result.k_done.cpu().numpy()
    desired = np.asarray(cfg['experiments']['desired_f'], float)
    method, p = Method[cfg['estimator']['method']], cfg['estimator']['estimator_params']
    header = not os.path.exists(path)
    for j in range(result.hi - result.lo):
        k = int(k_done[j])
        cam = plant.camera_pose_batch(q[:k, :, j]) if k else np.zeros((0, 6))   # computePose (ur10_simulation.py:151-163)
        cols = {'experiment_id': result.lo + j, 'status': ExperimentStatus(int(status[j])), 'rho': result.plan.value[result.lo + j],
                't': result.t[:k]}
        cols.update({f'q_{i + 1}': q[:k, i, j] for i in range(6)})
        cols.update({name: cam[:, i] for i, name in enumerate(CSV_COLUMNS[10:16])})
        cols.update({f'f_{i + 1}': f[:k, i, j] for i in range(8)})
        cols.update({f'desired_f_{i + 1}': np.full(k, desired[i]) for i in range(8)})
        cols.update({f'noise_{i + 1}': noise[:k, i, j] for i in range(8)})
        cols['kernel_bw'] = bandwidth_log(method, k, p.get('kernel_bw', 1.0), p.get('annealing', False), cfg['experiments']['dt'],
                                          cfg['experiments']['t_max'])                      # -1 unless MCKF (experiment.py:330)
        pd.DataFrame(data=cols).to_csv(path, mode='a', index=False, header=header)
        header = False


def write_results_parquet(result, cfg, plant, path, trials_per_group=2048):
    """The reference's results table (main.py:152-196: one row per logged step, the 41 columns of results.csv, same names, same order) as a
    Parquet file, for sweeps where the long-format CSV is impractical (65 536 trials x 299 rows x 41 columns is 6.7 GB of text).  Streams:
    ``trials_per_group`` trials at a time are copied from the device, expanded and written as one row group, so the host never holds more
    than one group (2 048 trials = 612 352 rows = 200 MB).  ``status`` is the reference's string (``ExperimentStatus.SUCCESS``), dictionary
    encoded; rows at and after a FAILed trial's k_done are dropped as the reference trims them (experiment.py:345-352).  Needs the 'q' and
    'f' streams.  Returns the number of rows written."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    desired = np.asarray(cfg['experiments']['desired_f'], float)
    method, p = Method[cfg['estimator']['method']], cfg['estimator']['estimator_params']
    status_all, k_all = result.status.cpu().numpy(), result.k_done.cpu().numpy()
    T, K = result.hi - result.lo, len(result.t)
    bw_full = bandwidth_log(method, K, p.get('kernel_bw', 1.0), p.get('annealing', False), cfg['experiments']['dt'], cfg['experiments']['t_max'])
    names = {0: str(ExperimentStatus(0)), 1: str(ExperimentStatus(1))}
    writer, rows_written = None, 0
    try:
        for a in range(0, T, trials_per_group):
            b = min(T, a + trials_per_group)
            q = result.streams['q'][:, :, a:b].cpu().numpy()               # [K][6][chunk]
            f = result.streams['f'][:, :, a:b].cpu().numpy()
            nz = result.noise[:, :, a:b].cpu().numpy()
            keep = (np.arange(K)[None, :] < k_all[a:b, None])              # (chunk, K): logged rows
            tt, kk = np.nonzero(keep)                                      # trial-major, step-minor: the reference's row order
            cam = plant.camera_pose_batch(np.moveaxis(q, 1, 2)[kk, tt])     # (rows, 6)
            cols = {'experiment_id': (result.lo + a + tt).astype(np.int64),
                    'status': pa.array([names[int(v)] for v in status_all[a:b]]).dictionary_encode().take(pa.array(tt)),
                    'rho': result.plan.value[result.lo + a + tt], 't': np.asarray(result.t)[kk]}
            cols.update({f'q_{i + 1}': q[kk, i, tt] for i in range(6)})
            cols.update({name: cam[:, i] for i, name in enumerate(CSV_COLUMNS[10:16])})
            cols.update({f'f_{i + 1}': f[kk, i, tt] for i in range(8)})
            cols.update({f'desired_f_{i + 1}': np.full(len(tt), desired[i]) for i in range(8)})
            cols.update({f'noise_{i + 1}': nz[kk, i, tt] for i in range(8)})
            cols['kernel_bw'] = bw_full[kk]
            table = pa.table({name: cols[name] for name in CSV_COLUMNS})
            if writer is None:
                writer = pq.ParquetWriter(path, table.schema, compression='zstd')
            writer.write_table(table)
            rows_written += len(tt)
    finally:
        if writer is not None:
            writer.close()
    return rows_written


def save_results_npz(result, cfg, path, streams=True):
    """Compact sink for sweeps too large for the long-format CSV (65 536 trials x 299 rows x 41 columns is 6.7 GB of text):
    per-trial rows (experiment_id, swept value, seed, status, k_done, ISE / IAE / ITAE norms, q_start), the clock, the config,
    and -- if ``streams`` -- whatever per-step tensors the run kept, trial-fastest as on the device ([step][component][trial]).
    For a FAILed trial only the first ``k_done`` rows of a stream are meaningful (the reference trims its logs there, experiment.py:345-352)."""
    data = {'experiment_id': np.arange(result.lo, result.hi), 'cell': result.plan.cell[result.lo:result.hi],
            'rho': result.plan.value[result.lo:result.hi], 'seed': result.plan.seed[result.lo:result.hi],
            'q_start': result.plan.q_start[result.lo:result.hi], 't': np.asarray(result.t),
            'status': result.status.cpu().numpy(), 'k_done': result.k_done.cpu().numpy(), 'stats': result.stats.cpu().numpy(),
            'stats_columns': np.array(['ise', 'iae', 'itae']), 'config': json.dumps(cfg)}
    if streams:
        for name, tensor in result.streams.items():
            data['stream_' + name] = tensor.cpu().numpy()
    np.savez_compressed(path, **data)
    return path
