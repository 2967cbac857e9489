"""PGPE on the device: the search half of the reference's examples/learning_agents.py (evotorch's `PGPE`, as `run_agent`
configures it), with the whole searcher state in HBM (die_pgpe_sample / die_pgpe_update, die_amd/csrc/die_search.hip).

    searcher = PGPE(10, center_init=rows0, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                    optimizer='clipup', optimizer_config=dict(max_speed=0.1, momentum=0.9))
    searcher.for_population(pop, epoch_iters=30).run(100)        # pop: a BatchedNeuralAutomataAgent of 10 candidates
    searcher.best_agent().save(...)

A generation is ask (one launch: symmetric samples into the (R, P) parameter matrix), the batched worlds' reset (device copies),
`epoch_iters` batched steps and tell (three or four launches: fitness, centred ranks, gradients, the optimiser's step, pop_best /
best, one row of statistics) — a fixed chain of launches with no host read.  The generic interface, `ask(params)` /
`tell(terms)`, works on any (R, P) float32 device matrix and any (T, R) float64 terms.

Differences from evotorch: the noise comes from Philox (counter-based, seeded), so a run is reproducible here but
not bit-equal to evotorch's; the fitness is the plain sum of a candidate's T terms.

CMAES (die_cmaes_sample / die_cmaes_update, die_amd/csrc/die_cmaes.hip) is the reference's other searcher (evotorch's
`CMAES(problem, stdev_init=0.1, popsize=10, separable=True)`): separable CMA-ES with the same population surface and the same
no-host-read generation.

Episodes: a population built with `episodes=E` evaluates each of the searcher's `popsize` candidates on E worlds in the same
launches (R = popsize·E replicas); `tell(terms, episodes=E)` folds the E sums of a candidate into its mean with one more
launch (die_*_update_episodes) and keeps them in `episode_fitness`."""
import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from .batch import BatchedNeuralAutomataAgent, _is_integer, _worlds_per_candidate, episode_seeds
from .device_array import _ptr, stream_ptr

OPTIMIZERS = {'clipup': _lib.DIE_PGPE_CLIPUP, 'adam': _lib.DIE_PGPE_ADAM}
HISTORY_COLUMNS = ('mean_eval', 'max_eval', 'min_eval', 'median_eval', 'grad_norm', 'mean_stdev')


def _resolve_device(device) -> torch.device:
    dev = torch.device(device if device is not None else 'cuda')
    if dev.type == 'cuda' and dev.index is None:                     # ('cuda' is the current device: tensors say cuda:N)
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _initial_center(center_init, num_params, initial_bounds, seed) -> torch.Tensor:
    """The float32 starting centre on the host: `center_init`, or drawn once in `initial_bounds` from the seed."""
    if center_init is not None:
        center = torch.as_tensor(center_init, dtype=torch.float32).detach().reshape(-1).cpu()
        if num_params is not None and center.numel() != int(num_params):
            raise ValueError(f'center_init of {center.numel()} values for num_params={num_params}')
        return center
    if num_params is None:
        raise ValueError('num_params, or a center_init to take it from')
    lo, hi = (float(v) for v in initial_bounds)
    g = torch.Generator().manual_seed(int(seed))          # NEProblem(initial_bounds=...): drawn once, on the host
    return lo + (hi - lo) * torch.rand(int(num_params), generator=g, dtype=torch.float32)


class _PopulationSearch:
    """What PGPE and CMAES share: an (R, P) float32 parameter matrix, a population binding whose generation is ask, reset,
    `epoch_iters` batched steps and tell, a (G, 6) history on the device, the pop_best / best rows as agents.  A subclass sets
    R, P, device, center, iter, _asked, _pop, _history, _s (its ctypes state, with history / history_rows), _pop_best, _best,
    _evals and _update (the name of its update entry point; `<_update>_episodes` folds), and defines ask / tell."""

    def _check_params(self, params: torch.Tensor):
        if tuple(params.shape) != (self.R, self.P) or params.dtype != torch.float32 or params.device != self.device \
                or not params.is_contiguous():
            raise ValueError(f'params: a contiguous ({self.R}, {self.P}) float32 tensor on {self.device}')

    def _check_terms(self, terms: torch.Tensor, episodes: int = 1):
        n = self.R * episodes
        if terms.dtype != torch.float64 or terms.device != self.device or terms.dim() not in (2, 3) \
                or tuple(terms.shape[1:2]) != (n,) or (terms.dim() == 3 and terms.shape[2] < 1) or terms.shape[0] < 1:
            raise ValueError(f'terms: a (T, {n}) or (T, {n}, 2) float64 tensor on {self.device}' +
                             (f' ({self.R} candidates x {episodes} episodes, candidate-major)' if episodes != 1 else ''))

    def _check_episodes(self, episodes) -> int:
        _worlds_per_candidate(episodes)
        if self.R * episodes > _lib.MAX_REPLICAS:
            raise ValueError(f'episodes={episodes}: {self.R} candidates x {episodes} episodes is more than {_lib.MAX_REPLICAS} replicas')
        return episodes

    @property
    def episode_fitness(self) -> torch.Tensor:
        """(C, E) float64 on the device: candidate c's sum of terms on each of its E worlds in the last `tell` (`fitness` is
        their mean, summed in episode order); the spread over e is the luck of the worlds.  E = 1: `fitness` as a column.
        On a `BatchedEnv(dynamics=episode_dynamics(dynamics, C))` column e is the score under dynamics[e]."""
        return self.fitness.view(self.R, 1) if self._episode_fitness is None else self._episode_fitness

    def _fold_buffers(self, episodes: int):
        """The (C, E) per-episode sums and the C folded terms of die_*_update_episodes, allocated at the first use of an E."""
        if self._episode_fitness is None or self._episode_fitness.shape[1] != episodes:
            self._episode_fitness = torch.zeros((self.R, episodes), dtype=torch.float64, device=self.device)
            self._folded = torch.zeros(self.R, dtype=torch.float64, device=self.device)
        return _ptr(self._episode_fitness), _ptr(self._folded)

    def _reserve_history(self):
        if self.iter >= self._history.shape[0]:         # grow the history on the device (no host read)
            h = torch.zeros((2 * self._history.shape[0], 6), dtype=torch.float64, device=self.device)
            h[:self._history.shape[0]].copy_(self._history)
            self._history = h
            self._s.history, self._s.history_rows = _ptr(h), h.shape[0]

    def _tell(self, params: torch.Tensor, terms: torch.Tensor, episodes) -> None:
        """`tell` once the subclass has chosen the rows: the checks, the update (with E > 1 episodes the folding one), iter + 1."""
        self._check_params(params)
        if type(episodes) is not int or episodes != 1:
            episodes = self._check_episodes(episodes)
        self._check_terms(terms, episodes)
        self._reserve_history()
        if episodes == 1:
            name, fold = self._update, ()
            self._episode_fitness = self._folded = None
        else:
            name, fold = self._update + '_episodes', (episodes, *self._fold_buffers(episodes))
        _lib.check(getattr(_lib.lib, name)(C.byref(self._s), _ptr(params), _ptr(terms), terms.shape[0], terms.stride(0), terms.stride(1),
                                           *fold, self.iter, stream_ptr(self.device)), name)
        self.iter += 1

    # ------------------------------------------------------------------ a population of NeuralAutomataAgents
    def for_population(self, pop, epoch_iters: int, env=None, *, reseed: Optional[int] = None, reseed_stride: int = 0):
        """Bind to a BatchedNeuralAutomataAgent: `step()` is then ask into `pop.parameters`, `pop.env.reset()`, `epoch_iters`
        batched steps, tell.  `env`, when given, must be the population's own BatchedEnv.  A BatchedPhysarumPopulation in unit
        mode binds the same way (what is used: R, P, parameters, env, and `reset()` where the population has one — called
        after the worlds' reset: it decodes the asked rows and re-draws the headings); best_agent() / pop_best_agent() /
        center_agent() then return PhysarumAgents.

        `reseed`: a new world every generation instead of the construction worlds — generation g (`iter` at ask) resets with
        `pop.env.reset(seed=reseed + g·R, seed_stride=reseed_stride)`.  Stride 0 (default): every candidate of a generation is
        evaluated on the same fresh world (what antithetic pairs and ranks compare); stride 1: a world per replica and
        generation.  The population's BatchedEnv needs the fixed layout (`max_agents` an int or None).

        A population built with `episodes=E` binds when popsize is its number of CANDIDATES (`pop.candidates`; a population
        without that attribute: `pop.R`): every generation then steps R = C·E replicas and `tell` folds with episodes=E.
        With `reseed`, generation g gives replica (c, e) the world of reseed + g·C·E + e + reseed_stride·c·E through
        `reset(seeds=...)` — stride 0: every candidate sees the same E fresh worlds; stride 1: every replica its own; E = 1:
        the formula above."""
        if any(not hasattr(pop, name) for name in ('R', 'P', 'parameters', 'env')):
            raise TypeError('pop: a BatchedNeuralAutomataAgent or a BatchedPhysarumPopulation (R, P, parameters, env)')
        if getattr(pop, 'natural', False):
            raise ValueError('a BatchedPhysarumPopulation of natural rows: one step size does not suit six units — build it in '
                             'unit mode (parameters=, space=ParameterSpace(lo, hi)) to search it')
        if env is not None and env is not pop.env:
            raise ValueError('this population was built for another BatchedEnv')
        candidates, episodes = getattr(pop, 'candidates', pop.R), getattr(pop, 'episodes', 1)
        if candidates != self.R:
            raise ValueError(f'popsize {self.R} != the population\'s {candidates} ' +
                             ('replicas' if episodes == 1 else f'candidates ({pop.R} replicas of {episodes} episodes each)'))
        self._check_episodes(episodes)
        if pop.P != self.P:
            raise ValueError(f'{self.P} search parameters for a population of {pop.P}')
        if pop.parameters.device != self.device:
            raise ValueError(f'population on {pop.parameters.device}, searcher on {self.device}')
        if int(epoch_iters) < 1:
            raise ValueError('epoch_iters: at least 1')
        if reseed is not None:
            if not _is_integer(reseed, exact=True):
                raise ValueError(f'reseed={reseed!r}: an integer seed, or None for the construction worlds')
            if not _is_integer(reseed_stride, 0, exact=True):
                raise ValueError(f'reseed_stride={reseed_stride!r}: a non-negative integer')
            if pop.env._fixed is None:
                raise ValueError("reseed needs a BatchedEnv with max_agents=N (or None for W·H): the 'alive' layout holds K_r slots "
                                 'per replica, and a new world has a new K_r')
        self._reseed, self._reseed_stride = reseed, int(reseed_stride)
        self._pop, self._epoch_iters, self._episodes = pop, int(epoch_iters), episodes
        # a population with state of its own between generations (a PhysarumAgent population's headings and table) says so
        # with a `reset()`.  BatchedNeuralAutomataAgent has none ON PURPOSE: its generation is ask, env.reset, steps, tell and
        # nothing else — giving it a `reset` method would add a call to every NCA generation
        self._pop_reset = getattr(pop, 'reset', None)
        self._results = torch.empty((self._epoch_iters, self.R * episodes, 2), dtype=torch.float64, device=self.device)
        if episodes > 1:
            self._fold_buffers(episodes)                # (allocated here, not in the first generation)
        else:
            self._episode_fitness = self._folded = None
        return self

    def step(self) -> None:
        """One generation on the bound population (no host read)."""
        if self._pop is None:
            raise RuntimeError('step(): bind a population first (for_population)')
        pop, env = self._pop, self._pop.env
        g = self.iter
        self.ask(pop.parameters)
        if self._reseed is None:
            env.reset()
        elif self._episodes == 1:
            env.reset(seed=self._reseed + g * self.R, seed_stride=self._reseed_stride)
        else:                                           # E > 1: the worlds from the seed list (and the fold in tell)
            env.reset(seeds=self._generation_seeds(g))
        if self._pop_reset is not None:
            self._pop_reset()
        for t in range(self._epoch_iters):
            env.step(pop, self._results[t])
        self.tell(self._results, episodes=self._episodes)

    def _generation_seeds(self, g: int):
        """The worlds of generation g under `reseed`: replica c·E + e gets reseed + g·C·E + e + reseed_stride·c·E."""
        return episode_seeds(self._reseed + g * self.R * self._episodes, self.R, self._episodes, self._reseed_stride)

    def run(self, generations: int) -> None:
        for _ in range(int(generations)):
            self.step()

    # ------------------------------------------------------------------ results (read on demand)
    def history(self) -> torch.Tensor:
        """(G, 6) float64 on the host, one row per generation: the searcher's HISTORY_COLUMNS."""
        return self._history[:self.iter].cpu()

    def _agent(self, row: torch.Tensor, template=None):
        if template is None and hasattr(self._pop, 'agent_from_row'):       # a BatchedPhysarumPopulation: a PhysarumAgent
            return self._pop.agent_from_row(row)
        template = template if template is not None else (self._pop.template if self._pop is not None else None)
        if template is None:
            raise RuntimeError('no NeuralAutomataAgent template: bind a population (for_population) or pass one')
        return BatchedNeuralAutomataAgent.unpack(template, row.cpu())

    def best_agent(self, template=None):
        """The best candidate evaluated so far, as a stand-alone agent of the population's kind (ready for save())."""
        return self._agent(self._best, template)

    def pop_best_agent(self, template=None):
        return self._agent(self._pop_best, template)

    def center_agent(self, template=None):
        return self._agent(self.center, template)


class PGPE(_PopulationSearch):
    """Policy-gradients with parameter-based exploration (Sehnke et al. 2010) with symmetric sampling and centred ranks, the
    arguments of evotorch's PGPE.  `popsize` is R (even, 2..64); the searcher maximises."""
    _update = 'die_pgpe_update'

    def __init__(self, popsize: int, num_params: Optional[int] = None, *, center_init=None,
                 initial_bounds: Tuple[float, float] = (-0.5, 0.5), radius_init: Optional[float] = None,
                 stdev_init=None, center_learning_rate: float, stdev_learning_rate: float, optimizer: str = 'clipup',
                 optimizer_config: Optional[dict] = None, stdev_max_change: Optional[float] = 0.2,
                 stdev_min: Optional[float] = None, stdev_max: Optional[float] = None, seed: int = 0, device=None):
        R = int(popsize)
        if R % 2 or not 2 <= R <= 64:
            raise ValueError(f'popsize {R}: an even number in 2..64 (symmetric pairs of samples, one replica each)')
        if optimizer not in OPTIMIZERS:
            raise ValueError(f'optimizer {optimizer!r}: one of {sorted(OPTIMIZERS)}')
        self.device = _resolve_device(device)
        center = _initial_center(center_init, num_params, initial_bounds, seed)
        self.R, self.P, self.seed = R, int(center.numel()), int(seed)
        if self.P < 1:
            raise ValueError('at least one parameter')
        if (radius_init is None) == (stdev_init is None):
            raise ValueError('exactly one of radius_init and stdev_init')
        if radius_init is not None:
            if not radius_init > 0:
                raise ValueError(f'radius_init {radius_init}: must be positive')
            stdev = torch.full((self.P,), math.sqrt(float(radius_init) ** 2 / self.P), dtype=torch.float32)
        else:
            stdev = torch.as_tensor(stdev_init, dtype=torch.float32).detach().cpu().expand(self.P).clone()
            if not bool((stdev > 0).all()):
                raise ValueError('stdev_init: must be positive')
        cfg = dict(optimizer_config or {})
        opt = OPTIMIZERS[optimizer]
        if opt == _lib.DIE_PGPE_CLIPUP:
            max_speed = float(cfg.pop('max_speed', 2.0 * center_learning_rate))     # evotorch's ClipUp default
            momentum = float(cfg.pop('momentum', 0.9))
            beta1, beta2, eps = 0.9, 0.999, 1e-8
        else:
            beta1, beta2 = (float(b) for b in cfg.pop('betas', (0.9, 0.999)))
            eps = float(cfg.pop('eps', 1e-8))
            max_speed, momentum = 0.0, 0.0
        if cfg:
            raise ValueError(f'optimizer_config: unknown keys {sorted(cfg)} for {optimizer!r}')
        dev, P = self.device, self.P
        f32 = dict(dtype=torch.float32, device=dev)
        self.center = center.to(dev)
        self.stdev = stdev.to(dev)
        self._opt_a = torch.zeros(P, **f32)
        self._opt_b = torch.zeros(P, **f32) if opt == _lib.DIE_PGPE_ADAM else None
        self._pop_best = torch.zeros(P, **f32)
        self._best = torch.zeros(P, **f32)
        self.fitness = torch.zeros(R, dtype=torch.float64, device=dev)
        self._evals = torch.tensor([-math.inf, -math.inf], dtype=torch.float64, device=dev)
        self._history = torch.zeros((64, 6), dtype=torch.float64, device=dev)
        self._work = torch.zeros(_lib.pgpe_work_doubles(P), dtype=torch.float64, device=dev)
        self._s = _lib.Pgpe(R, opt, P, self.seed & 0xFFFFFFFFFFFFFFFF, float(center_learning_rate), float(stdev_learning_rate),
                            max_speed, momentum, beta1, beta2, eps, -1.0 if stdev_max_change is None else float(stdev_max_change),
                            -math.inf if stdev_min is None else float(stdev_min), math.inf if stdev_max is None else float(stdev_max),
                            _ptr(self.center), _ptr(self.stdev), _ptr(self._opt_a), None if self._opt_b is None else _ptr(self._opt_b),
                            _ptr(self._pop_best), _ptr(self._best), _ptr(self.fitness), _ptr(self._evals), _ptr(self._history),
                            self._history.shape[0], _ptr(self._work))
        self.iter = 0                                   # generations told so far
        self._asked = None
        self._pop = None
        self._episode_fitness = self._folded = None

    # ------------------------------------------------------------------ generic interface
    def ask(self, params: torch.Tensor) -> torch.Tensor:
        """Fill `params` (R, P) with this generation's symmetric samples: rows 2i, 2i + 1 = center ± stdev·z_i.  One launch."""
        self._check_params(params)
        _lib.check(_lib.lib.die_pgpe_sample(C.byref(self._s), _ptr(params), self.iter, stream_ptr(self.device)), 'die_pgpe_sample')
        self._asked = params
        return params

    def tell(self, terms: torch.Tensor, params: Optional[torch.Tensor] = None, *, episodes: int = 1) -> None:
        """Update from the evaluated rows (those of the last `ask` unless `params` is given): candidate r's fitness is the sum
        over t of terms[t, r] — a (T, R) float64 tensor, or the (T, R, 2) die_step_result tensor of `BatchedEnv.run` (word 0:
        the reward).  Three or four launches, no host read.

        `episodes=E`: terms of (T, R·E[, 2]), replica c·E + e candidate c's e-th world; candidate c's fitness is the mean of
        its E sums, added in episode order (float64) — one more launch; the sums stay in `episode_fitness`."""
        params = self._asked if params is None else params
        if params is None:
            raise RuntimeError('tell() before ask()')
        self._tell(params, terms, episodes)

    # ------------------------------------------------------------------ results (read on demand)
    @property
    def status(self) -> dict:
        h = self.history()
        ev = self._evals.cpu().tolist()
        return dict(center=self.center.cpu(), stdev=self.stdev.cpu(), pop_best=self._pop_best.cpu(), pop_best_eval=ev[0],
                    best=self._best.cpu(), best_eval=ev[1], mean_eval=float(h[-1, 0]) if len(h) else math.nan,
                    median_eval=float(h[-1, 3]) if len(h) else math.nan, iter=self.iter)


CMAES_HISTORY_COLUMNS = ('mean_eval', 'max_eval', 'min_eval', 'median_eval', 'sigma', 'mean_stdev')


def cmaes_constants(popsize: int, num_params: int, *, c_sigma_ratio: float = 1.0, damp_sigma_ratio: float = 1.0,
                    c_c_ratio: float = 1.0, c_1_ratio: float = 1.0, c_mu_ratio: float = 1.0, active: bool = True) -> dict:
    """The weights and constants of separable CMA-ES for lambda = popsize, d = num_params, as include/die_hip.h states them
    (float64, on the host): weights (lambda values, best rank first), mu, mu_eff, mu_eff_minus, c_sigma, d_sigma, c_c, c_1,
    c_mu, chi_d."""
    lam, d = int(popsize), float(num_params)
    mu = lam // 2
    wp = [math.log((lam + 1) / 2.0) - math.log(k) for k in range(1, lam + 1)]
    pos = wp[:mu]
    spos = math.fsum(pos)
    w = [v / spos for v in pos]
    mu_eff = 1.0 / math.fsum(v * v for v in w)
    neg = wp[mu:]
    sneg = math.fsum(neg)
    sneg2 = math.fsum(v * v for v in neg)
    mu_eff_minus = sneg * sneg / sneg2 if sneg2 > 0 else 0.0
    c_sigma = c_sigma_ratio * (mu_eff + 2.0) / (d + mu_eff + 5.0)
    d_sigma = damp_sigma_ratio * (1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (d + 1.0)) - 1.0) + c_sigma)
    sd = math.sqrt(d)
    c_c = c_c_ratio * (1.0 + 1.0 / d + mu_eff / d) / (sd + 1.0 / d + 2.0 * mu_eff / d)
    c_1 = c_1_ratio / (d + 2.0 * sd + mu_eff / d)
    c_mu = c_mu_ratio * min(1.0 - c_1, (0.25 + mu_eff + 1.0 / mu_eff - 2.0) / (d + 4.0 * sd + mu_eff / 2.0))
    chi_d = sd * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d))
    if active and sneg2 > 0:
        a_mu = 1.0 + c_1 / c_mu if c_mu > 0 else math.inf
        a_mueff = 1.0 + 2.0 * mu_eff_minus / (mu_eff + 2.0)
        a_posdef = (1.0 - c_1 - c_mu) / (d * c_mu) if c_mu > 0 else math.inf
        scale = min(a_mu, a_mueff, a_posdef) / math.fsum(abs(v) for v in neg)
        w += [v * scale for v in neg]
    else:
        w += [0.0] * len(neg)
    return dict(weights=w, mu=mu, mu_eff=mu_eff, mu_eff_minus=mu_eff_minus, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1,
                c_mu=c_mu, chi_d=chi_d)


class CMAES(_PopulationSearch):
    """Separable CMA-ES (Ros & Hansen 2008; the learning rates of Akimoto & Hansen) with active negative weights and
    cumulative step-size control, the arguments of evotorch's CMAES.  `popsize` is lambda = R (2..64, default
    4 + floor(3 ln P)); the searcher maximises.  The covariance is diagonal: separable=False (a P x P eigendecomposition per
    generation) is not here.  The state (m, C, p_sigma, p_c, sigma) is float64 on the device; `sigma`, `C`, `stdev`,
    `p_sigma` and `p_c` read it back on demand."""
    _update = 'die_cmaes_update'

    def __init__(self, popsize: Optional[int] = None, num_params: Optional[int] = None, *, stdev_init: float, center_init=None,
                 initial_bounds: Tuple[float, float] = (-0.5, 0.5), c_m: float = 1.0, c_sigma_ratio: float = 1.0,
                 damp_sigma_ratio: float = 1.0, c_c_ratio: float = 1.0, c_1_ratio: float = 1.0, c_mu_ratio: float = 1.0,
                 active: bool = True, csa_squared: bool = False, separable: bool = True, seed: int = 0, device=None):
        if not separable:
            raise NotImplementedError('separable=False: the full covariance needs a P x P eigendecomposition every generation; '
                                      'only separable CMA-ES (a diagonal covariance) is implemented')
        self.device = _resolve_device(device)
        P = torch.as_tensor(center_init).numel() if center_init is not None else num_params
        if P is None:
            raise ValueError('num_params, or a center_init to take it from')
        if int(P) < 1:
            raise ValueError('at least one parameter')
        R = 4 + int(math.floor(3.0 * math.log(int(P)))) if popsize is None else int(popsize)
        if not 2 <= R <= _lib.MAX_REPLICAS:
            raise ValueError(f'popsize {R}: in 2..{_lib.MAX_REPLICAS} (one replica each)')
        center = _initial_center(center_init, num_params, initial_bounds, seed)
        self.R, self.P, self.seed = R, int(center.numel()), int(seed)
        sigma0 = float(stdev_init)
        if not (sigma0 > 0 and math.isfinite(sigma0)):
            raise ValueError(f'stdev_init {stdev_init}: a positive, finite sigma')
        if not float(c_m) > 0:
            raise ValueError(f'c_m {c_m}: must be positive')
        k = cmaes_constants(R, self.P, c_sigma_ratio=float(c_sigma_ratio), damp_sigma_ratio=float(damp_sigma_ratio),
                            c_c_ratio=float(c_c_ratio), c_1_ratio=float(c_1_ratio), c_mu_ratio=float(c_mu_ratio),
                            active=bool(active))
        if not (0 < k['c_sigma'] <= 1 and k['d_sigma'] > 0 and 0 < k['c_c'] <= 1 and k['c_1'] >= 0 and k['c_mu'] >= 0
                and k['c_1'] + k['c_mu'] <= 1):
            raise ValueError(f'the ratios give c_sigma {k["c_sigma"]:g}, d_sigma {k["d_sigma"]:g}, c_c {k["c_c"]:g}, '
                             f'c_1 {k["c_1"]:g}, c_mu {k["c_mu"]:g}: need c_sigma, c_c in (0, 1], d_sigma > 0, c_1 + c_mu <= 1')
        self.constants = k
        dev, P = self.device, self.P
        f64 = dict(dtype=torch.float64, device=dev)
        self.center = center.to(torch.float64).to(dev)
        self._C = torch.ones(P, **f64)
        self._p_sigma = torch.zeros(P, **f64)
        self._p_c = torch.zeros(P, **f64)
        self._sigma = torch.full((2,), sigma0, **f64)
        self._pop_best = torch.zeros(P, dtype=torch.float32, device=dev)
        self._best = torch.zeros(P, dtype=torch.float32, device=dev)
        self.fitness = torch.zeros(R, **f64)
        self._evals = torch.tensor([-math.inf, -math.inf], **f64)
        self._history = torch.zeros((64, 6), **f64)
        self._work = torch.zeros(_lib.cmaes_work_doubles(R, P), **f64)
        weights = (C.c_double * _lib.MAX_REPLICAS)(*k['weights'])
        self._s = _lib.Cmaes(R, int(bool(csa_squared)), P, self.seed & 0xFFFFFFFFFFFFFFFF, float(c_m), k['c_sigma'], k['d_sigma'],
                             k['c_c'], k['c_1'], k['c_mu'], k['mu_eff'], k['chi_d'], weights, _ptr(self.center), _ptr(self._C),
                             _ptr(self._p_sigma), _ptr(self._p_c), _ptr(self._sigma), _ptr(self._pop_best), _ptr(self._best),
                             _ptr(self.fitness), _ptr(self._evals), _ptr(self._history), self._history.shape[0], _ptr(self._work))
        self.iter = 0                                   # generations told so far
        self._asked = None
        self._asked_iter = None
        self._pop = None
        self._episode_fitness = self._folded = None

    # ------------------------------------------------------------------ generic interface
    def ask(self, params: torch.Tensor) -> torch.Tensor:
        """Fill `params` (R, P) with this generation's samples: row i = m + sigma·sqrt(C)·z_i.  One launch."""
        self._check_params(params)
        _lib.check(_lib.lib.die_cmaes_sample(C.byref(self._s), _ptr(params), self.iter, stream_ptr(self.device)), 'die_cmaes_sample')
        self._asked, self._asked_iter = params, self.iter
        return params

    def tell(self, terms: torch.Tensor, *, episodes: int = 1) -> None:
        """Update from the rows of this generation's `ask` (z is regenerated from its Philox counter, so the ask must be of the
        same generation): candidate r's fitness is the sum over t of terms[t, r] — a (T, R) float64 tensor, or the (T, R, 2)
        die_step_result tensor of `BatchedEnv.run` (word 0: the reward).  Four launches, no host read.

        `episodes=E`: terms of (T, R·E[, 2]), replica c·E + e candidate c's e-th world; candidate c's fitness is the mean of
        its E sums, added in episode order (float64) — one more launch; the sums stay in `episode_fitness`."""
        if self._asked is None or self._asked_iter != self.iter:
            raise RuntimeError(f'tell() before ask() of generation {self.iter}')
        self._tell(self._asked, terms, episodes)

    # ------------------------------------------------------------------ results (read on demand)
    @property
    def sigma(self) -> float:
        """The step size of the next generation."""
        return float(self._sigma[self.iter & 1].cpu())

    @property
    def C(self) -> torch.Tensor:
        """The diagonal covariance (P,) float64 on the host."""
        return self._C.cpu()

    @property
    def stdev(self) -> torch.Tensor:
        """sigma·sqrt(C): the per-parameter standard deviation of the next generation's samples."""
        return self.sigma * self._C.cpu().sqrt()

    @property
    def p_sigma(self) -> torch.Tensor:
        return self._p_sigma.cpu()

    @property
    def p_c(self) -> torch.Tensor:
        return self._p_c.cpu()

    @property
    def status(self) -> dict:
        h = self.history()
        ev = self._evals.cpu().tolist()
        return dict(center=self.center.cpu(), sigma=self.sigma, stdev=self.stdev, pop_best=self._pop_best.cpu(),
                    pop_best_eval=ev[0], best=self._best.cpu(), best_eval=ev[1],
                    mean_eval=float(h[-1, 0]) if len(h) else math.nan, median_eval=float(h[-1, 3]) if len(h) else math.nan,
                    iter=self.iter)
