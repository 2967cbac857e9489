"""Batched env replicas (BASELINE configs[4]): R worlds of one shape stepped by ONE launch pair per step
(`die_forward_env_step_batch`).  No reference counterpart — the reference steps one `Env` per Python call; a small grid
costs more in launches and host calls than in kernel time, and R replicas share those.

Replica r is exactly the stand-alone `Env(field_size, dynamics, seed=seed + r, max_agents='alive')` driven by
`PhysarumAgent(max_agents=K_r, seed=agent_seed + r, ...)`: same initial state, same Philox streams, same kernels'
arithmetic — bit for bit (tests/test_gpu_parity.py::test_batched_replicas_equal_stand_alone_runs).

`BatchedNeuralAutomataAgent` is a population of NeuralAutomataAgent candidates, one per replica (the evaluation half of
examples/learning_agents.py): replica r is `Env(field_size, dynamics, seed=seeds[r], max_agents='alive')` driven by a
NeuralAutomataAgent holding row r of the (R, P) parameter matrix — L + 2 launches per step for the whole population
(`die_nca_env_step_batch`), bit for bit the stand-alone runs (tests/test_gpu_nca_batch.py).

A device food-flow operator (`WaveSequence` / `PerlinNoiseSequence.get_flow_operator`) runs on every replica: replica r is then
the stand-alone run with a fresh operator over the same sequence whose counter starts where the batch's stood at the first
batched step — every replica sees the same t, and the batch's operator advances once per batched step.  One more launch
per step (`die_food_flow_batch`) in the small-world regime (tests/test_gpu_flow_batch.py).

`Dynamics(agents_die=True)` (compat='intended') runs on the replicas too: replica r is then the stand-alone Env of that
pressure, starved slots zeroed and `num_agents` falling.  One more launch per step in the small-world regime, the dead-slot +
lifecycle pass of every replica (tests/test_gpu_batch_lifecycle.py).

`max_agents=N` (an int, or None for W·H as the reference) gives every replica N slots — its K_r seeded agents first, then a
dead tail — so that every world fits one layout and `reset(seed=...)` can seed new worlds on the device (`die_init_batch`: five
launches for the whole batch, no host read).  Replica r is then `Env(field_size, dynamics, seed=seeds[r], max_agents=N)`, bit
for bit; the step runs its dead-slot pass (one more launch per step, as under agents_die) (tests/test_gpu_reseed.py).

`BatchedPhysarumPopulation` is a population of PhysarumAgent candidates whose six constructor arguments differ per replica
(a parameter sweep, or the candidates of a search): replica r is `Env(field_size, dynamics, seed=seeds[r])` driven by
`PhysarumAgent(max_agents=K_r, seed=seed + r, **row r)` — the same launch pair per step (`die_physarum_env_step_batch`), each
workgroup fetching its replica's row of a device table, bit for bit the stand-alone runs (tests/test_gpu_physarum_pop.py).

Episodes: both populations take `episodes=E` — C = R / E candidates, each evaluated on E worlds in the same launches.  Replica
r = c·E + e is candidate c on its e-th world (candidate-major), `parameters` stays ONE (C, P) matrix (the kernels read row r / E;
nothing is expanded), and `reset(seeds=[...])` / `episode_seeds` give the replicas their worlds (`die_init_batch_seeds`).  The
searchers fold the E sums of a candidate into its fitness (tests/test_gpu_episodes.py).

Agent dropout: `BatchedNeuralAutomataAgent(..., dropout_seed=S, dropout_seed_stride=K)` trains a template with
`p_agent_dropout > 0` — replica r's sense planes are multiplied by the counter-based mask of key S + r·K at the population's
`dropout_step`, inside the last conv launch (`die_nca_env_step_batch_dropout`); replica r is then the stand-alone run of
`NeuralAutomataAgent(dropout_seed=S + r·K)`, bit for bit (tests/test_gpu_dropout.py).

Per-replica Dynamics: `BatchedEnv(field_size, dynamics=[d_0 … d_{R-1}], replicas=R)` puts replica r under d_r — rate_feed,
rate_decay_chem, diffuse_sigma, food_infinite and whether the (one) food-flow operator reaches it may differ, everything else must
agree.  Replica r is then `Env(field_size, d_r, seed=seeds[r], max_agents=...)`, bit for bit: the kernels fetch replica r's row of a
device table built once at construction (`die_dynamics_rows`), the field sweep is launched once per gaussian radius present, and
the flow is applied under a replica mask (`die_food_flow_batch_masked`).  `episode_dynamics` lays E dynamics out for a population
with `episodes=E`: `episode_fitness[:, e]` of a searcher is then the score under dynamics e (tests/test_gpu_dynamics_rows.py).

`Dynamics(agents_born=True)`: after a step's deaths every replica's well-fed agents breed into its dead slots, in slot order
(`die_agent_births_batch`: three more launches per step whatever R, the step's last) — replica r is the stand-alone Env of that
rule at the same world step, `num_agents` rising where colonies grow (tests/test_gpu_births.py)."""
import ctypes as C
import dataclasses
import math
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch.nn.utils import parameters_to_vector, vector_to_parameters

from . import _lib
from .agent.evo import NeuralAutomataAgent, check_given
from .agent.gradient import join64, split64
from .data_init import DeviceFoodFlow, device_flow_kind, food_spec_from_seed
from .device_array import Q32, DeviceAction, _ptr, stream_ptr
from .env import BoundaryCondition, Dynamics, Env, _identity_food_flow, linear_action_cost
from .functional import _bare_medium


class BatchedEnv:
    """R replicas.  Two regimes, chosen by world size (`per_replica`):
      * small worlds (below Env.PIC_MIN_CELLS cells): ONE launch pair for the whole batch (die_forward_env_step_batch) — a
        small grid is bound by launches and host calls, which the replicas then share;
      * large worlds (BASELINE configs[4]: 16384² fp16): a replica fills the GPU by itself, and what counts is the step
        each replica takes — the tile-binned step (no claim plane, no re-sort), which the one-launch-pair form does not
        have.  Each replica is then a stand-alone `Env` stepped on its OWN HIP stream (the latency-bound agent kernel of one
        replica overlaps the bandwidth-bound field kernel of another); `step` fans out and joins the streams.
    Either way replica r is the stand-alone run of seeds[r] (default seed + r), bit for bit.  `seeds=[s] * R` starts every
    replica from the same world (how a population of candidates is compared).

    `max_agents`: 'alive' (default) gives replica r exactly its K_r seeded agents; an int N, or None for W·H, gives every
    replica N slots (alive first, then dead ones) — the layout `reset(seed=...)` needs, since a new world has a new K_r.

    `dynamics`: one `Dynamics` for every replica, or a sequence of R of them (replica r lives under dynamics[r]: domain
    randomisation, a robustness sweep).  In a sequence rate_feed, rate_decay_chem, diffuse_sigma and food_infinite may differ;
    op_food_flow is, per entry, the identity or ONE device operator object (it advances once per batched step and reaches the
    replicas that name it); boundary, op_action_cost, strict_cost, agents_die, compat and init_agent_ratio must agree.
    `replica_dynamics(r)` returns replica r's; `dynamics` keeps the shared fields (those of dynamics[0], with the operator).
    A single `Dynamics` takes the launches it always took."""

    # the R stock planes of a population that senses its agents' stocks (NeuralAutomataAgent(with_stock_channel=True); small
    # worlds): lazy, and zeroed again whenever the preceding step did not build them (`_stock_planes`)
    _stock = None
    _serial = 0                                     # steps and resets of any kind so far
    _stock_serial = -1                              # `_serial` right after the last step that built the stock planes

    def __init__(self, field_size: Tuple[int, int], dynamics: Union[Dynamics, Sequence[Dynamics], None] = None, *, replicas: int, seed: int = 0,
                 field_dtype: torch.dtype = torch.float32, device=None, per_replica: Optional[bool] = None,
                 seeds: Optional[Sequence[int]] = None, max_agents: Union[str, int, None] = 'alive'):
        if not 1 <= replicas <= 64:
            raise ValueError('1..64 replicas')
        if seeds is not None and len(seeds) != replicas:
            raise ValueError(f'{len(seeds)} seeds for {replicas} replicas')
        self._dyn = None                            # a sequence was given: replica r's Dynamics
        self._flow_mask = None                      # … and the replicas its flow operator reaches (bit r)
        if dynamics is not None and not isinstance(dynamics, Dynamics):
            self.dynamics, self._dyn, self._flow_mask = _shared_dynamics(dynamics, replicas)
        else:
            self.dynamics = dynamics or Dynamics()
        d = self.dynamics
        if d.agents_die and d.compat != 'intended':
            raise NotImplementedError(f"batched replicas: agents_die with compat={d.compat!r} (the host-driven frozen-indexer "
                                      "sequence of Env); only compat='intended' is batched")
        if d.agents_born:
            Env._check_births(d)
            if d.compat != 'intended':
                raise NotImplementedError(f"batched replicas: agents_born with compat={d.compat!r}; only compat='intended' has births")
        if d.apply_sense_mask:
            raise NotImplementedError('batched replicas: apply_sense_mask is not batched')
        if d.diffuse_mode != 'wrap' or not isinstance(d.boundary, BoundaryCondition):
            raise NotImplementedError(f"batched replicas: diffuse_mode={d.diffuse_mode!r}, boundary={d.boundary!r}: only 'wrap' "
                                      'diffusion and a BoundaryCondition are batched')
        if isinstance(max_agents, str):
            if max_agents != 'alive':
                raise ValueError(f"max_agents={max_agents!r}: 'alive', a number of slots or None (W·H)")
            self._fixed = None
        elif max_agents is None:
            self._fixed = int(field_size[0]) * int(field_size[1])
        else:
            if not _is_integer(max_agents, 1):
                raise ValueError(f'max_agents={max_agents!r}: at least one slot per replica')
            self._fixed = int(max_agents)
        slots = 'alive' if self._fixed is None else self._fixed
        self.R, self.seed = int(replicas), int(seed)
        self.seeds = [self.seed + r for r in range(self.R)] if seeds is None else [int(q) for q in seeds]
        self.W, self.H = int(field_size[0]), int(field_size[1])
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.dtype = field_dtype
        self.per_replica = (self.W * self.H >= Env.PIC_MIN_CELLS) if per_replica is None else bool(per_replica)
        self.chem_node = None                       # the chem planes' autograd handle (differentiable_chem / differentiable_step)
        if self.per_replica:
            # every replica Env gets its own Dynamics: its flow operator is its own (step keeps the counters in line)
            self.envs = [Env(field_size, dataclasses.replace(self.replica_dynamics(r)), seed=self.seeds[r], max_agents=slots,
                             field_dtype=field_dtype, device=self.device, sync=False) for r in range(self.R)]
            self.n = [e.agents.N for e in self.envs]
            self.Nmax = max(self.n)
            self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.R)]
            self._obs = [e._get_current_obs for e in self.envs]
            self._steps = 0
            self._initial = [_env_snapshot(e) for e in self.envs]
            self._flow_k0 = getattr(self.dynamics.op_food_flow, '_k', None)
            return
        # every replica starts as the stand-alone Env with seeds[r] would; its state is copied into slice r
        envs = [Env(field_size, d, seed=self.seeds[r], max_agents=slots, field_dtype=field_dtype, device=self.device, sort_every=0,
                    pic=False) for r in range(self.R)]
        self.n = [e.agents.N for e in envs]
        for r, e in enumerate(envs):
            # (only a world seeded with no agent at all: 'alive' keeps one dead placeholder slot; e._num_seeded, not e._all_alive,
            # which agents_born makes False by rule)
            if self._fixed is None and e._num_seeded < e.agents.N:
                raise NotImplementedError(f'batched replicas: replica {r} (seed {self.seeds[r]}) has no alive agent; dead slots are '
                                          'not modelled by the batched step')
        self.Nmax = max(self.n)
        R, W, H, Nm, dev = self.R, self.W, self.H, self.Nmax, self.device
        # the whole state of the batch is views into ONE allocation: reset() restores it with a single copy
        views, total = [], 0
        for name, shape, dt in (('owner', (R, W, H), torch.int64), ('food', (R, W, H), field_dtype), ('chem', (R, W, H), field_dtype),
                                ('chem_next', (R, W, H), field_dtype), ('x', (R, Nm), torch.int32), ('y', (R, Nm), torch.int32),
                                ('alive', (R, Nm), torch.uint8), ('agent_food', (R, Nm), torch.float32)):
            nbytes = math.prod(shape) * torch.empty((), dtype=dt).element_size()
            views.append((name, shape, dt, total, nbytes))
            total += -(-nbytes // 256) * 256
        self._state = torch.zeros(total, dtype=torch.uint8, device=dev)
        for name, shape, dt, off, nbytes in views:
            setattr(self, name, self._state[off:off + nbytes].view(dt).view(shape))
        for r, e in enumerate(envs):
            self.owner[r].copy_(e.medium.owner); self.food[r].copy_(e.medium.food); self.chem[r].copy_(e.medium.chem)
            k = self.n[r]
            self.x[r, :k].copy_(e.agents.x); self.y[r, :k].copy_(e.agents.y)
            self.alive[r, :k].copy_(e.agents.alive); self.agent_food[r, :k].copy_(e.agents.agent_food)
        self.epoch = 1
        # dead slots (agents_die, the fixed layout): the claim pass stashes every dead slot's feed and action cost for the
        # lifecycle pass
        dead = d.agents_die or self._fixed is not None
        ws = _lib.lib.die_batch_lifecycle_workspace_bytes(R, Nm) if dead else _lib.lib.die_batch_workspace_bytes(R)
        self._births_ws = None
        if d.agents_born:                           # the birth pass's counts and rank lists, behind the step's workspace
            ws = -(-int(ws) // 256) * 256
            births = int(_lib.lib.die_births_workspace_bytes(R, Nm))
            self._ws = torch.zeros(ws + births, dtype=torch.uint8, device=dev)
            self._births_ws = self._ws[ws:]
        else:
            self._ws = torch.zeros(int(ws), dtype=torch.uint8, device=dev)
        if self._fixed is not None:                 # reset(seed=...): die_init_batch's scan workspace and (K_r, overflow) words
            self._init_ws = torch.zeros(int(_lib.lib.die_init_batch_workspace_bytes(W, H, R)), dtype=torch.uint8, device=dev)
            self._counts = torch.zeros((R, 2), dtype=torch.int64, device=dev)
        self._rows = self._rows_host = None
        if self._dyn is not None:                   # the table the kernels read: built once, not state (reset leaves it alone)
            self._rows_host = (_lib.DynamicsRow * R)()
            structs = (_lib.Dynamics * R)(*[self._dynamics_struct(q) for q in self._dyn])
            _lib.check(_lib.lib.die_dynamics_rows(structs, R, W, H, self._rows_host), 'die_dynamics_rows')
            self._rows = torch.frombuffer(bytearray(bytes(self._rows_host)), dtype=torch.uint8).to(dev)
        self._steps = 0
        self._births_pass = None                    # the world step of the birth pass whose lists the workspace holds (births_record)
        self._initial = (self._state.clone(), self.chem, self.chem_next)
        self._flow_k0 = getattr(self.dynamics.op_food_flow, '_k', None)

    def replica_dynamics(self, r: int) -> Dynamics:
        """The Dynamics replica r lives under: dynamics[r] of a sequence, else the one `dynamics`."""
        if not 0 <= r < self.R:
            raise IndexError(f'replica {r} of {self.R}')
        return self.dynamics if self._dyn is None else self._dyn[r]

    def reset(self, *, seed: Optional[int] = None, seed_stride: int = 1, seeds: Optional[Sequence[int]] = None) -> None:
        """Every replica back to the state it was constructed in: bit for bit a fresh BatchedEnv of the same arguments (and a
        flow operator whose counter stands where this one's stood then).  Device copies from a snapshot taken at construction,
        on the current stream (one copy in the small-world regime); nothing is rebuilt and nothing is read back (the device loop
        of die_amd.search.PGPE).

        `seed`: new worlds instead — replica r becomes the world of seed + r·seed_stride, bit for bit a fresh BatchedEnv of
        those seeds (same max_agents), and `seeds` says so.  Needs the fixed layout (`max_agents` an int or None).  Small worlds:
        one die_init_batch call on the current stream, no host read and no allocation; a world seeding more than N agents is
        clipped as Env's agents_from_medium clips it, and the next `check()` raises.  Large worlds (per_replica): `Env.reset`
        of every replica, which reads each count back (and raises at once on such a world).

        `seeds`: the same with the world of every replica given — any R integers, repeats allowed, no pattern (the E worlds
        of every candidate: `episode_seeds`).  Not together with `seed`.  Small worlds: one die_init_batch_seeds call, the same
        five launches, the list handed to the kernels by value."""
        listed = seeds is not None
        if listed and seed is not None:
            raise ValueError('reset: seed= (seed + r·seed_stride) or seeds= (a list of R seeds), not both')
        if (listed or seed is not None) and self._fixed is None:
            raise ValueError(f"reset({'seeds' if listed else 'seed'}=...) needs every replica to hold the same number of slots: build "
                             "the BatchedEnv with max_agents=N (or None for W·H) instead of 'alive'")
        if listed:
            seeds = list(seeds)
            if len(seeds) != self.R:
                raise ValueError(f'reset(seeds=...): {len(seeds)} seeds for {self.R} replicas')
            for q in seeds:
                if not _is_integer(q):
                    raise ValueError(f'reset(seeds=...): {q!r} is not an integer seed')
            seeds = [int(q) for q in seeds]
        elif seed is not None:
            if not _is_integer(seed_stride, 0):
                raise ValueError(f'seed_stride={seed_stride!r}: a non-negative integer')
            seed, seed_stride = int(seed), int(seed_stride)
            seeds = [seed + r * seed_stride for r in range(self.R)]
        if self._flow_k0 is not None:
            self.dynamics.op_food_flow._k = self._flow_k0
        self._steps = 0
        self._births_pass = None
        self._serial += 1                           # (the stock planes of an earlier step say nothing about the worlds to come)
        self.chem_node = None                       # the worlds start over: an autograd handle of the chem planes ends here
        if seeds is not None:
            self._reseed(seeds, seed, seed_stride)
            self.seeds = seeds
            return
        if self.per_replica:
            for e, snap in zip(self.envs, self._initial):
                _env_restore(e, snap)
            self._obs = [e._get_current_obs for e in self.envs]
            return
        self._state.copy_(self._initial[0])
        self.chem, self.chem_next = self._initial[1:]
        self.epoch = 1

    def _reseed(self, seeds: List[int], seed: Optional[int], seed_stride: int) -> None:
        """The worlds of `seeds`; `seed` is None when they came as a list (else seeds[r] = seed + r·seed_stride)."""
        self.chem_node = None
        if self.per_replica:
            for r, (e, q) in enumerate(zip(self.envs, seeds)):
                try:
                    e.reset(seed=q)
                except ValueError as err:
                    raise ValueError(f'replica {r} (seed {q}): {err}') from err
            self._obs = [e._get_current_obs for e in self.envs]
            return
        self.chem, self.chem_next = self._initial[1:]
        self.epoch = 1
        m, a, _, b = self._structs()
        # Env._init_data: the Perlin food of DataInitializer.init_medium (its spec holds no seed-drawn value the kernel reads)
        spec = food_spec_from_seed(seeds[0] if seed is None else seed, scale=0.5, perlin_octaves=8, threshold=1.0)
        mask = 0xFFFFFFFFFFFFFFFF
        if seed is None:                            # the list: read during the call, passed by value
            name, worlds = 'die_init_batch_seeds', ((C.c_uint64 * self.R)(*[q & mask for q in seeds]), self.R)
        else:
            name, worlds = 'die_init_batch', (seed & mask, seed_stride & mask)
        _lib.check(getattr(_lib.lib, name)(C.byref(m), C.byref(a), C.byref(b), float(self.dynamics.init_agent_ratio), *worlds,
                                           C.byref(spec), _ptr(self._counts), _ptr(self._init_ws), self._init_ws.numel(),
                                           stream_ptr(self.device)), name)

    # ------------------------------------------------------------------
    def _structs(self):
        fdt = _lib.DIE_F32 if self.dtype == torch.float32 else _lib.DIE_F16
        m = _lib.Medium(self.W, self.H, fdt, self.epoch, _ptr(self.owner), _ptr(self.food), _ptr(self.chem), _ptr(self.chem_next),
                        0, 0, 0, 0, 0, 0, 0, 0, None)
        a = _lib.Agents(self.Nmax, _ptr(self.x), _ptr(self.y), _ptr(self.alive), _ptr(self.agent_food), None)
        return m, a, self._dynamics_struct(self.dynamics), self._batch_struct()

    def _stock_planes(self) -> torch.Tensor:
        """The (R, W, H) uint64 stock planes a stock-channel population's step builds and reads (die_nca_env_step_batch_stock).
        Zeroed on allocation, and again unless the step just before this one built them: then every word they hold carries an
        earlier epoch of the current 1..31 cycle (the library clears them with the claim planes on the wrap).  After anything else
        — a plain population's step, `step_action`, a reset — a tag of an earlier build could read as occupied, so they start over."""
        if self._stock is None:
            self._stock = torch.zeros((self.R, self.W, self.H), dtype=torch.int64, device=self.device)
        elif self._stock_serial != self._serial:
            self._stock.zero_()
        return self._stock

    def _batch_struct(self) -> _lib.Batch:
        return _lib.Batch(self.R, 0, self.W * self.H, self.Nmax, 1, (C.c_int64 * 64)(*self.n))

    def _dynamics_struct(self, d: Dynamics) -> _lib.Dynamics:
        boundary = _lib.DIE_BOUNDARY_WRAP if d.boundary == BoundaryCondition.wrap else _lib.DIE_BOUNDARY_LIMIT
        cost = _lib.DIE_COST_LINEAR if d.op_action_cost is linear_action_cost else _lib.DIE_COST_ZERO
        return _lib.Dynamics(d.rate_feed, d.rate_decay_chem, d.diffuse_sigma, boundary, cost, 0.02, 0.01, int(d.food_infinite), int(d.agents_die),
                             int(self._fixed is not None), 0, 0)

    def _births(self, a: _lib.Agents, b: _lib.Batch, results: torch.Tensor) -> None:
        """`Dynamics(agents_born=True)`: the birth pass of every replica (die_agent_births_batch, three launches whatever R) as the
        step's last launches — replica r breeds as the stand-alone Env of seeds[r] does at this world step."""
        d = self.dynamics
        p = _lib.Births(float(d.born_threshold), _lib.DIE_BOUNDARY_WRAP if d.boundary == BoundaryCondition.wrap else _lib.DIE_BOUNDARY_LIMIT,
                        float(d.born_spread), self._steps & 0xFFFFFFFF, 0)
        seeds = (C.c_uint64 * self.R)(*[q & 0xFFFFFFFFFFFFFFFF for q in self.seeds])
        _lib.check(_lib.lib.die_agent_births_batch(C.byref(a), C.byref(b), C.byref(p), seeds, _ptr(results), _ptr(self._births_ws),
                                                   self._births_ws.numel(), stream_ptr(self.device)), 'die_agent_births_batch')
        self._births_pass = self._steps

    def births_record(self):
        """Who was born to whom in every replica's birth pass of the step that just ran: a `die_amd.functional.BirthsRecord` whose
        `parent_of` and `child_of` are (R, Nmax) int32 device tensors by slot id — row r the stand-alone `Env.births_record()` of
        replica r, the slots from n[r] on -1 — freshly allocated per call, with every replica's world seed and the world step.  One
        launch for all R (die_births_record_batch), only when asked.  Valid after a step that ran the pass (`step`, `step_action`)
        and until the next step or reset; otherwise ValueError.  Large worlds (`per_replica`) hold a stand-alone Env per replica:
        `envs[r].births_record()`."""
        from .functional import BirthsRecord
        if self.per_replica:
            raise NotImplementedError('births_record: large worlds (per_replica) are not batched — every replica is a stand-alone Env: '
                                      'use envs[r].births_record()')
        if not self.dynamics.agents_born:
            raise ValueError('births_record: these worlds have no births (Dynamics(agents_born=False))')
        if self._births_pass is None:
            raise ValueError('births_record: no birth pass yet (valid after a step, until the next step or reset)')
        out = torch.empty((2, self.R, self.Nmax), dtype=torch.int32, device=self.device)
        b = self._batch_struct()
        _lib.check(_lib.lib.die_births_record_batch(C.byref(b), _ptr(self._births_ws), self._births_ws.numel(), _ptr(out[0]), _ptr(out[1]),
                                                    stream_ptr(self.device)), 'die_births_record_batch')
        return BirthsRecord(out[0], out[1], self.seeds, self._births_pass, self.n)

    def check(self):
        """Synchronise; raise if a replica's tile-binned step reported a bookkeeping error since the last check (per-replica
        regime: every replica is an `Env` of its own; the one-launch-pair regime runs the classic kernels, which have no such word),
        or if a `reset(seed=...)` since the last check seeded more agents than a replica has slots (the flags are cleared)."""
        torch.cuda.synchronize(self.device)
        if self.per_replica:
            for e in self.envs:
                e.check()
        elif self._fixed is not None:
            over = [r for r, f in enumerate(self._counts[:, 1].tolist()) if f]
            if over:
                self._counts[:, 1].zero_()
                raise ValueError('reset(seed=...) seeded more agents than max_agents=' + str(self._fixed) + ' slots in ' +
                                 ', '.join(f'replica {r} (seed {self.seeds[r]})' for r in over) + ' — the agents were clipped; '
                                 '(a seed of an earlier reset since the last check() may be the one)')

    def step(self, agent: Union['BatchedPhysarumAgent', 'BatchedPhysarumPopulation', 'BatchedNeuralAutomataAgent'],
             results: Optional[torch.Tensor] = None, action: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step of every replica: `agent.forward` + `Env.step` fused, two launches for the whole batch (L + 2 for a
        BatchedNeuralAutomataAgent of L layers, L + 3 when it senses the agents' stocks: the build of the R stock planes this
        BatchedEnv owns, L + 5 when its agents carry memory channels: that build, the expand and the memory read-out, L + 4
        with signal channels: that build and the field's update, L + 6 with both; one more with dead slots, one more with a flow; for a BatchedPhysarumPopulation a
        decode launch first when `parameters` was written since the last one).  Returns the (R, 2) float64 tensor of
        die_step_result words (device; `read_results` decodes).

        `action`: an optional contiguous (3, R, Nmax) float32 device tensor the step writes the agents' actions into (rows dx, dy,
        deposit — the `act` argument of the library's batched steps): afterwards `action[:, r, :n[r]]` is what replica r's agent
        did, bit for bit the stand-alone agent's `forward(obs).data` — a teacher's target for `differentiable_action`.  The slots
        from n[r] on are left as they were.  The step itself does not change with it.  Small worlds only.

        One path for the three agent kinds.  What is particular to a kind it says itself: `_check_step(env)` (its refusals),
        `_replica_agent(r)` (replica r's stand-alone agent, large worlds), `_claim_epoch(env)` (the epoch its claims are made
        at), `_launch(...)` (its struct and its library entry point), `_stepped()` (its counters after a step), `_inherit(env)` (what
        its newborns receive after the births: nothing for the two Physarum kinds) and
        `_builds_stock_planes` (whether its step builds the env's stock planes).  A step that is refused leaves the batch as it was."""
        agent._check_step(self)                     # every refusal before anything is launched
        flow = self._flow_kind()
        act = None
        if action is not None:
            if self.per_replica:
                raise NotImplementedError('step(action=...): large worlds (per_replica) step a stand-alone Env per replica; read '
                                          'each agent\'s own action there')
            self._check_action(action, 'no grad', no_grad=True)
            act = _lib.Action(self.Nmax, action[0].data_ptr(), action[1].data_ptr(), action[2].data_ptr())
        if results is None:
            results = torch.empty((self.R, 2), dtype=torch.float64, device=self.device)
        if self.per_replica:
            self._step_per_replica(agent, flow, results)
            agent._stepped()
            return results
        epoch = self.epoch
        agent._claim_epoch(self)
        m, a, dyn, b = self._structs()
        rows = () if self._rows is None else (_ptr(self._rows), self._rows_host)    # per-replica Dynamics: each replica under its row
        try:
            agent._launch((C.byref(m), C.byref(a)), (None if act is None else C.byref(act), C.byref(dyn), C.byref(b), _ptr(results), _ptr(self._ws), self._ws.numel()),
                          rows, stream_ptr(self.device))
        except Exception:
            self.epoch = epoch                      # refused before any launch: nothing changed
            raise
        agent._calls += 1
        agent._stepped()
        results = self._launched(flow, m, a, b, results, agent._builds_stock_planes)
        agent._inherit(self)                        # (after the births: what the newborns receive from their parents)
        return results

    def _launched(self, flow: Optional[int], m, a, b, results: torch.Tensor, built_stock_planes: bool = False) -> torch.Tensor:
        """What follows the launches of `step` and of `step_action` alike: the births, the plane swap, the flow, the counters."""
        self._serial += 1
        if built_stock_planes:                      # (a population with memory builds them as its standing planes): the next may build on top
            self._stock_serial = self._serial
        if self.dynamics.agents_born:
            self._births(a, b, results)
        self.chem_node = None                       # the field changed: an autograd handle of the chem planes ends here
        self.chem, self.chem_next = self.chem_next, self.chem      # (differentiable_step sets this step's node afterwards)
        self._food_flow(flow, m, b)
        self._steps += 1
        return results

    def _advance_claim_epoch(self) -> None:
        """Claims at the next epoch; at the wrap the claim planes start over.  For every step whose sensing does not read the
        claim planes: the two Physarum kinds' (their `_claim_epoch`) and `step_action`'s."""
        self.epoch += 1
        if self.epoch > _lib.OWNER_EPOCH_MAX:
            self.owner.zero_()
            self.epoch = 1

    def _check_action(self, action, note: str, contiguous: bool = True, no_grad: bool = False) -> None:
        """The (3, R, Nmax) float32 action tensor of `step(action=...)`, `step_action` and `differentiable_step`, or the ValueError
        that says what it must be — `note`: what the caller adds in brackets; `no_grad`: the tensor the recording step writes into,
        which says only what it takes; the others also what they got."""
        want, tensor = (3, self.R, self.Nmax), isinstance(action, torch.Tensor)
        if (tensor and tuple(action.shape) == want and action.dtype == torch.float32 and action.device == self.device
                and (action.is_contiguous() or not contiguous) and not (no_grad and action.requires_grad)):
            return
        got = ''
        if not no_grad and not tensor:
            got = f', got {type(action).__name__}'
        elif not no_grad:
            got = f', got {(tuple(action.shape), action.dtype, str(action.device)) + ((action.stride(),) if contiguous else ())}'
        raise ValueError(f"action: a {'contiguous ' if contiguous else ''}{want} float32 tensor on {self.device} ({note}){got}")

    def step_action(self, action: torch.Tensor, results: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step of every replica with the caller's actions: `Env.step(action)` of R worlds, no agent forward (an own torch
        policy reading `medium_tensor()`, a replay of what `step(agent, action=buf)` recorded).  `action`: a contiguous
        (3, R, Nmax) float32 tensor on the env's device, rows dx, dy, deposit; replica r reads `action[:, r, :n[r]]`, the padding is
        never read; a tensor with a graph is read detached.  Replica r is bit for bit the stand-alone `Env.step` of those values
        (tests/test_gpu_batch_step_action.py).  Small worlds: one claim launch for the whole batch (`die_env_step_batch`, `_rows`
        under per-replica Dynamics), one more with dead slots, the sweep(s), one more with a flow.  Large worlds (per_replica): every
        replica's own `Env.step` on its stream.  Returns the (R, 2) result words as `step` does; a refused step leaves the batch as
        it was."""
        self._check_action(action, 'rows dx, dy, deposit; replica r reads [:, r, :n[r]]')      # every refusal before anything is launched
        flow = self._flow_kind()
        action = action.detach()
        if results is None:
            results = torch.empty((self.R, 2), dtype=torch.float64, device=self.device)
        if self.per_replica:
            self._step_per_replica(_ReplicaActions(action, self.n), flow, results)
            return results
        epoch = self.epoch
        self._advance_claim_epoch()
        m, a, dyn, b = self._structs()
        act = _lib.Action(self.Nmax, action[0].data_ptr(), action[1].data_ptr(), action[2].data_ptr())
        args = (C.byref(m), C.byref(a), C.byref(act), C.byref(dyn), C.byref(b), _ptr(results), _ptr(self._ws), self._ws.numel())
        if self._rows is None:
            name, rows = 'die_env_step_batch', ()
        else:
            name, rows = 'die_env_step_batch_rows', (_ptr(self._rows), self._rows_host)
        try:
            _lib.check(getattr(_lib.lib, name)(*args, *rows, stream_ptr(self.device)), name)
        except Exception:
            self.epoch = epoch                      # refused before any launch: nothing changed
            raise
        return self._launched(flow, m, a, b, results)

    # ------------------------------------------------------------------ the differentiable step (die_env_grad.hip, batched)
    def _check_differentiable(self, what: str) -> None:
        """What the batched chem adjoint covers; raises before anything is launched or changed (Env._check_differentiable: the
        constructor has already refused a sense mask, a diffuse_mode other than 'wrap' and compat='reference')."""
        if self.per_replica:
            raise NotImplementedError(f'{what}: large worlds (per_replica) are not batched — every replica is a stand-alone Env: use '
                                      f'envs[r].differentiable_step / envs[r].differentiable_chem, the stand-alone Env.differentiable_step')
        if self.dtype != torch.float32:
            raise NotImplementedError(f'{what}: fp32 fields only (this batch holds {self.dtype})')

    def differentiable_chem(self) -> torch.Tensor:
        """The chem node: an (R, W, H) fp32 tensor holding a copy of the current chem planes, kept as `chem_node`, the planes'
        autograd handle.  On the first call, or after anything but `differentiable_step` changed the worlds, a leaf with
        requires_grad=False; after a `differentiable_step` that step's output, whose backward reaches the actions and the nodes of
        the steps before it.  `step`, `step_action`, `run` and `reset` (all forms) drop it, which cuts the graph there."""
        self._check_differentiable('differentiable_chem')
        if self.chem_node is None:
            self.chem_node = self.chem.clone()
        return self.chem_node

    def differentiable_step(self, action: torch.Tensor, results: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`step_action` with a graph through the chem planes: `Env.differentiable_step` with an R in front.  `action`: the
        (3, R, Nmax) fp32 tensor of `BatchedNeuralAutomataAgent.differentiable_action()` (or any fp32 tensor of that shape, with or
        without a graph).  The worlds are stepped by `step_action(action.detach())` — state and result words bit for bit its — and
        `chem_node` becomes this step's output,
            chem'_r = (1 − decay_r) · G_r(chem_r + D_r),   D_r[cell] = deposit of the slot of replica r that won the cell,
        differentiated with respect to the previous node (if it is still current) and the action's deposit row
        (die_env_step_backward_batch: the sweep(s) on the gradient planes and one gather, R worlds per launch).  dx and dy get
        zero gradient, as do the padding slots.  The agent is never called here: a replay through `step(agent, action=...)` would
        advance its dropout counter a second time.  Who deposited where (die_deposit_cells_batch) and the diffusion constants —
        sigma and decay, or the per-replica Dynamics table — are kept by the graph, so `backward` may run after further steps or a
        reset.  agents_die, the fixed slot layout, a food flow, per-replica Dynamics and episodes are all taken; fp16 fields and
        large worlds raise NotImplementedError, a wrong action ValueError, before anything is launched or changed."""
        self._check_differentiable('differentiable_step')
        if self.dynamics.agents_born:
            raise NotImplementedError('differentiable_step: agents_born is not supported (a newborn has no action to differentiate)')
        self._check_action(action, 'BatchedNeuralAutomataAgent.differentiable_action', contiguous=False)
        prev = self.chem_node
        results = self.step_action(action.detach().contiguous(), results)
        cells = torch.empty((self.R, self.Nmax), dtype=torch.int32, device=self.device)
        m, a, _, b = self._structs()
        _lib.check(_lib.lib.die_deposit_cells_batch(C.byref(m), C.byref(a), C.byref(b), _ptr(cells), stream_ptr(self.device)),
                   'die_deposit_cells_batch')
        self.chem_node = _BatchedFieldStep.apply(prev, action, cells, self.chem, self)
        return results

    def medium_tensor(self) -> torch.Tensor:
        """The observation of every replica: (R, 3, W, H) float32 on the device, channels agents / food / chem — `replica_numpy(r)[0]`
        for every r without leaving the device (the agents channel is 1 where the claim word carries the current epoch).  What an
        external torch policy reads before `step_action`.  Torch ops only; small worlds."""
        if self.per_replica:
            raise NotImplementedError('medium_tensor: large worlds (per_replica) hold a stand-alone Env per replica; read '
                                      'envs[r].medium there')
        occ = ((self.owner >> (32 + _lib.OWNER_EPOCH_SHIFT)) & _lib.OWNER_EPOCH_MAX) == self.epoch
        return torch.stack([occ.to(torch.float32), self.food.to(torch.float32), self.chem.to(torch.float32)], dim=1)

    def _flow_kind(self) -> Optional[int]:
        """The batched flow of `dynamics.op_food_flow` (DIE_FLOW_WAVE / DIE_FLOW_PERLIN; None for the identity).  Any other
        operator is refused: a host operator would cost a round trip per replica and step."""
        op = self.dynamics.op_food_flow
        if op is _identity_food_flow:
            return None
        kind = device_flow_kind(op)
        if kind is None:
            raise NotImplementedError(f'batched replicas: food-flow operator {op!r} is not batched — only the device operators of '
                                      'WaveSequence / PerlinNoiseSequence (get_flow_operator) are; step the replicas one at a time')
        return kind

    def _food_flow(self, flow: Optional[int], m: _lib.Medium, b: _lib.Batch):
        """Env._food_flow of every replica: one launch, after the step (the next sensing reads the flowed food)."""
        if flow is None:
            return
        op = self.dynamics.op_food_flow
        seq = op.seq
        octaves, seed = (seq._octaves, seq._seed & 0xFFFFFFFFFFFFFFFF) if flow == _lib.DIE_FLOW_PERLIN else (0, 0)
        if self._flow_mask is None:
            _lib.check(_lib.lib.die_food_flow_batch(C.byref(m), C.byref(b), flow, op.next_t(), op.scale, op.decay, octaves, seed,
                                                    stream_ptr(self.device)), 'die_food_flow_batch')
        else:                                       # per-replica Dynamics: the replicas that name the operator
            _lib.check(_lib.lib.die_food_flow_batch_masked(C.byref(m), C.byref(b), flow, op.next_t(), op.scale, op.decay, octaves, seed,
                                                           self._flow_mask, stream_ptr(self.device)), 'die_food_flow_batch_masked')

    def _step_per_replica(self, agent, flow: Optional[int], results: torch.Tensor) -> None:
        """Large worlds: replica r is its own Env stepped by `agent._replica_agent(r)` on its own stream.  With a flow, each Env gets
        an operator of its own over the batch's sequence, at the batch's counter: all apply the same t, each on its stream."""
        op = self.dynamics.op_food_flow
        for r, e in enumerate(self.envs):
            if flow is not None and self._flow_mask is not None and not (self._flow_mask >> r) & 1:
                continue                            # per-replica Dynamics: this replica's food does not flow (it keeps the identity)
            e.dynamics.op_food_flow = op if flow is None else DeviceFoodFlow(op.seq, op.scale, op.decay)
            if flow is not None:
                e.dynamics.op_food_flow._k = op._k
        cur = torch.cuda.current_stream(self.device)
        start = cur.record_event()
        for r, (e, st) in enumerate(zip(self.envs, self.streams)):
            st.wait_event(start)
            with torch.cuda.stream(st):
                self._obs[r], res, *_ = e.step(agent._replica_agent(r).forward(self._obs[r]))
                results[r].copy_(res)
            cur.wait_stream(st)
        if flow is not None:
            op.next_t()
        agent._calls += 1
        self._steps += 1

    def run(self, agent: Union['BatchedPhysarumAgent', 'BatchedPhysarumPopulation', 'BatchedNeuralAutomataAgent'], n_steps: int) -> torch.Tensor:
        out = torch.empty((n_steps, self.R, 2), dtype=torch.float64, device=self.device)
        for i in range(n_steps):
            self.step(agent, out[i])
        return out

    @staticmethod
    def read_results(results: torch.Tensor):
        host = results.cpu()
        return host[..., 0].numpy().copy(), host[..., 1].contiguous().view(torch.int64).numpy().copy()

    def replica_numpy(self, r: int):
        """(medium (3, W, H), agents (4, K_r)) of replica r, float64 like `Env.medium.to_numpy()` / `Env.agents.to_numpy()`."""
        if self.per_replica:
            torch.cuda.synchronize(self.device)
            return self.envs[r].medium.to_numpy(), self.envs[r].agents.to_numpy()
        occ = (((self.owner[r] >> (32 + _lib.OWNER_EPOCH_SHIFT)) & _lib.OWNER_EPOCH_MAX) == self.epoch).to(torch.float64)
        medium = np.stack([occ.cpu().numpy(), self.food[r].to(torch.float64).cpu().numpy(), self.chem[r].to(torch.float64).cpu().numpy()])
        k = self.n[r]
        q = lambda t: ((t[r, :k].to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / Q32).cpu().numpy()
        agents = np.stack([q(self.x), q(self.y), self.alive[r, :k].to(torch.float64).cpu().numpy(),
                           self.agent_food[r, :k].to(torch.float64).cpu().numpy()])
        return medium, agents


class _ReplicaActions:
    """`BatchedEnv.step_action` on large worlds: what `_step_per_replica` asks of an agent, answered from a (3, R, Nmax) action
    tensor — replica r's 'agent' hands its Env `action[:, r, :n[r]]` as a DeviceAction in slot order."""

    def __init__(self, action: torch.Tensor, n: Sequence[int]):
        self._action, self._n, self._calls = action, n, 0

    def _replica_agent(self, r: int) -> '_ReplicaActions':
        self._r = r
        return self

    def forward(self, obs) -> DeviceAction:
        k = self._n[self._r]
        act = DeviceAction(k, self._action.device)
        act.data = self._action[:, self._r, :k].contiguous()
        return act


def episode_seeds(seed: int, candidates: int, episodes: int, candidate_stride: int = 0) -> List[int]:
    """The R = candidates·episodes seeds of `BatchedEnv.reset(seeds=...)` in candidate-major order: replica c·E + e gets
    seed + e + candidate_stride·c·E.  Stride 0: every candidate sees the same E worlds; stride 1: every replica its own."""
    for name, v, low in (('candidates', candidates, 1), ('episodes', episodes, 1), ('candidate_stride', candidate_stride, 0)):
        if not _is_integer(v, low):
            raise ValueError(f'{name}={v!r}: an integer >= {low}')
    seed, C_, E, stride = int(seed), int(candidates), int(episodes), int(candidate_stride)
    return [seed + e + stride * c * E for c in range(C_) for e in range(E)]


def episode_dynamics(dynamics: Sequence[Dynamics], candidates: int) -> List[Dynamics]:
    """The R = candidates·E dynamics of `BatchedEnv(dynamics=...)` for a population with `episodes=E = len(dynamics)`, in
    candidate-major order: replica c·E + e gets dynamics[e] — every candidate is scored under every listed dynamics, and a
    searcher's `episode_fitness[:, e]` is the score under dynamics[e].  The twin of `episode_seeds`."""
    dynamics = list(dynamics)
    if not dynamics or not all(isinstance(q, Dynamics) for q in dynamics):
        raise ValueError('dynamics: a non-empty sequence of Dynamics')
    if not _is_integer(candidates, 1):
        raise ValueError(f'candidates={candidates!r}: an integer >= 1')
    return [dynamics[e] for _ in range(int(candidates)) for e in range(len(dynamics))]


_MUST_AGREE = ('boundary', 'op_action_cost', 'strict_cost', 'agents_die', 'agents_born', 'born_threshold', 'born_spread', 'compat',
               'init_agent_ratio', 'apply_sense_mask', 'diffuse_mode')


def _shared_dynamics(dynamics, replicas: int):
    """A sequence of per-replica Dynamics, checked: (the Dynamics of the shared fields, the list, the flow's replica mask)."""
    dyn = list(dynamics)
    if len(dyn) != replicas:
        raise ValueError(f'{len(dyn)} dynamics for {replicas} replicas')
    for r, q in enumerate(dyn):
        if not isinstance(q, Dynamics):
            raise TypeError(f'dynamics[{r}]: a Dynamics, not {type(q).__name__}')
    first, op, mask = dyn[0], None, 0
    for r, q in enumerate(dyn):
        for name in _MUST_AGREE:
            u, v = getattr(q, name), getattr(first, name)
            if (u is not v) if callable(u) or callable(v) else (u != v):
                raise ValueError(f'replica {r}: dynamics[{r}].{name}={u!r} differs from dynamics[0].{name}={v!r} — {name} must agree '
                                 'across the replicas of a batch (rate_feed, rate_decay_chem, diffuse_sigma, food_infinite and the '
                                 'food flow may differ)')
        if q.op_food_flow is not _identity_food_flow:
            if op is None:
                op = q.op_food_flow
            elif q.op_food_flow is not op:
                raise ValueError(f'replica {r}: dynamics[{r}].op_food_flow is a second food-flow operator — every entry takes the '
                                 'identity or the SAME operator object (it advances once per batched step)')
            mask |= 1 << r
    return dataclasses.replace(first, op_food_flow=_identity_food_flow if op is None else op), dyn, mask


def _is_integer(v, low: Optional[int] = None, exact: bool = False) -> bool:
    """An integer, not a bool, at least `low`.  `exact`: an `int` itself (2.0 and numpy's integers are refused); otherwise any
    value equal to its int()."""
    if isinstance(v, bool) or (not isinstance(v, int) if exact else int(v) != v):
        return False
    return low is None or int(v) >= low


def _worlds_per_candidate(episodes) -> int:
    """An `episodes` argument, checked (the populations here and the searchers of die_amd.search)."""
    if not _is_integer(episodes, 1, exact=True):
        raise ValueError(f'episodes={episodes!r}: an integer >= 1 (worlds per candidate)')
    return episodes


def _episodes(env, episodes) -> int:
    """`episodes` of a population on `env`, checked: R = candidates·episodes replicas."""
    _worlds_per_candidate(episodes)
    if env.R % episodes:
        raise ValueError(f'episodes={episodes}: the BatchedEnv holds {env.R} replicas, not a multiple of {episodes} — replica c·E + e is '
                         'candidate c on its e-th world')
    return episodes


def _env_snapshot(e: Env) -> dict:
    """Device copies of what a step of a stand-alone Env changes (its medium planes and agent arrays), and the host words
    that describe them."""
    M, A = e.medium, e.agents
    return dict(planes=(M.owner.clone(), M.food.clone(), M.chem.clone()), epoch=M.epoch, N=A.N,
                agents=(A.x.clone(), A.y.clone(), A.alive.clone(), A.agent_food.clone()),
                slot=None if A.slot is None else A.slot.clone(), all_alive=e._all_alive)


def _env_restore(e: Env, snap: dict) -> None:
    """The Env of `snap` again, as its constructor left it: planes copied back, agent arrays fresh copies (a re-sort or the
    tile-binned step may have swapped the arrays themselves), the tile-binned state dropped (a fresh Env builds it at its first
    step too), the step counter at 0.  No host read."""
    M, A = e.medium, e.agents
    e._agents_changed()
    for dst, src in zip((M.owner, M.food, M.chem), snap['planes']):
        dst.copy_(src)
    M.epoch, M.owner_stale = snap['epoch'], None
    A.x, A.y, A.alive, A.agent_food = (t.clone() for t in snap['agents'])
    A.slot = None if snap['slot'] is None else snap['slot'].clone()
    A.N = snap['N']
    e._all_alive = snap['all_alive']
    e._steps = 0
    e._births_pass, e._births_consumed = None, False
    e._pic = None
    e._frozen = None
    e._fuse_forward = True
    e._host_read_pending = False
    e._pic_status_written = False
    e._status_word = None
    e.last_result = None


class _PhysarumReplicas:
    """What BatchedPhysarumAgent and BatchedPhysarumPopulation share: a heading per agent slot of every replica (small worlds; a
    list `agents` of R stand-alone PhysarumAgents in large ones), and a step that senses and claims at one epoch."""

    def _alloc_headings(self) -> None:
        env = self.env
        self._hd_hi = torch.zeros((env.R, env.Nmax), dtype=torch.int32, device=env.device)
        self._hd_lo = torch.zeros_like(self._hd_hi)

    def direction_rads_numpy(self, r: int) -> np.ndarray:
        if self.env.per_replica:
            torch.cuda.synchronize(self.env.device)
            return self.agents[r].direction_rads_numpy()
        k = self.env.n[r]
        return join64(self._hd_hi[r, :k].contiguous(), self._hd_lo[r, :k].contiguous()).cpu().numpy()

    # ------------------------------------------------------------------ BatchedEnv.step
    def _check_step(self, env: BatchedEnv) -> None:
        pass

    def _replica_agent(self, r: int):
        return self.agents[r]

    _claim_epoch = staticmethod(BatchedEnv._advance_claim_epoch)      # `_claim_epoch(env)`: senses and claims at one epoch, the next
    _builds_stock_planes = False                    # (a step of this kind leaves the env's stock planes alone)

    def _stepped(self) -> None:
        pass

    def _inherit(self, env: BatchedEnv) -> None:
        pass                                        # (headings are not heritable: a newborn takes its slot's)


class _Population:
    """What the two populations share: `parameters`, ONE (candidates, P) float32 device matrix, one row per candidate."""

    def _matrix(self, rows, what: str, columns) -> torch.Tensor:
        """`rows` as a tensor of one row per candidate, or the refusal (`what` names the argument, `columns` its P columns)."""
        t = torch.as_tensor(rows).detach()
        if tuple(t.shape) != (self.candidates, self.P):
            rows_are = 'R replicas' if self.episodes == 1 else f'{self.candidates} candidates of {self.episodes} episodes each'
            raise ValueError(f'{what} of shape {tuple(t.shape)}: ({self.candidates}, {self.P}) expected ({rows_are} x {columns})')
        return t

    def _check_parameters(self, p: Optional[torch.Tensor] = None) -> None:
        p = self.parameters if p is None else p
        if not isinstance(p, torch.Tensor):
            raise ValueError(f'parameters: a ({self.candidates}, {self.P}) float32 tensor on {self.env.device}')
        if tuple(p.shape) != (self.candidates, self.P) or p.dtype != torch.float32 or p.device != self.env.device or not p.is_contiguous():
            raise ValueError(f'parameters must stay a contiguous ({self.candidates}, {self.P}) float32 tensor on {self.env.device}')

    def _check_step(self, env: BatchedEnv) -> None:
        if env is not self.env:
            raise ValueError('this population was built for another BatchedEnv')
        self._check_parameters()


class BatchedPhysarumAgent(_PhysarumReplicas):
    """R PhysarumAgent objects as one: replica r's headings and Philox streams are those of
    `PhysarumAgent(max_agents=K_r, seed=seed + r, ...)` (core/agent/gradient.py:139-166)."""

    def __init__(self, env: BatchedEnv, scale: float = 0.005, deposit: float = 4.0, sense_offset: float = 0.03,
                 normalized_grad: bool = True, grad_clip: Optional[float] = 1e-5, turn_angle: int = 30, sense_angle: int = 90,
                 turn_tolerance: float = 0.1, seed: int = 0):
        self.env, self.seed = env, int(seed)
        self._calls = 0
        if env.per_replica:
            from .agent.gradient import PhysarumAgent
            self.agents = [PhysarumAgent(max_agents=env.n[r], scale=scale, deposit=deposit, sense_offset=sense_offset,
                                         normalized_grad=normalized_grad, grad_clip=grad_clip, turn_angle=turn_angle,
                                         sense_angle=sense_angle, turn_tolerance=turn_tolerance, seed=self.seed + r) for r in range(env.R)]
            return
        self._p = dict(scale=scale, deposit=deposit, sense_offset=sense_offset, normalized=normalized_grad,
                       grad_clip=-1.0 if grad_clip is None else grad_clip, turn=math.radians(turn_angle),
                       sense=math.radians(sense_angle), rtol=turn_tolerance)
        self._alloc_headings()
        for r in range(env.R):                      # the headings a stand-alone agent of that seed starts with
            k = env.n[r]
            _lib.check(_lib.lib.die_init_heading(_ptr(self._hd_hi[r]), _ptr(self._hd_lo[r]), None, None, k, self._p['turn'],
                                                 (self.seed + r) & 0xFFFFFFFFFFFFFFFF, stream_ptr(env.device)), 'die_init_heading')

    def _struct(self) -> _lib.GradientAgent:
        p = self._p
        return _lib.GradientAgent(_lib.DIE_AGENT_PHYSARUM, int(bool(p['normalized'])), p['scale'], p['deposit'], 0.0, p['sense_offset'], 0.0,
                                  p['grad_clip'], p['turn'], p['sense'], p['rtol'], _ptr(self._hd_hi), _ptr(self._hd_lo), None, None, None,
                                  self.seed & 0xFFFFFFFFFFFFFFFF, self._calls & 0xFFFFFFFF, 0, None)

    def _launch(self, front: tuple, back: tuple, rows: tuple, stream) -> None:
        """The library's step: (m, a), this agent's struct, (the action or None, d, b, results, workspace), the Dynamics rows, the stream."""
        name = 'die_forward_env_step_batch_rows' if rows else 'die_forward_env_step_batch'
        _lib.check(getattr(_lib.lib, name)(*front, C.byref(self._struct()), *back, *rows, stream), name)


PARAMETER_NAMES = ('scale', 'deposit', 'sense_offset', 'turn_angle', 'sense_angle', 'turn_tolerance')
PHYSARUM_DEFAULTS = (0.005, 4.0, 0.03, 30.0, 90.0, 0.1)            # PhysarumAgent's constructor defaults, in that order


def _check_physarum_values(v: np.ndarray, rows: Sequence) -> None:
    """What a PhysarumAgent accepts, on (n, 6) float32 values; `rows` names each row in the error."""
    checks = ((0, lambda c: c >= 0, '>= 0'), (2, lambda c: c >= 0, '>= 0'), (3, lambda c: (c > 0) & (c <= 180), 'in (0, 180]'),
              (4, lambda c: (c >= 0) & (c <= 180), 'in [0, 180]'), (5, lambda c: c >= 0, '>= 0'))
    if not np.all(np.isfinite(v)):
        r, j = (int(i[0]) for i in np.nonzero(~np.isfinite(v)))
        raise ValueError(f'row {rows[r]}, column {PARAMETER_NAMES[j]}: {v[r, j]} is not finite')
    for j, ok, what in checks:
        bad = np.nonzero(~ok(v[:, j]))[0]
        if len(bad):
            raise ValueError(f'row {rows[int(bad[0])]}, column {PARAMETER_NAMES[j]}: {v[bad[0], j]} must be {what}')


class ParameterSpace:
    """The box a unit-mode BatchedPhysarumPopulation is searched in: value j = lo[j] + (hi[j] - lo[j])·clamp(u[j], 0, 1) in
    float32 (one product, one sum, each rounded), columns in PARAMETER_NAMES order.  The default brackets the reference's
    PhysarumAgent defaults (0.005, 4.0, 0.03, 30, 90, 0.1):
        lo = (0.001, 0.5, 0.005,  5,  10, 0.0)
        hi = (0.02,  8.0, 0.1,   90, 180, 0.5)
    Both ends of every decoded range must be values a PhysarumAgent accepts, so that every decoded row is."""
    DEFAULT_LO = (0.001, 0.5, 0.005, 5.0, 10.0, 0.0)
    DEFAULT_HI = (0.02, 8.0, 0.1, 90.0, 180.0, 0.5)

    def __init__(self, lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None):
        self.lo = np.array(self.DEFAULT_LO if lo is None else lo, dtype=np.float32).reshape(-1)
        self.hi = np.array(self.DEFAULT_HI if hi is None else hi, dtype=np.float32).reshape(-1)
        if self.lo.shape != (6,) or self.hi.shape != (6,):
            raise ValueError(f'lo and hi: 6 values each, in the order {PARAMETER_NAMES}')
        for j, name in enumerate(PARAMETER_NAMES):
            if not (np.isfinite(self.lo[j]) and np.isfinite(self.hi[j]) and self.lo[j] <= self.hi[j]):
                raise ValueError(f'column {name}: bounds ({self.lo[j]}, {self.hi[j]}) must be finite with lo <= hi')
        _check_physarum_values(np.stack([self.lo, self.decode(np.ones(6, dtype=np.float32))]), ('lo', 'hi'))

    def decode(self, u) -> np.ndarray:
        """Search coordinates (..., 6) -> values, float32, by the expressions of die_physarum_decode_batch."""
        u = np.asarray(u, dtype=np.float32)
        c = np.fmin(np.fmax(u, np.float32(0)), np.float32(1))        # (a NaN coordinate reads as 0)
        span = self.hi - self.lo
        t = span * c
        return (self.lo + t).astype(np.float32)

    def encode(self, values) -> np.ndarray:
        """Values -> search coordinates (float32; columns with lo == hi map to 0): where a search may start."""
        span = (self.hi - self.lo).astype(np.float64)
        v = np.asarray(values, dtype=np.float64)
        return np.where(span > 0, (v - self.lo) / np.where(span > 0, span, 1.0), 0.0).astype(np.float32)

    def _struct(self) -> _lib.ParameterSpace:
        return _lib.ParameterSpace((C.c_float * 6)(*self.lo.tolist()), (C.c_float * 6)(*self.hi.tolist()))


class BatchedPhysarumPopulation(_Population, _PhysarumReplicas):
    """R PhysarumAgent candidates whose scale, deposit, sense_offset, turn_angle, sense_angle and turn_tolerance differ per
    replica; candidate r steps replica r of a BatchedEnv exactly as `candidate(r)` steps the stand-alone Env of seeds[r].
    normalized_grad and grad_clip are shared (they choose the kernel), as a NeuralAutomataAgent population shares its
    architecture.

    `episodes=E`: C = R / E candidates (`candidates`), candidate c stepping the E replicas c·E … c·E + E − 1, each the
    stand-alone Env of seeds[c·E + e] driven by `PhysarumAgent(max_agents=K_r, seed=seed + r, **row c)` — the headings stay per
    replica.  `parameters`, `set_values`, `set_parameters` and `values()` are then (C, 6); `table()` keeps R rows (row r = row
    r // E of the decode, written by the one decode launch).  Read "(R, 6)" below as "(C, 6)".

    `parameters` is ONE (R, 6) float32 device tensor, columns in PARAMETER_NAMES order:
      * natural mode (`values=`, default: every row the reference's defaults): a row holds the constructor arguments
        themselves (angles in degrees).  Checked on the host here and in `set_values`;
      * unit mode (`parameters=`, `space=` a ParameterSpace, default ParameterSpace()): a row holds search coordinates, decoded
        on the device as lo + (hi - lo)·clamp(u, 0, 1) — valid whatever a searcher writes.  What PGPE / CMAES bind to.
    One launch (`die_physarum_decode_batch`) turns the rows into the table the step kernel reads.  It runs at construction,
    in `reset()`, in `decode()`, and before a step when torch has counted an in-place write to `parameters` since — so
    in-place torch writes are seen by the next step.  Two things to know: a write torch does not count (a kernel writing through
    the raw pointer, such as a searcher's `ask(pop.parameters)` called by hand) is NOT seen until `decode()` or `reset()` — the
    searchers' own generation calls `reset()`; and an in-place write to NATURAL rows is decoded unchecked (only the constructor
    and `set_values` check on the host: a turn_angle of 0 or a NaN written in place reaches the kernels as it is) — use
    `set_values`, or unit mode, where the device clamp keeps every row valid.

    "Bit for bit the stand-alone run" has one caveat: the two cosines of a row (c_turn, c_sense) come from the device's float64
    cos here and from the host's libm for a stand-alone agent; both are rounded to float32, so they differ only where the
    libraries' last-bit difference straddles a float32 rounding boundary (about 1 row in 10^8; `table()` shows the values).

    Small worlds: nothing here reads the device back except `values()`, `table()`, `candidate()` and
    `direction_rads_numpy()`.  Large worlds (`env.per_replica`): R PhysarumAgent objects are built from `values()` at
    construction and at `reset()` — a host read each time, and the only moments a write to `parameters` is taken up."""
    PARAMETER_NAMES = PARAMETER_NAMES
    P = 6

    def __init__(self, env: BatchedEnv, values=None, *, parameters=None, space: Optional[ParameterSpace] = None,
                 normalized_grad: bool = True, grad_clip: Optional[float] = 1e-5, seed: int = 0, episodes: int = 1):
        self.episodes = _episodes(env, episodes)
        self.candidates = env.R // self.episodes
        if values is not None and parameters is not None:
            raise ValueError('values= (natural rows) or parameters= (unit rows with a space), not both')
        self.natural = parameters is None
        if self.natural and space is not None:
            raise ValueError('space= goes with parameters= (unit mode); natural rows hold the values themselves')
        if not self.natural and space is None:
            space = ParameterSpace()
        if space is not None and not isinstance(space, ParameterSpace):
            raise TypeError('space: a ParameterSpace')
        self.env, self.R, self.seed, self.space = env, env.R, int(seed), space
        self.normalized_grad, self.grad_clip = bool(normalized_grad), grad_clip
        dev = env.device
        self.parameters = torch.empty((self.candidates, self.P), dtype=torch.float32, device=dev)
        self._table = torch.zeros(self.R * C.sizeof(_lib.PhysarumRow), dtype=torch.uint8, device=dev)
        self._values = torch.zeros((self.candidates, self.P), dtype=torch.float32, device=dev)
        self._space_struct = None if space is None else space._struct()
        self._seen = None                           # (`parameters`' address, its torch version counter) at the last decode
        self._calls = 0
        if self.natural:
            rows = np.tile(np.float32(PHYSARUM_DEFAULTS), (self.candidates, 1)) if values is None else values
            self.parameters.copy_(self._natural_rows(rows))
        else:
            self.parameters.copy_(self._rows(parameters, 'parameters'))
        if not env.per_replica:
            self._alloc_headings()
        self.reset()

    # ------------------------------------------------------------------ parameters
    def _rows(self, rows, what: str) -> torch.Tensor:
        return self._matrix(rows, what, PARAMETER_NAMES).to(torch.float32)

    def _natural_rows(self, rows) -> torch.Tensor:
        t = self._rows(rows, 'values')
        _check_physarum_values(t.cpu().numpy(), range(self.candidates))
        return t

    def set_values(self, values) -> None:
        """Natural mode: copy an (R, 6) matrix of constructor arguments in (checked on the host first)."""
        if not self.natural:
            raise ValueError('set_values: this population holds unit rows (set_parameters); its values are decoded from them')
        self.parameters.copy_(self._natural_rows(values))
        self.decode()

    def set_parameters(self, parameters) -> None:
        """Unit mode: copy an (R, 6) matrix of search coordinates in."""
        if self.natural:
            raise ValueError('set_parameters: this population holds natural rows (set_values checks them)')
        self.parameters.copy_(self._rows(parameters, 'parameters'))
        self.decode()

    def decode(self) -> None:
        """`parameters` -> the table and the decoded values.  One launch, no host read."""
        self._check_parameters()
        mode = _lib.DIE_PHYSARUM_NATURAL if self.natural else _lib.DIE_PHYSARUM_UNIT
        space = None if self._space_struct is None else C.byref(self._space_struct)
        if self.episodes == 1:
            _lib.check(_lib.lib.die_physarum_decode_batch(_ptr(self.parameters), self.R, mode, space, _ptr(self._table),
                                                          _ptr(self._values), stream_ptr(self.env.device)), 'die_physarum_decode_batch')
        else:                                       # C rows in, the R-row table out: row c·E + e is candidate c's
            _lib.check(_lib.lib.die_physarum_decode_episodes(_ptr(self.parameters), self.candidates, self.episodes, mode, space,
                                                             _ptr(self._table), _ptr(self._values), stream_ptr(self.env.device)),
                       'die_physarum_decode_episodes')
        self._seen = (self.parameters.data_ptr(), self.parameters._version)

    def _sync(self) -> None:
        if (self.parameters.data_ptr(), self.parameters._version) != self._seen:     # written in place, or rebound
            self.decode()

    def values(self) -> np.ndarray:
        """The decoded (R, 6) float32 values (natural mode: the rows themselves), read from the device."""
        self._sync()
        return self._values.cpu().numpy().copy()

    def table(self) -> np.ndarray:
        """The device table as a structured array of R die_physarum_row records (read from the device)."""
        self._sync()
        return np.frombuffer(self._table.cpu().numpy().tobytes(), dtype=np.dtype(_lib.PhysarumRow)).copy()

    def _agent(self, v: np.ndarray, max_agents: int, seed: Optional[int]):
        from .agent.gradient import PhysarumAgent
        return PhysarumAgent(max_agents=max_agents, scale=float(v[0]), deposit=float(v[1]), sense_offset=float(v[2]),
                             normalized_grad=self.normalized_grad, grad_clip=self.grad_clip, turn_angle=float(v[3]),
                             sense_angle=float(v[4]), turn_tolerance=float(v[5]), seed=seed)

    def candidate(self, r: int):
        """Candidate r as a stand-alone PhysarumAgent(max_agents=K_r, seed=seed + r, **decoded row r) (with episodes: the
        agent of its first replica, r·E)."""
        return self._agent(self.values()[r], self.env.n[r * self.episodes], self.seed + r * self.episodes)

    def replica_agent(self, r: int):
        """The stand-alone PhysarumAgent replica r steps as: PhysarumAgent(max_agents=K_r, seed=seed + r, **decoded row r // E)."""
        return self._agent(self.values()[r // self.episodes], self.env.n[r], self.seed + r)

    def agent_from_row(self, row, max_agents: int = 10 ** 6, seed: Optional[int] = None):
        """A stand-alone PhysarumAgent from one row of this population's kind (a searcher's best / centre), decoded on the
        host with the device's float32 expressions."""
        v = np.asarray(torch.as_tensor(row).detach().cpu().to(torch.float32).numpy()).reshape(self.P)
        if not self.natural:
            v = self.space.decode(v)
        _check_physarum_values(v[None], ('given',))
        return self._agent(v, max_agents, seed)

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        """Headings and the forward-call counter as at construction, for the current `parameters` (the turn angle sets the
        headings' lattice): the decode launch and one `die_physarum_heading_batch` launch, no host read (small worlds)."""
        self._calls = 0
        self.decode()
        if self.env.per_replica:
            v = self.values()
            self.agents = [self._agent(v[r // self.episodes], self.env.n[r], self.seed + r) for r in range(self.R)]
            return
        b = self.env._batch_struct()
        _lib.check(_lib.lib.die_physarum_heading_batch(_ptr(self._hd_hi), _ptr(self._hd_lo), C.byref(b), _ptr(self._table),
                                                       self.seed & 0xFFFFFFFFFFFFFFFF, stream_ptr(self.env.device)),
                   'die_physarum_heading_batch')

    def _struct(self) -> _lib.GradientAgent:
        return _lib.GradientAgent(_lib.DIE_AGENT_PHYSARUM, int(self.normalized_grad), 0.0, 0.0, 0.0, 0.0, 0.0,
                                  -1.0 if self.grad_clip is None else self.grad_clip, 0.0, 0.0, 0.0, _ptr(self._hd_hi), _ptr(self._hd_lo),
                                  None, None, None, self.seed & 0xFFFFFFFFFFFFFFFF, self._calls & 0xFFFFFFFF, 0, None)

    def _launch(self, front: tuple, back: tuple, rows: tuple, stream) -> None:
        """BatchedPhysarumAgent._launch with the population's table after the struct (decoded first if `parameters` was written)."""
        self._sync()
        name = 'die_physarum_env_step_batch_rows' if rows else 'die_physarum_env_step_batch'
        _lib.check(getattr(_lib.lib, name)(*front, C.byref(self._struct()), _ptr(self._table), *back, *rows, stream), name)


def _architecture(agent: NeuralAutomataAgent) -> dict:
    """What every candidate of a population shares: the stack's shape, its boundary, the observed channels, the action scale."""
    layers = agent.model.conv_layers()
    return dict(kernel_sizes=tuple(int(k.kernel_size[0]) for k in layers), boundary=tuple(k.padding_mode for k in layers),
                with_agent_channel='agents' in agent.obs_channels, with_stock_channel=agent.with_stock_channel, scale=agent.action_coefs[0], deposit=agent.action_coefs[2],
                shapes=tuple(tuple(k.weight.shape) for k in layers), hidden_channels=agent.model.hidden_channels,
                hidden_activation=agent.model.hidden_activation, memory_channels=agent.memory_channels,
                signal_channels=agent.signal_channels, signal_constants=agent.signal_constants if agent.signal_channels else None,
                memory_inherit=agent.memory_inherit, memory_mutation=agent.memory_mutation)


class BatchedNeuralAutomataAgent(_Population):
    """A population of R NeuralAutomataAgent candidates of one architecture, candidate r stepping replica r of a BatchedEnv.
    The weights are ONE (R, P) float32 device tensor `parameters`: row r is `parameters_to_vector(model.parameters())` of
    candidate r — the layout evolution strategies hand around.  In-place writes to `parameters` are seen by the next step.
    (No `reset()` method here, deliberately: the searchers call a population's `reset()` every generation when it has one.)

    `episodes=E`: C = R / E candidates (`candidates`), candidate c stepping the E replicas c·E … c·E + E − 1 — replica c·E + e is
    `Env(field_size, dynamics, seed=env.seeds[c·E + e], max_agents=...)` driven by the agent of row c, bit for bit.  `parameters`
    is then ONE (C, P) matrix: the conv launches read row r / E (die_nca_batch.episodes), nothing is copied or expanded.

    Agent dropout (a template with `p_agent_dropout > 0` in training mode — torch's default, and where evotorch leaves a model)
    is opt-in through `dropout_seed`:
      * None (default): such a template is refused at the first step (the stand-alone agent's torch-RNG mask cannot be
        reproduced per replica);
      * an int: replica r's sense planes are multiplied by the counter-based mask (include/die_hip.h die_nca_dropout) of key
        `dropout_seed + r·dropout_seed_stride` — with episodes r = c·E + e — at forward call `dropout_step`, inside the last conv
        launch: replica r is the stand-alone run of `NeuralAutomataAgent(dropout_seed=dropout_seed + r·dropout_seed_stride)`.
        Stride 0 gives every replica the same mask (common random numbers across candidates).
    `dropout_step` is a public counter: it starts at 0, every `env.step` advances it by one, it may be written (setting it back
    replays the masks), and nothing resets it — not `env.reset()`, not the searchers — so every generation sees new masks.  In
    eval mode, or with p = 0, nothing is masked and the step is the one without dropout.

    The stock channel (a template built with `with_stock_channel=True`; every candidate then has it, `from_agents` refuses a
    mixed population): layer 0 reads one plane more, the `agent_food` of the agent standing on each cell.  `env.step` takes
    die_nca_env_step_batch_stock / die_nca_wide_env_step_batch_stock: one launch more (L + 3), which builds all R stock planes —
    owned by the BatchedEnv — from the agents as the step finds them; replica r stays the stand-alone run of `replica_agent(r)`,
    a stock-channel agent, bit for bit.  P grows by the first layer's extra input channel; episodes, agents_die, agents_born,
    max_agents, flows, per-replica Dynamics, dropout_seed, `action=` and both searchers take it as they are, and large worlds
    (`per_replica`) go through the stand-alone agents.  Refused with NotImplementedError before any launch and before
    `dropout_step` moves: `differentiable_sense`, `differentiable_action` and `forward_device` (so no action with a graph
    through such a population ever reaches `env.differentiable_step`).

    Memory channels (a template built with `memory_channels=M`; every candidate then has them, `from_agents` refuses a mix):
    `memory` is ONE (R, M, Nmax) float32 device tensor, `memory[r, :, :n[r]]` the stand-alone `replica_agent(r).memory` — by slot
    id, which is the storage index here.  `env.step` takes die_nca_wide_env_step_batch_memory: the standing build (the
    BatchedEnv's stock planes: one build serves the stock channel too), the expand into R·M planes this population owns, the L
    wide layers giving 3 + M planes, the memory read-out, then the parent's launches — L + 5 in all — and replica r stays the
    stand-alone run of `replica_agent(r)`, memory included, bit for bit.  With `episodes=E` every replica has its own memory: it
    is state of the world run, not of the candidate.  Large worlds (`per_replica`) go through the stand-alone agents, each
    keeping its own (`memory` is then None: read `agents[r].memory`).  `replica_agent(r)` / `candidate(r)` return agents with
    blank memory.  `reset_memory()` zeroes every replica's; a population WITH memory also carries an instance attribute `reset`
    bound to it — the searchers call a population's `reset()` every generation when it has one, after `env.reset()` — so every
    generation starts from blank memory, while a memoryless population still has no `reset`.  agents_die, max_agents and
    `reset(seed=...)`, flows, per-replica Dynamics, dropout_seed, `action=`, the stock channel and both searchers take memory as
    they are.  Refused with NotImplementedError: `Dynamics(agents_born=True)` together with memory and no rule of inheritance
    (`memory_inherit=None`), HERE in the constructor — a slot can die and be refilled within one step, so a newborn would inherit a
    dead agent's memory, and the stand-alone agent cannot see the Dynamics to refuse it itself.  With a rule
    (`memory_inherit='blank'` / `'copy'`, `memory_mutation`) the population breeds: `env.step(pop)` runs one more hook after the
    births, `inherit_memory(env.births_record())` — the record launch and die_memory_inherit_batch, two launches for all R — and
    replica r stays the stand-alone run of `replica_agent(r)`, which carries the rule.  Also refused: `differentiable_sense`,
    `differentiable_action` and `forward_device`,
    before any launch and before `dropout_step` or `memory` change.  The differentiable call of a population with memory is
    `recurrent_action(memory=None, parameters=None) -> (action, memory_next)`: the step's forward half with a graph through the
    read-outs, the stack and the expand, a `(C, P)` gradient, and `memory_next` chained from call to call for backpropagation
    through time (die_memory_grad.hip's batched twins, die_nca_wide_sense_batch_store_memory / _backward_batch_memory).

    Signal channels (a template built with `signal_channels=K`; every candidate then has them and the same three constants,
    `from_agents` refuses a mix): the population holds the fields of all replicas, `signals` an (R, K, W, H) float32 view of them —
    `signals[r]` the stand-alone `replica_agent(r).signals`, bit for bit.  `env.step` takes die_nca_wide_env_step_batch_signal: the
    standing build, the expand if M > 0, the L wide layers giving 3 + K + M planes, the memory read-out if M > 0, ONE launch that
    updates all K·R planes (die_signal.hip) into a second buffer that is then swapped, and the parent's launches — L + 4 in all,
    L + 6 with memory.  With `episodes=E` every replica has its own field.  Large worlds (`per_replica`) keep one stand-alone agent
    per replica, each with its own field (`signals` is then None: read `agents[r].signals`).  `reset_signals()` zeroes every
    replica's, and the instance attribute `reset` a memory population carries exists with K > 0 alone too and zeroes the memory and
    the fields — so the searchers score every candidate from a blank field.  agents_die, max_agents and `reset(seed=...)`, flows,
    per-replica Dynamics, dropout_seed, `action=`, the stock channel, memory and both searchers take signals as they are, and so
    does `Dynamics(agents_born=True)` while M = 0: the field has no per-slot state.  Refused with NotImplementedError before any
    launch and before `dropout_step`, `memory` or `signals` change: `differentiable_sense`, `differentiable_action`,
    `forward_device` and `recurrent_action`.  The call that has the adjoints is `signalling_action`: a step's forward half with a graph,
    through the field, the stack, the memory and, with `env.differentiable_step`, the worlds."""

    _signal_channels = 0                            # (a population without signal channels has neither)
    _signals = _signals_next = None

    def __init__(self, env: BatchedEnv, template: NeuralAutomataAgent, parameters=None, episodes: int = 1, *,
                 dropout_seed: Optional[int] = None, dropout_seed_stride: int = 1):
        if not isinstance(template, NeuralAutomataAgent):
            raise TypeError('template: a NeuralAutomataAgent')
        if template.memory_channels and env.dynamics.agents_born and template.memory_inherit is None:
            raise NotImplementedError(f'memory_channels={template.memory_channels} with Dynamics(agents_born=True): a slot can die and '
                                      'be refilled within one step, so a newborn would inherit a dead agent\'s memory (inheritance at '
                                      'birth is not defined yet)')
        if dropout_seed is not None and not _is_integer(dropout_seed):
            raise ValueError(f'dropout_seed={dropout_seed!r}: an integer, or None')
        if not _is_integer(dropout_seed_stride, 0):
            raise ValueError(f'dropout_seed_stride={dropout_seed_stride!r}: a non-negative integer')
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        self.dropout_seed_stride = int(dropout_seed_stride)
        self.dropout_step = 0
        self.episodes = _episodes(env, episodes)
        self.candidates = env.R // self.episodes
        self.env, self.template, self.R = env, template, env.R
        self._arch = _architecture(template)
        self._wide = template.model.wide            # hidden_channels / hidden_activation: die_nca_wide_env_step_batch
        self._stock_channel = template.with_stock_channel      # the *_stock entry points: one launch more, layer 0 one plane more
        self._memory_channels = template.memory_channels       # die_nca_wide_env_step_batch_memory: L + 5 launches
        # this population's step builds the env's stock planes (with memory: as its standing planes), so the next may build on top
        self._signal_channels = template.signal_channels       # die_nca_wide_env_step_batch_signal: L + 4 launches, L + 6 with memory
        self._builds_stock_planes = bool(self._stock_channel or self._memory_channels or self._signal_channels)
        self.memory = None                          # (R, M, Nmax) float32 by slot id (small worlds; large ones: agents[r].memory)
        self._signals = self._signals_next = None   # (K, R, W, H) float32 each (small worlds; large ones: agents[r].signals)
        if self._signal_channels:
            self.reset = self.reset_state           # on the INSTANCE: the searchers call `reset()` where a population has one
        elif self._memory_channels:
            self.reset = self.reset_memory
        template._check_wide()
        layers = template.model.conv_layers()
        for k in layers:
            if k.padding_mode not in _lib.PAD_MODES:
                raise NotImplementedError(f"boundary={k.padding_mode!r}: one of {sorted(_lib.PAD_MODES)}")
        if len(set(self._arch['boundary'])) != 1 or len(layers) > _lib.NCA_MAX_LAYERS:
            raise NotImplementedError(f'one boundary for every layer, at most {_lib.NCA_MAX_LAYERS} layers')
        self._layers = []                           # (k, cin, cout, offset in a row)
        self._acts = []                             # die_nca_layer.reserved of every layer
        off = 0
        for li, k in enumerate(layers):
            cout, cin, kk, _ = k.weight.shape
            # a wide stack's layers carry their activation in `reserved` (the last layer's is its tanh); a narrow one's say 0
            act = _lib.NCA_ACTIVATIONS['tanh' if li == len(layers) - 1 else self._arch['hidden_activation']] if self._wide else 0
            self._layers.append((int(kk), int(cin), int(cout), off))
            self._acts.append(act)
            off += k.weight.numel()
        self._channels = max(cout for _, _, cout, _ in self._layers) if self._wide else 4      # planes per replica of a scratch set
        self.P = off
        if parameters is None:
            parameters = parameters_to_vector(template.model.parameters()).detach().reshape(1, -1).expand(self.candidates, -1)
        self._matrix(parameters, 'parameters', 'P weights')         # (refused before anything is allocated)
        self.parameters = torch.empty((self.candidates, self.P), dtype=torch.float32, device=env.device)
        self.set_parameters(parameters)
        self._calls = 0
        self._c = None                              # (parameters' address, NcaLayer array, NcaBatch) of the last step
        if env.per_replica:
            self.agents = [self.unpack(template, self.parameters[r // self.episodes]) for r in range(self.R)]
            return
        need = _lib.lib.die_nca_wide_batch_scratch_bytes(env.W, env.H, self.R, len(layers), self._channels) if self._wide else \
            _lib.lib.die_nca_batch_scratch_bytes(env.W, env.H, self.R, len(layers))
        self._scratch = torch.empty(int(need) // 4, dtype=torch.float32, device=env.device)
        if self._memory_channels:
            M = self._memory_channels
            self.memory = torch.zeros((self.R, M, env.Nmax), dtype=torch.float32, device=env.device)
            # plane j of replica r at (j·R + r)·W·H: a batched layer launch reads plane j of every replica one plane apart
            self._memory_planes = torch.empty((M, self.R, env.W, env.H), dtype=torch.float32, device=env.device)
        if self._signal_channels:
            # plane k of replica r at (k·R + r)·W·H, as the memory planes lie: layer 0 reads plane k of every replica one plane apart
            self._signals = torch.zeros((self._signal_channels, self.R, env.W, env.H), dtype=torch.float32, device=env.device)
            self._signals_next = torch.empty_like(self._signals)

    @property
    def signals(self) -> Optional[torch.Tensor]:
        """The signal fields of every replica as an (R, K, W, H) float32 view (None without signal channels, and on large worlds,
        where every stand-alone agent keeps its own).  The view is of the current buffer: take it again after a step."""
        return None if self._signals is None else self._signals.permute(1, 0, 2, 3)

    def reset_signals(self) -> None:
        """A blank field for every replica (large worlds: for every stand-alone agent).  A population without signal channels has
        nothing to reset."""
        if self._signals is not None:
            self._signals.zero_()
        for ag in getattr(self, 'agents', ()):
            ag.reset_signals()

    def reset_state(self) -> None:
        """Blank memory and blank fields: what the searchers' `reset()` does for a population with signal channels."""
        self.reset_memory()
        self.reset_signals()

    def reset_memory(self) -> None:
        """Blank memory for every replica (large worlds: for every stand-alone agent).  A population without memory channels
        has nothing to reset."""
        if self.memory is not None:
            self.memory.zero_()
        for ag in getattr(self, 'agents', ()):
            ag.reset_memory()

    @classmethod
    def from_agents(cls, env: BatchedEnv, agents: Sequence[NeuralAutomataAgent], episodes: int = 1, *,
                    dropout_seed: Optional[int] = None, dropout_seed_stride: int = 1) -> 'BatchedNeuralAutomataAgent':
        """Candidate r = agents[r]; every agent must share agents[0]'s architecture."""
        if len(agents) * _episodes(env, episodes) != env.R:
            raise ValueError(f'{len(agents)} agents for {env.R} replicas' + (f' of {episodes} episodes per candidate' if episodes != 1 else ''))
        want = _architecture(agents[0])
        for r, ag in enumerate(agents):
            if _architecture(ag) != want:
                raise ValueError(f'agent {r}: architecture {_architecture(ag)} differs from agent 0\'s {want}')
        return cls(env, agents[0], cls.pack(agents), episodes, dropout_seed=dropout_seed, dropout_seed_stride=dropout_seed_stride)

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def pack(agents: Sequence[NeuralAutomataAgent]) -> torch.Tensor:
        """(R, P) float32: row r = parameters_to_vector of agents[r]'s model (on that model's device)."""
        return torch.stack([parameters_to_vector(ag.model.parameters()).detach().to(torch.float32) for ag in agents])

    @staticmethod
    def unpack(template: NeuralAutomataAgent, row: torch.Tensor, dropout_seed: Optional[int] = None) -> NeuralAutomataAgent:
        """A stand-alone agent of the template's constructor arguments whose weights are `row` (copied); `dropout_seed`, when
        given, replaces the template's."""
        args = dict(template.init_params)
        args.update(args.pop('model_kwargs', {}))
        if dropout_seed is not None:
            args['dropout_seed'] = dropout_seed
        with torch.random.fork_rng(devices=[]):     # (the throw-away initial weights leave the caller's RNG alone)
            ag = NeuralAutomataAgent(**args)
        ag.model.train(template.model.training)
        ref = next(ag.model.parameters())
        vector_to_parameters(row.detach().to(device=ref.device, dtype=ref.dtype).clone(), ag.model.parameters())
        return ag

    def set_parameters(self, parameters) -> None:
        """Copy an (R, P) matrix of candidate rows in ((C, P) with episodes: one row per candidate)."""
        with torch.no_grad():                       # (`parameters` may be a leaf that requires grad: an optimiser's)
            self.parameters.copy_(self._matrix(parameters, 'parameters', 'P weights'))

    def candidate(self, r: int) -> NeuralAutomataAgent:
        """Candidate r as a stand-alone NeuralAutomataAgent (on the host: `save()` the winner).  With a `dropout_seed` it carries
        the key of its replica (with episodes: of its first replica, r·E), `dropout_seed + r·E·dropout_seed_stride`, and a
        `dropout_step` of 0: set it to the population's counter at the step to be replayed."""
        return self.unpack(self.template, self.parameters[r].cpu(), self._replica_dropout_seed(r * self.episodes))

    def replica_agent(self, r: int) -> NeuralAutomataAgent:
        """The stand-alone NeuralAutomataAgent replica r steps as: the weights of row r // E and, with a `dropout_seed`, the key
        `dropout_seed + r·dropout_seed_stride` (its `dropout_step` starts at 0)."""
        return self.unpack(self.template, self.parameters[r // self.episodes].cpu(), self._replica_dropout_seed(r))

    def _replica_dropout_seed(self, r: int) -> Optional[int]:
        return None if self.dropout_seed is None else self.dropout_seed + r * self.dropout_seed_stride

    def _replica_agent(self, r: int) -> NeuralAutomataAgent:
        ag = self.agents[r]                         # its candidate's row is reloaded every step: in-place writes are seen
        vector_to_parameters(self.parameters[r // self.episodes].detach(), ag.model.parameters())
        if self.dropout_seed is not None:           # replica r's own key, at the population's counter
            ag.dropout_seed, ag.dropout_step = self._replica_dropout_seed(r), self.dropout_step
            ag.model.train(self.template.model.training)
        return ag

    def _dropout(self) -> Optional[_lib.NcaDropout]:
        """die_nca_dropout of the coming step, or None when nothing is masked (eval mode, p = 0)."""
        model = self.template.model
        if self.dropout_seed is None or not (model.agent_dropout.p > 0 and model.training):
            return None
        return _lib.nca_dropout(model.agent_dropout.p, self.dropout_seed, self.dropout_seed_stride, self.dropout_step)

    def _stepped(self) -> None:
        if self.dropout_seed is not None:
            self.dropout_step += 1                  # counts forward calls, masked or not (as NeuralAutomataAgent.sense does)
        if self._signals is not None:               # the step wrote every replica's next field into the second buffer
            self._signals, self._signals_next = self._signals_next, self._signals

    def _inherit(self, env: BatchedEnv) -> None:
        """BatchedEnv.step's hook after the births: with a rule (`memory_inherit`) the newborns of every replica receive their memory."""
        if self.template.memory_inherit is not None and env.dynamics.agents_born:
            self.inherit_memory(env.births_record())

    def inherit_memory(self, record, memory: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`NeuralAutomataAgent.inherit_memory` for every replica in one launch (die_memory_inherit_batch): `record` the
        `env.births_record()` of the step that just ran.  `memory` None: `self.memory`, the (R, M, Nmax) tensor, is updated in place
        and returned — `env.step(population)` does this by itself after the births where the template has a rule; after
        `env.step_action(...)` it is the caller's.  `memory`: an (R, M, Nmax) float32 tensor on the env's device, the `memory_next`
        of `recurrent_action` / `signalling_action`: returns `functional.inherit_memory_batch(...)` with a `grad_fn` and leaves
        `self.memory` holding the same bits.  Replica r is the stand-alone `replica_agent(r).inherit_memory` on the record of its
        own stand-alone Env, bit for bit.  Refused with ValueError before any launch, `memory` untouched: a population without
        memory channels or without a rule, a record that is no batched BirthsRecord, a memory of the wrong shape, dtype or
        device; large worlds (`per_replica`) with NotImplementedError: `agents[r].inherit_memory(env.envs[r].births_record())`."""
        from .functional import check_inherit_operands, inherit_memory_, inherit_memory_batch
        t, M = self.template, self._memory_channels
        if not M:
            raise ValueError('inherit_memory: a population without memory channels (memory_channels=0) has nothing to inherit')
        if t.memory_inherit is None:
            raise ValueError("inherit_memory: this population has no rule (memory_inherit=None): build its template with "
                             "memory_inherit='blank' or 'copy'")
        if self.env.per_replica:
            raise NotImplementedError('inherit_memory: large worlds (per_replica) are not batched — every replica steps a stand-alone '
                                      'agent: use agents[r].inherit_memory(env.envs[r].births_record())')
        if memory is None:
            check_inherit_operands('inherit_memory (self.memory)', self.memory, record, True, M, contiguous=True)
            return inherit_memory_(self.memory, record, t.memory_inherit, t.memory_mutation)
        check_inherit_operands('inherit_memory', memory, record, True, M)
        out = inherit_memory_batch(memory, record, t.memory_inherit, t.memory_mutation)
        with torch.no_grad():
            self.memory.copy_(out)                  # the population's own copy, not the graph's tensor
        return out

    # ------------------------------------------------------------------ step
    def _check_step(self, env: BatchedEnv) -> None:
        super()._check_step(env)
        model = self.template.model
        if model.agent_dropout.p > 0 and model.training and self.dropout_seed is None:
            raise NotImplementedError('p_agent_dropout > 0 in training mode: without a dropout_seed its mask is a host-RNG torch op, '
                                      'not batched (build the population with dropout_seed=S for the counter-based mask, call '
                                      'model.eval(), or step the candidates one at a time)')

    def _claim_epoch(self, env: BatchedEnv) -> None:
        # the sensing reads the claim plane at the current epoch, the claims are made at the next one; at the wrap the
        # library clears the claim planes between the two (Env.step runs forward before its next_epoch the same way)
        self._sense_epoch = env.epoch
        env.epoch = env.epoch % _lib.OWNER_EPOCH_MAX + 1

    def _launch(self, front: tuple, back: tuple, rows: tuple, stream) -> None:
        """BatchedPhysarumAgent._launch with the dropout mask of the coming step after the workspace: one entry point without
        it, one with it (the same step, its last conv launch masked), and with Dynamics rows one for both, the mask nullable."""
        drop = self._dropout()
        mask = None if drop is None else C.byref(drop)
        if self._wide or self._stock_channel:       # ONE entry point whatever is set: the mask and the two tables are all nullable
            tail = (mask, *(rows or (None, None)))
            if self._signal_channels:               # the memory variant's tail (M = 0: no memory), then K, both field buffers, the constants
                name = 'die_nca_wide_env_step_batch_signal'
                tail += (_ptr(self.env._stock_planes()), self._memory_channels, _ptr(self.memory) if self._memory_channels else None,
                         _ptr(self._memory_planes) if self._memory_channels else None, int(self._stock_channel), self._signal_channels,
                         _ptr(self._signals), _ptr(self._signals_next), *self.template.signal_constants)
            elif self._memory_channels:             # then the env's stock planes, M, the memory, its planes, whether layer 0 reads the stock
                name = 'die_nca_wide_env_step_batch_memory'
                tail += (_ptr(self.env._stock_planes()), self._memory_channels, _ptr(self.memory), _ptr(self._memory_planes),
                         int(self._stock_channel))
            elif self._stock_channel:               # then the env's stock planes
                name = 'die_nca_wide_env_step_batch_stock' if self._wide else 'die_nca_env_step_batch_stock'
                tail += (_ptr(self.env._stock_planes()),)
            else:
                name = 'die_nca_wide_env_step_batch'
        elif rows:
            name, tail = 'die_nca_env_step_batch_rows', (mask, *rows)
        elif drop is None:
            name, tail = 'die_nca_env_step_batch', ()
        else:
            name, tail = 'die_nca_env_step_batch_dropout', (mask,)
        _lib.check(getattr(_lib.lib, name)(*front, C.byref(self._struct(self._sense_epoch)), *back, *tail, stream), name)

    def _nca_batch(self, base: int, sense_epoch: int, scratch: Optional[torch.Tensor] = None):
        """(layer array, die_nca_batch) reading the (C, P) matrix at address `base` (a wide stack's layers carry their activation,
        0 for a narrow one's); `scratch`: the step's planes, none for the calls that keep every layer in caller-owned storage."""
        layers = (_lib.NcaLayer * len(self._layers))(*[_lib.NcaLayer(k, cin, cout, act, base + 4 * off, self.P)
                                                        for (k, cin, cout, off), act in zip(self._layers, self._acts)])
        nca = _lib.NcaBatch(len(self._layers), _lib.PAD_MODES[self._arch['boundary'][0]], int(self._arch['with_agent_channel']), sense_epoch,
                            layers, (C.c_float * 3)(*self.template.action_coefs), 0 if self.episodes == 1 else self.episodes,
                            _ptr(scratch), 0 if scratch is None else scratch.numel() * 4)
        return layers, nca

    def _struct(self, sense_epoch: int) -> _lib.NcaBatch:
        """The step's die_nca_batch: built once per `parameters` storage, only the sensing epoch is written every step."""
        base = self.parameters.data_ptr()
        if self._c is None or self._c[0] != base:
            self._c = (base, *self._nca_batch(base, 0, self._scratch))
        nca = self._c[2]
        nca.sense_epoch = sense_epoch
        return nca

    # ------------------------------------------------------------------ the differentiable twins (die_nca_grad.hip, batched)
    def _refuse_large_worlds(self, what: str, alone: str) -> None:
        if self.env.per_replica:
            raise NotImplementedError(f'{what}: large worlds (per_replica) are not batched — a large world fills the GPU '
                                      f'through the stand-alone {alone}')

    def _check_differentiable(self, parameters: Optional[torch.Tensor], what: str = 'differentiable mode') -> torch.Tensor:
        """Every refusal of a differentiable call, before anything is launched; returns the matrix the call reads.  `what`: the
        word the messages carry — 'differentiable mode' for the narrow calls, 'forward_device' for the wide twin, which takes a wide
        stack and refuses a narrow one."""
        wide = what == 'forward_device'
        self.template._check_differentiable(what, wide_ok=wide)
        if wide and not self._wide:
            raise ValueError('forward_device: a narrow population (hidden_channels and hidden_activation both None) is differentiated '
                             'by differentiable_sense')
        env = self.env
        self._refuse_large_worlds(what, 'ConvolutionModel.forward_device (replica_agent(r).model)' if wide else
                                  'NeuralAutomataAgent.differentiable_action (replica_agent(r))')
        if self._arch['boundary'][0] not in ('circular', 'zeros'):
            raise NotImplementedError(f"boundary={self._arch['boundary'][0]!r} in {what}: 'circular' or 'zeros' (step() "
                                      f"takes all of {sorted(_lib.PAD_MODES)})")
        self._check_step(env)
        p = self.parameters if parameters is None else parameters
        self._check_parameters(p)
        return p

    def _differentiable(self, parameters: Optional[torch.Tensor], what: str) -> torch.Tensor:
        """`differentiable_sense` and `forward_device` alike: the refusals, the graph's node, the dropout counter."""
        p = self._check_differentiable(parameters, what)
        out = _BatchedSense.apply(self, p, self.env.chem_node, None, None)
        if self.dropout_seed is not None:
            self.dropout_step += 1
        return out

    def differentiable_sense(self, parameters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The sense planes of every replica with a `grad_fn`: (R, 3, W, H) float32, `out[r]` bit for bit replica r's stand-alone
        `differentiable_sense` (what the coming `env.step` would read).  `parameters`: the (C, P) float32 device matrix to read and
        to differentiate with respect to — default `self.parameters`, which may have been marked `requires_grad_()`; its gradient
        is a (C, P) tensor, row c the float64 sum over candidate c's E worlds of the stand-alone gradients, rounded once (E = 1:
        the stand-alone gradient of replica c, bit for bit; no float atomics, the same bits on every run).

        L conv launches forward for all R replicas (L + 1 with a dropout mask: masked for the value, unmasked for the graph) and
        2 L backward.  Every layer's output lives in storage the graph owns and the first layer's inputs (claim, food and chem
        planes of all replicas) are copied, so `backward` may run after `env.step`.  With a `dropout_seed`, in training mode and
        p > 0, replica r is masked with key `dropout_seed + r·dropout_seed_stride` at `dropout_step`; the counter advances once per
        call whenever a `dropout_seed` is set.  Small worlds, 'circular' / 'zeros' boundaries; anything else raises
        NotImplementedError before any launch.  `step()` is untouched by all this.  A population of wide stacks
        (`hidden_channels` / `hidden_activation`) is refused here: NotImplementedError too, before any launch and before
        `dropout_step` moves.  Its gradients come from `forward_device` and `die_amd.functional.gather_scale_batch`.  A
        population with the stock channel (`with_stock_channel=True`) is refused the same way, here, in `differentiable_action`
        and in `forward_device`: the stock plane is piecewise constant in the weights and the adjoint calls do not take its kind."""
        return self._differentiable(parameters, 'differentiable mode')

    def differentiable_action(self, parameters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The actions of every replica with a `grad_fn`: (3, R, Nmax) float32 in the batch's action layout (what
        `env.step(..., action=...)` fills) — `out[:, r, :env.n[r]]` is replica r's stand-alone `differentiable_action`, bit for
        bit; the padding slots from n[r] on are 0 and receive no gradient.  One more launch than `differentiable_sense` each way
        (the read-out and its adjoint, die_gather_scale_batch / _backward_batch); the slots' coordinates are copied.  Where several
        slots of a replica with a non-zero gradient stand on one cell their terms are added by fp32 atomics in arrival order;
        otherwise (alive agents never share a cell) the gradient's bits are fixed."""
        sense = self.differentiable_sense(parameters)
        return _BatchedReadOut.apply(sense, self)

    def forward_device(self, parameters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A population of wide stacks on the device, differentiable — the wide twin of `differentiable_sense`, and the batched
        twin of `ConvolutionModel.forward_device`: (R, 3, W, H) float32 with a `grad_fn`, `out[r]` bit for bit what the coming
        `env.step` would sense on replica r and what `replica_agent(r).model.forward_device` returns on its planes.
        `parameters`: the (C, P) float32 device matrix to read and to differentiate with respect to — default `self.parameters`;
        its gradient is a (C, P) tensor, row c the float64 sum over candidate c's E worlds rounded once (E = 1: the stand-alone
        gradient of replica c, bit for bit; no float atomics, the same bits on every run).

        L launches of the wide layer kernel forward for all R replicas (L + 1 with a dropout mask) and 3 L − 1 backward
        (die_nca_wide_backward_batch: both adjoint GEMMs on the fp32 matrix instruction with the replica in blockIdx.z, and the
        fold), 3 L when the env carries a chem node that needs a gradient (`benv.differentiable_step`): the chem channel's planes
        of the first layer's input gradient then go to that node.  Every layer's output lives in storage the graph owns and the
        first layer's inputs are copied, so `backward` may run after `env.step`.  With a `dropout_seed`, in training mode and
        p > 0, replica r is masked with key `dropout_seed + r·dropout_seed_stride` at `dropout_step`; the counter advances once per
        call whenever a `dropout_seed` is set.  Refused before any launch and before `dropout_step` moves: a narrow population
        (ValueError: it has `differentiable_sense`), a population with the stock channel, large worlds (`per_replica`) and
        'reflect' / 'replicate' boundaries (NotImplementedError)."""
        return self._differentiable(parameters, 'forward_device')

    def recurrent_action(self, memory: Optional[torch.Tensor] = None, parameters: Optional[torch.Tensor] = None):
        """`env.step`'s forward half for a population with memory channels, with a graph: `(action, memory_next)`, (3, R, Nmax)
        and (R, M, Nmax) float32, both with a `grad_fn` — the batched twin of `NeuralAutomataAgent.recurrent_action`.
        `action[:, r, :n[r]]` and `memory_next[r, :, :n[r]]` are bit for bit `replica_agent(r).recurrent_action(obs_r,
        memory[r, :, :n[r]])`; `action` is also what `env.step(pop, action=buf)` records and `memory_next` what that step leaves in
        `pop.memory`.  The padding slots from n[r] on are 0 and receive no gradient.

        `memory`: None — `self.memory`, a constant of the graph — or an (R, M, Nmax) float32 tensor on the env's device, used as
        given: the `memory_next` of the previous call gives backpropagation through time, its `.detach()` truncates the gradient
        there, a leaf that requires grad receives one.  `parameters`: the (C, P) matrix to read and differentiate with respect
        to (default `self.parameters`); its gradient is a (C, P) tensor, row c the float64 sum over candidate c's E worlds rounded
        once (E = 1: replica c's stand-alone gradient, bit for bit at one step).

        In order: the standing planes and the record (`functional.memory_record_batch`: a buffer this population owns, not the
        env's stock planes), the expand (`functional.memory_planes_batch`), the wide stack (die_nca_wide_sense_batch_store_memory:
        L launches, L + 1 with a mask), the read-out of planes 0..2 (die_gather_scale_batch) and of planes 3.. through the record:
        L + 5 launches forward.  Backward: the two scatters into ONE (R, 3 + M, W, H) buffer, the stack's adjoint
        (die_nca_wide_backward_batch_memory: 3 L with the first layer's input gradient, which the incoming memory's graph or a
        chem node asks for, else 3 L - 1) and the expand's gather.  Records, planes and every layer's output are kept by the
        graph, so `backward` may run after the worlds have been stepped or reset.  With `env.chem_node` current the node is the
        stack's chem plane: `env.differentiable_step(action)` between two calls unrolls through the worlds too.

        The population is left as a step's forward would leave it: `self.memory` holds a copy of `memory_next`'s values in its
        own storage, `dropout_step` has advanced once if a `dropout_seed` is set.  episodes, agents_die, max_agents, per-replica
        Dynamics, a food flow and seeded dropout are taken.  Refused before any launch, and before `dropout_step` or `memory`
        change: a population without memory (ValueError: it has `forward_device`); with NotImplementedError the stock channel,
        large worlds (`per_replica`), fp16 fields, 'reflect' / 'replicate' and an unseeded `p_agent_dropout` > 0 in training
        mode; with ValueError a `memory` of the wrong shape, dtype or device."""
        if self._signal_channels:
            self.template._check_signals('recurrent_action')
        if not self._memory_channels:
            raise ValueError('recurrent_action: a population without memory channels (memory_channels=0) is differentiated by '
                             'forward_device / differentiable_action')
        action, _, memory_next = self._stateful_action('recurrent_action', None, memory, parameters)
        return action, memory_next

    def signalling_action(self, signals: Optional[torch.Tensor] = None, memory: Optional[torch.Tensor] = None,
                          parameters: Optional[torch.Tensor] = None):
        """`env.step`'s forward half for a population with signal channels, with a graph: `(action, signals_next, memory_next)`,
        (3, R, Nmax), (R, K, W, H) and (R, M, Nmax) float32, each with a `grad_fn` (`memory_next` is None without memory) — the
        batched twin of `NeuralAutomataAgent.signalling_action`.  `action[:, r, :n[r]]`, `signals_next[r]` and `memory_next[r, :,
        :n[r]]` are bit for bit `replica_agent(r).signalling_action(obs_r, signals[r], memory[r, :, :n[r]])`; `action` is also what
        `env.step(pop, action=buf)` records, `signals_next` what that step leaves in `pop.signals` and `memory_next` what it leaves
        in `pop.memory`.

        `signals`: None — `self.signals`, a constant of the graph — or an (R, K, W, H) float32 tensor on the env's device, of any
        strides (inside, the fields lie (K, R, W, H); gradients come back in the shape given): the `signals_next` of the previous
        call gives backpropagation through time through the medium, its `.detach()` truncates the gradient there, a leaf that
        requires grad receives one.  `memory` and `parameters`: as in `recurrent_action` — the gradient of `parameters` is a
        (C, P) tensor, row c the float64 sum over candidate c's E worlds rounded once.  With `env.chem_node` current the node is
        the stack's chem plane: `env.differentiable_step(action)` between two calls unrolls through the worlds too.

        In order: the standing planes (a buffer this population owns, one build for both records), `functional.signal_record_batch`
        (ONE die_signal_cells_batch launch), with memory `functional.memory_record_batch` and `memory_planes_batch`, the wide stack
        (die_nca_wide_sense_batch_store_signal: L launches, L + 1 with a mask), the read-out of planes 0..2
        (die_gather_scale_batch), `functional.signal_step_batch` on planes 3 .. 3 + K - 1 and `functional.gather_memory_batch` on
        planes 3 + K .. .  Backward: the scatters, ONE die_signal_step_backward_batch launch for all K·R planes, the stack's adjoint
        (die_nca_wide_backward_batch_signal: 3 L with the first layer's input gradient, which an incoming field or memory with a
        graph or a chem node asks for, else 3 L - 1) and the expand's gather.  Two gradients reach a `signals_next` that is handed
        on — the next stack's input gradient and the next link's field gradient — and autograd sums them.  Records, planes and
        every layer's output are kept by the graph, so `backward` may run after the worlds were stepped, reset or reseeded and
        after `reset_signals()`.

        The population is left as a step's forward leaves it: `self.signals` and `self.memory` hold copies of the values in their
        own storage, `dropout_step` has advanced once if a `dropout_seed` is set.  Refused before any launch, and before
        `dropout_step`, `signals` or `memory` change: a population without signal channels (ValueError: it has `recurrent_action`
        / `forward_device`); with NotImplementedError the stock channel, large worlds (`per_replica`), fp16 fields, 'reflect' /
        'replicate' and an unseeded `p_agent_dropout` > 0 in training mode; with ValueError a `signals` or `memory` of the wrong
        shape, dtype, device or type, and a `memory` given to a population without memory channels."""
        if not self._signal_channels:
            raise ValueError('signalling_action: a population without signal channels (signal_channels=0) is differentiated by '
                             'recurrent_action (memory channels) or forward_device / differentiable_action')
        return self._stateful_action('signalling_action', signals, memory, parameters)

    def _check_stateful(self, what: str, parameters: Optional[torch.Tensor]) -> torch.Tensor:
        """Every refusal `recurrent_action` and `signalling_action` share, before anything is launched (`what`: the caller's name,
        the prefix of the texts and the stand-alone method that large worlds are sent to); returns the matrix the call reads."""
        env = self.env
        if self._stock_channel:
            raise NotImplementedError(f'{what}: no gradients with the stock channel (with_stock_channel=True): its plane is '
                                      'piecewise constant in the weights and the adjoint kernels do not take its kind')
        self._refuse_large_worlds(what, f'NeuralAutomataAgent.{what} (replica_agent(r))')
        if env.dtype != torch.float32:
            raise NotImplementedError(f'{what}: fp32 fields only (this batch holds {env.dtype})')
        if self._arch['boundary'][0] not in ('circular', 'zeros'):
            raise NotImplementedError(f"{what}: boundary={self._arch['boundary'][0]!r} in differentiable mode: 'circular' or "
                                      f"'zeros' (step() takes all of {sorted(_lib.PAD_MODES)})")
        self._check_step(env)
        p = self.parameters if parameters is None else parameters
        self._check_parameters(p)
        return p

    def _stateful_action(self, what: str, signals, memory, parameters):
        """The one body of `recurrent_action` (K = 0: no field, `signals_next` None) and `signalling_action`: the refusals, the
        standing planes and the records, the expand, the stack (`_BatchedSense`), the read-outs, the population's own copies.
        One branch: without a field the read-out is the fused node `_BatchedRecurrentReadOut` — ONE gradient buffer that its two
        scatters fill — with a field three nodes whose gradients autograd adds; other launches and another order of sums, so
        neither form replaces the other bit for bit."""
        from .functional import (_standing_planes_batch, gather_memory_batch, memory_planes_batch, memory_record_batch,
                                 signal_record_batch, signal_step_batch)
        K, M, env = self._signal_channels, self._memory_channels, self.env
        p = self._check_stateful(what, parameters)
        if signals is not None:
            check_given(what, 'signals', signals, (self.R, K, env.W, env.H), env.device)
        if memory is not None and not M:
            raise ValueError(f'{what}: memory given to a population without memory channels (memory_channels=0)')
        if memory is not None:
            check_given(what, 'memory', memory, (self.R, M, env.Nmax), env.device)
        field = None
        if K:
            # the fields as the launches read them, (K, R, W, H); the population's own are copied: they are written below, the graph's stay
            field = self._signals.clone() if signals is None else signals.permute(1, 0, 2, 3).contiguous()
        if M and memory is None:
            memory = self.memory
        standing = _standing_planes_batch(self)
        cells = signal_record_batch(self, standing) if K else None
        record = memory_record_batch(self, standing) if M else None
        expanded = memory_planes_batch(memory, record) if M else None
        sense = _BatchedSense.apply(self, p, env.chem_node, field, expanded)
        if self.dropout_seed is not None:
            self.dropout_step += 1
        signals_next = None
        if not K:
            action, memory_next = _BatchedRecurrentReadOut.apply(sense, self, record)
        else:
            action = _BatchedReadOut.apply(sense[:, :3], self)
            deposit, sigma, decay = self.template.signal_constants
            signals_next = signal_step_batch(field.permute(1, 0, 2, 3), sense[:, 3:3 + K], cells, deposit=deposit, sigma=sigma, decay=decay)
            memory_next = gather_memory_batch(sense[:, 3 + K:], record) if M else None
        with torch.no_grad():                       # the population's own copies, not the graph's tensors
            if K:
                self._signals.copy_(signals_next.permute(1, 0, 2, 3))
            if M:
                self.memory.copy_(memory_next)
        return action, signals_next, memory_next

    def render(self, r: int) -> np.ndarray:
        """Replica r's last sense planes with the channel axis last: the stand-alone agent's `render()[0]`."""
        if self.env.per_replica:
            torch.cuda.synchronize(self.env.device)
            return self.agents[r].render()[0]
        if self._calls == 0:
            return np.ones((2, 2, 3))
        L, W, H = len(self._layers), self.env.W, self.env.H
        sets = self._scratch.view(-1, self.R, self._channels, W, H)
        return torch.moveaxis(sets[(L - 1) % sets.shape[0], r, :3], 0, -1).cpu().numpy()


def _geometry(env: BatchedEnv) -> _lib.Medium:
    """A die_medium that only says how large a replica is (the read-out's cell arithmetic)."""
    return _bare_medium(env.W, env.H, 1)


class _BatchedFieldStep(torch.autograd.Function):
    """BatchedEnv.differentiable_step's node: the value is a copy of the chem planes the step left, the backward
    die_env_step_backward_batch — the forward's own sweep on the gradient planes and a gather at the recorded winners' cells."""

    @staticmethod
    def forward(ctx, prev_node, action, cells, chem, env):
        ctx.save_for_backward(cells)
        d = env.dynamics
        ctx.batch, ctx.size, ctx.dev = env._batch_struct(), (env.R, env.W, env.H, env.Nmax), chem.device
        ctx.sigma, ctx.decay = float(d.diffuse_sigma), float(d.rate_decay_chem)
        ctx.rows = None if env._rows is None else (env._rows, env._rows_host)      # per-replica Dynamics: built once, never written
        return chem.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        cells, = ctx.saved_tensors
        (R, W, H, Nmax), dev = ctx.size, ctx.dev
        g = grad.to(dtype=torch.float32).contiguous()
        grad_chem = torch.empty((R, W, H), dtype=torch.float32, device=dev)
        grad_action = None
        if ctx.needs_input_grad[1]:
            grad_action = torch.zeros((3, R, Nmax), dtype=torch.float32, device=dev)     # dx, dy: positions are constants of the parameters
        rows = (None, None) if ctx.rows is None else (_ptr(ctx.rows[0]), ctx.rows[1])
        _lib.check(_lib.lib.die_env_step_backward_batch(W, H, C.byref(ctx.batch), _ptr(g), ctx.sigma, ctx.decay, *rows, _ptr(cells),
                                                        _ptr(grad_chem), None if grad_action is None else grad_action[2].data_ptr(),
                                                        stream_ptr(dev)), 'die_env_step_backward_batch')
        return grad_chem if ctx.needs_input_grad[0] else None, grad_action, None, None, None


# the stack's entry points by the kind of population: (store, the adjoint's workspace query, the adjoint).  The stateful kinds'
# calls end in the planes their first layer reads besides the field's: (mem_planes, M) and (mem_planes, M, signal_planes, K)
_SENSE_CALLS = {
    'narrow': ('die_nca_sense_batch_store', 'die_nca_backward_batch_workspace_bytes', 'die_nca_backward_batch'),    # (or `_inputs`, below)
    'wide': ('die_nca_wide_sense_batch_store', 'die_nca_wide_backward_batch_workspace_bytes', 'die_nca_wide_backward_batch'),
    'memory': ('die_nca_wide_sense_batch_store_memory', 'die_nca_wide_backward_batch_memory_workspace_bytes',
               'die_nca_wide_backward_batch_memory'),
    'signal': ('die_nca_wide_sense_batch_store_signal', 'die_nca_wide_backward_batch_signal_workspace_bytes',
               'die_nca_wide_backward_batch_signal'),
}


def _sense_kind(pop, K: int, M: int) -> str:
    return 'signal' if K else 'memory' if M else 'wide' if pop._wide else 'narrow'


def _state_planes(K: int, M: int, field, mem_planes) -> tuple:
    """What the stateful kinds' three calls end in (nothing for a narrow or a plain wide stack)."""
    memory = (_ptr(mem_planes) if M else None, M)
    return memory + (_ptr(field), K) if K else memory if M else ()


class _BatchedSense(torch.autograd.Function):
    """The stack of every differentiable call of a BatchedNeuralAutomataAgent, ONE node: differentiable_sense (narrow),
    forward_device (wide), recurrent_action (a wide stack whose first layer also reads the M expanded memory planes of every replica,
    `mem_planes`, and whose last layer gives M planes more) and signalling_action (the K signal planes too, `field`, the (K, R, W, H)
    contiguous field as the launches read it, ahead of the memory's).  `field` / `mem_planes` are None where the population has no
    such channels.  The entry points: `_SENSE_CALLS`.  A narrow stack has two adjoints — die_nca_backward_batch, or with the env's chem
    node as an input that needs a gradient die_nca_backward_batch_inputs; every wide kind ONE, whose `grad_in` is null where nothing
    asks for it.  Returns (R, 3 + K + M, W, H); the backward hands the (C, P) gradient to `parameters`, the chem channel of the first
    layer's input gradient to the env's chem node, its K signal channels to `field` and its M memory channels to the expand —
    views, in their (·, R, W, H) shapes."""

    @staticmethod
    def forward(ctx, pop, parameters, chem_node, field, mem_planes):
        env = pop.env
        R, W, H, L, dev, Cm = env.R, env.W, env.H, len(pop._layers), env.device, pop._channels
        K, M = (pop._signal_channels if field is not None else 0), (pop._memory_channels if mem_planes is not None else 0)
        with_agents = pop._arch['with_agent_channel']
        # as they are now: the worlds will be stepped (the claim plane only where the first layer reads it)
        planes = [env.food.clone(), env.chem.clone()] + ([env.owner.clone()] if with_agents else [])
        # (M, R, W, H): the expand's own storage, as the launch reads it
        state = ([field] if K else []) + ([mem_planes.contiguous()] if M else [])
        store = torch.empty((L, R, Cm, W, H), dtype=torch.float32, device=dev)
        drop = pop._dropout()
        masked = None if drop is None else torch.empty((R, Cm, W, H), dtype=torch.float32, device=dev)
        # (the stateful calls refuse fp16 fields before they come here)
        ctx.epoch, ctx.fdt = env.epoch, _lib.DIE_F32 if env.dtype == torch.float32 else _lib.DIE_F16
        ctx.batch, ctx.pop, ctx.size, ctx.channels = env._batch_struct(), pop, (R, W, H, L), (K, M)
        ctx.drop = None if drop is None else (drop.p, drop.seed, drop.seed_stride, drop.step)
        m = _BatchedSense._medium(ctx, planes)
        layers, nca = pop._nca_batch(parameters.data_ptr(), ctx.epoch)
        name = _SENSE_CALLS[_sense_kind(pop, K, M)][0]
        _lib.check(getattr(_lib.lib, name)(C.byref(m), C.byref(ctx.batch), C.byref(nca), _ptr(store), store.numel() * 4,
                                           None if masked is None else _ptr(masked), None if drop is None else C.byref(drop),
                                           *_state_planes(K, M, field, state[-1] if M else None), stream_ptr(dev)), name)
        # everything the backward reads goes through save_for_backward: freed with the graph after a backward without retain_graph
        ctx.save_for_backward(parameters, store, *state, *planes)
        return (store[L - 1] if masked is None else masked)[:, :3 + K + M]

    @staticmethod
    def _medium(ctx, planes) -> _lib.Medium:
        R, W, H, _ = ctx.size
        owner = _ptr(planes[2]) if len(planes) == 3 else None
        return _lib.Medium(W, H, ctx.fdt, ctx.epoch, owner, _ptr(planes[0]), _ptr(planes[1]), None, 0, 0, 0, 0, 0, 0, 0, 0, None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (K, M), (R, W, H, L) = ctx.channels, ctx.size
        parameters, store, *planes = ctx.saved_tensors
        field = planes.pop(0) if K else None
        mem_planes = planes.pop(0) if M else None
        pop, dev = ctx.pop, store.device
        kind = _sense_kind(pop, K, M)
        _, query, name = _SENSE_CALLS[kind]
        state = _state_planes(K, M, field, mem_planes)
        g = grad.to(dtype=torch.float32).contiguous()               # (R, 3 + K + M, W, H)
        m = _BatchedSense._medium(ctx, planes)
        layers, nca = pop._nca_batch(parameters.data_ptr(), ctx.epoch)
        need = int(getattr(_lib.lib, query)(W, H, R, L if kind == 'narrow' else C.byref(nca), *state[1::2]))
        if need < 0:
            raise ValueError(f'a stack or shape {name} does not take')
        ws = torch.empty((need // 4,), dtype=torch.float32, device=dev)
        out = torch.empty_like(parameters)                          # (C, P): every element is written (the layers tile a row)
        drop = None if ctx.drop is None else _lib.NcaDropout(*ctx.drop, 0)
        args = (C.byref(m), C.byref(ctx.batch), C.byref(nca), _ptr(store), _ptr(g), (3 + K + M) * W * H, _ptr(out), pop.P,
                None if drop is None else C.byref(drop), _ptr(ws), need)
        # the first layer's inputs are ([agents,] food, chem, signal_0 .., memory_0 ..): food and the claims are constants of the
        # parameters, chem is the env's node, the signal planes the incoming field, the memory planes the expand's output; with none
        # of them asking for a gradient (no node, or a leaf that asks for nothing) no input gradient is computed
        to_node, to_field, to_memory = ctx.needs_input_grad[2:5]
        first = len(planes)                                         # the signal planes' first channel
        cin = first + K + M
        grad_in = torch.empty((R, cin, W, H), dtype=torch.float32, device=dev) if to_node or to_field or to_memory else None
        if kind != 'narrow':                        # one call, `grad_in` nullable
            args += (_ptr(grad_in), cin * W * H, *state)
        elif grad_in is not None:
            name, args = 'die_nca_backward_batch_inputs', args + (_ptr(grad_in), cin * W * H)
        _lib.check(getattr(_lib.lib, name)(*args, stream_ptr(dev)), name)
        return (None, out, grad_in[:, first - 1] if to_node else None,
                grad_in[:, first:first + K].permute(1, 0, 2, 3) if to_field else None,
                grad_in[:, first + K:].permute(1, 0, 2, 3) if to_memory else None)


class _BatchedReadOut(torch.autograd.Function):
    """BatchedNeuralAutomataAgent.differentiable_action's last step: die_gather_scale_batch, die_gather_scale_backward_batch."""

    @staticmethod
    def forward(ctx, sense, pop):
        env = pop.env
        R, W, H, dev = env.R, env.W, env.H, env.device
        if sense.stride()[1:] != (W * H, H, 1) or sense.stride(0) < 3 * W * H:
            sense = sense.contiguous()
        out = torch.empty((3, R, env.Nmax), dtype=torch.float32, device=dev)
        x, y = env.x.clone(), env.y.clone()                          # where the slots stand now: the worlds will be stepped
        ctx.m, ctx.batch, ctx.coefs, ctx.size = _geometry(env), env._batch_struct(), tuple(pop.template.action_coefs), (R, W, H, env.Nmax)
        a = _lib.Agents(env.Nmax, _ptr(x), _ptr(y), None, None, None)
        u = _lib.Action(env.Nmax, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        _lib.check(_lib.lib.die_gather_scale_batch(C.byref(ctx.m), C.byref(a), C.byref(ctx.batch), sense.data_ptr(), sense.stride(0),
                                                   (C.c_float * 3)(*ctx.coefs), C.byref(u), stream_ptr(dev)), 'die_gather_scale_batch')
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y = ctx.saved_tensors
        R, W, H, Nmax = ctx.size
        g = grad.to(dtype=torch.float32).contiguous()
        planes = torch.empty((R, 3, W, H), dtype=torch.float32, device=x.device)     # (cleared by the call)
        a = _lib.Agents(Nmax, _ptr(x), _ptr(y), None, None, None)
        u = _lib.Action(Nmax, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr())
        _lib.check(_lib.lib.die_gather_scale_backward_batch(C.byref(ctx.m), C.byref(a), C.byref(ctx.batch), C.byref(u),
                                                            (C.c_float * 3)(*ctx.coefs), _ptr(planes), 3 * W * H, stream_ptr(x.device)),
                   'die_gather_scale_backward_batch')
        return planes, None


class _BatchedRecurrentReadOut(torch.autograd.Function):
    """BatchedNeuralAutomataAgent.recurrent_action's last step, ONE node for both read-outs of the (R, 3 + M, W, H) sense planes:
    die_gather_scale_batch on planes 0..2 and the record's gather on planes 3.. forward; backward one (R, 3 + M, W, H) buffer that
    the two scatters clear and fill between them (die_gather_scale_backward_batch, then die_gather_memory_backward_batch) — the
    gradient at the sense planes is assembled where the stack's adjoint reads it, no slicing or padding in between."""

    @staticmethod
    def forward(ctx, sense, pop, record):
        from .functional import _index_gather_batch
        env = pop.env
        R, W, H, dev, M = env.R, env.W, env.H, env.device, pop._memory_channels
        if sense.stride()[1:] != (W * H, H, 1) or sense.stride(0) < (3 + M) * W * H:
            sense = sense.contiguous()
        action = torch.empty((3, R, env.Nmax), dtype=torch.float32, device=dev)
        x, y = env.x.clone(), env.y.clone()                          # where the slots stand now: the worlds will be stepped
        ctx.m, ctx.batch, ctx.coefs = _geometry(env), env._batch_struct(), tuple(pop.template.action_coefs)
        ctx.size, ctx.record = (R, W, H, env.Nmax, M), record
        a = _lib.Agents(env.Nmax, _ptr(x), _ptr(y), None, None, None)
        u = _lib.Action(env.Nmax, action[0].data_ptr(), action[1].data_ptr(), action[2].data_ptr())
        _lib.check(_lib.lib.die_gather_scale_batch(C.byref(ctx.m), C.byref(a), C.byref(ctx.batch), sense.data_ptr(), sense.stride(0),
                                                   (C.c_float * 3)(*ctx.coefs), C.byref(u), stream_ptr(dev)), 'die_gather_scale_batch')
        memory_next = _index_gather_batch(record, record.cell, sense[:, 3:], W * H, sense.stride(0), M)
        ctx.save_for_backward(x, y)
        return action, memory_next

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_action, grad_memory):
        x, y = ctx.saved_tensors
        R, W, H, Nmax, M = ctx.size
        r, dev = ctx.record, x.device
        ga = grad_action.to(dtype=torch.float32).contiguous()
        gm = grad_memory.to(dtype=torch.float32).contiguous()
        planes = torch.empty((R, 3 + M, W, H), dtype=torch.float32, device=dev)      # (cleared by the two calls between them)
        stride = (3 + M) * W * H
        a = _lib.Agents(Nmax, _ptr(x), _ptr(y), None, None, None)
        u = _lib.Action(Nmax, ga[0].data_ptr(), ga[1].data_ptr(), ga[2].data_ptr())
        sp = stream_ptr(dev)
        # (the first call clears from its first plane to its last, the memory planes of all replicas but the last among them; the
        # second clears its own M planes of every replica: in this order nothing either adds is wiped)
        _lib.check(_lib.lib.die_gather_scale_backward_batch(C.byref(ctx.m), C.byref(a), C.byref(ctx.batch), C.byref(u),
                                                            (C.c_float * 3)(*ctx.coefs), _ptr(planes), stride, sp),
                   'die_gather_scale_backward_batch')
        _lib.check(_lib.lib.die_gather_memory_backward_batch(W, H, M, C.byref(r._batch), _ptr(r.cell), _ptr(gm), Nmax,
                                                             planes[:, 3:].data_ptr(), W * H, stride, sp), 'die_gather_memory_backward_batch')
        return planes, None, None
