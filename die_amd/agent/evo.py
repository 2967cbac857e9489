"""NeuralAutomataAgent / ConvolutionModel (reference core/agent/evo.py:18-209): same constructor arguments,
`forward(obs) -> action`, `render()`, `save` / `load`.  The model stays a torch `nn.Module` (its parameters are what the
evolution loop of examples/learning_agents.py edits); `NeuralAutomataAgent.forward` — medium → conv stack → tanh →
per-agent read-out → scaled action — runs on the device through libdie_hip.so (`die_conv2d_circular`,
`die_gather_scale`) on the medium's own planes: no host copy of the field, no torch op on the path."""
import ctypes as C
import io
import os
from abc import abstractmethod
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np
import torch as th
from torch import nn

from .. import _lib
from ..base_types import DataChannels
from ..device_array import DeviceAction, _ptr, stream_ptr
from .base import Agent, save_args


_CHECKPOINT_KEYS = ('params_dict', 'model_state')      # the layout of a saved agent (core/agent/evo.py:24-42): kept, so that files interchange


def _omit_defaults(params: Dict[str, Any], *names: str) -> None:
    """Takes the named constructor arguments out of `params` (an `init_params` dict) while they are at their default — None, 0 or
    False: the arguments the reference does not have, so that a saved agent without them stays loadable by the reference."""
    for name in names:
        if name in params and not params[name]:
            del params[name]


_SIGNAL_ARGUMENTS = ('signal_channels', 'signal_deposit', 'signal_sigma', 'signal_decay')
SIGNAL_MAX_RADIUS = 8                                      # die_signal_step takes die_diffuse_decay's radii


def signal_radius(sigma: float) -> int:
    """The gaussian's radius as the library computes it from the float32 sigma (scipy's int(truncate * sigma + .5), truncate 4)."""
    return int(4.0 * float(np.float32(sigma)) + 0.5)


def _signal_arguments(channels, deposit, sigma, decay):
    """NeuralAutomataAgent's four signal arguments, checked: (K, (deposit, sigma, decay)) or the ValueError that says which is wrong."""
    if channels is None:
        channels = 0
    if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, float, np.integer, np.floating)) or \
            int(channels) != channels or not 0 <= channels <= _lib.SIGNAL_MAX_CHANNELS:
        raise ValueError(f'signal_channels={channels!r}: an integer in 1..{_lib.SIGNAL_MAX_CHANNELS}, or 0 / None for none')
    try:
        deposit, sigma, decay = float(deposit), float(sigma), float(decay)
    except (TypeError, ValueError):
        raise ValueError(f'signal_deposit={deposit!r}, signal_sigma={sigma!r}, signal_decay={decay!r}: three numbers') from None
    if not np.isfinite(deposit):
        raise ValueError(f'signal_deposit={deposit!r}: a finite number')
    if not (np.isfinite(sigma) and sigma > 0 and 1 <= signal_radius(sigma) <= SIGNAL_MAX_RADIUS):
        raise ValueError(f'signal_sigma={sigma!r}: its radius int(4 sigma + .5) must lie in 1..{SIGNAL_MAX_RADIUS}')
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f'signal_decay={decay!r}: a number in [0, 1]')
    return int(channels), (deposit, sigma, decay)


_HEREDITY_ARGUMENTS = ('memory_inherit', 'memory_mutation')


def _heredity_arguments(mode, mutation, memory_channels: int):
    """NeuralAutomataAgent's two heredity arguments, checked: (mode or None, mutation as a float) or the ValueError that says which is
    wrong — a mode other than 'blank' / 'copy', a mutation that is no finite float >= 0 or comes without 'copy', either without
    memory channels."""
    from ..functional import inherit_arguments
    if mode is None:
        inherit_arguments('copy', mutation, 'NeuralAutomataAgent')          # (a bad number is a bad number whatever the mode)
        if float(mutation) != 0.0:
            raise ValueError(f"memory_mutation={mutation!r} needs memory_inherit='copy'")
        return None, 0.0
    mode, mutation = inherit_arguments(mode, mutation, 'NeuralAutomataAgent')
    if not memory_channels:
        raise ValueError(f'memory_inherit={mode!r} without memory channels (memory_channels=0): there is nothing to inherit')
    return mode, mutation


def check_given(what: str, name: str, t, want: tuple, device) -> None:
    """A `signals` or `memory` tensor handed to `recurrent_action` / `signalling_action` (the agent's and the population's), or
    the ValueError that says what it must be and what it got."""
    if not isinstance(t, th.Tensor) or t.dtype != th.float32 or tuple(t.shape) != want or t.device != device:
        got = (tuple(t.shape), t.dtype, str(t.device)) if isinstance(t, th.Tensor) else type(t).__name__
        raise ValueError(f'{what}: {name} must be a {want} float32 tensor on {device}, got {got}')


def _layer_arrays(li: int, w: th.Tensor, planes, dst: th.Tensor):
    """What a narrow layer launch takes beside its weights `w`: the input `planes` [(tensor, DIE_PLANE_* kind)] as a die_conv_plane
    array and the first cout planes of `dst` as a pointer array — or the ValueError of a weight that does not fit the planes."""
    cout, cin, k, k2 = w.shape
    if k != k2 or cin != len(planes):
        raise ValueError(f'layer {li}: weight {tuple(w.shape)} does not fit {len(planes)} input planes')
    return ((_lib.ConvPlane * cin)(*[_lib.ConvPlane(t.data_ptr(), kind, 0) for t, kind in planes]),
            (C.c_void_p * cout)(*[dst[o].data_ptr() for o in range(cout)]))


class TorchAgent(Agent, nn.Module):
    """An agent whose behaviour is a torch model (core/agent/evo.py:18-42): `save` writes the constructor arguments and the
    model's state_dict under the reference's two keys, `load` rebuilds the agent from them."""

    @property
    @abstractmethod
    def model(self) -> nn.Module:
        """The module whose parameters the evolution loop edits."""

    def save(self, file: Union[str, os.PathLike, io.IOBase]):
        th.save(dict(zip(_CHECKPOINT_KEYS, (self.init_params, self.model.state_dict()))), file)

    @classmethod
    def load(cls, file: Union[str, os.PathLike, io.IOBase]):
        loaded = th.load(file)                                         # ONE read: `file` may be a stream
        ctor_args, weights = (loaded[k] for k in _CHECKPOINT_KEYS)
        ctor_args = dict(ctor_args)
        ctor_args.update(ctor_args.pop('model_kwargs', {}))            # **model_kwargs of NeuralAutomataAgent are stored nested
        restored = cls(**ctor_args)
        restored.model.load_state_dict(weights)
        return restored


class ConvolutionModel(nn.Module):
    """The perception model of core/agent/evo.py:45-118: a stack of bias-free 'same'-padded Conv2d layers (one per entry of
    `kernel_sizes`; every layer keeps the observation channels except the last, which maps them to the action channels), a Tanh
    that brings the outputs into [-1, 1], and an (inverted-)dropout mask over cells.  The submodule names `kernels.<i>` and
    `agent_dropout` are the reference's, so state_dicts interchange; the device path (NeuralAutomataAgent.sense) reads the
    layers' weights and never calls this module's forward.

    `hidden_channels` and `hidden_activation` (no reference counterpart; both None: exactly the module above) make a "wide stack":
      * `hidden_channels=C`, 1 <= C <= 32: the layers are obs -> C, C -> C, ..., C -> actions (at least two layers);
      * `hidden_activation` 'tanh' / 'relu' / None: applied after every layer but the last, as a module between the convs (the
        convs' names `kernels.<i>` then skip the activations' indices); the last layer keeps the Tanh and the dropout mask.
    A stack with either one set runs on the device through the wide layer kernel (die_conv2d_wide: kernel sizes 1, 3 and 5, every
    boundary), also where its widths would fit the narrow one.  Both stay out of `init_params` while None.

    `memory_channels=M` > 0 (NeuralAutomataAgent(memory_channels=M), which also counts the M planes into `num_obs_channels` and
    `num_act_channels`): the stack is a wide stack whatever the two arguments above say — a single layer obs -> actions included
    — and `forward_device` refuses it: the planes alone do not say whose memory they hold, its gradients come from
    `NeuralAutomataAgent.recurrent_action`.  Kept out of `init_params` while 0.

    `signal_channels=K` > 0 (NeuralAutomataAgent(signal_channels=K), which counts the K planes into `num_obs_channels` and
    `num_act_channels` as well): a wide stack too, whatever else is set, and `forward_device` refuses it — the field's update has no
    adjoint.  Kept out of `init_params` while 0."""

    def __init__(self,
                 num_obs_channels: int = 3,
                 num_act_channels: int = 3,
                 kernel_sizes: Sequence[int] = (3,),
                 boundary: str = 'circular',
                 p_agent_dropout: float = 0.,
                 requires_grad: bool = True,
                 hidden_channels: Optional[int] = None,
                 hidden_activation: Optional[str] = None,
                 memory_channels: int = 0,
                 signal_channels: int = 0,
                 ):
        self._init_params = save_args(self.__init__, locals())
        _omit_defaults(self._init_params, 'hidden_channels', 'hidden_activation', 'memory_channels', 'signal_channels')
        if hidden_channels is not None:
            if isinstance(hidden_channels, bool) or int(hidden_channels) != hidden_channels or \
                    not 1 <= hidden_channels <= _lib.NCA_WIDE_MAX_CHANNELS:
                raise ValueError(f'hidden_channels={hidden_channels!r}: an integer in 1..{_lib.NCA_WIDE_MAX_CHANNELS}, or None')
            if len(kernel_sizes) < 2:
                raise ValueError('hidden_channels needs at least two layers (a single layer has no hidden channels)')
            hidden_channels = int(hidden_channels)
        if hidden_activation not in _lib.NCA_ACTIVATIONS:
            raise ValueError(f"hidden_activation={hidden_activation!r}: 'tanh', 'relu' or None")
        if hidden_channels is not None or hidden_activation is not None or memory_channels or signal_channels:
            for size in kernel_sizes:
                if size not in _lib.NCA_WIDE_KERNEL_SIZES:
                    raise NotImplementedError(f'kernel size {size} in a wide stack (hidden_channels / hidden_activation / '
                                              f'memory_channels): one of {_lib.NCA_WIDE_KERNEL_SIZES} (32 * 32 * 49 weights do not fit '
                                              'LDS next to a tile)')
        if (memory_channels or signal_channels) and max(num_obs_channels, num_act_channels) > _lib.NCA_WIDE_MAX_CHANNELS:
            raise ValueError(f'{num_obs_channels} -> {num_act_channels} channels: at most {_lib.NCA_WIDE_MAX_CHANNELS} a layer')
        super().__init__()
        self.hidden_channels, self.hidden_activation = hidden_channels, hidden_activation
        self.memory_channels = int(memory_channels)
        self.signal_channels = int(signal_channels)
        depth = len(kernel_sizes)
        width = num_obs_channels if hidden_channels is None else hidden_channels
        stack = nn.Sequential()
        for level, size in enumerate(kernel_sizes):
            widens_to_actions = level == depth - 1
            stack.append(nn.Conv2d(num_obs_channels if level == 0 else width, num_act_channels if widens_to_actions else width, size,
                                   padding='same', padding_mode=boundary, bias=False))
            if hidden_activation is not None and not widens_to_actions:
                stack.append(nn.Tanh() if hidden_activation == 'tanh' else nn.ReLU())
        stack.append(nn.Tanh())
        self.agent_dropout = nn.Dropout(p_agent_dropout)
        self.kernels = stack
        self.requires_grad_(requires_grad)

    @property
    def wide(self) -> bool:
        """A stack with `hidden_channels`, `hidden_activation`, `memory_channels` or `signal_channels` set: every layer goes through the
        wide entry points."""
        return self.hidden_channels is not None or self.hidden_activation is not None or self.memory_channels > 0 or self.signal_channels > 0

    def conv_layers(self):
        return [layer for layer in self.kernels if isinstance(layer, nn.Conv2d)]

    def init_weights(self):
        for layer in self.conv_layers():
            nn.init.xavier_uniform_(layer.weight)

    def forward(self, input: th.Tensor) -> th.Tensor:
        """The torch evaluation (what the reference runs; here the fp32 reference of the device path in tests, and for callers
        that hold plain tensors): the cells' dropout mask is drawn on the field's own device."""
        keep = self.agent_dropout(th.ones(input.shape[-2:], device=input.device, dtype=input.dtype))
        return self.kernels(input) * keep

    def forward_device(self, planes: th.Tensor, dropout=None) -> th.Tensor:
        """A wide stack on the device, differentiable: `planes` (num_obs_channels, W, H), float32 on a GPU -> (num_act_channels, W,
        H) with a `grad_fn`.  Every layer is one `die_amd.functional.conv2d_wide` (die_conv2d_wide forward, die_conv2d_wide_backward
        backward): the hidden activation after every layer but the last, Tanh and the optional mask `dropout` = (p, seed, step) —
        the counter-based mask of `NeuralAutomataAgent(dropout_seed=seed)` at `dropout_step` = step — after the last.  The weights
        reach the device by a differentiable `.to()`, so gradients land in `parameters()` wherever the model lives.  The values are
        bit for bit what `NeuralAutomataAgent.sense` returns on a medium holding those planes: the same launches.  Boundaries
        'circular' and 'zeros' where a gradient is needed.  A narrow model (neither `hidden_channels` nor `hidden_activation`)
        raises ValueError: it has `NeuralAutomataAgent.differentiable_sense`."""
        if self.signal_channels:
            raise NotImplementedError(f'forward_device: no gradients through signal channels (signal_channels={self.signal_channels}): '
                                      'the field\'s update has no adjoint')
        if self.memory_channels:
            raise NotImplementedError('forward_device: no gradients through memory channels (memory_channels > 0): the read-out into '
                                      'the memory and the expand onto the field have no adjoint')
        if not self.wide:
            raise ValueError('forward_device: a narrow model (hidden_channels and hidden_activation both None) is differentiated by '
                             'NeuralAutomataAgent.differentiable_sense')
        return self._stack_device(planes, dropout)

    def _stack_device(self, planes: th.Tensor, dropout=None) -> th.Tensor:
        """`forward_device`'s layers, for the callers that have made their own refusals (`forward_device`, and
        `NeuralAutomataAgent.recurrent_action` for a stack with memory channels)."""
        from ..functional import conv2d_wide
        layers = self.conv_layers()
        out = planes
        for li, layer in enumerate(layers):
            last = li == len(layers) - 1
            weight = layer.weight.to(device=planes.device, dtype=th.float32).contiguous()
            out = conv2d_wide(out, weight, activation='tanh' if last else self.hidden_activation, padding_mode=layer.padding_mode,
                              dropout=dropout if last else None)
        return out


class NeuralAutomataAgent(TorchAgent):
    """core/agent/evo.py:121-209.

    `dropout_seed` (no reference counterpart) chooses where the mask of `p_agent_dropout` comes from in training mode:
      * None (default): a torch-RNG `nn.Dropout` multiply after the device layers, as the reference draws it — not
        reproducible per call;
      * an int: the counter-based mask of include/die_hip.h (die_nca_dropout), a pure function of (dropout_seed, `dropout_step`,
        cell), applied inside the last layer's launch (`die_conv2d_dropout`).  `dropout_step` is the forward-call counter: it
        starts at 0, every `sense` advances it by one, and it may be read and written (setting it back replays the masks).
    It is kept out of `init_params` while None, so saved files stay loadable by the reference.

    `with_stock_channel` (no reference counterpart; core/agent/evo.py leaves it as "TODO: agents should have access to their own
    resource stock"): True appends a last observation channel `'agent_food'` — a (W, H) float32 plane holding, on every cell, the
    `agent_food` of the agent standing there as `sense` finds the agents (after the previous step's feed, deaths and births):
    alive slots only, the highest slot id where several share a cell, 0 elsewhere, negative stocks kept.  The
    first channels of `kernels.0.weight` keep their meaning.  `sense(medium, agents)` then needs the agents (ValueError before any
    launch without them; `forward(obs)` passes its own), builds the plane on the device (die_stock_plane at `medium.epoch`, one
    launch more) and hands it to the first layer as DIE_PLANE_STOCK.  The agent owns one stock plane per (W, H, device), zeroed
    when it is allocated and whenever `medium.epoch` is not greater than the epoch of its last build on it.  Narrow and wide
    stacks, fp16 fields, every boundary, both dropout masks and tile-binned worlds take it.  Refused with the channel on, each
    with NotImplementedError before any launch and before `dropout_step` moves: `differentiable_sense` and
    `differentiable_action` (the plane is piecewise constant in the weights and the adjoint calls do not take its kind), and a
    decomposed medium (die_amd/dist.py).  Kept out of `init_params` while False, saved and restored by `load` while True.

    `memory_channels=M`, 1 <= M <= 8 (no reference counterpart; core/agent/learning.py: "TODO: need joint channels info for the
    system"; 0 / None: absent, nothing changes): every agent carries M values from one forward to the next.
      * The stack is a wide stack (die_conv2d_wide: kernel sizes 1, 3, 5; `hidden_channels` None: hidden layers as wide as the
        observation; a single layer obs -> 3 + M is allowed).  The observation channels are `[agents]`, `env_food`, `chem1`,
        `memory_0` .. `memory_{M-1}`, `[agent_food]` — the stock plane stays last — and `kernels.0.weight` has that many input
        channels in that order.  The last layer has 3 + M output channels: rows 0..2 are dx, dy, deposit as ever, rows 3.. the new
        memory; the last layer's tanh and the dropout mask apply to every one of them (a masked cell yields memory 0).
        `render()` keeps showing the first three planes.
      * `memory`: the (M, N) float32 device tensor, indexed by SLOT ID (`agents.slot[i]` where a slot array exists, else the
        storage index), so it follows an agent through every re-sort.  None until the first `sense` / `forward`, which allocates
        it as zeros for `agents.N` slots; it may be assigned (a contiguous (M, N) float32 tensor on the medium's device).
        `reset_memory()` zeroes it and lets the next forward take another N; until then a forward with a different N raises
        ValueError before any launch.
      * One `forward(obs)`: the standing plane (die_stock_plane at `medium.epoch`: alive slots only, the highest slot id on a
        shared cell — the stock channel's own plane, one build for both) is expanded into M fp32 planes `P_j[c] = memory[j][winner
        of c]`, 0 on empty cells (die_memory_planes); the stack runs; `die_gather_scale` reads planes 0..2 into the action; and
        die_gather_memory writes `memory[j][slot] = S[3 + j][cell of the slot]` for alive slots, +0 for dead ones (no
        coefficient; a slot's next occupant starts blank; two agents sharing a cell get the same memory).  `sense(medium, agents)`
        needs the agents (ValueError before any launch without them) and returns all 3 + M planes; `memory_planes(medium, agents)`
        gives the M planes the coming forward would sense.
      * Gradients: `recurrent_action(obs, memory=None) -> (action, memory_next)` is `forward` with a graph through the read-out,
        the stack and the expand (die_memory_grad.hip); chaining `memory_next` is backpropagation through time.  Not for
        populations, the stock channel, fp16 fields or decomposed worlds.
      * Refused with NotImplementedError before any launch, and before `dropout_step` or `memory` change: the memoryless
        `differentiable_sense`, `differentiable_action`, `model.forward_device`, and a decomposed medium (die_amd/dist.py).
        `Dynamics(agents_born=True)` is refused together with memory too while no rule of inheritance is set (`memory_inherit`
        None: a slot can die and be refilled within one step, so a newborn would inherit a dead agent's memory) — but a
        stand-alone agent cannot see the Dynamics, so that refusal sits where the Dynamics is known: the
        `BatchedNeuralAutomataAgent` constructor.  With a stand-alone `Env` it is the caller's.
      * Heredity: `memory_inherit` 'blank' / 'copy' (None: no rule, nothing changes) and `memory_mutation` = a >= 0 (only with
        'copy') say what a newborn's memory holds under `Dynamics(agents_born=True)`.  After a step's birth pass
        has matched parent p to free slot f, and on the memory as this step's read-out left it: 'blank' `memory[m][f] = +0`;
        'copy' `memory[m][f] = memory[m][p]`, bits preserved; 'copy' with a > 0 the parent's value plus `a * u`, u uniform in
        [-1, 1] from the births' own Philox key and step on a stream of its own (two separately rounded fp32 operations).  The
        parent keeps its memory, every other slot is left alone (die_memory_inherit, one launch).  With a rule `forward(obs)`
        marks the action it returns, and `Env.step` hands the record of its birth pass (`env.births_record()`) to
        `inherit_memory`: `env.step(agent.forward(obs))` and `Env.run(agent, n)` inherit without a further call; a refilled slot's
        memory is always overwritten, so the refusal above is gone.  Both arguments are kept out of `init_params` while the mode
        is None and are saved and restored otherwise.  ValueError in the constructor: another mode, a mutation that is negative,
        not finite or no number, a mutation with 'blank', either argument without memory channels.
    Kept out of `init_params` while 0, saved and restored by `load` while positive (the memory itself is state, not saved).

    `signal_channels=K`, 1 <= K <= 8, with `signal_deposit`, `signal_sigma`, `signal_decay` (no reference counterpart; core/__init__.py
    of the reference: "abstracted actionable channels: let the medium have channels rgbc, and enable the Agent to sense 'rgb' and to
    act on 'g' and 'c'"; 0 / None: absent, nothing changes): the agents write and read a field of K planes that stays where it was
    written, diffuses and decays — memory's public counterpart.
      * A wide stack, as with memory.  The observation channels are `[agents]`, `env_food`, `chem1`, `signal_0` .. `signal_{K-1}`,
        `memory_0` .. `memory_{M-1}`, `[agent_food]`; the last layer has 3 + K + M output channels: rows 0..2 dx, dy, deposit, rows
        3 .. 3 + K - 1 the emissions, then the memory rows.  Tanh and the dropout mask fall on every plane (a masked cell emits 0).
      * `signals`: the (K, W, H) float32 device tensor, whatever the field's dtype; None until the first `sense` / `forward`, which
        allocates it as zeros for the medium's (W, H, device).  `reset_signals()` zeroes it and lets the next forward take another
        shape; until then a forward on a medium of another shape raises ValueError before any launch.
      * One `forward(obs)`: the stack reads F_k as plain fp32 planes; actions and the memory read-out as ever; then die_signal_step:
        `E_k[c] = occupied(c) ? signal_deposit * S[3 + k][c] : +0` on the standing plane's cells (alive slots only — the stock and
        memory build, one for all three; agents sharing a cell emit once; emissions may be negative, so agents can erase) and
        `F_k <- (1 - signal_decay) * gaussian(F_k + E_k, signal_sigma, mode='wrap', truncate=4)` in fp32, into a second buffer that
        is then swapped.  `sense()` alone leaves the field untouched: its clock is the agent's forward count, as memory's is.
        Signalling is free of action cost.
      * Gradients: `signalling_action(obs, signals=None, memory=None) -> (action, signals_next, memory_next)` is `forward` with a
        graph through the read-outs, the stack and the field's update (die_signal_grad.hip); chaining `signals_next` is
        backpropagation through time through the field.  Not for populations, the stock channel, fp16 fields or decomposed worlds.
      * Refused with NotImplementedError before any launch, and before `dropout_step`, `memory` or `signals` change: the other
        differentiable calls (`differentiable_sense`, `differentiable_action`, `model.forward_device`, `recurrent_action`) and a
        decomposed medium.  `signal_sigma` must give a radius int(4 sigma + .5) in 1..8, `signal_decay` lie in [0, 1],
        `signal_deposit` be finite: ValueError in the constructor.
    All four are kept out of `init_params` while K is 0, saved and restored by `load` while positive (the field is state, not saved)."""

    def __init__(self,
                 scale: float = 0.1,
                 deposit: float = 1.0,
                 with_agent_channel: bool = True,
                 initial_obs=None,
                 dropout_seed: Optional[int] = None,
                 with_stock_channel: bool = False,
                 memory_channels: Optional[int] = 0,
                 signal_channels: Optional[int] = 0,
                 signal_deposit: float = 1.0,
                 signal_sigma: float = 0.5,
                 signal_decay: float = 0.1,
                 memory_inherit: Optional[str] = None,
                 memory_mutation: float = 0.0,
                 **model_kwargs,
                 ):
        self._init_params = save_args(self.__init__, locals())
        self._init_params.pop('initial_obs', None)            # an observation is not a constructor parameter worth saving
        self.signal_channels, self.signal_constants = _signal_arguments(signal_channels, signal_deposit, signal_sigma, signal_decay)
        self.signals: Optional[th.Tensor] = None               # (K, W, H) float32, from the first forward on
        self._signals_next: Optional[th.Tensor] = None         # the second buffer the update writes, swapped in afterwards
        self._signals_rebind = True                            # the next forward may allocate for its own medium
        self._standing: Optional[th.Tensor] = None             # the standing plane of the last sense with agents
        for name, value in zip(_SIGNAL_ARGUMENTS, (self.signal_channels, *self.signal_constants)):
            if self.signal_channels:                           # (saved as the checked values; all four kept out while K is 0)
                self._init_params[name] = value
            else:
                self._init_params.pop(name, None)
        if memory_channels is None:
            memory_channels = 0
        if isinstance(memory_channels, (bool, np.bool_)) or not isinstance(memory_channels, (int, float, np.integer, np.floating)) or \
                int(memory_channels) != memory_channels or not 0 <= memory_channels <= _lib.MEMORY_MAX_CHANNELS:
            raise ValueError(f'memory_channels={memory_channels!r}: an integer in 1..{_lib.MEMORY_MAX_CHANNELS}, or 0 / None for none')
        self.memory_channels = int(memory_channels)
        self.memory_inherit, self.memory_mutation = _heredity_arguments(memory_inherit, memory_mutation, self.memory_channels)
        for name, value in zip(_HEREDITY_ARGUMENTS, (self.memory_inherit, self.memory_mutation)):
            if self.memory_inherit is not None:                # (saved as the checked values; both kept out while the mode is None)
                self._init_params[name] = value
            else:
                self._init_params.pop(name, None)
        self.memory: Optional[th.Tensor] = None                # (M, N) float32 by slot id, from the first forward on
        self._memory_rebind = True                             # the next forward may allocate for its own N
        self._memory_planes = {}                               # (W, H, device) -> (M, W, H) float32: the expanded memory
        if not isinstance(with_stock_channel, (bool, np.bool_)):
            raise ValueError(f'with_stock_channel={with_stock_channel!r}: True or False')
        self.with_stock_channel = bool(with_stock_channel)
        # (saved as the checked values; kept out while at their defaults, as dropout_seed is while None: see ConvolutionModel)
        self._init_params.update(memory_channels=self.memory_channels, with_stock_channel=self.with_stock_channel)
        _omit_defaults(self._init_params, 'memory_channels', 'with_stock_channel')
        _omit_defaults(self._init_params['model_kwargs'], 'hidden_channels', 'hidden_activation')
        super().__init__()
        self.dropout_seed = dropout_seed
        self.dropout_step = 0
        self.obs_channels = list(DataChannels.medium) if with_agent_channel else list(DataChannels.medium[1:])
        self.obs_channels += [f'signal_{k}' for k in range(self.signal_channels)]      # after the field's planes, before the memory's
        self.obs_channels += [f'memory_{j}' for j in range(self.memory_channels)]      # … which come before the stock's
        if self.with_stock_channel:
            self.obs_channels.append(DataChannels.agents[3])   # 'agent_food': always the LAST observation channel
        self._stock = {}                                       # (W, H, device) -> [uint64 stock plane, epoch of its last build]
        if self.memory_channels:                               # (a model without memory is built exactly as before)
            model_kwargs = dict(model_kwargs, memory_channels=self.memory_channels)
        if self.signal_channels:                               # (nor does a model without signals say anything about them)
            model_kwargs = dict(model_kwargs, signal_channels=self.signal_channels)
        self._model = ConvolutionModel(num_obs_channels=len(self.obs_channels),
                                       num_act_channels=len(DataChannels.actions) + self.signal_channels + self.memory_channels,
                                       **model_kwargs)
        self.action_coefs = (float(scale), float(scale), float(deposit))
        self._sense_output: Optional[th.Tensor] = None         # (3, W, H) on the device after the first forward
        self._planes = {}                                      # device scratch by (W, H, device): ping-pong plane sets

    @property
    def model(self) -> ConvolutionModel:
        return self._model

    @property
    def init_params(self) -> Dict[str, Any]:
        return self._init_params

    @property
    def dropout_seed(self) -> Optional[int]:
        return self._dropout_seed

    @dropout_seed.setter
    def dropout_seed(self, seed: Optional[int]):
        if seed is not None and (isinstance(seed, bool) or int(seed) != seed):
            raise ValueError(f'dropout_seed={seed!r}: an integer, or None for the torch-RNG mask')
        self._dropout_seed = None if seed is None else int(seed)
        if seed is None:
            self._init_params.pop('dropout_seed', None)
        else:
            self._init_params['dropout_seed'] = self._dropout_seed

    # ------------------------------------------------------------------
    def _device_weights(self, device):
        layers = self._model.conv_layers()
        for k in layers:
            if k.padding_mode not in _lib.PAD_MODES:
                raise NotImplementedError(f"boundary={k.padding_mode!r}: one of {sorted(_lib.PAD_MODES)}")
        # uploaded on every call (≈ 100 floats): in-place writes through `param.data` — how evotorch's fill_parameters
        # loads each candidate — change neither `_version` nor `data_ptr()`, so no cheap key tells a stale copy apart
        return [k.weight.detach().to(device=device, dtype=th.float32).contiguous() for k in layers]

    def _scratch(self, W, H, device, n_sets, channels=4):
        key = (W, H, str(device))
        sets = self._planes.get(key)
        if sets is None or len(sets) < n_sets or sets[0].shape[0] < channels:
            sets = [th.empty((channels, W, H), dtype=th.float32, device=device) for _ in range(n_sets)]
            self._planes[key] = sets
        return sets

    def _check_wide(self, what: str = None):
        """A wide stack's refusals, before any launch: a kernel size the wide layer kernel does not take, or (`what`) a
        differentiable call."""
        if not self._model.wide:
            return
        if what is not None:
            raise NotImplementedError(f'{what}: no gradients for a wide stack (hidden_channels / hidden_activation): the adjoint '
                                      'kernels take the narrow layers only')
        for k in self._model.conv_layers():
            if int(k.kernel_size[0]) not in _lib.NCA_WIDE_KERNEL_SIZES:
                raise NotImplementedError(f'kernel size {int(k.kernel_size[0])} in a wide stack (hidden_channels / hidden_activation): '
                                          f'one of {_lib.NCA_WIDE_KERNEL_SIZES} (32 * 32 * 49 weights do not fit LDS next to a tile)')

    def _check_stock(self, what: str = None, medium=None):
        """The stock channel's refusals, before any launch: (`what`) a differentiable call, (`medium`) a decomposed world."""
        if not self.with_stock_channel:
            return
        if what is not None:
            raise NotImplementedError(f'{what}: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise '
                                      'constant in the weights and the adjoint kernels do not take its kind')
        if medium is not None and getattr(medium, 'world', None) is not None:
            raise NotImplementedError('with_stock_channel=True on a decomposed medium (die_amd/dist.py): the stock plane is built for '
                                      'periodic single-tile planes only')

    def _check_memory(self, what: str = None, medium=None):
        """The memory channels' refusals, before any launch: (`what`) a differentiable call, (`medium`) a decomposed world."""
        if not self.memory_channels:
            return
        if what is not None:
            # (the text is pinned word for word by tests/test_gpu_nca_call_sequence.py; recurrent_action is the call that has the adjoints)
            raise NotImplementedError(f'{what}: no gradients through memory channels (memory_channels={self.memory_channels}): the '
                                      'read-out into the memory and the expand onto the field have no adjoint')
        if medium is not None and getattr(medium, 'world', None) is not None:
            raise NotImplementedError(f'memory_channels={self.memory_channels} on a decomposed medium (die_amd/dist.py): the standing '
                                      'plane is built for periodic single-tile planes only')

    def _check_signals(self, what: str = None, medium=None):
        """The signal channels' refusals, before any launch: (`what`) a differentiable call, (`medium`) a decomposed world, or a
        medium of another shape or device than the field was allocated for (ValueError, until `reset_signals()`)."""
        K = self.signal_channels
        if not K:
            return
        if what is not None:
            raise NotImplementedError(f'{what}: no gradients through signal channels (signal_channels={K}): the field\'s update has '
                                      'no adjoint')
        if medium is None:
            return
        if getattr(medium, 'world', None) is not None:
            raise NotImplementedError(f'signal_channels={K} on a decomposed medium (die_amd/dist.py): the signal field is kept for '
                                      'periodic single-tile planes only')
        sig = self.signals
        if sig is not None and not self._signals_rebind and (tuple(sig.shape) != (K, medium.W, medium.H) or sig.device != medium.device):
            raise ValueError(f'signals holds a {tuple(sig.shape[1:])} field on {sig.device}, the medium is {(medium.W, medium.H)} on '
                             f'{medium.device}: call reset_signals() to start blank on it')

    def reset_signals(self) -> None:
        """A blank field: zero it where it is, and let the next forward allocate anew if its medium has another shape."""
        if self.signals is not None:
            self.signals.zero_()
        self._signals_rebind = True

    def _signals_for(self, medium) -> th.Tensor:
        """`signals` for this medium: allocated as zeros at the first forward (and at the first after `reset_signals()` on a
        medium of another shape), with the second buffer the update writes."""
        shape = (self.signal_channels, medium.W, medium.H)
        sig = self.signals
        if sig is None or tuple(sig.shape) != shape or sig.device != medium.device:
            sig = self.signals = th.zeros(shape, dtype=th.float32, device=medium.device)
        nxt = self._signals_next
        if nxt is None or tuple(nxt.shape) != shape or nxt.device != medium.device:
            self._signals_next = th.empty(shape, dtype=th.float32, device=medium.device)
        self._signals_rebind = False
        return sig

    def _check_differentiable(self, what: str, wide_ok: bool = False):
        """What no differentiable call takes — signal channels, memory channels, a wide stack (unless `wide_ok`: the wide twin,
        BatchedNeuralAutomataAgent.forward_device), the stock channel — refused in that order, before any launch."""
        self._check_signals(what)
        self._check_memory(what)
        if not wide_ok:
            self._check_wide(what)
        self._check_stock(what)

    def _check_boundary(self, prefix: str = ''):
        """The boundaries the adjoint kernels take, before any launch (`prefix`: the caller's name where its texts carry one)."""
        for k in self._model.conv_layers():
            if k.padding_mode not in ('circular', 'zeros'):
                raise NotImplementedError(f"{prefix}boundary={k.padding_mode!r} in differentiable mode: 'circular' or 'zeros' "
                                          f"(sense() and forward() take all of {sorted(_lib.PAD_MODES)})")

    def _field_planes(self, medium) -> Dict[str, Any]:
        """The observation channels the medium itself holds, as first-layer source planes: channel -> (tensor, DIE_PLANE_* kind).
        Under `Dynamics(apply_sense_mask=True)` (`medium.sense_mask` set) the food and chem planes are masked copies, the cells
        outside the mask zeroed (core/env.py:292-298: every agent gets `medium.where(sense_mask, 0)`) — two copies on the cold path.
        The agents channel needs none: an occupied cell is inside the mask by its own weight (w0² ≈ 0.04 against the 0.0005 the
        rounding keeps)."""
        medium._ensure_owner()
        fkind = _lib.DIE_PLANE_F32 if medium.dtype == th.float32 else _lib.DIE_PLANE_F16
        food, chem = medium.food, medium.chem
        mask = getattr(medium, 'sense_mask', None)
        if mask is not None:
            seen = mask != 0
            zero = th.zeros((), dtype=medium.dtype, device=medium.device)
            food, chem = th.where(seen, food, zero), th.where(seen, chem, zero)
        return {'agents': (medium.owner, _lib.DIE_PLANE_AGENTS), 'env_food': (food, fkind), 'chem1': (chem, fkind)}

    @staticmethod
    def _check_sense_mask(what: str, medium):
        """The differentiable calls read the medium unmasked: under a sense mask they are refused before any launch, as
        `Env._check_differentiable` refuses the step."""
        if getattr(medium, 'sense_mask', None) is not None:
            raise NotImplementedError(f'{what}: apply_sense_mask is not differentiable here')

    def _dropout(self) -> Optional[_lib.NcaDropout]:
        """die_nca_dropout of the coming call — the counter-based mask of `dropout_seed` at `dropout_step`, applied inside the last
        layer's launch — or None where nothing is masked that way (no seed, eval mode, p = 0)."""
        model = self._model
        if self._dropout_seed is None or not (model.agent_dropout.p > 0 and model.training):
            return None
        return _lib.nca_dropout(model.agent_dropout.p, self._dropout_seed, 0, self.dropout_step)

    def reset_memory(self) -> None:
        """Blank memory: zero it where it is, and let the next forward allocate anew if its agents have another N."""
        if self.memory is not None:
            self.memory.zero_()
        self._memory_rebind = True

    def _check_memory_slots(self, medium, agents) -> None:
        """What `sense` needs of the agents and of `memory`, before any launch and before anything is allocated."""
        M = self.memory_channels
        if agents is None:
            raise ValueError(f'sense(medium, agents): memory_channels={M} needs the agents whose memory the planes show')
        if getattr(agents, 'global_slots', False):
            raise NotImplementedError(f'memory_channels={M} on a decomposed world (die_amd/dist.py): its slots carry world ids')
        mem = self.memory
        if mem is None:
            return
        if not isinstance(mem, th.Tensor) or mem.dim() != 2 or mem.shape[0] != M or mem.dtype != th.float32 or not mem.is_contiguous() \
                or mem.device != medium.device:
            if self._memory_rebind and isinstance(mem, th.Tensor) and mem.device != medium.device:
                return                                           # reset since: the next forward allocates on this device
            raise ValueError(f'memory: a contiguous ({M}, N) float32 tensor on {medium.device}')
        if mem.shape[1] != agents.N and not self._memory_rebind:
            raise ValueError(f'memory holds {mem.shape[1]} slots, the agents have {agents.N}: call reset_memory() to start blank with them')

    def _memory_for(self, medium, agents) -> th.Tensor:
        """`memory` for these agents: allocated as zeros at the first forward (and at the first after `reset_memory()` with
        another N)."""
        mem = self.memory
        if mem is None or mem.shape[1] != agents.N or mem.device != medium.device:
            mem = self.memory = th.zeros((self.memory_channels, agents.N), dtype=th.float32, device=medium.device)
        self._memory_rebind = False
        return mem

    def memory_planes(self, medium, agents) -> th.Tensor:
        """The (M, W, H) float32 planes a forward would sense now: on every cell the memory of the agent standing there (alive
        slots only, the highest slot id on a shared cell), +0 elsewhere.  Builds the standing plane at `medium.epoch` and expands
        `memory` into planes this agent owns (valid until the next call); allocates `memory` as `sense` does."""
        if not self.memory_channels:
            raise ValueError('memory_planes: an agent without memory channels has none')
        self._check_memory(medium=medium)
        self._check_memory_slots(medium, agents)
        return self._expand_memory(medium, agents, self._stock_plane(medium, agents))

    def _expand_memory(self, medium, agents, standing: th.Tensor) -> th.Tensor:
        dev, W, H, M = medium.device, medium.W, medium.H, self.memory_channels
        mem = self._memory_for(medium, agents)
        key = (W, H, str(dev))
        planes = self._memory_planes.get(key)
        if planes is None:
            planes = self._memory_planes[key] = th.empty((M, W, H), dtype=th.float32, device=dev)
        m = medium.c_struct(need_owner=False)
        _lib.check(_lib.lib.die_memory_planes(C.byref(m), _ptr(standing), medium.epoch, M, _ptr(mem), max(agents.N, 1), agents.N,
                                              _ptr(planes), W * H, stream_ptr(dev)), 'die_memory_planes')
        return planes

    def _stock_plane(self, medium, agents) -> th.Tensor:
        """The agents' stocks on their cells, built at `medium.epoch` on the plane this agent owns for (W, H, device)."""
        dev, W, H = medium.device, medium.W, medium.H
        key = (W, H, str(dev))
        entry = self._stock.get(key)
        if entry is None:
            entry = self._stock[key] = [th.zeros((W, H), dtype=th.int64, device=dev), medium.epoch]
        elif medium.epoch <= entry[1]:                           # a word of this or a later epoch would read as an agent: start over
            entry[0].zero_()
        entry[1] = medium.epoch
        m, a = medium.c_struct(need_owner=False), agents.c_struct()
        _lib.check(_lib.lib.die_stock_plane(C.byref(m), C.byref(a), medium.epoch, _ptr(entry[0]), stream_ptr(dev)), 'die_stock_plane')
        return entry[0]

    def sense(self, medium, agents=None) -> th.Tensor:
        """ConvolutionModel.forward over the medium on the device → (3, W, H) float32 tensor.  `agents`: the DeviceAgents whose
        stocks the `'agent_food'` channel shows — required with `with_stock_channel=True` (ValueError before any launch), unused
        otherwise.  With `memory_channels=M` the agents are required as well, and the tensor holds all 3 + M planes of the last
        layer (planes 3.. are what `forward` reads out into `memory`).  With `signal_channels=K` the stack reads `signals` (allocated
        here as zeros at the first call) and the tensor holds 3 + K + M planes: 3 .. 3 + K - 1 the emissions, then the memory's.
        The field itself is left as it is — only `forward` advances it — and the agents, where given, get their standing plane
        built for it.

        Under `Dynamics(apply_sense_mask=True)` the food and chem planes are read through `medium.sense_mask` (cells outside it
        count as 0, as in the reference's observation).  The stock, memory and signal planes are not part of the medium and stay
        as they are.  The differentiable entries (`differentiable_sense`, `differentiable_action`, `recurrent_action`,
        `signalling_action`) raise NotImplementedError under a mask, before any launch."""
        self._check_wide()
        self._check_stock(medium=medium)
        self._check_memory(medium=medium)
        self._check_signals(medium=medium)
        if self.with_stock_channel and agents is None:
            raise ValueError("sense(medium, agents): with_stock_channel=True needs the agents whose stocks the 'agent_food' channel shows")
        if self.memory_channels:
            self._check_memory_slots(medium, agents)
        medium.sensed()
        dev, W, H = medium.device, medium.W, medium.H
        weights = self._device_weights(dev)
        sp = stream_ptr(dev)
        wide = self._model.wide
        src = self._field_planes(medium)
        # ONE build serves the stock channel, memory and signals (a bare `sense(medium)` of a signal agent needs none: it emits nothing)
        needs_standing = self.with_stock_channel or self.memory_channels or (self.signal_channels and agents is not None)
        standing = self._standing = self._stock_plane(medium, agents) if needs_standing else None
        if self.with_stock_channel:
            src['agent_food'] = (standing, _lib.DIE_PLANE_STOCK)
        if self.signal_channels:                                 # the field as it is now, plain fp32 planes whatever the medium's dtype
            field = self._signals_for(medium)
            for k in range(self.signal_channels):
                src[f'signal_{k}'] = (field[k], _lib.DIE_PLANE_F32)
        if self.memory_channels:                                 # the one standing plane serves both: here its payload is ignored
            expanded = self._expand_memory(medium, agents, standing)
            for j in range(self.memory_channels):
                src[f'memory_{j}'] = (expanded[j], _lib.DIE_PLANE_F32)
        planes = [src[c] for c in self.obs_channels]
        sets = self._scratch(W, H, dev, 2, max(4, *(w.shape[0] for w in weights)) if wide else 4)
        drop = self._dropout()
        for li, w in enumerate(weights):
            cout, cin, k, _ = w.shape
            dst = sets[li % 2]
            cin_arr, out_arr = _layer_arrays(li, w, planes, dst)
            last = li == len(weights) - 1
            pad = _lib.PAD_MODES[self._model.conv_layers()[li].padding_mode]
            if wide:                                             # every layer of a wide stack: die_conv2d_wide
                act = _lib.NCA_ACTIVATIONS['tanh' if last else self._model.hidden_activation]
                _lib.check(_lib.lib.die_conv2d_wide(W, H, cin, cin_arr, medium.epoch, cout, dst.data_ptr(), W * H, k, _ptr(w), act, pad,
                                                    C.byref(drop) if last and drop is not None else None, sp), 'die_conv2d_wide')
            elif last and drop is not None:
                _lib.check(_lib.lib.die_conv2d_dropout(W, H, cin, cin_arr, medium.epoch, cout, out_arr, k, _ptr(w), 1, pad, C.byref(drop), sp),
                           'die_conv2d_dropout')
            else:
                _lib.check(_lib.lib.die_conv2d(W, H, cin, cin_arr, medium.epoch, cout, out_arr, k, _ptr(w), int(last), pad, sp), 'die_conv2d')
            planes = [(dst[o], _lib.DIE_PLANE_F32) for o in range(cout)]
        out = sets[(len(weights) - 1) % 2][:len(planes)]         # the last layer's planes (scratch: valid until the next call)
        if self._dropout_seed is not None:
            self.dropout_step += 1                               # counts forward calls, masked or not
        elif self._model.agent_dropout.p > 0 and self._model.training:     # rare path: the torch-RNG mask of core/agent/evo.py:114-116
            out = out * self._model.agent_dropout(th.ones((W, H), device=dev))
        return out

    def forward(self, obs) -> DeviceAction:
        """:150-174."""
        agents, medium = obs
        sense = self.sense(medium, agents)
        self._sense_output = sense[:3]                           # (with signal or memory channels the planes 3.. follow: not rendered)
        action = DeviceAction(agents.N, agents.device, agents.slot, capacity=agents.capacity)
        action.global_slots = agents.global_slots
        planes = (C.c_void_p * 3)(*[sense[c].data_ptr() for c in range(3)])
        coefs = (C.c_float * 3)(*self.action_coefs)
        m, a, u = medium.c_struct(need_owner=False), agents.c_struct(), action.c_struct()
        _lib.check(_lib.lib.die_gather_scale(C.byref(m), C.byref(a), planes, coefs, C.byref(u), stream_ptr(agents.device)),
                   'die_gather_scale')
        K, (W, H) = self.signal_channels, (medium.W, medium.H)
        if self.memory_channels:                                 # planes 3 + K .. at the agents' cells, before anything moves
            _lib.check(_lib.lib.die_gather_memory(C.byref(m), C.byref(a), self.memory_channels, sense[3 + K].data_ptr(), W * H,
                                                  _ptr(self.memory), max(agents.N, 1), stream_ptr(agents.device)), 'die_gather_memory')
        if K:                                                    # planes 3 .. 3 + K - 1 at the standing plane's cells: the field's next state
            deposit, sigma, decay = self.signal_constants
            _lib.check(_lib.lib.die_signal_step(C.byref(m), _ptr(self._standing), medium.epoch, K, sense[3].data_ptr(), W * H, _ptr(self.signals),
                                                _ptr(self._signals_next), W * H, deposit, sigma, decay, stream_ptr(agents.device)),
                       'die_signal_step')
            self.signals, self._signals_next = self._signals_next, self.signals
        action._keepalive = sense
        if self.memory_inherit is not None:                      # `env.step(agent.forward(obs))` under agents_born: the step's birth
            action._heredity_agent = self                        # pass hands its record to this agent's `inherit_memory`
        return action

    def inherit_memory(self, record, memory: Optional[th.Tensor] = None) -> th.Tensor:
        """Heredity (`memory_inherit` 'blank' / 'copy', `memory_mutation`): the newborns of one birth pass receive
        their memory.  `record`: the `BirthsRecord` of `env.births_record()`, taken after the step (or `apply_births()`) that ran the
        pass and after this agent's forward of that step.

        `memory` None: `self.memory` is updated in place (die_memory_inherit, one launch) and returned.  `Env.step` does exactly
        this by itself for the action of this agent's `forward` — the loop `env.step(agent.forward(obs))` and `Env.run(agent, n)`
        need no further call.  An action that carries no agent (`step_action`, a tensor, `apply_births()`) needs the call.

        `memory`: an (M, N) float32 tensor on the record's device — the `memory_next` of `recurrent_action` / `signalling_action`:
        returns `functional.inherit_memory(memory, record, mode, mutation)`, a new tensor with a `grad_fn` (a child's gradient
        reaches its parent under 'copy'), and leaves `self.memory` holding a copy of the same bits, as `recurrent_action` does.

        Refused with ValueError before any launch, `memory` untouched: an agent without memory channels or without a mode, a
        record that is no stand-alone BirthsRecord, a memory of the wrong shape, dtype or device."""
        from ..functional import check_inherit_operands, inherit_memory, inherit_memory_
        M = self.memory_channels
        if not M:
            raise ValueError('inherit_memory: an agent without memory channels (memory_channels=0) has nothing to inherit')
        if self.memory_inherit is None:
            raise ValueError("inherit_memory: this agent has no rule (memory_inherit=None): build it with memory_inherit='blank' or 'copy'")
        if memory is None:
            check_inherit_operands('inherit_memory (self.memory)', self.memory, record, False, M, contiguous=True)
            return inherit_memory_(self.memory, record, self.memory_inherit, self.memory_mutation)
        check_inherit_operands('inherit_memory', memory, record, False, M)
        out = inherit_memory(memory, record, self.memory_inherit, self.memory_mutation)
        self.memory = out.detach().clone()                       # the agent's own copy, not the graph's tensor
        self._memory_rebind = False
        return out

    # ------------------------------------------------------------------ the differentiable twins (die_nca_grad.hip)
    def differentiable_sense(self, medium) -> th.Tensor:
        """`sense` with a `grad_fn`: (3, W, H) float32 on the medium's device, bit-identical to `sense`, whose backward is the
        conv stack's adjoint on the device (die_conv2d_backward per layer).  Gradients land in `model.parameters()` wherever the
        model lives (the weights go in through a differentiable `.to(device)`).  The medium gets none — unless it carries a chem
        node (`Env.differentiable_chem` / `differentiable_step`, dropped by whatever else changes the field): then the node is an
        input of the graph, the first layer's backward also asks die_conv2d_backward for `grad_in`, and the `chem1` channel's plane
        of it goes to the node (the food and claim planes' gradients are discarded: they are constants of the parameters).  The
        forward reads the medium's own planes either way: same values, same launches.

        Every layer's output goes into storage of its own (not the ping-pong scratch), and the first layer's inputs — the two
        field planes and the claim plane — are COPIED (3 planes), so that `backward` may run after the medium has been stepped.
        With a `dropout_seed` in training mode the last layer is launched twice, masked (the value returned) and unmasked
        (tanh(z), kept for the backward, which recomputes the mask from its key); `dropout_step` advances once per call, as in
        `sense`.  Boundaries 'circular' and 'zeros'; 'reflect' / 'replicate' raise NotImplementedError before any launch.
        `sense` and `forward` are untouched by all this: never differentiable, same scratch, same launches.

        A wide stack (`hidden_channels` / `hidden_activation`) is refused here: NotImplementedError, before any launch and before
        `dropout_step` moves.  Its gradients come from `ConvolutionModel.forward_device` and `die_amd.functional`.  An agent with
        the stock channel (`with_stock_channel=True`) is refused the same way: its plane is piecewise constant in the weights."""
        self._check_differentiable('differentiable_sense')
        layers = self._model.conv_layers()
        self._check_boundary()
        self._check_sense_mask('differentiable_sense', medium)   # (after the refusals that do not look at the medium)
        medium.sensed()
        dev = medium.device
        weights = [k.weight.to(device=dev, dtype=th.float32).contiguous() for k in layers]
        return self._dropout_applied(_DifferentiableSense.apply(self, medium, getattr(medium, 'chem_node', None), *weights), medium)

    def _dropout_applied(self, sense: th.Tensor, medium) -> th.Tensor:
        """What follows the stack of every differentiable call: with a `dropout_seed` the counter advances (the stack masked the
        planes itself), without one the torch-RNG mask falls on all planes."""
        if self._dropout_seed is not None:
            self.dropout_step += 1
        elif self._model.agent_dropout.p > 0 and self._model.training:     # a torch multiply, autograd's own business
            sense = sense * self._model.agent_dropout(th.ones((medium.W, medium.H), device=medium.device))
        return sense

    def differentiable_action(self, obs) -> th.Tensor:
        """`forward` with a `grad_fn`: (3, N) float32, rows dx, dy, deposit for EVERY slot in the agents' array order — the values
        `forward(obs)` puts in its DeviceAction's `data[:, :N]`, bit for bit.  Its backward is the read-out's adjoint
        (die_gather_scale_backward: the slots' gradients scattered onto their cells, then `differentiable_sense`'s backward).
        The slots' coordinates are copied, so `backward` may run after the world has been stepped.  Where several slots with a
        non-zero gradient stand on one cell their terms are summed by fp32 atomic adds in arrival order; otherwise (alive agents
        never share a cell) the gradients are bit-reproducible run to run.  A wide stack raises NotImplementedError, as in
        `differentiable_sense`, and so does an agent with the stock channel."""
        self._check_differentiable('differentiable_action')
        agents, medium = obs
        self._check_boundary()
        self._check_sense_mask('differentiable_action', medium)
        sense = self.differentiable_sense(medium)
        self._sense_output = sense.detach()
        return _DifferentiableReadOut.apply(sense, agents, medium, self.action_coefs)

    def recurrent_action(self, obs, memory: Optional[th.Tensor] = None):
        """`forward` of an agent with memory channels, with a graph: `(action, memory_next)`, (3, N) and (M, N) float32, both with a
        `grad_fn`.  `action` holds, bit for bit, what `forward(obs)` puts in its DeviceAction's `data[:, :N]` (the agents' array
        order), `memory_next` what `forward` leaves in `self.memory` (slot order), given the same incoming memory.

        `memory`: None — `self.memory`, allocated as `forward` allocates it and a constant of the graph — or an (M, N) float32
        tensor on the medium's device, used as given: the `memory_next` of the previous call gives backpropagation through time,
        its `.detach()` truncates the gradient there, a leaf that requires grad receives one.

        In order: the standing plane (die_stock_plane, the agent's own plane), the record of where every slot stands
        (`functional.memory_record`: die_memory_cells), the expand (`functional.memory_planes`), the observation planes stacked in
        `obs_channels` order, the wide stack (`functional.conv2d_wide` per layer), `functional.gather_scale` on planes 0..2 and
        `functional.gather_memory` on planes 3.. .  The record is kept by the graph, so `backward` may run after the world has
        been stepped, re-sorted or reset.  If the medium carries a chem node (`Env.differentiable_chem` / `differentiable_step`)
        the node is the stack's chem plane, as in `differentiable_sense`: `env.differentiable_step(action)` followed by another
        `recurrent_action` backpropagates through the world as well as through the memory.

        The agent is left as `forward(obs)` would leave it: `self.memory` holds a copy of `memory_next`'s values, `dropout_step`
        has advanced once if a `dropout_seed` is set, `_sense_output` is set.  An unseeded `p_agent_dropout` > 0 in training mode
        is a torch mask multiply on all 3 + M planes, as in `differentiable_sense`.

        Under `Dynamics(agents_born=True)` (an agent with `memory_inherit` set) the chain goes through the births: the actions
        are tensors, which carry no agent, so the link after every step is the caller's —

            action, memory_next = agent.recurrent_action(obs, memory)
            obs, *_ = env.step(action)                               # a plain step: deaths, then the birth pass
            memory = agent.inherit_memory(env.births_record(), memory_next)

        `inherit_memory` with a tensor has a `grad_fn` (a gather: under 'copy' a child's gradient is added to its parent's), so
        the loop is backpropagation through time across births; the world itself is not differentiated there
        (`differentiable_step` refuses `agents_born`).

        Refused before any launch, and before `dropout_step` or `memory` change: an agent without memory channels (ValueError: it
        has `differentiable_action`); with NotImplementedError the stock channel (the adjoint calls do not take its plane kind), a
        decomposed medium, fp16 fields and the boundaries 'reflect' / 'replicate'; with ValueError a `memory` of the wrong shape,
        dtype or device."""
        self._check_signals('recurrent_action')
        if not self.memory_channels:
            raise ValueError('recurrent_action: an agent without memory channels (memory_channels=0) is differentiated by '
                             'differentiable_action')
        action, _, memory_next = self._stateful_action('recurrent_action', obs, None, memory)
        return action, memory_next

    def signalling_action(self, obs, signals: Optional[th.Tensor] = None, memory: Optional[th.Tensor] = None):
        """`forward` of an agent with signal channels, with a graph: `(action, signals_next, memory_next)` — (3, N), (K, W, H) and
        (M, N) float32, each with a `grad_fn`; `memory_next` is None without memory channels.  `action` holds, bit for bit, what
        `forward(obs)` puts in its DeviceAction's `data[:, :N]`, `signals_next` what it leaves in `self.signals` and `memory_next`
        what it leaves in `self.memory`, given the same incoming field and memory.

        `signals`: None — `self.signals`, allocated or bound as `forward` does it and a constant of the graph — or a (K, W, H)
        float32 tensor on the medium's device, used as given: the `signals_next` of the previous call gives backpropagation through
        time through the field, its `.detach()` truncates the gradient there, a leaf that requires grad receives one.  `memory`: as
        in `recurrent_action`.

        In order: the standing plane (die_stock_plane, the agent's own plane, one build for both records), the record of the cells
        stood on (`functional.signal_record`: die_signal_cells) and, with memory, of where every slot stands
        (`functional.memory_record`), the expand (`functional.memory_planes`), the observation planes stacked in `obs_channels`
        order — `signal_k` is `signals[k]`, `chem1` the medium's chem node where it carries one — the wide stack
        (`functional.conv2d_wide` per layer), `functional.gather_scale` on planes 0..2, `functional.signal_step` on planes
        3 .. 3 + K - 1 and `functional.gather_memory` on planes 3 + K .. .  The records are kept by the graph, so `backward` may run
        after the world has been stepped, re-sorted or reset and after `reset_signals()`.  Two gradients reach a `signals_next`
        that is handed on — the next stack's input gradient and the next link's field gradient — and autograd sums them.

        The agent is left as `forward(obs)` would leave it: `self.signals` and `self.memory` hold copies of the values (not the
        graph's tensors), `dropout_step` has advanced once if a `dropout_seed` is set, `_sense_output` is set.  An unseeded
        `p_agent_dropout` > 0 in training mode is a torch mask multiply on all planes, as in `recurrent_action`.

        Refused before any launch, and before `dropout_step`, `signals` or `memory` change: an agent without signal channels
        (ValueError: it has `recurrent_action` / `differentiable_action`); with NotImplementedError the stock channel (its
        gradients are out of scope), a decomposed medium, fp16 fields and the boundaries 'reflect' / 'replicate'; with ValueError
        a `signals` or `memory` of the wrong shape, dtype or device, and a medium of another shape than the one `self.signals` is
        bound to (until `reset_signals()`).  Populations have the batched twin, `BatchedNeuralAutomataAgent.signalling_action`: one
        launch per kernel for all replicas, the same bits per replica."""
        if not self.signal_channels:
            raise ValueError('signalling_action: an agent without signal channels (signal_channels=0) is differentiated by '
                             'recurrent_action (memory channels) or differentiable_action')
        return self._stateful_action('signalling_action', obs, signals, memory)

    def _check_stateful(self, what: str, obs, signals, memory) -> None:
        """Every refusal `recurrent_action` and `signalling_action` share, in their one order, before any launch (`what`: the
        caller's name, the prefix of the texts).  On a decomposed medium the signal channels speak where the agent has them, else
        the memory channels; a field bound to another shape speaks last but one, a sense mask (NotImplementedError) last."""
        K, M = self.signal_channels, self.memory_channels
        self._check_stock(what)
        self._check_boundary(f'{what}: ')
        agents, medium = obs
        if getattr(medium, 'world', None) is not None:
            self._check_signals(medium=medium)
            self._check_memory(medium=medium)
        if medium.dtype != th.float32:
            raise NotImplementedError(f'{what}: fp32 fields only (this medium is {medium.dtype})')
        if signals is not None:
            check_given(what, 'signals', signals, (K, medium.W, medium.H), medium.device)
        if memory is not None and not M:
            raise ValueError(f'{what}: memory given to an agent without memory channels (memory_channels=0)')
        if M and memory is None:
            self._check_memory_slots(medium, agents)
        elif M:
            check_given(what, 'memory', memory, (M, agents.N), medium.device)
            if getattr(agents, 'global_slots', False):
                raise NotImplementedError(f'memory_channels={M} on a decomposed world (die_amd/dist.py): its slots carry world ids')
        self._check_signals(medium=medium)                       # a field bound to another shape: ValueError until reset_signals()
        self._check_sense_mask(what, medium)                     # a sense mask speaks after everything else

    def _stateful_action(self, what: str, obs, signals, memory):
        """The one body of `recurrent_action` (K = 0: no field, `signals_next` None) and `signalling_action`: the refusals, the
        standing plane and the records, the expand, the stack, the read-outs, the agent's own copies."""
        from ..functional import gather_memory, gather_scale, memory_planes, memory_record, signal_record, signal_step
        K, M = self.signal_channels, self.memory_channels
        self._check_stateful(what, obs, signals, memory)
        agents, medium = obs
        medium.sensed()
        field = None
        if K:
            own = self._signals_for(medium)                      # allocated or bound as `forward` does it
            field = own if signals is None else signals
        if M and memory is None:
            memory = self._memory_for(medium, agents)
        standing = self._stock_plane(medium, agents)
        if K:
            self._standing = standing
        cells = signal_record(obs, standing) if K else None
        record = memory_record(obs, standing) if M else None
        expanded = memory_planes(memory, record) if M else None
        node = getattr(medium, 'chem_node', None)

        def plane(c):
            if c.startswith('signal_'):
                return field[int(c[len('signal_'):])]
            if c.startswith('memory_'):
                return expanded[int(c[len('memory_'):])]
            return node if c == 'chem1' and node is not None else medium.sel(c).float()

        planes = th.stack([plane(c) for c in self.obs_channels])
        p, seed = self._model.agent_dropout.p, self._dropout_seed
        masked = seed is not None and p > 0 and self._model.training
        sense = self._dropout_applied(self._model._stack_device(planes, (p, seed, self.dropout_step) if masked else None), medium)
        self._sense_output = sense.detach()[:3]
        action = gather_scale(sense[:3], obs, self.action_coefs)
        signals_next = memory_next = None
        if K:
            deposit, sigma, decay = self.signal_constants
            signals_next = signal_step(field, sense[3:3 + K], cells, deposit=deposit, sigma=sigma, decay=decay)
            self.signals = signals_next.detach().clone()         # the agent's own copies, not the graph's tensors
        if M:
            memory_next = gather_memory(sense[3 + K:], record)
            self.memory = memory_next.detach().clone()
            self._memory_rebind = False
        return action, signals_next, memory_next

    def render(self) -> Sequence[np.ndarray]:
        """:176-181: the transformed medium with the channel axis last."""
        if self._sense_output is None:
            return [np.ones((2, 2, 3))]
        return [th.moveaxis(self._sense_output, 0, -1).cpu().numpy()]


class _DifferentiableSense(th.autograd.Function):
    """NeuralAutomataAgent.differentiable_sense: the forward is `sense`'s launches into storage the graph owns, the backward
    one die_conv2d_backward per layer, last layer first."""

    @staticmethod
    def forward(ctx, agent, medium, chem_node, *weights):
        dev, W, H = medium.device, medium.W, medium.H
        ctx.chem_channel = None if chem_node is None else agent.obs_channels.index('chem1')     # (its values ARE medium.chem's)
        sp = stream_ptr(dev)
        src = agent._field_planes(medium)
        planes = src_planes = [(src[c][0].clone(), src[c][1]) for c in agent.obs_channels]     # as they are now: the medium will be stepped
        drop = agent._dropout()
        pads = [_lib.PAD_MODES[k.padding_mode] for k in agent._model.conv_layers()]
        first, hidden, out, tanh_out = [t for t, _ in planes], [], None, None
        for li, w in enumerate(weights):
            cout, cin, k, _ = w.shape
            last = li == len(weights) - 1

            def launch(masked):
                dst = th.empty((cout, W, H), dtype=th.float32, device=dev)
                cin_arr, out_arr = _layer_arrays(li, w, planes, dst)
                if masked:
                    _lib.check(_lib.lib.die_conv2d_dropout(W, H, cin, cin_arr, medium.epoch, cout, out_arr, k, _ptr(w), 1, pads[li],
                                                           C.byref(drop), sp), 'die_conv2d_dropout')
                else:
                    _lib.check(_lib.lib.die_conv2d(W, H, cin, cin_arr, medium.epoch, cout, out_arr, k, _ptr(w), int(last), pads[li], sp),
                               'die_conv2d')
                return dst

            out = tanh_out = launch(False)
            if last and drop is not None:
                out = launch(True)                               # what `sense` returns; tanh_out stays unmasked for the backward
            planes = [(out[o], _lib.DIE_PLANE_F32) for o in range(cout)]
            if not last:
                hidden.append(out)
        ctx.kinds, ctx.pads, ctx.epoch, ctx.size, ctx.dev = [kind for _, kind in src_planes], pads, medium.epoch, (W, H), dev
        ctx.drop = None if drop is None else (drop.p, drop.seed, drop.step)
        # everything the backward reads goes through save_for_backward: freed with the graph after a backward without retain_graph
        ctx.save_for_backward(*weights, tanh_out, *first, *hidden)
        return out

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        saved = ctx.saved_tensors
        L, n_first = len(ctx.pads), len(ctx.kinds)
        weights, tanh_out, first, hidden = saved[:L], saved[L], saved[L + 1:L + 1 + n_first], saved[L + 1 + n_first:]
        (W, H), dev = ctx.size, ctx.dev
        sp = stream_ptr(dev)
        g = grad.to(dtype=th.float32).contiguous()
        drop = None if ctx.drop is None else _lib.nca_dropout(ctx.drop[0], ctx.drop[1], 0, ctx.drop[2])
        grads = [None] * L
        to_node = ctx.chem_channel is not None and ctx.needs_input_grad[2]
        need = [_lib.lib.die_conv2d_backward_workspace_bytes(W, H, w.shape[1], w.shape[0], w.shape[2]) for w in weights]
        if min(need) < 0:
            raise ValueError('a layer shape die_conv2d_backward does not take (1..4 channels, kernel size 1, 3, 5 or 7)')
        ws = th.empty((max(need) // 4,), dtype=th.float32, device=dev)            # one workspace, sized for the largest layer
        for li in reversed(range(L)):
            w = weights[li]
            cout, cin, k, _ = w.shape
            last = li == L - 1
            inputs = list(zip(first, ctx.kinds)) if li == 0 else [(hidden[li - 1][c], _lib.DIE_PLANE_F32) for c in range(cin)]
            cin_arr = (_lib.ConvPlane * cin)(*[_lib.ConvPlane(t.data_ptr(), kind, 0) for t, kind in inputs])
            g_arr = (C.c_void_p * cout)(*[g[o].data_ptr() for o in range(cout)])
            grad_w = th.empty_like(w)
            # the first layer's input is the medium: a gradient there only for a chem node that asks for one
            grad_in = th.empty((cin, W, H), dtype=th.float32, device=dev) if li > 0 or to_node else None
            gin_arr = None if grad_in is None else (C.c_void_p * cin)(*[grad_in[c].data_ptr() for c in range(cin)])
            t_arr = (C.c_void_p * cout)(*[tanh_out[o].data_ptr() for o in range(cout)]) if last else None
            _lib.check(_lib.lib.die_conv2d_backward(W, H, cin, cin_arr, ctx.epoch, cout, g_arr, k, _ptr(w), _ptr(grad_w), gin_arr, t_arr,
                                                    C.byref(drop) if last and drop is not None else None, ctx.pads[li], _ptr(ws),
                                                    need[li], sp), 'die_conv2d_backward')
            grads[li] = grad_w
            g = grad_in
        return (None, None, g[ctx.chem_channel] if to_node else None, *grads)


class _DifferentiableReadOut(th.autograd.Function):
    """NeuralAutomataAgent.differentiable_action's last step: die_gather_scale forward, die_gather_scale_backward backward."""

    @staticmethod
    def forward(ctx, sense, agents, medium, coefs):
        sense = sense.contiguous()
        N, dev = agents.N, agents.device
        out = th.empty((3, N), dtype=th.float32, device=dev)
        planes = (C.c_void_p * 3)(*[sense[c].data_ptr() for c in range(3)])
        cf = (C.c_float * 3)(*coefs)
        m, a = medium.c_struct(need_owner=False), agents.c_struct()
        u = _lib.Action(N, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        _lib.check(_lib.lib.die_gather_scale(C.byref(m), C.byref(a), planes, cf, C.byref(u), stream_ptr(dev)), 'die_gather_scale')
        ctx.save_for_backward(agents.x.clone(), agents.y.clone())             # where the slots stand now: the world will be stepped
        ctx.N, ctx.m, ctx.coefs, ctx.size, ctx.dev = N, m, tuple(coefs), (medium.W, medium.H), dev
        return out

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, y = ctx.saved_tensors
        g = grad.to(dtype=th.float32).contiguous()
        planes = th.empty((3, *ctx.size), dtype=th.float32, device=ctx.dev)      # (cleared by the call)
        p_arr = (C.c_void_p * 3)(*[planes[c].data_ptr() for c in range(3)])
        cf = (C.c_float * 3)(*ctx.coefs)
        a = _lib.Agents(ctx.N, _ptr(x), _ptr(y), None, None, None)
        u = _lib.Action(ctx.N, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr())
        _lib.check(_lib.lib.die_gather_scale_backward(C.byref(ctx.m), C.byref(a), C.byref(u), cf, p_arr, stream_ptr(ctx.dev)),
                   'die_gather_scale_backward')
        return planes, None, None, None


class _DifferentiableFieldStep(th.autograd.Function):
    """Env.differentiable_step's node: the value is a copy of the chem plane the step left, the backward die_env_step_backward —
    the forward's own diffusion sweep on the gradient plane (on the torus Gᵀ = G) and a gather at the recorded winners' cells."""

    @staticmethod
    def forward(ctx, prev_node, action, cells, chem, sigma, decay):
        ctx.save_for_backward(cells)
        ctx.sigma, ctx.decay, ctx.size, ctx.dev = float(sigma), float(decay), tuple(chem.shape), chem.device
        return chem.clone()

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        cells, = ctx.saved_tensors
        (W, H), dev, N = ctx.size, ctx.dev, cells.numel()
        g = grad.to(dtype=th.float32).contiguous()
        grad_chem = th.empty((W, H), dtype=th.float32, device=dev)
        grad_action = None
        if ctx.needs_input_grad[1]:
            grad_action = th.zeros((3, N), dtype=th.float32, device=dev)      # dx, dy: positions are constants of the parameters
        _lib.check(_lib.lib.die_env_step_backward(W, H, _ptr(g), ctx.sigma, ctx.decay, N if grad_action is not None else 0, _ptr(cells),
                                                  _ptr(grad_chem), None if grad_action is None else grad_action[2].data_ptr(),
                                                  stream_ptr(dev)), 'die_env_step_backward')
        return grad_chem if ctx.needs_input_grad[0] else None, grad_action, None, None, None, None
