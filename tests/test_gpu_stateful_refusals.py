"""The refusals of the four stateful differentiable calls, whole: `recurrent_action` and `signalling_action` of
BatchedNeuralAutomataAgent and of the stand-alone NeuralAutomataAgent.  The bit-for-bit files (test_gpu_memory_grad.py,
test_gpu_memory_grad_batch.py, test_gpu_signal_grad.py, test_gpu_signal_grad_batch.py) match a word of each message; here every
single fault a body can raise is pinned as (exception type, full text), the device's name written `@`, and for every pair of
faults that stand next to each other in a body's order of refusals, who speaks first.  After every refusal: `dropout_step`,
`memory` and `signals` are the same objects holding the same values, and the world's bits are unchanged.  Nothing is launched
beyond building the worlds.

The expected values are literals at the end of the file; `python -m tests.test_gpu_stateful_refusals` prints them."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
W, H, R = 13, 10, 2                  # the shapes tests/test_gpu_signal_grad_batch.py refuses on
WIDE = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh')
CONSTANTS = (0.75, 0.8, 0.05)        # signal_deposit, signal_sigma, signal_decay

# what a fault changes in the case's description (`_population_refusal` / `_agent_refusal` read it)
FAULTS = {
    'signal channels': dict(K=2),
    'no signal channels': dict(K=0),
    'no memory channels': dict(M=0),
    'stock': dict(stock=True),
    'per_replica': dict(per_replica=True),
    'decomposed medium': dict(world=True),
    'fp16': dict(fp16=True),
    'reflect': dict(boundary='reflect'),
    'replicate': dict(boundary='replicate'),
    'own parameters no tensor': dict(own='no tensor'),
    'own parameters of another dtype': dict(own='dtype'),
    'unseeded dropout': dict(seeded=False),
    'parameters no tensor': dict(parameters='no tensor'),
    'parameters of another shape': dict(parameters='shape'),
    'parameters of another dtype': dict(parameters='dtype'),
    'parameters on another device': dict(parameters='device'),
    'parameters not contiguous': dict(parameters='strides'),
    'signals of another shape': dict(signals='shape'),
    'signals in the inner layout': dict(signals='inner'),
    'signals of another dtype': dict(signals='dtype'),
    'signals on another device': dict(signals='device'),
    'signals no tensor': dict(signals='no tensor'),
    'memory without memory channels': dict(M=0, memory='right'),
    'memory of another shape': dict(memory='shape'),
    'memory of another dtype': dict(memory='dtype'),
    'memory on another device': dict(memory='device'),
    'memory no tensor': dict(memory='no tensor'),
    'world slot ids': dict(global_slots=True),
    'world slot ids, memory given': dict(global_slots=True, memory='right'),
    'held memory no tensor': dict(held='no tensor'),
    'held memory of another dtype': dict(held='dtype'),
    'held memory of other slots': dict(held='slots'),
    'field of another shape': dict(bound='shape'),
}
BOUNDARY = ['reflect', 'replicate']
OWN = ['own parameters no tensor', 'own parameters of another dtype']
PARAMETERS = ['parameters no tensor', 'parameters of another shape', 'parameters of another dtype', 'parameters on another device',
              'parameters not contiguous']
SIGNALS = ['signals of another shape', 'signals of another dtype', 'signals on another device', 'signals no tensor']
MEMORY = ['memory of another shape', 'memory of another dtype', 'memory on another device', 'memory no tensor']
HELD = ['world slot ids', 'held memory no tensor', 'held memory of another dtype', 'held memory of other slots']

# method: (K and M without a fault, the single faults in the body's order, the adjacent pairs)
METHODS = {
    'population.recurrent_action': (
        dict(K=0, M=2),
        ['signal channels', 'no memory channels', 'stock', 'per_replica', 'fp16'] + BOUNDARY + OWN + ['unseeded dropout'] + PARAMETERS
        + MEMORY,
        [('signal channels', 'no memory channels'), ('no memory channels', 'stock'), ('stock', 'per_replica'), ('per_replica', 'fp16'),
         ('fp16', 'reflect'), ('reflect', 'own parameters no tensor'), ('own parameters of another dtype', 'unseeded dropout'),
         ('unseeded dropout', 'parameters no tensor'), ('parameters of another shape', 'memory of another shape')]),
    'population.signalling_action': (
        dict(K=2, M=2),
        ['no signal channels', 'stock', 'per_replica', 'fp16'] + BOUNDARY + OWN + ['unseeded dropout'] + PARAMETERS
        + ['signals in the inner layout'] + SIGNALS + ['memory without memory channels'] + MEMORY,
        [('no signal channels', 'stock'), ('stock', 'per_replica'), ('per_replica', 'fp16'), ('fp16', 'reflect'),
         ('reflect', 'own parameters no tensor'), ('own parameters of another dtype', 'unseeded dropout'),
         ('unseeded dropout', 'parameters no tensor'), ('parameters of another shape', 'signals of another shape'),
         ('signals of another shape', 'memory without memory channels'), ('signals no tensor', 'memory of another shape')]),
    'agent.recurrent_action': (
        dict(K=0, M=2),
        ['signal channels', 'no memory channels', 'stock'] + BOUNDARY + ['decomposed medium', 'fp16'] + HELD + MEMORY
        + ['world slot ids, memory given'],
        [('signal channels', 'no memory channels'), ('no memory channels', 'stock'), ('stock', 'reflect'),
         ('reflect', 'decomposed medium'), ('decomposed medium', 'fp16'), ('fp16', 'held memory no tensor'),
         ('fp16', 'memory of another shape'), ('world slot ids', 'held memory no tensor'), ('memory of another shape', 'world slot ids')]),
    'agent.signalling_action': (
        dict(K=2, M=2),
        ['no signal channels', 'stock'] + BOUNDARY + ['decomposed medium', 'fp16'] + SIGNALS + ['memory without memory channels'] + HELD
        + MEMORY + ['world slot ids, memory given', 'field of another shape'],
        [('no signal channels', 'stock'), ('stock', 'reflect'), ('reflect', 'decomposed medium'), ('decomposed medium', 'fp16'),
         ('fp16', 'signals of another shape'), ('signals of another shape', 'memory without memory channels'),
         ('signals no tensor', 'held memory no tensor'), ('signals of another dtype', 'memory of another shape'),
         ('world slot ids', 'held memory no tensor'), ('memory of another shape', 'world slot ids'),
         ('held memory of other slots', 'field of another shape'), ('memory no tensor', 'field of another shape'),
         ('world slot ids, memory given', 'field of another shape')]),
}
CASES = [(method, case) for method, (_, single, pairs) in METHODS.items() for case in single + [' + '.join(p) for p in pairs]]


def _spec(method: str, case: str) -> dict:
    """The case's description: the method's K and M, then what each of its faults changes."""
    spec = dict(METHODS[method][0])
    for fault in case.split(' + '):
        spec.update(FAULTS[fault])
    return spec


def _candidates(n: int, spec: dict, **kw):
    torch.manual_seed(1)
    deposit, sigma, decay = CONSTANTS
    sig = dict(signal_channels=spec['K'], signal_deposit=deposit, signal_sigma=sigma, signal_decay=decay) if spec['K'] else {}
    if 'boundary' in spec:
        kw['boundary'] = spec['boundary']
    return [die.NeuralAutomataAgent(scale=0.05, deposit=2.0, memory_channels=spec['M'], p_agent_dropout=0.25,
                                    with_stock_channel=spec.get('stock', False), **sig, **dict(WIDE, **kw)) for _ in range(n)]


def _given(variant, shape, inner=None):
    """A `signals`, `memory` or `parameters` argument: None, right, or wrong in one way."""
    if variant is None:
        return None
    if variant == 'right':
        return torch.zeros(shape, device=DEV)
    if variant == 'shape':
        return torch.zeros(shape[:-1] + (shape[-1] + 1,), device=DEV)
    if variant == 'inner':
        return torch.zeros(inner, device=DEV)
    if variant == 'dtype':
        return torch.zeros(shape, dtype=torch.float64, device=DEV)
    if variant == 'device':
        return torch.zeros(shape)
    if variant == 'strides':
        return torch.zeros(shape[::-1], device=DEV).t()
    assert variant == 'no tensor'
    return np.zeros(shape, dtype=np.float32)


def _observe(call, device) -> tuple:
    with pytest.raises(Exception) as err:
        call()
    return type(err.value).__name__, str(err.value).replace(str(device), '@')


def _population_refusal(method: str, spec: dict) -> tuple:
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.3), replicas=R, seed=2, device=DEV,
                      field_dtype=torch.float16 if spec.get('fp16') else torch.float32, per_replica=True if spec.get('per_replica') else None)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _candidates(R, spec), dropout_seed=3 if spec.get('seeded', True) else None)
    pop.dropout_step = 4
    K, M, Nmax = spec['K'], spec['M'], benv.Nmax
    held, field = pop.memory, pop._signals
    if held is not None:
        held.fill_(0.5)
    if field is not None:
        field.fill_(0.25)
    if 'own' in spec:
        pop.parameters = _given(spec['own'], (pop.candidates, pop.P))
    before = None if benv.per_replica else (benv._state.cpu().numpy().copy(), benv.epoch)
    signals = _given(spec.get('signals'), (R, 2, W, H), inner=(2, R + 1, W, H))
    memory = _given(spec.get('memory'), (R, 2, Nmax))
    parameters = _given(spec.get('parameters'), (pop.candidates, pop.P))
    if method == 'recurrent_action':
        seen = _observe(lambda: pop.recurrent_action(memory, parameters), benv.device)
    else:
        seen = _observe(lambda: pop.signalling_action(signals, memory, parameters), benv.device)
    assert pop.dropout_step == 4 and pop.memory is held and pop._signals is field
    assert (held is None or bool((held == 0.5).all())) and (field is None or bool((field == 0.25).all()))
    if before is not None:
        assert np.array_equal(before[0], benv._state.cpu().numpy()) and before[1] == benv.epoch
    return seen


def _env_bits(env):
    m, a = env.medium, env.agents
    return [t.cpu().numpy().copy() for t in (m.owner, m.food, m.chem, a.x, a.y, a.alive, a.agent_food)] + [m.epoch, a.N]


def _agent_refusal(method: str, spec: dict) -> tuple:
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.3), seed=2, max_agents='alive', device=DEV,
                  field_dtype=torch.float16 if spec.get('fp16') else torch.float32)
    ag, = _candidates(1, spec, dropout_seed=3)
    ag = ag.to(env.device)
    ag.dropout_step = 4
    K, M, N = spec['K'], spec['M'], env.agents.N
    # an agent in mid-run: its memory and its field bound to this world
    if M:
        ag.memory, ag._memory_rebind = torch.full((M, N), 0.5, device=DEV), False
    if K:
        ag.signals, ag._signals_rebind = torch.full((K, W + (1 if spec.get('bound') == 'shape' else 0), H), 0.25, device=DEV), False
    if 'held' in spec:
        ag.memory = _given('shape' if spec['held'] == 'slots' else spec['held'], (M, N))
    held, field = ag.memory, ag.signals
    kept = None if held is None else np.array(held.cpu() if isinstance(held, torch.Tensor) else held)
    if spec.get('world'):
        env.medium.world = (2 * W, H, 0, 0)
    if spec.get('global_slots'):
        env.agents.global_slots = True
    before = _env_bits(env)
    obs = env._get_current_obs
    signals = _given(spec.get('signals'), (2, W, H))
    memory = _given(spec.get('memory'), (2, N))
    if method == 'recurrent_action':
        seen = _observe(lambda: ag.recurrent_action(obs, memory), env.device)
    else:
        seen = _observe(lambda: ag.signalling_action(obs, signals, memory), env.device)
    assert ag.dropout_step == 4 and ag.memory is held and ag.signals is field
    assert held is None or np.array_equal(kept, np.array(held.cpu() if isinstance(held, torch.Tensor) else held))
    assert field is None or bool((field == 0.25).all())
    assert all(np.array_equal(u, v) for u, v in zip(before, _env_bits(env)))
    return seen


def _refusal(method: str, case: str) -> tuple:
    whose, name = method.split('.')
    return (_population_refusal if whose == 'population' else _agent_refusal)(name, _spec(method, case))


@pytest.mark.parametrize('method,case', CASES, ids=['%s: %s' % c for c in CASES])
def test_the_refusal_whole_and_what_it_leaves_alone(method, case):
    assert _refusal(method, case) == EXPECT[method][case]


def test_every_case_has_its_literal():
    assert {m: list(v) for m, v in EXPECT.items()} == {m: [c for q, c in CASES if q == m] for m in METHODS}


# ------------------------------------------------------------------------------------------------ recording
def _record():
    out = ['EXPECT = {']
    for method in METHODS:
        out.append('    %r: {' % method)
        out += ['        %r:\n            %r,' % (case, _refusal(method, case)) for q, case in CASES if q == method]
        out.append('    },')
    print('\n'.join(out + ['}']))


# ------------------------------------------------------------------------------------------------ the recorded values
EXPECT = {
    'population.recurrent_action': {
        'signal channels':
            ('NotImplementedError', "recurrent_action: no gradients through signal channels (signal_channels=2): the field's update has no adjoint"),
        'no memory channels':
            ('ValueError', 'recurrent_action: a population without memory channels (memory_channels=0) is differentiated by forward_device / differentiable_action'),
        'stock':
            ('NotImplementedError', 'recurrent_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'per_replica':
            ('NotImplementedError', 'recurrent_action: large worlds (per_replica) are not batched — a large world fills the GPU through the stand-alone NeuralAutomataAgent.recurrent_action (replica_agent(r))'),
        'fp16':
            ('NotImplementedError', 'recurrent_action: fp32 fields only (this batch holds torch.float16)'),
        'reflect':
            ('NotImplementedError', "recurrent_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'replicate':
            ('NotImplementedError', "recurrent_action: boundary='replicate' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'own parameters no tensor':
            ('ValueError', 'parameters: a (2, 720) float32 tensor on @'),
        'own parameters of another dtype':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'unseeded dropout':
            ('NotImplementedError', 'p_agent_dropout > 0 in training mode: without a dropout_seed its mask is a host-RNG torch op, not batched (build the population with dropout_seed=S for the counter-based mask, call model.eval(), or step the candidates one at a time)'),
        'parameters no tensor':
            ('ValueError', 'parameters: a (2, 720) float32 tensor on @'),
        'parameters of another shape':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'parameters of another dtype':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'parameters on another device':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'parameters not contiguous':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'memory of another shape':
            ('ValueError', "recurrent_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 40), torch.float32, '@')"),
        'memory of another dtype':
            ('ValueError', "recurrent_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 39), torch.float64, '@')"),
        'memory on another device':
            ('ValueError', "recurrent_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 39), torch.float32, 'cpu')"),
        'memory no tensor':
            ('ValueError', 'recurrent_action: memory must be a (2, 2, 39) float32 tensor on @, got ndarray'),
        'signal channels + no memory channels':
            ('NotImplementedError', "recurrent_action: no gradients through signal channels (signal_channels=2): the field's update has no adjoint"),
        'no memory channels + stock':
            ('ValueError', 'recurrent_action: a population without memory channels (memory_channels=0) is differentiated by forward_device / differentiable_action'),
        'stock + per_replica':
            ('NotImplementedError', 'recurrent_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'per_replica + fp16':
            ('NotImplementedError', 'recurrent_action: large worlds (per_replica) are not batched — a large world fills the GPU through the stand-alone NeuralAutomataAgent.recurrent_action (replica_agent(r))'),
        'fp16 + reflect':
            ('NotImplementedError', 'recurrent_action: fp32 fields only (this batch holds torch.float16)'),
        'reflect + own parameters no tensor':
            ('NotImplementedError', "recurrent_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'own parameters of another dtype + unseeded dropout':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
        'unseeded dropout + parameters no tensor':
            ('NotImplementedError', 'p_agent_dropout > 0 in training mode: without a dropout_seed its mask is a host-RNG torch op, not batched (build the population with dropout_seed=S for the counter-based mask, call model.eval(), or step the candidates one at a time)'),
        'parameters of another shape + memory of another shape':
            ('ValueError', 'parameters must stay a contiguous (2, 720) float32 tensor on @'),
    },
    'population.signalling_action': {
        'no signal channels':
            ('ValueError', 'signalling_action: a population without signal channels (signal_channels=0) is differentiated by recurrent_action (memory channels) or forward_device / differentiable_action'),
        'stock':
            ('NotImplementedError', 'signalling_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'per_replica':
            ('NotImplementedError', 'signalling_action: large worlds (per_replica) are not batched — a large world fills the GPU through the stand-alone NeuralAutomataAgent.signalling_action (replica_agent(r))'),
        'fp16':
            ('NotImplementedError', 'signalling_action: fp32 fields only (this batch holds torch.float16)'),
        'reflect':
            ('NotImplementedError', "signalling_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'replicate':
            ('NotImplementedError', "signalling_action: boundary='replicate' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'own parameters no tensor':
            ('ValueError', 'parameters: a (2, 1008) float32 tensor on @'),
        'own parameters of another dtype':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'unseeded dropout':
            ('NotImplementedError', 'p_agent_dropout > 0 in training mode: without a dropout_seed its mask is a host-RNG torch op, not batched (build the population with dropout_seed=S for the counter-based mask, call model.eval(), or step the candidates one at a time)'),
        'parameters no tensor':
            ('ValueError', 'parameters: a (2, 1008) float32 tensor on @'),
        'parameters of another shape':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'parameters of another dtype':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'parameters on another device':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'parameters not contiguous':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'signals in the inner layout':
            ('ValueError', "signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ((2, 3, 13, 10), torch.float32, '@')"),
        'signals of another shape':
            ('ValueError', "signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ((2, 2, 13, 11), torch.float32, '@')"),
        'signals of another dtype':
            ('ValueError', "signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ((2, 2, 13, 10), torch.float64, '@')"),
        'signals on another device':
            ('ValueError', "signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ((2, 2, 13, 10), torch.float32, 'cpu')"),
        'signals no tensor':
            ('ValueError', 'signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ndarray'),
        'memory without memory channels':
            ('ValueError', 'signalling_action: memory given to a population without memory channels (memory_channels=0)'),
        'memory of another shape':
            ('ValueError', "signalling_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 40), torch.float32, '@')"),
        'memory of another dtype':
            ('ValueError', "signalling_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 39), torch.float64, '@')"),
        'memory on another device':
            ('ValueError', "signalling_action: memory must be a (2, 2, 39) float32 tensor on @, got ((2, 2, 39), torch.float32, 'cpu')"),
        'memory no tensor':
            ('ValueError', 'signalling_action: memory must be a (2, 2, 39) float32 tensor on @, got ndarray'),
        'no signal channels + stock':
            ('ValueError', 'signalling_action: a population without signal channels (signal_channels=0) is differentiated by recurrent_action (memory channels) or forward_device / differentiable_action'),
        'stock + per_replica':
            ('NotImplementedError', 'signalling_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'per_replica + fp16':
            ('NotImplementedError', 'signalling_action: large worlds (per_replica) are not batched — a large world fills the GPU through the stand-alone NeuralAutomataAgent.signalling_action (replica_agent(r))'),
        'fp16 + reflect':
            ('NotImplementedError', 'signalling_action: fp32 fields only (this batch holds torch.float16)'),
        'reflect + own parameters no tensor':
            ('NotImplementedError', "signalling_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (step() takes all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'own parameters of another dtype + unseeded dropout':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'unseeded dropout + parameters no tensor':
            ('NotImplementedError', 'p_agent_dropout > 0 in training mode: without a dropout_seed its mask is a host-RNG torch op, not batched (build the population with dropout_seed=S for the counter-based mask, call model.eval(), or step the candidates one at a time)'),
        'parameters of another shape + signals of another shape':
            ('ValueError', 'parameters must stay a contiguous (2, 1008) float32 tensor on @'),
        'signals of another shape + memory without memory channels':
            ('ValueError', "signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ((2, 2, 13, 11), torch.float32, '@')"),
        'signals no tensor + memory of another shape':
            ('ValueError', 'signalling_action: signals must be a (2, 2, 13, 10) float32 tensor on @, got ndarray'),
    },
    'agent.recurrent_action': {
        'signal channels':
            ('NotImplementedError', "recurrent_action: no gradients through signal channels (signal_channels=2): the field's update has no adjoint"),
        'no memory channels':
            ('ValueError', 'recurrent_action: an agent without memory channels (memory_channels=0) is differentiated by differentiable_action'),
        'stock':
            ('NotImplementedError', 'recurrent_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'reflect':
            ('NotImplementedError', "recurrent_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'replicate':
            ('NotImplementedError', "recurrent_action: boundary='replicate' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'decomposed medium':
            ('NotImplementedError', 'memory_channels=2 on a decomposed medium (die_amd/dist.py): the standing plane is built for periodic single-tile planes only'),
        'fp16':
            ('NotImplementedError', 'recurrent_action: fp32 fields only (this medium is torch.float16)'),
        'world slot ids':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'held memory no tensor':
            ('ValueError', 'memory: a contiguous (2, N) float32 tensor on @'),
        'held memory of another dtype':
            ('ValueError', 'memory: a contiguous (2, N) float32 tensor on @'),
        'held memory of other slots':
            ('ValueError', 'memory holds 40 slots, the agents have 39: call reset_memory() to start blank with them'),
        'memory of another shape':
            ('ValueError', "recurrent_action: memory must be a (2, 39) float32 tensor on @, got ((2, 40), torch.float32, '@')"),
        'memory of another dtype':
            ('ValueError', "recurrent_action: memory must be a (2, 39) float32 tensor on @, got ((2, 39), torch.float64, '@')"),
        'memory on another device':
            ('ValueError', "recurrent_action: memory must be a (2, 39) float32 tensor on @, got ((2, 39), torch.float32, 'cpu')"),
        'memory no tensor':
            ('ValueError', 'recurrent_action: memory must be a (2, 39) float32 tensor on @, got ndarray'),
        'world slot ids, memory given':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'signal channels + no memory channels':
            ('NotImplementedError', "recurrent_action: no gradients through signal channels (signal_channels=2): the field's update has no adjoint"),
        'no memory channels + stock':
            ('ValueError', 'recurrent_action: an agent without memory channels (memory_channels=0) is differentiated by differentiable_action'),
        'stock + reflect':
            ('NotImplementedError', 'recurrent_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'reflect + decomposed medium':
            ('NotImplementedError', "recurrent_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'decomposed medium + fp16':
            ('NotImplementedError', 'memory_channels=2 on a decomposed medium (die_amd/dist.py): the standing plane is built for periodic single-tile planes only'),
        'fp16 + held memory no tensor':
            ('NotImplementedError', 'recurrent_action: fp32 fields only (this medium is torch.float16)'),
        'fp16 + memory of another shape':
            ('NotImplementedError', 'recurrent_action: fp32 fields only (this medium is torch.float16)'),
        'world slot ids + held memory no tensor':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'memory of another shape + world slot ids':
            ('ValueError', "recurrent_action: memory must be a (2, 39) float32 tensor on @, got ((2, 40), torch.float32, '@')"),
    },
    'agent.signalling_action': {
        'no signal channels':
            ('ValueError', 'signalling_action: an agent without signal channels (signal_channels=0) is differentiated by recurrent_action (memory channels) or differentiable_action'),
        'stock':
            ('NotImplementedError', 'signalling_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'reflect':
            ('NotImplementedError', "signalling_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'replicate':
            ('NotImplementedError', "signalling_action: boundary='replicate' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'decomposed medium':
            ('NotImplementedError', 'signal_channels=2 on a decomposed medium (die_amd/dist.py): the signal field is kept for periodic single-tile planes only'),
        'fp16':
            ('NotImplementedError', 'signalling_action: fp32 fields only (this medium is torch.float16)'),
        'signals of another shape':
            ('ValueError', "signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ((2, 13, 11), torch.float32, '@')"),
        'signals of another dtype':
            ('ValueError', "signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ((2, 13, 10), torch.float64, '@')"),
        'signals on another device':
            ('ValueError', "signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ((2, 13, 10), torch.float32, 'cpu')"),
        'signals no tensor':
            ('ValueError', 'signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ndarray'),
        'memory without memory channels':
            ('ValueError', 'signalling_action: memory given to an agent without memory channels (memory_channels=0)'),
        'world slot ids':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'held memory no tensor':
            ('ValueError', 'memory: a contiguous (2, N) float32 tensor on @'),
        'held memory of another dtype':
            ('ValueError', 'memory: a contiguous (2, N) float32 tensor on @'),
        'held memory of other slots':
            ('ValueError', 'memory holds 40 slots, the agents have 39: call reset_memory() to start blank with them'),
        'memory of another shape':
            ('ValueError', "signalling_action: memory must be a (2, 39) float32 tensor on @, got ((2, 40), torch.float32, '@')"),
        'memory of another dtype':
            ('ValueError', "signalling_action: memory must be a (2, 39) float32 tensor on @, got ((2, 39), torch.float64, '@')"),
        'memory on another device':
            ('ValueError', "signalling_action: memory must be a (2, 39) float32 tensor on @, got ((2, 39), torch.float32, 'cpu')"),
        'memory no tensor':
            ('ValueError', 'signalling_action: memory must be a (2, 39) float32 tensor on @, got ndarray'),
        'world slot ids, memory given':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'field of another shape':
            ('ValueError', 'signals holds a (14, 10) field on @, the medium is (13, 10) on @: call reset_signals() to start blank on it'),
        'no signal channels + stock':
            ('ValueError', 'signalling_action: an agent without signal channels (signal_channels=0) is differentiated by recurrent_action (memory channels) or differentiable_action'),
        'stock + reflect':
            ('NotImplementedError', 'signalling_action: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and the adjoint kernels do not take its kind'),
        'reflect + decomposed medium':
            ('NotImplementedError', "signalling_action: boundary='reflect' in differentiable mode: 'circular' or 'zeros' (sense() and forward() take all of ['circular', 'reflect', 'replicate', 'zeros'])"),
        'decomposed medium + fp16':
            ('NotImplementedError', 'signal_channels=2 on a decomposed medium (die_amd/dist.py): the signal field is kept for periodic single-tile planes only'),
        'fp16 + signals of another shape':
            ('NotImplementedError', 'signalling_action: fp32 fields only (this medium is torch.float16)'),
        'signals of another shape + memory without memory channels':
            ('ValueError', "signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ((2, 13, 11), torch.float32, '@')"),
        'signals no tensor + held memory no tensor':
            ('ValueError', 'signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ndarray'),
        'signals of another dtype + memory of another shape':
            ('ValueError', "signalling_action: signals must be a (2, 13, 10) float32 tensor on @, got ((2, 13, 10), torch.float64, '@')"),
        'world slot ids + held memory no tensor':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
        'memory of another shape + world slot ids':
            ('ValueError', "signalling_action: memory must be a (2, 39) float32 tensor on @, got ((2, 40), torch.float32, '@')"),
        'held memory of other slots + field of another shape':
            ('ValueError', 'memory holds 40 slots, the agents have 39: call reset_memory() to start blank with them'),
        'memory no tensor + field of another shape':
            ('ValueError', 'signalling_action: memory must be a (2, 39) float32 tensor on @, got ndarray'),
        'world slot ids, memory given + field of another shape':
            ('NotImplementedError', 'memory_channels=2 on a decomposed world (die_amd/dist.py): its slots carry world ids'),
    },
}


if __name__ == '__main__':
    _record()
