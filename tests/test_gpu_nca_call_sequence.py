"""The library calls of the NeuralAutomataAgent paths, pinned: which entry points `BatchedEnv.step`, the batched differentiable
calls and the stand-alone agent make, in which order, and which of their nullable arguments are null — the cases
tests/test_gpu_batch_step_path.py leaves out (wide stacks, the stock channel, memory channels, `action=`, `step_action`, births,
the gradients, the stand-alone agent) — and which refusal wins where a template is wide, has the stock channel and carries memory
at once.  The results of those calls are the business of the bit-for-bit files (test_gpu_nca_batch.py, test_gpu_nca_wide.py,
test_gpu_stock.py, test_gpu_memory.py, test_gpu_nca_grad_batch.py, test_gpu_nca_wide_grad_batch.py …).

A call is logged as (name, positions of the arguments that were None); the memory step also logs (memory_channels, with_stock)."""
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.functional import gather_scale_batch

pytestmark = pytest.mark.gpu

W, H, R = 32, 32, 4
STEPS = ('die_nca_env_step_batch', 'die_nca_env_step_batch_dropout', 'die_nca_env_step_batch_rows', 'die_nca_wide_env_step_batch',
         'die_nca_env_step_batch_stock', 'die_nca_wide_env_step_batch_stock', 'die_nca_wide_env_step_batch_memory')
RECORDED = STEPS + (
    'die_env_step_batch', 'die_env_step_batch_rows', 'die_agent_births_batch', 'die_food_flow_batch', 'die_food_flow_batch_masked',
    'die_stock_plane_batch', 'die_memory_planes_batch', 'die_gather_memory_batch',
    'die_nca_sense_batch_store', 'die_nca_wide_sense_batch_store', 'die_nca_backward_batch_workspace_bytes', 'die_nca_backward_batch',
    'die_nca_backward_batch_inputs', 'die_nca_wide_backward_batch_workspace_bytes', 'die_nca_wide_backward_batch',
    'die_gather_scale_batch', 'die_gather_scale_backward_batch', 'die_deposit_cells_batch', 'die_env_step_backward_batch',
    'die_stock_plane', 'die_memory_planes', 'die_conv2d', 'die_conv2d_dropout', 'die_conv2d_wide', 'die_gather_scale', 'die_gather_memory',
    'die_conv2d_backward', 'die_gather_scale_backward',
    # the stateful paths: memory and signal channels with gradients, stand-alone and batched
    'die_memory_cells', 'die_memory_cells_batch', 'die_signal_cells', 'die_signal_cells_batch', 'die_signal_step', 'die_signal_step_batch',
    'die_signal_step_backward', 'die_signal_step_backward_batch', 'die_memory_planes_backward', 'die_memory_planes_backward_batch',
    'die_gather_memory_backward', 'die_gather_memory_backward_batch', 'die_nca_wide_sense_batch_store_memory',
    'die_nca_wide_sense_batch_store_signal', 'die_nca_wide_backward_batch_memory', 'die_nca_wide_backward_batch_signal',
    'die_nca_wide_backward_batch_memory_workspace_bytes', 'die_nca_wide_backward_batch_signal_workspace_bytes',
    'die_conv2d_wide_backward', 'die_conv2d_wide_backward_workspace_bytes')
# argument positions (include/die_hip.h): the batched steps' action, mask and the two Dynamics tables; the memory step's M and with_stock
ACT, DROP, ROWS, ROWS_HOST, MEM_M, MEM_STOCK = 3, 9, 10, 11, 13, 16


@pytest.fixture
def calls(monkeypatch):
    """The RECORDED library calls made, in order: each attribute of the CDLL is wrapped to log the call and forward it."""
    log = []
    for name in RECORDED:
        def recorder(*args, _fn=getattr(_lib.lib, name), _name=name):
            entry = (_name, tuple(i for i, a in enumerate(args) if a is None))
            if _name == 'die_nca_wide_env_step_batch_memory':
                entry += ((args[MEM_M], args[MEM_STOCK]),)
            log.append(entry)
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, recorder)
    return log


def _dynamics(listed: bool = False, **kw):
    """One Dynamics, or R of them with two diffuse_sigma."""
    if not listed:
        return die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15, **kw)
    return [die.Dynamics(diffuse_sigma=(0.8, 0.5)[r % 2], init_agent_ratio=0.15, **kw) for r in range(R)]


WIDE = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='relu')
KINDS = {                                                   # template arguments, step entry point, (M, with_stock) of the memory call
    'narrow': (dict(kernel_sizes=(3,)), None, None),
    'wide': (WIDE, 'die_nca_wide_env_step_batch', None),
    'narrow_stock': (dict(kernel_sizes=(3,), with_stock_channel=True), 'die_nca_env_step_batch_stock', None),
    'wide_stock': (dict(WIDE, with_stock_channel=True), 'die_nca_wide_env_step_batch_stock', None),
    'memory': (dict(kernel_sizes=(3, 3), memory_channels=2), 'die_nca_wide_env_step_batch_memory', (2, 0)),
    'memory_stock': (dict(kernel_sizes=(3, 3), memory_channels=2, with_stock_channel=True), 'die_nca_wide_env_step_batch_memory', (2, 1)),
}


def _template(kind: str, p: float = 0.0, **kw):
    torch.manual_seed(5)
    return die.NeuralAutomataAgent(scale=0.01, deposit=2.0, boundary='circular', p_agent_dropout=p, **dict(KINDS[kind][0], **kw))


def _population(benv, kind: str, dropout: bool = False, episodes: int = 1):
    if dropout:
        return BatchedNeuralAutomataAgent(benv, _template(kind, 0.5), episodes=episodes, dropout_seed=3)
    return BatchedNeuralAutomataAgent(benv, _template(kind), episodes=episodes)


def _step_call(kind: str, listed: bool, dropout: bool, action: bool = False):
    """The one call of a step by the rules of the batched layer.  A narrow stack: the `_rows` entry point under per-replica
    Dynamics (its mask nullable), else the dropout one when a mask is active, else the plain one.  Every other kind has ONE entry
    point whose mask and two tables are nullable.  The action is null unless `step(action=...)` gave one."""
    name, memory = KINDS[kind][1:]
    nulls = [] if action else [ACT]
    if name is None:
        name = 'die_nca_env_step_batch' + ('_rows' if listed else '_dropout' if dropout else '')
        if listed and not dropout:
            nulls.append(DROP)
    else:
        nulls += ([] if dropout else [DROP]) + ([] if listed else [ROWS, ROWS_HOST])
    return (name, tuple(nulls)) + (() if memory is None else (memory,))


@pytest.mark.parametrize('dropout', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('listed', [False, True], ids=['one', 'listed'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_the_call_of_a_batched_step(calls, kind, listed, dropout):
    benv = BatchedEnv((W, H), _dynamics(listed), replicas=R, seed=3)
    assert not benv.per_replica and (benv._rows is not None) == listed
    pop = _population(benv, kind, dropout)
    assert pop._dropout() is not None if dropout else pop._dropout() is None
    builds = 'stock' in kind or 'memory' in kind                 # the step builds the env's stock planes (its standing planes)
    for step in (1, 2):
        del calls[:]
        benv.step(pop)
        assert calls == [_step_call(kind, listed, dropout)]
        assert benv._serial == step and benv._stock_serial == (step if builds else -1)
    torch.cuda.synchronize()
    assert (benv._steps, pop._calls, benv.epoch, pop.dropout_step) == (2, 2, 3, 2 if dropout else 0)


def test_the_call_of_a_batched_step_with_episodes(calls):
    benv = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
    pop = _population(benv, 'narrow', episodes=2)
    assert (pop.candidates, pop.episodes) == (2, 2)
    for _ in range(2):
        del calls[:]
        benv.step(pop)
        assert calls == [_step_call('narrow', False, False)]
    torch.cuda.synchronize()


def test_the_call_of_a_batched_step_that_records_the_action(calls):
    benv = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
    pop = _population(benv, 'narrow')
    buf = torch.zeros((3, R, benv.Nmax), dtype=torch.float32, device=benv.device)
    for _ in range(2):
        del calls[:]
        benv.step(pop, action=buf)
        assert calls == [_step_call('narrow', False, False, action=True)]
    torch.cuda.synchronize()
    assert buf.any()


def test_step_action_after_a_stock_step_makes_the_next_one_start_its_planes_over(calls):
    benv = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
    pop = _population(benv, 'narrow_stock')
    buf = torch.zeros((3, R, benv.Nmax), dtype=torch.float32, device=benv.device)
    benv.step(pop)
    assert (benv._serial, benv._stock_serial) == (1, 1)         # this step built the planes: the next stock step may build on top
    del calls[:]
    benv.step_action(buf)
    assert calls == [('die_env_step_batch', ())]
    assert (benv._serial, benv._stock_serial) == (2, 1)         # … but not after this one: `_stock_planes` zeroes them first
    stock = benv._stock
    stock.fill_(-1)
    assert benv._stock_planes() is stock and not stock.any()
    del calls[:]
    benv.step(pop)
    assert calls == [_step_call('narrow_stock', False, False)]
    assert (benv._serial, benv._stock_serial) == (3, 3)
    torch.cuda.synchronize()
    assert (benv._steps, pop._calls, benv.epoch) == (3, 2, 4)


def test_births_are_a_step_s_last_call(calls):
    benv = BatchedEnv((W, H), _dynamics(agents_die=True, agents_born=True), replicas=R, seed=3, max_agents=400)
    pop = _population(benv, 'narrow')
    for _ in range(2):
        del calls[:]
        benv.step(pop)
        assert calls == [_step_call('narrow', False, False), ('die_agent_births_batch', ())]
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- batched gradients
def _gradient_calls(call: str, dropout: bool, to_node: bool):
    """(forward, backward) of one differentiable call.  The store call's masked planes and mask are null without a mask; the
    backward's mask likewise.  A chem node that needs a gradient picks die_nca_backward_batch_inputs for a narrow stack and a
    non-null `grad_in` (position 11) for a wide one."""
    store = () if dropout else (5, 6)
    drop = () if dropout else (8,)
    if call == 'forward_device':
        forward = [('die_nca_wide_sense_batch_store', store)]
        backward = [('die_nca_wide_backward_batch_workspace_bytes', ()), ('die_nca_wide_backward_batch', drop + (() if to_node else (11,)))]
    else:
        forward = [('die_nca_sense_batch_store', store)]
        backward = [('die_nca_backward_batch_workspace_bytes', ()),
                    ('die_nca_backward_batch_inputs' if to_node else 'die_nca_backward_batch', drop)]
    if call == 'differentiable_action':
        forward, backward = forward + [('die_gather_scale_batch', ())], [('die_gather_scale_backward_batch', ())] + backward
    return forward, backward


@pytest.mark.parametrize('dropout', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('node', ['none', 'leaf', 'stepped'])
@pytest.mark.parametrize('call', ['differentiable_sense', 'differentiable_action', 'forward_device'])
def test_the_calls_of_a_batched_gradient(calls, call, node, dropout):
    benv = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
    wide = call == 'forward_device'
    pop = _population(benv, 'wide' if wide else 'narrow', dropout)
    p = pop.parameters.detach().clone().requires_grad_()
    earlier = []                                                 # the backward of the graph behind the chem node, which runs afterwards
    if node == 'leaf':
        assert not benv.differentiable_chem().requires_grad
    elif node == 'stepped':                                      # a node that needs a gradient: the step's action has a graph
        action = gather_scale_batch(pop.forward_device(p), pop) if wide else pop.differentiable_action(p)
        benv.differentiable_step(action)
        assert benv.chem_node.requires_grad
        first = _gradient_calls('forward_device' if wide else 'differentiable_sense', dropout, False)[1]
        earlier = [('die_env_step_backward_batch', (6, 7)), ('die_gather_scale_backward_batch', ())] + first
    step0 = pop.dropout_step
    forward, backward = _gradient_calls(call, dropout, node == 'stepped')
    del calls[:]
    out = getattr(pop, call)(p)
    assert calls == forward
    assert pop.dropout_step == step0 + (1 if dropout else 0)
    del calls[:]
    out.sum().backward()
    torch.cuda.synchronize()
    assert calls == backward + earlier
    assert p.grad is not None and tuple(p.grad.shape) == (R, pop.P)


# ---------------------------------------------------------------------------------------------------- the stand-alone agent
ALONE = {                                                   # template arguments (two layers: a last one and one that is not)
    'narrow': dict(kernel_sizes=(3, 3)),
    'narrow_dropout': dict(kernel_sizes=(3, 3), p_agent_dropout=0.5, dropout_seed=3),
    'wide': WIDE,
    'stock': dict(kernel_sizes=(3, 3), with_stock_channel=True),
    'memory': dict(kernel_sizes=(3, 3), memory_channels=2),
    'memory_stock': dict(kernel_sizes=(3, 3), memory_channels=2, with_stock_channel=True),
}


def _alone(kind: str):
    torch.manual_seed(5)
    env = die.Env((W, H), _dynamics(), seed=3, max_agents='alive')
    return env, die.NeuralAutomataAgent(scale=0.01, deposit=2.0, boundary='circular', **ALONE[kind]).to(env.device)


def _sense_calls(kind: str):
    """`sense`: the standing plane where the stock channel or memory needs it, the memory's expand, then a launch per layer —
    the wide layer call (its mask, position 12, null) for a wide stack, else die_conv2d with the last layer masked in its launch."""
    build = [('die_stock_plane', ())] if 'stock' in kind or 'memory' in kind else []
    build += [('die_memory_planes', ())] if 'memory' in kind else []
    if kind == 'wide' or 'memory' in kind:
        return build + [('die_conv2d_wide', (12,))] * 2
    return build + [('die_conv2d', ()), ('die_conv2d_dropout' if kind == 'narrow_dropout' else 'die_conv2d', ())]


@pytest.mark.parametrize('kind', list(ALONE))
def test_the_calls_of_a_stand_alone_sense_and_forward(calls, kind):
    env, ag = _alone(kind)
    del calls[:]
    ag.sense(env.medium, env.agents)
    assert calls == _sense_calls(kind)
    del calls[:]
    ag.forward(env._get_current_obs)
    assert calls == _sense_calls(kind) + [('die_gather_scale', ())] + ([('die_gather_memory', ())] if 'memory' in kind else [])
    torch.cuda.synchronize()
    assert ag.dropout_step == (2 if kind == 'narrow_dropout' else 0)


@pytest.mark.parametrize('kind', ['narrow', 'narrow_dropout'])
def test_the_calls_of_a_stand_alone_differentiable_sense(calls, kind):
    """Forward: every layer unmasked, then the last once more masked.  Backward, last layer first (die_conv2d_backward: grad_in 10,
    tanh_out 11, mask 12): the last layer has its tanh planes and, with a mask, the mask; the first has neither and, without a
    chem node, no `grad_in`."""
    env, ag = _alone(kind)
    masked = kind == 'narrow_dropout'
    del calls[:]
    out = ag.differentiable_sense(env.medium)
    assert calls == [('die_conv2d', ())] * 2 + ([('die_conv2d_dropout', ())] if masked else [])
    del calls[:]
    out.sum().backward()
    torch.cuda.synchronize()
    assert calls == [('die_conv2d_backward', () if masked else (12,)), ('die_conv2d_backward', (10, 11, 12))]
    assert ag.dropout_step == (1 if masked else 0)


# ---------------------------------------------------------------------------------------------------- the stateful calls
STATEFUL = {                                                # the call, K, M
    'recurrent': ('recurrent_action', 0, 2),
    'signalling': ('signalling_action', 2, 0),
    'signalling_memory': ('signalling_action', 2, 2),
}


@pytest.mark.parametrize('dropout', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('node', ['none', 'stepped'])
@pytest.mark.parametrize('kind', list(STATEFUL))
@pytest.mark.parametrize('who', ['alone', 'population'])
def test_the_calls_of_two_chained_stateful_calls(calls, who, kind, node, dropout):
    """Two calls, the second given the first's `memory_next` / `signals_next`, then `backward()` on the sum of everything returned:
    the calls of each forward, of the `differentiable_step` between them ('stepped': the env carries a chem node that needs a
    gradient) and of the backward, as literals (STATEFUL_CALLS, below).  The docstrings' counts are the cross-check: a two-layer
    population's `recurrent_action` makes 4 calls forward (L + 5 launches: the build and the record, the expand, the stack's L,
    the two read-outs), its stack's adjoint is given `grad_in` wherever a memory with a graph or a chem node asks for it, and the
    K·R planes of a population's field take ONE die_signal_step_backward_batch per link."""
    name, K, M = STATEFUL[kind]
    kw = dict(kernel_sizes=(3, 3), memory_channels=M, p_agent_dropout=0.5 if dropout else 0.0, **(dict(signal_channels=K) if K else {}))
    seed = 3 if dropout else None
    torch.manual_seed(5)
    if who == 'alone':
        env = die.Env((W, H), _dynamics(), seed=3, max_agents='alive')
        ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, boundary='circular', dropout_seed=seed, **kw).to(env.device)
        call = lambda state: getattr(ag, name)(env._get_current_obs, *state)
    else:
        env = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
        pop = BatchedNeuralAutomataAgent(env, die.NeuralAutomataAgent(scale=0.01, deposit=2.0, boundary='circular', **kw), dropout_seed=seed)
        assert (pop._dropout() is not None) == dropout
        p = pop.parameters.detach().clone().requires_grad_()
        call = lambda state: getattr(pop, name)(*state, p)
    if node == 'stepped':
        assert not env.differentiable_chem().requires_grad
    state = (None,) * (2 if K else 1)                            # (memory,) / (signals, memory)
    log, total = [], 0
    for link in range(2):
        del calls[:]
        out = call(state)
        log.append(list(calls))
        total = total + sum(t.sum() for t in out if t is not None)
        state = out[1:]
        if node == 'stepped' and link == 0:
            del calls[:]
            env.differentiable_step(out[0])
            log.append(list(calls))
    del calls[:]
    total.backward()
    torch.cuda.synchronize()
    log.append(list(calls))
    print('    %r: %r,' % ('%s-%s-%s-%s' % (who, kind, node, 'dropout' if dropout else 'plain'), log))
    assert log == STATEFUL_CALLS['%s-%s-%s-%s' % (who, kind, node, 'dropout' if dropout else 'plain')]
    assert (ag if who == 'alone' else pop).dropout_step == (2 if dropout else 0)


# ---------------------------------------------------------------------------------------------------- refusals
MEMORY = ('{what}: no gradients through memory channels (memory_channels=2): the read-out into the memory and the expand onto the '
          'field have no adjoint')
WIDE_STACK = ('{what}: no gradients for a wide stack (hidden_channels / hidden_activation): the adjoint kernels take the narrow '
              'layers only')
STOCK = ('{what}: no gradients with the stock channel (with_stock_channel=True): its plane is piecewise constant in the weights and '
         'the adjoint kernels do not take its kind')
COMBINATIONS = [(wide, stock, memory) for wide in (False, True) for stock in (False, True) for memory in (False, True)
                if wide or stock or memory]


def _refused(call, message: str):
    with pytest.raises(NotImplementedError) as err:
        call()
    assert type(err.value) is NotImplementedError and str(err.value) == message


@pytest.mark.parametrize('wide,stock,memory', COMBINATIONS)
def test_which_refusal_of_a_differentiable_call_wins(calls, wide, stock, memory):
    """Memory before the wide stack before the stock channel — memory channels make a wide stack whatever else is set — and
    `forward_device`, which takes a wide stack, memory before the stock channel.  All before any launch and before `dropout_step`
    moves."""
    kw = dict(kernel_sizes=(3, 3), p_agent_dropout=0.5, **(dict(hidden_channels=8, hidden_activation='relu') if wide else {}),
              **(dict(with_stock_channel=True) if stock else {}), **(dict(memory_channels=2) if memory else {}))
    torch.manual_seed(5)
    env = die.Env((W, H), _dynamics(), seed=3, max_agents='alive')
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, dropout_seed=3, **kw).to(env.device)
    benv = BatchedEnv((W, H), _dynamics(), replicas=R, seed=3)
    pop = BatchedNeuralAutomataAgent(benv, ag, dropout_seed=3)
    assert pop._dropout() is not None and ag.model.wide == (wide or memory)
    wins = MEMORY if memory else WIDE_STACK if wide else STOCK
    del calls[:]
    _refused(lambda: ag.differentiable_sense(env.medium), wins.format(what='differentiable_sense'))
    _refused(lambda: ag.differentiable_action(env._get_current_obs), wins.format(what='differentiable_action'))
    _refused(lambda: pop.differentiable_sense(), wins.format(what='differentiable mode'))
    _refused(lambda: pop.differentiable_action(), wins.format(what='differentiable mode'))
    if memory or stock:                                          # (a wide stack alone is what forward_device takes)
        _refused(lambda: pop.forward_device(), (MEMORY if memory else STOCK).format(what='forward_device'))
    assert calls == [] and (ag.dropout_step, pop.dropout_step) == (0, 0)
    assert ag.memory is None and (pop.memory is None or not pop.memory.any())


# ---------------------------------------------------------------------------------------------------- the recorded stateful calls
# per case: the first call's forward, ['stepped': the differentiable_step between,] the second call's forward, the backward
STATEFUL_CALLS = {
    'alone-recurrent-none-plain': [
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-recurrent-none-dropout': [
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-recurrent-stepped-plain': [
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [],
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-recurrent-stepped-dropout': [
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [],
        [('die_stock_plane', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling-none-plain': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()),
         ('die_signal_step', ())],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()),
         ('die_signal_step', ())],
        [('die_signal_step_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling-none-dropout': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_signal_step', ())],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_signal_step', ())],
        [('die_signal_step_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling-stepped-plain': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()),
         ('die_signal_step', ())],
        [],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()),
         ('die_signal_step', ())],
        [('die_signal_step_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling-stepped-dropout': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_signal_step', ())],
        [],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_conv2d_wide', (12,)), ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)),
         ('die_gather_scale', ()), ('die_signal_step', ())],
        [('die_signal_step_backward', ()), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14)),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling_memory-none-plain': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()), ('die_memory_planes_backward', ())],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_signal_step_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14)), ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling_memory-none-dropout': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()),
         ('die_memory_planes_backward', ())],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()),
         ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_signal_step_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14)), ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling_memory-stepped-plain': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()), ('die_memory_planes_backward', ())],
        [],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()), ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_signal_step_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14)), ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (14,)), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'alone-signalling_memory-stepped-dropout': [
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()),
         ('die_memory_planes_backward', ())],
        [],
        [('die_stock_plane', ()), ('die_signal_cells', ()), ('die_memory_cells', ()), ('die_memory_planes', ()), ('die_conv2d_wide', (12,)),
         ('die_conv2d_wide', ()), ('die_conv2d_wide', (12,)), ('die_gather_scale', ()), ('die_signal_step', ()),
         ('die_memory_planes_backward', ())],
        [('die_gather_memory_backward', ()), ('die_signal_step_backward', ()), ('die_gather_scale_backward', ()),
         ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', (8, 14)), ('die_memory_planes_backward', ()), ('die_gather_memory_backward', ()),
         ('die_signal_step_backward', (6,)), ('die_gather_scale_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()),
         ('die_conv2d_wide_backward', ()), ('die_conv2d_wide_backward_workspace_bytes', ()), ('die_conv2d_wide_backward', (8, 14, 16))],
    ],
    'population-recurrent-none-plain': [
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', (5, 6)), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', (5, 6)), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', (8,)),
         ('die_memory_planes_backward_batch', ()), ('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', (8, 11))],
    ],
    'population-recurrent-none-dropout': [
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', ()), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', ()), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', ()),
         ('die_memory_planes_backward_batch', ()), ('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', (11,))],
    ],
    'population-recurrent-stepped-plain': [
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', (5, 6)), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', (5, 6)), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', (8,)),
         ('die_memory_planes_backward_batch', ()), ('die_env_step_backward_batch', (6, 7)), ('die_gather_scale_backward_batch', ()),
         ('die_gather_memory_backward_batch', ()), ('die_nca_wide_backward_batch_memory_workspace_bytes', ()),
         ('die_nca_wide_backward_batch_memory', (8, 11))],
    ],
    'population-recurrent-stepped-dropout': [
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', ()), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_memory', ()), ('die_gather_scale_batch', ()), ('die_memory_planes_backward_batch', ())],
        [('die_gather_scale_backward_batch', ()), ('die_gather_memory_backward_batch', ()),
         ('die_nca_wide_backward_batch_memory_workspace_bytes', ()), ('die_nca_wide_backward_batch_memory', ()),
         ('die_memory_planes_backward_batch', ()), ('die_env_step_backward_batch', (6, 7)), ('die_gather_scale_backward_batch', ()),
         ('die_gather_memory_backward_batch', ()), ('die_nca_wide_backward_batch_memory_workspace_bytes', ()),
         ('die_nca_wide_backward_batch_memory', (11,))],
    ],
    'population-signalling-none-plain': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (5, 6, 7)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (5, 6, 7)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8, 13)),
         ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8, 11, 13))],
    ],
    'population-signalling-none-dropout': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (7,)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (7,)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (13,)),
         ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (11, 13))],
    ],
    'population-signalling-stepped-plain': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (5, 6, 7)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (5, 6, 7)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8, 13)),
         ('die_env_step_backward_batch', (6, 7)), ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8, 11, 13))],
    ],
    'population-signalling-stepped-dropout': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (7,)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_nca_wide_sense_batch_store_signal', (7,)),
         ('die_gather_scale_batch', ()), ('die_signal_step_batch', ())],
        [('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (13,)),
         ('die_env_step_backward_batch', (6, 7)), ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (11, 13))],
    ],
    'population-signalling_memory-none-plain': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', (5, 6)), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', (5, 6)), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8,)),
         ('die_memory_planes_backward_batch', ()), ('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', (7,)),
         ('die_gather_scale_backward_batch', ()), ('die_nca_wide_backward_batch_signal_workspace_bytes', ()),
         ('die_nca_wide_backward_batch_signal', (8, 11))],
    ],
    'population-signalling_memory-none-dropout': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', ()), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', ()), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', ()),
         ('die_memory_planes_backward_batch', ()), ('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', (7,)),
         ('die_gather_scale_backward_batch', ()), ('die_nca_wide_backward_batch_signal_workspace_bytes', ()),
         ('die_nca_wide_backward_batch_signal', (11,))],
    ],
    'population-signalling_memory-stepped-plain': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', (5, 6)), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', (5, 6)), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8,)),
         ('die_memory_planes_backward_batch', ()), ('die_env_step_backward_batch', (6, 7)), ('die_gather_memory_backward_batch', ()),
         ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (8, 11))],
    ],
    'population-signalling_memory-stepped-dropout': [
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', ()), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_env_step_batch', ()), ('die_deposit_cells_batch', ())],
        [('die_stock_plane_batch', ()), ('die_signal_cells_batch', ()), ('die_memory_cells_batch', ()), ('die_memory_planes_batch', ()),
         ('die_nca_wide_sense_batch_store_signal', ()), ('die_gather_scale_batch', ()), ('die_signal_step_batch', ()),
         ('die_memory_planes_backward_batch', ())],
        [('die_gather_memory_backward_batch', ()), ('die_signal_step_backward_batch', ()), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', ()),
         ('die_memory_planes_backward_batch', ()), ('die_env_step_backward_batch', (6, 7)), ('die_gather_memory_backward_batch', ()),
         ('die_signal_step_backward_batch', (7,)), ('die_gather_scale_backward_batch', ()),
         ('die_nca_wide_backward_batch_signal_workspace_bytes', ()), ('die_nca_wide_backward_batch_signal', (11,))],
    ],
}
