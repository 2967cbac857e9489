"""The host-side rules of every entry point that takes a die_nca_batch, and of the batched stock / memory calls that take a
die_batch alone, written down as they stand: one table of single faults applied to every call it is a fault for, the return code
and the FULL last-error text of each, a dozen double faults (which of two rules speaks first), and what the byte queries return
and leave in the last-error text.  CPU only: fake pointers, every call is refused on the host before anything is launched.

The expected values (EXPECT_*, at the end of the file) are literals recorded from the library — `python -m
tests.test_nca_stack_rules_cpu` prints them, on a machine WITHOUT a GPU only: recording also runs the unfaulted calls to see that
they pass every check, and those reach the launch.  The test itself makes only the calls listed in the literals, all refusals.
A text is stored with the call's own name replaced by `@`, and the calls that answer alike are listed together."""
import ctypes as C
import os
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, R, N = 24, 72, 4, 10           # the smallest world at which every rule is reachable: 2 x 2 tiles, H % 4 == 0
CELLS = W * H
MEM = 2                              # memory channels of the *_memory calls
TANH, RELU = 1, 2
REFLECT, REPLICATE = 2, 3
SLOT_MASK = 0x07FFFFFF               # DIE_OWNER_SLOT_MASK: agent_stride goes up to SLOT_MASK - 1
FAKE = 1 << 28                       # never dereferenced


def _buf(i):
    """fake buffer i, 4 MiB from the next: larger than anything a call lays out at this size"""
    return FAKE + (i << 22)


OWNER, FOOD, CHEM, CHEM_NEXT, WEIGHTS, SCRATCH, STORE, GSENSE, GRAD, WORK, STOCK, MEMORY, MEMPLANES, RESULTS, WS, X, Y, ALIVE, AFOOD, \
    REC0, REC1, ROWS = (_buf(i) for i in range(22))


@pytest.fixture(scope='module')
def lib():
    return _lib()


def _lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the calls
# kind: 'narrow' / 'wide' (a die_nca_batch of that kind) or None (a die_batch alone); group: what else the call takes
CALLS = {
    'n.step': dict(fn='die_nca_env_step_batch', kind='narrow', group='step'),
    'n.step_dropout': dict(fn='die_nca_env_step_batch_dropout', kind='narrow', group='step'),
    'n.step_rows': dict(fn='die_nca_env_step_batch_rows', kind='narrow', group='step'),
    'n.step_stock': dict(fn='die_nca_env_step_batch_stock', kind='narrow', group='step', stock=True),
    'w.step': dict(fn='die_nca_wide_env_step_batch', kind='wide', group='step'),
    'w.step_stock': dict(fn='die_nca_wide_env_step_batch_stock', kind='wide', group='step', stock=True),
    'w.step_memory': dict(fn='die_nca_wide_env_step_batch_memory', kind='wide', group='step', memory=MEM),
    'w.step_memory+stock': dict(fn='die_nca_wide_env_step_batch_memory', kind='wide', group='step', memory=MEM, stock=True),
    'n.store': dict(fn='die_nca_sense_batch_store', kind='narrow', group='store'),
    'w.store': dict(fn='die_nca_wide_sense_batch_store', kind='wide', group='store'),
    'w.store_memory': dict(fn='die_nca_wide_sense_batch_store_memory', kind='wide', group='store', memory=MEM),
    'n.adjoint': dict(fn='die_nca_backward_batch', kind='narrow', group='adjoint'),
    'n.adjoint_inputs': dict(fn='die_nca_backward_batch_inputs', kind='narrow', group='adjoint'),
    'w.adjoint': dict(fn='die_nca_wide_backward_batch', kind='wide', group='adjoint'),
    'w.adjoint_memory': dict(fn='die_nca_wide_backward_batch_memory', kind='wide', group='adjoint', memory=MEM),
    'stock_plane': dict(fn='die_stock_plane_batch', kind=None, group='slots', planes=True),
    'memory_planes': dict(fn='die_memory_planes_batch', kind=None, group='slots', planes=True),
    'gather_memory': dict(fn='die_gather_memory_batch', kind=None, group='slots', planes=True),
    'memory_cells': dict(fn='die_memory_cells_batch', kind=None, group='slots', planes=True),
    'memory_planes_adjoint': dict(fn='die_memory_planes_backward_batch', kind=None, group='slots', planes=False),
    'gather_memory_adjoint': dict(fn='die_gather_memory_backward_batch', kind=None, group='slots', planes=False),
}
# the byte queries: the scalar ones take (W, H, replicas, n_layers[, max_channels]), the others the stack itself
QUERIES = {
    'die_nca_batch_scratch_bytes': dict(kind='narrow', scalar=True),
    'die_nca_sense_batch_store_bytes': dict(kind='narrow', scalar=True),
    'die_nca_backward_batch_workspace_bytes': dict(kind='narrow', scalar=True),
    'die_nca_wide_batch_scratch_bytes': dict(kind='wide', scalar=True),
    'die_nca_wide_sense_batch_store_bytes': dict(kind='wide', scalar=True),
    'die_nca_wide_backward_batch_workspace_bytes': dict(kind='wide', scalar=False),
    'die_nca_wide_backward_batch_memory_workspace_bytes': dict(kind='wide', scalar=False, memory=MEM),
}
EPISODES = (0, 2)


def _config(spec, episodes):
    """the unfaulted arguments of a call: a stack of two layers, (3 -> 3, 3 -> 3) narrow and (3 -> 8, 8 -> 3) wide, with `memory`
    planes more into layer 0 and out of the last layer and the stock plane as one more input"""
    mem, extra = spec.get('memory', 0), spec.get('memory', 0) + (1 if spec.get('stock') else 0)
    mid = 3 if spec.get('kind') == 'narrow' else 8
    layers = [dict(k=3, cin=3 + extra, cout=mid, act=TANH if spec.get('kind') == 'wide' else 0, weights=WEIGHTS),
              dict(k=3, cin=mid, cout=3 + mem, act=TANH if spec.get('kind') == 'wide' else 0, weights=WEIGHTS + (1 << 20))]
    return dict(W=W, H=H, replicas=R, episodes=episodes, pad=0, agent_channel=1, sense_epoch=1, dtype=None, food=FOOD, layers=layers,
                n_layers=None, null_stack=False, null_layers=False, scratch_short=0, plane_stride=None, agent_stride=N, n=[N] * 64,
                maxc=4 if spec.get('kind') == 'narrow' else 32)


def _stride(layer):
    return layer.get('stride', layer['cout'] * layer['cin'] * layer['k'] * layer['k'])


def _structs(L, spec, cfg):
    cells = cfg['W'] * cfg['H']
    m = L.Medium(cfg['W'], cfg['H'], L.DIE_F32 if cfg['dtype'] is None else cfg['dtype'], 2, OWNER, cfg['food'], CHEM, CHEM_NEXT,
                 0, 0, 0, 0, 0, 0, 0, 0, None)
    arr = (L.NcaLayer * max(len(cfg['layers']), L.NCA_MAX_LAYERS + 1))(
        *[L.NcaLayer(y['k'], y['cin'], y['cout'], y['act'], y['weights'], _stride(y)) for y in cfg['layers']])
    n_layers = len(cfg['layers']) if cfg['n_layers'] is None else cfg['n_layers']
    cmax = max(y['cout'] for y in cfg['layers'])
    if spec.get('kind') == 'wide':
        scratch = 2 * cfg['replicas'] * cmax * cells * 4
    else:
        scratch = 2 * cfg['replicas'] * 4 * cells * 4
    nca = L.NcaBatch(n_layers, cfg['pad'], cfg['agent_channel'], cfg['sense_epoch'], None if cfg['null_layers'] else arr,
                     (C.c_float * 3)(0.01, 0.01, 2.0), cfg['episodes'], SCRATCH, scratch - cfg['scratch_short'])
    b = L.Batch(cfg['replicas'], 0, cells if cfg['plane_stride'] is None else cfg['plane_stride'], cfg['agent_stride'], 1,
                (C.c_int64 * 64)(*cfg['n']))
    return m, arr, nca, b


def _invoke(L, name, cfg):
    """the call `name` with the arguments of cfg: its return code"""
    spec = CALLS[name]
    name = spec['fn']
    fn = getattr(L.lib, name)
    m, arr, nca, b = _structs(L, spec, cfg)
    cells, reps, mem = cfg['W'] * cfg['H'], cfg['replicas'], spec.get('memory', 0)
    pm, pb, pn = C.byref(m), C.byref(b), None if cfg['null_stack'] else C.byref(nca)
    a = L.Agents(N, X, Y, ALIVE, AFOOD, None)
    if spec['group'] == 'step':
        d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
        rows_host = (L.DynamicsRow * 64)()
        for r in range(64):
            rows_host[r].radius = 3
        head = (pm, C.byref(a), pn, None, C.byref(d), pb, RESULTS, WS, 64 * L.lib.die_batch_workspace_bytes(1))
        rows = (ROWS, rows_host)
        if name == 'die_nca_env_step_batch':
            return fn(*head, None)
        if name == 'die_nca_env_step_batch_dropout':
            return fn(*head, C.byref(L.NcaDropout(0.25, 7, 1, 0, 0)), None)
        if spec.get('memory'):
            return fn(*head, None, *rows, STOCK, mem, MEMORY, MEMPLANES, int(bool(spec.get('stock'))), None)
        if spec.get('stock'):
            return fn(*head, None, *rows, STOCK, None)
        return fn(*head, None, *rows, None)
    cmax = max(y['cout'] for y in cfg['layers']) if spec['kind'] else 0
    chan = 4 if spec['kind'] == 'narrow' else cmax
    if spec['group'] == 'store':
        tail = (MEMPLANES, mem, None) if mem else (None,)
        return fn(pm, pb, pn, STORE, 2 * max(reps, 1) * chan * cells * 4, None, None, *tail)
    if spec['group'] == 'adjoint':
        row = sum(_stride(y) for y in cfg['layers'])
        head = (pm, pb, pn, STORE, GSENSE, (3 + mem) * cells, GRAD, row, None, WORK, 1 << 22)
        if name == 'die_nca_backward_batch':
            return fn(*head, None)
        if name == 'die_nca_backward_batch_inputs':
            return fn(*head, REC0, 4 * cells, None)
        if mem:
            return fn(*head, None, 0, MEMPLANES, mem, None)
        return fn(*head, None, 0, None)
    if name == 'die_stock_plane_batch':
        return fn(pm, C.byref(a), pb, 1, STOCK, None)
    if name == 'die_memory_planes_batch':
        return fn(pm, pb, STOCK, 1, MEM, MEMORY, cfg['agent_stride'], MEMPLANES, None)
    if name == 'die_gather_memory_batch':
        return fn(pm, C.byref(a), pb, MEM, MEMPLANES, cells, MEM * cells, MEMORY, cfg['agent_stride'], None)
    if name == 'die_memory_cells_batch':
        return fn(pm, C.byref(a), pb, STOCK, 1, REC0, REC1, None)
    if name == 'die_memory_planes_backward_batch':
        return fn(cfg['W'], cfg['H'], MEM, pb, REC0, MEMPLANES, cells, MEM * cells, MEMORY, cfg['agent_stride'], None)
    if name == 'die_gather_memory_backward_batch':
        return fn(cfg['W'], cfg['H'], MEM, pb, REC0, MEMORY, cfg['agent_stride'], MEMPLANES, cells, MEM * cells, None)
    raise KeyError(name)


SENTINEL = b'die_dropout_mask: null argument'
UNTOUCHED = SENTINEL.decode()      # a query that leaves the last-error text alone


def _query(L, name, cfg):
    """a byte query with the arguments of cfg, after a refusal whose text is known: (the value, the last-error text afterwards)"""
    spec = QUERIES[name]
    fn = getattr(L.lib, name)
    m, arr, nca, b = _structs(L, spec, cfg)
    n_layers = len(cfg['layers']) if cfg['n_layers'] is None else cfg['n_layers']
    assert L.lib.die_dropout_mask(0, 0, None, 0, 0, None, None) == -1 and L.lib.die_last_error() == SENTINEL
    if spec['scalar']:
        cmax = max(y['cout'] for y in cfg['layers'])
        value = fn(cfg['W'], cfg['H'], cfg['replicas'], n_layers, *((cmax,) if spec['kind'] == 'wide' else ()))
    else:
        pn = None if cfg['null_stack'] else C.byref(nca)
        value = fn(cfg['W'], cfg['H'], cfg['replicas'], pn, *((spec['memory'],) if spec.get('memory') else ()))
    return value, L.lib.die_last_error()


# ------------------------------------------------------------------------------------------------ the faults
# name -> (the calls it is a fault for, what it changes).  A fault is applied only where the call refuses it: a call that takes
# the faulted arguments would launch.
def _nca(spec):
    return spec['kind'] is not None


def _layer(i, **kw):
    return lambda cfg, spec: cfg['layers'][i].update(kw)


def _set(**kw):
    return lambda cfg, spec: cfg.update(kw)


def _cout0(cfg, spec):                                   # one past the kind's maximum, the chain kept whole
    cfg['layers'][0]['cout'] = cfg['layers'][1]['cin'] = cfg['maxc'] + 1


def _n(r, value):
    def change(cfg, spec):
        cfg['n'][r] = cfg['agent_stride'] + 1 if value is None else value
    return change


FAULTS = {
    'null stack': (_nca, _set(null_stack=True)),
    'null layers': (_nca, _set(null_layers=True)),
    '0 layers': (_nca, _set(n_layers=0)),
    'one layer too many': (_nca, _set(n_layers=9)),
    'bad padding mode': (_nca, _set(pad=4)),
    'with_agent_channel 2': (_nca, _set(agent_channel=2)),
    'episodes 3': (_nca, _set(episodes=3)),
    '0 replicas': (lambda s: True, _set(replicas=0)),
    '65 replicas': (lambda s: True, _set(replicas=65)),
    'kernel size 2': (_nca, _layer(0, k=2)),
    'kernel size 7': (lambda s: s['kind'] == 'wide', _layer(0, k=7)),
    'kernel size 9': (lambda s: s['kind'] == 'narrow', _layer(0, k=9)),
    'cin breaks the chain': (_nca, lambda cfg, spec: cfg['layers'][1].update(cin=cfg['layers'][1]['cin'] + 1)),
    'cout past the maximum': (_nca, _cout0),
    'bad activation': (lambda s: s['kind'] == 'wide', _layer(0, act=3)),
    'last layer not tanh': (lambda s: s['kind'] == 'wide', _layer(1, act=RELU)),
    'null weights': (_nca, _layer(0, weights=None)),
    'weight_stride one short': (_nca, lambda cfg, spec: cfg['layers'][0].update(stride=_stride(cfg['layers'][0]) - 1)),
    'reflect on one cell': (_nca, _set(pad=REFLECT, W=1)),
    'last layer one plane short': (_nca, lambda cfg, spec: cfg['layers'][1].update(cout=cfg['layers'][1]['cout'] - 1)),
    'scratch one byte short': (lambda s: s.get('group') == 'step', _set(scratch_short=1)),
    'plane_stride one cell short': (lambda s: s.get('group') in ('step', 'store', 'adjoint') or s.get('planes'), _set(plane_stride=CELLS - 1)),
    'agent_stride 0': (lambda s: 'group' in s, _set(agent_stride=0)),
    'agent_stride past the slot mask': (lambda s: s.get('group') == 'slots', _set(agent_stride=SLOT_MASK)),
    'n[1] = -1': (lambda s: 'group' in s, _n(1, -1)),
    'n[3] past agent_stride': (lambda s: 'group' in s, _n(3, None)),
    'bad dtype': (lambda s: s.get('group') in ('step', 'store', 'adjoint'), _set(dtype=7)),
    'null food plane': (lambda s: s.get('group') in ('step', 'store', 'adjoint'), _set(food=None)),
    'sense_epoch 0': (lambda s: s.get('group') in ('step', 'store', 'adjoint'), _set(sense_epoch=0)),
    'reflect on the adjoint': (lambda s: s.get('group') == 'adjoint' or s.get('scalar') is False, _set(pad=REFLECT)),
    'replicate on the adjoint': (lambda s: s.get('group') == 'adjoint' or s.get('scalar') is False, _set(pad=REPLICATE)),
}
# the faults a scalar query can be given at all
SCALAR_FAULTS = ('0 layers', 'one layer too many', '0 replicas', '65 replicas', 'cout past the maximum')
# which of two rules speaks first: (call, fault, fault)
DOUBLES = [
    ('n.step', 'scratch one byte short', 'kernel size 9'),
    ('w.step', 'scratch one byte short', 'kernel size 7'),
    ('w.step_memory', 'scratch one byte short', 'last layer one plane short'),
    ('n.store', 'plane_stride one cell short', 'kernel size 2'),
    ('w.store', 'plane_stride one cell short', 'kernel size 2'),
    ('n.adjoint', 'n[1] = -1', 'cin breaks the chain'),
    ('w.adjoint', 'n[1] = -1', 'last layer not tanh'),
    ('n.store', 'plane_stride one cell short', 'agent_stride 0'),
    ('w.adjoint_memory', 'agent_stride 0', 'n[1] = -1'),
    ('stock_plane', 'plane_stride one cell short', 'agent_stride 0'),
    ('memory_planes', 'plane_stride one cell short', 'n[1] = -1'),
    ('gather_memory', 'agent_stride past the slot mask', 'plane_stride one cell short'),
    ('memory_cells', 'plane_stride one cell short', 'agent_stride 0'),
    ('memory_cells', 'plane_stride one cell short', 'n[3] past agent_stride'),
    ('memory_planes_adjoint', 'agent_stride 0', '65 replicas'),
    ('gather_memory_adjoint', 'agent_stride past the slot mask', 'n[1] = -1'),
]


def _faulted(spec, episodes, *faults):
    cfg = _config(spec, episodes)
    for f in faults:
        FAULTS[f][1](cfg, spec)
    return cfg


def _observe(L, name, episodes, *faults):
    """(return code, last-error text with the call's own name as `@`)"""
    rc = _invoke(L, name, _faulted(CALLS[name], episodes, *faults))
    return rc, L.lib.die_last_error().decode().replace(CALLS[name]['fn'], '@')


def _expand(ids):
    """'a b/E2': call a with both episode counts, call b with episodes = 2 only"""
    for key in ids.split():
        name, _, only = key.partition('/E')
        for e in EPISODES if not only else (int(only),):
            yield name, e


def _query_faults(name):
    spec = QUERIES[name]
    return [f for f in FAULTS if (f in SCALAR_FAULTS if spec['scalar'] else FAULTS[f][0](spec))]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('fault', list(FAULTS))
def test_single_fault_is_refused_as_recorded(lib, fault):
    """every call the fault applies to, with 4 replicas and episodes 0 and 2: the code and the whole text"""
    applies = sorted((n, e) for n, s in CALLS.items() if FAULTS[fault][0](s) for e in EPISODES)
    assert sorted(k for ids in EXPECT_SINGLE[fault].values() for k in _expand(ids)) == applies, 'the table misses a call or has one twice'
    for (rc, text), ids in EXPECT_SINGLE[fault].items():
        assert rc in (-1, -3), (fault, rc)                      # a refusal: nothing else may be recorded, or replayed
        for name, episodes in _expand(ids):
            assert _observe(lib, name, episodes, fault) == (rc, text), (fault, name, episodes)


@pytest.mark.parametrize('case', range(len(DOUBLES)), ids=['%s: %s + %s' % d for d in DOUBLES])
def test_double_fault_precedence_is_as_recorded(lib, case):
    name, first, second = DOUBLES[case]
    rc, text = EXPECT_DOUBLE[case]
    assert rc in (-1, -3)
    assert _observe(lib, name, 0, first, second) == (rc, text)
    assert _observe(lib, name, 0, second, first) == (rc, text)


@pytest.mark.parametrize('name', list(QUERIES))
def test_byte_queries_answer_and_leave_the_error_text_as_recorded(lib, name):
    spec = QUERIES[name]
    assert sorted(EXPECT_QUERY[name]) == sorted(['none'] + _query_faults(name))
    for fault, want in EXPECT_QUERY[name].items():
        for episodes in EPISODES:
            value, err = _query(lib, name, _faulted(spec, episodes, *(() if fault == 'none' else (fault,))))
            assert (value, err.decode()) == want, (name, fault, episodes)


def test_every_listed_call_and_fault_family_is_recorded():
    assert set(EXPECT_SINGLE) == set(FAULTS) and len(EXPECT_DOUBLE) == len(DOUBLES) >= 12 and set(EXPECT_QUERY) == set(QUERIES)
    assert {name for groups in EXPECT_SINGLE.values() for ids in groups.values() for name, _ in _expand(ids)} == set(CALLS)


# ------------------------------------------------------------------------------------------------ recording
def _record():
    import torch
    assert not torch.cuda.is_available(), 'recording runs the unfaulted calls up to their launch: only where there is no GPU'
    L = _lib()
    for name in CALLS:                                           # the unfaulted arguments pass every check: the launch is what fails
        for e in EPISODES:
            rc, text = _observe(L, name, e)
            assert rc == -2 and ('launch failed' in text or 'clearing' in text), (name, e, rc, text)
    out = ['EXPECT_SINGLE = {']
    for fault, (applies, _) in FAULTS.items():
        groups = {}
        for name, spec in CALLS.items():
            if applies(spec):
                seen = [_observe(L, name, e, fault) for e in EPISODES]
                for e, o in zip(EPISODES, seen):
                    groups.setdefault(o, []).append(name if seen[0] == seen[1] else '%s/E%d' % (name, e))
        out.append('    %r: {' % fault)
        for o, ids in groups.items():
            out.append('        %r:' % (o,))
            out += ['            %r' % (line + ' ') for line in textwrap.wrap(' '.join(dict.fromkeys(ids)), 120)]
            out[-1] = out[-1][:-2] + "',"
        out.append('    },')
    out += ['}', 'EXPECT_DOUBLE = [']
    out += ['    %r,' % (_observe(L, name, 0, first, second),) for name, first, second in DOUBLES]
    out += [']', 'EXPECT_QUERY = {']
    for name, spec in QUERIES.items():
        out.append('    %r: {' % name)
        for fault in ['none'] + _query_faults(name):
            seen = {(v, err.decode()) for v, err in (_query(L, name, _faulted(spec, e, *(() if fault == 'none' else (fault,)))) for e in EPISODES)}
            assert len(seen) == 1, (name, fault, seen)           # (a query does not look at the episodes beyond their own rule)
            out.append(('        %r: %r,' % (fault, seen.pop())).replace(repr(UNTOUCHED), 'UNTOUCHED'))
        out.append('    },')
    print('\n'.join(out + ['}']))


# ------------------------------------------------------------------------------------------------ the recorded values
EXPECT_SINGLE = {
    'null stack': {
        (-1, '@: null argument'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'null layers': {
        (-1, '@: null stack, layer list or scratch'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: null stack or layer list'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    '0 layers': {
        (-1, '@: 1..8 layers (got 0)'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'one layer too many': {
        (-1, '@: 1..8 layers (got 9)'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'bad padding mode': {
        (-1, '@: bad padding mode 4'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'with_agent_channel 2': {
        (-1, '@: with_agent_channel is 0 or 1'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'episodes 3': {
        (-1, '@: episodes 3: at least 1 (0 reads as 1) and a divisor of the 4 replicas'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    '0 replicas': {
        (-1, '@: 1..64 replicas'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: 1..64 replicas (got 0)'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory stock_plane memory_planes '
            'gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    '65 replicas': {
        (-1, '@: 1..64 replicas'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: 1..64 replicas (got 65)'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory stock_plane memory_planes '
            'gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    'kernel size 2': {
        (-1, '@: layer 0: kernel size 2 (odd sizes up to 7)'):
            'n.step n.step_dropout n.step_rows n.step_stock n.store n.adjoint n.adjoint_inputs',
        (-1, '@: layer 0: kernel size 2 (1, 3 or 5)'):
            'w.step w.step_stock w.step_memory w.step_memory+stock w.store w.store_memory w.adjoint w.adjoint_memory',
    },
    'kernel size 7': {
        (-1, '@: layer 0: kernel size 7 (1, 3 or 5)'):
            'w.step w.step_stock w.step_memory w.step_memory+stock w.store w.store_memory w.adjoint w.adjoint_memory',
    },
    'kernel size 9': {
        (-1, '@: layer 0: kernel size 9 (odd sizes up to 7)'):
            'n.step n.step_dropout n.step_rows n.step_stock n.store n.adjoint n.adjoint_inputs',
    },
    'cin breaks the chain': {
        (-1, '@: layer 1: 4 -> 3 channels (input has 3, at most 4 out)'):
            'n.step n.step_dropout n.step_rows n.step_stock n.store n.adjoint n.adjoint_inputs',
        (-1, '@: layer 1: 9 -> 3 channels (input has 8, at most 32 out)'):
            'w.step w.step_stock w.store w.adjoint',
        (-1, '@: layer 1: 9 -> 5 channels (input has 8, at most 32 out)'):
            'w.step_memory w.step_memory+stock w.store_memory w.adjoint_memory',
    },
    'cout past the maximum': {
        (-1, '@: layer 0: 3 -> 5 channels (input has 3, at most 4 out)'):
            'n.step n.step_dropout n.step_rows n.store n.adjoint n.adjoint_inputs',
        (-1, '@: layer 0: 4 -> 5 channels (input has 4, at most 4 out)'):
            'n.step_stock',
        (-1, '@: layer 0: 3 -> 33 channels (input has 3, at most 32 out)'):
            'w.step w.store w.adjoint',
        (-1, '@: layer 0: 4 -> 33 channels (input has 4, at most 32 out)'):
            'w.step_stock',
        (-1, '@: layer 0: 5 -> 33 channels (input has 5, at most 32 out)'):
            'w.step_memory w.store_memory w.adjoint_memory',
        (-1, '@: layer 0: 6 -> 33 channels (input has 6, at most 32 out)'):
            'w.step_memory+stock',
    },
    'bad activation': {
        (-1, "@: layer 0: activation 3 (0 none, 1 tanh, 2 relu; the last layer's is tanh)"):
            'w.step w.step_stock w.step_memory w.step_memory+stock w.store w.store_memory w.adjoint w.adjoint_memory',
    },
    'last layer not tanh': {
        (-1, "@: layer 1: activation 2 (0 none, 1 tanh, 2 relu; the last layer's is tanh)"):
            'w.step w.step_stock w.step_memory w.step_memory+stock w.store w.store_memory w.adjoint w.adjoint_memory',
    },
    'null weights': {
        (-1, "@: layer 0: null weights or stride below a replica's block"):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'weight_stride one short': {
        (-1, "@: layer 0: null weights or stride below a replica's block"):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'reflect on one cell': {
        (-1, "@: layer 0: 'reflect' padding of 1 cells needs a field larger than that (1x72)"):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'last layer one plane short': {
        (-1, '@: the last layer gives 2 planes (dx, dy, deposit: 3)'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock n.store w.store n.adjoint n.adjoint_inputs w.adjoint',
        (-1, '@: the last layer gives 4 planes (dx, dy, deposit and 2 memory planes: 5)'):
            'w.step_memory w.step_memory+stock w.store_memory w.adjoint_memory',
    },
    'scratch one byte short': {
        (-1, '@: scratch too small (221183 < 221184)'):
            'n.step n.step_dropout n.step_rows n.step_stock',
        (-1, '@: scratch too small (442367 < 442368)'):
            'w.step w.step_stock w.step_memory w.step_memory+stock',
    },
    'plane_stride one cell short': {
        (-1, '@: strides smaller than a replica'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: plane_stride 1727 smaller than a plane'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
        (-1, '@: plane_stride 1727 smaller than a plane (1728 cells)'):
            'stock_plane memory_planes gather_memory memory_cells',
    },
    'agent_stride 0': {
        (-1, '@: strides smaller than a replica'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: agent_stride 0'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
        (-1, '@: agent_stride 0 outside 1..134217726'):
            'stock_plane memory_planes gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    'agent_stride past the slot mask': {
        (-1, '@: agent_stride 134217727 outside 1..134217726'):
            'stock_plane memory_planes gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    'n[1] = -1': {
        (-1, '@: replica 1 has -1 agents'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
        (-1, '@: replica 1 has -1 agents (0..10)'):
            'stock_plane memory_planes gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    'n[3] past agent_stride': {
        (-1, '@: replica 3 has 11 agents'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
        (-1, '@: replica 3 has 11 agents (0..10)'):
            'stock_plane memory_planes gather_memory memory_cells memory_planes_adjoint gather_memory_adjoint',
    },
    'bad dtype': {
        (-1, '@: bad field dtype 7'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock n.store w.store '
            'w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'null food plane': {
        (-1, '@: null plane, or chem_next not a second plane'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: null plane'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'sense_epoch 0': {
        (-1, '@: claims at epoch 2 cannot follow sensing at epoch 0'):
            'n.step n.step_dropout n.step_rows n.step_stock w.step w.step_stock w.step_memory w.step_memory+stock',
        (-1, '@: sense_epoch 0'):
            'n.store w.store w.store_memory n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'reflect on the adjoint': {
        (-3, "@: the adjoint of 'reflect' / 'replicate' padding is not implemented ('circular' and 'zeros' are)"):
            'n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
    'replicate on the adjoint': {
        (-3, "@: the adjoint of 'reflect' / 'replicate' padding is not implemented ('circular' and 'zeros' are)"):
            'n.adjoint n.adjoint_inputs w.adjoint w.adjoint_memory',
    },
}
EXPECT_DOUBLE = [
    (-1, '@: scratch too small (221183 < 221184)'),
    (-1, '@: layer 0: kernel size 7 (1, 3 or 5)'),
    (-1, '@: the last layer gives 4 planes (dx, dy, deposit and 2 memory planes: 5)'),
    (-1, '@: plane_stride 1727 smaller than a plane'),
    (-1, '@: plane_stride 1727 smaller than a plane'),
    (-1, '@: replica 1 has -1 agents'),
    (-1, '@: replica 1 has -1 agents'),
    (-1, '@: plane_stride 1727 smaller than a plane'),
    (-1, '@: agent_stride 0'),
    (-1, '@: plane_stride 1727 smaller than a plane (1728 cells)'),
    (-1, '@: plane_stride 1727 smaller than a plane (1728 cells)'),
    (-1, '@: plane_stride 1727 smaller than a plane (1728 cells)'),
    (-1, '@: agent_stride 0 outside 1..134217726'),
    (-1, '@: replica 3 has 11 agents (0..10)'),
    (-1, '@: 1..64 replicas (got 65)'),
    (-1, '@: agent_stride 134217727 outside 1..134217726'),
]
EXPECT_QUERY = {
    'die_nca_batch_scratch_bytes': {
        'none': (221184, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'cout past the maximum': (221184, UNTOUCHED),
    },
    'die_nca_sense_batch_store_bytes': {
        'none': (221184, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'cout past the maximum': (221184, UNTOUCHED),
    },
    'die_nca_backward_batch_workspace_bytes': {
        'none': (160768, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'cout past the maximum': (160768, UNTOUCHED),
    },
    'die_nca_wide_batch_scratch_bytes': {
        'none': (442368, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'cout past the maximum': (-1, UNTOUCHED),
    },
    'die_nca_wide_sense_batch_store_bytes': {
        'none': (442368, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'cout past the maximum': (-1, UNTOUCHED),
    },
    'die_nca_wide_backward_batch_workspace_bytes': {
        'none': (235008, UNTOUCHED),
        'null stack': (-1, UNTOUCHED),
        'null layers': (-1, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        'bad padding mode': (-1, UNTOUCHED),
        'with_agent_channel 2': (-1, UNTOUCHED),
        'episodes 3': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'kernel size 2': (-1, UNTOUCHED),
        'kernel size 7': (-1, UNTOUCHED),
        'cin breaks the chain': (-1, UNTOUCHED),
        'cout past the maximum': (-1, UNTOUCHED),
        'bad activation': (-1, UNTOUCHED),
        'last layer not tanh': (-1, UNTOUCHED),
        'null weights': (235008, UNTOUCHED),
        'weight_stride one short': (235008, UNTOUCHED),
        'reflect on one cell': (-1, UNTOUCHED),
        'last layer one plane short': (-1, UNTOUCHED),
        'reflect on the adjoint': (-1, UNTOUCHED),
        'replicate on the adjoint': (-1, UNTOUCHED),
    },
    'die_nca_wide_backward_batch_memory_workspace_bytes': {
        'none': (244224, UNTOUCHED),
        'null stack': (-1, UNTOUCHED),
        'null layers': (-1, UNTOUCHED),
        '0 layers': (-1, UNTOUCHED),
        'one layer too many': (-1, UNTOUCHED),
        'bad padding mode': (-1, UNTOUCHED),
        'with_agent_channel 2': (-1, UNTOUCHED),
        'episodes 3': (-1, UNTOUCHED),
        '0 replicas': (-1, UNTOUCHED),
        '65 replicas': (-1, UNTOUCHED),
        'kernel size 2': (-1, UNTOUCHED),
        'kernel size 7': (-1, UNTOUCHED),
        'cin breaks the chain': (-1, UNTOUCHED),
        'cout past the maximum': (-1, UNTOUCHED),
        'bad activation': (-1, UNTOUCHED),
        'last layer not tanh': (-1, UNTOUCHED),
        'null weights': (244224, UNTOUCHED),
        'weight_stride one short': (244224, UNTOUCHED),
        'reflect on one cell': (-1, UNTOUCHED),
        'last layer one plane short': (-1, UNTOUCHED),
        'reflect on the adjoint': (-1, UNTOUCHED),
        'replicate on the adjoint': (-1, UNTOUCHED),
    },
}

if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    _record()
