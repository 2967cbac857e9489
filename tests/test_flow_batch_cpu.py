"""die_food_flow_batch and the batched food-flow classification, CPU side: the library exports the entry point, bad arguments
are refused on the host before any launch, and only the device operators of WaveSequence / PerlinNoiseSequence are taken for
the batch.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_entry_point_exported(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert hasattr(so, 'die_food_flow_batch')
    assert 'die_food_flow_batch' in lib.EXPORTS
    assert (lib.DIE_FLOW_WAVE, lib.DIE_FLOW_PERLIN) == (1, 2)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _call(lib, *, W=64, H=48, dtype=None, replicas=4, plane_stride=None, kind=None, octaves=8, null=None, gW=0):
    L = lib
    m = L.Medium(W, H, L.DIE_F32 if dtype is None else dtype, 1, FAKE, FAKE, FAKE, FAKE + 8, gW, H if gW else 0, 0, 0, 0, 0, 0, 0, None)
    if null == 'food':
        m.food = None
    b = L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    return L.lib.die_food_flow_batch(None if null == 'm' else C.byref(m), None if null == 'b' else C.byref(b),
                                     L.DIE_FLOW_PERLIN if kind is None else kind, 0.25, 0.5, 0.5, octaves, 11, None)


@pytest.mark.parametrize('case, kw, needle', [
    ('null medium', dict(null='m'), b'null argument'),
    ('null batch', dict(null='b'), b'null argument'),
    ('null food plane', dict(null='food'), b'null argument'),
    ('no replica', dict(replicas=0), b'replicas'),
    ('65 replicas', dict(replicas=65), b'replicas'),
    ('planes overlap', dict(plane_stride=64 * 48 - 1), b'plane_stride'),
    ('kind 0', dict(kind=0), b'unknown flow kind 0'),
    ('kind 3', dict(kind=3), b'unknown flow kind 3'),
    ('perlin without octaves', dict(octaves=0), b'octaves 0'),
    ('one row', dict(W=1, H=48), b'at least 2x2'),
    ('one column', dict(W=64, H=1), b'at least 2x2'),
    ('H % 4', dict(W=64, H=46), b'H % 4'),
    ('bad dtype', dict(dtype=7), b'dtype 7'),
    ('a tile of a larger world', dict(gW=128), b'whole world'),
])
def test_bad_arguments_refused_before_launch(lib, case, kw, needle):
    assert _call(lib, **kw) == -1, case
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_flow_classification(lib):
    import die_amd as die
    from die_amd.data_init import DeviceFoodFlow, FieldSequence, device_flow_kind

    size = (16, 12)
    assert device_flow_kind(die.WaveSequence(size, dt=0.01).get_flow_operator(scale=0.5, decay=0.5)) == lib.DIE_FLOW_WAVE
    assert device_flow_kind(die.PerlinNoiseSequence(size, dt=0.05).get_flow_operator(0.5, 0.5)) == lib.DIE_FLOW_PERLIN

    class Ramp(FieldSequence):                  # host field only: its operator is a Python closure
        def __getitem__(self, t):
            return np.full(self._size, t)

    class OwnWave(die.WaveSequence):            # a field of its own on the device
        def _flow(self, medium, t, scale, decay):
            pass

    class Tuned(die.WaveSequence):              # same field, other time points: batched
        def __init__(self, field_size):
            super().__init__(field_size, dt=0.5, t_bounds=(0, 2))

    assert device_flow_kind(lambda food: food * 0.5) is None
    assert device_flow_kind(Ramp(size).get_flow_operator(1.0, 1.0)) is None
    own = OwnWave(size).get_flow_operator(1.0, 1.0)
    assert isinstance(own, DeviceFoodFlow) and device_flow_kind(own) is None
    assert device_flow_kind(Tuned(size).get_flow_operator(1.0, 1.0)) == lib.DIE_FLOW_WAVE
    from die_amd.env import _identity_food_flow
    assert device_flow_kind(_identity_food_flow) is None
