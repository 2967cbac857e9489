"""The world-building entry points (initialisation, headings, food flows, the read-out; stand-alone and batched) write the bits
recorded in tests/golden/init_flow_pins.json, for every case of tests/golden/make_init_flow_pins.py.

The stand-alone and the batched kernels call one device body per computation, so a test that compares the two families cannot
see a change of that body, and the oracle tests allow a tolerance.  These digests were recorded at the commit the JSON names,
before the bodies were shared; any change of a value fails here without a tolerance."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_init_flow_pins', os.path.join(GOLDEN, 'make_init_flow_pins.py'))
pins_script = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins_script)

with open(os.path.join(GOLDEN, 'init_flow_pins.json')) as _f:
    RECORDED = json.load(_f)


def test_the_recorded_cases_are_the_case_list():
    assert sorted(RECORDED['pins']) == sorted(pins_script.CASES)
    assert len(RECORDED['commit']) == 40


@pytest.mark.parametrize('name', list(pins_script.CASES))
def test_bits_are_the_recorded_ones(name):
    assert pins_script.digest(pins_script.CASES[name]()) == RECORDED['pins'][name]
