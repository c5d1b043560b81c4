"""What ``ops.ChebConv``, ``ops.conv_windows`` and the models' conv trunk launch, case by case (tools/conv_trace.py: single
layers on every arm, ``cgcnn`` / ``finetuning_cgcnn`` steps, forwards, window decodes and Grad-CAM passes), against the
sequences recorded in tests/golden/conv_dispatch.json: the library entry points in call order, the layer's own ``(what, kernel
templates)`` pairs of ``_lib.dispatch_log`` (``conv_trace.LAYER_WHATS``: a case does not depend on what ran before it) and the
number of ``ops._side_stream`` calls.  A change that moves, adds or drops a launch of
the layer shows here by name.  The recorded templates assume the 256 CUs of an MI355X; ``python tools/conv_trace.py --golden``
rewrites the file.  Needs an MI355X: ``-m gpu``."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('conv_trace', os.path.join(ROOT, 'tools', 'conv_trace.py'))
conv_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(conv_trace)
with open(os.path.join(ROOT, 'tests', 'golden', 'conv_dispatch.json')) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope='module')
def world():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, 'the recorded dispatch assumes 256 CUs'
    w = conv_trace.World()
    yield w
    w.close()


def test_cases_and_golden_file_agree():
    assert sorted(GOLDEN) == sorted(name for name, _, _, _ in conv_trace.CASES)


def test_recorded_cases_reach_every_entry_point():
    """The condition the trace stands on: no launching entry point of the layer is absent from the recorded sequences."""
    assert conv_trace.missing_entry_points(GOLDEN) == []


@pytest.mark.parametrize('name', [name for name, _, _, _ in conv_trace.CASES])
def test_case_launches_what_was_recorded(world, name):
    rec, want = conv_trace.run_case(world, name, hashes=False), GOLDEN[name]
    assert rec['calls'] == want['calls']
    assert rec['dispatch'] == want['dispatch']
    assert rec['side_streams'] == want['side_streams']
