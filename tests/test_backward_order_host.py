"""Host: CprTrainer._backward_order() on every configuration of tests/backward_order_cases.py equals tests/golden/backward_order.json name
for name (tools/gen_backward_order.py wrote it on the commit before the units functions of training.py replaced the hand-written lists), and
is the set of trainable parameters, each exactly once.  No device needed."""
import json
import os

import pytest

from tests import backward_order_cases as C


@pytest.fixture(scope='module')
def pinned(golden_dir):
    with open(os.path.join(golden_dir, 'backward_order.json')) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(pinned):
    assert sorted(pinned) == sorted(C.CASES)


@pytest.mark.parametrize('name', list(C.CASES))
def test_flat_order_is_the_pinned_one_and_names_every_trainable_parameter_once(pinned, name):
    order, trainable = C.order_names(name)
    assert len(set(order)) == len(order) and sorted(order) == sorted(trainable)
    assert order == pinned[name]
