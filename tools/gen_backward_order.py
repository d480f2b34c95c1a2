"""The flat parameter order of every configuration in tests/backward_order_cases.py (no device needed):
  python tools/gen_backward_order.py
  tests/golden/backward_order.json   {case: [parameter name, ..]} -- CprTrainer._backward_order() name for name.
The flat order decides the gradient buckets and every ready point, so a change to the units functions of training.py must leave this file
as it is: generate it on the commit BEFORE such a change; tests/test_backward_order_host.py compares the lists on the commit after."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import backward_order_cases as C  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'backward_order.json')


def main():
    out = {}
    for name in C.CASES:
        order, trainable = C.order_names(name)
        assert sorted(order) == sorted(trainable), 'case %s: the order is not the trainable parameters, each once' % name
        out[name] = order
        print('%-34s %4d parameters' % (name, len(order)), flush=True)
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(OUT, len(out), 'cases', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
