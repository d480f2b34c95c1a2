"""tests/golden/build_host_math.npz: torch.log / torch.cdist as the build host computes them on every input the assigner cost
checks of tests/test_oracle_golden.py feed them (oracle/host_math.py).  Run on the host that produced tests/golden/assigners.npz
and p2p_options.npz (the fixtures' cost bits must come out of the oracle here, which this script checks):
  python -m oracle.gen_golden_host_math"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import cpr_oracle as O  # noqa: E402
from oracle import gen_golden_r6 as R6  # noqa: E402
from oracle import host_math  # noqa: E402
from oracle import p2p_options_oracle as PO  # noqa: E402
from oracle.gen_golden import GOLDEN, assigner_inputs  # noqa: E402


def hungarian_v2_cases(g):
    """(case, oracle outputs) of test_hungarian_v2_matches_reference_fixture."""
    for case in range(5):
        n_side, G, C, k = [int(v) for v in g['ha%d_cfg' % case]]
        pred, logits, gt, labels, shp = assigner_inputs(200 + case, n_side, 4, G, C)
        yield case, O.hungarian_assign_v2(pred, logits, gt, labels, shp, topk_k=k)


def general_cost_cases():
    """(case, oracle outputs) of test_general_match_cost_oracle_matches_reference."""
    for ci, (seed, n_side, G, C, cc, rc, k) in enumerate(R6.COST_CASES):
        pred, logits, gt, labels, shape = assigner_inputs(seed, n_side, 4, G, C)
        cc = cc if isinstance(cc, list) else [cc]
        rc = rc if isinstance(rc, list) else [rc]
        yield ci, PO.hungarian_assign_v2(cc, rc, k, pred, logits, gt, labels, shape)


def run():
    ga = np.load(os.path.join(GOLDEN, 'assigners.npz'))
    gp = np.load(os.path.join(GOLDEN, 'p2p_options.npz'))
    with host_math.record() as rec:
        for case, (inds, _, _) in hungarian_v2_cases(ga):
            assert np.array_equal(inds.numpy(), ga['ha%d_gt_inds' % case]), 'not the fixtures\' host (ha%d)' % case
        for ci, (_, _, cost) in general_cost_cases():
            assert np.array_equal(cost.numpy().astype(np.float32), gp['cost%d:cost' % ci]), 'not the fixtures\' host (cost%d)' % ci
    path = os.path.join(GOLDEN, 'build_host_math.npz')
    host_math.save(path, rec)
    return path


if __name__ == '__main__':
    print(run())
