"""The BUILD host's math library as data (test infrastructure).

Two torch CPU primitives the reference's match costs call give host-dependent bits: ``torch.log`` (MKL VML: the Xeon and EPYC
kernels differ in the last bit, see cpr_oracle._log_cr) and ``torch.cdist(p=2)`` on more than 25 rows (an MKL sgemm whose
blocking differs between CPUs).  The assigner fixtures (tests/golden/assigners.npz, p2p_options.npz) hold the reference's cost
bits as the build host computed them, so a bit-exact comparison of the oracle's costs against them only holds on such a host.

``record()`` runs a callable with both primitives wrapped and returns what they computed; ``replay(table)`` swaps them for
lookups into such a recording, so the oracle evaluates its costs with the build host's primitives on any machine:
  python -m oracle.gen_golden_host_math     (on the build host)  ->  tests/golden/build_host_math.npz
An input the recording does not hold is an error: the recording must be regenerated with the fixtures it belongs to."""
import contextlib
import hashlib

import numpy as np
import torch


def _key(*tensors, p=2.0):
    h = hashlib.sha1(repr(float(p)).encode())
    for t in tensors:
        t = t.detach().contiguous()
        h.update(repr((str(t.dtype), tuple(t.shape))).encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()[:24]


@contextlib.contextmanager
def record():
    """Within the block torch.log / torch.cdist are the host's own, and every fp32 result is kept -> dict for ``save``."""
    real_log, real_cdist = torch.log, torch.cdist
    logs, cdists = {}, {}

    def log(x, *a, **k):
        y = real_log(x, *a, **k)
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and not a and not k:
            xb, yb = x.detach().contiguous().numpy().view(np.int32).ravel(), y.detach().contiguous().numpy().view(np.int32).ravel()
            logs.update(zip(xb.tolist(), yb.tolist()))
        return y

    def cdist(x1, x2, p=2.0, **k):
        y = real_cdist(x1, x2, p=p, **k)
        if x1.dtype == torch.float32 and float(p) == 2.0 and not k:
            cdists[_key(x1, x2, p=p)] = y.detach().numpy().copy()
        return y

    torch.log, torch.cdist = log, cdist
    out = dict(logs=logs, cdists=cdists)
    try:
        yield out
    finally:
        torch.log, torch.cdist = real_log, real_cdist


def save(path, rec):
    x = np.array(sorted(rec['logs']), dtype=np.int32)
    y = np.array([rec['logs'][int(v)] for v in x], dtype=np.int32)
    np.savez_compressed(path, log_x=x, log_y=y, **{'cdist:' + k: v for k, v in rec['cdists'].items()})


@contextlib.contextmanager
def replay(path):
    """Within the block torch.log and torch.cdist(p=2) return the recorded build-host values (fp32 inputs), the real ones otherwise
    (cdist with another p sums exact per-element terms in a fixed order: the same bits everywhere)."""
    t = np.load(path)
    lx, ly = t['log_x'], t['log_y']
    cd = {k[len('cdist:'):]: t[k] for k in t.files if k.startswith('cdist:')}
    real_log, real_cdist = torch.log, torch.cdist

    def log(x, *a, **k):
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and not a and not k):
            return real_log(x, *a, **k)
        xb = x.detach().contiguous().numpy().view(np.int32).ravel()
        i = np.minimum(np.searchsorted(lx, xb), len(lx) - 1)
        missing = int((lx[i] != xb).sum())
        assert missing == 0, '%d log inputs are not in the build-host recording %s' % (missing, path)
        return torch.from_numpy(ly[i].view(np.float32).reshape(x.shape))

    def cdist(x1, x2, p=2.0, **k):
        if x1.dtype != torch.float32 or float(p) != 2.0 or k:
            return real_cdist(x1, x2, p=p, **k)
        key = _key(x1, x2, p=p)
        assert key in cd, 'cdist input not in the build-host recording %s' % path
        return torch.from_numpy(cd[key].copy())

    torch.log, torch.cdist = log, cdist
    try:
        yield
    finally:
        torch.log, torch.cdist = real_log, real_cdist
