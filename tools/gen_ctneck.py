"""Reference outputs and gradients of CTResNetNeck (needs the reference tree; the .npz travels):
  python tools/gen_ctneck.py
  tests/golden/ctneck.npz   the reference's own CTResNetNeck class (T/mmdet/models/necks/ct_resnet_neck.py) run in fp64 on the cases of
                            tests/ctneck_ref.py, in train mode (BatchNorm batch statistics) unless the case says otherwise.
The archive has the format of tools/gen_fpn_extra_levels.py (see there: ``name:out0`` in full or sampled, ``name:norm:<tensor>`` /
``name:sample:<tensor>`` of the gradient of the fixed linear functional wrt every parameter and the input ``in0``, ``name:fp32:<tensor>``
conditioning entries and the admission rule, ``cases``, ``keys:<name>``, byte-reproducible members), plus ``name:stat:<buffer>``: every
BatchNorm buffer (running_mean, running_var, num_batches_tracked) after the one forward.
oracle/ref_loader.py's mmcv stand-in builds an nn.Conv2d whatever ``conv_cfg`` says, so a ConvModule subclass is installed after
ref_loader.load() that maps ``conv_cfg=dict(type='deconv')`` to nn.ConvTranspose2d -- what mmcv's CONV_LAYERS registers under 'deconv'
(same attribute names, same state-dict keys)."""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
for p in (ROOT, TOOLS, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_fpn_extra_levels as G  # noqa: E402
import ctneck_ref as C  # noqa: E402
from oracle.gen_golden import GOLDEN, grad_sample_index  # noqa: E402

OUT = os.path.join(GOLDEN, 'ctneck.npz')


def run_reference(CTResNetNeck, cfg, dtype):
    neck = CTResNetNeck(**C.constructor_kwargs(cfg)).to(dtype)
    neck.load_state_dict(C.case_state_dict(cfg, dtype), strict=True)
    neck.train(cfg['train'])
    x = C.case_input(cfg, dtype).requires_grad_(True)
    outs = neck([x])
    assert isinstance(outs, tuple) and len(outs) == 1
    (C.functional_weight(cfg, outs[0].shape, dtype) * outs[0]).sum().backward()
    grads = {n: p.grad for n, p in neck.named_parameters()}
    grads[C.INPUT] = x.grad
    return neck, outs[0].detach(), grads


def reference_case(CTResNetNeck, name, cfg):
    neck, o, grads = run_reference(CTResNetNeck, cfg, torch.float64)
    _, o32, grads32 = run_reference(CTResNetNeck, cfg, torch.float32)
    out = {'keys:' + name: np.array(json.dumps([[k, list(v.shape)] for k, v in neck.state_dict().items()]))}
    key = name + ':out0'
    if o.numel() <= C.FULL:
        out[key] = o.numpy()
    else:
        flat = o.flatten()
        out[key + ':sample'] = flat[torch.from_numpy(grad_sample_index(flat.numel(), C.OUT_K))].numpy()
        out[key + ':norm'] = np.float64(float(flat.norm()))
    out[key + ':absmax'] = np.float64(float(o.abs().max()))
    out[key + ':shape'] = np.array(o.shape, dtype=np.int64)
    worst_out = float((o32.double() - o).abs().max() / o.abs().max())
    out[name + ':fp32:out0'] = np.float64(worst_out)
    worst_grad = 0.0
    for k, gr in grads.items():
        flat = gr.detach().flatten()
        out['%s:norm:%s' % (name, k)] = np.float64(float(flat.norm()))
        out['%s:sample:%s' % (name, k)] = flat[torch.from_numpy(grad_sample_index(flat.numel(), C.GRAD_K))].numpy()
        err = G.rel_l2(grads32[k].flatten(), flat)
        out['%s:fp32:%s' % (name, k)] = np.float64(err)
        worst_grad = max(worst_grad, err)
    for k, v in neck.state_dict().items():
        if k.split('.')[-1] in ('running_mean', 'running_var', 'num_batches_tracked'):
            out['%s:stat:%s' % (name, k)] = v.detach().numpy()
    print('%-16s output %s  fp32-vs-fp64: output %.2e (admit %.1e)  gradients %.2e (admit %.1e)' % (
        name, tuple(o.shape), worst_out, G.ADMIT_OUT, worst_grad, G.ADMIT_GRAD), flush=True)
    assert worst_out <= G.ADMIT_OUT and worst_grad <= G.ADMIT_GRAD, 'case %s is ill-conditioned in fp32: change its seed or sizes' % name
    return out


def main():
    from oracle import ref_loader
    assert ref_loader.available(), 'needs the reference tree (oracle/ref_loader.py)'
    torch.set_num_threads(4)
    ref_loader.load()
    base = sys.modules['mmcv.cnn'].ConvModule

    class ConvModule(base):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, **kw):
            super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, **kw)
            if conv_cfg is not None:
                assert conv_cfg == dict(type='deconv'), conv_cfg
                self.conv = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride, padding, bias=self.conv.bias is not None)
    sys.modules['mmcv.cnn'].ConvModule = ConvModule
    mod = importlib.import_module('mmdet.models.necks.ct_resnet_neck')
    mod.ConvModule = ConvModule
    out = {'cases': np.array(json.dumps(C.CASES, sort_keys=True))}
    for name, cfg in C.CASES.items():
        out.update(reference_case(mod.CTResNetNeck, name, cfg))
    G.save_npz(OUT, out)
    print(OUT, len(out), 'arrays', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
