"""Reference outputs and gradients of the HRNet backbone (needs the reference tree; the .npz travels):
  python tools/gen_hrnet.py
  tests/golden/hrnet.npz   the reference's own class (mmdet.models.backbones.hrnet.HRNet, imported after oracle.ref_loader.load())
                           run in fp64 on tests/hrnet_ref.CASES, in the archive format of tools/gen_fpn_extra_levels.py.
Per case ``name``:
  name:out<l>            branch output l in full where it has <= FULL elements, else name:out<l>:sample (grad_sample_index(numel,
                         OUT_K)) and name:out<l>:norm; always name:out<l>:absmax and name:out<l>:shape
  name:norm:<tensor> / name:sample:<tensor>   gradient of the linear functional sum_l <w_l, out_l> (hrnet_ref.functional_weight) wrt
                         every parameter and wrt ``conv2_in``, the image-side input of conv2 (ReLU(bn1(conv1(img)))): L2 norm and the
                         values at grad_sample_index(numel, GRAD_K)
  name:fp32:worst        conditioning: the reference alone in fp32 against its fp64 run, the worst output (max|diff| / max|level|) and the
                         worst gradient (rel-L2) -- one pair per case, not one entry per tensor: about a thousand tensors would put the
                         archive past 1 MiB.  A case is admitted only when both stay within ADMIT_OUT / ADMIT_GRAD, a quarter of the bars
                         the GPU tests hold the port to; otherwise change its seed -- never the bars.
  keys:<name>            (JSON) the reference class's state-dict keys and shapes, in its order
``cases`` (JSON): the configurations.  ``raises:widen_branch0``: the error the reference's forward raises on hrnet_ref.WIDEN_BRANCH0
(a stage that widens a branch other than the last), which therefore has no case.  Weights: synthetic.hrnet_state_dict(extra, seed), loaded strictly; inputs
and functional weights: seeded normals rounded to fp32 once.  Fixed member timestamps: a rerun reproduces the file byte for byte."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.gen_golden import grad_sample_index  # noqa: E402
from tests import hrnet_ref as HR  # noqa: E402
from tools.gen_fpn_extra_levels import ADMIT_GRAD, ADMIT_OUT, rel_l2, save_npz  # noqa: E402


def load_class():
    from oracle import ref_loader
    assert ref_loader.available(), 'needs the reference tree (oracle/ref_loader.py)'
    ref_loader.load()
    return importlib.import_module('mmdet.models.backbones.hrnet').HRNet


def run_reference(HRNet, cfg, dtype):
    m = HRNet(cfg['extra']).to(dtype)
    m.load_state_dict(HR.case_state_dict(cfg, dtype), strict=True)
    m.train()       # norm_eval=True: every BatchNorm in eval mode
    assert not any(b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    seen = {}
    m.conv2.register_forward_pre_hook(lambda mod, inp: (inp[0].retain_grad(), seen.setdefault('conv2_in', inp[0]))[0])
    outs = m(HR.case_input(cfg, dtype))
    total = sum((HR.functional_weight(cfg, l, o.shape, dtype) * o).sum() for l, o in enumerate(outs))
    total.backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    assert all(g is not None for g in grads.values())
    grads['conv2_in'] = seen['conv2_in'].grad
    return m, [o.detach() for o in outs], grads


def reference_case(HRNet, name, cfg):
    m, outs, grads = run_reference(HRNet, cfg, torch.float64)
    _, outs32, grads32 = run_reference(HRNet, cfg, torch.float32)
    out = {'keys:' + name: np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))}
    worst_out = worst_grad = 0.0
    for l, (o, o32) in enumerate(zip(outs, outs32)):
        key = '%s:out%d' % (name, l)
        if o.numel() <= HR.FULL:
            out[key] = o.numpy()
        else:
            flat = o.flatten()
            out[key + ':sample'] = flat[torch.from_numpy(grad_sample_index(flat.numel(), HR.OUT_K))].numpy()
            out[key + ':norm'] = np.float64(float(flat.norm()))
        out[key + ':absmax'] = np.float64(float(o.abs().max()))
        out[key + ':shape'] = np.array(o.shape, dtype=np.int64)
        err = float((o32.double() - o).abs().max() / o.abs().max())
        worst_out = max(worst_out, err)
    for key, gr in grads.items():
        flat = gr.detach().flatten()
        out['%s:norm:%s' % (name, key)] = np.float64(float(flat.norm()))
        out['%s:sample:%s' % (name, key)] = flat[torch.from_numpy(grad_sample_index(flat.numel(), HR.GRAD_K))].numpy()
        err = rel_l2(grads32[key].flatten(), flat)
        worst_grad = max(worst_grad, err)
    print('%-18s outputs %s  fp32-vs-fp64: outputs %.2e (admit %.1e)  gradients %.2e (admit %.1e)  min grad norm %.3g' % (
        name, [tuple(o.shape[2:]) for o in outs], worst_out, ADMIT_OUT, worst_grad, ADMIT_GRAD,
        min(float(v) for k, v in out.items() if k.startswith(name + ':norm:'))), flush=True)
    out['%s:fp32:worst' % name] = np.array([worst_out, worst_grad])
    assert worst_out <= ADMIT_OUT and worst_grad <= ADMIT_GRAD, 'case %s is ill-conditioned in fp32: change its seed' % name
    return out


def main():
    torch.set_num_threads(min(8, int(os.environ.get('OMP_NUM_THREADS', '8'))))
    HRNet = load_class()
    out = {'cases': np.array(json.dumps(HR.CASES, sort_keys=True))}
    for name, cfg in HR.CASES.items():
        out.update(reference_case(HRNet, name, cfg))
    try:
        run_reference(HRNet, HR.WIDEN_BRANCH0, torch.float32)
        raise AssertionError('the reference ran hrnet_ref.WIDEN_BRANCH0: give it a case')
    except RuntimeError as e:
        out['raises:widen_branch0'] = np.array(str(e))
        print('widen_branch0: the reference raises:', e)
    save_npz(HR.GOLDEN, out)
    print(HR.GOLDEN, len(out), 'arrays', os.path.getsize(HR.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
