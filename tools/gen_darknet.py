"""Reference outputs and gradients of the Darknet backbone (needs the reference tree; the .npz travels):
  python tools/gen_darknet.py
  tests/golden/darknet.npz   the reference's own class (mmdet.models.backbones.darknet.Darknet, imported after
                             oracle.ref_loader.load()) run in fp64 on tests/darknet_ref.CASES, in the archive format of
                             tools/gen_hrnet.py / tools/gen_fpn_extra_levels.py.
The loader's ``mmcv.cnn.ConvModule`` stand-in builds nn.ReLU for every act_cfg, so after ``ref_loader.load()`` this tool installs a
ConvModule subclass that honours act_cfg type='LeakyReLU' (its negative_slope) into sys.modules['mmcv.cnn'] and only then imports the
backbone's module, as tools/gen_mobilenet_v2.py does for ReLU6.  The oracle package itself stays as it is.
Per case ``name``:
  name:out<l>            output l in full where it has <= FULL elements, else name:out<l>:sample (grad_sample_index(numel, OUT_K)) and
                         name:out<l>:norm; always name:out<l>:absmax and name:out<l>:shape
  name:norm:<tensor> / name:sample:<tensor>   gradient of the linear functional sum_l <w_l, out_l> (darknet_ref.functional_weight) wrt
                         every parameter that trains and wrt ``stage1_in``, the image-side input of the first stride-2 conv
                         (LeakyReLU(bn(conv1(img)))), where something in front of it trains: L2 norm and the values at
                         grad_sample_index(numel, GRAD_K)
  name:fp32:worst        conditioning: the reference alone in fp32 against its fp64 run, the worst output (max|diff| / max|level|) and
                         the worst gradient (rel-L2).  A case is admitted only when both stay within ADMIT_OUT / ADMIT_GRAD, a quarter
                         of the bars the GPU tests hold the port to; otherwise change its seed -- never the bars.  A leaky net flips an
                         activation's slope where fp32 and fp64 disagree on a sign, which costs 4e-3 .. 7e-3 on a gradient: such a seed
                         is discarded.  The four seeds in darknet_ref.CASES were admitted as first chosen.
  keys:<name>            (JSON) the reference class's state-dict keys and shapes, in its order
``cases`` (JSON): the configurations.  ``flags:<k>`` (JSON): [[parameter key, requires_grad]] and [[BatchNorm module name, training]]
of the small architecture after ``train()`` with frozen_stages = k, for k in darknet_ref.FLAG_STAGES.  ``raises:depth``: the text of the
KeyError the reference raises for an unknown depth.  Weights: synthetic.darknet_state_dict(depth, seed), loaded strictly, so the
depth-53 case stores no weights; inputs and functional weights: seeded normals rounded to fp32 once.  Fixed member timestamps: a rerun
reproduces the file byte for byte."""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.gen_golden import grad_sample_index  # noqa: E402
from tests import darknet_ref as DR  # noqa: E402
from tools.gen_fpn_extra_levels import ADMIT_GRAD, ADMIT_OUT, rel_l2, save_npz  # noqa: E402


def load_class():
    from oracle import ref_loader
    assert ref_loader.available(), 'needs the reference tree (oracle/ref_loader.py)'
    ref_loader.load()
    cnn = sys.modules['mmcv.cnn']
    base = cnn.ConvModule

    class ConvModule(base):
        """The stand-in with the activation its act_cfg names: nn.LeakyReLU(negative_slope) for type='LeakyReLU'."""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            act = kw.get('act_cfg', dict(type='ReLU'))
            if act is not None:
                assert act.get('type') in ('ReLU', 'LeakyReLU'), act
                if act['type'] == 'LeakyReLU':
                    self.activate = nn.LeakyReLU(negative_slope=act.get('negative_slope', 0.01), inplace=kw.get('inplace', True))
    cnn.ConvModule = ConvModule
    return DR.add_small_arch(importlib.import_module('mmdet.models.backbones.darknet').Darknet)


def run_reference(Darknet, cfg, dtype):
    m = Darknet(**DR.constructor_kwargs(cfg)).to(dtype)
    assert all(isinstance(c.activate, nn.LeakyReLU) and c.activate.negative_slope == cfg['negative_slope']
               for c in m.modules() if hasattr(c, 'activate'))
    m.load_state_dict(DR.case_state_dict(cfg, dtype), strict=True)
    m.train()       # norm_eval=True: every BatchNorm in eval mode; frozen_stages applied
    assert not any(b.training for b in m.modules() if isinstance(b, nn.BatchNorm2d))
    seen = {}

    def tap(mod, inp):
        if inp[0].requires_grad:
            inp[0].retain_grad()
        seen[DR.STEM_IN] = inp[0]
    m.conv_res_block1.conv.register_forward_pre_hook(tap)
    outs = m(DR.case_input(cfg, dtype))
    total = sum((DR.functional_weight(cfg, l, o.shape, dtype) * o).sum() for l, o in enumerate(outs))
    total.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    assert all(g is not None for g in grads.values())
    if seen[DR.STEM_IN].requires_grad:
        grads[DR.STEM_IN] = seen[DR.STEM_IN].grad
    return m, [o.detach() for o in outs], grads


def reference_case(Darknet, name, cfg):
    m, outs, grads = run_reference(Darknet, cfg, torch.float64)
    _, outs32, grads32 = run_reference(Darknet, cfg, torch.float32)
    out = {'keys:' + name: np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()]))}
    worst_out = worst_grad = 0.0
    for l, (o, o32) in enumerate(zip(outs, outs32)):
        key = '%s:out%d' % (name, l)
        if o.numel() <= DR.FULL:
            out[key] = o.numpy()
        else:
            flat = o.flatten()
            out[key + ':sample'] = flat[torch.from_numpy(grad_sample_index(flat.numel(), DR.OUT_K))].numpy()
            out[key + ':norm'] = np.float64(float(flat.norm()))
        out[key + ':absmax'] = np.float64(float(o.abs().max()))
        out[key + ':shape'] = np.array(o.shape, dtype=np.int64)
        worst_out = max(worst_out, float((o32.double() - o).abs().max() / o.abs().max()))
    for key, gr in grads.items():
        flat = gr.detach().flatten()
        out['%s:norm:%s' % (name, key)] = np.float64(float(flat.norm()))
        out['%s:sample:%s' % (name, key)] = flat[torch.from_numpy(grad_sample_index(flat.numel(), DR.GRAD_K))].numpy()
        worst_grad = max(worst_grad, rel_l2(grads32[key].flatten(), flat))
    print('%-10s outputs %s  fp32-vs-fp64: outputs %.2e (admit %.1e)  gradients %.2e (admit %.1e)  %d gradients, min norm %.3g' % (
        name, [tuple(o.shape[1:]) for o in outs], worst_out, ADMIT_OUT, worst_grad, ADMIT_GRAD, len(grads),
        min(float(v) for k, v in out.items() if k.startswith(name + ':norm:'))), flush=True)
    out['%s:fp32:worst' % name] = np.array([worst_out, worst_grad])
    assert worst_out <= ADMIT_OUT and worst_grad <= ADMIT_GRAD, 'case %s is ill-conditioned in fp32: change its seed' % name
    return out


def train_flags(Darknet, frozen_stages):
    m = Darknet(depth=DR.SMALL_DEPTH, frozen_stages=frozen_stages)
    m.train()
    return [[[n, bool(p.requires_grad)] for n, p in m.named_parameters()],
            [[n, bool(b.training)] for n, b in m.named_modules() if isinstance(b, nn.BatchNorm2d)]]


def main():
    torch.set_num_threads(min(8, int(os.environ.get('OMP_NUM_THREADS', '8'))))
    Darknet = load_class()
    out = {'cases': np.array(json.dumps(DR.CASES, sort_keys=True))}
    for name, cfg in DR.CASES.items():
        out.update(reference_case(Darknet, name, cfg))
    for k in DR.FLAG_STAGES:
        out['flags:%d' % k] = np.array(json.dumps(train_flags(Darknet, k)))
    try:
        Darknet(depth=7)
        raise AssertionError('the reference built depth 7')
    except KeyError as e:
        out['raises:depth'] = np.array(e.args[0])
        print('unknown depth: the reference raises KeyError:', e.args[0])
    save_npz(DR.GOLDEN, out)
    print(DR.GOLDEN, len(out), 'arrays', os.path.getsize(DR.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
