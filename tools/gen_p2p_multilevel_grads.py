"""Reference gradients of P2PHead on several FPN levels / several points per cell (needs the reference tree; the .npz travels):
  python tools/gen_p2p_multilevel_grads.py
  tests/golden/p2p_multilevel_grads.npz   loss.backward() through the reference's own P2PHead for the forward-pinned cases
                                          ``defaults_k4`` (one level, the 4-point grid) and ``two_levels`` (strides 4 and 8) of
                                          oracle/gen_golden_r6.py, and ``two_levels_k4_c2`` (two levels, the 4-point grid, C = 2:
                                          J = 8 output channels per tower): total loss, and per head parameter / per level's
                                          input feature the L2 norm and a strided sample (oracle.gen_golden.grad_sample_index).
Inputs and head weights are re-derived from the seeds by oracle.gen_golden_r6.head_inputs / head_state_dict (read-only imports).
The archive is written with fixed member timestamps, so a rerun reproduces the file byte for byte."""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.gen_golden import GOLDEN, grad_sample_index  # noqa: E402
from oracle.gen_golden_r6 import HEAD_CASES, SHIPPED_ASSIGNER, build_reference_head, head_inputs  # noqa: E402

GRID4 = [(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)]
CASES = {
    'defaults_k4': HEAD_CASES['defaults_k4'],
    'two_levels': HEAD_CASES['two_levels'],
    'two_levels_k4_c2': dict(C=2, hw=32, G=6, strides=[4, 8], anchors=GRID4, std=0.05, seed=16,
                             loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                             loss_reg=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=0.5), assigner=SHIPPED_ASSIGNER),
}
OUT = os.path.join(GOLDEN, 'p2p_multilevel_grads.npz')


def reference_grads(R, name, cfg):
    head = build_reference_head(R, cfg)
    feats, batch = head_inputs(cfg)
    feats = tuple(f.clone().requires_grad_(True) for f in feats)
    cls_outs, pts_outs = head(feats)
    losses = head.loss(cls_outs, pts_outs, batch['gt_bboxes'], batch['gt_labels'], batch['img_metas'],
                       gt_bboxes_ignore=[torch.zeros((0, 4)) for _ in batch['gt_labels']])
    total = sum(sum(v) for k, v in losses.items())
    total.backward()
    out = {name + ':total_loss': np.float64(float(total.detach()))}
    named = [('bbox_head.' + n, p.grad) for n, p in head.named_parameters()] + [('feat%d' % l, f.grad) for l, f in enumerate(feats)]
    for key, gr in named:
        gr = gr.detach().double().flatten()
        out['%s:norm:%s' % (name, key)] = np.float64(float(gr.norm()))
        out['%s:sample:%s' % (name, key)] = gr[torch.from_numpy(grad_sample_index(gr.numel()))].numpy().astype(np.float32)
    return out


def save_npz(path, arrays):
    """np.savez_compressed's layout with a fixed timestamp on every member (np.load reads it as any .npz)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    from oracle import ref_loader
    assert ref_loader.available(), 'needs the reference tree (oracle/ref_loader.py)'
    torch.set_num_threads(4)
    R = ref_loader.load()
    importlib.import_module('mmdet.models.losses.mse_loss')          # registers MSELoss (the head's own default loss_reg)
    out = {}
    for name, cfg in CASES.items():
        out.update(reference_grads(R, name, cfg))
        print(name, 'total loss', float(out[name + ':total_loss']), flush=True)
    save_npz(OUT, out)
    print(OUT, len(out), 'arrays')


if __name__ == '__main__':
    main()
