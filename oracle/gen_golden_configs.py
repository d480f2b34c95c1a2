"""Merged model / schedule configs of the reference's shipped config files (build container only; test infrastructure).

  python -m oracle.gen_golden_configs

  tests/golden/reference_configs.json   for each config file of CONFIGS: the result of
                                        ``Config.fromfile`` on the reference tree (``_base_`` chain merged, ``_delete_`` applied),
                                        restricted to what the drop-in build and its checks read: model, train_cfg, test_cfg,
                                        optimizer_config, checkpoint_config and the per-GPU batch of ``data``.
Tuples are stored as {"__tuple__": [...]} so the builders see the types the files wrote."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
# paths under the reference tree; tests/test_host_cpu.py::test_reference_configs_build_unmodified runs once per entry
CONFIGS = [
    'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_1x_TinyPersonV2_640.py',
    'configs2/TinyPersonV2/coarsepointv2/coarse_point_refine_r50_fpns4_0.5x_TinyPersonV2_640.py',
    'configs2/COCO/coarsepointv2/coarse_point_refine_r50_fpn_1x_coco400.py',
    'configs2/COCO/coarsepointv2/coarse_point_refine_r101_fpn_1x_coco400.py',
    'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_1x_fl_sl1_TinyPersonV2_640.py',
    'configs2/TinyPersonV2/p2p/p2p_r50_fpns4_0.5x_fl_sl1_TinyPersonV2_640.py',
    'configs2/COCO/p2p/p2p_r101_fpn_1x_fl_sl1_coco400_coarse.py',
    'configs2/COCO/p2p/p2p_r50_fpn_1x_fl_sl1_coco400_coarse.py',
    'configs2/COCO/p2p/p2p_r50_fpns4_1x_fl_sl1_coco.py',
    'configs2/DOTA/coarsepointv2/coarse_point_refine_r50_fpns4_1x_DOTA_1024.py',
    'configs2/DOTA/p2p/p2p_r50_fpn_1x_fl_sl1_DOTA_coarse.py',
    'configs2/_base_/models/cpr/coarse_point_refine_r50_fpns4_1x.py',    # refine_bag_policy='only_refine_bag'
]

KEYS = ('model', 'train_cfg', 'test_cfg', 'optimizer_config', 'checkpoint_config')
DATA_KEYS = ('samples_per_gpu', 'workers_per_gpu')


def encode(o):
    if isinstance(o, dict):
        return {k: encode(v) for k, v in o.items()}
    if isinstance(o, tuple):
        return {'__tuple__': [encode(v) for v in o]}
    if isinstance(o, list):
        return [encode(v) for v in o]
    assert o is None or isinstance(o, (bool, int, float, str)), type(o)
    return o


def decode(o):
    """Inverse of ``encode`` (used by the tests)."""
    if isinstance(o, dict):
        if set(o) == {'__tuple__'}:
            return tuple(decode(v) for v in o['__tuple__'])
        return {k: decode(v) for k, v in o.items()}
    if isinstance(o, list):
        return [decode(v) for v in o]
    return o


def run(configs=CONFIGS):
    from oracle import ref_loader
    from pointtinybenchmark_amd.config import Config
    assert ref_loader.available(), 'needs the reference tree (%s)' % ref_loader.REF_ROOT
    out = {}
    for rel in configs:
        cfg = Config.fromfile(os.path.join(ref_loader.REF_ROOT, rel))
        rec = {k: encode(cfg[k]) for k in KEYS if k in cfg}
        if 'data' in cfg:
            rec['data'] = {k: cfg.data[k] for k in DATA_KEYS if k in cfg.data}
        out[rel] = rec
    path = os.path.join(GOLDEN, 'reference_configs.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return path


if __name__ == '__main__':
    print(run())
