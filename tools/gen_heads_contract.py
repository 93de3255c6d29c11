"""Writes tests/golden/heads_contract.json: for each of the ten registered dense
heads, built on the CPU with the constructor arguments of its GPU tests, the
ordered state_dict keys, the ordered (name, shape) of named_parameters and,
after ``torch.manual_seed(0); head.init_weights()``, the order of the normal_
draws and the float64 sum of every parameter (together they pin the order in
which init_weights draws from the RNG).

Checkpoints, the optimizer wire format and GradArena's buckets are functions
of these orders; tests/test_heads_contract_host.py compares a fresh build with
the file.  Only public constructors and init_weights are used, so the same
script describes any commit:

    python tools/gen_heads_contract.py --provenance 'commit <sha>'
"""
import argparse
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

OUT = os.path.join(REPO, 'tests', 'golden', 'heads_contract.json')

_KD = 'KnowledgeDistillationKLDivLoss'
_FOCAL = dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25,
              loss_weight=1.0)
_CTR = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)


def head_configs():
    """name -> build_head config, as tests/test_gpu_{lossblock,v2,imitation,
    atss,fcos,retina}.py build them."""
    from ld_amd import model_zoo
    from ld_amd.config import ConfigDict
    cfgs = {}
    for name, det in (('GFLHead', model_zoo.gfl_detector(101)),
                      ('LDHead', model_zoo.ld_detector(50, 101)),
                      ('GFocalHead', model_zoo.gflv2_detector(101)),
                      ('LDv2Head', model_zoo.ldv2_detector(50, 101))):
        cfgs[name] = dict(det['bbox_head'],
                          train_cfg=ConfigDict.wrap(model_zoo._TRAIN_CFG),
                          test_cfg=ConfigDict.wrap(model_zoo._TEST_CFG))
    atss = dict(
        num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', ratios=[1.0],
                              octave_base_scale=8, scales_per_octave=1,
                              strides=[8, 16, 32, 64, 128]),
        bbox_coder=dict(type='DeltaXYWHBBoxCoder',
                        target_means=[.0, .0, .0, .0],
                        target_stds=[0.1, 0.1, 0.2, 0.2]),
        loss_cls=_FOCAL, loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
        loss_centerness=_CTR,
        train_cfg=ConfigDict.wrap(dict(
            assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1,
            pos_weight=-1, debug=False)))
    fcos = dict(
        num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
        strides=[8, 16, 32, 64, 128], loss_cls=_FOCAL,
        loss_bbox=dict(type='GIoULoss', loss_weight=1.0),
        loss_centerness=_CTR, norm_on_bbox=False, centerness_on_reg=True,
        dcn_on_last_conv=False, center_sampling=True, conv_bias=True)
    retina = dict(
        num_classes=80, in_channels=256, stacked_convs=4, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4,
                              scales_per_octave=3, ratios=[0.5, 1.0, 2.0],
                              strides=[8, 16, 32, 64, 128]),
        bbox_coder=dict(type='DeltaXYWHBBoxCoder',
                        target_means=[.0, .0, .0, .0],
                        target_stds=[1.0, 1.0, 1.0, 1.0]),
        loss_cls=_FOCAL, loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
        reg_decoded_bbox=True,
        train_cfg=ConfigDict.wrap(dict(
            assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5,
                          neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1),
            allowed_border=-1, pos_weight=-1, debug=False)))
    for plain, ld, common, lw_ld, t_kd in (
            ('ATSSGFLHead', 'LDATSSHead', atss, 0.25, 2),
            ('FCOSGFLHead', 'LDFCOSHead', fcos, 0.25, 2),
            ('RetinaGFLHead', 'LDRetinaHead', retina, 5, 8)):
        cfgs[plain] = dict(common, type=plain)
        cfgs[ld] = dict(common, type=ld,
                        loss_ld=dict(type=_KD, loss_weight=lw_ld, T=10),
                        loss_kd=dict(type=_KD, loss_weight=10, T=t_kd))
    return cfgs


def rng_probe():
    """float64 sum of a fixed seeded normal_ draw.  normal_ goes through
    SIMD math that differs by an ulp between CPU families, so sums of drawn
    weights compare with ``==`` only where this probe reproduces."""
    import torch
    torch.manual_seed(0)
    return _sum64(torch.empty(4099).normal_(0, 0.01))


def _sum64(t):
    # numpy's pairwise float64 sum: one thread, a fixed order
    import numpy as np
    return float(np.add.reduce(t.detach().double().numpy().ravel()))


def init_head(cfg):
    """build_head(cfg) on the CPU, then ``torch.manual_seed(0);
    head.init_weights()`` -> (head, [[name, mean, std], ...] of the normal_
    draws in the order init_weights made them)."""
    import torch
    from ld_amd.registry import build_head
    head = build_head(copy.deepcopy(cfg))
    names = {id(p): n for n, p in head.named_parameters()}
    draws, normal_ = [], torch.nn.init.normal_

    def logged(tensor, mean=0.0, std=1.0, **kw):
        draws.append([names[id(tensor)], float(mean), float(std)])
        return normal_(tensor, mean, std, **kw)

    torch.nn.init.normal_ = logged
    try:
        torch.manual_seed(0)
        head.init_weights()
    finally:
        torch.nn.init.normal_ = normal_
    return head, draws


def replay_mismatches(head, draws):
    """Names of the parameters that are not bit-equal to the same draws made
    afresh, in the order ``draws``, on this machine (machine-independent: both
    sides use this machine's normal_)."""
    import torch
    params = dict(head.named_parameters())
    torch.manual_seed(0)
    return [n for n, mean, std in draws
            if not torch.equal(params[n].detach(),
                               torch.empty_like(params[n]).normal_(mean, std))]


def contract(cfg):
    """The pinned views of one head built from ``cfg`` on the CPU."""
    head, draws = init_head(cfg)
    assert not replay_mismatches(head, draws)
    return dict(
        state_dict=list(head.state_dict()),
        parameters=[[n, list(p.shape)] for n, p in head.named_parameters()],
        init_draws=draws,
        init_sums=[_sum64(p) for p in head.parameters()])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--provenance', required=True,
                    help='what the file was generated from (the commit)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    doc = dict(provenance=args.provenance, rng_probe=rng_probe(),
               heads={k: contract(c) for k, c in head_configs().items()})
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
