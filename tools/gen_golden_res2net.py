"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/res2net.npz by EXECUTING THE
REFERENCE's Res2Net on CPU (the reference package is imported, unmodified,
through oracle/ref_shim.py).  Run from the repo root in the build container,
never on the GPU machine:

    python tools/gen_golden_res2net.py

Reference entry points exercised (file:line under the reference tree):
  mmdet/models/backbones/res2net.py:17-162   Bottle2neck
  mmdet/models/backbones/res2net.py:165-241  Res2Layer (avg_down shortcut)
  mmdet/models/backbones/res2net.py:244-351  Res2Net (deep stem)

Weights are ld_amd.synthetic.seeded_state_dict, inputs and cotangents come from
seeded generators; only the reference's results are stored:
  d{50,101}_keys / _shapes   state_dict key list and shapes (no DCN: the
                             reference's DCN op does not run here)
  {case}_cfg                 depth, n, h, w, seed, step
  {case}_shape{i} / _out{i}  stage output i, every ``step``-th element (fp32)
  r2_50_grad_names           sampled parameters (+ 'x1': the input of layer2)
  r2_50_grad_steps           the sampling stride of each
  r2_50_g64_{j}              float64 gradient, every step-th element
  r2_50_e32_{j}              max |float32 run - float64 run| on that sample
The gradient run: frozen_stages=1, norm_eval=True, train(); the stem and layer1
run under no_grad, their output x1 is a leaf, the loss is sum_i <out_i, cot_i>
over the four outputs (out_0 = x1) with cot_i = randn(seed COT_SEED + i).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, REPO)

import gen_golden as G  # noqa: E402,F401  (installs ref_shim)

from ld_amd import synthetic  # noqa: E402

CASES = [  # name, depth, (n, h, w), seed
    ('r2_50', 50, (2, 64, 96), 41),
    ('r2_101', 101, (1, 70, 90), 43),
]
OUT_CAP = 4000  # stored elements per stage output
GRAD_CAP = 1500  # stored elements per gradient
COT_SEED = 500
GRAD_PARAMS = (
    ['layer2.0.convs.%d.weight' % i for i in range(3)] +
    ['layer2.0.bns.%d.%s' % (i, p) for i in range(3)
     for p in ('weight', 'bias')] +
    ['layer2.0.downsample.1.weight', 'layer2.0.downsample.2.weight',
     'layer2.0.downsample.2.bias'] +
    ['layer2.1.convs.%d.weight' % i for i in range(3)] +
    ['layer2.1.bns.%d.%s' % (i, p) for i in range(3)
     for p in ('weight', 'bias')] +
    ['layer3.0.conv1.weight', 'layer3.0.bn1.weight', 'layer3.0.bn1.bias',
     'layer4.2.conv3.weight', 'layer4.2.bn3.weight', 'layer4.2.bn3.bias'])


def sample_step(numel, cap):
    """An odd stride that keeps at most about ``cap`` elements."""
    return max(1, numel // cap) | 1


def cotangents(shapes):
    return [torch.randn(tuple(s), generator=torch.Generator().manual_seed(
        COT_SEED + i)) for i, s in enumerate(shapes)]


def _build(depth, seed, **kw):
    from mmdet.models.backbones import Res2Net
    net = Res2Net(depth=depth, scales=4, base_width=26, **kw)
    net.load_state_dict(synthetic.seeded_state_dict(net.state_dict(),
                                                    seed=seed))
    return net


def _grads(net, x, dtype):
    """-> {name: flat gradient} of GRAD_PARAMS and 'x1'."""
    net = net.to(dtype)
    net.train()
    with torch.no_grad():
        x1 = net.maxpool(net.stem(x.to(dtype)))
        x1 = net.layer1(x1)
    x1.requires_grad_(True)
    outs, t = [x1], x1
    for name in net.res_layers[1:]:
        t = getattr(net, name)(t)
        outs.append(t)
    cots = cotangents([o.shape for o in outs])
    loss = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots))
    for p in net.parameters():
        p.grad = None
    loss.backward()
    params = dict(net.named_parameters())
    g = {k: params[k].grad.detach().reshape(-1).clone() for k in GRAD_PARAMS}
    g['x1'] = x1.grad.detach().reshape(-1).clone()
    return g


def main():
    d = {}
    for name, depth, (n, h, w), seed in CASES:
        net = _build(depth, seed)
        net.eval()
        sd = net.state_dict()
        d[f'd{depth}_keys'] = np.array(list(sd.keys()))
        d[f'd{depth}_shapes'] = np.array(
            ['x'.join(str(v) for v in t.shape) for t in sd.values()])
        x = torch.randn(n, 3, h, w,
                        generator=torch.Generator().manual_seed(seed + 100))
        with torch.no_grad():
            outs = net(x)
        step = max(sample_step(o.numel(), OUT_CAP) for o in outs)
        d[name + '_cfg'] = np.array([depth, n, h, w, seed, step])
        for i, o in enumerate(outs):
            d[f'{name}_shape{i}'] = np.array(o.shape)
            d[f'{name}_out{i}'] = o.numpy().reshape(-1)[::step].astype(
                np.float32)
        print(name, [tuple(o.shape) for o in outs], 'step', step)
        if name != 'r2_50':
            continue
        net = _build(depth, seed, frozen_stages=1, norm_eval=True)
        g32 = _grads(net, x, torch.float32)
        g64 = _grads(net, x, torch.float64)
        names = GRAD_PARAMS + ['x1']
        steps = [sample_step(g64[k].numel(), GRAD_CAP) for k in names]
        d[name + '_grad_names'] = np.array(names)
        d[name + '_grad_steps'] = np.array(steps)
        for j, (k, s) in enumerate(zip(names, steps)):
            a64 = g64[k][::s].numpy()
            d[f'{name}_g64_{j}'] = a64
            d[f'{name}_e32_{j}'] = np.array(float(np.abs(
                g32[k][::s].double().numpy() - a64).max()))
            print(f'  {k}: max|g| {np.abs(a64).max():.3e} fp32 err '
                  f'{float(d[f"{name}_e32_{j}"]):.3e}')
    path = os.path.join(REPO, 'tests', 'golden', 'res2net.npz')
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
