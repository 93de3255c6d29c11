"""GPU (-m gpu): BatchNorm2d with batch statistics (layers.bn_train_act,
ld_bn_train_forward / ld_bn_train_backward).

Kernel cases against the float64 restatement of tests/_bn_train_ref64.py at
16 u S (every dispatch path: M = 2, scalar, vector, several slices, a
misaligned view, offset mean, a constant channel), the operand forms (frozen
affine, input without gradient, arena slices), the running statistics, bitwise
determinism, the eval coefficients after a training forward, the blocks and a
whole R18 against torch float64 at the composite bar 2e-4 of each tensor's max,
eager == step list == hipGraph for a GFL-R18 with norm_eval=False, and the
refusals."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_train_ref64 as T  # noqa: E402
import _norm_ref64 as R  # noqa: E402
from _norm_ref64 import BAR, U, check, check_exact, f32, f64  # noqa: E402

pytestmark = pytest.mark.gpu

COMPOSITE = 2e-4  # of each tensor's max: test_gpu_res2net / test_gpu_virtual_ranks


def _dev():
    return torch.device('cuda:0')


def _d(a, grad=False, misalign=False):
    """numpy -> a device leaf; ``misalign``: an offset view, 4 bytes past a
    16-byte boundary."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(_dev())  # (a copy: a is read-only)
    if misalign:
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(t.shape).detach()
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t.requires_grad_(grad)


def _run(inp, relu, with_res, frozen=False, x_grad=True, update=True,
         misalign=False, buffers=None):
    """One forward + backward of the node on a case's operands."""
    from ld_amd import layers as Y
    x = _d(inp['x'], x_grad, misalign)
    g, b = _d(inp['gamma'], not frozen), _d(inp['beta'], not frozen)
    res = _d(inp['res'], True) if with_res else None
    if buffers is None:
        buffers = (_d(inp['running_mean']), _d(inp['running_var']),
                   torch.zeros((), dtype=torch.long, device=_dev()))
    rm, rv, nbt = buffers
    y = Y.bn_train_act(x, g, b, rm, rv, nbt, T.EPS, T.MOMENTUM, res, relu,
                       update_stats=update)
    y.backward(_d(inp['dy']))
    return dict(y=y.detach(), dx=x.grad, dres=res.grad if with_res else None,
                dgamma=g.grad, dbeta=b.grad, running_mean=rm, running_var=rv,
                count=nbt, x=x, g=g, b=b)


def _check_case(ref, got, relu, with_res, what, frozen=False, x_grad=True):
    fwd, bwd, run = ref['fwd'], ref['bwd'], ref['run']
    assert ref['undecided'] == 0
    assert float(fwd['rstd_cancel'].max()) < U
    w = dict(y=check(got['y'], fwd['y'], fwd['S'], what + ' y'))
    if x_grad:
        w['dx'] = check(got['dx'], *bwd['dx'], what + ' dx')
    else:
        assert got['dx'] is None
    if with_res:
        w['dres'] = check(got['dres'], *bwd['dres'], what + ' dres')
    if frozen:
        assert got['dgamma'] is None and got['dbeta'] is None
    else:
        w['dgamma'] = check(got['dgamma'], *bwd['dgamma'], what + ' dgamma')
        w['dbeta'] = check(got['dbeta'], *bwd['dbeta'], what + ' dbeta')
    w['rm'] = check(got['running_mean'], *run['mean'], what + ' running_mean')
    w['rv'] = check(got['running_var'], *run['var'], what + ' running_var')
    assert int(got['count']) == run['count'] == 1
    print(what, {k: round(v, 2) for k, v in w.items()})
    return w


def _check_stats(ref, inp, misalign=False):
    """mean / rstd / scale / shift as the forward leaves them for backward."""
    from ld_amd import layers as Y
    fwd = ref['fwd']
    with torch.no_grad():
        _, scale, mean, rstd = Y._bn_train_forward(
            _d(inp['x'], misalign=misalign), _d(inp['gamma']), _d(inp['beta']),
            None, None, None, T.EPS, T.MOMENTUM, None, False, False)
    check(mean, fwd['mean'], fwd['S_mean'], 'mean')
    check(rstd, fwd['rstd'], fwd['rstd'], 'rstd', bar=fwd['bar_rstd'])
    check(scale, fwd['scale'], fwd['S_scale'], 'scale',
          bar=np.abs(f64(inp['gamma'])) * fwd['bar_rstd'] +
          BAR * U * fwd['S_scale'])


KERNEL_CASES = [(s, '', False) for s in T.SHAPES] + [
    ((2, 40, 1028), '', True),        # offset view: the scalar fallback
    ((2, 40, 1028), 'offset', False),  # x = 256 + noise
    ((2, 40, 1028), 'const', False),   # channel 0 constant: var = 0
]


@pytest.mark.parametrize('relu,with_res', T.FLAGS)
@pytest.mark.parametrize('shape,tag,misalign', KERNEL_CASES)
def test_kernels_against_float64(shape, tag, misalign, relu, with_res):
    ref = T.bn_train_reference(*shape, relu, with_res, tag)
    inp = ref['inp']
    got = _run(inp, relu, with_res, misalign=misalign)
    what = f'{shape} {tag} misalign={misalign} relu={relu} res={with_res}'
    _check_case(ref, got, relu, with_res, what)
    _check_stats(ref, inp, misalign)
    if tag == 'const':
        assert ref['fwd']['var'][0] == 0.0
        rs = 1.0 / np.sqrt(R.eps32(T.EPS))
        assert ref['fwd']['rstd'][0] == rs
    if shape == (1, 3, 2):
        # M = 2: the running variance takes the unbiased factor 2
        var = ref['fwd']['var']
        want = (1 - T.MOMENTUM) * f64(inp['running_var']) + \
            T.MOMENTUM * 2.0 * var
        np.testing.assert_allclose(ref['run']['var'][0], want, rtol=1e-12)


@pytest.mark.parametrize('relu,with_res', [(True, True), (False, False)])
def test_frozen_affine(relu, with_res):
    ref = T.bn_train_reference(2, 40, 1028, relu, with_res)
    got = _run(ref['inp'], relu, with_res, frozen=True)
    _check_case(ref, got, relu, with_res, 'frozen affine', frozen=True)


@pytest.mark.parametrize('shape', [(2, 5, 253), (2, 40, 1028)])
def test_input_without_gradient(shape):
    ref = T.bn_train_reference(*shape, True, True)
    got = _run(ref['inp'], True, True, x_grad=False)
    _check_case(ref, got, True, True, 'no input gradient', x_grad=False)


def test_parameter_gradients_accumulate_into_arena_slices():
    ref = T.bn_train_reference(2, 40, 1028, True, True)
    inp, bwd = ref['inp'], ref['bwd']
    from ld_amd import layers as Y
    assert Y.DIRECT_GRADS[0]
    x, g, b = _d(inp['x'], True), _d(inp['gamma'], True), _d(inp['beta'], True)
    res = _d(inp['res'], True)
    g._ld_grad = torch.zeros(40, device=_dev())
    b._ld_grad = torch.zeros(40, device=_dev())
    rm, rv = _d(inp['running_mean']), _d(inp['running_var'])
    nbt = torch.zeros((), dtype=torch.long, device=_dev())
    for k in range(2):
        y = Y.bn_train_act(x, g, b, rm, rv, nbt, T.EPS, T.MOMENTUM, res, True,
                           update_stats=k == 0)
        y.backward(_d(inp['dy']))
    assert g.grad is None and b.grad is None  # they went into the slices
    # the sum of two equal gradients: twice the value, twice the S
    check(g._ld_grad, 2 * bwd['dgamma'][0], 2 * bwd['dgamma'][1], 'dgamma x 2')
    check(b._ld_grad, 2 * bwd['dbeta'][0], 2 * bwd['dbeta'][1], 'dbeta x 2')
    check(x.grad, 2 * bwd['dx'][0], 2 * bwd['dx'][1], 'dx x 2')
    assert int(nbt) == 1


def test_running_statistics_after_one_and_three_forwards():
    from ld_amd import layers as Y
    inp = T.bn_train_inputs(3, 8, 2050, False, False)
    x, g, b = _d(inp['x']), _d(inp['gamma']), _d(inp['beta'])
    rm, rv = _d(inp['running_mean']), _d(inp['running_var'])
    nbt = torch.zeros((), dtype=torch.long, device=_dev())
    r = dict(mean=(f64(inp['running_mean']), None),
             var=(f64(inp['running_var']), None), count=0)
    for k in range(3):
        with torch.no_grad():  # the no-autograd path updates them too
            Y.bn_train_act(x, g, b, rm, rv, nbt, T.EPS, T.MOMENTUM, None, True)
        r = T.bn_train_running(inp['x'], r['mean'][0], r['var'][0], r['count'],
                               T.MOMENTUM, r['mean'][1], r['var'][1])
        if k in (0, 2):
            check(rm, *r['mean'], f'running_mean after {k + 1}')
            check(rv, *r['var'], f'running_var after {k + 1}')
            assert int(nbt) == r['count'] == k + 1
    before = (rm.clone(), rv.clone(), nbt.clone())
    with torch.no_grad():
        Y.bn_train_act(x, g, b, rm, rv, nbt, T.EPS, T.MOMENTUM, None, True,
                       update_stats=False)
    check_exact(rm, before[0], 'running_mean, update off')
    check_exact(rv, before[1], 'running_var, update off')
    assert int(nbt) == int(before[2]) == 3


@pytest.mark.parametrize('shape', [(3, 8, 2050), (2, 5, 253)])
def test_two_runs_are_bit_identical(shape):
    inp = T.bn_train_inputs(*shape, True, True)
    a, b = _run(inp, True, True), _run(inp, True, True)
    for k in ('y', 'dx', 'dres', 'dgamma', 'dbeta', 'running_mean',
              'running_var', 'count'):
        assert torch.equal(a[k], b[k]), k


def test_small_workspace_is_refused_before_any_launch():
    from ld_amd import lib as L
    lib = L.get_lib()
    N, C, P = 2, 8, 64
    dev = _dev()
    x = torch.randn(N, C, P, device=dev)
    y = torch.full_like(x, 7.0)
    v = [torch.full((C, ), 7.0, device=dev) for _ in range(6)]
    need = lib.ld_bn_train_workspace_bytes(N, C, P)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.ld_bn_train_forward(
        L.ptr(x), None, L.ptr(v[0]), L.ptr(v[1]), 1e-5, 0.1, N, C, P, 1, 1,
        None, None, None, L.ptr(y), L.ptr(v[2]), L.ptr(v[3]), L.ptr(v[4]),
        L.ptr(v[5]), L.ptr(ws), need - 1, L.stream_ptr(dev))
    assert rc == -1
    rc = lib.ld_bn_train_backward(
        L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(v[0]), L.ptr(v[1]), L.ptr(v[2]),
        N, C, P, 1, L.ptr(y), None, L.ptr(v[3]), L.ptr(v[4]), 0, L.ptr(ws),
        need - 1, L.stream_ptr(dev))
    assert rc == -1
    rc = lib.ld_bn_train_backward(  # deferring is refused as well
        L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(v[0]), L.ptr(v[1]), L.ptr(v[2]),
        N, C, P, 1, L.ptr(y), None, L.ptr(v[3]), L.ptr(v[4]), L.LD_GRAD_DEFER,
        L.ptr(ws), need, L.stream_ptr(dev))
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and all(bool((t == 7.0).all()) for t in v)


@pytest.mark.parametrize('trainable', [True, False])
def test_eval_coefficients_follow_a_training_forward(trainable):
    """No optimizer step between: the cached eval scale / shift must not
    survive the raw update of the running statistics."""
    from ld_amd.cnn import build_norm_layer
    inp = T.bn_train_inputs(2, 40, 1028, False, False)
    _, bn = build_norm_layer(dict(type='BN', requires_grad=trainable), 40)
    bn.to(_dev())
    with torch.no_grad():
        bn.weight.copy_(_d(inp['gamma']))
        bn.bias.copy_(_d(inp['beta']))
        bn.running_mean.copy_(_d(inp['running_mean']))
        bn.running_var.copy_(_d(inp['running_var']))
    x = _d(inp['x'])
    old = [f32(bn.running_mean), f32(bn.running_var)]

    def eval_check(what):
        bn.eval()
        with torch.no_grad():
            y = bn.forward3(x, None, False)
        ref = R.bn_forward(inp['x'], inp['gamma'], inp['beta'],
                           f32(bn.running_mean), f32(bn.running_var), bn.eps)
        check(y, ref['y'], ref['S'], what)
    eval_check('before')  # fills the cache
    bn.train()
    with torch.enable_grad():
        bn.forward3(x, None, True)
    assert not np.array_equal(f32(bn.running_mean), old[0])
    assert not np.array_equal(f32(bn.running_var), old[1])
    assert int(bn.num_batches_tracked) == 1
    eval_check('after the training forward')


# ------------------------------------------------------------- the modules --
def _f64_leaves(mod):
    P = {k: v.detach().double().cpu().requires_grad_(v.requires_grad)
         for k, v in mod.named_parameters()}
    B = {k: v.detach().cpu().double() if v.dtype.is_floating_point
         else v.detach().cpu().clone() for k, v in mod.named_buffers()}
    return P, B


def _ref_cb(P, B, mod, conv, bn, x, res=None, relu=True):
    """conv -> BN (in the module's own mode) -> (+ res) -> ReLU with torch
    float64 ops on the CPU; updates B as nn.BatchNorm2d would."""
    c, n = mod.get_submodule(conv), mod.get_submodule(bn)
    y = F.conv2d(x, P[conv + '.weight'], None, c.stride, c.padding, 1,
                 getattr(c, 'groups', 1))
    y = F.batch_norm(y, B[bn + '.running_mean'], B[bn + '.running_var'],
                     P[bn + '.weight'], P[bn + '.bias'], n.training,
                     n.momentum, n.eps)
    if n.training:
        B[bn + '.num_batches_tracked'] += 1
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def _ref_basic(P, B, mod, pre, x):
    blk = mod.get_submodule(pre.rstrip('.')) if pre else mod
    out = _ref_cb(P, B, mod, pre + 'conv1', pre + 'bn1', x)
    idt = x
    if blk.downsample is not None:
        idt = _ref_cb(P, B, mod, pre + 'downsample.0', pre + 'downsample.1', x,
                      relu=False)
    return _ref_cb(P, B, mod, pre + 'conv2', pre + 'bn2', out, res=idt)


def _ref_bottleneck(P, B, mod, pre, x):
    out = _ref_cb(P, B, mod, pre + 'conv1', pre + 'bn1', x)
    out = _ref_cb(P, B, mod, pre + 'conv2', pre + 'bn2', out)
    idt = _ref_cb(P, B, mod, pre + 'downsample.0', pre + 'downsample.1', x,
                  relu=False)
    return _ref_cb(P, B, mod, pre + 'conv3', pre + 'bn3', out, res=idt)


def _ref_conv_module(P, B, mod, pre, x):
    return _ref_cb(P, B, mod, 'conv', 'bn', x)


def _down(cin, cout, stride):
    from ld_amd.cnn import build_conv_layer, build_norm_layer
    return nn.Sequential(
        build_conv_layer(None, cin, cout, 1, stride=stride, bias=False),
        build_norm_layer(dict(type='BN'), cout)[1])


def _make_block(kind):
    from ld_amd.cnn import ConvModule
    from ld_amd.resnet import BasicBlock, Bottleneck, ResNeXtBottleneck
    torch.manual_seed(5)
    if kind == 'basic':
        return BasicBlock(16, 16, stride=2, downsample=_down(16, 16, 2)), 16, \
            _ref_basic
    if kind == 'bottleneck':
        return Bottleneck(64, 16, stride=2, downsample=_down(64, 64, 2)), 64, \
            _ref_bottleneck
    if kind == 'resnext':
        return ResNeXtBottleneck(64, 64, groups=8, base_width=8, stride=2,
                                 downsample=_down(64, 256, 2)), 64, \
            _ref_bottleneck
    return ConvModule(16, 64, 3, padding=1, norm_cfg=dict(type='BN')), 16, \
        _ref_conv_module


def _randomise_norms(mod, seed):
    g = torch.Generator().manual_seed(seed)
    from ld_amd.cnn import BatchNorm2d
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))


def _gap(got, ref):
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu().reshape(ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _block_gaps(kind, training):
    blk, cin, restate = _make_block(kind)
    _randomise_norms(blk, 11)
    blk.to(_dev())
    blk.train(training)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, cin, 16, 24, generator=g)
    P, B = _f64_leaves(blk)
    x64 = x.double().requires_grad_(True)
    y64 = restate(P, B, blk, '', x64)
    dy = torch.randn(y64.shape, generator=g)
    y64.backward(dy.double())
    xd = x.to(_dev()).requires_grad_(True)
    y3, lv = blk.forward3(xd.reshape(2, cin, -1), ((16, 24), ))
    y = y3.view(2, -1, lv[0][0], lv[0][1])
    y.backward(dy.to(_dev()))
    gaps = dict(y=_gap(y, y64), dx=_gap(xd.grad, x64.grad))
    for k, p in blk.named_parameters():
        gaps['d ' + k] = _gap(p.grad, P[k].grad)
    for k, b in blk.named_buffers():
        if b.dtype.is_floating_point:
            gaps[k] = _gap(b, B[k])
        else:
            assert int(b) == int(B[k]) == (1 if training else 0), k
    return gaps


@pytest.mark.parametrize('kind', ['basic', 'bottleneck', 'resnext',
                                  'conv_module'])
def test_blocks_against_torch_float64(kind):
    ev = _block_gaps(kind, False)  # the existing eval-mode code, same bar
    tr = _block_gaps(kind, True)
    we, wt = max(ev, key=ev.get), max(tr, key=tr.get)
    print(f'{kind}: eval gap {ev[we]:.3g} ({we}); training gap {tr[wt]:.3g} '
          f'({wt})')
    assert ev[we] <= COMPOSITE, (we, ev[we])
    assert tr[wt] <= COMPOSITE, (wt, tr[wt])


def _ref_r18(P, B, net, x):
    y = _ref_cb(P, B, net, 'conv1', 'bn1', x)
    y = F.max_pool2d(y, 3, 2, 1)
    outs = []
    for i in range(1, 5):
        for j in range(len(getattr(net, f'layer{i}'))):
            y = _ref_basic(P, B, net, f'layer{i}.{j}.', y)
        outs.append(y)
    return outs


def test_resnet18_norm_eval_false_against_torch_float64():
    from ld_amd import synthetic
    from ld_amd.resnet import ResNet
    net = ResNet(depth=18, frozen_stages=1, norm_eval=False)
    net.load_state_dict(synthetic.seeded_state_dict(net.state_dict(), seed=3))
    net.to(_dev()).train()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 64, 96, generator=g)
    P, B = _f64_leaves(net)
    outs64 = _ref_r18(P, B, net, x.double())
    dys = [torch.randn(o.shape, generator=g) for o in outs64]
    # stage 0 is the frozen layer1: it carries no gradient on either side
    assert [o.requires_grad for o in outs64] == [False, True, True, True]
    torch.autograd.backward(outs64[1:], [d.double() for d in dys[1:]])
    outs = net(x.to(_dev()))
    assert outs[3].shape[2:] == (2, 3)  # layer4: M = 2 * 2 * 3 = 12
    assert [o.requires_grad for o in outs] == [False, True, True, True]
    torch.autograd.backward(list(outs[1:]), [d.to(_dev()) for d in dys[1:]])
    gaps = {f'stage {i}': _gap(o, r)
            for i, (o, r) in enumerate(zip(outs, outs64))}
    n_grad = 0
    for k, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, k
            gaps['d ' + k] = _gap(p.grad, P[k].grad)
            n_grad += 1
        else:
            assert p.grad is None and k.startswith(('conv1', 'bn1', 'layer1'))
    assert n_grad > 30
    for k, b in net.named_buffers():
        trained = k.startswith(('layer2', 'layer3', 'layer4'))
        if b.dtype.is_floating_point:
            gaps[k] = _gap(b, B[k])
        else:
            assert int(b) == int(B[k]) == (1 if trained else 0), k
    worst = max(gaps, key=gaps.get)
    print(f'R18 norm_eval=False: worst gap {gaps[worst]:.3g} ({worst}) of '
          f'{len(gaps)} tensors')
    assert gaps[worst] <= COMPOSITE, (worst, gaps[worst])


# ----------------------------------------------------------------- capture --
def _gfl_r18():
    from ld_amd import model_zoo, synthetic
    from ld_amd.registry import build_detector
    cfg = copy.deepcopy(model_zoo.gfl_detector(18))
    cfg['backbone']['norm_eval'] = False
    det = build_detector(cfg)
    det.load_state_dict(synthetic.seeded_state_dict(det.state_dict(), seed=1))
    return det.to(_dev()).train()


def _batch(seed):
    from ld_amd import synthetic
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), [3, 2], seed)
    return dict(img=b['img'].to(_dev()), img_metas=b['img_metas'],
                gt_bboxes=[x.to(_dev()) for x in b['gt_bboxes']],
                gt_labels=[x.to(_dev()) for x in b['gt_labels']])


def _trainer():
    from ld_amd.train import SGDTrainer
    return SGDTrainer(_gfl_r18(), lr=0.01)


def _assert_same_state(tr, eager, what):
    assert torch.equal(tr.arena.flat_param, eager.arena.flat_param), what
    assert torch.equal(tr.flat_momentum, eager.flat_momentum), what
    eb = dict(eager.model.named_buffers())
    n = 0
    for k, b in tr.model.named_buffers():
        assert torch.equal(b, eb[k]), (what, k)
        n += k.endswith('num_batches_tracked') and int(b) == 3
    assert n >= 15, (what, n)  # the norm layers of layer2-4 counted 3 batches


def test_three_steps_eager_equals_captured():
    from ld_amd import train as TR
    eager = _trainer()
    from ld_amd.cnn import BatchNorm2d
    assert any(m.training for m in eager.model.modules()
               if isinstance(m, BatchNorm2d))
    for _ in range(3):
        out_e = eager.step(_batch(21))
    torch.cuda.synchronize()
    launchers = ['list'] + (['graph'] if TR.graph_queues_ok() else [])
    for launcher in launchers:
        tr = _trainer()
        g = TR.GraphedStep(tr, _batch(21), warmup=1, launcher=launcher)
        g.replay()
        out_g = g.replay()
        torch.cuda.synchronize()
        _assert_same_state(tr, eager, launcher)
        assert float(out_g['loss']) == float(out_e['loss']), launcher
        assert np.isfinite(float(out_g['loss']))


# ---------------------------------------------------------------- refusals --
def test_refuses_bf16_mode_on_the_device():
    from ld_amd import layers as Y
    from ld_amd.cnn import BatchNorm2d
    bn = BatchNorm2d(16).to(_dev()).train()
    before = bn.running_mean.clone()
    Y.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16'):
            bn.forward3(torch.randn(2, 16, 24, device=_dev()))
    finally:
        Y.set_precision('fp32')
    assert torch.equal(bn.running_mean, before) and \
        int(bn.num_batches_tracked) == 0


def test_refuses_training_bn_after_dcn_on_the_device():
    from ld_amd.cnn import BatchNorm2d, build_conv_layer
    from ld_amd.resnet import _conv_bn
    conv = build_conv_layer(dict(type='DCN', deform_groups=1), 16, 16, 3,
                            padding=1, bias=False).to(_dev())
    bn = BatchNorm2d(16).to(_dev()).train()
    with pytest.raises(NotImplementedError, match='DeformConv2dPack'):
        _conv_bn(torch.randn(2, 16, 12, device=_dev()), ((3, 4), ), conv, bn)
    assert int(bn.num_batches_tracked) == 0


def test_refuses_virtual_ranks_with_a_training_bn():
    from ld_amd.train import SGDTrainer
    det = _gfl_r18()
    with pytest.raises(NotImplementedError, match='virtual_ranks=2'):
        SGDTrainer(det, lr=0.01, virtual_ranks=2)
    det.backbone.norm_eval = True
    det.train()
    tr = SGDTrainer(det, lr=0.01, virtual_ranks=2)  # eval-mode norms: accepted
    det.backbone.norm_eval = False
    det.train()
    with pytest.raises(NotImplementedError, match='training mode'):
        tr.step([_batch(21), _batch(22)])


def test_refuses_one_value_per_channel_on_the_device():
    from ld_amd.cnn import BatchNorm2d
    bn = BatchNorm2d(16).to(_dev()).train()
    with pytest.raises(ValueError, match='Expected more than 1 value'):
        bn.forward3(torch.randn(1, 16, 1, device=_dev()))
