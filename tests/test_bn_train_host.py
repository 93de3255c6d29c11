"""Training-mode BatchNorm2d without a device: tests/_bn_train_ref64.py equals
torch's own definition in float64, the 16 u S bars are sharp (planted defects
on an fp32 restatement of the device's operations break them, the restatement
itself passes), the backbones put the right norm layers in training mode, and
the refusals that need no device are raised by name."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_train_ref64 as T  # noqa: E402
from _norm_ref64 import check  # noqa: E402

HOST_SHAPES = ((1, 3, 2), (2, 5, 253), (3, 8, 2050))


def _t(a, grad=False):
    t = torch.from_numpy(np.asarray(a, dtype=np.float64).copy())
    return t.requires_grad_(grad)


@pytest.mark.parametrize('relu,with_res', T.FLAGS)
@pytest.mark.parametrize('shape', HOST_SHAPES)
def test_restatement_equals_torch_float64(shape, relu, with_res):
    ref = T.bn_train_reference(*shape, relu, with_res)
    inp, fwd, bwd = ref['inp'], ref['fwd'], ref['bwd']
    e32 = T.eps32(T.EPS)
    x, g, b = _t(inp['x'], True), _t(inp['gamma'], True), _t(inp['beta'], True)
    res = _t(inp['res'], True) if with_res else None
    rm, rv = _t(inp['running_mean']), _t(inp['running_var'])
    bn = torch.nn.BatchNorm2d(shape[1], eps=e32, momentum=T.MOMENTUM).double()
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    y = F.batch_norm(x[..., None], bn.running_mean, bn.running_var, g, b, True,
                     T.MOMENTUM, e32)[..., 0]
    bn.num_batches_tracked += 1  # what nn.BatchNorm2d.forward does beside it
    if with_res:
        y = y + res
    if relu:
        y = torch.relu(y)
    y.backward(_t(inp['dy']))
    kw = dict(rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(fwd['y'], y.detach().numpy(), **kw)
    np.testing.assert_allclose(bwd['dx'][0], x.grad.numpy(), **kw)
    np.testing.assert_allclose(bwd['dgamma'][0], g.grad.numpy(), **kw)
    np.testing.assert_allclose(bwd['dbeta'][0], b.grad.numpy(), **kw)
    if with_res:
        np.testing.assert_allclose(bwd['dres'][0], res.grad.numpy(), **kw)
    run = ref['run']
    np.testing.assert_allclose(run['mean'][0], bn.running_mean.numpy(), **kw)
    np.testing.assert_allclose(run['var'][0], bn.running_var.numpy(), **kw)
    assert run['count'] == int(bn.num_batches_tracked) == 1


def test_three_updates_equal_the_torch_module():
    inp = T.bn_train_inputs(2, 5, 253, False, False)
    bn = torch.nn.BatchNorm2d(5, eps=T.EPS, momentum=T.MOMENTUM).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(_t(inp['running_mean']))
        bn.running_var.copy_(_t(inp['running_var']))
    rm, rv, cnt = T.f64(inp['running_mean']), T.f64(inp['running_var']), 0
    for k in range(3):
        xk = (inp['x'] * np.float32(k + 1)).astype(np.float32)
        bn(_t(xk)[..., None])
        r = T.bn_train_running(xk, rm, rv, cnt, T.MOMENTUM)
        rm, rv, cnt = r['mean'][0], r['var'][0], r['count']
    np.testing.assert_allclose(rm, bn.running_mean.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rv, bn.running_var.numpy(), rtol=1e-9, atol=1e-9)
    assert cnt == int(bn.num_batches_tracked) == 3


def _emulated(shape, relu, with_res, tag='', defect=None):
    ref = T.bn_train_reference(*shape, relu, with_res, tag)
    inp = ref['inp']
    got = T.device_emulation(inp['x'], inp['gamma'], inp['beta'], T.EPS,
                             T.MOMENTUM, inp['running_mean'],
                             inp['running_var'], inp['dy'], inp['res'], relu,
                             defect)
    return ref, got


def _check_all(ref, got, only=None):
    fwd, bwd, run = ref['fwd'], ref['bwd'], ref['run']
    worst = {}
    pairs = dict(
        y=(fwd['y'], fwd['S'], None), mean=(fwd['mean'], fwd['S_mean'], None),
        rstd=(fwd['rstd'], fwd['rstd'], fwd['bar_rstd']),
        running_mean=run['mean'] + (None, ), running_var=run['var'] + (None, ),
        dx=bwd['dx'] + (None, ), dres=bwd['dres'] + (None, ),
        dgamma=bwd['dgamma'] + (None, ), dbeta=bwd['dbeta'] + (None, ))
    for name, (val, S, bar) in pairs.items():
        if only is None or name in only:
            worst[name] = check(got[name], val, S, name, bar=bar)
    return worst


EMULATED = [(s, '') for s in HOST_SHAPES + ((2, 40, 1028), )] + \
    [((2, 40, 1028), 'offset'), ((2, 40, 1028), 'const')]


@pytest.mark.parametrize('relu,with_res', T.FLAGS)
@pytest.mark.parametrize('shape,tag', EMULATED)
def test_device_arithmetic_fits_the_bars(shape, relu, with_res, tag):
    """The fp32 restatement of the kernels' operations stays inside every bar:
    the rounding counts of the helper's docstring hold."""
    ref, got = _emulated(shape, relu, with_res, tag)
    assert ref['undecided'] == 0
    assert float(ref['fwd']['rstd_cancel'].max()) < T.U
    worst = _check_all(ref, got)
    print(shape, relu, with_res, tag, {k: round(v, 2) for k, v in worst.items()})
    if tag == 'const':
        assert ref['fwd']['var'][0] == 0.0
        assert ref['fwd']['rstd'][0] == 1.0 / np.sqrt(T.eps32(T.EPS))


# which result each defect must push outside its bar
BROKEN_BY = dict(running_var_biased='running_var', norm_var_unbiased='y',
                 dx_m_minus_1='dx', dx_no_xhat_term='dx', stats_drop_one='mean',
                 dgamma_drop_one='dgamma')


@pytest.mark.parametrize('defect', T.DEFECTS)
@pytest.mark.parametrize('shape', [(2, 5, 253), (3, 8, 2050)])
def test_planted_defect_breaks_the_bar(shape, defect):
    ref, got = _emulated(shape, True, True, defect=defect)
    with pytest.raises(AssertionError, match='outside the bar'):
        _check_all(ref, got, only=(BROKEN_BY[defect], ))


def test_every_defect_is_planted():
    assert set(BROKEN_BY) == set(T.DEFECTS)


# ------------------------------------------------------------ module logic --
def _bn_modes(net):
    from ld_amd.cnn import BatchNorm2d
    return {n: m.training for n, m in net.named_modules()
            if isinstance(m, BatchNorm2d)}


def _backbones():
    from ld_amd.resnet import Res2Net, ResNet, ResNeXt
    return (
        (ResNet, dict(depth=18)),
        (ResNeXt, dict(depth=50, groups=32, base_width=4)),
        (Res2Net, dict(depth=50, scales=4, base_width=26)),
    )


@pytest.mark.parametrize('i', range(3))
def test_norm_eval_false_trains_the_unfrozen_stages(i):
    cls, kw = _backbones()[i]
    net = cls(frozen_stages=1, norm_eval=False, **kw).train()
    modes = _bn_modes(net)
    assert modes
    for name, training in modes.items():
        frozen = not name.startswith(('layer2', 'layer3', 'layer4'))
        assert training == (not frozen), name
    assert not any(_bn_modes(net.eval()).values())


@pytest.mark.parametrize('i', range(3))
def test_norm_eval_true_is_unchanged(i):
    cls, kw = _backbones()[i]
    net = cls(frozen_stages=1, norm_eval=True, **kw).train()
    assert not any(_bn_modes(net).values())


@pytest.mark.parametrize('i', range(3))
def test_state_dict_keys_do_not_depend_on_norm_eval(i):
    cls, kw = _backbones()[i]
    a = cls(frozen_stages=1, norm_eval=False, **kw).train().state_dict()
    b = cls(frozen_stages=1, norm_eval=True, **kw).train().state_dict()
    assert list(a) == list(b)
    assert any(k.endswith('num_batches_tracked') for k in a)
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)


# ---------------------------------------------------------------- refusals --
def _train_bn(c=4, **kw):
    from ld_amd.cnn import BatchNorm2d
    return BatchNorm2d(c, **kw).train()


def test_refuses_one_value_per_channel():
    bn = _train_bn()
    with pytest.raises(ValueError,
                       match='Expected more than 1 value per channel'):
        bn.forward3(torch.zeros(1, 4, 1))


def test_refuses_cumulative_average():
    bn = _train_bn(momentum=None)
    with pytest.raises(NotImplementedError, match='momentum=None'):
        bn.forward3(torch.zeros(2, 4, 6))


def test_refuses_bf16_mode():
    from ld_amd import layers as Y
    bn = _train_bn()
    Y.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16'):
            bn.forward3(torch.zeros(2, 4, 6))
    finally:
        Y.set_precision('fp32')


def test_refuses_training_bn_after_dcn():
    from ld_amd.cnn import build_conv_layer
    from ld_amd.resnet import _conv_bn
    conv = build_conv_layer(dict(type='DCN', deform_groups=1), 16, 16, 3,
                            padding=1, bias=False)
    with pytest.raises(NotImplementedError, match='DeformConv2dPack'):
        _conv_bn(torch.zeros(2, 16, 12), ((3, 4), ), conv, _train_bn(16))


def test_refuses_training_bn_after_dcn_in_a_conv_module():
    from ld_amd.cnn import ConvModule
    m = ConvModule(16, 16, 3, padding=1, conv_cfg=dict(type='DCN'),
                   norm_cfg=dict(type='BN')).train()
    with pytest.raises(NotImplementedError, match='DeformConv2dPack'):
        m.forward3(torch.zeros(2, 16, 12), ((3, 4), ))


def test_sync_bn_stays_refused():
    from ld_amd.cnn import build_norm_layer
    with pytest.raises(NotImplementedError, match='SyncBN'):
        build_norm_layer(dict(type='SyncBN'), 8)


def test_eval_mode_still_refuses_the_host():
    """Eval mode is the existing path: a CPU tensor is refused by the library
    boundary, not by a training-mode message."""
    from ld_amd import lib as L
    from ld_amd.cnn import BatchNorm2d
    with pytest.raises(L.LdError):
        BatchNorm2d(4).eval().forward3(torch.zeros(2, 4, 6))


def test_workspace_and_argument_validation_without_a_device():
    from ld_amd import lib as L
    lib = L.get_lib()
    assert lib.ld_bn_train_workspace_bytes(2, 8, 100) > 0
    assert lib.ld_bn_train_workspace_bytes(1, 8, 1) == 0  # M == 1
    assert lib.ld_bn_train_workspace_bytes(0, 8, 4) == 0
    z = None
    assert lib.ld_bn_train_forward(z, z, z, z, 1e-5, 0.1, 2, 8, 100, 1, 1, z,
                                   z, z, z, z, z, z, z, z, 0, z) == -1
    assert lib.ld_bn_train_backward(z, z, z, z, z, z, 2, 8, 100, 1, z, z, z,
                                    z, 0, z, 0, z) == -1
