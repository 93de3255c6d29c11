"""CPU checks of the config's optimizer recipe: the StepLrUpdaterHook restatement
(ld_amd.schedule), DefaultOptimizerConstructor's paramwise rules on the LD-FCOS
student (ld_amd.optim) and the per-parameter optimizer state in torch.optim.SGD's
format.  No device needed."""
import math

import pytest
import torch

LD_COCO = dict(policy='step', warmup='linear', warmup_iters=500,
               warmup_ratio=0.001, step=[8, 11])


def _sched(**kw):
    from ld_amd.schedule import build_lr_schedule
    return build_lr_schedule(kw)


def _lr(s, base, epoch, it):
    """The lr one group trains with at (epoch, iter), the hook's call order."""
    s.before_run([base])
    s.before_train_epoch(epoch, it)
    out = s.before_train_iter(epoch, it)
    return (out if out is not None else s.regular_lr)[0]


@pytest.mark.parametrize('epoch,it,want', [
    (0, 0, 2.5e-6), (0, 250, 0.00125125), (0, 499, 0.002495005),
    (0, 500, 0.0025), (8, 5000, 2.5e-4), (11, 9000, 2.5e-5)])
def test_ld_coco_recipe_table(epoch, it, want):
    s = _sched(**LD_COCO)
    assert math.isclose(_lr(s, 0.0025, epoch, it), want, rel_tol=1e-12)
    assert math.isclose(s.lr_at(0.0025, epoch, it), want, rel_tol=1e-12)


def test_fcos_recipe_warmup_ratio_third():
    s = _sched(policy='step', warmup='linear', warmup_iters=500,
               warmup_ratio=1.0 / 3, step=[8, 11])
    assert math.isclose(_lr(s, 0.01, 0, 0), 0.01 / 3, rel_tol=1e-12)
    assert math.isclose(_lr(s, 0.01, 0, 250), 0.01 * 2 / 3, rel_tol=1e-12)
    assert math.isclose(_lr(s, 0.01, 0, 500), 0.01, rel_tol=1e-15)
    assert math.isclose(_lr(s, 0.01, 9, 6000), 0.001, rel_tol=1e-12)


def test_voc_recipe_single_milestone():
    s = _sched(policy='step', warmup='linear', warmup_iters=500,
               warmup_ratio=0.001, step=[3])
    assert _lr(s, 0.00375, 2, 3000) == 0.00375
    assert math.isclose(_lr(s, 0.00375, 3, 4000), 0.000375, rel_tol=1e-12)
    # an int step: every 3 epochs
    s = _sched(policy='step', step=3)
    assert math.isclose(_lr(s, 0.1, 7, 0), 0.001, rel_tol=1e-12)


def test_constant_and_exp_warmup():
    s = _sched(policy='step', warmup='constant', warmup_iters=10,
               warmup_ratio=0.25, step=[8])
    assert _lr(s, 0.02, 0, 0) == 0.02 * 0.25
    assert _lr(s, 0.02, 0, 9) == 0.02 * 0.25
    assert _lr(s, 0.02, 0, 10) == 0.02
    s = _sched(policy='step', warmup='exp', warmup_iters=10, warmup_ratio=0.01,
               step=[8])
    assert math.isclose(_lr(s, 0.02, 0, 0), 0.02 * 0.01, rel_tol=1e-12)
    assert math.isclose(_lr(s, 0.02, 0, 5), 0.02 * 0.01**0.5, rel_tol=1e-12)


def test_min_lr_clamps_the_regular_lr():
    s = _sched(policy='step', step=[1, 2, 3], min_lr=1e-4)
    assert math.isclose(_lr(s, 0.01, 1, 0), 0.001, rel_tol=1e-12)
    assert math.isclose(_lr(s, 0.01, 2, 0), 1e-4, rel_tol=1e-12)  # by gamma
    assert _lr(s, 0.01, 3, 0) == 1e-4       # 1e-5 -> min_lr exactly


def test_by_iter_schedule():
    s = _sched(policy='step', by_epoch=False, step=[100, 200], warmup='linear',
               warmup_iters=10, warmup_ratio=0.5)
    s.before_run([0.1])
    assert s.before_train_epoch(0) is None  # by_epoch=False: nothing per epoch
    assert math.isclose(s.before_train_iter(0, 0)[0], 0.05, rel_tol=1e-12)
    assert s.before_train_iter(0, 10) == [0.1]
    assert math.isclose(s.before_train_iter(0, 150)[0], 0.01, rel_tol=1e-12)
    assert math.isclose(s.before_train_iter(3, 250)[0], 0.001, rel_tol=1e-12)


def test_warmup_boundary_branches():
    s = _sched(**LD_COCO)
    s.before_run([0.0025, 0.005])
    assert s.before_train_epoch(0) == [0.0025, 0.005]
    w = s.before_train_iter(0, 499)
    assert math.isclose(w[1], 2 * 0.002495005, rel_tol=1e-12)
    assert s.before_train_iter(0, 500) == [0.0025, 0.005]   # it == warmup_iters
    assert s.before_train_iter(0, 501) is None               # nothing after it
    assert s.before_train_epoch(8) == pytest.approx([2.5e-4, 5e-4], rel=1e-12)
    assert s.before_train_iter(8, 8000) is None


def test_schedule_refusals():
    from ld_amd.schedule import build_lr_schedule
    with pytest.raises(NotImplementedError, match='CosineAnnealing'):
        build_lr_schedule(dict(policy='CosineAnnealing', min_lr=0))
    with pytest.raises(NotImplementedError, match='warmup_by_epoch'):
        build_lr_schedule(dict(policy='step', step=[8], warmup_by_epoch=True))
    with pytest.raises(ValueError):
        build_lr_schedule(dict(policy='step', step=[8], warmup='cosine',
                               warmup_iters=5))
    assert build_lr_schedule(None) is None


# ------------------------------------------------------------- paramwise --
@pytest.fixture(scope='module')
def fcos_student():
    from ld_amd import model_zoo
    from ld_amd.registry import build_detector
    return build_detector(model_zoo.ld_fcos_detector(18, 18))


FCOS_OPT = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0001,
                paramwise_cfg=dict(bias_lr_mult=2.0, bias_decay_mult=0.0))


def test_fcos_paramwise_classes(fcos_student):
    from ld_amd import cnn
    from ld_amd.optim import build_optimizer
    det = fcos_student
    opt = build_optimizer(det, FCOS_OPT, dict(grad_clip=None))
    pc = opt['param_classes']
    assert opt['grad_clip'] is None and opt['lr'] == 0.01
    allp = list(det.parameters())
    assert len(pc.mults) == len(allp) and [id(p) for p in pc.params] == \
        [id(p) for p in allp]
    assert sum(not p.requires_grad for p in allp) > 0  # frozen stem / BN
    owner = {}
    for mname, m in det.named_modules():
        for pname, p in m.named_parameters(recurse=False):
            owner.setdefault(id(p), (m, pname))
    kinds = set()
    for p, m_ in zip(allp, pc.mults):
        mod, pname = owner[id(p)]
        if not p.requires_grad:
            assert m_ == (1.0, 1.0)
        elif isinstance(mod, (cnn.BatchNorm2d, cnn.GroupNorm)):
            assert m_ == (1.0, 1.0)
            kinds.add('norm')
        elif pname == 'bias':
            assert m_ == (2.0, 0.0), type(mod)
            kinds.add('bias')
        else:
            assert pname in ('weight', 'scale') and m_ == (1.0, 1.0)
            kinds.add(pname)
    assert kinds == {'norm', 'bias', 'weight', 'scale'}
    assert pc.classes == [(1.0, 1.0), (2.0, 0.0)]


def test_custom_keys_precedence(fcos_student):
    from ld_amd.optim import classify
    names, mults = classify(fcos_student, dict(
        bias_lr_mult=2.0, bias_decay_mult=0.0,
        custom_keys={'bbox_head': dict(lr_mult=0.5),
                     'bbox_head.conv_cls': dict(lr_mult=3.0, decay_mult=0.2)}))
    m = dict(zip(names, mults))
    # longest key first: beats 'bbox_head' and the bias rule
    assert m['bbox_head.conv_cls.bias'] == (3.0, 0.2)
    assert m['bbox_head.conv_cls.weight'] == (3.0, 0.2)
    # a custom key sets decay_mult too (default 1), the bias rule is skipped
    assert m['bbox_head.conv_reg.bias'] == (0.5, 1.0)
    assert m['bbox_head.scales.0.scale'] == (0.5, 1.0)
    # no key matches: the bias rule
    assert m['neck.lateral_convs.0.conv.bias'] == (2.0, 0.0)
    # equal length: alphabetical order decides ('cls' before 'onv')
    names, mults = classify(fcos_student, dict(custom_keys={
        'onv': dict(lr_mult=7.0), 'cls': dict(lr_mult=5.0)}))
    m = dict(zip(names, mults))
    assert m['bbox_head.conv_cls.bias'] == (5.0, 1.0)
    assert m['bbox_head.conv_reg.bias'] == (7.0, 1.0)


def test_refusals(fcos_student):
    from ld_amd.optim import build_optimizer
    det = fcos_student
    with pytest.raises(NotImplementedError, match='Adam'):
        build_optimizer(det, dict(type='Adam', lr=1e-3))
    with pytest.raises(NotImplementedError, match='nesterov'):
        build_optimizer(det, dict(type='SGD', lr=0.01, nesterov=True))
    with pytest.raises(NotImplementedError, match='dampening'):
        build_optimizer(det, dict(type='SGD', lr=0.01, dampening=0.1))
    with pytest.raises(NotImplementedError, match='dcn_offset_lr_mult'):
        build_optimizer(det, dict(type='SGD', lr=0.01, paramwise_cfg=dict(
            dcn_offset_lr_mult=0.1)))
    with pytest.raises(NotImplementedError, match='norm_type'):
        build_optimizer(det, dict(type='SGD', lr=0.01),
                        dict(grad_clip=dict(max_norm=35, norm_type=1)))
    clip = build_optimizer(det, dict(type='SGD', lr=0.01),
                           dict(grad_clip=dict(max_norm=35, norm_type=2)))
    assert clip['grad_clip'] == dict(max_norm=35.0, norm_type=2)
    assert clip['param_classes'] is None


def test_chunk_ids_follow_the_arena(fcos_student):
    import copy
    from ld_amd.optim import build_optimizer
    from ld_amd.train import GradArena
    det = copy.deepcopy(fcos_student)
    pc = build_optimizer(det, FCOS_OPT)['param_classes']
    arena = GradArena(list(det.parameters()))
    ids = pc.chunk_ids(arena)
    assert ids.dtype == torch.uint8 and ids.numel() == arena.numel // 64
    cls_of = {id(p): c for p, c in zip(pc.params, pc.class_of)}
    for p, o in zip(arena.order, arena.offsets):
        assert int(ids[o // 64]) == cls_of[id(p)]
        assert int(ids[(o + p.numel() - 1) // 64]) == cls_of[id(p)]


# ------------------------------------------------- optimizer state (CPU) --
def _fcos_trainer(det, with_schedule=True):
    from ld_amd.train import SGDTrainer
    cfg = dict(optimizer=FCOS_OPT, optimizer_config=dict(grad_clip=None),
               lr_config=dict(LD_COCO) if with_schedule else None)
    return SGDTrainer.from_config(det, cfg)


def test_paramwise_state_dict_round_trips_through_torch_sgd(fcos_student):
    import copy
    from ld_amd.train import SGDTrainer
    det = copy.deepcopy(fcos_student)
    tr = _fcos_trainer(det)
    sd = tr.state_dict()
    allp = list(det.parameters())
    assert len(sd['param_groups']) == len(allp)
    pc = tr.param_classes
    for i, (g, (lm, dm)) in enumerate(zip(sd['param_groups'], pc.mults)):
        assert g['params'] == [i]
        assert g['initial_lr'] == 0.01 * lm
        assert g['weight_decay'] == 0.0001 * dm
    # torch.optim.SGD with mmcv's per-parameter groups loads it and gives it back
    opt = torch.optim.SGD([dict(params=[p]) for p in allp], lr=0.01,
                          momentum=0.9, weight_decay=0.0001)
    opt.load_state_dict(sd)
    assert [g['weight_decay'] for g in opt.param_groups] == \
        [g['weight_decay'] for g in sd['param_groups']]
    tr2 = _fcos_trainer(copy.deepcopy(fcos_student))
    tr2.load_state_dict(opt.state_dict())
    assert tr2.base_lr == 0.01 and tr2.weight_decay == 0.0001
    # a group that contradicts the classification: named in the error
    bad = opt.state_dict()
    k = pc.class_of.index(1)
    bad['param_groups'][k]['weight_decay'] = 0.0001
    with pytest.raises(ValueError, match=pc.names[k].replace('.', r'\.')):
        tr2.load_state_dict(bad)
    # one form into a trainer built for the other
    plain = SGDTrainer(copy.deepcopy(fcos_student), lr=0.01)
    with pytest.raises(ValueError):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError):
        tr2.load_state_dict(plain.state_dict())


def test_single_group_form_unchanged_without_the_features(fcos_student):
    import copy
    from ld_amd.train import SGDTrainer
    tr = SGDTrainer(copy.deepcopy(fcos_student), lr=0.01)
    g, = tr.state_dict()['param_groups']
    assert list(g) == ['lr', 'momentum', 'dampening', 'weight_decay',
                       'nesterov', 'params']
    from ld_amd.schedule import build_lr_schedule
    tr = SGDTrainer(copy.deepcopy(fcos_student), lr=0.01,
                    lr_schedule=build_lr_schedule(LD_COCO))
    g, = tr.state_dict()['param_groups']
    assert g['initial_lr'] == 0.01


def test_norm_and_depthwise_decay_rules():
    from collections import OrderedDict
    import torch.nn as nn
    from ld_amd import cnn
    from ld_amd.optim import classify
    model = nn.Sequential(OrderedDict(
        conv=cnn.Conv2d(3, 8, 3), gn=cnn.GroupNorm(4, 8),
        dw=nn.Conv2d(8, 8, 3, groups=8), bn=nn.BatchNorm2d(8)))
    names, mults = classify(model, dict(norm_decay_mult=0.0,
                                        dwconv_decay_mult=0.5,
                                        bias_lr_mult=2.0, bias_decay_mult=0.1))
    assert dict(zip(names, mults)) == {
        'conv.weight': (1.0, 1.0), 'conv.bias': (2.0, 0.1),
        'gn.weight': (1.0, 0.0), 'gn.bias': (1.0, 0.0),   # norm: no bias lr
        'dw.weight': (1.0, 0.5), 'dw.bias': (2.0, 0.5),   # dw before bias decay
        'bn.weight': (1.0, 0.0), 'bn.bias': (1.0, 0.0)}


def test_deformable_conv_refused_only_when_trainable():
    from collections import OrderedDict
    import torch.nn as nn
    from ld_amd import cnn
    from ld_amd.optim import classify
    model = nn.Sequential(OrderedDict(conv=cnn.Conv2d(8, 8, 3),
                                      dcn=cnn.DeformConv2dPack(8, 8, 3, padding=1)))
    with pytest.raises(NotImplementedError, match='dcn'):
        classify(model, dict(bias_lr_mult=2.0))
    model.dcn.requires_grad_(False)  # a frozen DCN (the config-4 teacher's)
    names, mults = classify(model, dict(bias_lr_mult=2.0))
    m = dict(zip(names, mults))
    assert m['conv.bias'] == (2.0, 1.0)
    assert all(v == (1.0, 1.0) for k, v in m.items() if k.startswith('dcn.'))


def test_from_config_refuses_momentum_config_and_fp16(fcos_student):
    import copy
    from ld_amd.train import SGDTrainer
    base = dict(optimizer=FCOS_OPT, optimizer_config=dict(grad_clip=None),
                lr_config=dict(LD_COCO))
    for key, val in (('momentum_config', dict(policy='cyclic')),
                     ('fp16', dict(loss_scale=512.0))):
        with pytest.raises(NotImplementedError, match=key):
            SGDTrainer.from_config(fcos_student, dict(base, **{key: val}))
    tr = SGDTrainer.from_config(copy.deepcopy(fcos_student),
                                dict(base, momentum_config=None, fp16=None))
    assert tr.lr_schedule is not None


# ------------------------------------------------------------ EpochRunner --
class _FakeTrainer:
    """What EpochRunner touches of a trainer / stepper, without a device."""

    def __init__(self, pulled, mode=None):
        self.epoch, self.iter, self.lr = 0, 0, 0.1
        self.begun, self.calls, self.pulled = [], [], pulled
        if mode is not None:
            self.mode, self.trainer = mode, self

    def begin_epoch(self, epoch):
        self.epoch = epoch
        self.begun.append((epoch, self.iter))

    def step(self, data, next_data=None):
        # the current batch and at most one more have been pulled
        assert len(self.pulled) <= len(self.calls) + 2
        self.calls.append((self.epoch, data, next_data))
        self.iter += 1
        return dict(loss=0.0, log_vars={'loss': float(self.iter)})


def _gen_batches(pulled, sizes):
    def make(epoch):
        for k in range(sizes[epoch]):
            item = (epoch, k)
            pulled.append(item)
            yield item
    return make


@pytest.mark.parametrize('mode', [None, 'pipelined'])
def test_epoch_runner_consumes_generators_one_ahead(tmp_path, mode):
    from ld_amd.runner import EpochRunner
    pulled = []
    tr = _FakeTrainer(pulled, mode)
    cfg = dict(runner=dict(max_epochs=4), log_config=dict(interval=2),
               checkpoint_config=dict(interval=1))
    r = EpochRunner(tr, cfg, tmp_path)
    saves = []
    r.save = lambda k: saves.append((k, tr.iter))
    sizes = [3, 0, 2, 1]  # an empty epoch still begins and checkpoints
    recs = r.run(_gen_batches(pulled, sizes))
    seq = [(e, k) for e in range(4) for k in range(sizes[e])]
    assert [c[1] for c in tr.calls] == seq
    assert [c[0] for c in tr.calls] == [e for e, _ in seq]
    # next_data is the following batch, across epoch boundaries; at the very
    # end the pipelined step gets its own batch, the others nothing
    assert [c[2] for c in tr.calls] == seq[1:] + \
        ([seq[-1]] if mode == 'pipelined' else [None])
    assert tr.begun == [(0, 0), (1, 3), (2, 3), (3, 5)]
    assert saves == [(1, 3), (2, 3), (3, 5), (4, 6)]
    assert [(x['epoch'], x['iter']) for x in recs] == [(1, 2), (3, 2)]
    assert tr.epoch == 4
