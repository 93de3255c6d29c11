"""The fused loss block (ld_amd/csrc/loss.hip) at the edges its parity tests
never reach, against the float64 autograd restatement tests/_loss_ref64.py.

Cases: tests/_loss_edges.py (each with counted claims, see
tests/test_loss_ref64_host.py).  Every case runs through
``lossblock.loss_block_forward`` with loose per-level tensors and with the
packed (N, C, A) arena.

The bar, per case and per output (each of the 8 loss rows, each gradient
family over all levels):

    max|gpu - ref64| <= K_ORACLE * e_oracle + F_SCALE * max|ref64|

where ``e_oracle`` is the float32 numpy oracle's own worst error against
ref64 on that output, computed here.  On top of it every element is held to
what the existing parity tests allow (losses LOSS_RTOL / LOSS_ATOL, gradients
rtol 5e-4 / atol 1e-7), so the bar is nowhere looser than theirs.  Where the
oracle has no such mode (the box losses other than GIoU) ``e_oracle`` is the
GIoU run's on the same inputs: all other terms are the same arithmetic and the
box-loss chains are of the same length.  With a non-unit upstream (entries
<= 2) it is twice the unit run's.

F_SCALE = 2^-22 is 4 ulp of fp32 at the output's scale: what remains when the
oracle's own error happens to be zero on an output.  K_ORACLE = 12 comes from
the measurement below: at most twice the worst ratio measured, because two
correct fp32 evaluations in different summation orders differ by a small
factor (precedent: 3 x the other implementation's error in tests/_gradcheck.py).

MEASURED on the MI355X over the 2 665 outputs the 266 tests of this module
compare.
K needed = (err - F_SCALE * scale) / e_oracle, worst over the cases:
    LDHead 6.16 (student_near_teacher, KD row: both fp32 evaluations form a
    loss of 2e-8 as a difference of O(1) terms; the errors are 4.6e-8 and
    7.4e-9), next 4.26 (the whole-step test, LD row); LDv2Head 3.46
    (box_ties_iou, grad_reg); LDATSSHead 1.09; LDFCOSHead 2.86; LDRetinaHead 2.65;
    non-unit upstream 0.55 (its e_oracle is doubled).
    Worst err / scale outside the cancelling rows: 1.2e-6 (grad_cls,
    two_temperatures), LDRetinaHead 5.6e-6 (KD row at T = 8).
Reg-side outputs (grad_reg, rows 2-4) per variant word, worst err / e_oracle
over the six variant cases, loose and packed:
    default (FAST) 2.58 | exact 2.93 | vec2 4.17 | vec4 2.58 | side_off 2.58 |
    one_xcd 2.58 | waves8 2.58 | small_nt 2.58 | round2 4.17;
    worst err / scale 4.1e-7 for every word.  The FAST forms need no larger k
    than the exact ones (2.58 against 2.93).
The whole module runs in 10 s; its slowest test is
test_step_with_empty_image (1.5 s), the slowest case run 0.5 s.
"""
import types

import numpy as np
import pytest
import torch

import _loss_edges as E
import _loss_ref64 as R

pytestmark = pytest.mark.gpu

LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-4     # tests/test_gpu_lossblock.py
GRAD_RTOL, GRAD_ATOL = 5e-4, 1e-7
K_ORACLE, F_SCALE = E.K_ORACLE, E.F_SCALE
ref64, oracle_error, _outputs = E.ref64, E.oracle_error, E.outputs
# rows that exist only with positives on the level (row 0 sums every cell, row 4
# is the VLR-LD term of cells that are not positives)
POS_ROWS = (1, 2, 3, 5, 6, 7)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _flags(flavour):
    from ld_amd import lib as L
    return dict(ld=0, v2=L.LD_LOSS_PROB_CLS, atss=L.LD_LOSS_ATSS,
                fcos=L.LD_LOSS_ATSS | L.LD_LOSS_FCOS,
                retina=L.LD_LOSS_RETINA)[flavour]


def variant_words():
    """The reg-side words of ld_loss_set_reg_variant (bit layout: the comment
    above LD_REG_VARIANT_DEFAULT in loss.hip)."""
    d = 0 | 4 | 8 | 16 | 32
    return dict(default=d, exact=d & ~16, vec2=d | 1, vec4=d | 2,
                side_off=d & ~32, one_xcd=d | 0x10000, waves8=d | 128,
                small_nt=d | 64, round2=-1)


WORDS = variant_words()


@pytest.fixture
def reg_variant():
    """Set the process-global reg-side word for one test, restore it after."""
    from ld_amd import lib as L
    lib = L.get_lib()
    prev = []

    def set_(word):
        p = lib.ld_loss_set_reg_variant(int(word))
        if not prev:
            prev.append(p)

    yield set_
    if prev:
        lib.ld_loss_set_reg_variant(prev[0])


def make_hp(case, **over):
    from ld_amd import lossblock as LB
    kw = dict(case['hp'])
    kw.update(over)
    if case['flavour'] in E.SIDE:   # the heads' stand-in features: the cls maps
        kw['feat_channels'] = case['maps']['cls'][0].shape[1]
    return LB.make_hp(flags=_flags(case['flavour']), **kw)


_TARGETS = {}


def device_targets(case, dev):
    """The dense targets from the target kernels (bbox_targets rewritten where
    the case says so), checked once against the oracle's arrays ref64 reads."""
    import ld_oracle as O
    from ld_amd import lossblock as LB
    key = (case['name'], case['flavour'])
    if key in _TARGETS:
        return _TARGETS[key]
    fl, sizes, NC = case['flavour'], case['sizes'], \
        case['hp'].get('num_classes', 80)
    gtb = [torch.from_numpy(b).reshape(-1, 4).to(dev) for b in case['boxes']]
    gtl = [torch.from_numpy(l).to(dev) for l in case['labels']]
    if fl == 'fcos':
        t = LB.fcos_targets(sizes, E.STRIDES, gtb, gtl, NC, O.FCOS_RANGES,
                            True, 1.5, dev)
    elif fl == 'retina':
        anchors = torch.from_numpy(
            np.concatenate(O.retina_grid_anchors(sizes))).to(dev)
        t = LB.retina_targets(
            sizes, E.STRIDES, case['metas'], gtb, gtl, [anchors], E.RETINA_B,
            types.SimpleNamespace(pos_iou_thr=0.5, neg_iou_thr=0.4,
                                  min_pos_iou=0.0), NC, dev)
    else:
        t = LB.atss_targets(sizes, E.STRIDES, case['metas'], gtb, gtl,
                            make_hp(case), dev)
    for n, a, box in case['overrides']:
        t['bbox_targets'][n, a] = torch.from_numpy(box).to(dev)
    torch.cuda.synchronize()
    o = case['targets']
    lab = t['labels'].cpu().numpy()
    pos = (lab >= 0) & (lab < NC)
    opos = (o['labels'] >= 0) & (o['labels'] < NC)
    assert np.array_equal(pos, opos)
    assert np.array_equal(lab[pos], o['labels'][opos])
    for k in ('label_weights', 'vlr', 'im'):
        assert np.array_equal(t[k].cpu().numpy(), o[k]), k
    assert np.array_equal(t['bbox_targets'].cpu().numpy()[pos],
                          o['bbox_targets'][opos])
    _TARGETS[key] = t
    return t


def _to_dev(lst, sizes, dev, packed):
    if lst is None:
        return None
    if not packed:
        return [x.to(dev) for x in lst]
    n, c = lst[0].shape[:2]
    arena = torch.empty((n, c, sum(h * w for h, w in sizes)), device=dev)
    views, off = [], 0
    for x, (h, w) in zip(lst, sizes):
        v = arena[:, :, off:off + h * w].view(n, c, h, w)
        v.copy_(x)
        views.append(v)
        off += h * w
    return views


def run_gpu(case, packed=False, upstream=None, **hp_over):
    """-> dict(losses (8, L) float32, grads {family: [per level]}, norm)."""
    from ld_amd import lossblock as LB
    dev = _dev()
    t = device_targets(case, dev)
    d = {k: _to_dev(v, case['sizes'], dev, packed)
         for k, v in case['maps'].items()}
    fl = case['flavour']
    if fl in E.SIDE:
        d['x'] = d['t_x'] = [c.detach() for c in d['cls']]
    if fl == 'v2':
        d['t_cls'] = d['kd_t']
    up = None if upstream is None else \
        torch.as_tensor(upstream, dtype=torch.float32).to(dev)
    losses, grads, norm, _ = LB.loss_block_forward(
        make_hp(case, **hp_over), t, d['cls'], d['reg'], d['t_cls'],
        d['t_reg'], d['x'], d['t_x'], upstream=up, kd_s=d.get('kd_s'),
        kd_t=d.get('kd_t'), ctr=d.get('ctr'))
    torch.cuda.synchronize()
    if fl in E.SIDE:
        grads = dict(grads, x=None)
    return dict(losses=losses.cpu().numpy(), norm=norm.cpu().numpy(),
                grads={k: None if g is None else [a.cpu().numpy() for a in g]
                       for k, g in grads.items()})


def compare(got, ref, e_oracle, tag, e_factor=1.0):
    """The bar of the module docstring on every output; prints each figure
    before it asserts.  -> worst err / bar."""
    g, r = _outputs(got), _outputs(ref)
    assert set(g) == set(r), (sorted(g), sorted(r))
    worst, bad = 0.0, []
    for k in sorted(r):
        assert g[k].shape == r[k].shape and np.isfinite(g[k]).all(), (tag, k)
        err = float(np.abs(g[k] - r[k]).max())
        scale = float(np.abs(r[k]).max())
        eo = e_factor * e_oracle.get(k, 0.0)
        bar = K_ORACLE * eo + F_SCALE * scale
        unit = eo + F_SCALE * scale
        print(f'LOSSEDGE {tag} {k} err {err:.3e} e_oracle {eo:.3e} scale '
              f'{scale:.3e} err/unit {err / unit if unit else 0.0:.3f}')
        if err > bar:
            bad.append((k, err, bar))
        if unit:
            worst = max(worst, err / unit)
        rt, at = (LOSS_RTOL, LOSS_ATOL) if k.startswith('row') else \
            (GRAD_RTOL, GRAD_ATOL)
        np.testing.assert_allclose(g[k], r[k], rtol=rt, atol=at,
                                   err_msg=f'{tag} {k}')
    assert not bad, f'{tag}: (output, max err, bar) {bad}'
    return worst


def exact_checks(case, got, ref):
    """What holds with no tolerance."""
    t, sizes, NC = case['targets'], case['sizes'], \
        case['hp'].get('num_classes', 80)
    B = case['num_base']
    cnt = R.counts(t, sizes, NC, B)
    assert float(got['norm'][0]) == ref['num_total_raw']
    # norm[1]: the sum the avg factor is formed from.  The guard is applied
    # HERE, so this checks norm[1], not the kernels' avg_divisor: with no
    # positive nothing is divided by it, and on the device its three forms at a
    # zero normaliser show only as finite (not NaN) losses and gradients
    fl, n1 = case['flavour'], float(got['norm'][1])
    if not sum(cnt['pos_per_image']):
        assert n1 == 0.0
    avg = max(float(got['norm'][0]), 1.0) if fl == 'retina' else \
        ((1.0 if n1 < 1e-12 else n1) if fl in ('atss', 'fcos') else n1 + 1e-6)
    np.testing.assert_allclose(avg, ref['avg_factor'], rtol=1e-5)
    # gradients of an image without a GT box
    for i, p in enumerate(cnt['pos_per_image']):
        if p:
            continue
        for k in ('reg', 'x', 'kd', 'ctr'):
            for a in got['grads'].get(k) or ():
                assert not a[i * B:(i + 1) * B].any(), (k, i)
    # grad_cls where the label weight is zero
    lw = np.asarray(t['label_weights'])
    for l, sl in enumerate(R.level_slices(sizes)):
        out = (lw[:, sl] == 0).reshape(lw.shape[0], 1, *sizes[l])
        g = got['grads']['cls'][l]
        assert not (g * out).any() and np.isfinite(g).all(), l
        if not cnt['pos_per_level'][l]:
            for r in POS_ROWS:
                assert got['losses'][r, l] == 0.0, (r, l)
    if not sum(cnt['pos_per_image']):
        assert not got['losses'][1:].any() and got['losses'][0].all()


def exact_at_equality(case, got):
    """Student == teacher, bit for bit: the three distillation rows are 0 and
    so is grad_reg wherever only distillation terms reach it."""
    assert not got['losses'][3:6].any()
    lab = case['targets']['labels']
    for l, sl in enumerate(R.level_slices(case['sizes'])):
        neg = ~((lab[:, sl] >= 0) & (lab[:, sl] < 80))
        neg = neg.reshape(lab.shape[0], 1, *case['sizes'][l])
        assert not (got['grads']['reg'][l] * neg).any(), l


PAIR_IDS = [f'{c}-{f}' for c, f in E.PAIRS]


@pytest.mark.parametrize('packed', [False, True], ids=['loose', 'packed'])
@pytest.mark.parametrize('name,flavour', E.PAIRS, ids=PAIR_IDS)
def test_case_vs_ref64(name, flavour, packed):
    case = E.build(name, flavour)
    got = run_gpu(case, packed)
    ref = ref64(name, flavour)
    again = run_gpu(case, packed)
    for k, a in _outputs(got).items():      # run-to-run bit equality
        assert np.array_equal(a, _outputs(again)[k]), k
    exact_checks(case, got, ref)
    compare(got, ref, oracle_error(name, flavour),
            f'{name} {flavour} {"packed" if packed else "loose"} default')
    if name == 'student_is_teacher':
        exact_at_equality(case, got)


def test_129_classes_refused():
    """ceil(129 / 16) = 9 class chunks > kZMax = 8."""
    from ld_amd import lib as L
    case = E.classes('ld', 129)
    case['name'] = 'classes_129'
    case['targets'] = E.oracle_targets(case)
    device_targets(case, _dev())
    with pytest.raises(L.LdError, match='UNSUPPORTED'):
        run_gpu(case)


VARIANT_CASES = ('ragged', 'ten_blocks', 'pos_every_level',
                 'two_temperatures', 'two_temperatures_t1',
                 'student_is_teacher')


@pytest.mark.parametrize('word', list(WORDS), ids=list(WORDS))
@pytest.mark.parametrize('packed', [False, True], ids=['loose', 'packed'])
@pytest.mark.parametrize('name', VARIANT_CASES)
def test_reg_variants_vs_ref64(reg_variant, name, packed, word):
    """Every selectable reg-side kernel form, held to the bar of the default."""
    case = E.build(name, 'ld')
    reg_variant(WORDS[word])
    got = run_gpu(case, packed)
    exact_checks(case, got, ref64(name, 'ld'))
    compare(got, ref64(name, 'ld'), oracle_error(name, 'ld'),
            f'{name} ld {"packed" if packed else "loose"} {word}')
    if name == 'student_is_teacher':
        exact_at_equality(case, got)


def _poisoned_pair(case, monkeypatch):
    """One run on zeroed workspace / gradient memory, one on 0xFF / NaN."""
    from ld_amd import lossblock as LB
    dev = _dev()
    run_gpu(case)                           # the cached workspace exists now
    ws = LB.workspace(dev, 1, 'loss')
    real = LB.alloc_level_views
    outs = []
    for byte, fill in ((0, 0.0), (255, float('nan'))):
        def filled(like, fill=fill):
            views = real(like)
            for v in views:
                v.fill_(fill)
            return views
        monkeypatch.setattr(LB, 'alloc_level_views', filled)
        ws.fill_(byte)
        outs.append(run_gpu(case))
        assert LB.workspace(dev, 1, 'loss').data_ptr() == ws.data_ptr()
    monkeypatch.setattr(LB, 'alloc_level_views', real)
    a, b = (_outputs(o) for o in outs)
    for k in a:
        assert np.isfinite(b[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('flavour', R.FLAVOURS)
@pytest.mark.parametrize('name', ['ten_blocks', 'all_empty'])
def test_poisoned_memory(monkeypatch, name, flavour):
    """Nothing the block reads is left over from an earlier launch: losses and
    gradients are finite and bit-identical on zeroed and on poisoned memory."""
    _poisoned_pair(E.build(name, flavour), monkeypatch)


@pytest.mark.parametrize('word', list(WORDS), ids=list(WORDS))
def test_poisoned_memory_reg_variants(monkeypatch, reg_variant, word):
    reg_variant(WORDS[word])
    _poisoned_pair(E.build('ragged', 'ld'), monkeypatch)


def _upstream(L):
    up = torch.rand((8, L), generator=torch.Generator().manual_seed(77),
                    dtype=torch.float64) * 1.5 + 0.5
    up[3, 0] = 0.0
    up[0, 1] = 0.0
    return up.numpy()


@pytest.mark.parametrize('flavour', R.FLAVOURS)
@pytest.mark.parametrize('name', ['ten_blocks', 'pos_every_level'])
def test_nonunit_upstream(name, flavour):
    """Every gradient family against autograd of sum(upstream * table)."""
    case = E.build(name, flavour)
    up = _upstream(len(case['sizes']))
    ref = R.loss_block(flavour, case['maps'], case['targets'], case['hp'],
                       upstream=up, num_base=case['num_base'])
    got = run_gpu(case, upstream=up)
    # the table itself does not depend on the upstream
    assert np.array_equal(got['losses'], run_gpu(case)['losses'])
    compare(got, ref, oracle_error(name, flavour),
            f'{name} {flavour} loose upstream', e_factor=2.0)


ZERO_ROWS = {0: 'lw_cls', 1: 'lw_bbox', 2: 'lw_dfl', 3: 'lw_ld',
             4: 'lw_ld_vlr', 5: 'lw_kd', 7: 'lw_im'}


@pytest.mark.parametrize('row', sorted(ZERO_ROWS))
def test_zero_upstream_row_is_zero_weight(row):
    """A zero upstream row = that term's loss weight set to 0, bit for bit."""
    case = E.build('ten_blocks', 'ld')
    up = np.ones((8, 5), np.float32)
    up[row] = 0.0
    a = run_gpu(case, upstream=up)
    b = run_gpu(case, **{ZERO_ROWS[row]: 0.0})
    for k in ('cls', 'reg', 'x'):
        for ga, gb in zip(a['grads'][k], b['grads'][k]):
            assert np.array_equal(ga, gb), k


def test_step_with_empty_image(monkeypatch):
    """The smallest whole train step (R50 student <- R101 teacher, 128x160)
    with num_gt [0, 2]: its loss table is the loss block's on the same head
    outputs (and ref64's within the bar), every parameter gradient finite."""
    import ld_oracle as O
    from ld_amd import lossblock as LB
    from ld_amd import model_zoo, synthetic
    dev = _dev()
    det = model_zoo.build_seeded_ld_detector(50, 101, dev, loss_im_weight=2.0)
    b = synthetic.synthetic_batch(2, (128, 150), (128, 160), [0, 2], 21)
    seen = []
    real = LB.loss_block_forward

    def cpu(ts):
        return [t.detach().cpu() for t in ts]

    def spy(hp, targets, *a, **kw):
        out = real(hp, targets, *a, **kw)
        again = real(hp, targets, *a, **kw)
        seen.append(dict(
            hp={k: getattr(hp, k) for k in R.HP_DEFAULT if hasattr(hp, k)},
            targets={k: targets[k].cpu().numpy() for k in (
                'labels', 'label_weights', 'bbox_targets', 'vlr', 'im')},
            maps=dict(zip(('cls', 'reg', 't_cls', 't_reg', 'x', 't_x'),
                          (cpu(t) for t in a[:6]))),
            losses=out[0].clone(), again=again[0].clone(),
            grads={k: [g.cpu().numpy() for g in out[1][k]]
                   for k in ('cls', 'reg', 'x')}))
        return out

    monkeypatch.setattr(LB, 'loss_block_forward', spy)
    losses = det(img=b['img'].to(dev), img_metas=b['img_metas'],
                 gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                 gt_labels=[x.to(dev) for x in b['gt_labels']])
    monkeypatch.setattr(LB, 'loss_block_forward', real)
    table = torch.stack([torch.stack(v) for v in losses.values()])
    loss, _ = det._parse_losses(losses)
    loss.backward()
    torch.cuda.synchronize()
    assert len(seen) == 1
    s = seen[0]
    assert torch.equal(table.detach(), s['losses'])
    assert torch.equal(s['again'], s['losses'])
    for k, p in det.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    sizes = [tuple(c.shape[2:]) for c in s['maps']['cls']]
    assert R.counts(s['targets'], sizes)['pos_per_image'][0] == 0
    ref = R.loss_block('ld', s['maps'], s['targets'], s['hp'])
    got = dict(losses=s['losses'].cpu().numpy(),
               grads=dict(s['grads'], kd=None, ctr=None))
    # the oracle on the same inputs (its IM region: the gibox cells the step
    # selected on the device)
    raw = O.get_targets(sizes, b['img_metas'],
                        [x.numpy() for x in b['gt_bboxes']],
                        [x.numpy() for x in b['gt_labels']])
    raw['im'] = s['targets']['im']
    orc = E.oracle_block(dict(flavour='ld', hp=s['hp'], maps=s['maps'],
                              sizes=sizes), dict(raw=raw))
    e_o = {k: float(np.abs(v - _outputs(ref)[k]).max())
           for k, v in _outputs(orc).items()}
    compare(got, ref, e_o, 'step_empty_image ld')
