"""CPU: tests/_loss_ref64.py (the loss block in float64, gradients by
autograd) and tests/_loss_edges.py (the edge cases) are what they claim to be.

  * _loss_ref64 equals the REFERENCE's stored losses and gradients on the
    cases of tests/golden/lossblock*.npz, for every flavour and for LDHead in
    every stored box-loss mode, within the tolerances the existing parity
    tests use against those fixtures (LOSS_RTOL / LOSS_ATOL; rtol 5e-4, atol
    1e-7), and the reference's outputs on the edge geometries themselves
    (tests/golden/loss_edges.npz, oracle/gen_golden.py --only loss_edges);
  * every case's claims are recounted with oracle/ld_oracle.py and numpy;
  * every wrong-rule switch of _loss_ref64 moves an output of the case aimed
    at it by more than the bar of tests/test_gpu_loss_edges.py;
  * the float32 numpy oracle agrees with _loss_ref64 on every case."""
import numpy as np
import pytest
import torch

import _iou_losses as IL
import _loss_edges as E
import _loss_ref64 as R
import ld_oracle as O
from ld_amd import synthetic

LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-4     # tests/test_gpu_lossblock.py
GRAD_RTOL, GRAD_ATOL = 5e-4, 1e-7
ROWS = dict(ld=list(range(8)), v2=list(range(8)), atss=[0, 1, 3, 4, 5, 6],
            fcos=[0, 1, 3, 4, 5, 6], retina=[0, 1, 3, 4, 5])
GOLDEN = dict(ld='lossblock', atss='lossblock_atss', fcos='lossblock_fcos',
              retina='lossblock_retina')


# --------------------------------------------- the stored reference outputs ---
def _golden_case(g, name, flavour):
    cfg = g[name + '_cfg']
    pad, shape = tuple(int(v) for v in cfg[:2]), tuple(int(v) for v in cfg[2:4])
    num_gt = [int(x) for x in g[name + '_num_gt']]
    b = synthetic.synthetic_batch(len(num_gt), shape, pad, num_gt, int(cfg[4]))
    sizes = synthetic.level_shapes(pad)
    c = dict(flavour=flavour, sizes=sizes, metas=b['img_metas'],
             boxes=[x.numpy() for x in b['gt_bboxes']],
             labels=[x.numpy() for x in b['gt_labels']], hp=dict(E.HP[flavour]),
             overrides=[], num_base=E.RETINA_B if flavour == 'retina' else 1,
             maps=E.head_inputs(flavour, len(num_gt), sizes, int(cfg[5])))
    c['targets'] = E.oracle_targets(c)
    return c


def _check_grads(g, name, flavour, grads, families):
    for k in families:
        gs = grads[k]
        if flavour == 'retina':   # back to the head's (N, 9 * C, H, W) maps
            gs = [a.reshape(a.shape[0] // E.RETINA_B, -1, *a.shape[2:])
                  for a in gs]
        for l, a in enumerate(gs):
            np.testing.assert_allclose(
                np.abs(a).sum(), g[f'{name}_g{k}_abs_sum'][l], rtol=2e-4,
                atol=1e-7, err_msg=f'{k}[{l}]')
            if f'{name}_g{k}_{l}' in g.files:
                got, want = a, g[f'{name}_g{k}_{l}']
            else:
                want = g[f'{name}_g{k}_{l}_sample']
                flat = a.reshape(-1)
                step = 11 if want.size == len(range(0, flat.size, 11)) \
                    else 1009
                got = flat[::step]
            np.testing.assert_allclose(got, want.reshape(got.shape),
                                       rtol=GRAD_RTOL, atol=GRAD_ATOL,
                                       err_msg=f'{k}[{l}]')


@pytest.mark.parametrize('name', ['small', 'small_crowd'])
@pytest.mark.parametrize('flavour', ['ld', 'atss', 'fcos', 'retina'])
def test_ref64_vs_reference_golden(golden, flavour, name):
    g = golden[GOLDEN[flavour]]
    c = _golden_case(g, name, flavour)
    r = R.loss_block(flavour, c['maps'], c['targets'], c['hp'],
                     num_base=c['num_base'])
    np.testing.assert_allclose(r['losses'][ROWS[flavour]], g[name + '_losses'],
                               rtol=LOSS_RTOL, atol=LOSS_ATOL)
    rest = [i for i in range(8) if i not in ROWS[flavour]]
    assert not r['losses'][rest].any()
    fam = dict(ld=('cls', 'reg', 'x'), atss=('cls', 'reg', 'ctr'),
               fcos=('cls', 'reg', 'ctr'), retina=('cls', 'reg'))[flavour]
    _check_grads(g, name, flavour, r['grads'], fam)


@pytest.mark.parametrize('name', ['small', 'small_crowd'])
@pytest.mark.parametrize('mode', ['iou', 'diou', 'ciou'])
def test_ref64_box_losses_vs_reference_golden(golden, mode, name):
    """LDHead with the other box losses (tests/golden/iou_losses.npz stores the
    reg gradient where it differs from the GIoU run's)."""
    base, g = golden['lossblock'], golden['iou_losses']
    c = _golden_case(base, name, 'ld')
    c['hp']['bbox_loss'] = mode
    r = R.loss_block('ld', c['maps'], c['targets'], c['hp'])
    key = f'lb_{name}_{mode}'
    np.testing.assert_allclose(r['losses'], g[key + '_losses'],
                               rtol=LOSS_RTOL, atol=LOSS_ATOL)
    for k in ('cls', 'reg', 'x'):
        for l, a in enumerate(r['grads'][k]):
            want = base[f'{name}_g{k}_{l}'].copy()
            if k == 'reg':
                want.reshape(-1)[g[f'{key}_greg_{l}_idx']] = \
                    g[f'{key}_greg_{l}_val']
            np.testing.assert_allclose(a, want, rtol=GRAD_RTOL, atol=GRAD_ATOL,
                                       err_msg=f'{k}[{l}]')


@pytest.mark.parametrize('name', ['v2_small', 'v2_small_crowd'])
def test_ref64_v2_vs_reference_golden(golden, name):
    """LDv2Head.loss: the quality branch in torch (net_oracle.quality_tail),
    the loss block by _loss_ref64, gradients chained through the tail as
    net_oracle.ldv2_loss_step chains the numpy oracle's."""
    import net_oracle as NO
    g = golden['lossblock_v2']
    cfg = [int(v) for v in g[name + '_cfg']]
    num_gt = [int(v) for v in g[name + '_num_gt']]
    b = synthetic.synthetic_batch(len(num_gt), tuple(cfg[2:4]), tuple(cfg[:2]),
                                  num_gt, cfg[4])
    sizes = synthetic.level_shapes(tuple(cfg[:2]))
    hi = synthetic.synthetic_head_inputs(len(num_gt), sizes, seed=cfg[5],
                                         num_classes=81)
    shapes = {'reg_conf.0.weight': (64, 20, 1, 1), 'reg_conf.0.bias': (64, ),
              'reg_conf.2.weight': (1, 64, 1, 1), 'reg_conf.2.bias': (1, )}
    sd = synthetic.seeded_state_dict(
        {k: torch.zeros(v) for k, v in shapes.items()}, seed=5)
    cf = [t.clone().requires_grad_(True) for t in hi['cls']]
    rg = [t.clone().requires_grad_(True) for t in hi['reg']]
    scores = [NO.quality_tail(sd, c, r, '')[0] for c, r in zip(cf, rg)]
    c = dict(flavour='v2', sizes=sizes, metas=b['img_metas'],
             boxes=[x.numpy() for x in b['gt_bboxes']],
             labels=[x.numpy() for x in b['gt_labels']], hp=dict(E.HP['v2']))
    t = E.oracle_targets(c)
    r = R.loss_block('v2', dict(
        cls=[s.detach() for s in scores], reg=hi['reg'], t_cls=hi['t_cls'],
        t_reg=hi['t_reg'], x=hi['x'], t_x=hi['t_x'], kd_s=hi['cls'],
        kd_t=hi['t_cls']), t, c['hp'])
    np.testing.assert_allclose(r['losses'], g[name + '_losses'],
                               rtol=LOSS_RTOL, atol=LOSS_ATOL)
    torch.autograd.backward(
        scores, [torch.from_numpy(a).float() for a in r['grads']['cls']])
    got = dict(cls=[c_.grad.double().numpy() + a
                    for c_, a in zip(cf, r['grads']['kd'])],
               reg=[r_.grad.double().numpy() + a
                    for r_, a in zip(rg, r['grads']['reg'])],
               x=r['grads']['x'])
    _check_grads(g, name, 'v2', got, ('cls', 'reg', 'x'))


@pytest.mark.parametrize('mode', IL.LOSSES)
def test_box_loss_rows_vs_reference_rows(golden, mode):
    """_loss_ref64.box_loss_rows and its autograd gradient on the 257 stored
    rows of tests/golden/iou_losses.npz (tests/_iou_losses.py: hand-written
    edge rows, then seeded ones) against the reference's own float64 values:
    the one place iou_linear meets a reference output."""
    g = golden['iou_losses']
    pred, target = IL.row_inputs(g)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    loss = R.box_loss_rows(mode, p, torch.from_numpy(target).double(), 1e-6)
    loss.sum().backward()
    np.testing.assert_allclose(loss.detach().numpy(), g[f'{mode}_loss64'],
                               rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(p.grad.numpy(), g[f'{mode}_grad64'],
                               rtol=1e-8, atol=1e-12)


# ------------------------------------------- the reference on the edge cases ---
EDGE_REF = [('ragged', 'ld'), ('ten_blocks', 'ld'), ('pos_every_level', 'ld'),
            ('two_temperatures', 'ld'), ('two_temperatures_t1', 'ld'),
            ('pos_every_level', 'atss'), ('pos_every_level', 'fcos'),
            ('pos_every_level', 'retina'), ('ragged', 'atss'),
            ('ragged', 'fcos'), ('ragged', 'retina'),
            ('empty_beside_full', 'fcos', 'full'), ('all_empty', 'fcos', 'full')]


@pytest.mark.parametrize('case', EDGE_REF, ids=['-'.join(c) for c in EDGE_REF])
def test_ref64_vs_reference_on_edge_geometries(golden, case):
    """tests/golden/loss_edges.npz: the reference's own ``loss`` on the edge
    cases it is defined for (the images without a GT box removed; LDFCOSHead,
    which is defined on them, also whole): loss tables, per-level gradient
    sums and abs-sums, every 101st element."""
    g = golden['loss_edges']
    name, flavour, full = case[0], case[1], len(case) == 3
    c = E.build(name, flavour) if full else \
        E.without_empty(E.build(name, flavour))
    r = R.loss_block(flavour, c['maps'], c['targets'], c['hp'],
                     num_base=c['num_base'])
    key = f'{name}_{flavour}' + ('_full' if full else '')
    np.testing.assert_allclose(r['losses'][ROWS[flavour]], g[key + '_losses'],
                               rtol=LOSS_RTOL, atol=LOSS_ATOL)
    for k, gs in r['grads'].items():
        if gs is None or f'{key}_g{k}_sum' not in g.files:
            continue
        if flavour == 'retina':
            gs = [a.reshape(a.shape[0] // E.RETINA_B, -1, *a.shape[2:])
                  for a in gs]
        for l, a in enumerate(gs):
            scale = float(g[f'{key}_g{k}_abs_sum'][l])
            np.testing.assert_allclose(np.abs(a).sum(), scale, rtol=2e-4,
                                       atol=1e-7)
            np.testing.assert_allclose(a.sum(), g[f'{key}_g{k}_sum'][l],
                                       rtol=0, atol=2e-4 * scale + 1e-7)
            np.testing.assert_allclose(
                a.reshape(-1)[::101], g[f'{key}_g{k}_{l}_every101'],
                rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=f'{k}[{l}]')


# ------------------------------------------------------------------ claims ---
@pytest.mark.parametrize('name,flavour', E.PAIRS,
                         ids=[f'{c}-{f}' for c, f in E.PAIRS])
def test_claims(name, flavour):
    """Every claim recounted from the oracle's targets and the inputs."""
    c = E.build(name, flavour)
    t, sizes, cl = c['targets'], c['sizes'], c['claims']
    NC = c['hp'].get('num_classes', 80)
    cnt = R.counts(t, sizes, NC, c['num_base'])
    assert sum(len(b) == 0 for b in c['boxes']) == cl['empty_images']
    for i, b in enumerate(c['boxes']):       # an empty image: the definition
        if len(b) == 0:
            rows = slice(i * c['num_base'], (i + 1) * c['num_base'])
            assert cnt['pos_per_image'][i] == 0
            assert not t['vlr'][rows].any() and not t['im'][rows].any()
    assert cnt == cl['counts']      # positives, VLR and IM cells, exactly
    seen = {'counts'}
    if 'level_cells' in cl:
        assert [h * w for h, w in sizes] == cl['level_cells']
        seen.add('level_cells')
    if 'total_pos' in cl:
        assert sum(cnt['pos_per_image']) == cl['total_pos']
        seen.add('total_pos')
    if 'lw_zero_min' in cl:
        lw = t['label_weights']
        full = [i for i, b in enumerate(c['boxes']) if len(b)]
        assert all((lw[i * c['num_base']] == 0).sum() >= cl['lw_zero_min']
                   for i in full)
        seen.add('lw_zero_min')
    if 'blocks_per_image' in cl:
        assert sum(-(-h * w // 256) for h, w in sizes) == \
            cl['blocks_per_image']
        # the one-XCD block order needs gridDim.x = 4 * blocks >= 32 and a tail
        assert 4 * cl['blocks_per_image'] >= 32 and \
            (4 * cl['blocks_per_image']) % 32
        seen.add('blocks_per_image')
    if 'im_without_pos_levels' in cl:
        got = [l for l in range(len(sizes)) if cnt['im_per_level'][l] and
               not cnt['pos_per_level'][l]]
        assert got == cl['im_without_pos_levels']
        seen.add('im_without_pos_levels')
    if 'levels_with_pos' in cl:
        assert sum(p > 0 for p in cnt['pos_per_level']) == \
            cl['levels_with_pos']
        seen.add('levels_with_pos')
    if 'temperatures_differ' in cl:
        assert sum(cnt['vlr_per_level']) and sum(cnt['pos_per_level'])
        assert (c['hp']['T_ld'] != c['hp']['T_ld_vlr']) == \
            cl['temperatures_differ']
        assert 1.0 in (c['hp']['T_ld'], c['hp']['T_kd'])   # T = 1 is run
        seen.add('temperatures_differ')
    if 'max_abs_logit' in cl:
        m = c['maps']
        assert max(float(v.abs().max()) for v in m['reg']) == \
            cl['max_abs_logit']
        sat = m['kd_s' if flavour == 'v2' else 'cls']
        assert {float(v) for t_ in sat for v in t_.unique()} == \
            {-100.0, -30.0, 30.0, 100.0}
        seen.add('max_abs_logit')
    if 'equal' in cl:
        m = c['maps']
        same = all(torch.equal(a, b)
                   for s, t_ in E.EQUAL_MAPS[flavour == 'v2']
                   for a, b in zip(m[s], m[t_]))
        assert same == cl['equal']
        seen.add('equal')
    if 'tied_edges' in cl:
        assert _tied_edges(c) == cl['tied_edges']
        seen.add('tied_edges')
    if 'cls_chunks' in cl:
        assert -(-c['maps']['cls'][0].shape[1] // 16) == cl['cls_chunks'] <= 8
        assert all(int(l.max()) < NC for l in c['labels'] if len(l))
        seen.add('cls_chunks')
    if 'im_chunks' in cl:
        ch = c['maps']['x'][0].shape[1]
        chunk = max(32, -(-ch // 8))
        assert -(-ch // chunk) == cl['im_chunks']
        seen.add('im_chunks')
    if 'prob_zero_one' in cl:
        lab = t['labels']
        pos = (lab >= 0) & (lab < NC)
        z = o = 0
        for l, sl in enumerate(R.level_slices(sizes)):
            p = c['maps']['cls'][l].permute(0, 2, 3, 1).reshape(
                lab.shape[0], -1, 81).numpy()
            z += int((p[pos[:, sl]] == 0).sum())
            o += int((p[pos[:, sl]] == 1).sum())
        assert [z, o] == cl['prob_zero_one']
        seen.add('prob_zero_one')
    assert seen | {'empty_images'} == set(cl), set(cl) - seen


def _tied_edges(c):
    """Per overridden anchor: how many edges of the predicted box (the
    Integral of its reg rows, in float32 and in float64) equal the target's."""
    out = []
    offs = np.cumsum([0] + [h * w for h, w in c['sizes']])
    for n, a, box in c['overrides']:
        l = int(np.searchsorted(offs, a, side='right') - 1)
        r, (h, w), s = a - offs[l], c['sizes'][l], c['strides'][l]
        row = c['maps']['reg'][l][n, :, r // w, r % w]
        ties = []
        for dt in (np.float32, np.float64):
            e, _ = O.integral(row.numpy()[None])
            e64 = (torch.softmax(row.double().reshape(4, 17), 1) *
                   torch.arange(17.0, dtype=torch.float64)).sum(1).numpy()
            d = e[0] if dt is np.float32 else e64
            cx, cy = dt(r % w), dt(r // w)
            pred = np.array([cx - d[0], cy - d[1], cx + d[2], cy + d[3]], dt)
            ties.append(int((pred == box.astype(dt) / dt(s)).sum()))
        assert ties[0] == ties[1]
        out.append(ties[0])
    return out


# --------------------------------------------------------------- mutations ---
MUTATIONS = [('nts_no_image_floor', 'empty_beside_full', 'ld'),
             ('nts_no_image_floor', 'ten_blocks', 'retina'),
             ('im_without_pos', 'ten_blocks', 'ld'),
             ('kd_batch_count', 'ten_blocks', 'ld'),
             ('kd_batch_count', 'pos_every_level', 'atss'),
             ('avg_no_guard', 'all_empty', 'ld'),
             ('avg_no_guard', 'all_empty', 'atss'),
             ('vlr_at_T_ld', 'two_temperatures', 'ld'),
             ('score_attached', 'ragged', 'ld'),
             ('score_attached', 'pos_every_level', 'v2')]


@pytest.mark.parametrize('rule,name,flavour', MUTATIONS,
                         ids=[f'{r}-{n}-{f}' for r, n, f in MUTATIONS])
def test_wrong_rules_exceed_the_bar(rule, name, flavour):
    """The bar of the GPU tests is not so wide that the bugs aimed at pass: the
    wrong rule moves an output by more than K_ORACLE * e_oracle + F_SCALE *
    scale.  With no positive in the batch nothing is divided by the avg factor
    in exact arithmetic, so its guard shows in the factor alone (on the device
    a missing guard gives 0 * inf = NaN, which the GPU tests' finiteness
    assertions see): there the factor is the output compared.  LDRetinaHead's
    max(num_total_samples, 1) cannot be reached: the sum of per-image
    max(P_i, 1) is never below 1."""
    c = E.build(name, flavour)
    right = E.ref64(name, flavour)
    wrong = R.loss_block(flavour, c['maps'], c['targets'], c['hp'],
                         num_base=c['num_base'], wrong=(rule, ))
    e_o = E.oracle_error(name, flavour)
    a, b = E.outputs(right), E.outputs(wrong)
    if rule == 'avg_no_guard':
        a = dict(avg=np.array([right['avg_factor']]))
        b = dict(avg=np.array([wrong['avg_factor']]))
    moved = []
    for k in a:
        bar = E.K_ORACLE * e_o.get(k, 0.0) + \
            E.F_SCALE * float(np.abs(a[k]).max())
        d = np.abs(a[k] - b[k]).max()
        if not np.isfinite(d) or d > bar:
            moved.append((k, float(d), bar))
    assert moved, (rule, name, flavour)


# -------------------------------------------------------- oracle agreement ---
# the oracle has GIoU only: the other box_ties modes would repeat the GIoU run
ORACLE_PAIRS = [(c, f) for c, f in E.PAIRS
                if not c.startswith('box_ties') or c == 'box_ties_giou']


@pytest.mark.parametrize('name,flavour', ORACLE_PAIRS,
                         ids=[f'{c}-{f}' for c, f in ORACLE_PAIRS])
def test_oracle_agrees_with_ref64(name, flavour):
    """The float32 oracle against float64, per output, at what the oracle is
    held to against the reference itself (tests/test_oracle_*.py): 2e-5 of the
    scale + 2e-6 on the losses, 2e-4 of the scale on the gradients.  Its worst
    error per output is the e_oracle of the GPU bar."""
    ref = E.ref64(name, flavour)
    assert np.isfinite(ref['losses']).all()
    e_o = E.oracle_error(name, flavour)
    out = E.outputs(ref)
    assert set(e_o) == set(out)
    for k, e in e_o.items():
        scale = float(np.abs(out[k]).max())
        assert np.isfinite(out[k]).all(), k
        tol = 2e-5 * scale + 2e-6 if k.startswith('row') else \
            2e-4 * scale + 2e-8
        assert e <= tol, (k, e, scale)
