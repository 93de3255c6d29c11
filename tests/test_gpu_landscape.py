"""GPU checks (-m gpu) of landscape.hip through ld_amd.landscape:
ld_levels_mix against torch's fp32 ``a * x + b * y`` on the CPU bit for bit,
ld_levels_abs_err / ld_levels_pearson against the float64 restatements of
tests/_landscape_oracle.py (rtol 1e-9 / atol 1e-9: double accumulation of
<= 2^16 terms is bounded by n * 2^-53 ~ 7e-12), TeacherStudentDiscrepancy
against the restatement applied to the models' own outputs, and
FeatureLandscape against ``simple_test``'s tail and a hand loop over the
grid points."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landscape_oracle as O  # noqa: E402

DEV = 'cuda:0'
COEFS = [(1.0, 0.0), (0.0, 1.0), (0.9, 0.7), (-0.3, 1.25), (0.5, 0.5),
         (2.0, -1.0), (0.1, 0.0), (0.0, -0.2), (1e-3, 1e3), (0.33, 0.67),
         (1.0, 1.0), (-1.0, -1.0), (0.7, 0.9), (3.0, 0.25), (0.6, 0.4),
         (0.25, 0.75), (0.8, 0.2)]


def _bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


# --------------------------------------------------------------------- mix --
MIX_LEVELS = {'p52': ((5, 7), (3, 4), (2, 2), (1, 1)),
              'p53': ((5, 7), (3, 4), (2, 3))}


@pytest.fixture(scope='module')
def mix_inputs():
    g = torch.Generator().manual_seed(11)
    out = {}
    for tag, levels in MIX_LEVELS.items():
        out[tag] = tuple([torch.randn(2, 5, h, w, generator=g)
                          for h, w in levels] for _ in range(2))
    return out


@pytest.mark.parametrize('K', [1, 3, 17])
@pytest.mark.parametrize('layout', ['levels', 'packed', 'offset'])
@pytest.mark.parametrize('tag', list(MIX_LEVELS))
def test_mix_equals_torch_cpu_bit_for_bit(mix_inputs, tag, layout, K):
    from ld_amd import lib as L
    from ld_amd.landscape import mix_levels
    assert L.LD_LEVELS_MIX_MAX_K == 16  # K = 17: one more than a launch takes
    own, other = mix_inputs[tag]
    levels = MIX_LEVELS[tag]
    x, _ = O.pack(own)
    y, _ = O.pack(other)
    coefs = COEFS[:K]
    ref = torch.cat([a * x + b * y for a, b in coefs])  # fp32, torch CPU
    if layout == 'levels':
        out, lv = mix_levels([f.to(DEV) for f in own],
                             [f.to(DEV) for f in other], coefs)
    else:
        def dev(t):
            if layout == 'packed':
                return t.to(DEV)
            buf = torch.empty(t.numel() + 1, device=DEV)  # base + one float
            buf[1:] = t.flatten().to(DEV)
            v = buf[1:].view(t.shape)
            assert v.data_ptr() % 16 == 4
            return v
        out, lv = mix_levels(dev(x), dev(y), coefs, levels=levels)
    assert lv == levels and out.is_cuda and out.is_contiguous()
    assert tuple(out.shape) == (K * 2, 5, x.shape[2])
    _bits(out, ref)
    _bits(out[:2], x)  # the (1, 0) point returns own bit for bit


# ----------------------------------------------------------------- abs_err --
ERR_LEVELS = ((13, 21), (7, 11), (1, 1))


@pytest.mark.parametrize('c', [1, 68, 80, 256])
def test_abs_err_against_float64(c):
    from ld_amd.landscape import levels_abs_err
    g = torch.Generator().manual_seed(100 + c)
    P = sum(h * w for h, w in ERR_LEVELS)
    t3, s3 = torch.randn(2, c, P, generator=g), torch.randn(2, c, P,
                                                            generator=g)
    ref = O.abs_err(t3, s3, ERR_LEVELS).numpy()
    td, sd = t3.to(DEV), s3.to(DEV)
    out = levels_abs_err(td, sd, ERR_LEVELS)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, 3)
    print('abs_err C', c, 'max rel diff',
          float(np.abs(out.cpu().numpy() / ref - 1).max()))
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-9, atol=0)
    _bits(levels_abs_err(td, sd, ERR_LEVELS), out)
    assert float(levels_abs_err(td, td, ERR_LEVELS).abs().max()) == 0.0


# ----------------------------------------------------------------- Pearson --
# segment lengths 1, 2, 63, 64, 65, 77 (one wave per row) and 4200 (a
# workgroup per row)
R_LEVELS = ((1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (7, 11), (50, 84))


@pytest.fixture(scope='module')
def pearson_inputs():
    g = torch.Generator().manual_seed(21)
    P = sum(h * w for h, w in R_LEVELS)
    N, c = 2, 7  # 14 rows: the last workgroup of a short level has idle waves
    s3 = torch.randn(N, c, P, generator=g)
    t3 = 0.6 * s3 + 0.8 * torch.randn(N, c, P, generator=g)
    t3[:, 0] = 2.5                          # a constant row (degenerate)
    t3[:, 1] = s3[:, 1]                     # an identical pair
    t3[:, 2] = -s3[:, 2]                    # a negated pair
    s3[:, 3] += 1e4                         # mean 1e4, unit variance
    t3[:, 3] += 1e4
    s3[1, 5] = -1.0                         # constant in the other operand
    return t3, s3


def test_pearson_against_float64(pearson_inputs):
    from ld_amd.landscape import levels_pearson
    t3, s3 = pearson_inputs
    N, c, _ = t3.shape
    td, sd = t3.to(DEV), s3.to(DEV)
    r_sum, counts = levels_pearson(td, sd, R_LEVELS)
    assert r_sum.dtype == torch.float64 and counts.dtype == torch.int32
    ref_sum, valid, bad = O.pearson(t3, s3, R_LEVELS)
    assert counts[..., 0].cpu().tolist() == valid.tolist()
    assert counts[..., 1].cpu().tolist() == bad.tolist()
    assert bad[:, 0].tolist() == [c, c]            # one position: every row
    assert bad[0, 1:].tolist() == [1] * 6 and bad[1, 1:].tolist() == [2] * 6
    print('pearson sum max abs diff',
          float((r_sum.cpu() - ref_sum).abs().max()))
    np.testing.assert_allclose(r_sum.cpu().numpy(), ref_sum.numpy(), rtol=0,
                               atol=1e-9)
    r2, c2 = levels_pearson(td, sd, R_LEVELS)
    _bits(r2, r_sum)
    _bits(c2, counts)
    # row by row: one channel per call
    rows = O.pearson_rows(t3, s3, R_LEVELS)        # (N, L, C)
    for k in range(c):
        r, cnt = levels_pearson(td[:, k:k + 1].contiguous(),
                                sd[:, k:k + 1].contiguous(), R_LEVELS)
        want = rows[:, :, k]
        nan = torch.isnan(want)
        assert (cnt[..., 1].cpu() == nan.int()).all()
        np.testing.assert_allclose(
            r.cpu().numpy(), torch.where(nan, torch.zeros_like(want),
                                         want).numpy(), rtol=0, atol=1e-9)
    want = rows[:, 1:]
    np.testing.assert_allclose(want[:, :, 1].numpy(), 1.0, atol=1e-12)
    np.testing.assert_allclose(want[:, :, 2].numpy(), -1.0, atol=1e-12)


# --------------------------------------------------------------- detectors --
def _seeded(cfg):
    from ld_amd import synthetic as S
    from ld_amd.registry import build_detector
    det = build_detector(cfg)
    det.load_state_dict(S.seeded_state_dict(det.state_dict(), seed=1))
    det.teacher_model.load_state_dict(
        S.seeded_state_dict(det.teacher_model.state_dict(), seed=2))
    return _ready(det)


def _ready(det):
    det.to(DEV).eval()
    for m in (det, det.teacher_model):  # seeded weights score low
        m.bbox_head.test_cfg['score_thr'] = 0.001
    return det


def _batch():
    from ld_amd import synthetic as S
    batch = S.synthetic_batch(2, (60, 90), (64, 96), [2, 3], 7)
    metas = batch['img_metas']
    for m, sf in zip(metas, (1.0, 1.25)):
        m['scale_factor'] = np.array([sf] * 4, dtype=np.float32)
    return batch['img'].to(DEV), metas


def _simple(model, img, metas, feats=None):
    """simple_test's tail -> [(dets, labels)] device tensors."""
    with torch.no_grad():
        x = model.extract_feat(img) if feats is None else feats
        outs = model.bbox_head(x)
        return model.bbox_head.get_bboxes(*outs, metas, rescale=True)


def _same_boxes(got, want):
    assert len(got) == len(want)
    for (d, l), (rd, rl) in zip(got, want):
        assert d.dtype == torch.float32 and l.dtype == torch.int64
        assert torch.isfinite(d).all()
        _bits(d, rd)
        _bits(l, rl)


@pytest.fixture(scope='module')
def ld():
    """The seeded R18 <- R18 LD detector, a batch of two 64 x 96 images, the
    plain detections of its student, and a small COCO ground truth: the three
    best student detections of each image."""
    from ld_amd import model_zoo
    from ld_amd.coco_eval import CocoGroundTruth
    det = _ready(model_zoo.build_seeded_ld_detector(18, 18, DEV))
    img, metas = _batch()
    plain = _simple(det, img, metas)
    assert sum(d.shape[0] for d, _ in plain) > 0
    anns = [dict(bboxes=d[:3, :4].cpu().numpy(), labels=l[:3].cpu().numpy())
            for d, l in plain]
    return dict(det=det, img=img, metas=metas, plain=plain, anns=anns,
                gt=CocoGroundTruth.from_annotations(anns, num_classes=80))


def test_discrepancy_against_the_restatement(ld):
    from ld_amd.landscape import TeacherStudentDiscrepancy
    det, img = ld['det'], ld['img']
    acc = TeacherStudentDiscrepancy(det)
    assert acc.teacher is det.teacher_model
    acc.add(img)
    acc.add(img[:1])
    got = acc.compute()
    adds = []
    with torch.no_grad():
        for im in (img, img[:1]):
            xs, xt = det.extract_feat(im), det.teacher_model.extract_feat(im)
            adds.append(([f.cpu() for f in xs], [f.cpu() for f in xt],
                         [[f.cpu() for f in o] for o in det.bbox_head(xs)],
                         [[f.cpu() for f in o]
                          for o in det.teacher_model.bbox_head(xt)]))
    want = O.discrepancy(adds)
    print('discrepancy', {k: np.asarray(v).tolist() for k, v in got.items()})
    assert set(got) == set(want) and got['num_images'] == 3
    assert want['feature_error'] > 0 and want['cls_error'] > 0
    for k in ('feature', 'cls', 'bbox'):
        np.testing.assert_allclose(got[f'{k}_error'], want[f'{k}_error'],
                                   rtol=1e-9)
        np.testing.assert_allclose(got[f'{k}_error_levels'],
                                   want[f'{k}_error_levels'], rtol=1e-9)
        assert got[f'{k}_error_levels'].shape == (5, )
    np.testing.assert_allclose(got['pearson'], want['pearson'], rtol=0,
                               atol=1e-9, equal_nan=True)
    assert got['degenerate_rows'].tolist() == want['degenerate_rows'].tolist()
    assert got['degenerate_rows'][4] == 3 * 256      # the 1 x 1 level


def test_discrepancy_of_a_model_with_itself(ld):
    from ld_amd.landscape import TeacherStudentDiscrepancy
    t = ld['det'].teacher_model
    acc = TeacherStudentDiscrepancy(t, t)
    acc.add(ld['img'])
    got = acc.compute()
    for k in ('feature', 'cls', 'bbox'):
        assert got[f'{k}_error'] == 0.0
        assert not got[f'{k}_error_levels'].any()
    np.testing.assert_allclose(got['pearson'][:4], 1.0, rtol=0, atol=1e-9)
    assert np.isnan(got['pearson'][4]) and got['num_images'] == 2


def test_landscape_identity_point_is_simple_test(ld):
    from ld_amd.coco_eval import CocoEvaluator
    from ld_amd.landscape import FeatureLandscape
    land = FeatureLandscape(ld['det'], coefs=[(1.0, 0.0)], chunk=1,
                            evaluator_factory=lambda: CocoEvaluator(ld['gt']))
    got = land.detect(ld['img'], ld['metas'], rescale=True)
    assert len(got) == 1
    _same_boxes(got[0], ld['plain'])
    land.add(ld['img'], ld['metas'], gt=[0, 1])
    ref = CocoEvaluator(ld['gt'])
    ref.add([0, 1], [d for d, _ in ld['plain']], [l for _, l in ld['plain']])
    res, want = land.compute(), ref.compute()
    assert isinstance(res, list) and len(res) == 1
    assert np.array_equal(res[0]['stats'], want['stats'], equal_nan=True)
    assert res[0]['stats'][0] > 0  # the GTs are its own best detections


def test_landscape_teacher_head_at_the_reference_point(ld):
    """coefs (0.9, 0.7) on the second model's head, the point the reference
    ships (single_stage.py:115-119), against the torch expression per
    level."""
    from ld_amd.coco_eval import CocoEvaluator
    from ld_amd.landscape import FeatureLandscape
    det, img, metas = ld['det'], ld['img'], ld['metas']
    land = FeatureLandscape(det, head='teacher',
                            evaluator_factory=lambda: CocoEvaluator(ld['gt']))
    got = land.detect(img, metas)
    with torch.no_grad():
        x = det.teacher_model.extract_feat(img)
        former = det.extract_feat(img)
        y = tuple(0.9 * a + 0.7 * b for a, b in zip(x, former))
    _same_boxes(got[0], _simple(det.teacher_model, img, metas, feats=y))


def test_landscape_grid_equals_a_hand_loop(ld):
    """A 2 x 2 grid, all four points in one head forward (batch 8), at
    chunk = 1 (batch 2) and as a hand loop -- mix_levels, head, get_bboxes,
    evaluator, one point at a time: the same detections bit for bit and the
    same evaluator results."""
    from ld_amd.coco_eval import CocoEvaluator
    from ld_amd.landscape import FeatureLandscape, mix_levels
    det, img, metas = ld['det'], ld['img'], ld['metas']
    fac = lambda: CocoEvaluator(ld['gt'])  # noqa: E731
    grid = FeatureLandscape.grid([1.0, 0.8], [0.0, 0.3])
    lands = {ch: FeatureLandscape(det, coefs=grid, chunk=ch,
                                  evaluator_factory=fac) for ch in (None, 1)}
    assert lands[None].chunks(4, 2, None) == [(0, 4)]
    head = det.bbox_head
    hand, hand_res = [], []
    with torch.no_grad():
        xs, xt = det.extract_feat(img), det.teacher_model.extract_feat(img)
        for a, b in grid:
            x3, lv = mix_levels(xs, xt, [(a, b)])
            boxes = head.get_bboxes(*head.forward_packed(x3, lv), metas,
                                    rescale=True)
            ev = fac()
            ev.add([0, 1], [d for d, _ in boxes], [l for _, l in boxes])
            hand.append(boxes)
            hand_res.append(ev.compute())
    dets = {ch: land.detect(img, metas) for ch, land in lands.items()}
    for k in range(4):  # measured before anything is asserted
        for (d, _), (rd, _) in zip(dets[None][k], dets[1][k]):
            print('point', grid[k], 'dets', tuple(d.shape), tuple(rd.shape),
                  'max |chunked - chunk 1|',
                  float((d - rd).abs().max()) if d.shape == rd.shape
                  else 'shapes differ')
    _same_boxes(hand[0], ld['plain'])
    for k in range(4):
        _same_boxes(dets[1][k], hand[k])
        _same_boxes(dets[None][k], hand[k])
    stats = []
    for ch, land in lands.items():
        land.add(img, metas, gt=[0, 1])
        res = land.compute()
        assert res.shape == (2, 2) and res.dtype == object
        for k, r in enumerate(res.reshape(-1)):
            assert np.array_equal(r['stats'], hand_res[k]['stats'],
                                  equal_nan=True)
            assert np.array_equal(r['precision'], hand_res[k]['precision'])
        stats.append([r['stats'][0] for r in res.reshape(-1)])
    print('AP over the grid', stats[0])
    assert stats[0][0] > 0


@pytest.mark.parametrize('kind', ['atss', 'gfocal'])
def test_landscape_other_heads(kind):
    """A head with a third output (ATSS centerness) and GFocalHead: finite
    detections, the (1, 0) identity, and the MapAccumulator /
    RecallAccumulator feeds."""
    from ld_amd import model_zoo
    from ld_amd.evaluation import MapAccumulator
    from ld_amd.landscape import FeatureLandscape
    from ld_amd.recall import RecallAccumulator
    det = _seeded(model_zoo.ld_atss_detector(18, 18) if kind == 'atss'
                  else model_zoo.ldv2_detector(18, 18))
    img, metas = _batch()
    plain = _simple(det, img, metas)
    assert sum(d.shape[0] for d, _ in plain) > 0
    gt_boxes = [d[:2, :4].clone() for d, _ in plain]
    gt_labels = [l[:2].clone() for _, l in plain]
    if kind == 'atss':
        fac = lambda: MapAccumulator(80, device=DEV)  # noqa: E731
        gt = (gt_boxes, gt_labels)
    else:
        fac = lambda: RecallAccumulator((1, 100), 0.5, device=DEV)  # noqa: E731,E501
        gt = gt_boxes
    land = FeatureLandscape(det, coefs=[(1.0, 0.0), (0.5, 0.5), (0.9, 0.7)],
                            evaluator_factory=fac)
    got = land.detect(img, metas)
    assert len(got) == 3
    _same_boxes(got[0], plain)
    for boxes in got[1:]:
        for d, l in boxes:
            assert d.shape[1] == 5 and torch.isfinite(d).all()
            assert l.shape[0] == d.shape[0]
    land.add(img, metas, gt=gt)
    res = land.compute()
    assert len(res) == 3
    if kind == 'atss':
        mean_ap, _ = res[0][0]
        assert mean_ap > 0
    else:
        assert res[0].shape == (2, 1) and res[0][1, 0] == 1.0
