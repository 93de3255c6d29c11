"""GPU tests (-m gpu) of the three target kernels of ld_amd/csrc/targets.hip on
the crafted cases of tests/_target_edges.py: IoU ties between GT boxes,
duplicate boxes, centre-distance ties at the k-th place of the top-k, IoU
exactly 1, flat candidate IoUs (std 0), a single candidate (NaN threshold),
130 GT boxes (second trip of the 128-box chunk loop), no GT box at all, top-k
1 / 4 / 12 / 16, explicit anchors, IoUs exactly on the MaxIoU thresholds, the
low-quality override, FCOS points on box edges and on regress-range bounds,
equal areas, clamped centre boxes.

Every comparison is exact (assert_array_equal on the full dense arrays)
against oracle/ld_oracle.py and, where the reference's rule is deterministic,
against what the reference itself produced (tests/golden/target_edges.npz).
tests/test_target_edges_host.py certifies that each case contains its edge and
that a wrong tie / threshold rule would change its outputs.

The kernels have no launch counters, so the paths are covered by the case
list: every ATSS case runs once with LD_ATSS_SELECT=scan and once with the
default (the window kernel for top-k <= 9, atss_select_kernel<16> above)."""
import functools

import numpy as np
import pytest
import torch

import ld_oracle as O
import _target_edges as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev_lists(c):
    return ([torch.from_numpy(b).to(DEV) for b in c['boxes']],
            [torch.from_numpy(l).to(DEV) for l in c['labels']])


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------- ATSS ---
def _atss_gpu(c):
    from ld_amd import lossblock as LB
    gtb, gtl = _dev_lists(c)
    t = LB.atss_targets(c['sizes'], c['strides'], c['metas'], gtb, gtl,
                        LB.make_hp(topk=c['topk']), torch.device(DEV))
    torch.cuda.synchronize()
    return {k: _np(t[k]) for k in ('labels', 'label_weights', 'bbox_targets',
                                   'vlr', 'im', 'counts')}


@functools.lru_cache(maxsize=None)
def _atss_oracle(name):
    """Computed once per case, shared by the scan and the window run."""
    return E.oracle_atss(O, {**E.ATSS_CASES, **E.STRESS_CASES}[name]())


def _check_atss(got, want, keys):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _atss_counts(c, o):
    """counts as ld_atss_targets lays them out: positives per image,
    positives per level, IM anchors per level, sum_i max(P_i, 1)."""
    pos = (o['labels'] >= 0) & (o['labels'] < 80)
    per_img = pos.sum(1)
    lv_pos, lv_im, off = [], [], 0
    for h, w in c['sizes']:
        sl = slice(off, off + h * w)
        off += h * w
        lv_pos.append(pos[:, sl].sum())
        lv_im.append((o['im'][:, sl] > 0).sum())
    return np.array(list(per_img) + lv_pos + lv_im +
                    [np.maximum(per_img, 1).sum()], np.int32)


@pytest.mark.parametrize('select', ['scan', 'window'])
@pytest.mark.parametrize('name', list(E.ATSS_CASES) + list(E.STRESS_CASES))
def test_atss_edges_vs_oracle_and_reference(monkeypatch, golden, name, select):
    c = {**E.ATSS_CASES, **E.STRESS_CASES}[name]()
    if select == 'scan':
        monkeypatch.setenv('LD_ATSS_SELECT', 'scan')
    else:
        monkeypatch.delenv('LD_ATSS_SELECT', raising=False)
    got = _atss_gpu(c)
    o = _atss_oracle(name)
    _check_atss(got, o, ('labels', 'label_weights', 'bbox_targets', 'vlr',
                         'im'))
    assert o['num_total_pos'] == _atss_counts(c, o)[-1]
    np.testing.assert_array_equal(got['counts'], _atss_counts(c, o))
    g = golden['target_edges']
    if f'atss_{name}' in set(str(k) for k in g['cases']):
        _check_atss(got, E.atss_from_golden(O, c, g, name),
                    ('labels', 'label_weights', 'bbox_targets', 'vlr'))
    else:
        assert name in E.ATSS_TOPK_TIE_CASES or name in E.STRESS_CASES


@pytest.mark.parametrize('name', E.ATSS_EXPLICIT_CASES)
def test_atss_assigner_explicit_anchors_on_edges(name):
    """ld_atss_targets_ex through ATSSAssigner.assign / get_vlr_region on each
    image's valid anchors, as the reference's heads call them."""
    from ld_amd.registry import build_assigner
    c = E.ATSS_CASES[name]()
    assigner = build_assigner(dict(type='ATSSAssigner', topk=c['topk']))
    per_level = O.grid_anchors(c['sizes'], tuple(c['strides']))
    for n, gts in enumerate(c['boxes']):
        anc, nl, _ = E.inside_anchors(O, c, n, per_level)
        a = torch.from_numpy(anc).to(DEV)
        gb = torch.from_numpy(gts).to(DEV)
        gl = torch.from_numpy(c['labels'][n]).to(DEV)
        ar = assigner.assign(a, nl, gb, None, gl)
        gi, mo = O.atss_assign(anc, nl, gts, c['topk'])
        np.testing.assert_array_equal(_np(ar.gt_inds), gi)
        np.testing.assert_array_equal(_np(ar.max_overlaps), mo)
        np.testing.assert_array_equal(
            _np(ar.labels), np.where(gi > 0, c['labels'][n][gi - 1], -1))
        np.testing.assert_array_equal(
            _np(assigner.get_vlr_region(a, nl, gb, None, gl)),
            O.vlr_region(anc, nl, gts, c['topk']))
        assert (gi > 0).any()


# ----------------------------------------------------------------- MaxIoU ---
def _pseudo_to_reference(t, sizes, B):
    """(N * B, A[, 4]) pseudo-image layout -> (N, A * B[, 4]) in the
    reference's order (level, cell, base anchor)."""
    N = t.shape[0] // B
    t = t.reshape((N, B) + t.shape[1:])
    out, off = [], 0
    for h, w in sizes:
        lv = np.moveaxis(t[:, :, off:off + h * w], 1, 2)
        off += h * w
        out.append(lv.reshape((N, h * w * B) + lv.shape[3:]))
    return np.concatenate(out, 1)


class _Assigner:
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou):
        self.pos_iou_thr, self.neg_iou_thr = pos_iou_thr, neg_iou_thr
        self.min_pos_iou = min_pos_iou


@pytest.mark.parametrize('name', list(E.MAXIOU_CASES))
def test_maxiou_edges_vs_oracle_and_reference(golden, name):
    from ld_amd import lossblock as LB
    c = E.MAXIOU_CASES[name]()
    B = 9
    anchors = [torch.from_numpy(a).to(DEV) for a in
               O.retina_grid_anchors(c['sizes'], tuple(c['strides']))]
    gtb, gtl = _dev_lists(c)
    t = LB.retina_targets(c['sizes'], c['strides'], c['metas'], gtb, gtl,
                          anchors, B, _Assigner(**c['assigner']), 80,
                          torch.device(DEV), want_gt_inds=True)
    torch.cuda.synchronize()
    o = E.oracle_maxiou(O, c)
    got = {k: _pseudo_to_reference(_np(t[k]), c['sizes'], B)
           for k in ('gt_inds', 'labels', 'label_weights', 'bbox_targets',
                     'vlr', 'im')}
    for k in ('gt_inds', 'labels', 'label_weights', 'bbox_targets'):
        np.testing.assert_array_equal(got[k], o[k], err_msg=k)
    # the VLR mask, then the values: bit-equal on these dyadic inputs
    np.testing.assert_array_equal(got['vlr'] > 0, o['vlr'] > 0)
    np.testing.assert_array_equal(got['vlr'], o['vlr'])
    assert not got['im'].any()
    # counts: positives per pseudo-image, per level, (no IM), normaliser
    N, L = len(c['boxes']), len(c['sizes'])
    counts = _np(t['counts'])
    pos = _np(t['labels']) < 80                      # (N * B, A)
    np.testing.assert_array_equal(counts[:N * B], pos.sum(1))
    off = 0
    for l, (h, w) in enumerate(c['sizes']):
        assert counts[N * B + l] == pos[:, off:off + h * w].sum()
        assert counts[N * B + L + l] == 0
        off += h * w
    assert counts[N * B + 2 * L] == o['num_total_pos']
    assert o['num_total_pos'] == sum(max(int(p.sum()), 1)
                                     for p in o['pos_mask'])
    # the reference's own outputs
    g = golden['target_edges']
    for n in range(N):
        np.testing.assert_array_equal(got['gt_inds'][n],
                                      g[f'maxiou_{name}_gt_inds_{n}'])
        if E.maxiou_vlr_is_stored(O, c, n):
            np.testing.assert_array_equal(got['vlr'][n],
                                          g[f'maxiou_{name}_vlr_{n}'])


# ------------------------------------------------------------------- FCOS ---
@pytest.mark.parametrize('cs', [False, True])
@pytest.mark.parametrize('name', list(E.FCOS_CASES))
def test_fcos_edges_vs_oracle_and_reference(golden, name, cs):
    from ld_amd import lossblock as LB
    c = E.FCOS_CASES[name]()
    gtb, gtl = _dev_lists(c)
    t = LB.fcos_targets(c['sizes'], c['strides'], gtb, gtl, 80,
                        O.FCOS_RANGES, cs, 1.5, torch.device(DEV))
    torch.cuda.synchronize()
    g = golden['target_edges']
    N, L = len(c['boxes']), len(c['sizes'])
    o = E.oracle_fcos(O, c, cs)
    ref = dict(
        labels=np.stack([g[f'fcos_{name}_cs{int(cs)}_labels_{n}']
                         for n in range(N)]).astype(np.int64),
        bbox_targets=np.stack([g[f'fcos_{name}_cs{int(cs)}_bbox_targets_{n}']
                               for n in range(N)]))
    labels, vlr, bt = _np(t['labels']), _np(t['vlr']), _np(t['bbox_targets'])
    for want in (o, ref):   # FULL dense arrays, unassigned points included
        np.testing.assert_array_equal(
            labels, np.where(want['labels'] == 81, 80, want['labels']))
        np.testing.assert_array_equal(vlr, (want['labels'] == 81).astype(
            np.float32))
        np.testing.assert_array_equal(bt, want['bbox_targets'])
    assert (_np(t['label_weights']) == 1).all() and not _np(t['im']).any()
    counts = _np(t['counts'])
    pos = o['labels'] < 80
    np.testing.assert_array_equal(counts[:N], pos.sum(1))
    off = 0
    for l, (h, w) in enumerate(c['sizes']):
        assert counts[N + l] == pos[:, off:off + h * w].sum()
        assert counts[N + L + l] == 0
        off += h * w
    assert counts[N + 2 * L] == pos.sum()
