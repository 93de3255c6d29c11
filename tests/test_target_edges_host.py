"""Host checks of the crafted target-assignment cases (tests/_target_edges.py):

 1. self-certification -- every case contains the edge its `claims` promise,
    recomputed with oracle/ld_oracle.py alone and asserted as counts;
 2. sensitivity -- a deliberately wrong tie / threshold rule (written here,
    never in oracle/) changes at least one dense output of the case aimed at
    it, so the case would catch that bug in a kernel;
 3. oracle == reference on every case stored in tests/golden/target_edges.npz
    (written by `oracle/gen_golden.py --only target_edges` from the reference's
    own assigners).  The top-k distance-tie cases are not stored: torch.topk's
    order among equals is unspecified and the oracle's documented rule (lower
    anchor index) is the definition; whether the reference happened to agree
    is kept as an informational array and not asserted."""
import numpy as np
import pytest

import ld_oracle as O
import _target_edges as E

F32 = np.float32


def _equal_dense(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _dup_pairs(c):
    n = 0
    for b in c['boxes']:
        for i in range(len(b)):
            n += sum(np.array_equal(b[i], b[j]) for j in range(i + 1, len(b)))
    return n


def _common(c):
    return dict(dup_pairs=_dup_pairs(c),
                max_gt=max(len(b) for b in c['boxes']),
                empty_images=sum(len(b) == 0 for b in c['boxes']))


def _check(claims, got):
    """A claimed count is a lower bound; a claimed 0 and the counts that are
    sizes ('max_gt', 'positives') are exact."""
    for k, want in claims.items():
        assert k in got, f'claim {k!r} is not measured'
        if want == 0 or k in ('max_gt', 'positives'):
            assert got[k] == want, (k, got[k], want)
        else:
            assert got[k] >= want, (k, got[k], want)


# ------------------------------------------------------------------- ATSS ---
def _atss_pos_matrix(anc, nl, gts, topk):
    """(A, G) IoU where the anchor is an above-threshold, centre-inside
    candidate of the GT, else -inf; plus the thresholds and candidate IoUs."""
    ov = O.bbox_overlaps(anc, gts)
    cands, _ = O._candidates(anc, nl, gts, topk)
    thr, co = O._atss_threshold(ov, cands)
    acx, acy = O._centres(anc)
    mn = np.minimum(
        np.minimum(acx[cands] - gts[None, :, 0], acy[cands] - gts[None, :, 1]),
        np.minimum(gts[None, :, 2] - acx[cands], gts[None, :, 3] - acy[cands]))
    pos = (co >= thr[None, :]) & (mn > F32(0.01))
    m = np.full(ov.shape, -np.inf, F32)
    gi = np.broadcast_to(np.arange(gts.shape[0])[None, :], cands.shape)
    m[cands[pos], gi[pos]] = ov[cands[pos], gi[pos]]
    return m, thr, co, ov


def measure_atss(c):
    got = _common(c)
    got.update(kth_ties=0, gt_iou_tie_anchors=0, iou_one=0, flat_gts=0,
               nan_thr=0)
    per_level = O.grid_anchors(c['sizes'], tuple(c['strides']))
    for n, gts in enumerate(c['boxes']):
        if len(gts) == 0:
            continue
        anc, nl, _ = E.inside_anchors(O, c, n, per_level)
        got['kth_ties'] += E.kth_ties(O, anc, nl, gts, c['topk'])
        m, thr, co, ov = _atss_pos_matrix(anc, nl, gts, c['topk'])
        got['iou_one'] += int((ov == F32(1)).sum())
        got['nan_thr'] += int(np.isnan(thr).sum())
        got['flat_gts'] += int(((co == co[:1]).all(0) &
                                (co.shape[0] > 1)).sum())
        if len(gts) > 1:
            s = np.sort(m, axis=1)
            tie = (s[:, -1] == s[:, -2]) & np.isfinite(s[:, -1])
            got['gt_iou_tie_anchors'] += int(tie.sum())
    t = E.oracle_atss(O, c)
    got['positives'] = int((t['labels'] < 80).sum())
    return got


@pytest.mark.parametrize('name', list(E.ATSS_CASES) + list(E.STRESS_CASES))
def test_atss_case_contains_its_edge(name):
    c = {**E.ATSS_CASES, **E.STRESS_CASES}[name]()
    got = measure_atss(c)
    print(name, got)
    _check(c['claims'], got)
    if name in E.ATSS_TOPK_TIE_CASES:
        assert got['kth_ties'] > 0
    elif name in E.ATSS_CASES:
        assert got['kth_ties'] == 0, 'reference rule not deterministic here'


def _atss_assign_high_gt(anchors, num_level, gts, topk=9):
    """WRONG on purpose: the highest GT index wins an IoU tie."""
    anchors = np.asarray(anchors, F32)
    gts = np.asarray(gts, F32).reshape(-1, 4)
    gt_inds = np.zeros(anchors.shape[0], np.int64)
    if gts.shape[0] == 0:
        return gt_inds, np.zeros(anchors.shape[0], F32)
    m = _atss_pos_matrix(anchors, num_level, gts, topk)[0]
    G = gts.shape[0]
    arg = G - 1 - m[:, ::-1].argmax(1)   # last maximum
    sel = np.isfinite(m.max(1))
    gt_inds[sel] = arg[sel] + 1
    return gt_inds, m.max(1)


def _candidates_high_anchor(anchors, num_level, gts, topk):
    """WRONG on purpose: the highest anchor index wins a distance tie."""
    _, dist = _ORIG_CANDIDATES(anchors, num_level, gts, topk)
    cands, start = [], 0
    for n in num_level:
        k = min(topk, n)
        if k > 0:
            d = dist[start:start + n]
            order = np.stack([np.lexsort((-np.arange(n), d[:, g]))[:k]
                              for g in range(d.shape[1])], 1)
            cands.append(order + start)
        start += n
    return np.concatenate(cands, 0), dist


_ORIG_CANDIDATES = O._candidates
ATSS_KEYS = ('labels', 'label_weights', 'bbox_targets', 'vlr', 'im')


@pytest.mark.parametrize('name', ['dup_gt', 'iou_tie', 'topk16'])
def test_atss_gt_tie_rule_is_visible(monkeypatch, name):
    c = E.ATSS_CASES[name]()
    right = E.oracle_atss(O, c)
    monkeypatch.setattr(O, 'atss_assign', _atss_assign_high_gt)
    wrong = E.oracle_atss(O, c)
    assert not _equal_dense(right, wrong, ATSS_KEYS)


@pytest.mark.parametrize('name', E.ATSS_TOPK_TIE_CASES)
def test_atss_distance_tie_rule_is_visible(monkeypatch, name):
    c = E.ATSS_CASES[name]()
    right = E.oracle_atss(O, c)
    monkeypatch.setattr(O, '_candidates', _candidates_high_anchor)
    wrong = E.oracle_atss(O, c)
    assert not _equal_dense(right, wrong, ATSS_KEYS)


def test_atss_wrong_rules_are_silent_without_ties(monkeypatch):
    """The two wrong rules change nothing on a case without the tie they
    mistreat: the differences above come from the ties alone."""
    c = E.ATSS_CASES['gt_is_anchor']()
    right = E.oracle_atss(O, c)
    monkeypatch.setattr(O, '_candidates', _candidates_high_anchor)
    monkeypatch.setattr(O, 'atss_assign', _atss_assign_high_gt)
    assert _equal_dense(right, E.oracle_atss(O, c), ATSS_KEYS)


# ----------------------------------------------------------------- MaxIoU ---
def _lowq(ov, min_pos):
    gt_max = ov.max(1)
    return (ov == gt_max[:, None]) & (gt_max >= F32(min_pos))[:, None]


def measure_maxiou(c):
    got = _common(c)
    got.update(iou_at_pos_thr=0, iou_at_neg_thr=0, shared_best_anchors=0,
               multi_argmax_gts=0, kth_ties=0)
    per_level = O.retina_grid_anchors(c['sizes'], tuple(c['strides']))
    a = c['assigner']
    for n, gts in enumerate(c['boxes']):
        if len(gts) == 0:
            continue
        anc, nl, _ = E.inside_anchors(O, c, n, per_level)
        got['kth_ties'] += E.kth_ties(O, anc, nl, gts, 9)
        ov = O.bbox_overlaps(gts, anc)
        lq = _lowq(ov, a['min_pos_iou'])
        mx = ov.max(0)
        free = ~lq.any(0)
        got['iou_at_pos_thr'] += int((free & (mx == F32(a['pos_iou_thr']))).sum())
        got['iou_at_neg_thr'] += int((free & (mx == F32(a['neg_iou_thr']))).sum())
        distinct = np.array([[not np.array_equal(gts[i], gts[j])
                              for j in range(len(gts))]
                             for i in range(len(gts))])
        for col in lq.T:
            g = np.nonzero(col)[0]
            if g.size > 1 and distinct[g[0], g[1:]].any():
                got['shared_best_anchors'] += 1
        got['multi_argmax_gts'] += int((lq.sum(1) > 1).sum())
    return got


@pytest.mark.parametrize('name', list(E.MAXIOU_CASES))
def test_maxiou_case_contains_its_edge(name):
    c = E.MAXIOU_CASES[name]()
    got = measure_maxiou(c)
    print(name, got)
    _check(c['claims'], got)


def _max_iou_wrong(rule):
    def assign(anchors, gts, pos_iou_thr=0.5, neg_iou_thr=0.4,
               min_pos_iou=0.0):
        anchors = np.asarray(anchors, F32)
        gts = np.asarray(gts, F32).reshape(-1, 4)
        out = np.full(anchors.shape[0], -1, np.int64)
        if gts.shape[0] == 0:
            out[:] = 0
            return out
        ov = O.bbox_overlaps(gts, anchors)
        mx, arg = ov.max(0), ov.argmax(0)
        neg = mx <= F32(neg_iou_thr) if rule == 'neg_inclusive' else \
            mx < F32(neg_iou_thr)
        out[(mx >= 0) & neg] = 0
        pos = mx > F32(pos_iou_thr) if rule == 'pos_strict' else \
            mx >= F32(pos_iou_thr)
        out[pos] = arg[pos] + 1
        lq = _lowq(ov, min_pos_iou)
        order = range(gts.shape[0])
        for g in (reversed(order) if rule == 'lowq_first' else order):
            out[lq[g]] = g + 1
        return out
    return assign


MAXIOU_KEYS = ('labels', 'label_weights', 'bbox_targets', 'gt_inds', 'vlr')


def test_maxiou_variant_with_the_right_rules_is_the_oracle(monkeypatch):
    for name in E.MAXIOU_CASES:
        c = E.MAXIOU_CASES[name]()
        right = E.oracle_maxiou(O, c)
        with monkeypatch.context() as m:
            m.setattr(O, 'max_iou_assign', _max_iou_wrong(None))
            assert _equal_dense(right, E.oracle_maxiou(O, c), MAXIOU_KEYS)


@pytest.mark.parametrize('name,rule', [('pos_edge', 'pos_strict'),
                                       ('neg_edge', 'neg_inclusive'),
                                       ('lowq_override', 'lowq_first'),
                                       ('dup_gt', 'lowq_first')])
def test_maxiou_wrong_rule_is_visible(monkeypatch, name, rule):
    c = E.MAXIOU_CASES[name]()
    right = E.oracle_maxiou(O, c)
    monkeypatch.setattr(O, 'max_iou_assign', _max_iou_wrong(rule))
    wrong = E.oracle_maxiou(O, c)
    assert not _equal_dense(right, wrong, MAXIOU_KEYS)
    if name == 'neg_edge':   # ignored under the right rule, weighted under <=
        assert (right['label_weights'] == 0).sum() > \
            (wrong['label_weights'] == 0).sum()


# ------------------------------------------------------------------- FCOS ---
def _fcos(c, center_sampling, rule=None, radius=1.5):
    """fcos_targets restated with one rule optionally WRONG on purpose:
    'inside_nonstrict' (>= 0), 'range_exclusive' (open upper and lower bound),
    'area_high' (higher GT index on equal areas), 'no_clamp' (centre box not
    clamped to the GT)."""
    pts = O.fcos_points(c['sizes'], tuple(c['strides']))
    P = np.concatenate(pts)
    per = [np.full(len(p), v, F32) for p, v in zip(pts, range(len(pts)))]
    lv = np.concatenate(per).astype(np.int64)
    lo = np.array([r[0] for r in O.FCOS_RANGES], F32)[lv]
    hi = np.array([min(r[1], 1e8) for r in O.FCOS_RANGES], F32)[lv]
    sr = (np.array(c['strides'], np.float64) * radius).astype(F32)[lv]
    INF = F32(1e8)
    labs, bts = [], []
    for gb, gl in zip(c['boxes'], c['labels']):
        A = P.shape[0]
        if gb.shape[0] == 0:
            labs.append(np.full(A, 80, np.int64))
            bts.append(np.zeros((A, 4), F32))
            continue
        xs, ys = P[:, 0:1], P[:, 1:2]
        bt = np.stack([xs - gb[None, :, 0], ys - gb[None, :, 1],
                       gb[None, :, 2] - xs, gb[None, :, 3] - ys], -1)
        areas = np.tile(((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[None],
                        (A, 1)).astype(F32)
        if center_sampling:
            cx = (gb[:, 0] + gb[:, 2]) / F32(2)
            cy = (gb[:, 1] + gb[:, 3]) / F32(2)
            c0, c1 = cx[None] - sr[:, None], cy[None] - sr[:, None]
            c2, c3 = cx[None] + sr[:, None], cy[None] + sr[:, None]
            if rule != 'no_clamp':
                c0 = np.maximum(c0, gb[None, :, 0])
                c1 = np.maximum(c1, gb[None, :, 1])
                c2 = np.minimum(c2, gb[None, :, 2])
                c3 = np.minimum(c3, gb[None, :, 3])
            mn = np.stack([xs - c0, ys - c1, c2 - xs, c3 - ys], -1).min(-1)
        else:
            mn = bt.min(-1)
        inside = mn >= 0 if rule == 'inside_nonstrict' else mn > 0
        mx = bt.max(-1)
        if rule == 'range_exclusive':
            in_range = (mx > lo[:, None]) & (mx < hi[:, None])
        else:
            in_range = (mx >= lo[:, None]) & (mx <= hi[:, None])
        areas[~inside] = INF
        areas[~in_range] = INF
        if rule == 'area_high':
            arg = areas.shape[1] - 1 - areas[:, ::-1].argmin(1)
        else:
            arg = areas.argmin(1)
        m = areas[np.arange(A), arg]
        in_some = (bt.min(-1) > 0).any(1)
        lab = gl[arg].astype(np.int64)
        lab[m == INF] = 80
        lab[in_some & (m == INF)] = 81
        labs.append(lab)
        bts.append(bt[np.arange(A), arg].astype(F32))
    return dict(labels=np.stack(labs), bbox_targets=np.stack(bts), points=P,
                level=lv)


def measure_fcos(c):
    got = _common(c)
    got.update(on_edge=0, on_bound_64=0, on_bound_128=0, area_tie_points=0,
               clamped_out=0)
    t = _fcos(c, False)
    P, lv = t['points'], t['level']
    sr = (np.array(c['strides'], np.float64) * 1.5).astype(F32)[lv]
    hit = {64: set(), 128: set()}
    for gb in c['boxes']:
        if len(gb) == 0:
            continue
        xs, ys = P[:, 0:1], P[:, 1:2]
        bt = np.stack([xs - gb[None, :, 0], ys - gb[None, :, 1],
                       gb[None, :, 2] - xs, gb[None, :, 3] - ys], -1)
        mn, mx = bt.min(-1), bt.max(-1)
        got['on_edge'] += int((mn == 0).sum())
        for bound, levels in ((64, (0, 1)), (128, (1, 2))):
            for l in levels:   # a point of level l, strictly inside, on the bound
                if ((mx == bound) & (mn > 0) & (lv == l)[:, None]).any():
                    hit[bound].add(l)
        area = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[None]
        lo = np.array([r[0] for r in O.FCOS_RANGES], F32)[lv][:, None]
        hi = np.array([min(r[1], 1e8) for r in O.FCOS_RANGES], F32)[lv][:, None]
        ok = (mn > 0) & (mx >= lo) & (mx <= hi)
        a = np.where(ok, area, np.inf)
        if a.shape[1] > 1:
            s = np.sort(a, 1)
            got['area_tie_points'] += int(((s[:, 0] == s[:, 1]) &
                                           np.isfinite(s[:, 0])).sum())
        cx, cy = (gb[:, 0] + gb[:, 2]) / 2, (gb[:, 1] + gb[:, 3]) / 2
        raw = np.stack([xs - (cx[None] - sr[:, None]),
                        ys - (cy[None] - sr[:, None]),
                        cx[None] + sr[:, None] - xs,
                        cy[None] + sr[:, None] - ys], -1).min(-1) > 0
        # level-0 points within the sampling radius but outside the box
        got['clamped_out'] += int((raw & ~(mn > 0) & (lv == 0)[:, None]).sum())
    got['on_bound_64'], got['on_bound_128'] = len(hit[64]), len(hit[128])
    return got


@pytest.mark.parametrize('name', list(E.FCOS_CASES))
def test_fcos_case_contains_its_edge(name):
    c = E.FCOS_CASES[name]()
    got = measure_fcos(c)
    print(name, got)
    _check(c['claims'], got)


@pytest.mark.parametrize('cs', [False, True])
def test_fcos_variant_with_the_right_rules_is_the_oracle(cs):
    for name in E.FCOS_CASES:
        c = E.FCOS_CASES[name]()
        right, mine = E.oracle_fcos(O, c, cs), _fcos(c, cs)
        assert _equal_dense(right, mine, ('labels', 'bbox_targets'))


@pytest.mark.parametrize('name,rule,cs', [
    ('on_edge', 'inside_nonstrict', False),
    ('on_edge', 'inside_nonstrict', True),
    ('range_bound', 'range_exclusive', False),
    ('range_bound', 'range_exclusive', True),
    ('area_tie', 'area_high', False),
    ('area_tie', 'area_high', True),
    ('sample_clamp', 'no_clamp', True)])
def test_fcos_wrong_rule_is_visible(name, rule, cs):
    c = E.FCOS_CASES[name]()
    right, wrong = _fcos(c, cs), _fcos(c, cs, rule)
    assert not _equal_dense(right, wrong, ('labels', 'bbox_targets'))


# -------------------------------------------------------- reference golden ---
def test_golden_covers_every_deterministic_case(golden):
    g = golden['target_edges']
    have = set(str(k) for k in g['cases'])
    want = {f'atss_{n}' for n in E.ATSS_CASES
            if n not in E.ATSS_TOPK_TIE_CASES}
    want |= {f'maxiou_{n}' for n in E.MAXIOU_CASES}
    want |= {f'fcos_{n}' for n in E.FCOS_CASES}
    assert have == want
    for n in E.ATSS_TOPK_TIE_CASES:   # informational only, never asserted
        assert g[f'info_atss_{n}_ref_agrees'].dtype == np.bool_


@pytest.mark.parametrize('name', [n for n in E.ATSS_CASES
                                  if n not in E.ATSS_TOPK_TIE_CASES])
def test_atss_oracle_equals_reference(golden, name):
    g = golden['target_edges']
    c = E.ATSS_CASES[name]()
    t = E.oracle_atss(O, c)
    ref = E.atss_from_golden(O, c, g, name)
    for n in range(len(c['boxes'])):
        for k in ('labels', 'label_weights', 'bbox_targets', 'vlr'):
            np.testing.assert_array_equal(t[k][n], ref[k][n], err_msg=(k, n))
        if len(c['boxes'][n]):   # the assigner's own outputs
            gi, mo = E.oracle_atss_assign(O, c, n)
            np.testing.assert_array_equal(gi, g[f'atss_{name}_gt_inds_{n}'])
            np.testing.assert_array_equal(
                mo, g[f'atss_{name}_max_overlaps_{n}'])


@pytest.mark.parametrize('name', list(E.MAXIOU_CASES))
def test_maxiou_oracle_equals_reference(golden, name):
    g = golden['target_edges']
    c = E.MAXIOU_CASES[name]()
    t = E.oracle_maxiou(O, c)
    for n in range(len(c['boxes'])):
        np.testing.assert_array_equal(t['gt_inds'][n],
                                      g[f'maxiou_{name}_gt_inds_{n}'])
        k = f'maxiou_{name}_vlr_{n}'
        if E.maxiou_vlr_is_stored(O, c, n):
            np.testing.assert_array_equal(t['vlr'][n], g[k])
        else:   # no GT box (the reference's region code crashes), or a
            assert k not in g   # distance tie at a 9th place (torch.topk)
        if not len(c['boxes'][n]):
            assert not t['vlr'][n].any()


@pytest.mark.parametrize('name', list(E.FCOS_CASES))
@pytest.mark.parametrize('cs', [False, True])
def test_fcos_oracle_equals_reference(golden, name, cs):
    g = golden['target_edges']
    c = E.FCOS_CASES[name]()
    t = E.oracle_fcos(O, c, cs)
    for n in range(len(c['boxes'])):
        np.testing.assert_array_equal(
            t['labels'][n], g[f'fcos_{name}_cs{int(cs)}_labels_{n}'])
        np.testing.assert_array_equal(
            t['bbox_targets'][n],
            g[f'fcos_{name}_cs{int(cs)}_bbox_targets_{n}'])
