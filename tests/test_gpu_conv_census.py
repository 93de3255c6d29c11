"""GPU (-m gpu): every conv launch the real steps make, one layer at a time,
against the sampled float64 reference (tests/_conv_ref64.py).

A census (tests/_conv_census.py) records what one step of each BASELINE config
at its per-GPU size launches -- configs 1, 2, 3 (bf16), 5 forward and backward,
config 4 forward, and a simple_test inference forward at 800x1344.  Every
unique Python-level call (descriptor, operand kinds, epilogue) is then replayed
with seeded operands of exactly that geometry through the same public path, the
replay must reach the same entry points with the same descriptors, and each
output is held to |got - ref| <= 16 u S (plus the epilogue / accumulate / C8
terms, _conv_ref64.epilogue).  Composite launches: the deformable im2col
against float64 bilinear sampling, the grouped conv as per-group dense convs;
the fused bottleneck stays pinned bit-exact to its three launches
(test_gpu_fused_block.py), which must hold the geometries the census finds.

Finally every record of the shipped tune table must have been looked up by a
checked launch, or be listed in UNREACHED with its reason.

One line per signature is printed (run with -s): config tags, entry point,
geometry, largest K, sample count, worst |got - ref| / (u S).
"""
import math
import os

import numpy as np
import pytest
import torch

import _conv_census as CC
import _conv_ref64 as R

pytestmark = pytest.mark.gpu

U = R.U
# Tune-table records no checked launch looks up (key: the 18 ints), with why.
# All are family 1: the bf16 kernels that take fp32 activations.  With the C8
# path on (LD_CONV_C8=1, the default) the bf16 step feeds these geometries as C8
# images (family 2); the records serve LD_CONV_C8=0 runs.  The replay with the
# C8 path off (test_replay_bf16_without_c8) reaches only the units whose
# operands can all be fp32 -- most bf16 units of the step take a C8-only
# activation, residual or output -- so these stay unreached.
UNREACHED = {
    (1, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 1024, 256, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 1, 0, 1, 1, 0),
    (0, 128, 128, 3, 3, 2, 1, 33600, 1, 200, 336, 0, 0, 0, 0, 0, 1, 0),
    (1, 1024, 512, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (0, 512, 2048, 1, 1, 1, 0, 2100, 1, 25, 42, 0, 0, 0, 0, 0, 1, 0),
    (0, 256, 128, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 0, 0, 0, 1, 0),
    (1, 256, 256, 3, 3, 1, 1, 8400, 1, 50, 84, 1, 1, 0, 0, 0, 1, 0),
    (0, 256, 256, 3, 3, 2, 1, 8400, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 256, 256, 3, 3, 1, 1, 8400, 1, 50, 84, 0, 0, 1, 0, 1, 1, 0),
    (0, 256, 256, 3, 3, 2, 1, 8400, 1, 100, 168, 0, 0, 1, 0, 1, 1, 0),
    (0, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 0, 0, 0, 0, 0, 1, 0),
    (0, 64, 64, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 1, 0, 1, 1, 0),
    (0, 64, 256, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 0, 0, 1, 1, 0),
    (0, 1024, 512, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 1, 0, 1, 1, 0),
    (0, 512, 256, 1, 1, 1, 0, 33600, 1, 100, 168, 0, 0, 1, 0, 1, 1, 0),
    (1, 2048, 1024, 1, 1, 1, 0, 2100, 1, 25, 42, 0, 0, 0, 0, 0, 1, 0),
    (0, 256, 512, 1, 1, 2, 0, 33600, 1, 200, 336, 0, 0, 0, 0, 0, 1, 0),
    (0, 256, 1024, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 1, 1, 1, 1, 0),
    (0, 128, 128, 3, 3, 2, 1, 33600, 1, 200, 336, 0, 0, 1, 0, 1, 1, 0),
    (0, 64, 64, 3, 3, 1, 1, 134400, 1, 200, 336, 0, 0, 1, 0, 1, 1, 0),
    (1, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 1, 0, 0, 0, 0, 1, 0),
    (1, 256, 256, 3, 3, 1, 1, 8400, 1, 50, 84, 1, 0, 0, 0, 0, 1, 0),
    (0, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 0, 0, 1, 0, 1, 1, 0),
    (0, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 0, 0, 1, 0, 1, 1, 0),
    (0, 512, 1024, 1, 1, 2, 0, 8400, 1, 100, 168, 0, 0, 0, 0, 1, 1, 0),
    (1, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 0, 1, 0, 0, 0, 1, 0),
    (0, 512, 1024, 1, 1, 2, 0, 8400, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 256, 64, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 1, 0, 1, 1, 0),
    (0, 512, 128, 1, 1, 1, 0, 33600, 1, 100, 168, 0, 0, 1, 0, 1, 1, 0),
    (0, 64, 256, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 1, 1, 1, 1, 0),
    (1, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 1, 1, 0, 0, 0, 1, 0),
    (0, 512, 128, 1, 1, 1, 0, 33600, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 512, 2048, 1, 1, 1, 0, 2100, 1, 25, 42, 0, 0, 1, 1, 1, 1, 0),
    (0, 1024, 512, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (1, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 0, 1, 0, 0, 0, 1, 0),
    (0, 1024, 2048, 1, 1, 2, 0, 2100, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (0, 1024, 2048, 1, 1, 2, 0, 2100, 1, 50, 84, 0, 0, 0, 0, 1, 1, 0),
    (0, 128, 512, 1, 1, 1, 0, 33600, 1, 100, 168, 0, 0, 0, 0, 0, 1, 0),
    (0, 512, 1024, 1, 1, 1, 0, 8400, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (0, 128, 512, 1, 1, 1, 0, 33600, 1, 100, 168, 0, 0, 1, 1, 1, 1, 0),
    (0, 256, 512, 1, 1, 2, 0, 33600, 1, 200, 336, 0, 0, 0, 0, 1, 1, 0),
    (0, 512, 512, 3, 3, 2, 1, 2100, 1, 50, 84, 0, 0, 1, 0, 1, 1, 0),
    (0, 2048, 512, 1, 1, 1, 0, 2100, 1, 25, 42, 0, 0, 1, 0, 1, 1, 0),
    (0, 256, 128, 1, 1, 1, 0, 134400, 1, 200, 336, 0, 0, 1, 0, 1, 1, 0),
    (0, 2048, 512, 1, 1, 1, 0, 2100, 1, 25, 42, 0, 0, 0, 0, 0, 1, 0),
    (0, 512, 512, 3, 3, 2, 1, 2100, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (1, 128, 128, 3, 3, 1, 1, 33600, 1, 100, 168, 1, 0, 0, 0, 0, 1, 0),
    (1, 256, 256, 3, 3, 1, 1, 8400, 1, 50, 84, 0, 1, 0, 0, 0, 1, 0),
    (1, 256, 256, 3, 3, 1, 1, 8400, 1, 50, 84, 0, 0, 0, 0, 0, 1, 0),
    (1, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 0, 0, 0, 0, 0, 1, 0),
    (1, 512, 512, 3, 3, 1, 1, 2100, 1, 25, 42, 1, 1, 0, 0, 0, 1, 0),
}


def _dev():
    assert torch.cuda.is_available(), 'this test needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def census():
    from ld_amd import lib as L
    dev = _dev()
    L.get_lib().ld_conv_tune_reset_hits()
    rec = CC.Recorder()
    for name in CC.CONFIGS:
        CC.run_config(name, rec, dev)
    print(f'\ncensus: {len(rec.units)} units, {len(rec.signatures())} conv '
          f'signatures, {len(rec.other)} composite signatures')
    orphans = [k for k in rec.other if k[0] == 'orphan']
    assert not orphans, f'conv launches outside the recorded paths: {orphans}'
    return rec


def _randn(shape, gen, dev, absval=False):
    t = torch.randn(shape, generator=gen, device=dev)
    return t.abs() if absval else t


def _c8_view(buf, N, C, P):
    """(N, C/8, P, 8) bf16 image -> (N, C, P) fp32."""
    return buf.view(N, C // 8, P, 8).permute(0, 1, 3, 2).reshape(N, C, P).float()


def _line(tags, entry, desc, K, ns, worst, worst8=0.0):
    N, cin, cout, k, s, p, lv = desc
    lvs = ','.join(f'{h}x{w}' for h, w in lv)
    print(f'{"+".join(sorted(tags)):44s} {entry:28s} N{N} {cin}>{cout} k{k}s{s}'
          f'p{p} [{lvs}] K={K} n={ns} worst={worst:.2f}' +
          (f' c8_bar_used={worst8:.2f}' if worst8 else ''))


def _gather(t, n, c, p):
    return t[torch.as_tensor(n, device=t.device), torch.as_tensor(c, device=t.device),
             torch.as_tensor(p, device=t.device)].double().cpu().numpy()


def _chan(t, c):
    return t[torch.as_tensor(c, device=t.device)].double().cpu().numpy()


def _replay_fwd(key, prec, want, dev, seed, c8_off=False):
    from ld_amd import layers as Y
    (_, desc, xk, has_bias, has_aff, resk, relu, emit_c8, c8_only, has_raw,
     has_raw_c8) = key
    N, cin, cout, k, s, p, levels = desc
    g = R.Geom(N, cin, cout, k, s, p, levels)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = _randn((N, cin, g.Pin), gen, dev, absval=seed % 2 == 1)
    w = _randn((cout, cin, k, k), gen, dev) / math.sqrt(cin * k * k)
    bias = _randn((cout, ), gen, dev) if has_bias else None
    scale = torch.rand(cout, generator=gen, device=dev) + 0.5 if has_aff else None
    shift = _randn((cout, ), gen, dev) if has_aff else None
    res = _randn((N, cout, g.Pout), gen, dev) if resk != 'none' else None
    xin = x
    if xk == 'c8':
        xin = Y.C8Act(Y.to_c8(x), x.shape)
    elif xk in ('cached', 'unwritten'):
        Y.to_c8(x)  # the producer / another consumer left the image attached
    rin = res
    if resk in ('c8', 'unwritten'):
        rin = Y.C8Act(Y.to_c8(res), res.shape)
    y_raw = torch.empty((N, cout, g.Pout), device=dev) if has_raw else None
    y_raw_c8 = torch.empty(N * cout * g.Pout, dtype=torch.bfloat16,
                           device=dev) if has_raw_c8 else None
    rec = CC.Recorder()
    with rec:
        out, _ = Y.conv_forward_raw(xin, w, s, p, levels, bias=bias, scale=scale,
                                    shift=shift, residual=rin, relu=relu,
                                    emit_c8=emit_c8, c8_only=c8_only, y_raw=y_raw,
                                    y_raw_c8=y_raw_c8)
    torch.cuda.synchronize()
    got_sigs = _same_sigs(rec.signatures(), want, c8_off)
    (entry, _, ep), = got_sigs
    bf16 = 'bf16' in entry
    n, co, pp = R.sample_elements(N, cout, g.out_levels, g.off_out, g.Pout, seed)
    ref, S, K = R.forward(g, x, w, n, co, pp, bf16=bf16)
    sc = _chan(scale, co) if has_aff else None
    sh = np.zeros_like(ref)
    if has_aff:
        sh = sh + _chan(shift, co)
    if has_bias:
        sh = sh + _chan(bias, co)
    rs = None
    if res is not None:
        rs = _gather(R.bf16_rne(res) if resk in ('c8', 'unwritten') else res,
                     n, co, pp)
    worst, worst8 = 0.0, 0.0
    outs = []
    if c8_only:
        outs.append(('c8_only', _c8_view(out.buf, N, cout, g.Pout), True))
    else:
        outs.append(('y', out, False))
        img = Y._c8_cached(out) if emit_c8 else None
        if ep[5]:  # the epilogue wrote the C8 image
            assert img is not None
            outs.append(('y_c8', _c8_view(img, N, cout, g.Pout), True))
    if has_raw or has_raw_c8:
        braw = _chan(bias, co) if has_bias else None
        outs.append(('y_raw', y_raw, False) if has_raw else
                    ('y_raw_c8', _c8_view(y_raw_c8, N, cout, g.Pout), True))
    for what, t, c8 in outs:
        if what.startswith('y_raw'):
            v, bar = R.epilogue(ref, S, None, braw, None, False, c8=c8)
        else:
            v, bar = R.epilogue(ref, S, sc, sh, rs, relu, c8=c8)
        got = _gather(t, n, co, pp)
        r = R.check(got, v, S, bar, what=f'{entry} {what} {desc}')
        if c8:  # bf16-rounded output: report the share of the bar used
            worst8 = max(worst8, float((np.abs(got - v) / bar).max()))
        else:
            worst = max(worst, r)
    return [(entry, int(K.max()), len(n), worst, worst8)]


def _same_sigs(got, want, c8_off):
    """The replay must reach the recorded entry points and descriptors; with
    the C8 path switched off (c8_off) it must reach the fp32-activation bf16
    kernels instead."""
    if not c8_off:
        assert got == want, f'replay reached {got}, the step {want}'
    else:
        assert got and not any('_c8' in s[0] for s in got), got
        assert {s[1] for s in got} == {s[1] for s in want}, (got, want)
    return got


def _replay_bwd(key, prec, want, dev, seed, c8_off=False):
    from ld_amd import layers as Y
    (_, desc, xk, dyk, need_x, need_w, has_add, sink, defer) = key
    N, cin, cout, k, s, p, levels = desc
    g = R.Geom(N, cin, cout, k, s, p, levels)
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = _randn((N, cin, g.Pin), gen, dev, absval=seed % 2 == 1)
    w = _randn((cout, cin, k, k), gen, dev) / math.sqrt(cout * k * k)
    dy = _randn((N, cout, g.Pout), gen, dev)
    add = _randn((N, cin, g.Pin), gen, dev) if has_add else None
    base = _randn(w.shape, gen, dev) if sink else None
    x8 = Y.C8Act(Y.to_c8(x), x.shape) if xk == 'c8' else None
    if xk in ('cached', 'unwritten'):
        Y.to_c8(x)
    dyin = dy
    if dyk == 'c8':
        dyin = Y.C8Act(Y.to_c8(dy), dy.shape)
    elif dyk in ('cached', 'unwritten'):
        Y.to_c8(dy)
    if sink:
        w._ld_grad = base.clone()
    Y.drop_deferred()
    saved = Y._DEFER_ON[0]
    Y._DEFER_ON[0] = defer
    rec = CC.Recorder()
    try:
        with rec:
            dx, dw, _ = Y._conv_backward(
                x, x8, w, dyin, (s, p, levels, False), (w, None), need_x, need_w,
                False, addend=None if add is None else add.clone())
            Y.wgrad_join(dev)
            Y.flush_deferred(dev)
        torch.cuda.synchronize()
    finally:
        Y._DEFER_ON[0] = saved
        Y.drop_deferred()
    got_sigs = _same_sigs(rec.signatures(), want, c8_off)
    rows = []
    for entry, _, extra in sorted(got_sigs):
        if 'dgrad' in entry:
            bf16 = 'bf16' in entry
            n, ci, q = R.sample_elements(N, cin, g.levels, g.off_in, g.Pin, seed)
            ref, S, K = R.dgrad(g, dy, w, n, ci, q, bf16=bf16)
            v, bar = R.epilogue(ref, S, res=_gather(add, n, ci, q)
                                if add is not None else None)
            worst = R.check(_gather(dx, n, ci, q), v, S, bar,
                            what=f'{entry} {desc}')
        else:
            bf16 = 'bf16' in entry or (entry == 'ld_conv_wgrad_partial' and
                                       extra[0] >= 1)
            got = w._ld_grad if sink else dw
            co, ci, t = R.sample_weights(g, seed, max_count=96)
            ref, S, K = R.wgrad(g, x, dy, co, ci, t, bf16=bf16)
            b = None
            if sink:
                b = base.reshape(cout, cin, -1)[
                    torch.as_tensor(co, device=dev), torch.as_tensor(ci, device=dev),
                    torch.as_tensor(t, device=dev)].double().cpu().numpy()
            v, bar = R.epilogue(ref, S, res=b)
            worst = R.check(_gather(got.reshape(cout, cin, -1), co, ci, t), v,
                            S, bar, what=f'{entry} {desc} {extra}')
            n = co
        rows.append((entry, int(K.max()), len(n), worst, 0.0))
    if sink:
        del w._ld_grad
    return rows


def _c8_free(key):
    """A bf16 unit whose operands and outputs can all be fp32 (so it can run
    with the C8 path off)."""
    if key[-1] != 'bf16':
        return False
    if key[0] == 'fwd':
        _, _, xk, _, _, resk, _, _, c8_only, _, raw_c8, _ = key
        return xk != 'c8' and resk not in ('c8', 'unwritten') and \
            not c8_only and not raw_c8
    return key[2] != 'c8' and key[3] != 'c8'


def _replay_all(census, kind, c8_off=False):
    dev = _dev()
    from ld_amd import layers as Y
    failures, seen = [], 0
    worst_all = 0.0
    for i, (key, e) in enumerate(sorted(census.units.items(), key=str)):
        if key[0] != kind or not e['sigs']:
            continue
        if c8_off and not (_c8_free(key) and
                           any('_c8' in s[0] for s in e['sigs'])):
            continue
        prec = key[-1]
        Y.set_precision(prec)
        Y.set_c8(not c8_off)
        try:
            run = _replay_fwd if kind == 'fwd' else _replay_bwd
            rows = run(key[:-1], prec, e['sigs'], dev, 1000 + i, c8_off)
            for entry, K, ns, worst, worst8 in rows:
                _line(e['tags'], entry, key[1], K, ns, worst, worst8)
                worst_all = max(worst_all, worst)
            seen += len(rows)
        except AssertionError as err:
            failures.append(f'{sorted(e["tags"])} {key}: {err}')
            print('FAIL', failures[-1])
        finally:
            Y.set_precision('fp32')
            Y.set_c8(True)
    print(f'{kind}{" (C8 path off)" if c8_off else ""}: {seen} signatures '
          f'checked, worst err/(uS) of the fp32 outputs {worst_all:.2f}')
    assert not failures, f'{len(failures)} failures:\n' + '\n'.join(failures)
    assert seen > 0


def test_census_covers_both_precisions(census):
    precs = {k[-1] for k in census.units}
    assert precs == {'fp32', 'bf16'}
    entries = {s[0] for s in census.signatures()}
    # the production entry points, including the C8 and deferred ones
    for e in ('ld_conv_forward', 'ld_conv_forward_smallc', 'ld_conv_bf16_forward_c8',
              'ld_conv_dgrad', 'ld_conv_bf16_dgrad_c8', 'ld_conv_wgrad_partial'):
        assert e in entries, e
    kinds = {k[0] for k in census.other}
    assert {'ld_gconv_forward', 'ld_deform_im2col'} <= kinds, kinds
    # the 7x7 stem at 800x1344
    assert any(s[0] == 'ld_conv_forward_smallc' and s[1][3] == 7 and
               s[1][6][0] == (800, 1344) for s in census.signatures())


def test_replay_forward(census):
    _replay_all(census, 'fwd')


def test_replay_backward(census):
    _replay_all(census, 'bwd')


def test_replay_bf16_without_c8(census):
    """The bf16 units the step ran on C8 operands, replayed with the C8 path
    off (LD_CONV_C8=0): the fp32-activation bf16 kernels and their tune
    records (family 1) at the same production geometries."""
    _replay_all(census, 'fwd', c8_off=True)
    _replay_all(census, 'bwd', c8_off=True)


def test_grouped_conv_per_group(census):
    from ld_amd import layers as Y
    dev = _dev()
    keys = sorted(k for k in census.other if k[0] == 'ld_gconv_forward')
    for i, key in enumerate(keys):
        _, N, cin, cout, groups, k, s, p, h, wd, has_aff, relu = key
        g = R.Geom(N, cin, cout, k, s, p, ((h, wd), ))
        gen = torch.Generator(device=dev).manual_seed(77 + i)
        x = _randn((N, cin, h * wd), gen, dev, absval=i % 2 == 1)
        cg, og = cin // groups, cout // groups
        wg = _randn((cout, cg, k, k), gen, dev) / math.sqrt(cg * k * k)
        scale = torch.rand(cout, generator=gen, device=dev) + 0.5 \
            if has_aff else None
        shift = _randn((cout, ), gen, dev) if has_aff else None
        y, _ = Y.gconv_forward(x, wg, groups, s, p, ((h, wd), ), scale, shift,
                               bool(relu))
        torch.cuda.synchronize()
        # per-group convs as one dense conv with a block-diagonal weight: the
        # zero blocks add exact zeros, S and the bar are those of the group
        dense = torch.zeros((cout, cin, k, k), device=dev)
        for gi in range(groups):
            dense[gi * og:(gi + 1) * og, gi * cg:(gi + 1) * cg] = \
                wg[gi * og:(gi + 1) * og]
        n, co, pp = R.sample_elements(N, cout, g.out_levels, g.off_out, g.Pout,
                                      i)
        ref, S, K = R.forward(g, x, dense, n, co, pp)
        v, bar = R.epilogue(ref, S, _chan(scale, co) if has_aff else None,
                            _chan(shift, co) if has_aff else None, None,
                            bool(relu))
        worst = R.check(_gather(y, n, co, pp), v, S, bar, what=f'gconv {key}')
        print(f'{"+".join(sorted(census.other[key]["tags"])):44s} '
              f'ld_gconv_forward N{N} {cin}>{cout} g{groups} k{k}s{s}p{p} '
              f'[{h}x{wd}] K={cg * k * k} n={len(n)} worst={worst:.2f}')
    assert keys


def _bilinear64(x, off, key, n, c, tap, p):
    """float64 DCNv1 bilinear sample (zero outside (-1, H) x (-1, W), corners
    outside the map 0) of the column element (n, c * k * k + tap, p), with the
    bar 4u sum |w_i x_i| + (coordinate error) * sum |x_i|."""
    _, N, cin, H, W, kh, kw, s, pad, dil = key
    wo = (W + 2 * pad - dil * (kw - 1) - 1) // s + 1
    ho_, wo_ = p // wo, p % wo
    ki, kj = tap // kw, tap % kw
    dev = x.device
    ti = torch.as_tensor
    oh = off[ti(n, device=dev), ti(2 * tap, device=dev), ti(p, device=dev)]
    ow = off[ti(n, device=dev), ti(2 * tap + 1, device=dev), ti(p, device=dev)]
    bh = ho_ * s - pad + ki * dil
    bw = wo_ * s - pad + kj * dil
    hh = bh + oh.double().cpu().numpy()
    ww = bw + ow.double().cpu().numpy()
    inside = (hh > -1) & (ww > -1) & (hh < H) & (ww < W)
    h0, w0 = np.floor(hh).astype(np.int64), np.floor(ww).astype(np.int64)
    lh, lw = hh - h0, ww - w0
    ref = np.zeros(len(n))
    sabs = np.zeros(len(n))
    xabs = np.zeros(len(n))
    xf = x.reshape(N, cin, H * W)
    for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw),
                       (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        r, cc = h0 + dh, w0 + dw
        ok = inside & (r >= 0) & (r < H) & (cc >= 0) & (cc < W)
        idx = np.where(ok, r * W + cc, 0)
        xv = xf[ti(n, device=dev), ti(c, device=dev),
                ti(idx, device=dev)].double().cpu().numpy() * ok
        ref += wt * xv
        sabs += np.abs(wt * xv)
        xabs += np.abs(xv)
    # fp32 h = base + offset, lh = h - floor(h): each weight off by <= ~2 u |h|
    dcoord = 4 * U * (np.abs(hh) + np.abs(ww) + 2)
    return ref, 4 * U * sabs + dcoord * xabs, sabs


def test_deform_im2col_vs_float64_bilinear(census):
    from ld_amd import layers as Y
    dev = _dev()
    keys = sorted(k for k in census.other if k[0] == 'ld_deform_im2col')
    for i, key in enumerate(keys):
        _, N, cin, H, W, kh, kw, s, pad, dil = key
        assert kh == kw and dil == 1
        ho = (H + 2 * pad - dil * (kh - 1) - 1) // s + 1
        wo = (W + 2 * pad - dil * (kw - 1) - 1) // s + 1
        gen = torch.Generator(device=dev).manual_seed(91 + i)
        x = _randn((N, cin, H * W), gen, dev)
        # offsets of a few pixels, with whole-pixel and out-of-map cases
        off = _randn((N, 2 * kh * kw, ho * wo), gen, dev) * 3
        off[:, :, ::7] = off[:, :, ::7].round()
        off[:, :, 5::11] += 2 * H
        col = Y.deform_im2col(x, off, H, W, kh, s, pad, dil)
        torch.cuda.synchronize()
        rng = np.random.default_rng(i)
        P = ho * wo
        pos = np.array(R.sample_positions(((ho, wo), ), (0, ), P, rng))
        m = len(pos)
        n = rng.integers(0, N, m)
        c = np.array([R.sample_channels(cin)[j % len(R.sample_channels(cin))]
                      for j in range(m)])
        tap = np.arange(m) % (kh * kw)
        ref, bar, sabs = _bilinear64(x, off, key, n, c, tap, pos)
        got = _gather(col, n, c * kh * kw + tap, pos)
        worst = R.check(got, ref, sabs, bar, what=f'deform_im2col {key}')
        print(f'{"+".join(sorted(census.other[key]["tags"])):44s} '
              f'ld_deform_im2col N{N} C{cin} [{H}x{W}] k{kh}s{s}p{pad} n={m} '
              f'worst={worst:.2f}')
    assert keys


def test_fused_bottleneck_geometries_are_pinned(census):
    """ld_bottleneck_c8_forward is held bit-exact to its three launches by
    test_gpu_fused_block.py; the census geometries must be among its cases."""
    import test_gpu_fused_block as FB
    keys = sorted(k for k in census.other if k[0] == 'ld_bottleneck_c8_forward')
    for k in keys:
        print('bottleneck', k, sorted(census.other[k]['tags']))
    pinned = set(FB.PRODUCTION_GEOMETRIES)
    missing = [k[1:] for k in keys if k[1:] not in pinned]
    assert not missing, f'fused bottleneck geometries not pinned: {missing}'


def _table_rows():
    from ld_amd import lib as L
    rows = []
    for line in open(L.TUNE_TABLE):
        if line.strip() and not line.startswith('#'):
            rows.append(tuple(int(v) for v in line.split()[:18]))
    return rows


def test_every_tune_record_is_checked(census):
    """Runs after the replays (file order): every record must have been found
    by a launch of the census or of its checked replay."""
    import ctypes as C
    from ld_amd import lib as L
    lib = L.get_lib()
    unreached, stale = [], []
    for key in _table_rows():
        arr = (C.c_int32 * 18)(*key)
        hits = lib.ld_conv_tune_hits(arr)
        assert hits >= 0, key
        if hits == 0 and key not in UNREACHED:
            unreached.append(key)
        if hits > 0 and key in UNREACHED:
            stale.append(key)
    print(f'tune table: {len(_table_rows())} records, '
          f'{len(UNREACHED)} listed as unreached')
    assert not unreached, ('tune records no checked launch looked up:\n' +
                           '\n'.join(' '.join(map(str, k)) for k in unreached))
    assert not stale, f'listed as unreached but looked up: {stale}'
