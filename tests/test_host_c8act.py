"""Host-side logic of the C8-only activation carrier (ld_amd.layers.C8Act,
DESIGN.md section 3.4): pure bookkeeping, runs without a GPU."""
import pytest
import torch

from ld_amd import layers as Y
from ld_amd.lib import LdError


def _c8_image(x):
    """(N, C, P) fp32 -> the bf16 (N, C/8, P, 8) image, flattened: the layout
    ld_conv_to_c8 writes (tests/test_gpu_bf16.py::test_to_c8_layout)."""
    n, c, p = x.shape
    return x.to(torch.bfloat16).reshape(n, c // 8, 8, p).permute(
        0, 1, 3, 2).reshape(-1).contiguous()


def test_c8act_views_share_the_buffer_and_round_trip():
    x = torch.randn(2, 32, 6 * 5)
    a = Y.C8Act(_c8_image(x), x.shape)
    assert a.shape == (2, 32, 30) and a.dim() == 3 and a.size(1) == 32
    assert not a.requires_grad and a.dtype == torch.float32
    v = a.view(2, 32, 6, 5)
    assert v.buf is a.buf and v.shape == (2, 32, 6, 5)
    assert v.reshape(2, 32, -1).shape == (2, 32, 30)
    assert v.reshape((2, 32, 30)).shape == (2, 32, 30)
    want = x.to(torch.bfloat16).float()
    assert torch.equal(a.float(), want)
    assert torch.equal(v.float(), want.reshape(2, 32, 6, 5))


def test_c8act_refuses_views_that_touch_batch_or_channels():
    a = Y.C8Act(torch.zeros(2 * 32 * 30, dtype=torch.bfloat16), (2, 32, 30))
    for bad in ((2, 16, 60), (1, 64, 30), (4, 32, 15), (2, 32, 31), (2, 960)):
        with pytest.raises(LdError):
            a.reshape(*bad)


def test_c8_only_is_a_bf16_mode_feature():
    """The C8-only teacher trunk needs bf16 mode, the C8 path and channel counts
    that are multiples of 32; LD_TEACHER_C8_ONLY=0 switches it off."""
    prev = Y._PRECISION[0]
    try:
        Y._PRECISION[0] = 'fp32'
        assert not Y.c8_only_available([64, 256])
        Y._PRECISION[0] = 'bf16'
        assert Y.c8_only_available([64, 256, 2048])
        assert not Y.c8_only_available([64, 80])
        Y.set_c8(False)
        assert not Y.c8_only_available([64])
        Y.set_c8(True)
    finally:
        Y._PRECISION[0] = prev
        Y.set_c8(True)


def test_c8_only_scope_nests_and_restores():
    assert not Y._C8_ONLY[0]
    with Y.c8_only_scope():
        assert Y._C8_ONLY[0]
        with Y.c8_only_scope():
            assert Y._C8_ONLY[0]
        assert Y._C8_ONLY[0]
    assert not Y._C8_ONLY[0]


def test_resnet_keeps_fp32_activations_outside_the_conditions():
    """ResNet._c8_only: only with the flag, under no_grad, in eval mode, in
    bf16 mode (no GPU needed to evaluate the predicate)."""
    from ld_amd import build_backbone
    bb = build_backbone(dict(
        type='ResNet', depth=18, num_stages=4, out_indices=(0, 1, 2, 3),
        frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=True),
        norm_eval=True, style='pytorch'))
    assert bb.train() is bb and bb.eval() is bb
    prev = Y._PRECISION[0]
    try:
        Y._PRECISION[0] = 'bf16'
        with torch.no_grad():
            assert not bb._c8_only()          # flag not set
            bb.c8_activations = True
            assert bb._c8_only()
            bb.train()
            assert not bb._c8_only()          # training mode
            bb.eval()
        assert not bb._c8_only()              # gradients enabled
        Y._PRECISION[0] = 'fp32'
        with torch.no_grad():
            assert not bb._c8_only()          # fp32 mode
    finally:
        Y._PRECISION[0] = prev


def test_retina_pseudo_image_views_share_memory():
    """RetinaGFLHead._pseudo: an (N, B * C, H, W) level map -- a strided slice
    of the level-concatenated (N, B * C, P) head output -- viewed as (N * B, C,
    H, W) WITHOUT a copy; gradients written through the view land in the
    original layout (what the fused loss block relies on)."""
    from ld_amd import model_zoo
    from ld_amd.registry import build_head
    head = build_head(dict(model_zoo.retina_gfl_detector(50)['bbox_head']))
    assert head.num_anchors == 9
    N, P = 2, 6 * 5 + 3 * 3
    full = torch.arange(N * 720 * P, dtype=torch.float32).reshape(N, 720, P)
    lv0 = full[:, :, :30].view(N, 720, 6, 5)      # non-contiguous level slice
    lv1 = full[:, :, 30:].view(N, 720, 3, 3)
    p0, p1 = head._pseudo([lv0, lv1], 80)
    assert p0.shape == (N * 9, 80, 6, 5) and p1.shape == (N * 9, 80, 3, 3)
    assert p0.data_ptr() == lv0.data_ptr() and p1.data_ptr() == lv1.data_ptr()
    # pseudo-image n * 9 + b, class c  ==  image n, channel b * 80 + c
    for n, b, c in ((0, 0, 0), (1, 4, 17), (1, 8, 79)):
        assert torch.equal(p0[n * 9 + b, c], lv0[n, b * 80 + c])
        assert torch.equal(p1[n * 9 + b, c], lv1[n, b * 80 + c])
    assert p0.stride() == (80 * P, P, 5, 1)
    # a contiguous gradient in the pseudo layout IS the (N, 720, H, W) gradient
    g = torch.randn(N * 9, 80, 6, 5)
    assert torch.equal(g.view(N, 720, 6, 5)[1, 4 * 80 + 17], g[1 * 9 + 4, 17])


def test_student_frozen_stages_run_c8_only_decision():
    """bf16 mode: a training student's frozen leading stages (frozen_stages = 1)
    run C8-only like the teacher's trunk; never in fp32 mode, under no_grad
    (inference keeps fp32 masters), or for the teacher-flagged backbone (its
    whole trunk already is)."""
    import torch
    from ld_amd import layers as Y
    from ld_amd import model_zoo
    from ld_amd.registry import build_backbone
    net = build_backbone(model_zoo._backbone(50)).train()
    assert net._frozen_c8_stages() == 0  # fp32 mode
    Y.set_precision('bf16')
    try:
        assert net._frozen_c8_stages() == 1
        with torch.no_grad():
            assert net._frozen_c8_stages() == 0
        net.c8_activations = True
        assert net._frozen_c8_stages() == 0
        net.c8_activations = False
        r18 = build_backbone(model_zoo._backbone(18)).train()
        # 64-channel BasicBlock stages: multiples of 32 -> eligible as well
        assert r18._frozen_c8_stages() == 1
        unfrozen = build_backbone(dict(model_zoo._backbone(50),
                                       frozen_stages=-1)).train()
        assert unfrozen._frozen_c8_stages() == 0
    finally:
        Y.set_precision('fp32')


# ---------------------------------------------------------------------------
# activation forms (ld_amd.layers, "activation forms" section):
# the image-only check precedes the device check, so CPU tensors suffice and no
# library call is reached
# ---------------------------------------------------------------------------
_LV = ((3, 4), )


def _placeholder():
    like = torch.zeros(2, 32, 12)
    return Y._image_only_output(like.shape,
                                torch.zeros(like.numel(), dtype=torch.bfloat16))


def _no_grad(fn):
    def run(*a):
        with torch.no_grad():
            return fn(*a)
    return run


def _bn(p, grad):
    one = torch.ones(32, requires_grad=grad)
    return Y.bn_act(p, one, one, one, one, 1e-5)


def _gn(p, grad):
    one = torch.ones(32, requires_grad=grad)
    return Y.gn_act(p, one, one, 4, 1e-5, _LV)


def _conv_fp32(p):
    assert Y.get_precision() == 'fp32'
    return Y.conv2d(p, torch.zeros(32, 32, 3, 3), None, 1, 1, _LV)


def _conv_backward_fp32(p):
    w = torch.zeros(32, 32, 3, 3)
    return Y._conv_backward(p, None, w, torch.zeros(2, 32, 12), (1, 1, _LV, False),
                            (w, None), False, True, False)


def _dcn_module(p):
    from ld_amd.cnn import DeformConv2dPack
    return DeformConv2dPack(32, 32, 3, padding=1).forward3_bn(p, _LV)


def _lost_image(p):
    Y._attach_c8(p, None)
    return Y.to_c8(p)


def _part():
    return torch.zeros(2, 8, 12)


READERS = [  # (the consumer's name in the message, a call that reads fp32 values)
    ('bn input', lambda p: _bn(p, True)),
    ('bn input', _no_grad(lambda p: _bn(p, False))),
    ('bn input', Y.relu),
    ('gn input', lambda p: _gn(p, True)),
    ('gn input', _no_grad(lambda p: _gn(p, False))),
    ('upsample_add fine map', lambda p: Y.upsample_add(p.view(2, 32, 3, 4),
                                                   torch.zeros(2, 32, 2, 2))),
    ('scale_levels input', lambda p: Y.scale_levels(p, torch.ones(1), _LV)),
    ('maxpool input', lambda p: Y.maxpool3x3s2(p.view(2, 32, 3, 4))),
    ('copy_into source', lambda p: Y.copy_into(torch.zeros(2, 32, 12), p)),
    ('level map', lambda p: Y._pack_launch([p.view(2, 32, 3, 4)], _LV)),
    # pack_levels: the single-level reshape, the non-contiguous torch.cat and the
    # PackLevelsFn / _pack_launch branch
    ('pack_levels input', lambda p: Y.pack_levels([p.view(2, 32, 3, 4)])),
    ('pack_levels input', lambda p: Y.pack_levels(
        [torch.zeros(2, 32, 3, 4), p.view(2, 32, 3, 4)[..., :2]])),
    ('pack_levels input', lambda p: Y.pack_levels(
        [torch.zeros(2, 32, 3, 4, requires_grad=True), p.view(2, 32, 3, 4)])),
    ('avgpool input', lambda p: Y.avgpool_ceil(p, (3, 4), 2)),
    ('res2 gather input', lambda p: Y._res2_gather(p, 0, 8, None)),
    ('res2 concat tail', lambda p: Y._res2_concat(
        (_part(), _part(), _part()), p, 8, (3, 4), 1, Y.RES2_TAIL_COPY)),
    ('dcn input', lambda p: Y.deform_im2col_fn(
        p, torch.zeros(2, 18, 12, requires_grad=True), 3, 4, 3, 1, 1)),
    ('dcn input', _no_grad(lambda p: Y.deform_im2col_fn(
        p, torch.zeros(2, 18, 12), 3, 4, 3, 1, 1))),
    ('trainable grouped conv input', lambda p: Y.gconv2d(
        p, torch.zeros(32, 1, 3, 3, requires_grad=True), 32, 1, 1, _LV)),
    ('grouped conv input', _no_grad(lambda p: Y.gconv2d(
        p, torch.zeros(32, 1, 3, 3), 32, 1, 1, _LV))),
    ('trainable DCN input', _dcn_module),
    ('conv input', _conv_fp32),
    ('conv backward: saved input', _conv_backward_fp32),
    ('to_c8', _lost_image),
]


@pytest.mark.parametrize('name,read', READERS,
                         ids=[f'{i}-{n[0]}' for i, n in enumerate(READERS)])
def test_every_fp32_reader_refuses_an_image_only_activation(name, read):
    with pytest.raises(LdError, match='only as a C8 image') as e:
        read(_placeholder())
    assert str(e.value).startswith(name + ':')
    # a C8Act is refused by the same guard, under the same name
    with pytest.raises(LdError, match='only as a C8 image'):
        Y._dev_f32(Y.C8Act(torch.zeros(768, dtype=torch.bfloat16), (2, 32, 12)),
                   name)


def test_views_of_a_placeholder_stay_flagged():
    p = _placeholder()
    v = p.view(2, 32, 3, 4)
    assert Y._unwritten(p) and Y._unwritten(v)
    assert Y._unwritten(v.reshape(2, 32, 12))
    levels = ((2, 4), (2, 2))
    assert all(Y._unwritten(t) for t in Y.split_levels(p, levels))
    plain = torch.zeros(2, 32, 12)
    cached = torch.zeros(2, 32, 12)
    Y._attach_c8(cached, torch.zeros(768, dtype=torch.bfloat16))
    for t in (plain, cached, plain.view(2, 32, 3, 4)):
        assert not Y._unwritten(t)
        assert Y._fp32_readable(t, 'reader') is t
        # past the image-only check: what refuses a CPU tensor is the device check
        with pytest.raises(LdError, match='only run on a HIP device'):
            Y._dev_f32(t, 'reader')
    assert Y._dev_f32(p, 'conv input', image_ok=True) is p


def test_cached_image_follows_the_tensor_and_its_version():
    x = torch.zeros(2, 32, 12)
    img = torch.zeros(768, dtype=torch.bfloat16)
    assert Y._c8_cached(x) is None
    Y._attach_c8(x, img)
    assert Y._c8_cached(x) is img
    assert Y._c8_operand(x) is img  # no conversion launch
    # a same-memory contiguous reshape view finds the image through its base
    assert Y._c8_cached(x.view(2, 32, 3, 4)) is img
    assert Y._c8_cached(x.view(2, 32, 3, 4).reshape(2, 32, 12)) is img
    assert Y._c8_cached(x[:, :, :6]) is None and Y._c8_cached(x[1:]) is None
    x.add_(1.0)  # an in-place write bumps the version: the image is stale
    assert Y._c8_cached(x) is None
    a = Y.C8Act(img, (2, 32, 12))
    assert Y._c8_operand(a) is img
    p = _placeholder()
    assert Y._c8_operand(p) is Y._c8_cached(p)
    Y._attach_c8(p, None)
    assert Y._c8_cached(p) is None and Y._unwritten(p)


@pytest.mark.parametrize('c8_on', [True, False])
@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_c8_writable_matches_the_five_spellings_it_replaced(mode, c8_on):
    prev = Y._PRECISION[0]
    try:
        Y._PRECISION[0] = mode
        Y.set_c8(c8_on)
        _C8, _PRECISION = Y._C8, Y._PRECISION
        for c in (16, 32, 48, 64):
            for P in (6, 8):
                for ptrs in ((4096, 8192, 512), (4096, 8196, 512), (4100, ) * 3):
                    p0 = ptrs[0]
                    side_output = bool(
                        _C8[0] and _PRECISION[0] == 'bf16' and c % 32 == 0 and
                        P % 4 == 0 and p0 % 16 == 0)
                    gn_forward = bool(
                        _C8[0] and _PRECISION[0] == 'bf16' and c % 32 == 0 and
                        P % 4 == 0 and p0 % 16 == 0)
                    aligned = all(p % 16 == 0 for p in ptrs)
                    gn_backward = bool(
                        aligned and _C8[0] and _PRECISION[0] == 'bf16' and
                        c % 32 == 0 and P % 4 == 0)
                    bn_backward = bool(
                        all(p % 16 == 0 for p in ptrs) and
                        _C8[0] and _PRECISION[0] == 'bf16' and c % 32 == 0 and
                        P % 4 == 0)
                    pack = bool(_C8[0] and _PRECISION[0] == 'bf16' and c % 32 == 0)
                    assert bool(Y._c8_writable(c, P, ptrs=(p0, ))) == side_output
                    assert bool(Y._c8_writable(c, P, ptrs=(p0, ))) == gn_forward
                    assert bool(Y._c8_writable(c, P, ptrs=ptrs)) == gn_backward
                    assert bool(Y._c8_writable(c, P, ptrs=list(ptrs))) == bn_backward
                    assert bool(Y._c8_writable(c, P, vec=1)) == pack
    finally:
        Y._PRECISION[0] = prev
        Y.set_c8(True)


def test_only_the_forms_section_touches_the_tensor_attributes():
    """Structural pin: the image / placeholder attributes are read and written
    between the two "activation forms" markers of layers.py and nowhere else."""
    import os
    root = os.path.dirname(os.path.abspath(Y.__file__))
    src = open(os.path.join(root, 'layers.py')).read()
    begin, end = '# activation forms: begin', '# activation forms: end'
    assert src.count(begin) == 1 and src.count(end) == 1
    inside = src[src.index(begin):src.index(end)]
    outside = src[:src.index(begin)] + src[src.index(end):]
    for attr in ('_ld_c8', '_ld_unwritten'):
        assert attr in inside
        assert attr not in outside
        for other in ('cnn.py', 'resnet.py'):
            assert attr not in open(os.path.join(root, other)).read(), other
